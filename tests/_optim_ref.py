"""fp64 reference and error bounds for the optimizer tests (tests/test_optim.py, tests/test_optim_gpu.py and the lifecycle
timelines of tests/_optim_timeline.py).

The reference is the update rule evaluated in fp64 (numpy) from the same fp32 inputs.  With u = 2^-24 the unit roundoff and
S the sum of the absolute values of the terms of an updated quantity, the accepted error is 8 u S elementwise: the rule has
at most five roundings per output (a few more with the hyper-parameters' own rounding to fp32), each relative to a partial
result no larger than S.  Adam's m and v are held to 8 u S, its parameter to u |p| + 16 u |lr m^ / (sqrt(v^) + eps)|.

Every quantity is referenced from the fp32 values it is computed FROM: buf / m / v from the step's inputs, the parameter
from the inputs and the buf / m / v the implementation stored (the fp32 values its update really read).  That is what the
bounds above are written for -- S of the parameter counts |lr buf| and Adam's bound is relative to the update term; neither
has room for the error of buf / m / v, which is bounded by ITS S and can exceed any multiple of u |buf| under cancellation
-- and it loses nothing: the stored buf / m / v are checked against their own bound in the same call.
"""
import math

import numpy as np

U = 2.0 ** -24


def f64(t):
    """A torch tensor (any device) or array as a flat fp64 numpy copy; None stays None."""
    if t is None:
        return None
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.array(t, dtype=np.float64).reshape(-1)


def effective(group):
    """(lr, weight decay) a group trains with: the policy keys of get_optim_policy() applied."""
    return float(group["lr"]) * float(group.get("lr_mult", 1)), float(group["weight_decay"]) * float(group.get("decay_mult", 1))


def global_norm(grads):
    return math.sqrt(sum(float((f64(g) ** 2).sum()) for g in grads))


def clip_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient; 1 without clipping.  A NaN norm gives a NaN coefficient, as there (and
    as the kernel and the torch-op path do): Python's min(1.0, nan) would be 1.0."""
    if max_norm is None:
        return 1.0
    c = max_norm / (norm + 1e-6)
    return c if c != c else min(1.0, c)


def sgd_stage(p, g, buf, p_out, buf_out, lr, wd, momentum, dampening, nesterov, coef=1.0):
    """{name: (reference, bound)} of one SGD step on one tensor.  p, g, buf: the fp32 inputs (buf None: first step);
    p_out / buf_out: what the implementation stored."""
    p, g, buf, buf_out = f64(p), f64(g), f64(buf), f64(buf_out)
    gp = coef * g + wd * p
    s_gp = np.abs(coef * g) + wd * np.abs(p)
    if momentum == 0:
        return {"p": (p - lr * gp, 8 * U * (np.abs(p) + lr * s_gp))}
    if buf is None:
        buf_ref, s_buf = gp, s_gp
    else:
        buf_ref = momentum * buf + (1 - dampening) * gp
        s_buf = momentum * np.abs(buf) + (1 - dampening) * s_gp
    if nesterov:
        p_ref = p - lr * (gp + momentum * buf_out)
        s_p = np.abs(p) + lr * (s_gp + momentum * np.abs(buf_out))
    else:
        p_ref = p - lr * buf_out
        s_p = np.abs(p) + np.abs(lr * buf_out)
    return {"momentum_buffer": (buf_ref, 8 * U * s_buf), "p": (p_ref, 8 * U * s_p)}


def adam_stage(p, g, m, v, p_out, m_out, v_out, lr, wd, betas, eps, t, coef=1.0):
    """{name: (reference, bound)} of Adam's step number t (1-based) on one tensor; m / v None: zeros."""
    p, g, m_out, v_out = f64(p), f64(g), f64(m_out), f64(v_out)
    m = np.zeros_like(p) if m is None else f64(m)
    v = np.zeros_like(p) if v is None else f64(v)
    b1, b2 = betas
    gp = coef * g + wd * p
    s_gp = np.abs(coef * g) + wd * np.abs(p)
    m_ref = b1 * m + (1 - b1) * gp
    s_m = b1 * np.abs(m) + (1 - b1) * s_gp
    v_ref = b2 * v + (1 - b2) * gp * gp
    s_v = b2 * np.abs(v) + (1 - b2) * s_gp * s_gp
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    upd = lr * (m_out / bc1) / (np.sqrt(v_out / bc2) + eps)
    p_ref = p - upd
    return {"exp_avg": (m_ref, 8 * U * s_m), "exp_avg_sq": (v_ref, 8 * U * s_v),
            "p": (p_ref, U * np.abs(p_ref) + 16 * U * np.abs(upd))}


def ratio(out, ref, bound):
    """Worst |out - ref| / bound; where the bound is 0 the value must be exact."""
    err = np.abs(f64(out) - ref)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def ratio_nonfinite(out, ref, bound):
    """ratio() for steps fed non-finite gradients.  Wherever the output or the reference is not finite the two must agree
    exactly -- NaN with NaN, an infinity with the infinity of the same sign -- or the ratio is inf; every other position goes
    through ratio() with its bound, which must be finite there.  With finite data throughout this is ratio()."""
    out = f64(out)
    if out.size == 0:
        return 0.0
    bound = np.broadcast_to(bound, out.shape)
    nf = ~(np.isfinite(out) & np.isfinite(ref))
    with np.errstate(invalid="ignore"):
        same = (np.isnan(out) & np.isnan(ref)) | (np.isinf(out) & (out == ref))
    fin = ~nf
    if (nf & ~same).any() or not np.isfinite(bound[fin]).all():
        return float("inf")
    return ratio(out[fin], ref[fin], bound[fin])


class Recorder:
    """Snapshots the fp32 inputs of an optimizer step and checks what the step stored against the staged reference.
    kind: "sgd" | "adam"; the hyper-parameters are read from the optimizer's groups at check time (lr may change)."""

    def __init__(self, kind, opt):
        self.kind, self.opt = kind, opt
        self.worst = {}

    def _group(self, p):
        for group in self.opt.param_groups:
            if any(q is p for q in group["params"]):
                return group
        raise KeyError("parameter not in the optimizer")

    def before(self, params):
        snap = []
        for p in params:
            st = self.opt.state.get(p, {})
            snap.append({"p": f64(p), "g": f64(p.grad), "momentum_buffer": f64(st.get("momentum_buffer")),
                         "exp_avg": f64(st.get("exp_avg")), "exp_avg_sq": f64(st.get("exp_avg_sq")),
                         "t": int(float(st["step"])) if "step" in st else 0})
        return snap

    def stages(self, p, b, coef=1.0):
        """The {name: (ref, bound)} of the step that took snapshot `b` of parameter p to its present state."""
        group = self._group(p)
        lr, wd = effective(group)
        st = self.opt.state.get(p, {})
        if b["g"] is None:                       # no gradient: untouched, exactly
            return {"p": (b["p"], np.zeros_like(b["p"]))}
        if self.kind == "sgd":
            return sgd_stage(b["p"], b["g"], b["momentum_buffer"], p, st.get("momentum_buffer"), lr, wd,
                             float(group["momentum"]), float(group["dampening"]), bool(group["nesterov"]), coef)
        return adam_stage(b["p"], b["g"], b["exp_avg"], b["exp_avg_sq"], p, st["exp_avg"], st["exp_avg_sq"], lr, wd,
                          tuple(float(x) for x in group["betas"]), float(group["eps"]), b["t"] + 1, coef)

    def check(self, params, snap, coef=1.0, scale=1.0, nonfinite=False):
        """Asserts every stored quantity within `scale` x its bound; keeps the worst ratio per quantity.  nonfinite: the
        step was fed NaN / inf on purpose -- those positions must match the reference's exactly (ratio_nonfinite)."""
        for p, b in zip(params, snap):
            st = self.opt.state.get(p, {})
            for name, (ref, bound) in self.stages(p, b, coef).items():
                out = p if name == "p" else st[name]
                r = (ratio_nonfinite if nonfinite else ratio)(out, ref, bound)
                self.worst[name] = max(self.worst.get(name, 0.0), r)
                assert r <= scale, "%s of a tensor of %d elements: error %.3g x its bound" % (name, b["p"].size, r)
        return self.worst


def compare(rec_a, params_a, snap_a, rec_b, params_b, snap_b, coef_a=1.0, coef_b=1.0, nonfinite=False):
    """Two implementations of one rule stepped from the same fp32 inputs: each stored quantity of A within
    bound_A + bound_B + |ref_A - ref_B| of B's -- twice the bound for buf / m / v, whose reference depends on the inputs alone,
    and for the parameter the same plus the distance of the two staged references (each parameter is held to the reference
    formed from its own buf / m / v).  nonfinite: as in Recorder.check, B's values standing for the reference.  Returns the
    worst ratio."""
    worst = 0.0
    for pa, ba, pb, bb in zip(params_a, snap_a, params_b, snap_b):
        sa, sb = rec_a.stages(pa, ba, coef_a), rec_b.stages(pb, bb, coef_b)
        assert set(sa) == set(sb)
        for name in sa:
            oa = pa if name == "p" else rec_a.opt.state[pa][name]
            ob = pb if name == "p" else rec_b.opt.state[pb][name]
            tol = sa[name][1] + sb[name][1] + np.abs(sa[name][0] - sb[name][0])
            r = (ratio_nonfinite if nonfinite else ratio)(oa, f64(ob), tol)
            worst = max(worst, r)
            assert r <= 1.0, "%s: the two implementations differ by %.3g x the allowed distance" % (name, r)
    return worst
