"""fp64 reference, error bounds and shared scenarios for the optimizer's extensions -- AdamW, the EMA shadow and the
non-finite guard (tests/test_optim_ext.py on the torch-op path, tests/test_optim_ext_gpu.py on the device).  The style and
the house rule are tests/_optim_ref.py's: every quantity is referenced in fp64 from the fp32 values it is computed FROM, and
with u = 2^-24 and S the sum of the absolute values of its terms the accepted error is 8 u S.

adamw_stage.  m and v are Adam's with g' = coef g (no L2 term): m = b1 m + (1 - b1) g' has the roundings of b1, 1 - b1, coef,
three products and one sum, v one more product: at most 8, each relative to a partial result no larger than S -> 8 u S, as
in adam_stage.  The parameter is p1 - upd with p1 = f p, f = 1 - lr wd formed in double and rounded once, and
upd = (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps) from the STORED m and v.  Adam's form is u |p_ref| (the subtraction's
rounding) + 16 u |upd| (the roundings of step_size, sqrt(bc2), eps, a square root, two divisions, a sum and a product: 8,
doubled because sqrt(v) / sqrt(bc2) + eps sits in a denominator).  The decay product adds two roundings relative to |p1|:
that of f and that of f p.  Bound: u |p_ref| + 2 u |p1| + 16 u |upd|.

ema_stage.  e = d e + (1 - d) p_out from the STORED p_out: the roundings of d and 1 - d, two products, one sum: 5 <= 8, each
relative to a partial result no larger than S = d |e| + (1 - d) |p_out| -> 8 u S.

torch.optim.AdamW orders its operations differently (m by lerp, the denominator as sqrt(v) / sqrt(bc2) + eps, addcdiv):
tests/test_optim_ext.py::test_adamw_against_torch_optim holds torch's own result to these bounds and the two results to the
sum of them, on the CPU.
"""
import math

import numpy as np
import torch

import _optim_ref as ref
from _optim_ref import U, f64


def adamw_stage(p, g, m, v, p_out, m_out, v_out, lr, wd, betas, eps, t, coef=1.0):
    """{name: (reference, bound)} of AdamW's step number t (1-based) on one tensor; m / v None: zeros."""
    p, g, m_out, v_out = f64(p), f64(g), f64(m_out), f64(v_out)
    m = np.zeros_like(p) if m is None else f64(m)
    v = np.zeros_like(p) if v is None else f64(v)
    b1, b2 = betas
    gp = coef * g
    s_gp = np.abs(gp)
    m_ref = b1 * m + (1 - b1) * gp
    s_m = b1 * np.abs(m) + (1 - b1) * s_gp
    v_ref = b2 * v + (1 - b2) * gp * gp
    s_v = b2 * np.abs(v) + (1 - b2) * s_gp * s_gp
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    p1 = (1 - lr * wd) * p
    upd = lr * (m_out / bc1) / (np.sqrt(v_out / bc2) + eps)
    p_ref = p1 - upd
    return {"exp_avg": (m_ref, 8 * U * s_m), "exp_avg_sq": (v_ref, 8 * U * s_v),
            "p": (p_ref, U * np.abs(p_ref) + 2 * U * np.abs(p1) + 16 * U * np.abs(upd))}


def ema_stage(e, p_out, decay):
    """(reference, bound) of the shadow after a step that stored p_out; e: the shadow before it."""
    e, p_out = f64(e), f64(p_out)
    return decay * e + (1 - decay) * p_out, 8 * U * (decay * np.abs(e) + (1 - decay) * np.abs(p_out))


class Recorder(ref.Recorder):
    """_optim_ref.Recorder with kind "adamw" and, where the optimizer keeps one, the EMA shadow as one more stored quantity
    (its decay is read from the optimizer at check time)."""

    def before(self, params):
        snap = super().before(params)
        for p, b in zip(params, snap):
            e = self.opt.state.get(p, {}).get("ema")
            b["ema"] = b["p"].copy() if e is None else f64(e)          # (created as a clone of p by its first step)
            if p in getattr(self.opt, "_uninit", ()):                   # a momentum buffer allocated but never written
                b["momentum_buffer"] = None
        return snap

    def stages(self, p, b, coef=1.0):
        st = self.opt.state.get(p, {})
        if self.kind == "adamw" and b["g"] is not None:
            group = self._group(p)
            lr, wd = ref.effective(group)
            out = adamw_stage(b["p"], b["g"], b["exp_avg"], b["exp_avg_sq"], p, st["exp_avg"], st["exp_avg_sq"], lr, wd,
                              tuple(float(x) for x in group["betas"]), float(group["eps"]), b["t"] + 1, coef)
        else:
            out = super().stages(p, b, coef)
        if b["g"] is not None and st.get("ema") is not None:
            out["ema"] = ema_stage(b["ema"], p, float(self.opt.ema_decay))
        return out


# ---- the guard's scenario, the same on both paths ---------------------------------------------------------------------
def bits(t):
    """A detached clone whose comparison with torch.equal is a comparison of bits (NaN payloads, signed zeros)."""
    return t.detach().clone().view(torch.int32)


def snapshot(opt, params):
    """The bits of every parameter and of every state tensor on its device (the host-side `step` counters excluded)."""
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append({"p": bits(p), **{k: bits(v) for k, v in st.items() if k != "step"}})
    return out


def unchanged(opt, params, snap):
    for p, s in zip(params, snap):
        st = opt.state.get(p, {})
        if not torch.equal(p.detach().view(torch.int32), s["p"]):
            return False
        if any(k not in st or not torch.equal(st[k].view(torch.int32), s[k]) for k in s if k != "p"):
            return False
        for k in set(st) - {"step"} - set(s):        # state the step created: a shadow equal to p, an unwritten momentum
            new = st[k].view(torch.int32)            # buffer, Adam's zeros
            if not (torch.equal(new, s["p"]) if k == "ema" else p in getattr(opt, "_uninit", ()) or not bool(new.any())):
                return False
    return True


def guard_case(opt, rec, params, fresh_grads, case, poison=(3, 5), first=False):
    """One ordinary step (unless `first`), one step fed `case` -- "nan" / "inf": one element of the tensors `poison`;
    "huge": every gradient times 1e25 -- and one ordinary step, each ordinary step held to its fp64 stage.  A poisoned step
    must leave every bit of p, the states and the shadows, count one skip, report a non-finite norm, name exactly the
    poisoned tensors and zero the gradients when the optimizer does that; "huge" must not be skipped.  fresh_grads(scale)
    installs new gradients.  Returns the recorder's worst ratios."""
    clip = opt.max_grad_norm

    def ordinary(nonfinite=False):
        fresh_grads(1.0)
        snap = rec.before(params)
        norm = ref.global_norm([p.grad for p in params if p.grad is not None])
        opt.step()
        rec.check(params, snap, coef=ref.clip_coef(norm, clip), nonfinite=nonfinite)
        assert abs(float(opt.last_grad_norm) - norm) <= 1e-6 * norm

    if not first:
        ordinary()
    fresh_grads(1e25 if case == "huge" else 1.0)
    with torch.no_grad():
        if case != "huge":
            for i in poison:
                params[i].grad[params[i].numel() // 2] = math.nan if case == "nan" else math.inf
    snap, before = rec.before(params), snapshot(opt, params)
    norm = ref.global_norm([p.grad for p in params if p.grad is not None])
    opt.step()
    got = float(opt.last_grad_norm)
    if case == "huge":
        assert opt.skipped_steps == 0 and 1e26 < got < math.inf and abs(got - norm) <= 1e-6 * norm
        assert opt.nonfinite_parameters() == []
        assert all(bool(torch.isfinite(p).all()) for p in params) and not unchanged(opt, params, before)
        if clip is not None:                 # (unclipped, Adam's fp32 g'^2 overflows where the fp64 reference's does not)
            rec.check(params, snap, coef=ref.clip_coef(norm, clip))
    else:
        assert unchanged(opt, params, before), "a skipped step wrote a parameter, a state or a shadow"
        assert opt.skipped_steps == 1 and int(opt.skipped) == 1 and opt.skipped.dtype == torch.int64
        assert not math.isfinite(got) and (got != got) == (case == "nan")
        named = opt.nonfinite_parameters()
        assert len(named) == len(poison) and {id(a) for a in named} == {id(params[i]) for i in poison}
        zeroed = all(not bool(p.grad.view(torch.int32).any()) for p in params if p.grad is not None)
        assert zeroed == opt.zero_grads
    # (unclipped "huge" leaves Adam's fp32 v at +inf, as it leaves torch's: there the stored and the reference's infinities
    # must coincide and every finite position keeps its bound)
    ordinary(nonfinite=case == "huge" and clip is None)
    assert opt.skipped_steps == (0 if case == "huge" else 1)
    return rec.worst
