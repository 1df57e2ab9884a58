"""Scripted timelines for RubiksSGD / RubiksAdam: what the optimizer's host side does BETWEEN steps -- the cached job table,
SGD's first-step flags, Adam's shared step counters, the hand-over between the one-launch path and the torch-op path.

A timeline is a function of (kind, device): it builds a Run over a small parameter set, changes something between steps (a
gradient appears, vanishes or moves; a hyper-parameter changes; state is loaded; a group is added) and calls
Run.step(path), declaring which path that step must take on the device -- "native" (the HIP launch) or "torch" (the same
rule in torch ops).  The declarations follow the rules written down in rubiksnet_amd/optim.py, not what the code does.  On
CPU tensors every step is on the torch path, and the declaration is read as "torch".

Run.step checks, every time:
  * every stored quantity against the fp64 rule evaluated from that step's fp32 inputs, within the bounds of
    tests/_optim_ref.py at scale 1 (Recorder.before / Recorder.check), with the clipping coefficient of the fp64 norm;
  * the increments of opt.native_steps / opt.torch_steps against the declared path;
  * a tensor without a gradient, and a momentum buffer of a group whose momentum is 0: bit-identical, state included;
  * Adam's state[p]["step"] against a count the harness keeps itself (the Recorder reads t from the optimizer's state: a
    wrong counter would otherwise move the reference with it), and that it stays a host tensor;
  * the gradients afterwards: zero with zero_grads, untouched without;
  * last_grad_norm within 1e-6 relative of the fp64 norm when clipping is on;
  * the guard elements around every misaligned tensor;
  * where a torch.optim twin exists: the twin, fed the same fp32 values before every step, within ref.compare.

The parameter set is test_optim_gpu's: its NUMELS, a parameter and a gradient 4 bytes into guarded buffers, a parameter that
never gets a gradient; and one more tensor of CHUNK + 1 elements, so that two parameters can exchange gradients.
tests/test_optim_lifecycle.py runs every timeline on the CPU, tests/test_optim_lifecycle_gpu.py on the device.
"""
import copy
import math

import numpy as np
import torch

import _optim_ref as ref
from rubiksnet_amd import optim

CHUNK = 4096
NUMELS = [0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]        # test_optim_gpu.NUMELS
GUARD = 12345.0
MIS_P, MIS_G, NO_G, PAIR = len(NUMELS), len(NUMELS) + 1, len(NUMELS) + 2, len(NUMELS) + 3
SGD_GROUP_CASES = [dict(momentum=0.9, dampening=0.0, nesterov=True), dict(momentum=0.0), dict(momentum=0.8, dampening=0.3)]
POLICY = [{"lr": 0.05, "weight_decay": 1e-2, "lr_mult": 0.1, "decay_mult": 0.0}, {"lr_mult": 3.0, "decay_mult": 2.0},
          {"lr": 0.02, "weight_decay": 1e-3}]
PLAIN = [{"lr": 0.05, "weight_decay": 1e-2}, {}, {"lr": 0.02, "weight_decay": 1e-3}]       # lr_mult = decay_mult = 1


def default_groups(kind, n_params=PAIR + 1, hypers=POLICY):
    """Three groups, every third tensor each; for SGD one with nesterov, one without momentum (no buffer), one with dampening."""
    groups = [dict(h, idx=list(range(i, n_params, 3))) for i, h in enumerate(hypers)]
    if kind == "sgd":
        for g, case in zip(groups, SGD_GROUP_CASES):
            g.update(case)
    return groups


def own_group(kind, idx):
    """The default groups with the tensors `idx` taken out into a fourth group of their own."""
    groups = default_groups(kind)
    for g in groups:
        g["idx"] = [i for i in g["idx"] if i not in idx]
    extra = dict(idx=list(idx), lr=0.03, lr_mult=0.5)
    if kind == "sgd":
        extra.update(momentum=0.7)
    return groups + [extra]


class ParamSet:
    """The parameters; `guarded` lists (buffer, first element, elements) of every misaligned tensor living between guards."""

    def __init__(self, dev, seed):
        self.dev, self.gen = dev, torch.Generator().manual_seed(seed)
        self.params = [torch.nn.Parameter(self.randn(n)) for n in NUMELS]
        self.guarded = []
        self.params.append(torch.nn.Parameter(self.misaligned(self.randn(CHUNK + 7))))      # 4 bytes into its buffer
        self.params.append(torch.nn.Parameter(self.randn(1027)))                            # aligned itself, misaligned gradient
        self.params.append(torch.nn.Parameter(self.randn(33)))                              # never gets a gradient
        self.params.append(torch.nn.Parameter(self.randn(CHUNK + 1)))                       # the size of params[7]
        self.live = set(range(len(self.params))) - {NO_G}      # who gets a gradient from fresh_grads()

    def randn(self, n, scale=1.0):
        return (torch.randn(n, generator=self.gen) * scale).to(self.dev)

    def misaligned(self, values):
        """`values` as a view that starts 4 bytes into a buffer of its own, guard elements at both ends."""
        n = values.numel()
        buf = torch.full((n + 8,), GUARD, device=self.dev)
        buf[1:1 + n] = values
        self.guarded.append((buf, 1, n))
        view = buf[1:1 + n]
        assert view.data_ptr() == buf.data_ptr() + 4 and (self.dev.type != "cuda" or view.data_ptr() % 16 == 4)
        return view

    def fresh_grads(self, scale=1.0):
        """New gradient tensors for the live parameters (new allocations: every address moves), None for the others."""
        keep = [p.grad for p in self.params]                 # held while the new ones are allocated: no address is reused
        for i, p in enumerate(self.params):
            if i not in self.live:
                p.grad = None
            elif i in (MIS_P, MIS_G):
                p.grad = self.misaligned(self.randn(p.numel(), scale))
            else:
                p.grad = self.randn(p.numel(), scale)
        del keep

    def refill_grads(self):
        """New values into the gradient tensors that are there: no address moves."""
        for p in self.params:
            if p.grad is not None:
                p.grad.copy_(self.randn(p.numel()))

    def guards_intact(self):
        return all(bool((b[:lo] == GUARD).all()) and bool((b[lo + n:] == GUARD).all()) for b, lo, n in self.guarded)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))     # (NaN equals itself here)


def _state_tensors(opt, p):
    return {k: v for k, v in opt.state.get(p, {}).items() if torch.is_tensor(v)}


class Run:
    """One optimizer over one ParamSet, and (twin=True) a torch.optim twin over clones of the parameters."""

    def __init__(self, kind, dev, seed, groups=None, twin=True, **kw):
        self.kind, self.dev, self.on_device = kind, dev, dev.type == "cuda"
        self.s = ParamSet(dev, seed)
        groups = default_groups(kind) if groups is None else groups
        self.members = sorted(i for g in groups for i in g["idx"])
        ours = [dict({k: v for k, v in g.items() if k != "idx"}, params=[self.s.params[i] for i in g["idx"]]) for g in groups]
        if kind == "sgd":
            self.opt = optim.RubiksSGD(ours, lr=0.1, weight_decay=5e-3, **kw)
        else:
            self.opt = optim.RubiksAdam(ours, lr=1e-2, weight_decay=5e-3, **kw)
        self.rec = ref.Recorder(kind, self.opt)
        self.t = {i: 0 for i in range(len(self.s.params))}   # steps every tensor has taken: what Adam's counters must say
        self.paths, self.worst_twin, self.worst_norm, self.last_coef = [], 0.0, 0.0, 1.0
        self.top = self.tparams = self.trec = None
        if twin:
            tparams = [torch.nn.Parameter(p.detach().clone()) for p in self.s.params]
            tgroups = [{"params": [tparams[i] for i in g["idx"]]} for g in groups]
            self.attach_twin(tparams, torch.optim.SGD(tgroups, lr=0.1) if kind == "sgd" else torch.optim.Adam(tgroups, lr=0.1))

    # ---- the twin ---------------------------------------------------------------------------------------------------
    def attach_twin(self, tparams, top):
        self.tparams, self.top, self.trec = tparams, top, ref.Recorder(self.kind, top)

    def _feed_twin(self):
        """The twin gets this step's fp32 inputs: our hyper-parameters (lr_mult / decay_mult multiplied in), parameters,
        state and gradients.  Its state must already have our keys and Adam's step counts: those are never copied."""
        for g, tg in zip(self.opt.param_groups, self.top.param_groups):
            tg["lr"], tg["weight_decay"] = ref.effective(g)
            for k in ("momentum", "dampening", "nesterov", "betas", "eps"):
                if k in g:
                    tg[k] = g[k]
        with torch.no_grad():
            for i in self.members:
                a, b = self.s.params[i], self.tparams[i]
                b.copy_(a)
                sa, sb = _state_tensors(self.opt, a), _state_tensors(self.top, b)
                assert set(sa) == set(sb), "tensor %d: our state has %s, torch's %s" % (i, sorted(sa), sorted(sb))
                for k, v in sa.items():
                    if k == "step":
                        assert float(v) == float(sb[k]), "tensor %d: our step count %g, torch's %g" % (i, float(v), float(sb[k]))
                    else:
                        sb[k].copy_(v)
                b.grad = None if a.grad is None else a.grad.detach().clone()

    def place_state(self, i, key, tensor):
        """Hands the optimizer (and the twin: a contiguous copy) a state tensor of the caller's making."""
        self.opt.state[self.s.params[i]][key] = tensor
        if self.top is not None:
            self.top.state[self.tparams[i]][key] = tensor.detach().clone().contiguous()

    def add_group(self, idx, **hyper):
        self.opt.add_param_group(dict(hyper, params=[self.s.params[i] for i in idx]))
        if self.top is not None:
            self.top.add_param_group({"params": [self.tparams[i] for i in idx]})
        self.members = sorted(self.members + list(idx))

    # ---- one step -----------------------------------------------------------------------------------------------------
    def _bits(self):
        return [(p.detach().clone(), {k: v.detach().clone() for k, v in _state_tensors(self.opt, p).items()},
                 None if p.grad is None else p.grad.detach().clone()) for p in self.s.params]

    def _check_counters(self):
        if self.kind != "adam":
            return
        for i, p in enumerate(self.s.params):
            st = self.opt.state.get(p, {})
            if "step" in st:
                assert torch.is_tensor(st["step"]) and not st["step"].is_cuda and st["step"].dim() == 0
                assert float(st["step"]) == self.t[i], "tensor %d: step %g after %d steps" % (i, float(st["step"]), self.t[i])
            else:
                assert self.t[i] == 0

    def step(self, path, same_table=False, nonfinite=False):
        """One opt.step() with everything checked.  path: "native" | "torch", what the step must take on the device.
        same_table: the step must neither build nor drop the job table.  nonfinite: the gradients hold NaN / inf on purpose."""
        assert path in ("native", "torch")
        opt, params = self.opt, self.s.params
        expect = path if self.on_device else "torch"
        mem = [params[i] for i in self.members]
        with_g = [i for i in self.members if params[i].grad is not None]
        assert with_g, "a timeline step needs a gradient"
        self._check_counters()
        bits = self._bits()
        snap = self.rec.before(mem)
        max_norm, coef, norm = opt.max_grad_norm, 1.0, None
        with np.errstate(all="ignore"):
            if max_norm is not None:
                norm = ref.global_norm([params[i].grad for i in with_g])
                coef = ref.clip_coef(norm, max_norm)
        self.last_coef = coef
        if self.top is not None:
            self._feed_twin()
            tmem, coef_t = [self.tparams[i] for i in self.members], 1.0
            tsnap = self.trec.before(tmem)                   # (the twin's snapshot holds the UNclipped gradients)
            if max_norm is not None:
                total = torch.nn.utils.clip_grad_norm_([self.tparams[i] for i in with_g], max_norm)
                coef_t = ref.clip_coef(float(total), max_norm)

        counts, table = (opt.native_steps, opt.torch_steps), opt._table
        opt.step()
        if self.on_device:
            torch.cuda.synchronize()
        took = (opt.native_steps - counts[0], opt.torch_steps - counts[1])
        self.paths.append("native" if took == (1, 0) else "torch" if took == (0, 1) else str(took))
        assert took == ((1, 0) if expect == "native" else (0, 1)), \
            "step %d must take the %s path: native_steps +%d, torch_steps +%d" % (len(self.paths), expect, *took)
        if same_table and self.on_device:
            assert table is not None and opt._table is table, "step %d built or dropped the job table" % len(self.paths)

        with np.errstate(all="ignore"):
            self.rec.check(mem, snap, coef=coef, nonfinite=nonfinite)
        for i, (p, (p0, st0, g0)) in enumerate(zip(params, bits)):
            st = _state_tensors(opt, p)
            if i not in with_g:                              # no gradient (or not the optimizer's): nothing of it moved
                assert torch.equal(p, p0) and set(st) == set(st0) and all(torch.equal(st[k], st0[k]) for k in st0), i
                assert (p.grad is None) == (g0 is None) and (g0 is None or torch.equal(p.grad, g0)), i
                continue
            self.t[i] += 1
            if self.kind == "sgd":
                group = self.rec._group(p)
                if float(group["momentum"]) == 0:            # torch keeps an old buffer, unread and unwritten
                    assert set(st) == set(st0) and all(torch.equal(st[k], st0[k]) for k in st0), i
                else:
                    assert set(st) == {"momentum_buffer"}, i
            else:
                assert set(st) == {"step", "exp_avg", "exp_avg_sq"}, i
            if opt.zero_grads:
                assert not p.grad.any(), "tensor %d: zero_grads left a gradient" % i
            else:
                assert _same_bits(p.grad, g0), "tensor %d: the step changed a gradient it was not to zero" % i
        self._check_counters()
        if max_norm is not None:
            got = float(opt.last_grad_norm)
            assert opt.last_grad_norm.dtype == torch.float32 and opt.last_grad_norm.device.type == self.dev.type
            if math.isfinite(norm):
                assert abs(got - norm) <= 1e-6 * norm, (got, norm)
                self.worst_norm = max(self.worst_norm, abs(got - norm) / norm if norm else 0.0)
            else:
                assert got == norm or (got != got and norm != norm), (got, norm)
        assert self.s.guards_intact(), "step %d wrote a guard element" % len(self.paths)

        if self.top is not None:
            self.top.step()
            with np.errstate(all="ignore"):
                w = ref.compare(self.rec, mem, snap, self.trec, tmem, tsnap, coef_a=coef, coef_b=coef_t, nonfinite=nonfinite)
            self.worst_twin = max(self.worst_twin, w)

    def report(self, name):
        twin = "; distance to torch.optim / allowed %.3g" % self.worst_twin if self.top is not None else ""
        norm = "; norm off by %.2g relative" % self.worst_norm if self.worst_norm else ""
        print("%s/%s on %s: %s; worst error / bound %s%s%s" % (name, self.kind, self.dev.type, " ".join(self.paths),
                                                               {k: float("%.3g" % v) for k, v in self.rec.worst.items()}, twin, norm))


# ---- the timelines ---------------------------------------------------------------------------------------------------
LATE = (8, MIS_G)          # several chunks in a group with momentum; a misaligned gradient in the group without


def _adam_path(kind, grouping):
    """Where a tensor's step count differs from its group's: RubiksAdam wants one count per group, RubiksSGD has none."""
    return "torch" if kind == "adam" and grouping == "shared" else "native"


def late_first_gradient(kind, dev, grouping="shared"):
    """A: two tensors have no gradient for two steps and then get one.  SGD: their buffers start as g' (the torch.empty_like
    they are allocated as must not show); the other tensors' records carry no first-step flag in that launch.  Adam with the
    late tensors in a group of their own: the groups' step counts differ, so do their bias corrections, all native.  Adam with
    them inside groups that have stepped: the counts within a group differ, and from then on every step is the torch path's."""
    run = Run(kind, dev, 11, groups=own_group(kind, LATE) if grouping == "own" else None)
    run.s.live -= set(LATE)
    for _ in range(2):
        run.s.fresh_grads()
        run.step("native")
    run.s.live |= set(LATE)
    for _ in range(2):
        run.s.fresh_grads()
        run.step(_adam_path(kind, grouping))
    assert [run.t[i] for i in LATE] == [2, 2] and run.t[0] == 4
    if kind == "sgd":
        assert all("momentum_buffer" in run.opt.state[run.s.params[i]] for i in (8,))
    run.report("A late first gradient (%s)" % grouping)
    return run


def gradient_disappears(kind, dev, grouping="shared"):
    """B: two tensors lose their gradient for two steps (Run.step holds them bit-identical meanwhile, Adam's step included).
    Back again, SGD goes on native with the old buffers and no first-step flag; Adam as in A."""
    run = Run(kind, dev, 12, groups=own_group(kind, LATE) if grouping == "own" else None)
    for live, path in ((True, "native"), (False, "native"), (True, _adam_path(kind, grouping))):
        run.s.live = (run.s.live | set(LATE)) if live else (run.s.live - set(LATE))
        for _ in range(2):
            run.s.fresh_grads()
            run.step(path)
    assert [run.t[i] for i in LATE] == [4, 4] and run.t[0] == 6
    run.report("B gradient disappears and returns (%s)" % grouping)
    return run


def address_churn(kind, dev):
    """C: every gradient re-allocated; two parameters of one size (in different groups) exchange their gradient tensors, so the
    same addresses come in another order; two parameters' .data re-pointed (one of them into a new guarded, misaligned
    buffer).  A table is kept only while no pointer moved: every step native, every guard intact."""
    run = Run(kind, dev, 13)
    p = run.s.params
    for _ in range(2):
        run.s.fresh_grads()
        run.step("native")
    assert p[7].shape == p[PAIR].shape and run.rec._group(p[7]) is not run.rec._group(p[PAIR])
    before = sorted(q.grad.data_ptr() for q in p if q.grad is not None)
    p[7].grad, p[PAIR].grad = p[PAIR].grad, p[7].grad
    assert before == sorted(q.grad.data_ptr() for q in p if q.grad is not None)
    run.step("native")
    old = [p[6].data, p[MIS_P].data]                         # held: the new tensors get new addresses
    p[6].data = p[6].detach().clone()
    p[MIS_P].data = run.s.misaligned(p[MIS_P].detach().clone())
    assert p[6].data_ptr() != old[0].data_ptr() and p[MIS_P].data_ptr() != old[1].data_ptr()
    snapshot = [t.clone() for t in old]
    run.step("native")
    run.s.fresh_grads()
    run.step("native")
    assert all(torch.equal(a, b) for a, b in zip(old, snapshot))            # the abandoned storage is nobody's any more
    run.report("C address churn")
    return run


def accumulation(kind, dev):
    """D: zero_grads=True and kept gradients, two micro-batches added in place per round, against a twin of ours that is handed
    the summed gradients in fresh tensors with zero_grads=False: bit-equal.  From the first step whose records carry no
    first-step flag on, no pointer moves and the table is the same object."""
    run = Run(kind, dev, 14, twin=False, max_grad_norm=5.0, zero_grads=True)
    other = Run(kind, dev, 14, twin=False, max_grad_norm=5.0)
    flags_spent = 1 if kind == "sgd" else 0                   # RubiksSGD drops the table whose first-step bits it spent
    for rnd in range(3):
        other.s.fresh_grads()
        micro = [[None if q.grad is None else run.s.randn(q.numel()) for q in other.s.params] for _ in range(2)]
        if rnd == 0:
            run.s.fresh_grads()
            for q in run.s.params:
                if q.grad is not None:
                    q.grad.zero_()
        for q, o, a, b in zip(run.s.params, other.s.params, *micro):
            if a is not None:
                assert not q.grad.any()
                q.grad.add_(a)
                q.grad.add_(b)
                o.grad.copy_(a + b)
        run.step("native", same_table=rnd > flags_spent)
        other.step("native")
        assert all(torch.equal(a, b) for a, b in zip(run.s.params, other.s.params))
        for a, b in zip(run.s.params, other.s.params):
            sa, sb = _state_tensors(run.opt, a), _state_tensors(other.opt, b)
            assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
        assert float(run.opt.last_grad_norm) == float(other.opt.last_grad_norm)
    run.report("D accumulation into kept gradients")
    return run


def hyper_parameters_move(kind, dev):
    """E: one hyper-parameter at a time changes between steps while the gradients keep their addresses (new values in place).
    They travel in the kernel arguments: the table stays the same object, except where SGD's momentum crosses 0 (a record
    holds a buffer only where it is used) and after a step that spent first-step flags."""
    run = Run(kind, dev, 15)
    opt, groups = run.opt, run.opt.param_groups
    run.s.fresh_grads()

    def step(same_table=True):
        run.s.refill_grads()
        run.step("native", same_table=same_table)

    step(same_table=False)
    step(same_table=kind == "adam")                           # (SGD: the first step's table went with its flags)
    groups[0]["weight_decay"] = 0.3
    step()
    groups[1]["lr_mult"] = 0.5
    step()
    groups[0]["decay_mult"] = 1.5
    step()
    groups[2]["lr"] = 0.004
    step()
    if kind == "sgd":
        assert groups[1]["momentum"] == 0.0 and not any(_state_tensors(opt, q) for q in groups[1]["params"])
        for mu, first in ((0.9, True), (0.0, False), (0.9, False)):
            groups[1]["momentum"] = mu
            held = [_state_tensors(opt, q).get("momentum_buffer") for q in groups[1]["params"]]
            assert all((h is None) == first for q, h in zip(groups[1]["params"], held) if q.grad is not None)
            step(same_table=False)                            # the buffer appears as g' / is left alone / is used again
            if not first:                                     # ... and it is the old tensor, not a new one
                assert all(_state_tensors(opt, q).get("momentum_buffer") is h for q, h in zip(groups[1]["params"], held))
            if first:
                step(same_table=False)                        # (the table that carried the flags is gone)
                step()
        groups[1]["momentum"] = 0.5
        step()
        groups[0]["nesterov"] = False
        step()
        groups[2]["dampening"] = 0.0
        step()
        groups[2]["nesterov"] = True
        step()
        groups[0]["dampening"] = 0.25
        step()
    else:
        groups[0]["betas"] = (0.8, 0.999)
        step()
        groups[1]["betas"] = (0.9, 0.95)
        step()
        groups[2]["eps"] = 1e-3
        step()
    for max_norm, clips in ((1.0, True), (1e4, False), (None, None)):       # the set's norm is ~ 170
        opt.max_grad_norm = max_norm
        step()                                                # (the clipping workspace joins a table that is kept)
        assert clips is None or ((run.last_coef < 1.0) == clips and (not run.on_device or opt._table.partials is not None))
    for flag in (True, False, True):
        opt.zero_grads = flag
        step()
    run.report("E hyper-parameters move")
    return run


def _guarded_state(run, sd):
    """`sd` with every state tensor moved to a view 4 bytes off a 16-byte boundary of ONE flat buffer, guards in between."""
    tensors = [(k, name) for k, st in sd["state"].items() for name, v in st.items() if torch.is_tensor(v) and v.numel() > 1 - v.dim()]     # (not `step`, not an empty tensor)
    offs, o = [], 1
    for k, name in tensors:
        offs.append(o)
        o = (o + sd["state"][k][name].numel() + 3) // 4 * 4 + 5
    flat = torch.full((o + 8,), GUARD, device=run.dev)
    free = torch.ones(flat.numel(), dtype=torch.bool, device=run.dev)
    for (k, name), lo in zip(tensors, offs):
        v = sd["state"][k][name]
        flat[lo:lo + v.numel()] = v.reshape(-1)
        free[lo:lo + v.numel()] = False
        sd["state"][k][name] = flat[lo:lo + v.numel()].view(v.shape)
        assert (sd["state"][k][name].data_ptr() - flat.data_ptr()) % 16 == 4
    return flat, free


def state_hand_over(kind, dev):
    """F: two steps, state_dict() into a torch.optim twin on the same device, one step of both; the twin's state_dict() into
    a fresh optimizer of ours, two steps of both, and a load_state_dict() into that optimizer while its table is live (the
    step must then write the loaded tensors); and that state once more as 4-bytes-off views into one guarded buffer, where
    the state alone puts every tensor on the dword path.  Ours is native throughout and Adam's counters go on counting."""
    groups = default_groups(kind, hypers=PLAIN)               # (torch reads the loaded groups' lr as it stands)
    run = Run(kind, dev, 16, groups=groups, twin=False)
    for _ in range(2):
        run.s.fresh_grads()
        run.step("native")
    tparams = [torch.nn.Parameter(q.detach().clone()) for q in run.s.params]
    tgroups = [{"params": [tparams[i] for i in g["idx"]]} for g in groups]
    top = torch.optim.SGD(tgroups, lr=0.1) if kind == "sgd" else torch.optim.Adam(tgroups, lr=0.1)
    top.load_state_dict(copy.deepcopy(run.opt.state_dict()))                # ours -> torch (a copy, as a saved file is)
    run.attach_twin(tparams, top)
    run.s.fresh_grads()
    run.step("native")
    run.report("F state hand-over, ours -> torch")

    def successor(before):
        """A fresh optimizer of ours on the twin's parameter values, the twin attached; its state is the caller's to load."""
        nxt = Run(kind, dev, 16, groups=groups, twin=False)
        with torch.no_grad():
            for a, b in zip(nxt.s.params, tparams):
                a.copy_(b)
        nxt.t = dict(before.t)
        nxt.attach_twin(tparams, top)
        nxt.s.fresh_grads()
        return nxt

    back = successor(run)
    back.opt.load_state_dict(copy.deepcopy(top.state_dict()))               # torch -> ours
    back.step("native")
    back.step("native", same_table=True)                                    # (no pointer moved, no flag to spend)
    held = [v for q in back.s.params for v in _state_tensors(back.opt, q).values()]
    back.opt.load_state_dict(copy.deepcopy(back.opt.state_dict()))          # new state tensors under a live table: no
    back.step("native")                                                     # pointer of its key moved, yet it must go
    assert back.on_device is False or all(v.dim() == 0 or not v.numel() or v.data_ptr() not in {h.data_ptr() for h in held}
                                          for q in back.s.params for v in _state_tensors(back.opt, q).values())
    back.report("F state hand-over, torch -> ours")

    last = successor(back)
    sd = copy.deepcopy(top.state_dict())
    flat, free = _guarded_state(last, sd)
    last.opt.load_state_dict(sd)                                            # (load_state_dict keeps the tensors it is given)
    for q in last.s.params:
        for k, v in _state_tensors(last.opt, q).items():
            assert k == "step" or not v.numel() or (v.data_ptr() - flat.data_ptr()) % 16 == 4, "the loaded state is no longer the view"
    aligned = [q for i, q in enumerate(last.s.params) if i not in (MIS_P, MIS_G) and q.numel()]
    assert not last.on_device or all(q.data_ptr() % 16 == 0 and q.grad.data_ptr() % 16 == 0 for q in aligned if q.grad is not None)
    last.step("native")
    assert bool((flat[free] == GUARD).all()), "a step on misaligned state wrote between the state tensors"
    last.report("F state hand-over, misaligned state")
    return last


def add_group_mid_run(kind, dev):
    """G: add_param_group() after two steps.  The old tensors go on (Adam: their counts survive the rebuild of the shared
    counter tensor), the new group starts at its first step; a group of its own has a count of its own: all native."""
    new = [5, 8, MIS_G]
    groups = default_groups(kind)
    for g in groups:
        g["idx"] = [i for i in g["idx"] if i not in new]
    run = Run(kind, dev, 17, groups=groups)
    run.s.live -= set(new)
    for _ in range(2):
        run.s.fresh_grads()
        run.step("native")
    run.add_group(new, lr=0.02, lr_mult=2.0, **({"momentum": 0.6} if kind == "sgd" else {"betas": (0.7, 0.99)}))
    run.s.live |= set(new)
    for _ in range(2):
        run.s.fresh_grads()
        run.step("native")
    assert [run.t[i] for i in new] == [2, 2, 2] and run.t[0] == 4
    run.report("G add_param_group mid-run")
    return run


def noncontiguous_gradient(kind, dev):
    """H: one step with a non-contiguous gradient on one tensor is the torch path's (the native path takes contiguous
    tensors); the steps before and after are native, on the state the other path left."""
    run = Run(kind, dev, 18)
    for path in ("native", "native", "torch", "native", "native"):
        run.s.fresh_grads()
        if path == "torch":
            q = run.s.params[8]
            q.grad = run.s.randn(2 * q.numel())[::2]
            assert not q.grad.is_contiguous()
        run.step(path)
    run.report("H one non-contiguous gradient")
    return run


def refused_after_flags(kind, dev):
    """H: a hand-placed non-contiguous momentum_buffer on one tensor, before the first step.  The table is refused when the
    state is looked at, after the other tensors' buffers have been allocated (uninitialised) and flagged for their first
    step: the torch path must still start them as g'.  With a contiguous buffer in its place the next step is native."""
    assert kind == "sgd"
    run = Run(kind, dev, 19)
    q = run.s.params[6]
    run.place_state(6, "momentum_buffer", run.s.randn(2 * q.numel())[::2])
    for _ in range(2):
        run.s.fresh_grads()
        run.step("torch")
    assert not run.opt.state[q]["momentum_buffer"].is_contiguous()
    run.opt.state[q]["momentum_buffer"] = run.opt.state[q]["momentum_buffer"].contiguous()
    for _ in range(2):
        run.s.fresh_grads()
        run.step("native")
    run.report("H table refused after the first-step flags")
    return run


def _mask(t):
    return ~torch.isfinite(t.detach())


def nonfinite_gradients(kind, dev, case):
    """I: one ordinary step, then one fed chosen values.  noclip: +inf, -inf and two NaN elements poison their own elements and
    no other.  clip-inf: the norm is inf and the coefficient 0, every other element moves by its decay alone, the inf element
    becomes NaN.  clip-nan: every tensor with a gradient is NaN throughout (clip_grad_norm_'s behaviour), the others untouched.
    huge: gradients of 1e25, whose squares overflow fp32 but not the fp64 sum: a finite norm, a correct step (no torch twin:
    clip_grad_norm_ forms the norm in fp32).  zeros: norm 0, coefficient 1."""
    clip = case != "noclip"
    run = Run(kind, dev, 20, twin=case != "huge", max_grad_norm=1.0 if clip else None)
    p = run.s.params
    run.s.live -= {7}
    run.s.fresh_grads()
    run.step("native")
    run.s.fresh_grads(scale=1e25 if case == "huge" else 1.0)
    with torch.no_grad():
        if case == "noclip":
            p[8].grad[5], p[8].grad[CHUNK + 3], p[4].grad[2], p[MIS_G].grad[7] = math.inf, -math.inf, math.nan, math.nan
        elif case == "clip-inf":
            p[8].grad[5] = math.inf
        elif case == "clip-nan":
            p[4].grad[2] = math.nan
        elif case == "zeros":
            for q in p:
                if q.grad is not None:
                    q.grad.zero_()
    poisoned = [None if q.grad is None else _mask(q.grad) for q in p]
    untouched = [q.detach().clone() for q in p]
    run.step("native", nonfinite=case in ("noclip", "clip-inf", "clip-nan"))
    norm = float(run.opt.last_grad_norm) if clip else None
    for i, (q, m) in enumerate(zip(p, poisoned)):
        if m is None:
            assert torch.equal(q, untouched[i])
        elif case == "clip-nan":
            assert bool(q.detach().isnan().all()), i
        else:
            assert torch.equal(_mask(q), m), "tensor %d: the non-finite elements are not the gradient's" % i
    if case == "clip-inf":
        assert norm == math.inf and bool(p[8].detach()[5].isnan())
    elif case == "clip-nan":
        assert norm != norm
    elif case == "huge":
        assert 1e26 < norm < math.inf and all(bool(torch.isfinite(q).all()) for q in p)
    elif case == "zeros":
        assert norm == 0.0
    run.report("I %s" % case)
    return run


TIMELINES = [("A-late-%s" % g, late_first_gradient, k, dict(grouping=g)) for k, g in (("sgd", "shared"), ("adam", "own"), ("adam", "shared"))]
TIMELINES += [("B-vanish-%s" % g, gradient_disappears, k, dict(grouping=g)) for k, g in (("sgd", "shared"), ("adam", "own"), ("adam", "shared"))]
for _name, _fn in (("C-churn", address_churn), ("D-accumulate", accumulation), ("E-hyper", hyper_parameters_move),
                   ("F-state", state_hand_over), ("G-add-group", add_group_mid_run), ("H-noncontiguous-grad", noncontiguous_gradient)):
    TIMELINES += [(_name, _fn, k, {}) for k in ("sgd", "adam")]
TIMELINES.append(("H-refused-after-flags", refused_after_flags, "sgd", {}))
TIMELINES += [("I-%s" % c, nonfinite_gradients, k, dict(case=c)) for c in ("noclip", "clip-inf", "clip-nan", "huge", "zeros")
              for k in ("sgd", "adam")]
IDS = ["%s-%s" % (name, kind) for name, _, kind, _ in TIMELINES]


def run_timeline(entry, dev):
    name, fn, kind, kw = entry
    return fn(kind, dev, **kw)
