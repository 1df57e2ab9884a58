"""The one-launch optimizer step (rk_optim.hip through rubiksnet_amd.optim) on the device, against the fp64 reference and
bounds of tests/_optim_ref.py.  One hand-made parameter set holds every size at which the kernel takes another path: no
element, fewer than one 16-byte access, a tail behind whole accesses, one element short of / exactly / one past a chunk,
several chunks; a parameter and a gradient that start 4 bytes into a larger buffer (dword path) between guard elements
that must stay untouched; a parameter without a gradient.  Every test prints the worst error as a multiple of its bound."""
import numpy as np
import pytest
import torch

import _optim_ref as ref
from rubiksnet_amd import RubiksNet, dp, optim

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK = 4096
NUMELS = [0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
GUARD = 12345.0


class _Set:
    """The parameter set.  `pbuf` / `gbufs` are the buffers behind the misaligned tensors (guard elements at both ends)."""

    def __init__(self, seed):
        self.gen = torch.Generator().manual_seed(seed)
        self.params = [torch.nn.Parameter(self._randn(n)) for n in NUMELS]
        self.pbuf = torch.full((CHUNK + 7 + 8,), GUARD, device=DEV)
        self.pbuf[1:1 + CHUNK + 7] = self._randn(CHUNK + 7)
        self.params.append(torch.nn.Parameter(self.pbuf[1:1 + CHUNK + 7]))      # 4 bytes into its buffer
        self.params.append(torch.nn.Parameter(self._randn(1027)))               # aligned itself, misaligned gradient
        self.params.append(torch.nn.Parameter(self._randn(33)))                 # never gets a gradient
        self.mis_p, self.mis_g, self.no_g = len(NUMELS), len(NUMELS) + 1, len(NUMELS) + 2
        assert self.params[self.mis_p].data_ptr() % 16 == 4 and self.params[self.mis_p].data_ptr() == self.pbuf.data_ptr() + 4
        self.gbufs = []

    def _randn(self, n):
        return torch.randn(n, generator=self.gen).to(DEV)

    def new_grads(self):
        """Fresh gradient tensors (new allocations: the pointers move), the two misaligned ones inside guarded buffers."""
        keep = [p.grad for p in self.params]                 # held while the new ones are allocated: no address is reused
        self.gbufs = []
        for i, p in enumerate(self.params):
            if i == self.no_g:
                p.grad = None
            elif i in (self.mis_p, self.mis_g):
                buf = torch.full((p.numel() + 8,), GUARD, device=DEV)
                buf[1:1 + p.numel()] = self._randn(p.numel())
                self.gbufs.append(buf)
                p.grad = buf[1:1 + p.numel()]
                assert p.grad.data_ptr() % 16 == 4
            else:
                p.grad = self._randn(p.numel())
        del keep

    def groups(self, n_groups=3):
        ps = self.params
        if n_groups == 3:
            return [{"params": ps[0::3], "lr": 0.05, "weight_decay": 1e-2, "lr_mult": 0.1, "decay_mult": 0.0},
                    {"params": ps[1::3], "lr_mult": 3.0, "decay_mult": 2.0},
                    {"params": ps[2::3], "lr": 0.02, "weight_decay": 1e-3}]
        return [{"params": ps[i::n_groups], "lr": 0.01 * (i + 1), "lr_mult": 1.0 + 0.25 * i} for i in range(n_groups)]

    def guards_intact(self):
        n = self.params[self.mis_p].numel()
        ok = bool((self.pbuf[0] == GUARD) and (self.pbuf[1 + n:] == GUARD).all())
        return ok and all(bool(b[0] == GUARD) and bool((b[-7:] == GUARD).all()) for b in self.gbufs)


SGD_GROUP_CASES = [dict(momentum=0.9, dampening=0.0, nesterov=True), dict(momentum=0.0), dict(momentum=0.8, dampening=0.3)]


def _make(kind, s, n_groups=3, **kw):
    groups = s.groups(n_groups)
    if kind == "sgd":
        for i, g in enumerate(groups):                       # nesterov, no momentum (no buffer), dampening: one group each
            g.update(SGD_GROUP_CASES[i % 3])
        return optim.RubiksSGD(groups, lr=0.1, weight_decay=5e-3, **kw)
    return optim.RubiksAdam(groups, lr=1e-2, weight_decay=5e-3, **kw)


def _run(kind, seed, steps=3, n_groups=3, max_norm=None, check=True, **kw):
    s = _Set(seed)
    opt = _make(kind, s, n_groups, max_grad_norm=max_norm, **kw)
    rec = ref.Recorder(kind, opt)
    untouched = s.params[s.no_g].detach().clone()
    norms = []
    for step in range(steps):
        s.new_grads()
        snap = rec.before(s.params)
        norm = ref.global_norm([p.grad for p in s.params if p.grad is not None])
        opt.step()
        if check:
            rec.check(s.params, snap, coef=ref.clip_coef(norm, max_norm))
        if max_norm is not None:
            norms.append((float(opt.last_grad_norm), norm))
        for group in opt.param_groups:                       # an lr schedule: no table upload, still the right rate
            group["lr"] *= 0.5
    torch.cuda.synchronize()
    assert s.guards_intact()
    assert torch.equal(s.params[s.no_g], untouched) and not opt.state.get(s.params[s.no_g])
    return s, opt, rec, norms


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_three_steps_against_fp64(kind):
    s, opt, rec, _ = _run(kind, 1)
    assert opt.native_steps == 3 and opt.torch_steps == 0
    if kind == "sgd":                                        # torch's state layout: a buffer where the group has momentum
        for g in opt.param_groups:
            for p in g["params"]:
                assert (("momentum_buffer" in opt.state[p]) == (g["momentum"] != 0)) or p is s.params[s.no_g]
    else:
        assert all(float(opt.state[p]["step"]) == 3 and not opt.state[p]["step"].is_cuda
                   for i, p in enumerate(s.params) if i != s.no_g)
    print("%s, 3 steps, 3 groups: worst error / bound %s" % (kind, rec.worst))


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_clipping_norm_and_determinism(kind):
    """The norm of this set is ~ 160 (25 600 standard normal values): max_norm 1 clips, 1e4 does not."""
    for max_norm in (1.0, 1e4):
        s, opt, rec, norms = _run(kind, 2, max_norm=max_norm)
        assert opt.native_steps == 3
        for got, want in norms:
            assert (ref.clip_coef(want, max_norm) < 1.0) == (max_norm == 1.0)
            assert abs(got - want) <= 1e-6 * want, (got, want)
        again = _run(kind, 2, max_norm=max_norm, check=False)[0]
        assert all(torch.equal(a, b) for a, b in zip(s.params, again.params))          # bit for bit
        print("%s, max_norm %g: worst error / bound %s; norm %.9g vs fp64 %.9g" % (kind, max_norm, rec.worst, *norms[-1]))


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_zero_grads_in_the_step(kind):
    plain = _run(kind, 3, steps=2, max_norm=5.0)[0]
    s, opt, rec, _ = _run(kind, 3, steps=2, max_norm=5.0, check=False, zero_grads=True)
    assert opt.native_steps == 2
    assert all(torch.equal(a, b) for a, b in zip(plain.params, s.params))
    assert all(not p.grad.any() for p in s.params if p.grad is not None) and any(p.grad.any() for p in plain.params if p.grad is not None)
    assert s.guards_intact()


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_nine_groups_take_the_torch_path(kind):
    s, opt, rec, _ = _run(kind, 4, steps=2, n_groups=9, max_norm=50.0)
    assert opt.torch_steps == 2 and opt.native_steps == 0
    print("%s, 9 groups (torch ops on the device): worst error / bound %s" % (kind, rec.worst))


def _kinds(net):
    kinds = {"shift": [], "conv": [], "bn": [], "fc": []}
    for n, p in net.named_parameters():
        k = "shift" if n.endswith("shift") else "fc" if "new_fc" in n else "conv" if p.dim() == 4 else "bn" if p.dim() == 1 else None
        if k:
            kinds[k].append(n)
    return kinds


@pytest.mark.parametrize("kind,amp", [("sgd", None), ("adam", torch.bfloat16)], ids=["sgd-fp32", "adam-bf16"])
def test_train_step_matches_the_torch_optimizer(kind, amp):
    """RubiksNet-Tiny, batch 1: dp.train_step with kind="hip_*" and a twin from the same seed with the torch optimizer the
    parent uses.  Same loss; every parameter within twice the bound of its twin's (tests/_optim_ref.py: compare).  Each
    twin is referenced from ITS OWN gradients: the fp32 backward gives both the same bits (128 of 128 tensors), the bf16
    backward does not (122 of 128 on an MI355X: a property of that backward, before any optimizer runs), and for a tensor
    whose two gradients differ the allowed distance grows by exactly the distance of the two fp64 references -- nothing else
    can be asked of two correct optimizers fed different gradients.  Where the gradients agree it is twice the bound."""
    nets, opts, losses = [], [], []
    clips = labels = None
    for k in ("hip_" + kind, kind):
        torch.manual_seed(5)
        net = RubiksNet("tiny", 11, num_frames=8, verbose=False).to(DEV)
        opt = dp.make_optimizer(net, lr=1e-2, lr_shift_mult=0.1, kind=k, weight_decay=5e-4)
        if clips is None:
            clips, labels = torch.randn(1, 8, 3, 224, 224, device=DEV), torch.randint(0, 11, (1,), device=DEV)
        before = {n: p.detach().clone() for n, p in net.named_parameters()}
        with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
            losses.append(float(dp.train_step(net, opt, clips, labels).detach()))
        nets.append((net, before))
        opts.append(opt)
    assert type(opts[0]) is (optim.RubiksSGD if kind == "sgd" else optim.RubiksAdam) and opts[0].native_steps == 1
    assert type(opts[1]) is (torch.optim.SGD if kind == "sgd" else torch.optim.Adam)
    assert losses[0] == losses[1] and np.isfinite(losses[0])
    (net_a, before_a), (net_b, before_b) = nets
    ra, rb = ref.Recorder(kind, opts[0]), ref.Recorder(kind, opts[1])
    pa, pb = [p for _, p in net_a.named_parameters()], [p for _, p in net_b.named_parameters()]
    assert all(p.grad is not None for p in pa + pb)

    def first_step(named_before, params):
        return [{"p": ref.f64(named_before[n]), "g": ref.f64(p.grad), "momentum_buffer": None, "exp_avg": None,
                 "exp_avg_sq": None, "t": 0} for (n, _), p in zip(named_before.items(), params)]

    sa, sb = first_step(before_a, pa), first_step(before_b, pb)
    ra.check(pa, sa)
    worst = ref.compare(ra, pa, sa, rb, pb, sb)
    moved = {n for (n, p) in net_a.named_parameters() if not torch.equal(p, before_a[n])}
    for k, names in _kinds(net_a).items():                   # the step really moved every kind of parameter
        assert names and moved.intersection(names), k
    assert all(torch.isfinite(p).all() for p in pa)
    same = sum(torch.equal(a.grad, b.grad) for a, b in zip(pa, pb))
    print("%s train step: loss %.6f, worst error / bound %s, distance to the torch twin / allowed %.6g, %d of %d tensors moved, "
          "%d gradients bit-equal to the twin's" % (kind, losses[0], ra.worst, worst, len(moved), len(pa), same))
