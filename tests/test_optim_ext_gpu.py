"""rk_optim_step_ext_f32 through rubiksnet_amd.optim on the device: AdamW, the EMA shadow and the non-finite guard against
the fp64 stages and bounds of tests/_optim_ext_ref.py.  The parameter set is tests/test_optim_gpu.py's -- every size at which
the kernel takes another path, a parameter and two gradients 4 bytes into guarded buffers, a parameter without a gradient
-- plus one aligned parameter of more than a chunk whose EMA SHADOW sits 4 bytes into a guarded buffer (the dword path is
then chosen by the shadow alone).  Tests that measure print the worst error as a multiple of its bound."""
import numpy as np
import pytest
import torch

import _optim_ext_ref as ext
import _optim_ref as ref
from rubiksnet_amd import RubiksNet, dp, optim
from test_optim_gpu import CHUNK, DEV, GUARD, SGD_GROUP_CASES, _Set

pytestmark = pytest.mark.gpu
KINDS = ["sgd", "adam", "adamw"]
CLASSES = {"sgd": optim.RubiksSGD, "adam": optim.RubiksAdam, "adamw": optim.RubiksAdamW}


class _ExtSet(_Set):
    def __init__(self, seed):
        super().__init__(seed)
        self.params.append(torch.nn.Parameter(self._randn(CHUNK + 5)))          # aligned itself; its shadow will not be
        self.mis_e = len(self.params) - 1
        self.ebuf = None

    def misalign_shadow(self, opt):
        """Replaces state[p]["ema"] of parameter mis_e by a view 4 bytes into a guarded buffer (before the first step)."""
        p = self.params[self.mis_e]
        self.ebuf = torch.full((p.numel() + 8,), GUARD, device=DEV)
        self.ebuf[1:1 + p.numel()] = p.detach()
        opt.state[p]["ema"] = self.ebuf[1:1 + p.numel()]
        assert opt.state[p]["ema"].data_ptr() % 16 == 4 and p.data_ptr() % 16 == 0

    def fill_grads(self, scale=1.0):
        """New values in the SAME gradient tensors (no pointer moves: the job table can stay)."""
        if not self.gbufs:
            self.new_grads()
        for p in self.params:
            if p.grad is not None:
                p.grad.copy_(self._randn(p.numel()) * scale)

    def guards_intact(self):
        ok = super().guards_intact()
        return ok and (self.ebuf is None or (bool(self.ebuf[0] == GUARD) and bool((self.ebuf[-7:] == GUARD).all())))


def _make(kind, s, torch_path=False, **kw):
    groups = s.groups(3)
    if kw.get("weight_decay") == 0.0:                        # (some groups name a decay of their own)
        for g in groups:
            g["weight_decay"] = 0.0
    if kind == "sgd":
        for g, case in zip(groups, SGD_GROUP_CASES):         # nesterov, no momentum (no buffer), dampening: one group each
            g.update(case)
        opt = optim.RubiksSGD(groups, lr=0.1, weight_decay=5e-3, **kw)
    else:
        opt = CLASSES[kind](groups, lr=1e-2, weight_decay=kw.pop("weight_decay", 5e-2 if kind == "adamw" else 5e-3), **kw)
    if torch_path:
        opt._lib = False                                     # "no built library": the torch-op path on the device
    if opt.ema_decay is not None and not torch_path:
        s.misalign_shadow(opt)
    return opt


def _run(kind, seed, steps=3, check=True, **kw):
    s = _ExtSet(seed)
    opt = _make(kind, s, **kw)
    rec = ext.Recorder(kind, opt)
    untouched = s.params[s.no_g].detach().clone()
    for step in range(steps):
        s.new_grads()                                        # fresh allocations: every step builds its table
        snap = rec.before(s.params)
        norm = ref.global_norm([p.grad for p in s.params if p.grad is not None])
        opt.step()
        if check:
            rec.check(s.params, snap, coef=ref.clip_coef(norm, opt.max_grad_norm))
        for group in opt.param_groups:
            group["lr"] *= 0.5
    torch.cuda.synchronize()
    assert s.guards_intact()
    assert torch.equal(s.params[s.no_g], untouched) and not opt.state.get(s.params[s.no_g])
    assert opt.native_steps == steps and opt.torch_steps == 0
    return s, opt, rec


CONFIGS = {"adamw": ("adamw", {}), "adamw-ema": ("adamw", dict(ema_decay=0.9)),
           "adam-ema-guard-clip": ("adam", dict(ema_decay=0.9, skip_nonfinite=True, max_grad_norm=1.0)),
           "sgd-ema-guard": ("sgd", dict(ema_decay=0.9, skip_nonfinite=True))}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_three_steps_against_fp64(name):
    kind, kw = CONFIGS[name]
    s, opt, rec = _run(kind, 1, **kw)
    if "ema_decay" in kw:
        assert "ema" in rec.worst and opt.state[s.params[s.mis_e]]["ema"].data_ptr() == s.ebuf.data_ptr() + 4
        assert not torch.equal(opt.state[s.params[s.mis_e]]["ema"], s.params[s.mis_e])
    else:
        assert all("ema" not in opt.state[p] for p in s.params)
    if kw.get("skip_nonfinite"):
        assert opt.skipped_steps == 0
    print("%s, 3 steps, 3 groups: worst error / bound %s" % (name, rec.worst))


def _same(sa, oa, sb, ob):
    keys = ("momentum_buffer", "exp_avg", "exp_avg_sq")
    for i, (p, q) in enumerate(zip(sa.params, sb.params)):
        if i == sa.no_g:
            continue
        if not torch.equal(p, q) or any(not torch.equal(oa.state[p][k], ob.state[q][k]) for k in keys if k in oa.state[p]):
            return False
        if set(oa.state[p]) - {"ema"} != set(ob.state[q]) - {"ema"}:
            return False
    return True


def test_adamw_without_decay_is_adam_without_decay():
    sa, oa, _ = _run("adamw", 2, check=False, weight_decay=0.0, max_grad_norm=1.0)
    sb, ob, _ = _run("adam", 2, check=False, weight_decay=0.0, max_grad_norm=1.0)
    assert _same(sa, oa, sb, ob)


@pytest.mark.parametrize("kind", KINDS)
def test_ema_and_guard_leave_the_plain_step_bit_for_bit(kind):
    sa, oa, _ = _run(kind, 3, check=False)
    sb, ob, _ = _run(kind, 3, check=False, ema_decay=0.9, skip_nonfinite=True)
    assert _same(sa, oa, sb, ob) and ob.skipped_steps == 0
    assert all("ema" not in oa.state[p] for p in sa.params)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_native_path_against_the_torch_op_path(kind):
    """Both on the device, stepped from the same fp32 inputs every time: within the sum of the two bounds."""
    kw = dict(ema_decay=0.9, skip_nonfinite=True, max_grad_norm=1.0)
    sa, sb = _ExtSet(4), _ExtSet(4)
    oa, ob = _make(kind, sa, **kw), _make(kind, sb, torch_path=True, **kw)
    ra, rb = ext.Recorder(kind, oa), ext.Recorder(kind, ob)
    worst = 0.0
    for step in range(2):
        sa.new_grads()
        sb.new_grads()
        assert all(torch.equal(p.grad, q.grad) for p, q in zip(sa.params, sb.params) if p.grad is not None)
        norm = ref.global_norm([p.grad for p in sa.params if p.grad is not None])
        coef = ref.clip_coef(norm, 1.0)
        xa, xb = ra.before(sa.params), rb.before(sb.params)
        oa.step()
        ob.step()
        ra.check(sa.params, xa, coef=coef)
        rb.check(sb.params, xb, coef=coef)
        worst = max(worst, ref.compare(ra, sa.params, xa, rb, sb.params, xb, coef_a=coef, coef_b=coef))
        with torch.no_grad():
            for p, q in zip(sa.params, sb.params):
                q.copy_(p)
                for k, v in oa.state.get(p, {}).items():
                    if k != "step":
                        ob.state[q][k].copy_(v)
    assert (oa.native_steps, oa.torch_steps, ob.native_steps, ob.torch_steps) == (2, 0, 0, 2) and sa.guards_intact()
    print("%s native against torch ops: worst distance / allowed %.3g (bounds: %s, %s)" % (kind, worst, ra.worst, rb.worst))


@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("case", ["nan", "inf", "huge"])
@pytest.mark.parametrize("kind", KINDS)
def test_guard(kind, case, clip):
    """The scenario of tests/test_optim_ext.py::test_guard on the device, the gradients rewritten in place so that the job
    table can stay: it must, across the skipped step.  Poisoned: a 4-element tensor and the misaligned parameter."""
    s = _ExtSet(5)
    opt = _make(kind, s, ema_decay=0.9, skip_nonfinite=True, max_grad_norm=clip, zero_grads=(case == "inf"))
    rec = ext.Recorder(kind, opt)
    tables = []

    def fresh(scale):
        tables.append(opt._table)
        s.fill_grads(scale)

    worst = ext.guard_case(opt, rec, s.params, fresh, case, poison=(3, s.mis_p))
    torch.cuda.synchronize()
    assert opt.native_steps == 3 and opt.torch_steps == 0 and s.guards_intact()
    # tables[2]: what the poisoned step left; the next step ran on that very table
    assert tables[2] is not None and opt._table is tables[2]
    assert kind == "sgd" or tables[1] is tables[2]           # (SGD's first table went with its first-step flags)
    print("%s guard %s clip %s: worst error / bound %s" % (kind, case, clip, worst))


def test_guard_on_the_very_first_step_keeps_sgd_first_step_semantics():
    """The skipped step wrote no momentum buffer: the table keeps its first-step bits and the next step spends them."""
    s = _ExtSet(6)
    opt = _make("sgd", s, ema_decay=0.9, skip_nonfinite=True)
    tables = []

    def fresh(scale):
        tables.append(opt._table)
        s.fill_grads(scale)

    ext.guard_case(opt, ext.Recorder("sgd", opt), s.params, fresh, "nan", poison=(3, s.mis_p), first=True)
    assert opt.native_steps == 2 and tables[1] is not None and tables[1].first_step and s.guards_intact()


def test_grad_norms_against_the_host():
    s = _ExtSet(7)
    opt = _make("adamw", s, max_grad_norm=1e4)
    s.new_grads()
    opt.step()
    got = opt.grad_norms()
    want = np.array([np.sqrt((ref.f64(p.grad) ** 2).sum()) for p in opt._table.params])
    assert got.dtype == torch.float64 and got.device == s.params[0].device and got.shape == (len(want),)
    assert [id(p) for p in opt._table.params] == [id(p) for g in opt.param_groups for p in g["params"] if p.grad is not None]
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-12, atol=0)
    assert opt.nonfinite_parameters() == []


def test_train_steps_with_ema_shadows_and_swap():
    """RubiksNet-Tiny, batch 1, two dp.train_step with AdamW + EMA + guard + clipping: every shadow follows the fp64 recursion
    over the recorded parameters within ema_stage's bound; under swap_ema the model scores the averaged weights, and the live
    logits come back bit for bit."""
    torch.manual_seed(5)
    net = RubiksNet("tiny", 11, num_frames=8, verbose=False).to(DEV)
    opt = dp.make_optimizer(net, lr=1e-2, lr_shift_mult=0.1, kind="hip_adamw", weight_decay=1e-2, ema_decay=0.9,
                            skip_nonfinite=True, max_grad_norm=20.0)
    clips, labels = torch.randn(1, 8, 3, 224, 224, device=DEV), torch.randint(0, 11, (1,), device=DEV)
    params = [p for p in net.parameters()]
    shadow = [ref.f64(p) for p in params]                    # e0 = p0
    worst = 0.0
    for step in range(2):
        loss = dp.train_step(net, opt, clips, labels)
        assert np.isfinite(float(loss.detach()))
        for i, p in enumerate(params):
            want, bound = ext.ema_stage(shadow[i], p, 0.9)
            worst = max(worst, ref.ratio(opt.state[p]["ema"], want, bound))
            shadow[i] = ref.f64(opt.state[p]["ema"])
    assert worst <= 1.0, worst
    assert type(opt) is optim.RubiksAdamW and opt.native_steps == 2 and opt.torch_steps == 0 and opt.skipped_steps == 0
    assert np.isfinite(float(opt.last_grad_norm)) and len(opt.ema_parameters()) == len(params)
    net.eval()
    with torch.no_grad():
        live = net(clips).clone()
        ptrs = [p.data_ptr() for p in params]
        with opt.swap_ema():
            assert all(p.data_ptr() != a for p, a in zip(params, ptrs))
            averaged = net(clips).clone()
        back = net(clips).clone()
    assert [p.data_ptr() for p in params] == ptrs
    assert torch.isfinite(averaged).all() and not torch.equal(live, averaged) and torch.equal(live, back)
    print("ema shadows of a Tiny train run: worst error / bound %.3g; |live - averaged| max %.3g" %
          (worst, float((live - averaged).abs().max())))
