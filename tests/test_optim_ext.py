"""RubiksAdamW, the EMA shadow and the non-finite guard of rubiksnet_amd.optim without a device: the torch-op path (what CPU
parameters get) against the fp64 stages and bounds of tests/_optim_ext_ref.py and against torch.optim.AdamW, the bit-equality
statements that tie the extensions to the plain optimizers, dp.make_optimizer's new kind and keywords, and the argument
checks of rk_optim_step_ext_f32.  Tests that measure print the worst error as a multiple of its bound."""
import copy
import ctypes
import math

import pytest
import torch

import _optim_ext_ref as ext
import _optim_ref as ref
from rubiksnet_amd import _native, dp, optim

SGD_GROUP_CASES = [dict(momentum=0.9, dampening=0.0, nesterov=True), dict(momentum=0.0), dict(momentum=0.8, dampening=0.3)]
KINDS = ["sgd", "adam", "adamw"]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (0, 1, 3, 5, 257, 1000)] + \
           [torch.nn.Parameter(torch.randn(6, 7, generator=g))]


def _set_grads(params, seed, scale=1.0, skip=()):
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(params):
        p.grad = None if i in skip else torch.randn(p.shape, generator=g) * scale


def _groups(params, policy=True):
    if policy:
        return [{"params": params[0::3], "lr": 0.05, "weight_decay": 1e-2, "lr_mult": 0.1, "decay_mult": 0.0},
                {"params": params[1::3], "lr_mult": 3.0, "decay_mult": 2.0},
                {"params": params[2::3]}]
    return [{"params": params[0::3], "lr": 0.05, "weight_decay": 1e-2}, {"params": params[1::3]}, {"params": params[2::3]}]


def _make(kind, params, policy=True, **kw):
    groups = _groups(params, policy)
    if kind == "sgd":
        for g, case in zip(groups, SGD_GROUP_CASES):
            g.update(case)
        return optim.RubiksSGD(groups, lr=0.1, weight_decay=5e-3, **kw)
    if kind == "adam":
        return optim.RubiksAdam(groups, lr=1e-2, weight_decay=kw.pop("weight_decay", 5e-3), eps=1e-8, **kw)
    return optim.RubiksAdamW(groups, lr=1e-2, weight_decay=kw.pop("weight_decay", 5e-2), eps=1e-8, **kw)


def _states_equal(oa, a, ob, b, keys):
    return all(torch.equal(p, q) and all(torch.equal(oa.state[p][k], ob.state[q][k]) for k in keys if k in oa.state[p])
               and float(oa.state[p].get("step", 0)) == float(ob.state[q].get("step", 0)) for p, q in zip(a, b))


def test_adamw_three_steps_against_fp64():
    params = _params(1)
    opt = _make("adamw", params)
    assert "RubiksAdamW" in optim.__all__ and opt.defaults["weight_decay"] == 5e-2
    assert optim.RubiksAdamW([torch.nn.Parameter(torch.zeros(1))]).defaults["weight_decay"] == 1e-2
    rec = ext.Recorder("adamw", opt)
    for step in range(3):
        _set_grads(params, 10 + step, skip=(4,) if step == 0 else ())
        snap = rec.before(params)
        opt.step()
        rec.check(params, snap)
        for group in opt.param_groups:
            group["lr"] *= 0.7
    assert opt.torch_steps == 3 and opt.native_steps == 0
    assert all(set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq"} for p in params)
    assert not torch.equal(params[5], _params(1)[5])
    print("adamw worst error / bound: %s" % rec.worst)


def test_adamw_against_torch_optim():
    """lr_mult = decay_mult = 1: torch.optim.AdamW's rule.  torch's own result is held to the reference and its bound
    (rb.check), and the two results to the sum of the bounds (ref.compare), stepped from the same fp32 inputs every time."""
    mine, theirs = _params(2), _params(2)
    opt = _make("adamw", mine, False)
    top = torch.optim.AdamW(_groups(theirs, False), lr=1e-2, weight_decay=5e-2, eps=1e-8)
    ra, rb = ext.Recorder("adamw", opt), ext.Recorder("adamw", top)
    worst = 0.0
    for step in range(3):
        _set_grads(mine, 20 + step)
        _set_grads(theirs, 20 + step)
        sa, sb = ra.before(mine), rb.before(theirs)
        opt.step()
        top.step()
        ra.check(mine, sa)
        rb.check(theirs, sb)
        worst = max(worst, ref.compare(ra, mine, sa, rb, theirs, sb))
        with torch.no_grad():
            for a, b in zip(mine, theirs):
                b.copy_(a)
                for k, v in opt.state[a].items():
                    if k != "step":
                        top.state[b][k].copy_(v)
    print("adamw worst distance to torch.optim.AdamW / allowed: %.3g (own bounds: %s, torch's: %s)" % (worst, ra.worst, rb.worst))


def test_adamw_state_dict_round_trips_with_torch():
    mine, theirs, back = _params(3), _params(3), _params(3)
    opt, again = _make("adamw", mine, False), _make("adamw", back, False)
    top = torch.optim.AdamW(_groups(theirs, False), lr=1e-2, weight_decay=5e-2, eps=1e-8)
    for step in range(2):
        _set_grads(mine, 30 + step)
        opt.step()
    sd = opt.state_dict()
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values()) and len(sd["state"]) == len(mine)
    top.load_state_dict(copy.deepcopy(sd))                     # ours -> torch
    with torch.no_grad():
        for a, b in zip(mine, theirs):
            b.copy_(a)
    ra, rb = ext.Recorder("adamw", opt), ext.Recorder("adamw", top)
    _set_grads(mine, 40)
    _set_grads(theirs, 40)
    sa, sb = ra.before(mine), rb.before(theirs)
    assert [b["t"] for b in sb] == [2] * len(theirs)
    opt.step()
    top.step()
    ra.check(mine, sa)
    w1 = ref.compare(ra, mine, sa, rb, theirs, sb)
    again.load_state_dict(copy.deepcopy(top.state_dict()))     # torch -> ours
    with torch.no_grad():
        for a, b in zip(theirs, back):
            b.copy_(a)
    rc = ext.Recorder("adamw", again)
    _set_grads(theirs, 41)
    _set_grads(back, 41)
    sb, sc = rb.before(theirs), rc.before(back)
    assert [b["t"] for b in sc] == [3] * len(back)
    top.step()
    again.step()
    rc.check(back, sc)
    w2 = ref.compare(rc, back, sc, rb, theirs, sb)
    print("adamw: distance to torch.optim.AdamW after a state_dict hand-over / allowed: %.3g, and back: %.3g" % (w1, w2))


def test_adamw_without_decay_is_adam_without_decay():
    a, b = _params(4), _params(4)
    oa, ob = _make("adamw", a, weight_decay=0.0, max_grad_norm=0.5), _make("adam", b, weight_decay=0.0, max_grad_norm=0.5)
    for step in range(3):
        _set_grads(a, 50 + step)
        _set_grads(b, 50 + step)
        oa.step()
        ob.step()
        assert _states_equal(oa, a, ob, b, ("exp_avg", "exp_avg_sq"))


@pytest.mark.parametrize("kind", KINDS)
def test_ema_and_guard_leave_the_plain_step_bit_for_bit(kind):
    """Finite gradients: p and every torch-named state equal the plain optimizer's bits; the shadow follows ema_stage,
    also through a change of ema_decay; no "ema" key without ema_decay."""
    a, b = _params(5), _params(5)
    oa, ob = _make(kind, a), _make(kind, b, ema_decay=0.9, skip_nonfinite=True)
    rec = ext.Recorder(kind, ob)
    start = [p.detach().clone() for p in b]
    for step in range(3):
        _set_grads(a, 60 + step)
        _set_grads(b, 60 + step)
        snap = rec.before(b)
        oa.step()
        ob.step()
        assert "ema" in rec.check(b, snap)
        assert _states_equal(oa, a, ob, b, ("momentum_buffer", "exp_avg", "exp_avg_sq"))
        if step == 0:                                          # e0 = the parameter before its first step
            d = torch.tensor(0.9)
            want = [(s * d + p.detach() * (1 - 0.9)) for s, p in zip(start, b)]
            assert all(torch.equal(ob.state[p]["ema"], w) for p, w in zip(b, want))
        ob.ema_decay = 0.5 if step == 0 else 0.99              # a schedule: read at every step
    assert all("ema" not in oa.state[p] for p in a) and all("ema" in ob.state[p] for p in b)
    assert [e.shape for e in ob.ema_parameters()] == [p.shape for g in ob.param_groups for p in g["params"]]
    assert oa.ema_parameters() == [None] * len(a) and ob.skipped_steps == 0
    if kind == "sgd":                                          # torch's layout besides: a buffer where the group has momentum
        assert all(("momentum_buffer" in ob.state[p]) == (g["momentum"] != 0) for g in ob.param_groups for p in g["params"])
    print("%s + EMA + guard: worst error / bound %s" % (kind, rec.worst))


def test_swap_ema_exchanges_and_restores():
    params = _params(6)
    opt = _make("adamw", params, ema_decay=0.5)
    for step in range(2):
        _set_grads(params, 70 + step)
        opt.step()
    live = [(p.data_ptr(), p.detach().clone()) for p in params]
    shadow = [(opt.state[p]["ema"].data_ptr(), opt.state[p]["ema"].clone()) for p in params]
    opt._table = object()
    with opt.swap_ema() as inside:
        assert inside is opt and opt._table is None
        for p, (lp, lv), (sp, sv) in zip(params, live, shadow):
            assert p.data_ptr() == sp and torch.equal(p, sv) and isinstance(p, torch.nn.Parameter)
            assert opt.state[p]["ema"].data_ptr() == lp and torch.equal(opt.state[p]["ema"], lv)
        assert any(not torch.equal(lv, sv) for (_, lv), (_, sv) in zip(live, shadow))
        opt._table = object()
    assert opt._table is None
    for p, (lp, lv), (sp, sv) in zip(params, live, shadow):
        assert p.data_ptr() == lp and torch.equal(p, lv)
        assert opt.state[p]["ema"].data_ptr() == sp and torch.equal(opt.state[p]["ema"], sv)
    with pytest.raises(KeyError):                              # an exception inside still swaps back
        with opt.swap_ema():
            raise KeyError("x")
    assert all(p.data_ptr() == lp for p, (lp, _) in zip(params, live))


@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("case", ["nan", "inf", "huge"])
@pytest.mark.parametrize("kind", KINDS)
def test_guard(kind, case, clip):
    params = _params(7)
    opt = _make(kind, params, ema_decay=0.9, skip_nonfinite=True, max_grad_norm=clip, zero_grads=(case == "inf"))
    seeds = iter(range(80, 90))
    worst = ext.guard_case(opt, ext.Recorder(kind, opt), params, lambda scale: _set_grads(params, next(seeds), scale), case)
    assert opt.torch_steps == 3
    print("%s guard %s clip %s: worst error / bound %s" % (kind, case, clip, worst))


def test_guard_on_the_very_first_step_keeps_sgd_first_step_semantics():
    params = _params(8)
    opt = _make("sgd", params, skip_nonfinite=True)
    seeds = iter(range(90, 99))
    ext.guard_case(opt, ext.Recorder("sgd", opt), params, lambda scale: _set_grads(params, next(seeds), scale), "nan", first=True)


def test_without_the_guard_a_nan_still_poisons_and_nothing_counts():
    params = _params(9)
    opt = _make("adamw", params, max_grad_norm=1.0)
    _set_grads(params, 99)
    with torch.no_grad():
        params[3].grad[1] = math.nan
    opt.step()
    assert all(bool(p.detach().isnan().all()) for p in params if p.numel()) and opt.skipped_steps == 0
    assert [id(p) for p in opt.nonfinite_parameters()] == [id(params[3])]


def test_make_optimizer_new_kind_and_keywords():
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2))
    net[0].register_parameter("shift", torch.nn.Parameter(torch.zeros(2, 4)))
    new = dp.make_optimizer(net, lr=0.1, lr_shift_mult=0.5, kind="hip_adamw", weight_decay=0.02, max_grad_norm=2.0, ema_decay=0.9,
                            skip_nonfinite=True)
    assert type(new) is optim.RubiksAdamW and new.max_grad_norm == 2.0 and new.ema_decay == 0.9 and new.skip_nonfinite
    assert [(g["lr"], g["lr_mult"], g["weight_decay"]) for g in new.param_groups] == [(0.1, 0.5, 0.02), (0.1, 1.0, 0.02)]
    for kind, cls in (("hip_sgd", optim.RubiksSGD), ("hip_adam", optim.RubiksAdam)):
        o = dp.make_optimizer(net, kind=kind, ema_decay=0.99, skip_nonfinite=True)
        assert type(o) is cls and o.ema_decay == 0.99 and o.skip_nonfinite
        o = dp.make_optimizer(net, kind=kind)
        assert o.ema_decay is None and not o.skip_nonfinite
    for kind in ("adam", "sgd"):
        with pytest.raises(ValueError):
            dp.make_optimizer(net, kind=kind, ema_decay=0.9)
        with pytest.raises(ValueError):
            dp.make_optimizer(net, kind=kind, skip_nonfinite=True)
    with pytest.raises(ValueError):
        optim.RubiksAdamW(net.parameters(), ema_decay=1.5)


def test_ext_abi_argument_checks_without_a_device():
    L = _native.lib()
    fn = L.rk_optim_step_ext_f32
    one, odd, inf = ctypes.c_void_p(16), ctypes.c_void_p(20), math.inf
    assert ctypes.sizeof(optim._AdamWHyper) == 32
    for rule, rec in ((0, optim._SgdHyper), (1, optim._AdamHyper), (2, optim._AdamWHyper)):
        hyper = (rec * 9)()
        assert fn(rule, None, 1, 1, hyper, 1, None, 0, 0.0, None, 0, None, 0.0, 0.0, 0, None, None) == -1
        assert fn(rule, one, 1, 1, None, 1, None, 0, 0.0, None, 0, None, 0.0, 0.0, 0, None, None) == -1
        assert fn(rule, one, 0, 1, hyper, 1, None, 0, 0.0, None, 0, None, 0.0, 0.0, 0, None, None) == -2
        assert fn(rule, one, 1, 1, hyper, 0, None, 0, 0.0, None, 0, None, 0.0, 0.0, 0, None, None) == -2
        assert fn(rule, one, 1, 1, hyper, 9, None, 0, 0.0, None, 0, None, 0.0, 0.0, 0, None, None) == -7      # a ninth group
        assert fn(rule, one, 1, 1, hyper, 1, None, 0, inf, None, 0, None, 0.0, 0.0, 1, one, None) == -4       # guard, no partials
        assert fn(rule, one, 1, 1, hyper, 1, one, 1, inf, None, 0, None, 0.0, 0.0, 1, None, None) == -1       # guard, no counter
        assert fn(rule, one, 1, 1, hyper, 1, one, 1, inf, None, 0, None, 0.0, 0.0, 1, odd, None) == -2        # misaligned counter
        assert fn(rule, one, 1, 1, hyper, 1, None, 0, 0.0, None, 0, odd, 0.9, 0.1, 0, None, None) == -2       # misaligned shadows
        assert fn(rule, one, 1, 1, hyper, 1, odd, 1, 1.0, None, 0, None, 0.0, 0.0, 0, None, None) == -2       # misaligned partials
        assert fn(rule, one, 1, 0, hyper, 8, one, 1, inf, None, 0, one, 0.9, 0.1, 1, one, None) == 0          # no chunk: no launch
    for rule in (-1, 3):                                                                                      # unknown rule
        assert fn(rule, one, 1, 1, (optim._AdamHyper * 1)(), 1, None, 0, 0.0, None, 0, None, 0.0, 0.0, 0, None, None) == -7
