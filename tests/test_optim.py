"""rubiksnet_amd.optim without a device: the chunk partition of rk_optim.hip, the C ABI's argument checks, and the torch-op
path of RubiksSGD / RubiksAdam (what CPU parameters get) against the fp64 reference of tests/_optim_ref.py and against
torch.optim.  Every test prints the worst observed error as a multiple of its bound."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import _optim_ref as ref
from rubiksnet_amd import RubiksNet, _native, dp, optim

CHUNK = 4096
NUMELS = [0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]


def _owners(numels, chunk, chunks, offsets):
    """How often each element of each tensor is visited when chunk b goes to the LAST record with chunk0 <= b (the
    kernel's search) and covers [(b - chunk0) chunk, min(numel, ... + chunk))."""
    seen = [np.zeros(n, dtype=np.int64) for n in numels]
    for b in range(chunks):
        j = max(i for i, c in enumerate(offsets) if c <= b)
        lo = (b - offsets[j]) * chunk
        assert lo < numels[j], "chunk %d starts past its tensor" % b
        seen[j][lo:min(numels[j], lo + chunk)] += 1
    return seen


@pytest.mark.parametrize("numels", [NUMELS, NUMELS[::-1], [0, 0, 5, 0], [CHUNK, 0, CHUNK]] + [[n] for n in NUMELS],
                         ids=lambda v: "x".join(map(str, v)))
def test_chunk_partition(numels):
    chunk, chunks, offsets = optim.chunk_partition(numels)
    assert chunk == CHUNK
    per = [-(-n // chunk) for n in numels]
    assert offsets == [sum(per[:i]) for i in range(len(numels))] and chunks == sum(per)
    for n, s in zip(numels, _owners(numels, chunk, chunks, offsets)):
        assert s.shape == (n,) and (s == 1).all()


def test_abi_argument_checks_without_a_device():
    L = _native.lib()
    one = ctypes.c_void_p(16)
    out = (ctypes.c_int * 3)()
    assert L.rk_debug_optim_chunks(None, 1, out) == -1
    assert L.rk_debug_optim_chunks((ctypes.c_longlong * 1)(-1), 1, out) == -2
    assert L.rk_debug_optim_chunks((ctypes.c_longlong * 1)(CHUNK * (2 ** 31)), 1, out) == -2
    assert L.rk_optim_sqnorm_workspace_bytes(0) == 0 and L.rk_optim_sqnorm_workspace_bytes(7) == 56
    assert L.rk_optim_sqnorm_many_f32(one, 1, 1, None, None) == -4
    for name, rec in (("rk_optim_sgd_many_f32", optim._SgdHyper), ("rk_optim_adam_many_f32", optim._AdamHyper)):
        fn, hyper = getattr(L, name), (rec * 9)()
        assert fn(None, 1, 1, hyper, 1, None, 0, 0.0, None, 0, None) == -1
        assert fn(one, 1, 1, None, 1, None, 0, 0.0, None, 0, None) == -1
        assert fn(one, 0, 1, hyper, 1, None, 0, 0.0, None, 0, None) == -2
        assert fn(one, 1, 1, hyper, 9, None, 0, 0.0, None, 0, None) == -7          # a ninth group: nothing launched
        assert fn(one, 1, 0, hyper, 8, None, 0, 0.0, None, 0, None) == 0           # no chunk: nothing to launch
    assert ctypes.sizeof(optim._SgdHyper) == 20 and ctypes.sizeof(optim._AdamHyper) == 32


def _params(seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g, dtype=dtype)) for n in (0, 1, 3, 5, 257, 1000)] + \
           [torch.nn.Parameter(torch.randn(6, 7, generator=g, dtype=dtype))]


def _set_grads(params, seed, skip=()):
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(params):
        p.grad = None if i in skip else torch.randn(p.shape, generator=g, dtype=p.dtype)


def _groups(params, policy):
    if policy:
        return [{"params": params[0::3], "lr": 0.05, "weight_decay": 1e-2, "lr_mult": 0.1, "decay_mult": 0.0},
                {"params": params[1::3], "lr_mult": 3.0, "decay_mult": 2.0},
                {"params": params[2::3]}]
    return [{"params": params[0::3], "lr": 0.05, "weight_decay": 1e-2}, {"params": params[1::3]}, {"params": params[2::3]}]


SGD_CASES = {"plain": dict(momentum=0.0), "momentum": dict(momentum=0.9), "dampening": dict(momentum=0.8, dampening=0.3),
             "nesterov": dict(momentum=0.9, nesterov=True)}


def _make(kind, params, policy, case=None, **kw):
    if kind == "sgd":
        return optim.RubiksSGD(_groups(params, policy), lr=0.1, weight_decay=5e-3, **dict(SGD_CASES[case], **kw))
    return optim.RubiksAdam(_groups(params, policy), lr=1e-2, weight_decay=5e-3, eps=1e-8, **kw)


def _make_torch(kind, params, case=None):
    if kind == "sgd":
        return torch.optim.SGD(_groups(params, False), lr=0.1, weight_decay=5e-3, **SGD_CASES[case])
    return torch.optim.Adam(_groups(params, False), lr=1e-2, weight_decay=5e-3, eps=1e-8)


@pytest.mark.parametrize("kind,case", [("sgd", c) for c in SGD_CASES] + [("adam", None)])
def test_cpu_path_three_steps_against_fp64(kind, case):
    params = _params(1)
    opt = _make(kind, params, True, case)
    rec = ref.Recorder(kind, opt)
    for step in range(3):
        _set_grads(params, 10 + step, skip=(4,) if step == 0 else ())      # (one tensor meets its first step later)
        snap = rec.before(params)
        opt.step()
        rec.check(params, snap)
        for group in opt.param_groups:
            group["lr"] *= 0.7
    assert opt.torch_steps == 3 and opt.native_steps == 0
    print("%s/%s worst error / bound: %s" % (kind, case, rec.worst))


@pytest.mark.parametrize("kind,case", [("sgd", c) for c in SGD_CASES] + [("adam", None)])
def test_cpu_path_against_torch_optim(kind, case):
    """lr_mult = decay_mult = 1: the same rule as torch.optim's, so the two stay within twice the bound of each other, stepped
    from the same fp32 inputs every time (the twin is re-seeded with our result after each step)."""
    mine, theirs = _params(2), _params(2)
    opt, top = _make(kind, mine, False, case), _make_torch(kind, theirs, case)
    ra, rb = ref.Recorder(kind, opt), ref.Recorder(kind, top)
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
    print("%s/%s worst distance to torch.optim / allowed: %.3g (own bounds: %s, torch's: %s)" % (kind, case, worst, ra.worst, rb.worst))


def test_get_optim_policy_is_honoured():
    """get_optim_policy() fed directly: shifts move by lr * shift_lr_mult * g, BatchNorm parameters and biases see no decay,
    weights do."""
    torch.manual_seed(0)
    policy = RubiksNet("tiny", num_classes=7, num_frames=8, verbose=False).backbone.get_optim_policy(shift_lr_mult=0.25)
    names = {g["name"]: g for g in policy}
    assert set(names) == {"weight", "bias", "bn", "shift"} and all(names[k]["params"] for k in ("weight", "bn", "shift"))
    lr, wd = 0.5, 0.125
    for cls, kw in ((optim.RubiksSGD, dict(momentum=0.0)), (optim.RubiksAdam, dict())):
        members = {k: [p for p in g["params"]] for k, g in names.items()}
        with torch.no_grad():
            for k, ps in members.items():
                for p in ps:
                    p.copy_(torch.rand_like(p) + 0.5)
                    p.grad = torch.ones_like(p) if k == "shift" else torch.zeros_like(p)
        before = {k: [p.detach().clone() for p in ps] for k, ps in members.items()}
        opt = cls([dict(g) for g in policy], lr=lr, weight_decay=wd, **kw)
        opt.step()
        for k in ("bn", "bias"):                                   # zero gradient, no decay: untouched, exactly
            assert all(torch.equal(p, b) for p, b in zip(members[k], before[k])), k
        assert all(not torch.equal(p, b) for p, b in zip(members["weight"], before["weight"]))     # decay alone moves them
        for p, b in zip(members["shift"], before["shift"]):
            if cls is optim.RubiksSGD:                             # g = 1, no decay: p - lr * shift_lr_mult, one rounding
                np.testing.assert_allclose(p.detach().numpy(), b.numpy() - lr * 0.25, rtol=2 * ref.U, atol=0)
            else:                                                  # Adam's first step is lr_eff * g / (|g| + eps)
                np.testing.assert_allclose(p.detach().numpy(), b.numpy() - lr * 0.25, rtol=1e-6, atol=0)
        if cls is optim.RubiksSGD:
            for p, b in zip(members["weight"], before["weight"]):
                np.testing.assert_allclose(p.detach().numpy(), (b.double() * (1 - lr * wd)).numpy(), rtol=4 * ref.U, atol=0)


@pytest.mark.parametrize("kind,case", [("sgd", "momentum"), ("adam", None)])
def test_state_dict_round_trips_with_torch(kind, case):
    mine, theirs, back = _params(3), _params(3), _params(3)
    opt, top, again = _make(kind, mine, False, case), _make_torch(kind, theirs, case), _make(kind, back, False, case)
    keys = {"sgd": {"momentum_buffer"}, "adam": {"step", "exp_avg", "exp_avg_sq"}}[kind]
    for step in range(2):
        _set_grads(mine, 30 + step)
        opt.step()
    sd = opt.state_dict()
    assert all(set(s) == keys for s in sd["state"].values()) and len(sd["state"]) == len(mine)
    top.load_state_dict(copy.deepcopy(sd))                     # ours -> torch (a copy, as a saved file is: load_state_dict keeps the tensors it is given)
    with torch.no_grad():
        for a, b in zip(mine, theirs):
            b.copy_(a)
    ra, rb = ref.Recorder(kind, opt), ref.Recorder(kind, top)
    _set_grads(mine, 40)
    _set_grads(theirs, 40)
    sa, sb = ra.before(mine), rb.before(theirs)
    assert [b["t"] for b in sb] == [2 if kind == "adam" else 0] * len(theirs)
    opt.step()
    top.step()
    ra.check(mine, sa)
    w1 = ref.compare(ra, mine, sa, rb, theirs, sb)
    again.load_state_dict(copy.deepcopy(top.state_dict()))     # torch -> ours
    with torch.no_grad():
        for a, b in zip(theirs, back):
            b.copy_(a)
    rc = ref.Recorder(kind, again)
    _set_grads(theirs, 41)
    _set_grads(back, 41)
    sb, sc = rb.before(theirs), rc.before(back)
    top.step()
    again.step()
    rc.check(back, sc)
    w2 = ref.compare(rc, back, sc, rb, theirs, sb)
    print("%s: distance to torch.optim after a state_dict hand-over / allowed: %.3g, and back: %.3g" % (kind, w1, w2))


@pytest.mark.parametrize("kind,case", [("sgd", "momentum"), ("adam", None)])
@pytest.mark.parametrize("max_norm", [0.5, 1e3], ids=["clipping", "not-clipping"])
def test_max_grad_norm_matches_clip_grad_norm(kind, case, max_norm):
    """Against torch.nn.utils.clip_grad_norm_ + torch.optim's step.  torch forms the norm in fp32 (ours: fp64): its coefficient
    may be off by the rounding of a sum of N squares, so the twin's gradient term is referenced with ITS coefficient -- read
    back from the gradients it scaled -- and the comparison allows the distance of the two references."""
    mine, theirs = _params(4), _params(4)
    opt, top = _make(kind, mine, False, case, max_grad_norm=max_norm), _make_torch(kind, theirs, case)
    ra, rb = ref.Recorder(kind, opt), ref.Recorder(kind, top)
    for step in range(2):
        _set_grads(mine, 50 + step)
        _set_grads(theirs, 50 + step)
        norm = ref.global_norm([p.grad for p in mine])
        coef = ref.clip_coef(norm, max_norm)
        assert (coef < 1.0) == (max_norm < 1.0)
        sa, sb = ra.before(mine), rb.before(theirs)            # (the twin's snapshot holds the UNclipped gradients)
        total = torch.nn.utils.clip_grad_norm_(theirs, max_norm)
        coef_t = min(1.0, max_norm / (float(total) + 1e-6))
        assert abs(float(total) - norm) <= 1e-6 * norm and abs(coef_t - coef) <= 1e-6 * coef
        opt.step()
        top.step()
        assert abs(float(opt.last_grad_norm) - norm) <= 1e-6 * norm
        ra.check(mine, sa, coef=coef)
        w = ref.compare(ra, mine, sa, rb, theirs, sb, coef_a=coef, coef_b=coef_t)
        with torch.no_grad():
            for a, b in zip(mine, theirs):
                b.copy_(a)
                for k, v in opt.state[a].items():
                    if k != "step":
                        top.state[b][k].copy_(v)
    print("%s max_norm %g: worst / bound %s, distance to clip_grad_norm_ + torch.optim / allowed %.3g" % (kind, max_norm, ra.worst, w))


def test_zero_grads_option_on_the_cpu_path():
    a, b = _params(5), _params(5)
    oa, ob = _make("sgd", a, True, "nesterov"), _make("sgd", b, True, "nesterov", zero_grads=True)
    for step in range(2):
        _set_grads(a, 60 + step)
        _set_grads(b, 60 + step)
        oa.step()
        ob.step()
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        assert all(not q.grad.any() for q in b) and any(p.grad.any() for p in a)


def test_make_optimizer_kinds():
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2))
    net[0].register_parameter("shift", torch.nn.Parameter(torch.zeros(2, 4)))
    assert type(dp.make_optimizer(net)) is torch.optim.Adam                      # the default and the old kinds: as before
    assert type(dp.make_optimizer(net, kind="adam")) is torch.optim.Adam
    old = dp.make_optimizer(net, lr=0.1, lr_shift_mult=0.5, kind="sgd", momentum=0.8, weight_decay=0.01)
    assert type(old) is torch.optim.SGD and [g["lr"] for g in old.param_groups] == [0.05, 0.1]
    with pytest.raises(ValueError):
        dp.make_optimizer(net, kind="sgd", max_grad_norm=1.0)
    new = dp.make_optimizer(net, lr=0.1, lr_shift_mult=0.5, kind="hip_sgd", momentum=0.8, weight_decay=0.01, max_grad_norm=2.0)
    assert type(new) is optim.RubiksSGD and new.max_grad_norm == 2.0
    assert [(g["lr"], g["lr_mult"], g["momentum"], g["weight_decay"]) for g in new.param_groups] == \
        [(0.1, 0.5, 0.8, 0.01), (0.1, 1.0, 0.8, 0.01)]
    assert [len(g["params"]) for g in new.param_groups] == [len(g["params"]) for g in old.param_groups] == [1, 4]
    adam = dp.make_optimizer(net, lr=0.1, lr_shift_mult=0.5, kind="hip_adam")
    assert type(adam) is optim.RubiksAdam and adam.max_grad_norm is None and adam.param_groups[0]["lr_mult"] == 0.5
