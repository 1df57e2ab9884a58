"""RubiksShift3D on bf16 / f16 activations next to an fp32 shift table (rk3d_*_sf32, rubiksnet_cuda.rubiks_shift_3d_*_sf32).

y and d(x) are the fp32 oracle on the widened inputs with the UNROUNDED shift, cast to the storage type, bit for bit (quantize
included); d(shift) comes back in fp32 at the accuracy the project asks of fp32-accumulated d(shift) (tests/test_parity_3d.py,
rk2d_*_sf32 in tests/test_parity_2d.py)."""
import os

import numpy as np
import pytest
import torch

from _util import DEV, rand, seed_of, special_shifts
from test_shift3d16 import GENERIC, STREAM

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
KINDS = ["generic", "wide", "integer", "half", "oob", "tiny"]
_cache = {}


def fwd(x, shift, s, p, q, y=None):
    from rubiksnet_amd import _native, rubiksnet_cuda

    if y is None:
        L = _native.lib()
        N, T, C, H, W = x.shape
        y = torch.empty((N, L.rk_out_len(T, s[0], p[0]), C, L.rk_out_len(H, s[1], p[1]), L.rk_out_len(W, s[2], p[2])),
                        dtype=x.dtype, device=x.device)
    assert rubiksnet_cuda.rubiks_shift_3d_forward_sf32(x, shift, s, p, q, y) == 0
    return y


def bwd(x, shift, gy, s, p, q, normalize=False, t_factor=1.0, want_gx=True, want_gs=True, gx=None):
    from rubiksnet_amd import rubiksnet_cuda

    if want_gx and gx is None:
        gx = torch.empty_like(x)
    gs = torch.empty_like(shift) if want_gs else None
    assert rubiksnet_cuda.rubiks_shift_3d_backward_sf32(x, shift, gy, s, p, gx if want_gx else None, gs, normalize, t_factor, q) == 0
    return gx, gs


def case(oracle, cfg, kind, dtype):
    """Inputs of one case and their oracle results, computed once: x, shift, gy (host tensors; x / gy in the storage type) and
    {quantize: (y_ref, gx_ref)} in fp32, the raw fp64 d(shift)."""
    key = (cfg, kind, dtype)
    if key not in _cache:
        dims, s, p = cfg
        C = dims[2]
        rng = np.random.default_rng(seed_of(cfg, kind, str(dtype), "rk3d_sf32"))
        x = torch.from_numpy(rand(rng, dims, np.float32)).to(dtype)
        sf = special_shifts(rng, 3, C, np.float32, kind)
        if kind == "generic":
            sf[0, 0], sf[1, 0] = 0.4990234375, -0.5009765625      # fp32 != their bf16 / f16 roundings (0.5 / -0.5)
        xf = x.float().numpy()
        refs = {}
        gy = None
        for q in (False, True):
            y_ref = oracle.rk3d_forward(xf, sf, s, p, q)
            if gy is None:
                gy = torch.from_numpy(rand(rng, y_ref.shape, np.float32)).to(dtype)
            gx_ref, _ = oracle.rk3d_backward(gy.float().numpy(), xf, sf, s, p, normalize_grad=False, quantize=q)
            refs[q] = (y_ref, gx_ref)
        _cache[key] = (x, torch.from_numpy(sf), gy, refs)
    return _cache[key]


def gshift_ref(oracle, x, shift, gy, s, p, normalize, t_factor):
    return oracle.rk3d_backward(gy.float().numpy().astype(np.float64), x.float().numpy().astype(np.float64),
                                shift.numpy().astype(np.float64), s, p, normalize_grad=normalize,
                                normalize_t_factor=t_factor)[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg", STREAM + GENERIC, ids=lambda c: "x".join(map(str, c[0])) + ("s" + "".join(map(str, c[1]))))
def test_bit_exact_and_raw_shift_gradient(oracle, cfg, kind, dtype):
    dims, s, p = cfg
    x, shift, gy, refs = case(oracle, cfg, kind, dtype)
    xd, sd, gd = x.to(DEV), shift.to(DEV), gy.to(DEV)
    gs_ref = gshift_ref(oracle, x, shift, gy, s, p, False, 1.0)
    bound = 1e-5 * max(1.0, float(np.abs(gs_ref).max()))
    for q in (False, True):
        y_ref, gx_ref = refs[q]
        y = fwd(xd, sd, s, p, q)
        assert y.dtype == dtype and torch.equal(y.cpu(), torch.from_numpy(y_ref).to(dtype)), "forward quantize=%s" % q
        gx, gs = bwd(xd, sd, gd, s, p, q)
        assert gx.dtype == dtype and torch.equal(gx.cpu(), torch.from_numpy(gx_ref).to(dtype)), "d(x) quantize=%s" % q
        assert gs.dtype == torch.float32
        err = float(np.abs(gs.cpu().numpy() - gs_ref).max())
        print("d(shift) raw: max err %.3g, bound %.3g (quantize=%s)" % (err, bound, q))
        assert err <= bound, (err, bound, q)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("t_factor", [1.0, 0.25, -1.0])
@pytest.mark.parametrize("cfg", [STREAM[0], GENERIC[0]], ids=["stream", "generic"])
def test_normalised_shift_gradient(oracle, cfg, t_factor, dtype):
    dims, s, p = cfg
    for kind in ("generic", "integer"):
        x, shift, gy, _ = case(oracle, cfg, kind, dtype)
        _, gs = bwd(x.to(DEV), shift.to(DEV), gy.to(DEV), s, p, False, normalize=True, t_factor=t_factor)
        ref = gshift_ref(oracle, x, shift, gy, s, p, True, t_factor)
        err = float(np.abs(gs.cpu().numpy() - ref).max())
        print("d(shift) normalised: max err %.3g (%s)" % (err, kind))
        np.testing.assert_allclose(gs.cpu().numpy(), ref, rtol=0, atol=2e-5)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("cfg", [STREAM[0], STREAM[3], STREAM[6], GENERIC[1]], ids=["stream", "ragged", "bands", "generic"])
def test_one_gradient_only(oracle, cfg, dtype):
    dims, s, p = cfg
    x, shift, gy, _ = case(oracle, cfg, "integer", dtype)
    xd, sd, gd = x.to(DEV), shift.to(DEV), gy.to(DEV)
    for q in (False, True):
        gx, gs = bwd(xd, sd, gd, s, p, q, normalize=True)
        _, gs1 = bwd(xd, sd, gd, s, p, q, normalize=True, want_gx=False)
        gx1, none = bwd(xd, sd, gd, s, p, q, normalize=True, want_gs=False)
        assert none is None and torch.equal(gs1, gs) and torch.equal(gx1, gx)


def guarded(t, sentinel):
    """A copy of `t` as a view one element into a larger buffer (2-byte aligned), the rest filled with the sentinel."""
    buf = torch.full((t.numel() + 9,), sentinel, dtype=t.dtype, device=DEV)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 2 and view.is_contiguous()
    return buf, view


def untouched(buf, n, sentinel):
    return bool((buf[:1] == sentinel).all() and (buf[1 + n:] == sentinel).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("cfg", [STREAM[0], STREAM[1], STREAM[3], STREAM[6], GENERIC[0]],
                         ids=["14x14", "7x7", "ragged", "bands", "stride2"])
def test_misaligned_views(oracle, cfg, dtype):
    """x, y, gy and gx one element into a larger buffer: y and d(x) are the aligned run's bits, the guard elements stay."""
    dims, s, p = cfg
    x, shift, gy, _ = case(oracle, cfg, "generic", dtype)
    sd = shift.to(DEV)
    y0 = fwd(x.to(DEV), sd, s, p, False)
    gx0, gs0 = bwd(x.to(DEV), sd, gy.to(DEV), s, p, False)
    S = 777.0
    xb, xv = guarded(x, S)
    gb, gv = guarded(gy, S)
    yb, yv = guarded(torch.zeros_like(y0), S)
    ob, ov = guarded(torch.zeros_like(gx0), S)
    fwd(xv, sd, s, p, False, y=yv)
    gx1, gs1 = bwd(xv, sd, gv, s, p, False, gx=ov)
    assert torch.equal(yv, y0) and torch.equal(ov, gx0)
    # d(shift) is no view and, behind a 2-byte aligned x, comes from the generic family: another fp32 summation order than
    # the streaming family's, so it is held to the bound of the raw d(shift) check, not to the aligned run's bits
    gs_ref = gshift_ref(oracle, x, shift, gy, s, p, False, 1.0)
    assert float(np.abs(gs1.cpu().numpy() - gs_ref).max()) <= 1e-5 * max(1.0, float(np.abs(gs_ref).max()))
    if cfg in GENERIC:
        assert torch.equal(gs1, gs0)
    assert untouched(xb, x.numel(), S) and untouched(gb, gy.numel(), S)
    assert untouched(yb, y0.numel(), S) and untouched(ob, gx0.numel(), S)


def test_native_node_against_the_cast_path():
    from rubiksnet_amd import config
    from rubiksnet_amd.shiftlib import RubiksShift3D

    torch.manual_seed(3)
    mod = RubiksShift3D(8).to(DEV)
    x0 = torch.randn(2, 4, 8, 14, 14, device=DEV).to(torch.bfloat16)
    gy = torch.randn(2, 4, 8, 14, 14, device=DEV).to(torch.bfloat16)
    runs = {}
    try:
        for on in ("1", "0"):
            config.reload(dict(os.environ, RK_SHIFT3D_16=on))
            x = x0.clone().requires_grad_(True)
            mod.shift.grad = None
            saved = []
            with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append((t.dtype, t.numel())), t)[1], lambda t: t):
                y = mod(x)
            y.backward(gy)
            runs[on] = (y.detach(), x.grad, mod.shift.grad.clone(), type(y.grad_fn).__name__, saved)
    finally:
        config.reload()
    y1, gx1, gs1, node1, saved1 = runs["1"]
    y0, gx0, gs0, node0, saved0 = runs["0"]
    assert "RubiksShift3D16" in node1 and "RubiksShift3D16" not in node0
    assert (torch.float32, x0.numel()) not in saved1 and (torch.float32, x0.numel()) in saved0
    assert y1.dtype == torch.bfloat16 and gx1.dtype == torch.bfloat16 and gs1.dtype == torch.float32
    assert torch.equal(y1, y0) and torch.equal(gx1, gx0)
    assert float((gs1 - gs0).abs().max()) <= 2e-5


def test_model_trains_on_the_native_node():
    from rubiksnet_amd import RubiksNet, config, dp
    from rubiksnet_amd.shiftlib import RubiksShift3D

    torch.manual_seed(0)
    net = RubiksNet("tiny", 6, verbose=False).to(DEV)
    opt = dp.make_optimizer(net, lr=1e-3)
    clips = torch.randn(1, 8, 3, 224, 224, device=DEV)
    labels = torch.tensor([2], device=DEV)
    nodes = []

    def hook(mod, inp, out):
        nodes.append((tuple(mod.stride), inp[0].dtype, type(out.grad_fn).__name__))

    hs = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, RubiksShift3D)]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = dp.train_step(net, opt, clips, labels)
    for h in hs:
        h.remove()
    assert torch.isfinite(loss)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    stride1 = [n for n in nodes if n[0] == (1, 1, 1)]
    assert len(stride1) >= 9 and len(stride1) < len(nodes)
    assert all(dt == torch.bfloat16 and "RubiksShift3D16" in name for _, dt, name in stride1), stride1

    net.eval()
    logits = {}
    try:
        for on in ("1", "0"):
            config.reload(dict(os.environ, RK_SHIFT3D_16=on))
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                logits[on] = net(clips).float()
    finally:
        config.reload()
    assert torch.equal(logits["1"], logits["0"])
