"""The stride (1,2,2) streaming family of RubiksShift3D on bf16 / f16 activations next to an fp32 shift table (rk3d_16.hpp).

y and d(x) are the fp32 oracle on the widened inputs with the UNROUNDED shift, cast to the storage type, bit for bit; d(shift)
comes back in fp32 within the bounds tests/test_shift3d16_gpu.py holds the stride-1 family to.  The shapes the family does not
take run through the same entry points and are held to the same bits."""
import os

import numpy as np
import pytest
import torch

from _util import DEV, rand, seed_of, special_shifts
from test_shift3d16_gpu import bwd, fwd, gshift_ref, guarded, untouched
from test_shift3d16_s2 import NOT_TAKEN, P0, S2, STREAM_S2, WO12

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
KINDS = ["generic", "wide", "integer", "half", "oob", "tiny", "parity"]
STREAMS = [(d, S2, P0) for d in STREAM_S2]
_cache = {}

# "parity": what a stride-2 window can get wrong and a stride-1 tap cannot.  (shift H, shift W) whose floors have the parities
# (even, even), (even, odd), (odd, even), (odd, odd), with both signs: a positive floor leaves the first source rows / columns
# outside every window, a negative one the last ones, and d(x) there is zero.
PARITY = [(0.3, -1.6), (-1.7, 1.4), (1.25, 2.6), (-2.4, -0.7)]


def ident(cfg):
    return "x".join(map(str, cfg[0])) + "s" + "".join(map(str, cfg[1])) + ("p" + "".join(map(str, cfg[2])) if any(cfg[2]) else "")


def shifts_of(rng, cfg, kind):
    C, H = cfg[0][2], cfg[0][3]
    if kind != "parity":
        sf = special_shifts(rng, 3, C, np.float32, kind)
        if kind == "generic":
            sf[0, 0], sf[1, 0] = 0.4990234375, -0.5009765625          # fp32 != their bf16 / f16 roundings (0.5 / -0.5)
        return sf
    sf = rng.uniform(-3.2, 3.2, (3, C)).astype(np.float32)
    sf[0] = rng.uniform(-1.5, 1.5, C)
    roll = (C + H // 8) % 4               # shapes with fewer than 4 channels start at different rows of the table
    for c in range(min(C, 4)):
        sf[1, c], sf[2, c] = PARITY[(c + roll) % 4]
    fl = np.floor(sf[1:, :min(C, 4)]).astype(int) % 2
    assert len({(a, b) for a, b in fl.T}) == min(C, 4)
    return sf


def case(oracle, cfg, kind, dtype):
    """Inputs of one case and their oracle results, computed once: x, shift, gy (host tensors; x / gy in the storage type),
    y and d(x) of the fp32 oracle, the raw d(shift) of the fp64 oracle."""
    key = (cfg, kind, dtype)
    if key not in _cache:
        dims, s, p = cfg
        rng = np.random.default_rng(seed_of(cfg, kind, str(dtype), "rk3d_sf32_s2"))
        x = torch.from_numpy(rand(rng, dims, np.float32)).to(dtype)
        sf = shifts_of(rng, cfg, kind)
        xf = x.float().numpy()
        y_ref = oracle.rk3d_forward(xf, sf, s, p, False)
        gy = torch.from_numpy(rand(rng, y_ref.shape, np.float32)).to(dtype)
        gx_ref, _ = oracle.rk3d_backward(gy.float().numpy(), xf, sf, s, p, normalize_grad=False, quantize=False)
        shift = torch.from_numpy(sf)
        _cache[key] = (x, shift, gy, y_ref, gx_ref, gshift_ref(oracle, x, shift, gy, s, p, False, 1.0))
    return _cache[key]


def check(oracle, cfg, kind, dtype):
    dims, s, p = cfg
    x, shift, gy, y_ref, gx_ref, gs_ref = case(oracle, cfg, kind, dtype)
    xd, sd, gd = x.to(DEV), shift.to(DEV), gy.to(DEV)
    y = fwd(xd, sd, s, p, False)
    assert y.dtype == dtype and torch.equal(y.cpu(), torch.from_numpy(y_ref).to(dtype)), "forward"
    gx, gs = bwd(xd, sd, gd, s, p, False)
    assert gx.dtype == dtype and torch.equal(gx.cpu(), torch.from_numpy(gx_ref).to(dtype)), "d(x)"
    assert gs.dtype == torch.float32
    bound = 1e-5 * max(1.0, float(np.abs(gs_ref).max()))
    err = float(np.abs(gs.cpu().numpy() - gs_ref).max())
    print("d(shift) raw: max err %.3g, bound %.3g" % (err, bound))
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg", STREAMS + [WO12], ids=ident)
def test_bit_exact_and_raw_shift_gradient(oracle, cfg, kind, dtype):
    from rubiksnet_amd import _native

    assert _native.lib().rk3d_sf32_streams(*cfg[0], *cfg[1], *cfg[2], 0, 2) == 1
    check(oracle, cfg, kind, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("kind", ["generic", "integer", "parity"])
@pytest.mark.parametrize("cfg", NOT_TAKEN, ids=ident)
def test_not_taken_shapes_bit_exact(oracle, cfg, kind, dtype):
    from rubiksnet_amd import _native

    assert _native.lib().rk3d_sf32_streams(*cfg[0], *cfg[1], *cfg[2], 0, 2) == 0
    check(oracle, cfg, kind, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("t_factor", [1.0, 0.25, -1.0])
@pytest.mark.parametrize("cfg", [STREAMS[0], STREAMS[4]], ids=["groups", "bands"])
def test_normalised_shift_gradient(oracle, cfg, t_factor, dtype):
    dims, s, p = cfg
    for kind in ("generic", "integer", "parity"):
        x, shift, gy = case(oracle, cfg, kind, dtype)[:3]
        _, gs = bwd(x.to(DEV), shift.to(DEV), gy.to(DEV), s, p, False, normalize=True, t_factor=t_factor)
        ref = gshift_ref(oracle, x, shift, gy, s, p, True, t_factor)
        err = float(np.abs(gs.cpu().numpy() - ref).max())
        print("d(shift) normalised: max err %.3g (%s)" % (err, kind))
        np.testing.assert_allclose(gs.cpu().numpy(), ref, rtol=0, atol=2e-5)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("kind", ["integer", "parity"])
@pytest.mark.parametrize("cfg", [STREAMS[0], STREAMS[2], STREAMS[4]], ids=["groups", "ragged", "bands"])
def test_one_gradient_only(oracle, cfg, kind, dtype):
    dims, s, p = cfg
    x, shift, gy = case(oracle, cfg, kind, dtype)[:3]
    xd, sd, gd = x.to(DEV), shift.to(DEV), gy.to(DEV)
    gx, gs = bwd(xd, sd, gd, s, p, False, normalize=True)
    _, gs1 = bwd(xd, sd, gd, s, p, False, normalize=True, want_gx=False)
    gx1, none = bwd(xd, sd, gd, s, p, False, normalize=True, want_gs=False)
    assert none is None and torch.equal(gs1, gs) and torch.equal(gx1, gx)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("cfg", [STREAMS[0], STREAMS[1], STREAMS[2], STREAMS[4]], ids=["groups", "56x56", "ragged", "bands"])
def test_misaligned_views(oracle, cfg, dtype):
    """x, y, gy and gx one element into a larger buffer: the generic family, y and d(x) are the aligned run's bits, the guard
    elements stay."""
    dims, s, p = cfg
    x, shift, gy, _, _, gs_ref = case(oracle, cfg, "parity", dtype)
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
    # d(shift) behind a 2-byte aligned x comes from the generic family, in another fp32 summation order: the raw bound
    assert float(np.abs(gs1.cpu().numpy() - gs_ref).max()) <= 1e-5 * max(1.0, float(np.abs(gs_ref).max()))
    assert untouched(xb, x.numel(), S) and untouched(gb, gy.numel(), S)
    assert untouched(yb, y0.numel(), S) and untouched(ob, gx0.numel(), S)


def test_native_node_against_the_cast_path():
    from rubiksnet_amd import config
    from rubiksnet_amd.shiftlib import RubiksShift3D

    torch.manual_seed(3)
    mod = RubiksShift3D(8, stride=(1, 2, 2)).to(DEV)
    x0 = torch.randn(2, 4, 8, 16, 16, device=DEV).to(torch.bfloat16)
    gy = torch.randn(2, 4, 8, 8, 8, device=DEV).to(torch.bfloat16)
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
    assert y1.shape == (2, 4, 8, 8, 8)
    assert y1.dtype == torch.bfloat16 and gx1.dtype == torch.bfloat16 and gs1.dtype == torch.float32
    assert torch.equal(y1, y0) and torch.equal(gx1, gx0)
    assert float((gs1 - gs0).abs().max()) <= 2e-5


def test_model_trains_with_the_large_strided_layers_on_the_native_node():
    from rubiksnet_amd import RubiksNet, config, dp
    from rubiksnet_amd.shiftlib import RubiksShift3D

    torch.manual_seed(0)
    net = RubiksNet("tiny", 6, verbose=False).to(DEV)
    opt = dp.make_optimizer(net, lr=1e-3)
    clips = torch.randn(1, 8, 3, 224, 224, device=DEV)
    labels = torch.tensor([2], device=DEV)
    nodes = []

    def hook(mod, inp, out):
        nodes.append((tuple(mod.stride), tuple(inp[0].shape[-2:]), inp[0].dtype, type(out.grad_fn).__name__))

    hs = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, RubiksShift3D)]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = dp.train_step(net, opt, clips, labels)
    for h in hs:
        h.remove()
    assert torch.isfinite(loss)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    large = [n for n in nodes if n[1] in ((112, 112), (56, 56))]
    assert {n[0] for n in large} == {(1, 1, 1), (1, 2, 2)} and {n[1] for n in large if n[0] == (1, 2, 2)} == {(112, 112), (56, 56)}
    assert all(dt == torch.bfloat16 and "RubiksShift3D16" in name for _, _, dt, name in large), large
    small = [n for n in nodes if n[0] == (1, 2, 2) and n[1] in ((28, 28), (14, 14))]
    assert {n[1] for n in small} == {(28, 28), (14, 14)}
    assert all("RubiksShift3D16" not in name for _, _, _, name in small), small

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
