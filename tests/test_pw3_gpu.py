"""The per-CU fp32 1x1 GEMM of the 257..288-row layers (rk_pw3.hip) where its column ranges do not end on frames, against
fp64 on the device, through the public entry points only (rk_pw_gemm_f32, rk_pw_gemm_fused_f32, rk_pw_gemm_stats_f32,
rk_pw_gemm_bnbwd_f32).  Reference semantics: rubiksnet/backbone.py:44-45 (Conv1x1), :123-135 (the block around it).

Each geometry class is found at run time: the first frame count, counting up, that the planner (rk_debug_pw_gemm_plan with
this device's CU count and this process's RK_PW2/3/4) gives to rk_pw3.hip with the wanted property -- a range that straddles
frames, a last workgroup without a second column half (a statistics record with n = 0), a last workgroup of a few columns,
the widest range, planes much shorter than a range, two launch rounds, 17 row blocks with a partial one, fewer reduction
stages than the LDS ring has.  tests/test_pw3_geometry.py holds the classes and checks the kernel's addresses for them without
a device.

Per call: Y (prefilled with NaN) whole against fp64 within 4e-6 sqrt(K) max|ref|; Y, the statistics records and the
BatchNorm-backward records sit between 64 sentinel floats that must survive; every record is compared on its own; a second
call gives the same bits.

Bounds of the per-tile sums (u = 2^-24, a tile has at most 112 columns = 7 per lane of a 16-lane row): s1 = sum(y - pivot) is
one rounded subtraction per term, at most 7 sequential additions in a lane and 4 across lanes, s2 = sum((y - pivot)^2) squares
the rounded difference (2 u) inside 7 fused multiply-adds and 4 additions: at most 12 / 13 roundings on any path, so
|error| <= 16 u sum|term| with the terms formed in fp64 from the stored Y.  The BatchNorm-backward pair: sum(dz) adds stored
values (at most 11 roundings), sum(dz xhat) rounds xhat = (x - mean) invstd twice before 7 fused multiply-adds and 4
additions: the same 16 u sum|term|."""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import test_pw3_geometry as geo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENT = -7777.25                                 # the guard bands' value
GUARD = 64
U16 = 16 * 2.0 ** -24

# name -> (a_is_mk, prologue, epilogue): the six instances of k_pw3_gemm
INSTANCES = {
    "mk-plain": (1, 0, 0), "mk-pro": (1, 1, 0), "mk-stats": (1, 0, 1), "mk-pro-stats": (1, 1, 1),
    "km-plain": (0, 0, 0), "km-bnbwd": (0, 0, 2),
}
FULL = ("control", "straddle", "empty-half")
CASES = [(c, i, r) for c in FULL for i in INSTANCES for r in (0, 1)]
CASES += [(c, i, 1) for c in sorted(geo.classes()) if c not in FULL for i in ("mk-pro-stats", "km-bnbwd")]
OFFSET_CASE = ("straddle", "mk-stats", 1)       # residual of 300 +- 0.5: the statistics' pivot matters


def _native():
    from rubiksnet_amd import _native
    return _native, _native.lib()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _modes():
    return tuple(int(os.environ.get(k, "1") or 0) for k in ("RK_PW2", "RK_PW3", "RK_PW4"))


@functools.lru_cache(maxsize=None)
def _shape(name):
    P, K, M, want = geo.classes(_cus())[name]
    found = geo.search(P, K, M, want, cus=_cus(), modes=_modes())
    assert found, "no frame count gives rk_pw3.hip the geometry %r at %d CUs" % (name, _cus())
    F, cw, nwg, last = found
    return F, K, M, P, cw, nwg, last


def bn_inputs(name, F, M, P):
    """the BatchNorm-backward epilogue's x and (a, b, mean, invstd), from the host generator: the mask is the same everywhere"""
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) + 1)
    bx = torch.randn(F, M, P, generator=g)
    pack = torch.stack([torch.rand(M, generator=g) + 0.5, torch.randn(M, generator=g) * 0.3, torch.randn(M, generator=g) * 0.1,
                        torch.rand(M, generator=g) + 0.5], dim=1).contiguous()
    return bx, pack


_cache = {}


def _inputs(name):
    """operands of a geometry, made once on the device and never written; one geometry is kept at a time"""
    if _cache.get("name") != name:
        _cache.clear()
        F, K, M, P, cw, nwg, last = _shape(name)
        g = torch.Generator(device=DEV).manual_seed(zlib.crc32(name.encode()))
        d = {"name": name}
        d["x"] = torch.randn(F, K, P, device=DEV, generator=g)
        d["r"] = torch.randn(F, M, P, device=DEV, generator=g)
        d["w"] = torch.randn(M, K, device=DEV, generator=g) / K ** 0.5
        d["wt"] = d["w"].t().contiguous()
        d["ka"] = torch.rand(K, device=DEV, generator=g) + 0.5
        d["kb"] = torch.randn(K, device=DEV, generator=g) * 0.3
        _cache.update(d)
    return _cache


def _product(name, pro):
    """fp64 A pro(X), [F, M, P], shared by the calls of a geometry"""
    d = _inputs(name)
    key = "ref%d" % pro
    if key not in d:
        K = d["x"].shape[1]
        xin = d["x"].double()
        if pro:
            xin = (xin * d["ka"].double().view(1, K, 1) + d["kb"].double().view(1, K, 1)).clamp_min_(0)
        d[key] = torch.matmul(d["w"].double(), xin)
    return d[key]


def _bn(name):
    d = _inputs(name)
    if "bx" not in d:
        F, K, M, P = _shape(name)[:4]
        bx, pack = bn_inputs(name, F, M, P)
        d["bx"], d["pack"] = bx.to(DEV), pack.to(DEV)
    return d["bx"], d["pack"]


def _guarded(n, fill):
    buf = torch.full((n + 2 * GUARD,), SENT, device=DEV)
    body = buf[GUARD:GUARD + n]
    body.fill_(fill)
    assert body.data_ptr() % 16 == 0
    return buf, body


def _guards_intact(buf):
    s = torch.full((GUARD,), SENT, device=DEV)
    return torch.equal(buf[:GUARD], s) and torch.equal(buf[-GUARD:], s)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _tiles(F, P, cw, nwg):
    """first column and column count of tile 2 wg + cs, and the tile of every column"""
    ntot = F * P
    c0 = np.repeat(np.arange(nwg, dtype=np.int64) * cw, 2)
    ncols = np.minimum(c0 + cw, ntot) - c0
    cs = np.tile([0, 1], nwg)
    first = c0 + 112 * cs
    n = np.where(cs == 0, np.minimum(ncols, 112), np.maximum(ncols - 112, 0))
    col = np.arange(ntot, dtype=np.int64)
    tile_of = 2 * (col // cw) + (col % cw >= 112)
    return (torch.from_numpy(first).to(DEV), torch.from_numpy(n).to(DEV), torch.from_numpy(tile_of).to(DEV))


def _call(name, inst, res, r):
    """one guarded call: (Y buffer, Y, record buffer or None, records or None)"""
    native, L = _native()
    F, K, M, P, cw, nwg, last = _shape(name)
    a_is_mk, pro, epi = INSTANCES[inst]
    d = _inputs(name)
    # the plan of exactly this call
    out = geo.plan(F, K, M, P, a_is_mk=a_is_mk, epi=epi, res=res, pro=pro, modes=_modes(), cus=_cus())
    assert out[:4] == (0, 3, cw, nwg), out
    A = d["w"] if a_is_mk else d["wt"]
    J = 2 * nwg
    if epi:
        assert out[4] == J == int(L.rk_pw_gemm_tiles(A.data_ptr(), F, K, M, P, a_is_mk))
    st = torch.cuda.current_stream().cuda_stream
    ybuf, y = _guarded(F * M * P, float("nan"))
    rp = r.data_ptr() if res else None
    ka, kb = (d["ka"].data_ptr(), d["kb"].data_ptr()) if pro else (None, None)
    x = d["x"]
    recbuf = rec = None
    if epi == 1:
        recbuf, rec = _guarded(M * J * 4, float("nan"))
        native.check(L.rk_pw_gemm_stats_f32(A.data_ptr(), x.data_ptr(), rp, y.data_ptr(), F, K, M, P, 1, ka, kb, 1, rec.data_ptr(), J,
                                            st), "rk_pw_gemm_stats_f32")
    elif epi == 2:
        bx, pack = _bn(name)
        recbuf, rec = _guarded(M * J * 2, float("nan"))
        native.check(L.rk_pw_gemm_bnbwd_f32(A.data_ptr(), x.data_ptr(), rp, y.data_ptr(), F, K, M, P, 0, bx.data_ptr(), pack.data_ptr(),
                                            rec.data_ptr(), J, st), "rk_pw_gemm_bnbwd_f32")
    elif pro:
        native.check(L.rk_pw_gemm_fused_f32(A.data_ptr(), x.data_ptr(), rp, y.data_ptr(), F, K, M, P, 1, ka, kb, 1, None, None, 0, st),
                     "rk_pw_gemm_fused_f32")
    else:
        native.check(L.rk_pw_gemm_f32(A.data_ptr(), x.data_ptr(), rp, y.data_ptr(), F, K, M, P, a_is_mk, st), "rk_pw_gemm_f32")
    return ybuf, y, recbuf, rec


@pytest.mark.parametrize("name,inst,res", CASES, ids=["%s-%s-%s" % (c, i, "res" if r else "nores") for c, i, r in CASES])
def test_instance_on_geometry(name, inst, res):
    native, L = _native()
    F, K, M, P, cw, nwg, last = _shape(name)
    a_is_mk, pro, epi = INSTANCES[inst]
    d = _inputs(name)
    J, ntot = 2 * nwg, F * P
    r = d["r"] * 0.5 + 300.0 if (name, inst, res) == OFFSET_CASE else d["r"]

    ybuf, y, recbuf, rec = _call(name, inst, res, r)
    ref = _product(name, pro)
    if res:
        ref = ref + r.double()
    worst = {}
    got = y.view(F, M, P).double()
    if epi == 2:
        bx, pack = _bn(name)
        pa, pb, mu, iv = (pack[:, i].double().view(1, M, 1) for i in range(4))
        pre = pa * bx.double() + pb                  # the kernel tests fmaf(a, x, b) <= 0: the sign of the exact value
        near = pre.abs() < 1e-12
        left_out = int(near.sum())
        assert left_out <= 1e-6 * near.numel(), left_out
        scale_y = float(ref.abs().max())
        ref = ref * (pre > 0)
        err = torch.where(near, torch.zeros_like(got), (got - ref).abs())
        assert not bool(torch.isnan(got).any())
    else:
        scale_y = float(ref.abs().max())
        err = (got - ref).abs()                      # NaN where the kernel stored nothing
    err = float(torch.nan_to_num(err, nan=float("inf")).max())
    worst["y"] = err / (4e-6 * K ** 0.5 * scale_y)
    del ref, err

    assert _guards_intact(ybuf), "Y's guard bands"
    if epi:
        assert _guards_intact(recbuf), "the records' guard bands"
        assert bool(torch.isfinite(rec).all()), "a record is unwritten or not finite"
        first, n, tile_of = _tiles(F, P, cw, nwg)
        assert int(n.sum()) == ntot and int(n[-1]) == max(last - 112, 0)
        cols = got.permute(1, 0, 2).reshape(M, ntot)          # the stored Y, [row][column]
        has = n > 0

    def tile_sums(v):                                           # fp64 sums of v [M, ntot] over each tile's own columns
        return torch.zeros(M, J, dtype=torch.float64, device=DEV).index_add_(1, tile_of, v)

    if epi == 1:
        s = rec.view(M, J, 4)
        assert torch.equal(s[:, :, 3].double(), n.double().view(1, J).expand(M, J)), "n of a tile"
        piv_y = cols[:, torch.where(has, first, torch.zeros_like(first))].float()
        assert _same_bits(s[:, :, 0][:, has].contiguous(), piv_y[:, has].contiguous()), "pivot != stored Y at the tile's first column"
        empty = s[:, ~has, :]
        assert bool((empty[:, :, 1:3] == 0).all()), "s1, s2 of a tile without columns"
        t = cols - s[:, :, 0].double()[:, tile_of]
        e1 = (s[:, :, 1].double() - tile_sums(t)).abs()
        e2 = (s[:, :, 2].double() - tile_sums(t * t)).abs()
        b1, b2 = U16 * tile_sums(t.abs()), U16 * tile_sums(t * t)
        worst["s1"] = float((e1 / b1.clamp_min(1e-300))[:, has].max()) if bool(has.any()) else 0.0
        worst["s2"] = float((e2 / b2.clamp_min(1e-300))[:, has].max()) if bool(has.any()) else 0.0
        del t, e1, e2, b1, b2
        out = torch.empty(4, M, device=DEV)
        gamma, beta = torch.ones(M, device=DEV), torch.zeros(M, device=DEV)
        native.check(L.rk_bn_finish_tiles_f32(s.data_ptr(), J, ntot, gamma.data_ptr(), beta.data_ptr(), None, None, out[0].data_ptr(),
                                              out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None, M, 1e-5, 0.1, None,
                                              torch.cuda.current_stream().cuda_stream), "rk_bn_finish_tiles_f32")
        mean, var = cols.mean(dim=1), cols.var(dim=1, unbiased=False)
        worst["mean"] = float((out[0].double() - mean).abs().max()) / (1e-6 * max(1.0, float(mean.abs().max())))
        invstd = 1.0 / torch.sqrt(var + 1e-5)
        worst["invstd"] = float(((out[1].double() - invstd).abs() / invstd).max()) / 3e-5
    elif epi == 2:
        b = rec.view(M, J, 2).double()
        assert bool((b[:, ~has, :] == 0).all()), "sums of a tile without columns"
        xhat = ((bx.double() - mu) * iv).permute(1, 0, 2).reshape(M, ntot)
        dx = cols * xhat
        scale = float(cols.abs().sum(dim=1).max())
        worst["sum dz"] = float((b[:, :, 0].sum(1) - cols.sum(dim=1)).abs().max()) / (2e-6 * scale)
        worst["sum dz xhat"] = float((b[:, :, 1].sum(1) - dx.sum(dim=1)).abs().max()) / (2e-5 * scale)
        e1 = (b[:, :, 0] - tile_sums(cols)).abs()
        e2 = (b[:, :, 1] - tile_sums(dx)).abs()
        b1, b2 = U16 * tile_sums(cols.abs()), U16 * tile_sums(dx.abs())
        worst["tile dz"] = float((e1 / b1.clamp_min(1e-300))[:, has].max())
        worst["tile dz xhat"] = float((e2 / b2.clamp_min(1e-300))[:, has].max())
        del xhat, dx, e1, e2, b1, b2

    # determinism: a second call, into fresh buffers, gives the same bits
    ybuf2, y2, recbuf2, rec2 = _call(name, inst, res, r)
    assert _same_bits(y, y2), "Y differs between two calls"
    if epi:
        assert _same_bits(rec, rec2), "the records differ between two calls"

    print("pw3 %s %s res=%d: F %d cw %d nwg %d last %d; error / bound: %s"
          % (name, inst, res, F, cw, nwg, last, ", ".join("%s %.3f" % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v <= 1.0, (k, v)
