"""RubiksShift3D on 16-bit activations next to an fp32 shift table (rk3d_*_sf32): everything that needs no device -- the
exported symbols, argument validation, the workspace size, the planner's 16-bit branch (rk_debug_3d_plan, elem_size 2), the
routing predicate rk3d_sf32_streams and the RK_SHIFT3D_16 switch."""
import ctypes

import pytest

from rubiksnet_amd import _native, config

NEW = ("rk3d_forward_bf16_sf32", "rk3d_forward_f16_sf32", "rk3d_backward_bf16_sf32", "rk3d_backward_f16_sf32",
       "rk3d_sf32_streams")

# (N, T, C, H, W), stride, padding -- the shapes of tests/test_shift3d16_gpu.py
STREAM = [((2, 3, 8, 14, 14), (1, 1, 1), (0, 0, 0)),
          ((1, 8, 16, 7, 7), (1, 1, 1), (0, 0, 0)),
          ((2, 4, 3, 56, 56), (1, 1, 1), (0, 0, 0)),
          ((3, 5, 10, 28, 28), (1, 1, 1), (0, 0, 0)),       # ragged last channel group
          ((1, 1, 4, 14, 14), (1, 1, 1), (0, 0, 0)),        # a walk of one plane
          ((2, 9, 6, 12, 16), (1, 1, 1), (0, 0, 0)),
          ((1, 3, 2, 72, 64), (1, 1, 1), (0, 0, 0))]        # a plane split into 2 bands of 36 rows (the networks: 112x112)
BANDS = {(1, 3, 2, 72, 64): 2}
GENERIC = [((2, 8, 6, 28, 28), (1, 2, 2), (0, 0, 0)),       # the networks' down-sampling form
           ((2, 3, 5, 9, 11), (1, 2, 2), (0, 1, 1)),
           ((1, 4, 3, 10, 7), (2, 1, 3), (1, 2, 0)),
           ((1, 2, 3, 5, 5), (1, 1, 1), (0, 0, 0))]         # 50-byte planes: no 16-byte slabs

K_FINALIZE = 18                                             # plan3d::Family (rk3d_plan.hpp); the 16-bit families follow it
GEN16 = {19, 20, 21}                                        # kGen16Fwd, kGen16BwdX, kGen16BwdS
STREAM16 = {22, 23}                                         # kStream16Fwd, kStream16Bwd


def plan(form, dims, s, p, quantize=0, gx=1, gshift=1, two_phase=0, aligned=15, elem=2):
    """(rc, launches as (family, grid), P, separate finalize)"""
    out = (ctypes.c_int * 30)()
    rc = _native.lib().rk_debug_3d_plan(form, elem, *dims, *s, *p, quantize, gx, gshift, two_phase, aligned, 0, -1, out)
    o = list(out)
    return rc, [(o[3 + 9 * i], o[3 + 9 * i + 6]) for i in range(o[0])], o[1], o[2]


def test_symbols():
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name


@pytest.mark.parametrize("sfx", ["bf16_sf32", "f16_sf32"])
def test_validation_without_a_device(sfx):
    L = _native.lib()
    fwd, bwd = getattr(L, "rk3d_forward_" + sfx), getattr(L, "rk3d_backward_" + sfx)
    one = ctypes.c_void_p(16)     # non-NULL dummy; never dereferenced on these paths
    dims, s1, p0 = (2, 8, 4, 6, 6), (1, 1, 1), (0, 0, 0)
    assert fwd(None, one, one, *dims, *s1, *p0, 0, None) == -1
    assert fwd(one, None, one, *dims, *s1, *p0, 0, None) == -1
    assert fwd(one, one, one, 0, 8, 4, 6, 6, *s1, *p0, 0, None) == -2
    assert fwd(one, one, one, *dims, 1, 0, 1, *p0, 0, None) == -3
    assert fwd(one, one, one, *dims, *s1, 0, -1, 0, 0, None) == -3
    assert bwd(None, one, one, one, one, *dims, *s1, *p0, 1, 1.0, 0, one, 1 << 20, None) == -1     # gshift needs x
    assert bwd(one, None, one, one, one, *dims, *s1, *p0, 1, 1.0, 0, one, 1 << 20, None) == -1
    assert bwd(one, one, one, one, one, 0, 8, 4, 6, 6, *s1, *p0, 1, 1.0, 0, one, 1 << 20, None) == -2
    assert bwd(one, one, one, one, one, *dims, 0, 1, 1, *p0, 1, 1.0, 0, one, 1 << 20, None) == -3
    assert bwd(one, one, one, one, one, *dims, *s1, *p0, 1, 1.0, 0, None, 0, None) == -4
    need = L.rk3d_backward_workspace_bytes(*dims, *s1, *p0, 2)
    assert need > 0 and bwd(one, one, one, one, one, *dims, *s1, *p0, 1, 1.0, 0, one, need - 1, None) == -4
    assert bwd(one, one, one, None, None, *dims, *s1, *p0, 1, 1.0, 0, one, 1 << 20, None) == -1


def test_workspace():
    L = _native.lib()
    assert L.rk3d_backward_workspace_bytes(2, 3, 8, 14, 14, 1, 1, 1, 0, 0, 0, 2) == 8 * 3 * (2 * 14) * 4
    # the pinned sizes of the other element sizes (tests/test_abi.py) are untouched
    assert L.rk3d_backward_workspace_bytes(32, 8, 64, 56, 56, 1, 1, 1, 0, 0, 0, 4) == 64 * 3 * 32 * 56 * 16
    assert L.rk3d_backward_workspace_bytes(32, 8, 64, 56, 56, 1, 1, 1, 0, 0, 0, 8) == 64 * 3 * 32 * 56 * 8
    for dims, s, p in STREAM + GENERIC:
        for aligned in (15, 14):
            rc, launches, P, fin = plan(1, dims, s, p, aligned=aligned)
            assert rc == 0 and P > 0 and fin == 1
            assert dims[2] * 3 * P * 4 <= L.rk3d_backward_workspace_bytes(*dims, *s, *p, 2), (dims, s, p)


@pytest.mark.parametrize("dims,s,p", STREAM)
def test_planner_streaming_shapes(dims, s, p):
    N, T, C = dims[:3]
    bands = BANDS.get(dims, 1)
    rc, launches, P, fin = plan(0, dims, s, p)
    assert rc == 0 and [f for f, _ in launches] == [22] and P == 0 and fin == 0
    rc, launches, P, fin = plan(1, dims, s, p)
    assert rc == 0 and [f for f, _ in launches] == [23, K_FINALIZE] and P == N * bands and fin == 1
    assert launches[1][1] == C                              # one finalize workgroup per channel
    rc, launches, P, fin = plan(1, dims, s, p, gshift=0)    # d(x) alone: no finalize
    assert rc == 0 and [f for f, _ in launches] == [23] and P == 0 and fin == 0
    rc, launches, P, fin = plan(1, dims, s, p, gx=0)
    assert rc == 0 and [f for f, _ in launches] == [23, K_FINALIZE] and P == N * bands
    # x not 16-byte aligned: the generic family
    rc, launches, P, fin = plan(0, dims, s, p, aligned=14)
    assert rc == 0 and [f for f, _ in launches] == [19]
    rc, launches, P, fin = plan(1, dims, s, p, aligned=14)
    assert rc == 0 and [f for f, _ in launches] == [20, 21, K_FINALIZE] and P == N * T and fin == 1
    # quantize: the generic family
    rc, launches, _, _ = plan(0, dims, s, p, quantize=1)
    assert rc == 0 and [f for f, _ in launches] == [19]
    assert _native.lib().rk3d_sf32_streams(*dims, *s, *p, 0, 2) == 1
    assert _native.lib().rk3d_sf32_streams(*dims, *s, *p, 1, 2) == 0
    assert _native.lib().rk3d_sf32_streams(*dims, *s, *p, 0, 4) == 0


@pytest.mark.parametrize("dims,s,p", GENERIC)
def test_planner_generic_shapes(dims, s, p):
    N, T, C = dims[:3]
    To = _native.lib().rk_out_len(T, s[0], p[0])
    for q in (0, 1):
        rc, launches, P, fin = plan(0, dims, s, p, quantize=q)
        assert rc == 0 and [f for f, _ in launches] == [19]
        rc, launches, P, fin = plan(1, dims, s, p, quantize=q)
        assert rc == 0 and [f for f, _ in launches] == [20, 21, K_FINALIZE] and P == N * To and fin == 1
    rc, launches, P, fin = plan(1, dims, s, p, gshift=0)
    assert rc == 0 and [f for f, _ in launches] == [20] and P == 0 and fin == 0
    assert _native.lib().rk3d_sf32_streams(*dims, *s, *p, 0, 2) == 0


def test_planner_new_families_and_unsupported_forms():
    seen = set()
    for dims, s, p in STREAM + GENERIC:
        for form in (0, 1):
            for aligned in (15, 14):
                seen |= {f for f, _ in plan(form, dims, s, p, aligned=aligned)[1]}
    assert seen == GEN16 | STREAM16 | {K_FINALIZE}
    assert all(f > K_FINALIZE for f in seen - {K_FINALIZE})
    dims, s, p = STREAM[0]
    assert plan(2, dims, s, p)[0] == -7                     # no BatchNorm-fused forms
    assert plan(3, dims, s, p)[0] == -7
    assert plan(1, dims, s, p, two_phase=1)[0] == -7        # no two-phase form
    # the fp32 plan of the same call does not know the new families
    assert all(f <= K_FINALIZE for f, _ in plan(1, dims, s, p, elem=4)[1])


def test_predicate_follows_the_planner():
    L = _native.lib()
    for dims, s, p in STREAM + GENERIC + [((2, 8, 8, 112, 112), (1, 1, 1), (0, 0, 0)), ((2, 8, 7, 7, 7), (1, 1, 1), (0, 0, 0))]:
        for q in (0, 1):
            streams = plan(0, dims, s, p, quantize=q)[1][0][0] in STREAM16
            assert L.rk3d_sf32_streams(*dims, *s, *p, q, 2) == int(streams), (dims, s, p, q)
    assert L.rk3d_sf32_streams(0, 8, 8, 14, 14, 1, 1, 1, 0, 0, 0, 0, 2) == 0      # invalid dimensions: no


def test_switch():
    assert config.Switches().shift3d_16 is True
    assert config.reload({}).shift3d_16 is True
    assert config.reload({"RK_SHIFT3D_16": "0"}).shift3d_16 is False
    assert config.reload({"RK_SHIFT3D_16": "1"}).shift3d_16 is True
    assert dataclass_fields()[-1] == "shift3d_16"


def dataclass_fields():
    import dataclasses

    return [f.name for f in dataclasses.fields(config.Switches)]
