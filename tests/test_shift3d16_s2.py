"""The stride (1,2,2) streaming family of RubiksShift3D on 16-bit activations (rk3d_16.hpp, geometry_s2): everything that
needs no device -- the planner's choice through rk_debug_3d_plan, the workspace bound and the routing predicate
rk3d_sf32_streams, which rubiks_shift_3d follows."""
import ctypes

import pytest

from rubiksnet_amd import _native
from test_shift3d16 import GENERIC, K_FINALIZE, STREAM

S2, P0 = (1, 2, 2), (0, 0, 0)
# (N, T, C, H, W) at stride (1,2,2), pad 0 -- the shapes of tests/test_shift3d16_s2_gpu.py
STREAM_S2 = [(2, 3, 8, 8, 16),          # several channels per group
             (1, 8, 3, 56, 56),         # the networks' 56 -> 28 form: G = 1, fewer packs than threads
             (3, 5, 10, 16, 16),        # the last channel group is ragged
             (1, 1, 4, 8, 8),           # a walk of one plane, Wo = 4
             (1, 3, 2, 72, 64),         # split into bands
             (2, 2, 2, 112, 112)]       # the networks' largest plane with its real band count
BANDS = {(1, 3, 2, 72, 64): 2, (2, 2, 2, 112, 112): 4}
# (dims, stride, padding) the family does not take
NOT_TAKEN = [((2, 8, 6, 28, 28), S2, P0),           # W % 8 != 0: the 28 -> 14 layers stay where they are
             ((2, 3, 4, 8, 12), S2, P0),            # W % 8 != 0
             ((2, 3, 4, 9, 16), S2, P0),            # odd H
             ((2, 3, 4, 8, 16), S2, (0, 1, 1)),     # padded
             ((2, 4, 4, 8, 16), (2, 2, 2), P0)]     # T-strided
# Listed with the shapes above as "Wo % 4 != 0"; but at pad 0 Wo = W / 2 = 12, so with W % 8 == 0 the condition on Wo can
# never fail and this shape has every property the family asks for.  It is kept in every check the not-taken shapes get
# that does not presuppose the answer (the predicate, the workspace, bit-exactness on the GPU).
WO12 = ((2, 3, 4, 10, 24), S2, P0)

STREAM16 = {22, 23}                     # plan3d::Family (rk3d_plan.hpp): the stride-1 streaming family; 19 .. 21 the generic one
FWD_S2, BWD_S2 = 24, 25                 # kStream16S2Fwd, kStream16S2Bwd


def plan(form, dims, s=S2, p=P0, quantize=0, gx=1, gshift=1, aligned=15, kernels=0):
    """(rc, launches as (family, variant x 5, grid), P, separate finalize)"""
    out = (ctypes.c_int * 30)()
    rc = _native.lib().rk_debug_3d_plan(form, 2, *dims, *s, *p, quantize, gx, gshift, 0, aligned, kernels, -1, out)
    o = list(out)
    return rc, [(o[3 + 9 * i], o[4 + 9 * i:9 + 9 * i], o[3 + 9 * i + 6]) for i in range(o[0])], o[1], o[2]


def families(form, dims, s=S2, p=P0, **kw):
    rc, launches, _, _ = plan(form, dims, s, p, **kw)
    assert rc == 0
    return [f for f, _, _ in launches]


@pytest.mark.parametrize("dims", STREAM_S2, ids=lambda d: "x".join(map(str, d)))
def test_planner_streaming_shapes(dims):
    N, T, C = dims[:3]
    bands = BANDS.get(dims, 1)
    rc, launches, P, fin = plan(0, dims)
    assert rc == 0 and [f for f, _, _ in launches] == [FWD_S2] and P == 0 and fin == 0
    rc, launches, P, fin = plan(1, dims)
    assert rc == 0 and [f for f, _, _ in launches] == [BWD_S2, K_FINALIZE] and P == N * bands and fin == 1
    assert launches[1][2] == C                              # one finalize workgroup per channel
    G = launches[0][1][3]
    assert launches[0][2] == N * -(-C // G) * bands         # a workgroup per clip, channel group and band
    assert bands == 1 or G == 1
    rc, launches, P, fin = plan(1, dims, gshift=0)          # d(x) alone: no finalize
    assert rc == 0 and [f for f, _, _ in launches] == [BWD_S2] and P == 0 and fin == 0
    rc, launches, P, fin = plan(1, dims, gx=0)
    assert rc == 0 and [f for f, _, _ in launches] == [BWD_S2, K_FINALIZE] and P == N * bands and fin == 1


def test_group_shapes():
    """What each streaming shape is there for, read off the plan: v[2] packs per thread, v[3] channels per group."""
    def fwd(dims):
        _, v, grid = plan(0, dims)[1][0]
        return v[3], grid

    G, grid = fwd((2, 3, 8, 8, 16))
    assert G >= 8 and grid == 2                              # all 8 channels in one group
    G, grid = fwd((1, 8, 3, 56, 56))
    assert G == 1 and grid == 3 and 28 * 28 // 4 < 256       # fewer packs than threads
    G, grid = fwd((3, 5, 10, 16, 16))
    assert 1 < G < 10 and 10 % G != 0 and grid == 3 * -(-10 // G)       # more than one group, the last one ragged
    G, grid = fwd((1, 1, 4, 8, 8))
    assert G >= 4 and grid == 1
    assert fwd((1, 3, 2, 72, 64)) == (1, 1 * 2 * 2)
    assert fwd((2, 2, 2, 112, 112)) == (1, 2 * 2 * 4)


@pytest.mark.parametrize("dims", STREAM_S2, ids=lambda d: "x".join(map(str, d)))
def test_what_sends_a_streaming_shape_to_the_generic_family(dims):
    N, T = dims[:2]
    assert families(0, dims, aligned=14) == [19]            # x not 16-byte aligned
    rc, launches, P, fin = plan(1, dims, aligned=14)
    assert rc == 0 and [f for f, _, _ in launches] == [20, 21, K_FINALIZE] and P == N * T and fin == 1
    assert families(0, dims, aligned=13) == [19]            # y
    assert families(1, dims, aligned=11) == [20, 21, K_FINALIZE]        # gx
    assert families(0, dims, quantize=1) == [19]
    assert families(1, dims, quantize=1) == [20, 21, K_FINALIZE]
    for kernels in (1, 2):                                  # RK_SHIFT_KERNELS=column, generic
        assert families(0, dims, kernels=kernels) == [19]
        assert families(1, dims, kernels=kernels) == [20, 21, K_FINALIZE]


@pytest.mark.parametrize("dims,s,p", NOT_TAKEN, ids=lambda v: "x".join(map(str, v)))
def test_planner_not_taken_shapes(dims, s, p):
    assert families(0, dims, s, p) == [19]
    assert families(1, dims, s, p) == [20, 21, K_FINALIZE]
    assert _native.lib().rk3d_sf32_streams(*dims, *s, *p, 0, 2) == 0


def test_workspace_holds_the_partials():
    L = _native.lib()
    for dims, s, p in [(d, S2, P0) for d in STREAM_S2] + NOT_TAKEN + [WO12]:
        for aligned in (15, 14):
            rc, launches, P, fin = plan(1, dims, s, p, aligned=aligned)
            assert rc == 0 and P > 0 and fin == 1
            assert dims[2] * 3 * P * 4 <= L.rk3d_backward_workspace_bytes(*dims, *s, *p, 2), (dims, s, p)


def test_predicate_is_the_first_launch():
    L = _native.lib()
    streaming = STREAM16 | {FWD_S2, BWD_S2}
    cases = [(d, S2, P0) for d in STREAM_S2] + NOT_TAKEN + [WO12] + STREAM + GENERIC
    for dims, s, p in cases:
        for q in (0, 1):
            for form in (0, 1):
                first = families(form, dims, s, p, quantize=q)[0]
                assert L.rk3d_sf32_streams(*dims, *s, *p, q, 2) == int(first in streaming), (dims, s, p, q, form)
    for dims in STREAM_S2:
        assert L.rk3d_sf32_streams(*dims, *S2, *P0, 0, 2) == 1
        assert L.rk3d_sf32_streams(*dims, *S2, *P0, 0, 4) == 0
    # the networks' four down-sampling layers at batch 32: the two large ones stream, 28 -> 14 and 14 -> 7 do not
    for C, H, streams in ((72, 112, 1), (144, 56, 1), (288, 28, 0), (576, 14, 0), (54, 112, 1), (108, 56, 1)):
        assert L.rk3d_sf32_streams(32, 8, C, H, H, *S2, *P0, 0, 2) == streams, (C, H)


def test_family_numbers():
    seen = set()
    for dims in STREAM_S2:
        for form in (0, 1):
            seen |= set(families(form, dims))
    assert seen == {FWD_S2, BWD_S2, K_FINALIZE}
    # appended: nothing before them has moved (tests/test_shift3d16.py pins 18 .. 23 over its own shapes)
    assert families(0, STREAM[0][0], STREAM[0][1], STREAM[0][2]) == [22]
    assert families(1, GENERIC[0][0], GENERIC[0][1], GENERIC[0][2]) == [20, 21, K_FINALIZE]
