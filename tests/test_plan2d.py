"""The kernel choice of RubiksShift2D (rk2d_plan.hpp: plan2d::plan, through rk_debug_2d_plan -- no device needed) against a table
recorded from the try-each-launcher dispatch it replaced (tests/golden/plan2d_parent.txt.gz, whose header says how it was made):
every call of the table ran the same kernel instantiations with the same grid, block and dynamic LDS, or failed with the same
status, before the planner existed; and the two answers derived from the plan -- the workspace sizes and rk2d_bn_fused_shape --
are what they were.

The sweep: every shape of test_parity_2d.py and test_bn_shift2d_gpu.py, the 2-D layers of the four tiers at batch 32, and planes
on the edge of each rule (W % 4, W % 8, W < 4, 14x14 with odd C, Ho * Wo of 64 / 65 / 255 / 256 / 257, planes too wide or tall
for the bands and rings, N around each frames-per-group constant, odd H at stride 2, mixed strides, padding) x every entry point
(the four S == T types, the two _sf32 types, the two BN types; forward, d(x) alone, both gradients) x quantize x each operand
aligned, off by 8 bytes or off by one element x every RK_SHIFT_KERNELS setting x 256 / 64 compute units."""
import ast
import ctypes
import gzip
import os
import re

import pytest

from rubiksnet_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))

# family (the enum of rk2d_plan.hpp) -> kernel instantiation from the planned variant
KERNELS = {
    1: "k2d_forward<{T},{S},{quant}>", 2: "k2d_backward_input<{T},{S},{quant}>", 3: "k2d_backward_shift<{T},{S}>",
    4: "k2d_finalize<{T},{S}>", 5: "k2d_finalize_bn", 6: "k2d_dma_interp<{negate},{rounds},2>", 7: "k2d_dma_backward<{rounds},1,1>",
    8: "k2d_stage_interp<{T},{S},{negate},{rounds},{bn}>", 9: "k2d_stage_backward<{T},{S},{rounds},{bn}>",
    10: "k2d_raw16_interp<{T},{S},{negate},{rounds},2,{bn}>", 11: "k2d_raw16_backward<{T},{S},{rounds},{bn}>",
    12: "k2d_tile_interp<{T},{S},14,14,4,{negate},{bn}>", 13: "k2d_tile_backward<{T},{S},14,14,3,{bn}>",
    14: "k2d_forward_column<{T},{S},{M},{vec},{bn}>", 15: "k2d_backward_column<{T},{S},{M},{single},{vec},{bn}>",
}
# table entry -> (activation type, shift type, element bytes, BN entry point)
ENTRIES = {0: ("float", "float", 4, 0), 1: ("double", "double", 8, 0), 2: ("__half", "__half", 2, 0),
           3: ("__hip_bfloat16", "__hip_bfloat16", 2, 0), 4: ("__half", "float", 2, 0), 5: ("__hip_bfloat16", "float", 2, 0),
           6: ("float", "float", 4, 1), 7: ("__hip_bfloat16", "float", 2, 1)}
BOOL = ("false", "true")


def family_of(kernel):
    return kernel.split("<")[0]


def aligned_bits(entry, mis):
    """rk_debug_2d_plan's `aligned` from the table's per-operand offsets (0: none, 1: 8 bytes, 2: one element)"""
    bits = 0
    for i, m in enumerate(mis):
        off = (0, 8, 4 if i == 3 else ENTRIES[entry][2])[m]          # (the BN pack is fp32)
        bits |= (2 if off % 16 == 0 else 1 if off % 8 == 0 else 0) << (2 * i)
    return bits


def planned(L, out, sk, cus, entry, form, dims, quantize, gshift, aligned):
    """(rc, [kernel, grid, block, lds] per launch, P, finalize) of one call"""
    T, S, elem, bn = ENTRIES[entry]
    rc = L.rk_debug_2d_plan(form + 2 * bn, elem, *dims, quantize, gshift, aligned, sk, cus, out)
    if rc:
        return rc, [], 0, 0
    launches = []
    for i in range(out[0]):
        o = out[3 + 11 * i:14 + 11 * i]
        name = KERNELS[o[0]].format(T=T, S=S, negate=BOOL[o[1]], bn=BOOL[o[2]], rounds=o[3], M=o[4], single=BOOL[o[5]],
                                    vec=BOOL[o[6]], quant=BOOL[o[7]])
        launches += [name, str(o[8]), str(o[9]), str(o[10])]
    return rc, launches, out[1], out[2]


@pytest.fixture(scope="module")
def table():
    with gzip.open(os.path.join(HERE, "golden", "plan2d_parent.txt.gz"), "rt") as f:
        rows = [line.split() for line in f if not line.startswith("#")]
    return [r for r in rows if r[0] != "S"], [[int(v) for v in r[1:]] for r in rows if r[0] == "S"]


def test_plan_matches_the_recorded_dispatch(table):
    L = _native.lib()
    out = (ctypes.c_int * 36)()
    calls, _ = table
    assert len(calls) == 67160
    bad = []
    for r in calls:
        call = [int(v) for v in r[:18]]
        want = (int(r[18]), r[20:-2], int(r[-2]), int(r[-1]))
        assert len(want[1]) == 4 * int(r[19])
        sk, cus, entry, form = call[:4]
        got = planned(L, out, sk, cus, entry, form, call[4:12], call[12], call[13], aligned_bits(entry, call[14:18]))
        if got != want:
            bad.append((call, want, got))
    assert not bad, "%d calls planned differently, e.g. %r" % (len(bad), bad[:3])


def test_planned_partials_fit_the_workspace(table):
    """A caller sizes the workspace with rk2d_backward_workspace_bytes / rk2d_backward_bn_workspace_bytes before the call: the P
    partials per channel and sum that the planned d(shift) launch writes -- two sums, four for the BN backward; 16 bytes each for
    fp32 and 16-bit storage (granule pairs), 8 for fp64 -- fit.  (The sizes are the process's: RK_SHIFT_KERNELS unset here, which
    is the largest of the three.)"""
    L = _native.lib()
    calls, _ = table
    n = 0
    for r in calls:
        entry, form, dims, gshift, rc, P = int(r[2]), int(r[3]), [int(v) for v in r[4:12]], int(r[13]), int(r[18]), int(r[-2])
        if rc or form == 0 or not gshift:
            assert P == 0, r
            continue
        assert P > 0, r
        C = dims[1]
        if ENTRIES[entry][3]:
            assert C * 4 * P * 16 <= L.rk2d_backward_bn_workspace_bytes(*dims), r
        else:
            elem = ENTRIES[entry][2]
            assert C * 2 * P * (8 if elem == 8 else 16) <= L.rk2d_backward_workspace_bytes(*dims, elem), r
        n += 1
    assert n > 20000


def test_workspace_sizes_are_what_they_were(table):
    L = _native.lib()
    assert L.rk2d_backward_workspace_bytes(4, 10, 7, 7, 1, 1, 0, 0, 4) == 10 * 2 * 4 * 16                 # P = N
    assert L.rk2d_backward_workspace_bytes(256, 288, 14, 14, 1, 1, 0, 0, 2) == 288 * 2 * 256 * 16        # N above the 64 tile groups
    assert L.rk2d_backward_workspace_bytes(256, 72, 56, 56, 1, 1, 0, 0, 4) == 72 * 2 * 256 * 16
    assert L.rk2d_backward_workspace_bytes(256, 72, 56, 56, 1, 1, 0, 0, 8) == 72 * 2 * 256 * 16          # (one size for every type)
    assert L.rk2d_backward_workspace_bytes(2, 2, 997, 8, 1, 1, 0, 0, 4) == 2 * 2 * 997 * 16              # one-row bands of a prime H
    assert L.rk2d_backward_workspace_bytes(1, 2, 4, 8192, 1, 1, 0, 0, 4) == 2 * 2 * 32 * 16              # column chunks of 1024
    assert L.rk2d_backward_bn_workspace_bytes(256, 288, 14, 14, 1, 1, 0, 0) == 288 * 4 * 256 * 16
    assert L.rk2d_backward_workspace_bytes(0, 10, 7, 7, 1, 1, 0, 0, 4) == 0
    _, shapes = table
    n = 0
    for sk, *dims, ws4, ws8, wsbn, _, _ in shapes:
        if sk == 0:                                                    # (this process: RK_SHIFT_KERNELS unset)
            assert (L.rk2d_backward_workspace_bytes(*dims, 4), L.rk2d_backward_workspace_bytes(*dims, 8),
                    L.rk2d_backward_bn_workspace_bytes(*dims)) == (ws4, ws8, wsbn), dims
            assert L.rk2d_backward_workspace_bytes(*dims, 2) == ws4
            n += 1
    assert n == 116


def test_bn_fused_shape_is_what_it_was_and_what_the_plan_says(table):
    """fused_bn.bn_relu_shift2d asks rk2d_bn_fused_shape BEFORE bn2's statistics run (their side effects must happen once): the
    answer is the recorded one for every swept shape and setting, and whenever it is 1 both BN entry points plan to RK_OK with
    aligned operands -- they cannot answer RK_ERR_UNSUPPORTED afterwards."""
    L = _native.lib()
    out = (ctypes.c_int * 36)()
    _, shapes = table
    ones = 0
    for sk, *dims, _, _, _, fused4, fused2 in shapes:
        for entry, fused in ((6, fused4), (7, fused2)):
            if sk == 0:
                assert L.rk2d_bn_fused_shape(*dims, ENTRIES[entry][2]) == fused, dims
            for cus in (256, 64):
                both = all(planned(L, out, sk, cus, entry, form, dims, 0, 1, 0xAA)[0] == 0 for form in (0, 1))
                assert both == bool(fused), (sk, dims, entry)
            ones += fused
    assert ones > 200
    assert L.rk2d_bn_fused_shape(4, 8, 14, 14, 1, 1, 0, 0, 8) == 0 and L.rk2d_bn_fused_shape(0, 8, 14, 14, 1, 1, 0, 0, 4) == 0


def _gpu_test_calls():
    """(entry, form, dims, quantize, gshift) of the calls tests/test_parity_2d.py and tests/test_bn_shift2d_gpu.py make on a GPU"""
    def pair(v):
        return (v, v) if isinstance(v, int) else tuple(v)

    def lists(path, arg):
        src = open(os.path.join(HERE, path)).read()
        return [ast.literal_eval(m) for m in re.findall(r'parametrize\("%s", (\[.*?\])\)' % re.escape(arg), src, re.S)]

    src = open(os.path.join(HERE, "test_parity_2d.py")).read()
    shapes = ast.literal_eval(re.search(r"^SHAPES = (\[.*?^\])", src, re.S | re.M).group(1))
    calls = []
    for (N, C, H, W, s, p) in shapes:                                  # fp32 / fp64: forward, both gradients
        for entry in (0, 1):
            for q in (0, 1):
                calls += [(entry, 0, (N, C, H, W) + pair(s) + pair(p), q, 0), (entry, 1, (N, C, H, W) + pair(s) + pair(p), q, 1)]
    enable_false, half = lists("test_parity_2d.py", "shape")
    for shape in enable_false:
        calls += [(0, 1, tuple(shape) + (1, 1, 0, 0), 0, 0), (0, 0, tuple(shape) + (1, 1, 0, 0), 0, 0), (0, 1, tuple(shape) + (1, 1, 0, 0), 0, 1)]
    for shape in half:                                                 # f16 / bf16, S == T
        for entry in (2, 3):
            calls += [(entry, 0, tuple(shape) + (1, 1, 0, 0), 0, 0), (entry, 1, tuple(shape) + (1, 1, 0, 0), 0, 1),
                      (entry, 1, tuple(shape) + (1, 1, 0, 0), 0, 0)]
    (sf32,) = lists("test_parity_2d.py", "cfg")
    for (N, C, H, W, s, p) in sf32:
        for entry in (4, 5):
            for q in (0, 1):
                calls += [(entry, 0, (N, C, H, W) + pair(s) + pair(p), q, 0), (entry, 1, (N, C, H, W) + pair(s) + pair(p), q, 1)]
            calls.append((entry, 1, (N, C, H, W) + pair(s) + pair(p), 1, 0))
    (bn,) = lists("test_bn_shift2d_gpu.py", "Fr,C,H,stride,padding")
    for (Fr, C, H, s, p) in bn:
        for entry in (6, 7):
            if entry == 6 and H in (56, 112, 16, 28, 12) and (s, p) == (1, 0):      # (the test skips these: nothing fused in fp32)
                continue
            calls += [(entry, 0, (Fr, C, H, H) + pair(s) + pair(p), 0, 1), (entry, 1, (Fr, C, H, H) + pair(s) + pair(p), 0, 1)]
    return calls


def test_gpu_test_shapes_reach_every_kernel_family(table):
    """tests/test_parity_2d.py and tests/test_bn_shift2d_gpu.py reach every kernel family on a GPU: over the calls they make (aligned
    operands, RK_SHIFT_KERNELS unset) the planned families are all the table contains."""
    L = _native.lib()
    out = (ctypes.c_int * 36)()
    reached = set()
    for entry, form, dims, q, gshift in _gpu_test_calls():
        rc, launches, _, _ = planned(L, out, 0, 256, entry, form, dims, q, gshift, 0xAA)
        assert rc == 0, (entry, form, dims)
        reached.update(family_of(k) for k in launches[::4])
    calls, _ = table
    in_table = {family_of(t) for r in calls for t in r[20:-2:4]}
    assert len(in_table) == 15
    assert reached == in_table, in_table - reached
