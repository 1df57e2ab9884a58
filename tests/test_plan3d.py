"""The kernel choice of RubiksShift3D (rk3d_plan.hpp: plan3d::plan, through rk_debug_3d_plan -- no device needed) against a table
recorded from the try-each-launcher dispatch it replaced (tests/golden/plan3d_parent.txt.gz, whose header says how it was made):
every call of the table ran the same kernel instantiations with the same grid, block and dynamic LDS, or failed with the same
status, before the planner existed.

The sweep: every shape of test_parity_3d.SHAPES, the layers of the four tiers at batch 32, and planes on the edge of each rule
(W % 4, W < 4, H * W of 255 / 256 / 257, W = 15 / 16, T of 1 .. 9, bands around 6 KB, LDS rings beyond the caps, odd H at stride 2,
Wo % 4, C * H * W % 4, temporal stride / padding, spatial padding) x every entry point x fp32 / fp64 x quantize x each operand
aligned or off by 4 bytes x every RK_SHIFT_KERNELS / RK_SLAB14 setting."""
import ast
import ctypes
import gzip
import os
import re

import pytest

from rubiksnet_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))

# family (the enum of rk3d_plan.hpp) -> kernel instantiation from the variant v[0..4]; t: f / d
KERNELS = {
    1: "k3d_plane_interp<{0},{2},{3},{1}>", 2: "k3d_dma_interp<{0},{2},2,{1}>", 3: "k3d_dma_backward<{2},{0},1,1,{1},{3},{4}>",
    4: "k3d_tile14_interp<{0},{1}>", 5: "k3d_tile14_backward<{0},{1},{2}>", 6: "k3d_slab_interp<{0},{2},3>",
    7: "k3d_slab_backward<{0},{1},{2},8>", 8: "k3d_translate<{0}>", 9: "k3d_s2_forward<4,2,{1}>", 10: "k3d_s2_backward<4,{0},{1},{2}>",
    11: "k3d_slab_s2_forward", 12: "k3d_slab_s2_backward<{0},{1}>", 13: "k3d_forward_column<{t},{2}>",
    14: "k3d_backward_column<{t},{0},{2},{3},{4},{1}>", 15: "k3d_forward_generic<{t},{0}>", 16: "k3d_backward_input_generic<{t},{0}>",
    17: "k3d_backward_shift_generic<{t}>", 18: "k3d_finalize<{t}>",
}
# table form -> (form, want_gx, want_gshift, two_phase) of rk_debug_3d_plan
FORMS = {0: (0, 0, 0, 0), 1: (1, 1, 1, 0), 2: (1, 1, 0, 0), 3: (1, 0, 1, 0), 4: (1, 1, 1, 1), 5: (2, 0, 0, 0), 6: (3, 1, 1, 0),
         7: (1, 0, 1, 1)}


def family_of(kernel):
    return re.match(r"k3d_[a-z0-9_]*[a-z0-9]", kernel).group(0)


def planned(L, out, sk, s14, form, elem, dims, quantize, misaligned):
    """(rc, [kernel, grid, block, lds] per launch, P, finalize) of one call"""
    rc = L.rk_debug_3d_plan(FORMS[form][0], elem, *dims, quantize, *FORMS[form][1:], 15 & ~misaligned, sk, s14, out)
    if rc:
        return rc, [], 0, 0
    launches = []
    for i in range(out[0]):
        o = out[3 + 9 * i:12 + 9 * i]
        launches += [KERNELS[o[0]].format(*o[1:6], t="f" if elem == 4 else "d"), str(o[6]), str(o[7]), str(o[8])]
    return rc, launches, out[1], out[2]


@pytest.fixture(scope="module")
def table():
    with gzip.open(os.path.join(HERE, "golden", "plan3d_parent.txt.gz"), "rt") as f:
        return [line.split() for line in f if not line.startswith("#")]


def test_plan_matches_the_recorded_dispatch(table):
    L = _native.lib()
    out = (ctypes.c_int * 30)()
    assert len(table) == 115632
    bad = []
    for r in table:
        call = [int(v) for v in r[:17]]
        want = (int(r[17]), r[19:-2], int(r[-2]), int(r[-1]))
        assert len(want[1]) == 4 * int(r[18])
        got = planned(L, out, call[0], call[1], call[2], call[3], call[4:15], call[15], call[16])
        if got != want:
            bad.append((call, want, got))
    assert not bad, "%d calls planned differently, e.g. %r" % (len(bad), bad[:3])


def test_planned_partials_fit_the_workspace(table):
    """A caller sizes the workspace with rk3d_backward_workspace_bytes / rk3d_backward_bn_workspace_bytes before the call: the
    P partials per channel and sum that the planned d(shift) launch writes (fp32: 16-byte granule pairs) fit."""
    L = _native.lib()
    n = 0
    for r in table:
        form, elem, dims, rc, P = int(r[2]), int(r[3]), [int(v) for v in r[4:15]], int(r[17]), int(r[-2])
        if rc or form in (0, 2, 5):
            continue
        assert P > 0, r
        C = dims[2]
        if form == 6:
            assert C * 5 * P * 16 <= L.rk3d_backward_bn_workspace_bytes(*dims), r
        else:
            assert C * 3 * P * (16 if elem == 4 else 8) <= L.rk3d_backward_workspace_bytes(*dims, elem), r
        n += 1
    assert n > 50000


def test_workspace_sizes_are_what_they_were():
    L = _native.lib()
    assert L.rk3d_backward_workspace_bytes(32, 8, 64, 56, 56, 1, 1, 1, 0, 0, 0, 4) == 64 * 3 * 32 * 56 * 16
    assert L.rk3d_backward_workspace_bytes(32, 8, 64, 56, 56, 1, 1, 1, 0, 0, 0, 8) == 64 * 3 * 32 * 56 * 8
    assert L.rk3d_backward_workspace_bytes(2, 9, 5, 7, 7, 2, 1, 1, 1, 0, 0, 4) == 5 * 3 * 2 * 7 * 16       # max(To = 5, H, chunks)
    assert L.rk3d_backward_workspace_bytes(1, 4, 2, 3, 1024, 1, 1, 1, 0, 0, 0, 4) == 2 * 3 * 12 * 16      # 12 chunks of 256
    assert L.rk3d_backward_bn_workspace_bytes(32, 8, 64, 56, 56, 1, 1, 1, 0, 0, 0) == 64 * 5 * 32 * 56 * 16
    assert L.rk3d_backward_workspace_bytes(0, 8, 64, 56, 56, 1, 1, 1, 0, 0, 0, 4) == 0


def test_parity_shapes_reach_every_kernel_family(table):
    """tests/test_parity_3d.py claims to reach every kernel family on a GPU: over its SHAPES x the forms it runs (forward,
    backward with both gradients / one of them, fp32 and fp64, quantize) and the BatchNorm forms and two-phase form that
    test_train_block_gpu.py and test_two_phase_backward run on shapes of the same classes, the planned families are all the
    table contains."""
    src = open(os.path.join(HERE, "test_parity_3d.py")).read()
    shapes = ast.literal_eval(re.search(r"^SHAPES = (\[.*?^\])", src, re.S | re.M).group(1))
    L = _native.lib()
    out = (ctypes.c_int * 30)()
    reached = set()
    for (N, T, C, H, W, s, p) in shapes:
        for form in FORMS:
            for elem in ((4, 8) if form < 4 else (4,)):
                for q in (0, 1):
                    _, launches, _, _ = planned(L, out, 0, -1, form, elem, (N, T, C, H, W) + tuple(s) + tuple(p), q, 0)
                    reached.update(family_of(k) for k in launches[::4])
    in_table = {family_of(t) for r in table for t in r[19:-2:4]}
    assert len(in_table) == 18
    assert reached == in_table, in_table - reached
