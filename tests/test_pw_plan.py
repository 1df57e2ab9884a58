"""The kernel choice of the fp32 1x1 GEMM (rk_pw.hip: plan_gemm, through rk_debug_pw_gemm_plan -- no device needed) against
tables recorded from the dispatch it replaced: every call below ran the same kernel instantiation with the same grid, block
and dynamic LDS, or failed with the same status, before the planner existed.

The sweep: every fp32 1x1 layer of the four tiers on planes with H * W % 4 == 0 (rubiksnet/backbone.py:139-171, widths 54 / 72;
forward (K, M) and d(input) (M, K)) x 8 .. 512 frames x both operand layouts x A aligned or not x every epilogue (none,
statistics, BatchNorm backward) with and without residual, prologue and output affine x every RK_PW2 / RK_PW3 / RK_PW4
setting, at 256 CUs."""
import ctypes
import gzip
import os

from rubiksnet_amd import _native

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rows(name):
    opener = gzip.open if name.endswith(".gz") else open
    with opener(os.path.join(GOLDEN, name), "rt") as f:
        return [line.split() for line in f if not line.startswith("#")]


def test_gemm_plan_matches_the_recorded_dispatch():
    L = _native.lib()
    out = (ctypes.c_int * 5)()
    rows = _rows("pw_gemm_plan_parent.txt.gz")
    assert len(rows) == 172800
    bad = []
    for r in rows:
        call, want = [int(v) for v in r[:13]], [int(v) for v in r[13:]]
        rc = L.rk_debug_pw_gemm_plan(*call, 256, out)
        got = [rc] + ([0] * 5 if rc else list(out))
        if got != want:
            bad.append((call, want, got))
    assert not bad, "%d calls planned differently, e.g. %r" % (len(bad), bad[:3])


def test_epilogue_plans_keep_the_tile_promise():
    """A caller of a training epilogue allocates rk_pw_gemm_tiles() records before the call: the planned kernel writes exactly
    that many.  (Shapes whose choice does not depend on the CU count, on this process's switches.)"""
    L = _native.lib()
    modes = [int(os.environ.get(k, "1") or 0) for k in ("RK_PW2", "RK_PW3", "RK_PW4")]
    out = (ctypes.c_int * 5)()
    n = 0
    for r in _rows("pw_gemm_plan_parent.txt.gz"):
        F, K, M, P, mk, al, epi, res, pro, ma = (int(v) for v in r[:10])
        if not epi or [int(v) for v in r[10:13]] != [1, 1, 1] or 256 < M <= 288:
            continue
        rc = L.rk_debug_pw_gemm_plan(F, K, M, P, mk, al, epi, res, pro, ma, *modes, 256, out)
        if rc == 0:
            assert out[4] == L.rk_pw_gemm_tiles(ctypes.c_void_p(4096 if al else 4100), F, K, M, P, mk), r
            n += 1
    assert n > 1000


def test_wgrad_plan_matches_the_recorded_dispatch():
    L = _native.lib()
    kinds = {"narrow": 0, "wide": 1, "pw2": 2}
    rows = _rows("pw_wgrad_plan_parent.txt")
    assert len(rows) == 600
    for F, K, M, P, pro, pw2, rc, kind, ws in rows:
        assert L.rk_debug_pw_wgrad_plan(int(F), int(K), int(M), int(P), int(pw2)) == kinds[kind], (F, K, M, P, pw2)
