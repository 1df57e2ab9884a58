"""Host reference of the streaming metrics (rubiksnet_amd.metrics, rk_metrics.hip), written from the rules in
include/rubiks_hip.h and shared by the CPU and GPU tests.  Test infrastructure: it calls nothing of the code under test.

The test logits are integer multiples of a power of two `unit` in [-8, 8] (2^-6 for fp32 / fp16, 2^-3 for bf16: every format
holds them exactly), so the sum over up to 10 views is exact in fp32 and the division by `views` is monotone: ranks, hits,
per-class counts and the confusion matrix are compared EXACTLY against integer arithmetic on the numerators.  The loss is
compared against fp64 on the exact rational consensus, per video within LOSS_TOL = 2e-5: |z| <= 8 gives a loss below
16 + ln K < 32, where an fp32 ulp is 1.9e-6; the rounding of z, a 2-ulp expf, a tree sum over K terms and the final
subtraction come to about 6e-6, and the bound leaves 3x over that.  The loss WORD of the state (a sum of llrint(loss * 2^32))
is within N * (LOSS_TOL * 2^32 + 1/2) units for N finite videos.
"""
import functools

import numpy as np

HEAD = 8
LOSS_TOL = 2e-5
UNIT = {"f32": 2.0 ** -6, "f16": 2.0 ** -6, "bf16": 2.0 ** -3}
GRID_K = (1, 3, 64, 65, 174, 1000)
GRID_V = (1, 2, 3, 6, 10)
GRID_B = (1, 5, 33)


def words(K, confusion):
    return HEAD + 2 * K + (K * K if confusion else 0)


def make_case(seed, B, V, K, unit):
    """(logits fp64 [B, V, K]: exact multiples of `unit` in [-8, 8]; labels int64 [B], the first forced to 0 and the last to
    K - 1 when there are several)."""
    rng = np.random.default_rng(seed)
    top = int(round(8 / unit))
    x = rng.integers(-top, top + 1, size=(B, V, K)).astype(np.float64) * unit
    y = rng.integers(0, K, size=B).astype(np.int64)
    if B > 1:
        y[0], y[-1] = 0, K - 1
    return x, y


@functools.lru_cache(maxsize=None)
def grid_case(B, V, K, unit):
    """One case of the grid with its reference (topk (1, 5), with the confusion matrix), computed once and read-only."""
    x, y = make_case(1000 * K + 10 * V + B, B, V, K, unit)
    ref = reference(x, y, (1, 5), True, unit)
    for a in (x, y) + tuple(v for v in ref.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return x, y, ref


def reference(x, labels, topk, confusion, unit):
    """x fp64 [B, V, K] (multiples of `unit`, or NaN / +-inf), labels int64 [B].  Returns dict(state int64 with word 1 = 0,
    loss_sum fp64 (the sum of the finite videos' losses), finite (their number), consensus fp64 [B, K], pred, rank int64 [B]
    (-1 where undefined), loss fp64 [B] (NaN where undefined))."""
    B, V, K = x.shape
    state = np.zeros(words(K, confusion), dtype=np.int64)
    consensus = np.zeros((B, K))
    pred = np.full(B, -1, dtype=np.int64)
    rank = np.full(B, -1, dtype=np.int64)
    loss = np.full(B, np.nan)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            s = x[b].sum(axis=0)                       # exact in fp64 for multiples of `unit` (NaN / inf propagate)
        consensus[b] = s / V                           # fp64; compared after rounding to fp32, which is what fp32 s / V gives
        finite = bool(np.isfinite(s).all())
        y = int(labels[b])
        if finite:
            n = np.rint(s / unit).astype(np.int64)     # the integer numerators: z = n * unit / V
            assert (n * unit == s).all()
            pred[b] = int(np.argmax(n))                # (numpy: the first of equal maxima)
        if not 0 <= y < K:
            state[3] += 1
            continue
        state[0] += 1
        state[HEAD + y] += 1
        if not finite:
            state[2] += 1
            continue
        rank[b] = int((n > n[y]).sum() + (n[:y] == n[y]).sum())
        z = n.astype(np.float64) * unit / V
        m = z.max()
        loss[b] = m + np.log(np.exp(z - m).sum()) - z[y]
        for slot, k in enumerate(topk):
            state[4 + slot] += rank[b] < k
        state[HEAD + K + y] += rank[b] == 0
        if confusion:
            state[HEAD + 2 * K + y * K + pred[b]] += 1
    done = np.isfinite(loss)
    return {"state": state, "loss_sum": float(loss[done].sum()), "finite": int(done.sum()), "consensus": consensus,
            "pred": pred, "rank": rank, "loss": loss}


def add(refs):
    """The reference of several updates into one meter."""
    return {"state": sum(r["state"] for r in refs), "loss_sum": sum(r["loss_sum"] for r in refs),
            "finite": sum(r["finite"] for r in refs)}


def check_state(got, ref, what=""):
    """got: int64 numpy state.  Every word but the loss word exactly; the loss word within the bound of the module docstring."""
    got = np.asarray(got)
    want = ref["state"]
    assert got.shape == want.shape, (what, got.shape, want.shape)
    mask = np.ones(got.size, dtype=bool)
    mask[1] = False
    bad = np.flatnonzero((got != want) & mask)
    assert bad.size == 0, "%s: %d integer words differ, first at %d: got %d, want %d" % (
        what, bad.size, bad[0], got[bad[0]], want[bad[0]])
    err = abs(int(got[1]) - ref["loss_sum"] * 2.0 ** 32)
    assert err <= ref["finite"] * (LOSS_TOL * 2.0 ** 32 + 0.5), "%s: loss word off by %g units (%g per video)" % (
        what, err, err / 2.0 ** 32 / max(ref["finite"], 1))


def check_outputs(out, ref, what=""):
    """out: dict of numpy arrays (consensus fp32, pred / rank int32, loss fp32) as update(outputs=...) returned them."""
    with np.errstate(invalid="ignore", over="ignore"):
        want_z = ref["consensus"].astype(np.float32)
    got_z = np.asarray(out["consensus"])
    assert got_z.dtype == np.float32 and np.array_equal(got_z, want_z, equal_nan=True), "%s: consensus" % what
    assert np.array_equal(np.asarray(out["pred"]).astype(np.int64), ref["pred"]), "%s: pred" % what
    assert np.array_equal(np.asarray(out["rank"]).astype(np.int64), ref["rank"]), "%s: rank" % what
    got, want = np.asarray(out["loss"]).astype(np.float64), ref["loss"]
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: which losses are NaN" % what
    if np.isfinite(want).any():
        err = np.nanmax(np.abs(got - want))
        assert err <= LOSS_TOL, "%s: loss off by %g" % (what, err)
