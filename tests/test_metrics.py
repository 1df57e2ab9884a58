"""rubiksnet_amd.metrics without a device: the torch-op path against the integer / fp64 host reference on the grid of the GPU
test, the state layout, the C ABI's argument checks, merge, the arithmetic of result(), and evaluate_streaming against
evaluate on a CPU RubiksNet-Tiny."""
import ctypes

import numpy as np
import pytest
import torch

import _metrics_ref as mr
from rubiksnet_amd import _native
from rubiksnet_amd.metrics import HEAD_WORDS, OUTPUTS, StreamMeter

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _update(meter, x, y, dtype, outputs=OUTPUTS):
    B, V, K = x.shape
    out = meter.update(torch.from_numpy(np.array(x)).to(dtype).reshape(B * V, K), torch.from_numpy(np.array(y)), outputs)
    return {k: v.numpy() for k, v in out.items()}


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_torch_path_matches_the_reference_on_the_grid(sfx):
    for K in mr.GRID_K:
        for V in mr.GRID_V:
            for B in mr.GRID_B:
                x, y, ref = mr.grid_case(B, V, K, mr.UNIT[sfx])
                meter = StreamMeter(K, topk=(1, 5), views=V)
                out = _update(meter, x, y, DTYPES[sfx])
                what = "%s K=%d V=%d B=%d" % (sfx, K, V, B)
                mr.check_outputs(out, ref, what)
                mr.check_state(meter.state.numpy(), ref, what)
                assert (meter.native_updates, meter.torch_updates) == (0, 1)


def test_the_grid_has_ties_with_the_label():
    """The tie rule is exercised by the data itself: videos whose label's consensus is shared by another class."""
    ties = 0
    for B in mr.GRID_B:
        x, y, _ = mr.grid_case(B, 2, 1000, mr.UNIT["f32"])
        s = x.sum(axis=1)
        ties += sum(int((s[b] == s[b, y[b]]).sum() > 1) for b in range(B))
    assert ties >= 10


def test_bad_labels_and_nonfinite_videos_in_torch_ops():
    K, V, B = 65, 3, 9
    x, y = mr.make_case(5, B, V, K, 2.0 ** -6)
    y[1], y[4] = -1, K
    x[2, 1, 7], x[5, 0, 64], x[7, 2, 0] = np.nan, np.inf, -np.inf
    ref = mr.reference(x, y, (1, 5), True, 2.0 ** -6)
    assert ref["state"][0] == 7 and ref["state"][2] == 3 and ref["state"][3] == 2
    meter = StreamMeter(K, views=V)
    out = _update(meter, x, y, torch.float32)
    mr.check_outputs(out, ref)
    mr.check_state(meter.state.numpy(), ref)
    res = meter.result()
    assert (res["videos"], res["nonfinite"], res["bad_labels"]) == (7, 3, 2)
    assert res["top1"] == pytest.approx(100.0 * int(ref["state"][4]) / 7)          # the NaN videos lower the accuracy
    assert res["loss"] == pytest.approx(ref["loss_sum"] / 4, abs=mr.LOSS_TOL + 4 * 2.0 ** -33)


def test_state_layout_and_state_bytes():
    L = _native.lib()
    for K in (1, 7, 174, 65536):
        assert L.rk_metrics_state_bytes(K, 0) == 8 * (8 + 2 * K)
        assert L.rk_metrics_state_bytes(K, 1) == 8 * (8 + 2 * K + K * K)
    assert L.rk_metrics_state_bytes(0, 1) == 0 and L.rk_metrics_state_bytes(65537, 0) == 0
    assert HEAD_WORDS == 8 == mr.HEAD
    for confusion in (False, True):
        m = StreamMeter(7, topk=(1, 3, 5), views=2, confusion=confusion)
        assert m.state is None and 8 * m.words == L.rk_metrics_state_bytes(7, int(confusion))
        m.update(torch.zeros(4, 7), torch.tensor([6, 0]))
        assert m.state.dtype == torch.int64 and m.state.numel() == m.words == mr.words(7, confusion)
    # all logits equal: every class ties with the label, which loses to the lower indices
    s = m.state.tolist()
    assert s[0] == 2 and s[2:8] == [0, 0, 1, 1, 1, 0]                  # hits at k = 1, 3, 5: only the video of label 0
    assert abs(s[1] / 2 ** 32 / 2 - np.log(7.0)) < 1e-6
    assert s[8:15] == [1, 0, 0, 0, 0, 0, 1] and s[15:22] == [1, 0, 0, 0, 0, 0, 0]
    conf = m.state[22:].view(7, 7)
    assert conf[0, 0] == 1 and conf[6, 0] == 1 and conf.sum() == 2


def test_argument_validation_without_a_device():
    """Every refusal comes back as its code before anything touches a device (dummy pointers, never dereferenced)."""
    L = _native.lib()
    one = ctypes.c_void_p(16)
    tail = (None, None, None, None, None)
    for name in ("rk_metrics_update_f32", "rk_metrics_update_bf16", "rk_metrics_update_f16"):
        fn = getattr(L, name)
        assert fn(None, one, one, 2, 1, 5, 0, 1, 1, 1, 1, 1, *tail) == -1
        assert fn(one, None, one, 2, 1, 5, 0, 1, 1, 1, 1, 1, *tail) == -1
        assert fn(one, one, None, 2, 1, 5, 0, 1, 1, 1, 1, 1, *tail) == -1
        for dims in ((0, 1, 5), (2, 0, 5), (2, 1, 0), (-1, 1, 5), (2, -3, 5), (2, 1, -5)):
            assert fn(one, one, one, *dims, 0, 1, 1, 1, 1, 1, *tail) == -2, dims
        assert fn(one, one, one, 2, 65, 5, 0, 1, 1, 1, 1, 1, *tail) == -7                # views > 64
        assert fn(one, one, one, 2, 1, 65537, 0, 1, 1, 1, 1, 1, *tail) == -7             # classes > 65536
        assert fn(one, one, one, 1 << 10, 32, 65536, 0, 1, 1, 1, 1, 1, *tail) == -2      # 2^31 logits
        assert fn(one, one, one, 2, 1, 5, 0, 5, 1, 1, 1, 1, *tail) == -7                 # five values of k
        assert fn(one, one, one, 2, 1, 5, 0, -1, 1, 1, 1, 1, *tail) == -2
        assert fn(one, one, one, 2, 1, 5, 0, 2, 1, 0, 1, 1, *tail) == -2                 # a k < 1
        assert fn(one, one, one, 2, 1, 5, 0, 4, 1, 2, 3, -4, *tail) == -2
        assert fn(one, one, ctypes.c_void_p(20), 2, 1, 5, 0, 1, 1, 1, 1, 1, *tail) == -2  # misaligned state
    for bad in (dict(num_classes=0), dict(num_classes=65537), dict(num_classes=5, views=65), dict(num_classes=5, views=0),
                dict(num_classes=5, topk=(1, 2, 3, 4, 5)), dict(num_classes=5, topk=(0,)), dict(num_classes=5, topk=(1, 1))):
        with pytest.raises(ValueError):
            StreamMeter(**bad)
    m = StreamMeter(5, views=2)
    for logits, labels in ((torch.zeros(3, 5), torch.zeros(1)), (torch.zeros(4, 6), torch.zeros(2)),
                           (torch.zeros(2, 3, 5), torch.zeros(2)), (torch.zeros(4, 5), torch.zeros(3))):
        with pytest.raises(ValueError):
            m.update(logits, labels.long())
    with pytest.raises(ValueError):
        m.update(torch.zeros(4, 5), torch.zeros(2).long(), outputs=("logits",))
    with pytest.raises(ValueError):
        m.state = torch.zeros(3, dtype=torch.int64)


def test_merge_equals_one_meter_fed_both_halves():
    K, V = 174, 3
    x, y = mr.make_case(9, 20, V, K, 2.0 ** -6)
    y[3] = K + 4
    x[11, 1, 5] = np.nan
    whole, a, b = (StreamMeter(K, topk=(1, 5, 200), views=V) for _ in range(3))
    _update(whole, x[:8], y[:8], torch.float32, ())
    _update(whole, x[8:], y[8:], torch.float32, ())
    _update(a, x[:8], y[:8], torch.float32, ())
    _update(b, x[8:], y[8:], torch.float32, ())
    assert a.merge(b) is a
    assert torch.equal(a.state, whole.state) and whole.torch_updates == 2
    empty = StreamMeter(K, topk=(1, 5, 200), views=V)
    assert torch.equal(empty.merge(a).state, whole.state) and torch.equal(a.merge(StreamMeter(K, (1, 5, 200), V)).state, whole.state)
    with pytest.raises(ValueError):
        a.merge(StreamMeter(K, topk=(1, 5), views=V))
    # [B, views, K] logits are the same update; reset() clears
    c = StreamMeter(K, topk=(1, 5, 200), views=V)
    c.update(torch.from_numpy(x[:8]).float(), torch.from_numpy(y[:8]))
    c.update(torch.from_numpy(x[8:]).float().transpose(0, 1).contiguous().transpose(0, 1), torch.from_numpy(y[8:]))
    assert torch.equal(c.state, whole.state)
    c.reset()
    assert int(c.state.abs().sum()) == 0 and c.result()["videos"] == 0


def test_result_arithmetic_on_a_hand_made_state():
    K = 4
    conf = np.array([[3, 1, 0, 0],
                     [2, 2, 0, 0],
                     [0, 0, 0, 0],
                     [1, 0, 1, 6]])
    m = StreamMeter(K, topk=(1, 2), views=1)
    s = torch.zeros(m.words, dtype=torch.int64)
    nonfinite = 2                                     # two more videos of class 1 whose logits were NaN
    videos = int(conf.sum()) + nonfinite
    s[0], s[1], s[2], s[3] = videos, int(24.5 * 2 ** 32), nonfinite, 5
    s[4], s[5] = int(np.trace(conf)), 13
    s[8:12] = torch.from_numpy(conf.sum(axis=1) + np.array([0, nonfinite, 0, 0]))
    s[12:16] = torch.from_numpy(np.diag(conf).copy())
    s[16:] = torch.from_numpy(conf.reshape(-1))
    m.state = s
    res = m.result()
    assert res["videos"] == 18 and res["nonfinite"] == 2 and res["bad_labels"] == 5
    assert res["loss"] == 24.5 / 16                                    # the mean over the finite videos only
    assert res["top1"] == 100.0 * 11 / 18 and res["top2"] == 100.0 * 13 / 18
    assert torch.equal(res["confusion"], torch.from_numpy(conf))
    per = res["per_class_acc"]
    assert per[0] == 3 / 4 and per[1] == 2 / 6 and torch.isnan(per[2]) and per[3] == 6 / 8
    assert res["mean_class_acc"] == pytest.approx((3 / 4 + 2 / 6 + 6 / 8) / 3, abs=1e-15)
    # without non-finite videos this is the reference script's mean of diag / row-sum over the classes it saw
    s[0], s[2] = 16, 0
    s[8:12] = torch.from_numpy(conf.sum(axis=1))
    seen = conf.sum(axis=1) > 0
    cls_acc = np.diag(conf)[seen] / conf.sum(axis=1)[seen]
    assert m.result()["mean_class_acc"] == pytest.approx(cls_acc.mean(), abs=1e-15)
    none = StreamMeter(K, confusion=False).result()
    assert none["confusion"] is None and none["videos"] == 0 and np.isnan(none["loss"]) and np.isnan(none["top1"])
    assert np.isnan(none["mean_class_acc"]) and bool(torch.isnan(none["per_class_acc"]).all())


def test_evaluate_streaming_agrees_with_evaluate_on_cpu_tiny(oracle):
    """RubiksNet-Tiny on the host (fp64 twin: the shift modules evaluated by the oracles), 2 batches of 3-view videos."""
    import _host_reference as hr
    from rubiksnet_amd import RubiksNet
    from rubiksnet_amd.evaluation import evaluate, evaluate_streaming

    torch.manual_seed(3)
    T, V, S, K = 8, 3, 32, 11
    net = hr.host_twin(RubiksNet("tiny", K, num_frames=T, verbose=False))
    batches = [(torch.randn(B, V * T * 3, S, S, dtype=torch.float64), torch.randint(0, K, (B,))) for B in (3, 2)]
    with hr.twin_guard():
        old = evaluate(net, batches, n_frames=T, views=V)
        new = evaluate_streaming(net, batches, n_frames=T, views=V, keep_logits=True)
    top = old["logits"].topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 1e-4                 # no ties, and none that fp32 could create
    assert new["videos"] == old["videos"] == 5
    # (evaluate forms each batch's percentage in fp32: a few ulp of 100, 1.2e-5 at most; a video is 20)
    assert new["top1"] == pytest.approx(old["top1"], abs=1e-4) and new["top5"] == pytest.approx(old["top5"], abs=1e-4)
    assert new["top5"] == 100.0 * round(old["top5"] * 5 / 100) / 5
    assert torch.equal(new["labels"], old["labels"]) and new["logits"].dtype == torch.float32
    assert torch.allclose(new["logits"].double(), old["logits"].double(), atol=1e-5, rtol=1e-5)
    want = torch.nn.functional.cross_entropy(old["logits"].double(), old["labels"]).item()
    assert new["loss"] == pytest.approx(want, abs=1e-4)
    assert int(new["confusion"].sum()) == 5 and new["nonfinite"] == 0 and new["bad_labels"] == 0
    meter = StreamMeter(K, topk=(1,), views=V, confusion=False)
    again = evaluate_streaming(net, batches, n_frames=T, views=V, meter=meter)
    assert again["top1"] == new["top1"] and "logits" not in again and meter.torch_updates == 2
