"""The streaming metrics launch (rk_metrics.hip through rubiksnet_amd.metrics.StreamMeter) on the device, against the
integer / fp64 host reference of tests/_metrics_ref.py (inputs and tolerances: that module's docstring)."""
import copy

import numpy as np
import pytest
import torch

import _metrics_ref as mr
from rubiksnet_amd import dp
from rubiksnet_amd.metrics import OUTPUTS, StreamMeter

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
LARGE_K = 4099            # above rk_metrics.hip's kZLds = 4096: the consensus is formed again in the second pass
GUARD = 64
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _dev(x, y, dtype):
    B, V, K = x.shape
    return torch.from_numpy(np.array(x)).to(dtype).reshape(B * V, K).to(DEV), torch.from_numpy(np.array(y)).to(DEV)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _guarded(meter):
    """The meter's state as a slice between guard words of one allocation."""
    big = torch.full((GUARD + meter.words + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    big[GUARD:GUARD + meter.words] = 0
    meter.state = big[GUARD:GUARD + meter.words]
    return big


def _guards_intact(big, words):
    host = big.cpu()
    return bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + words:] == SENTINEL).all())


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_state_and_outputs_match_the_reference_on_the_grid(sfx):
    for K in mr.GRID_K:
        for V in mr.GRID_V:
            for B in mr.GRID_B:
                x, y, ref = mr.grid_case(B, V, K, mr.UNIT[sfx])
                meter = StreamMeter(K, topk=(1, 5), views=V)
                out = meter.update(*_dev(x, y, DTYPES[sfx]), outputs=OUTPUTS)
                what = "%s K=%d V=%d B=%d" % (sfx, K, V, B)
                mr.check_outputs(_host(out), ref, what)
                mr.check_state(meter.state.cpu().numpy(), ref, what)
                assert (meter.native_updates, meter.torch_updates) == (1, 0)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_classes_beyond_the_on_chip_consensus(sfx):
    x, y = mr.make_case(41, 3, 2, LARGE_K, mr.UNIT[sfx])
    ref = mr.reference(x, y, (1, 5, 5000), False, mr.UNIT[sfx])
    meter = StreamMeter(LARGE_K, topk=(1, 5, 5000), views=2, confusion=False)
    big = _guarded(meter)
    out = meter.update(*_dev(x, y, DTYPES[sfx]), outputs=OUTPUTS)
    mr.check_outputs(_host(out), ref, sfx)
    mr.check_state(meter.state.cpu().numpy(), ref, sfx)
    assert ref["state"][6] == 3 and _guards_intact(big, meter.words) and meter.native_updates == 1


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_bad_labels_and_nonfinite_logits_inside_guard_words(sfx):
    """Labels -1 and K count in bad_labels only; a NaN, a +inf and a -inf in single views make their videos misses at every
    k; every other word is exact, and nothing outside the state is written."""
    K, V, B = 65, 3, 9
    x, y = mr.make_case(5, B, V, K, mr.UNIT[sfx])
    y[1], y[4] = -1, K
    x[2, 1, 7], x[5, 0, 64], x[7, 2, 0] = np.nan, np.inf, -np.inf
    ref = mr.reference(x, y, (1, 5), True, mr.UNIT[sfx])
    assert ref["state"][0] == 7 and ref["state"][2] == 3 and ref["state"][3] == 2
    meter = StreamMeter(K, views=V)
    big = _guarded(meter)
    out = meter.update(*_dev(x, y, DTYPES[sfx]), outputs=OUTPUTS)
    mr.check_outputs(_host(out), ref, sfx)
    mr.check_state(meter.state.cpu().numpy(), ref, sfx)
    # far-off labels and a batch of nothing but bad labels
    far = torch.tensor([2 ** 40, -2 ** 40, K * K, -(2 ** 31) - 1, 2 ** 31, 2 ** 32, K + 1, -K, 2 ** 62], device=DEV)
    meter.update(_dev(x, y, DTYPES[sfx])[0], far)
    want = ref["state"].copy()
    want[3] += B
    mr.check_state(meter.state.cpu().numpy(), dict(ref, state=want), sfx)
    assert _guards_intact(big, meter.words) and meter.native_updates == 2
    res = meter.result()
    assert (res["videos"], res["nonfinite"], res["bad_labels"]) == (7, 3, 2 + B)
    assert res["top1"] == 100.0 * int(ref["state"][4]) / 7


def test_three_updates_on_a_side_stream_and_run_to_run_bits():
    K, V = 174, 3
    parts = [mr.make_case(60 + i, B, V, K, 2.0 ** -6) for i, B in enumerate((33, 5, 17))]
    ref = mr.add([mr.reference(x, y, (1, 5), True, 2.0 ** -6) for x, y in parts])
    dev_parts = [_dev(x, y, torch.float32) for x, y in parts]
    side = torch.cuda.Stream(DEV)
    states = []
    for _ in range(2):
        meter = StreamMeter(K, views=V)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            for logits, labels in dev_parts:
                meter.update(logits, labels)             # back to back: nothing between them waits
        side.synchronize()
        assert meter.native_updates == 3
        states.append(meter.state.cpu())
    mr.check_state(states[0].numpy(), ref)
    assert torch.equal(states[0], states[1])


def test_without_the_confusion_matrix():
    K, V, B = 174, 3, 33
    x, y, ref = mr.grid_case(B, V, K, 2.0 ** -6)
    meter = StreamMeter(K, views=V, confusion=False)
    big = _guarded(meter)
    meter.update(*_dev(x, y, torch.float32))
    assert meter.state.numel() == 8 + 2 * K
    mr.check_state(meter.state.cpu().numpy(), dict(ref, state=ref["state"][:8 + 2 * K]))
    assert _guards_intact(big, meter.words) and meter.result()["confusion"] is None


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_native_and_torch_paths_agree(sfx):
    K, V, B = 174, 3, 33
    x, y = mr.make_case(8, B, V, K, mr.UNIT[sfx])
    y[3], x[9, 2, 100] = K, np.nan
    logits, labels = _dev(x, y, DTYPES[sfx])
    native, twin = StreamMeter(K, views=V), StreamMeter(K, views=V)
    twin.native = False
    a = _host(native.update(logits, labels, outputs=OUTPUTS))
    b = _host(twin.update(logits, labels, outputs=OUTPUTS))
    assert (native.native_updates, native.torch_updates, twin.native_updates, twin.torch_updates) == (1, 0, 0, 1)
    sa, sb = native.state.cpu(), twin.state.cpu()
    assert abs(int(sa[1]) - int(sb[1])) <= B * mr.LOSS_TOL * 2.0 ** 32
    sa[1] = sb[1] = 0
    assert torch.equal(sa, sb)
    for name in ("consensus", "pred", "rank"):
        assert np.array_equal(a[name], b[name], equal_nan=True), name
    assert np.array_equal(np.isnan(a["loss"]), np.isnan(b["loss"])) and np.nanmax(np.abs(a["loss"] - b["loss"])) <= mr.LOSS_TOL
    merged = StreamMeter(K, views=V).merge(native).merge(twin)          # states of the two paths add up
    assert merged.result()["videos"] == 2 * (B - 1) and merged.result()["nonfinite"] == 2


def test_train_step_with_a_meter_is_the_same_step():
    from rubiksnet_amd import RubiksNet

    torch.manual_seed(11)
    net = RubiksNet("tiny", 11, num_frames=8, verbose=False).to(DEV).train()
    twin = copy.deepcopy(net)
    clips = torch.randn(2, 8, 3, 224, 224, device=DEV)
    labels = torch.randint(0, 11, (2,), device=DEV)
    meter = StreamMeter(11, topk=(1, 5))
    loss = dp.train_step(net, dp.make_optimizer(net, lr=0.1, kind="sgd", momentum=0.0), clips, labels, meter=meter)
    want = dp.train_step(twin, dp.make_optimizer(twin, lr=0.1, kind="sgd", momentum=0.0), clips, labels)
    assert loss.dtype == torch.float32 and torch.equal(loss.detach().view(torch.int32), want.detach().view(torch.int32))
    for (name, p), q in zip(net.state_dict().items(), twin.state_dict().values()):
        assert torch.equal(p, q), name
    res = meter.result()
    assert meter.native_updates == 1 and res["videos"] == 2 and res["nonfinite"] == 0
    assert abs(res["loss"] - float(loss.detach())) <= mr.LOSS_TOL


def test_evaluate_streaming_reports_what_evaluate_reports():
    """loader (full-resolution boxes, V = 3) -> RubiksNet-Tiny, 2 videos: the case of tests/test_augment_gpu.py."""
    from rubiksnet_amd import RubiksNet, augment
    from rubiksnet_amd.evaluation import evaluate, evaluate_streaming

    B, T, V, S = 2, 8, 3, 224
    loader = augment.SyntheticFrameLoader(B, n_frames=T, size=S, num_classes=7, device=DEV, views=V,
                                          box_fn=lambda n, gen: augment.full_res_boxes(n, (256, 340), S, flip=False))
    clips, labels = next(loader)
    net = RubiksNet("tiny", num_classes=7, num_frames=T, verbose=False).to(DEV).eval()
    batches = [(clips.view(B, V * T * 3, S, S), labels)]
    old = evaluate(net, batches, n_frames=T, views=V)
    meter = StreamMeter(7, topk=(1, 5), views=V)
    new = evaluate_streaming(net, batches, n_frames=T, views=V, meter=meter, keep_logits=True)
    assert meter.native_updates == 1 and meter.torch_updates == 0
    assert new["videos"] == old["videos"] == B
    assert new["top1"] == old["top1"] and new["top5"] == old["top5"]       # (0, 50 or 100: exact in evaluate's fp32 too)
    assert tuple(new["logits"].shape) == (B, 7) and torch.equal(new["labels"], old["labels"])
    assert torch.allclose(new["logits"], old["logits"], atol=1e-5, rtol=1e-5)
    assert int(new["confusion"].sum()) == B
