"""Crop / resize / flip on the device (rk_clip_resample_u8_*, rubiksnet_amd.augment) against the numpy restatement of
its definition (tests/_resample_ref.py, itself checked byte for byte against Pillow in tests/test_augment.py) and the
fixtures generated from the reference's transforms.  fp32 is bit-identical; bf16 is the fp32 result rounded once to
nearest-even.  Tiny tensors: every reference is computed once per session."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import _resample_ref as rr
from rubiksnet_amd import augment

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NPZ = sorted(os.path.basename(p)[len("augment_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "augment_*.npz")))

# name -> (B, T, Hs, Ws, V, (Sh, Sw), boxes, odd base offset)
CASES = {
    # 141-byte rows and x0 * 3 = 9: no source run is 16-byte aligned, the base is odd; 24 rows = a full band + a ragged
    # one; non-square; the two clips differ in box, crop size and flip; T = 3
    "misaligned_two_bands_flip_mix": (2, 3, 33, 47, 1, (24, 20), [(3, 2, 35, 28, 20, 24, 0, 0, 1), (5, 1, 21, 30, 20, 24, 0, 0, 0)], 1),
    # 7 x 6 -> 36 x 40: two taps everywhere, both edges clamp, three bands; T = 1
    "upscale_5x": (1, 1, 9, 11, 1, (40, 36), [(2, 1, 7, 6, 36, 40, 0, 0, 0)], 0),
    "identity_x_only": (1, 1, 34, 30, 1, (17, 20), [(3, 4, 20, 30, 20, 17, 0, 0, 1)], 3),
    "identity_y_only": (1, 2, 20, 30, 1, (16, 24), [(3, 4, 12, 16, 24, 16, 0, 0, 0)], 0),
    # ratios 7.74 / 6.76 (17 and 15 taps: one output row per pass of the row buffer) and 2.5 / 3.1
    "downscale_many_taps": (2, 1, 120, 150, 1, (17, 19), [(1, 2, 147, 115, 19, 17, 0, 0, 0), (40, 30, 48, 53, 19, 17, 0, 0, 1)], 0),
    # evaluation: the whole frame scaled to 28 x 20, three windows x flip mix per clip, V = 3
    "views3_scaled_windows": (2, 2, 33, 47, 3, (16, 16), [(0, 0, 47, 33, 28, 20, 0, 2, 0), (0, 0, 47, 33, 28, 20, 12, 2, 1),
                                                          (0, 0, 47, 33, 28, 20, 6, 4, 0), (0, 0, 47, 33, 28, 20, 12, 0, 0),
                                                          (0, 0, 47, 33, 28, 20, 0, 4, 1), (0, 0, 47, 33, 28, 20, 6, 2, 1)], 0),
    # the second clip's box ends on the last row and column of the last frame of the allocation
    "last_row_and_column": (2, 2, 25, 31, 1, (8, 8), [(0, 0, 31, 25, 8, 8, 0, 0, 0), (21, 13, 10, 12, 8, 8, 0, 0, 0)], 0),
}


def _frames(name):
    B, T, Hs, Ws = CASES[name][:4]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    return rng.integers(0, 256, (B, T, Hs, Ws, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _want(name):
    """The fp32 reference of a case, computed once and shared (read-only) by the fp32 and bf16 tests."""
    B, T, Hs, Ws, V, out_hw, boxes, _ = CASES[name]
    want = rr.clips_f32(_frames(name), np.asarray(boxes, dtype=np.int32), out_hw, views=V)
    want.setflags(write=False)
    return want


def _device_frames(frames, offset):
    """The frames on the device, `offset` bytes into an allocation (so the base is as misaligned as asked)."""
    buf = torch.empty(frames.size + offset, dtype=torch.uint8, device=DEV)
    view = buf[offset:].view(frames.shape)
    view.copy_(torch.from_numpy(frames))
    assert view.is_contiguous() and view.data_ptr() % 16 == offset % 16
    return view


def _same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_is_bit_identical_to_the_definition(name):
    B, T, Hs, Ws, V, out_hw, boxes, offset = CASES[name]
    frames = _device_frames(_frames(name), offset)
    got = augment.frames_u8_to_clips(frames, torch.tensor(boxes, dtype=torch.int32), out_hw, views=V)
    assert tuple(got.shape) == (B * V, T, 3) + tuple(out_hw) and got.dtype == torch.float32
    got = got.cpu().numpy()
    want = _want(name)
    assert _same_bits(got, want), "%d of %d elements differ, max |diff| %g" % (
        (got != want).sum(), want.size, np.abs(got - want).max())


@pytest.mark.parametrize("name", ["misaligned_two_bands_flip_mix", "downscale_many_taps", "views3_scaled_windows"])
def test_bf16_is_the_fp32_result_rounded_once(name):
    B, T, Hs, Ws, V, out_hw, boxes, offset = CASES[name]
    frames = _device_frames(_frames(name), offset)
    dev_boxes = torch.tensor(boxes, dtype=torch.int32).to(DEV)                 # device boxes: trusted, not copied
    out = torch.empty(B * V, T, 3, *out_hw, dtype=torch.bfloat16, device=DEV)
    got = augment.frames_u8_to_clips(frames, dev_boxes, out_hw, views=V, dtype=torch.bfloat16, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = torch.from_numpy(np.array(_want(name))).to(torch.bfloat16)          # round to nearest even, once
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("name", NPZ)
def test_matches_the_reference_transforms(name):
    """Bit-identical to the reference's GroupMultiScaleCrop (+ flip) / GroupFullResSample / GroupOverSample / scale +
    centre crop, then Stack -> ToTorchFormatTensor -> GroupNormalize (fixtures of tests/golden/gen_augment_golden.py)."""
    g = np.load(os.path.join(GOLDEN, "augment_%s.npz" % name))
    want = g["out"]
    V, T, _, sh, sw = want.shape
    got = augment.frames_u8_to_clips(torch.from_numpy(g["frames"]).to(DEV), torch.from_numpy(g["boxes"]), (sh, sw), views=V,
                                     mean=tuple(g["mean"]), std=tuple(g["std"]))
    assert _same_bits(got.cpu().numpy(), want)


def test_python_entry_point_checks_its_arguments():
    frames = torch.zeros(2, 2, 12, 14, 3, dtype=torch.uint8, device=DEV)
    ok = torch.tensor([(0, 0, 14, 12, 8, 8, 0, 0, 0)] * 2, dtype=torch.int32)
    assert augment.frames_u8_to_clips(frames, ok, 8).shape == (2, 2, 3, 8, 8)
    with pytest.raises(ValueError, match="outside the frame"):
        augment.frames_u8_to_clips(frames, torch.tensor([(0, 0, 14, 12, 8, 8, 0, 0, 0), (1, 0, 14, 12, 8, 8, 0, 0, 0)],
                                                        dtype=torch.int32), 8)
    with pytest.raises(ValueError, match=r"\[4, 9\]"):
        augment.frames_u8_to_clips(frames, ok, 8, views=2)
    with pytest.raises(ValueError, match="dtype"):
        augment.frames_u8_to_clips(frames, ok, 8, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="out must be"):
        augment.frames_u8_to_clips(frames, ok, 8, out=torch.empty(2, 2, 3, 8, 9, device=DEV))
    with pytest.raises(RuntimeError, match="contiguous"):
        augment.frames_u8_to_clips(frames[:, :, :, ::2], ok, 8)


def test_loader_draws_fresh_boxes_and_matches_the_definition():
    """Three batches from a two-slot loader: each is the definition applied to the slot's frames with the boxes drawn for
    it, and the slot that comes round again got new boxes."""
    loader = augment.SyntheticFrameLoader(3, n_frames=2, frame_hw=(40, 52), size=16, num_classes=5, device=DEV, seed=3)
    seen = []
    for i in range(3):
        slot = i % 2
        clips, labels = next(loader)
        torch.cuda.synchronize()
        boxes = loader._host_boxes[slot].clone()
        assert tuple(clips.shape) == (3, 2, 3, 16, 16) and torch.equal(labels.cpu(), loader._labels[slot])
        want = rr.clips_f32(loader._host[slot].numpy(), boxes.numpy(), (16, 16))
        assert _same_bits(clips.cpu().numpy(), want), i
        seen.append(boxes)
    assert not torch.equal(seen[0], seen[2])


def test_loader_feeds_three_view_evaluation():
    """loader (full-resolution boxes, V = 3) -> evaluation.evaluate(views=3) on RubiksNet-Tiny, 2 videos."""
    from rubiksnet_amd import RubiksNet
    from rubiksnet_amd.evaluation import evaluate

    B, T, V, S = 2, 8, 3, 224
    loader = augment.SyntheticFrameLoader(B, n_frames=T, size=S, num_classes=7, device=DEV, views=V,
                                          box_fn=lambda n, gen: augment.full_res_boxes(n, (256, 340), S, flip=False))
    clips, labels = next(loader)
    assert tuple(clips.shape) == (B * V, T, 3, S, S)
    torch.cuda.synchronize()
    # no scaling: the resampler is the identity, so the three views are plain windows of the frames
    frames = loader._host[0].numpy()
    for oc, (ox, oy) in enumerate([(0, 16), (116, 16), (58, 16)] * B):
        win = frames[oc // V, :, oy:oy + S, ox:ox + S].transpose(0, 3, 1, 2)
        assert _same_bits(clips[oc].cpu().numpy(), rr.normalise(win, augment.IMAGENET_MEAN, augment.IMAGENET_STD)), oc
    net = RubiksNet("tiny", num_classes=7, num_frames=T, verbose=False).to(DEV).eval()
    res = evaluate(net, [(clips.view(B, V * T * 3, S, S), labels)], n_frames=T, views=V)
    assert res["videos"] == B and tuple(res["logits"].shape) == (B, 7) and torch.isfinite(res["logits"]).all()
