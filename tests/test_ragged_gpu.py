"""The ragged crop / resize / flip entry (rk_clip_resample_ragged_u8_*, augment.ragged_u8_to_clips) and the two feeders on
it (dataset.FrameLoader, dataset.DeviceFrameCache): against the reference's transforms through the existing fixtures,
against the numpy restatement of the definition (tests/_resample_ref.py), against rk_clip_resample_u8_* on a uniform
batch, and with tables that lie.  fp32 is bit-identical; bf16 is that rounded once.  Tiny tensors throughout."""
import functools
import os

import numpy as np
import pytest
import torch

import _resample_ref as rr
from rubiksnet_amd import augment, dataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32))


def _pack(videos):
    """numpy videos [F, H, W, 3] -> (arena uint8 tensor, clips int64 [B, 4]) through the collate function."""
    arena, clips, _ = dataset.pack_clips([(torch.from_numpy(np.ascontiguousarray(v)), 0) for v in videos])
    return arena, clips


def _definition(arena, clips, frame_idx, boxes, out_hw, views, mean=augment.IMAGENET_MEAN, std=augment.IMAGENET_STD):
    """The definition in numpy from the very tables the kernel gets: output frame (oc, t) is frame frame_idx[oc, t] of
    record oc // views under box oc."""
    arena, clips = np.asarray(arena), np.asarray(clips)
    frame_idx, boxes = np.asarray(frame_idx), np.asarray(boxes)
    out = np.empty((frame_idx.shape[0], frame_idx.shape[1], 3) + tuple(out_hw), dtype=np.uint8)
    for oc in range(frame_idx.shape[0]):
        off, h, w, nf = (int(v) for v in clips[oc // views])
        video = arena[off:off + nf * h * w * 3].reshape(nf, h, w, 3)
        for t, f in enumerate(frame_idx[oc]):
            assert 0 <= f < nf, (oc, t, f, nf)
            out[oc, t] = rr.frame_u8(video[int(f)], boxes[oc], out_hw).transpose(2, 0, 1)
    return rr.normalise(out, mean, std)


def _fixture(name):
    return np.load(os.path.join(GOLDEN, "augment_%s.npz" % name))


# ------------------------------------------------------------------------------------------------- the reference's transforms
@pytest.mark.parametrize("names, order", [(("train_b", "train_c"), None), (("train_a", "train_d"), [0, 2, 1])])
def test_two_sizes_in_one_arena_match_the_reference_transforms(names, order):
    """train_b (33x47) + train_c (40x52) -> 24 (two bands), T = 2; train_a + train_d -> 16 with frames [0, 2, 1]."""
    g = [_fixture(n) for n in names]
    T, size = g[0]["out"].shape[1], g[0]["out"].shape[-1]
    assert [x["frames"].shape[2:4] for x in g] in ([(33, 47), (40, 52)], [(40, 52), (33, 47)]) and g[1]["out"].shape[1] == T
    order = list(range(T)) if order is None else order
    arena, clips = _pack([x["frames"][0] for x in g])
    frame_idx = torch.tensor([order, order], dtype=torch.int32)
    boxes = torch.from_numpy(np.concatenate([x["boxes"] for x in g]))
    want = np.concatenate([x["out"][:, order] for x in g])
    mean, std = tuple(g[0]["mean"]), tuple(g[0]["std"])
    got = augment.ragged_u8_to_clips(arena.to(DEV), clips, frame_idx, boxes, size, mean=mean, std=std)
    assert tuple(got.shape) == (2, T, 3, size, size) and _same_bits(got.cpu().numpy(), want)
    got16 = augment.ragged_u8_to_clips(arena.to(DEV), clips, frame_idx, boxes, size, mean=mean, std=std, dtype=torch.bfloat16)
    assert torch.equal(got16.cpu().view(torch.int16), torch.from_numpy(want).to(torch.bfloat16).view(torch.int16))


# ------------------------------------------------------------------------------------------------- the definition
MIXED_HW = [(33, 47), (40, 52), (17, 91)]
MIXED_F = [3, 3, 5]
MIXED_OUT = (10, 12)
# three views per video: a plain crop, a flipped one, and a scaled whole frame with a window; the third video's first view
# shrinks 88 columns to 12 (7.3: 16 taps) and 17 rows to 10
MIXED_BOXES = [(3, 2, 35, 28, 12, 10, 0, 0, 0), (5, 1, 21, 30, 12, 10, 0, 0, 1), (0, 0, 47, 33, 28, 20, 9, 4, 1),
               (0, 0, 52, 40, 12, 10, 0, 0, 1), (11, 7, 30, 30, 12, 10, 0, 0, 0), (0, 0, 52, 40, 26, 20, 14, 10, 0),
               (1, 0, 88, 17, 12, 10, 0, 0, 0), (40, 3, 24, 12, 12, 10, 0, 0, 1), (0, 0, 91, 17, 64, 12, 31, 1, 1)]
# repeated, reversed and out-of-order indices, each inside its own video
MIXED_IDX = [[0, 0, 2], [2, 2, 1], [1, 2, 1], [2, 1, 0], [0, 2, 2], [1, 1, 1], [4, 0, 2], [4, 3, 2], [0, 4, 4]]


@functools.lru_cache(maxsize=None)
def _mixed():
    rng = np.random.default_rng(21)
    videos = [rng.integers(0, 256, (f, h, w, 3), dtype=np.uint8) for f, (h, w) in zip(MIXED_F, MIXED_HW)]
    arena, clips = _pack(videos)
    assert clips[:, 0].tolist() == [0, 13959, 32679]              # an odd offset; odd row pitches too: 141, 273
    frame_idx = torch.tensor(MIXED_IDX, dtype=torch.int32)
    boxes = torch.tensor(MIXED_BOXES, dtype=torch.int32)
    want = _definition(arena.numpy(), clips, frame_idx, boxes, MIXED_OUT, 3)
    want.setflags(write=False)
    return arena, clips, frame_idx, boxes, want


def test_mixed_batch_is_bit_identical_to_the_definition():
    arena, clips, frame_idx, boxes, want = _mixed()
    got = augment.ragged_u8_to_clips(arena.to(DEV), clips, frame_idx, boxes, MIXED_OUT, views=3)
    assert tuple(got.shape) == (9, 3, 3) + MIXED_OUT and got.dtype == torch.float32
    got = got.cpu().numpy()
    assert _same_bits(got, want), "%d of %d elements differ" % ((got != want).sum(), want.size)


def test_mixed_batch_at_an_odd_base_in_bf16_with_device_tables():
    """The arena one byte into its allocation (every video at an odd address), tables already on the device, out given."""
    arena, clips, frame_idx, boxes, want = _mixed()
    buf = torch.empty(arena.numel() + 1, dtype=torch.uint8, device=DEV)
    dev_arena = buf[1:]
    dev_arena.copy_(arena)
    assert dev_arena.data_ptr() % 2 == 1
    out = torch.empty(9, 3, 3, *MIXED_OUT, dtype=torch.bfloat16, device=DEV)
    got = augment.ragged_u8_to_clips(dev_arena, clips.to(DEV), frame_idx.to(DEV), boxes.to(DEV), MIXED_OUT, views=3,
                                     dtype=torch.bfloat16, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got.cpu().view(torch.int16), torch.from_numpy(np.array(want)).to(torch.bfloat16).view(torch.int16))


def test_uniform_batch_equals_the_uniform_entry_bit_for_bit():
    """B = 2, T = 3, 33x47, two views, 24 x 20 output (a full band and a ragged one), identity indices."""
    rng = np.random.default_rng(22)
    frames = rng.integers(0, 256, (2, 3, 33, 47, 3), dtype=np.uint8)
    boxes = torch.tensor([(3, 2, 35, 28, 20, 24, 0, 0, 1), (5, 1, 21, 30, 20, 24, 0, 0, 0),
                          (0, 0, 47, 33, 40, 28, 13, 3, 0), (0, 0, 47, 33, 20, 24, 0, 0, 1)], dtype=torch.int32)
    dev_frames = torch.from_numpy(frames).to(DEV)
    arena, clips = _pack(list(frames))
    frame_idx = torch.arange(3, dtype=torch.int32).repeat(4, 1)
    for dtype, bits in ((torch.float32, torch.int32), (torch.bfloat16, torch.int16)):
        want = augment.frames_u8_to_clips(dev_frames, boxes, (24, 20), views=2, dtype=dtype)
        got = augment.ragged_u8_to_clips(dev_frames.view(-1), clips, frame_idx, boxes, (24, 20), views=2, dtype=dtype)
        assert tuple(got.shape) == (4, 3, 3, 24, 20) and torch.equal(got.view(bits), want.view(bits))
        if dtype == torch.float32:
            assert _same_bits(got.cpu().numpy(), _definition(arena.numpy(), clips, frame_idx, boxes, (24, 20), 2))


# ------------------------------------------------------------------------------------------------- tables that lie
def test_a_record_past_the_arena_gives_zeros_and_indices_are_clamped():
    """Everything the kernel could reach lies in one allocation the test owns: [canary | arena | canary].  The arena's
    bytes are below 128 and the canaries are 255, so a canary byte under any tap lifts an output above what the arena can
    give.  The middle record of the table claims one frame more than the arena holds (the claim ends inside the trailing
    canary, never outside the allocation): its two output clips are zeros, the clips around it are right.  Indices -3
    and F + 5 show the first and the last frame."""
    rng = np.random.default_rng(23)
    hw, F = [(12, 15), (9, 21), (14, 11)], [3, 2, 3]
    videos = [rng.integers(0, 128, (f, h, w, 3), dtype=np.uint8) for f, (h, w) in zip(F, hw)]
    arena, clips = _pack(videos)
    margin = 14 * 11 * 3 * 2                                            # two frames of the last video: more than the lie
    buf = torch.full((margin + arena.numel() + margin,), 255, dtype=torch.uint8, device=DEV)
    dev_arena = buf[margin:margin + arena.numel()]
    dev_arena.copy_(arena)
    table = clips[[0, 2, 1]].clone()                                    # table order is not arena order
    honest = table.clone()
    table[1, 3] = F[2] + 1                                              # the last video of the arena, one frame too many
    assert table[1, 0] + table[1, 3] * 14 * 11 * 3 > arena.numel()
    assert table[1, 0] + table[1, 3] * 14 * 11 * 3 <= arena.numel() + margin
    frame_idx = torch.tensor([[-3, F[0] + 5], [1, 0], [0, 3], [3, 3], [-3, F[1] + 5], [2 ** 31 - 1, -2 ** 31]], dtype=torch.int32)
    clamped = torch.tensor([[0, F[0] - 1], [1, 0], [0, 2], [2, 2], [0, F[1] - 1], [F[1] - 1, 0]], dtype=torch.int32)
    boxes = torch.tensor([(0, 0, 15, 12, 8, 8, 0, 0, 0), (2, 1, 12, 10, 8, 8, 0, 0, 1), (0, 0, 11, 14, 8, 8, 0, 0, 0),
                          (1, 2, 9, 9, 8, 8, 0, 0, 1), (0, 0, 21, 9, 16, 8, 5, 0, 0), (4, 0, 16, 9, 8, 8, 0, 0, 1)],
                         dtype=torch.int32)
    augment.check_ragged(arena.numel(), honest, clamped, boxes, 8, views=2)
    with pytest.raises(ValueError, match="clip 1: .*outside the arena"):
        augment.check_ragged(arena.numel(), table, clamped, boxes, 8, views=2)
    with pytest.raises(ValueError, match="clip 0: frame index"):
        augment.check_ragged(arena.numel(), honest, frame_idx, boxes, 8, views=2)
    got = augment.ragged_u8_to_clips(dev_arena, table.to(DEV), frame_idx.to(DEV), boxes.to(DEV), 8, views=2).cpu().numpy()
    want = _definition(arena.numpy(), honest, clamped, boxes, (8, 8), 2)
    assert _same_bits(got[[0, 1, 4, 5]], want[[0, 1, 4, 5]])
    assert not got[2:4].any()
    ceiling = rr.normalise(np.full((3, 1, 1), 127, dtype=np.uint8), augment.IMAGENET_MEAN, augment.IMAGENET_STD).reshape(3, 1, 1)
    assert (got <= ceiling).all()                                       # no canary byte under any tap
    # the other ways a record can lie, each decided from the record alone: all their clips are zeros
    for field, value in ((0, -1), (1, 0), (2, 16385), (3, 0), (0, arena.numel() + 1), (3, 2 ** 62)):
        lie = honest.clone()
        lie[0, field] = value
        out = augment.ragged_u8_to_clips(dev_arena, lie.to(DEV), clamped.to(DEV), boxes.to(DEV), 8, views=2).cpu().numpy()
        assert not out[:2].any() and _same_bits(out[2:], _definition(arena.numpy(), honest, clamped, boxes, (8, 8), 2)[2:]), (
            field, value)


# ------------------------------------------------------------------------------------------------- feeders
def _videos(seed, shapes):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, 256, s + (3,), dtype=np.uint8)) for s in shapes]


FEED_SHAPES = [(9, 33, 47), (12, 40, 52), (7, 30, 61)]


def test_frame_loader_yields_the_definition_of_what_it_reports():
    videos = _videos(31, FEED_SHAPES)
    ds = dataset.InMemoryVideos(videos, [4, 1, 3], num_segments=3, generator=torch.Generator().manual_seed(2))
    loader = dataset.FrameLoader(ds, 2, "train", device=DEV, size=16, num_workers=0, seed=5, shuffle=False)
    assert len(loader) == 2 and loader.views == 1
    seen = []
    for epoch in range(2):                                          # the second epoch reuses both slots
        for i, (clips, labels) in enumerate(loader):
            torch.cuda.synchronize()
            t = loader.tables
            n = 2 if i == 0 else 1
            assert tuple(clips.shape) == (n, 3, 3, 16, 16) and labels.tolist() == [4, 1, 3][2 * i:2 * i + n]
            assert t["clips"][:, 1:3].tolist() == [list(s[1:]) for s in FEED_SHAPES[2 * i:2 * i + n]]
            want = _definition(t["arena"].numpy(), t["clips"], t["frame_idx"], t["boxes"], (16, 16), 1)
            assert _same_bits(clips.cpu().numpy(), want), (epoch, i)
            seen.append(t["boxes"].clone())
    assert not torch.equal(seen[0], seen[2])                        # fresh boxes every epoch


def test_device_frame_cache_yields_the_definition_of_what_it_reports():
    videos = _videos(31, FEED_SHAPES)
    with pytest.raises(RuntimeError, match="over the budget"):
        dataset.DeviceFrameCache(list(zip(videos, [4, 1, 3])), 2, "train", device=DEV, size=16, num_segments=3,
                                 budget_bytes=100000)
    cache = dataset.DeviceFrameCache(list(zip(videos, [4, 1, 3])), 2, "train", device=DEV, size=16, seed=5, shuffle=False,
                                     num_segments=3, budget_bytes=1 << 20)
    assert len(cache) == 2 and cache.arena.is_cuda and cache.arena.numel() == sum(v.numel() for v in videos)
    host_arena = torch.cat([v.reshape(-1) for v in videos]).numpy()
    for i, (clips, labels) in enumerate(cache):
        t = cache.tables
        n = 2 if i == 0 else 1
        assert tuple(clips.shape) == (n, 3, 3, 16, 16) and labels.tolist() == [4, 1, 3][2 * i:2 * i + n]
        assert t["frame_idx"].shape == (n, 3) and (t["frame_idx"] % 2 == 1).all()      # even frame numbers, 0-based
        want = _definition(host_arena, t["clips"], t["frame_idx"], t["boxes"], (16, 16), 1)
        assert _same_bits(clips.cpu().numpy(), want), i


def test_two_clip_three_crop_feed_through_streaming_evaluation():
    """2 videos x (3 full-resolution crops x 2 temporal clips) from a twice_sample test set -> evaluate_streaming on
    RubiksNet-Tiny; the same six views per video made by hand with the uniform entry give the same clips and logits."""
    from rubiksnet_amd import RubiksNet
    from rubiksnet_amd.evaluation import evaluate_streaming

    T, S = 8, 224
    videos = _videos(41, [(20, 230, 250), (17, 226, 300)])
    ds = dataset.InMemoryVideos(videos, [2, 5], num_segments=T, test_mode=True, twice_sample=True)
    box_fn = lambda hw, gen: augment.full_res_boxes(1, hw, S, flip=False)      # noqa: E731
    loader = dataset.FrameLoader(ds, 2, "test", device=DEV, size=S, views=3, box_fn=box_fn, num_workers=0)
    assert loader.temporal_clips == 2 and loader.views == 6
    batches = [(c.view(c.shape[0] // 6, -1, S, S).clone(), l.clone()) for c, l in loader]
    assert len(batches) == 1 and tuple(batches[0][0].shape) == (2, 6 * T * 3, S, S)
    by_hand = []
    for v in videos:
        idx = torch.from_numpy(dataset.segment_indices(v.shape[0], T, "test", twice_sample=True)) - 1
        boxes = augment.full_res_boxes(1, tuple(v.shape[1:3]), S, flip=False)
        for c in range(3):
            for k in range(2):                                      # crop-major, temporal clip minor
                frames = v[idx[k * T:(k + 1) * T]].unsqueeze(0).contiguous().to(DEV)
                by_hand.append(augment.frames_u8_to_clips(frames, boxes[c:c + 1], S))
    by_hand = torch.cat(by_hand)
    assert torch.equal(batches[0][0].view(12, T, 3, S, S), by_hand)
    cache = dataset.DeviceFrameCache(ds, 2, "test", device=DEV, size=S, views=3, box_fn=box_fn)
    assert torch.equal(next(iter(cache))[0], by_hand)

    net = RubiksNet("tiny", num_classes=7, num_frames=T, verbose=False).to(DEV).eval()
    res = evaluate_streaming(net, batches, n_frames=T, views=6, keep_logits=True)
    with torch.no_grad():
        per_view = net(by_hand).float()
    want, m = per_view.view(2, 6, -1).mean(1).cpu(), float(per_view.abs().max())
    assert res["videos"] == 2 and res["labels"].tolist() == [2, 5]
    # the same 12 clips in the same order through the same network: the only freedom is how the six-term mean is summed.
    # With |logit| <= m: five adds of partial sums <= 6 m err at most 30 m 2^-24, a sixth of that after the division, one
    # more rounding for it: 6 m 2^-24 from the exact mean per side, 12 m 2^-24 between two orders
    torch.testing.assert_close(res["logits"], want, rtol=0, atol=12 * m * 2.0 ** -24)
