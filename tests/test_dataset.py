"""rubiksnet_amd.dataset on the host: the frame sampling pinned against the reference's (tests/golden/dataset_indices.json,
written by tests/golden/gen_dataset_golden.py from rubiksnet/dataset/core.py), the dataset over frame folders, the
collate function, and the argument checks of the ragged device entry.  No device."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from rubiksnet_amd import augment, dataset

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _golden():
    with open(os.path.join(GOLDEN, "dataset_indices.json")) as fh:
        return json.load(fh)


def _cases():
    for key, want in _golden()["cases"].items():
        nf, ns, split, nl, flags = key.split(",")
        dense, alls, twice, even = (c == "1" for c in flags)
        yield key, want, (int(nf), int(ns), split), dict(new_length=int(nl), dense_sample=dense, all_sample=alls,
                                                         twice_sample=twice, only_even_indices=even)


def _with_draws(monkeypatch, pick):
    """Replace the sampling hook by one that answers every draw with pick(bound) and records the bounds."""
    bounds = []

    def draw(bound, size, generator=None):
        bounds.append(int(bound))
        return np.full(1 if size is None else size, pick(bound), dtype=np.int64)

    monkeypatch.setattr(dataset, "_draw", draw)
    return bounds


def test_the_fixture_covers_what_the_issue_lists():
    g = _golden()
    assert g["num_frames"] == [2, 3, 7, 8, 9, 16, 17, 40, 63, 64, 65, 130] and g["num_segments"] == [8, 16]
    assert len(g["cases"]) == 12 * 2 * 3 * len(g["new_length"]) * 16
    assert not any("error" in c for c in g["cases"].values())
    assert sum("bounds" in c for c in g["cases"].values()) > 100


@pytest.mark.parametrize("which, pick", [("lo", lambda b: 0), ("hi", lambda b: b - 1)])
def test_indices_and_bounds_equal_the_reference(monkeypatch, which, pick):
    bounds = _with_draws(monkeypatch, pick)
    for key, want, args, kw in _cases():
        del bounds[:]
        got = dataset.segment_indices(*args, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.int64, key
        assert got.tolist() == want.get(which, want["lo"]), key
        assert bounds == want.get("bounds", []), key


def test_real_draws_stay_inside_the_reference_bounds(monkeypatch):
    real = dataset._draw
    seen = []

    def draw(bound, size, generator=None):
        v = real(bound, size, generator)
        seen.append((int(bound), np.asarray(v)))
        assert len(v) == (1 if size is None else size)
        return v

    monkeypatch.setattr(dataset, "_draw", draw)
    gen = torch.Generator().manual_seed(5)
    for key, want, args, kw in _cases():
        if "bounds" not in want:
            continue
        del seen[:]
        got = dataset.segment_indices(*args, generator=gen, **kw)
        assert [b for b, _ in seen] == want["bounds"], key
        assert all(0 <= v.min() and v.max() < b for b, v in seen), key
        lo, hi = np.asarray(want["lo"]), np.asarray(want["hi"])
        assert got.shape == lo.shape and got.min() >= 1 and got.max() <= max(args[0], 2), key
        if not (kw["dense_sample"] or kw["all_sample"]) and len(want["bounds"]) == 1 and want["bounds"][0] * args[1] <= args[0]:
            assert ((lo <= got) & (got <= hi)).all(), key          # a per-segment jitter: each index between the two pins


def test_generator_makes_the_draws_repeatable():
    a = dataset.segment_indices(130, 8, "train", generator=torch.Generator().manual_seed(1))
    b = dataset.segment_indices(130, 8, "train", generator=torch.Generator().manual_seed(1))
    c = [dataset.segment_indices(130, 8, "train", generator=torch.Generator().manual_seed(s)).tolist() for s in range(2, 8)]
    assert a.tolist() == b.tolist() and any(x != a.tolist() for x in c)
    with pytest.raises(ValueError, match="split"):
        dataset.segment_indices(10, 8, "eval")


# ------------------------------------------------------------------------------------------------- frame folders
SIZES = {"a": (9, 7, 11), "b": (6, 8, 5), "c": (2, 4, 4), "d": (7, 5, 9)}        # folder -> (frames, H, W)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """Tiny PNG frames {:03d}.png (lossless: what comes back must equal what was written), a list file, the arrays."""
    from PIL import Image
    root = tmp_path_factory.mktemp("frames")
    rng = np.random.default_rng(7)
    arrays, lines = {}, []
    for label, (name, (nf, h, w)) in enumerate(SIZES.items()):
        arrays[name] = rng.integers(0, 256, (nf, h, w, 3), dtype=np.uint8)
        os.makedirs(root / name)
        for p in range(1, nf + 1):
            if (name, p) != ("d", 4):                                # d's frame 4 is missing: frame 2 stands in
                Image.fromarray(arrays[name][p - 1], mode="RGB").save(root / name / ("%03d.png" % p))
        lines.append("%s %d %d" % (name, nf, label + 3))
    with open(root / "list.txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return str(root), str(root / "list.txt"), arrays


def _ds(folder, **kw):
    root, lst, _ = folder
    kw.setdefault("image_tmpl", "{:03d}.png")
    return dataset.RubiksDataset(root, lst, **kw)


def test_list_parsing_and_the_three_frames_filter(folder):
    ds = _ds(folder, num_segments=2)
    assert [(r.path, r.num_frames, r.label) for r in ds.video_list] == [("a", 9, 3), ("b", 6, 4), ("d", 7, 6)]
    assert len(_ds(folder, num_segments=2, test_mode=True)) == 4                       # the filter applies outside test mode ...
    assert len(_ds(folder, num_segments=2, test_mode=True, remove_missing=True)) == 3  # ... or when asked for
    assert ds.split == "train" and _ds(folder, random_shift=False).split == "val" and _ds(folder, test_mode=True).split == "test"
    with pytest.raises(NotImplementedError):
        _ds(folder, image_tmpl="{:06d}-{}_{:05d}.jpg")


def test_frames_and_labels_equal_what_was_written(folder):
    arrays = folder[2]
    ds = _ds(folder, num_segments=3, test_mode=True, only_even_indices=False)
    for i, name in enumerate(["a", "b", "c"]):
        frames, label = ds[i]
        idx = dataset.segment_indices(SIZES[name][0], 3, "test")
        assert frames.dtype == torch.uint8 and tuple(frames.shape) == (3,) + SIZES[name][1:] + (3,)
        assert np.array_equal(frames.numpy(), arrays[name][idx - 1]) and label == i + 3
    # a seeded training draw reads the frames segment_indices names under the same seed
    ds = _ds(folder, num_segments=2, generator=torch.Generator().manual_seed(3))
    frames, _ = ds[0]
    idx = dataset.segment_indices(9, 2, "train", generator=torch.Generator().manual_seed(3))
    assert (idx % 2 == 0).all() and np.array_equal(frames.numpy(), arrays["a"][idx - 1])


def test_new_length_two_and_the_last_frame_step(folder):
    arrays = folder[2]
    ds = _ds(folder, num_segments=2, new_length=2, test_mode=True)
    frames, _ = ds[1]                                                # 6 frames: tick 2.5 -> 2, 4 -> frames 2, 3, 4, 5
    assert np.array_equal(frames.numpy(), arrays["b"][[1, 2, 3, 4]])
    record = ds.video_list[1]
    frames, _ = ds.get(record, [6])                                  # p < num_frames fails: the last frame repeats
    assert np.array_equal(frames.numpy(), arrays["b"][[5, 5]])
    whole, label = ds.whole(0)
    assert np.array_equal(whole.numpy(), arrays["a"]) and label == 3 and ds.num_frames_of(0) == 9


def test_missing_frame_falls_back_to_frame_two_with_a_warning(folder):
    arrays = folder[2]
    ds = _ds(folder, num_segments=1, test_mode=True)
    record = ds.video_list[3]
    with pytest.warns(UserWarning, match="error loading image"):
        frames, label = ds.get(record, [3, 4, 5])
    assert np.array_equal(frames.numpy(), arrays["d"][[2, 1, 4]]) and label == 6


def test_transform_gets_the_list_of_pil_images(folder):
    ds = _ds(folder, num_segments=2, test_mode=True, transform=lambda imgs: [(im.mode, im.size) for im in imgs])
    got, label = ds[0]
    assert got == [("RGB", (11, 7))] * 2 and label == 3
    with pytest.raises(ValueError, match="not found"):
        dataset.RubiksDataset(folder[0], folder[1], image_tmpl="x{:03d}.png")[0]


def test_pack_clips_three_sizes_one_odd_offset(folder):
    arrays = folder[2]
    samples = [(torch.from_numpy(arrays[n][:k]), lab) for n, k, lab in (("a", 3, 5), ("b", 2, 0), ("d", 4, 9))]
    arena, clips, labels = dataset.pack_clips(samples)
    assert arena.dtype == torch.uint8 and arena.dim() == 1 and arena.numel() == sum(s.numel() for s, _ in samples)
    assert clips.dtype == torch.int64 and clips.tolist() == [[0, 7, 11, 3], [693, 8, 5, 2], [933, 5, 9, 4]]
    assert clips[1, 0] % 2 == 1 and labels.tolist() == [5, 0, 9]
    for (off, h, w, k), (s, _) in zip(clips.tolist(), samples):
        assert torch.equal(arena[off:off + k * h * w * 3].view(k, h, w, 3), s)
    augment.check_ragged(arena.numel(), clips, torch.zeros(3, 2, dtype=torch.int32),
                         torch.tensor([(0, 0, 4, 4, 4, 4, 0, 0, 0)] * 3, dtype=torch.int32), 4)
    with pytest.raises(ValueError, match="uint8"):
        dataset.pack_clips([(torch.zeros(2, 3, 3, 3), 0)])


def test_two_workers_decode_and_pack(folder):
    arrays = folder[2]
    ds = _ds(folder, num_segments=2, test_mode=True, only_even_indices=False)
    dl = torch.utils.data.DataLoader(ds, batch_size=2, num_workers=2, collate_fn=dataset.pack_clips)
    names = ["a", "b", "c", "d"]
    batches = list(dl)
    assert len(batches) == 2
    for b, (arena, clips, labels) in enumerate(batches):
        assert labels.tolist() == [2 * b + 3, 2 * b + 4]
        for (off, h, w, k), name in zip(clips.tolist(), names[2 * b:]):
            idx = dataset.segment_indices(SIZES[name][0], 2, "test")
            assert (k, h, w) == (2,) + SIZES[name][1:]
            assert np.array_equal(arena[off:off + k * h * w * 3].view(k, h, w, 3).numpy(), arrays[name][idx - 1])


def test_return_dataset_is_the_reference_table(tmp_path):
    os.makedirs(tmp_path / "somethingv2" / "label")
    with open(tmp_path / "somethingv2" / "label" / "category.txt", "w") as fh:
        fh.write("Pushing something\nPulling something\nDropping something\n")
    root = str(tmp_path)
    j = os.path.join
    assert dataset.return_dataset("ucf101", root) == (101, j(root, "ucf101/label/train.txt"), j(root, "ucf101/label/val.txt"),
                                                      j(root, "ucf101/rgb"), "img_{:05d}.jpg")
    assert dataset.return_dataset("hmdb", root) == (51, j(root, "hmdb/label/train.txt"), j(root, "hmdb/label/val.txt"),
                                                    j(root, "hmdb/rgb"), "img_{:05d}.jpg")
    assert dataset.return_dataset("kinetics", root) == (400, j(root, "kinetics/labels/train_videofolder.txt"),
                                                        j(root, "kinetics/labels/val_videofolder.txt"),
                                                        j(root, "kinetics/images"), "img_{:05d}.jpg")
    v2 = (3, j(root, "somethingv2/label/train_videofolder.txt"), j(root, "somethingv2/label/val_videofolder.txt"),
          j(root, "somethingv2/rgb"), "{:06d}.jpg")
    assert dataset.return_dataset("somethingv2", root) == v2 and dataset.return_dataset("something", root) == v2
    with pytest.raises(FileNotFoundError):
        dataset.return_dataset("somethingv1", root)
    with pytest.raises(ValueError, match="Unknown dataset"):
        dataset.return_dataset("imagenet", root)


def test_in_memory_videos_sample_like_the_dataset(folder):
    arrays = folder[2]
    mem = dataset.InMemoryVideos([arrays["a"], arrays["b"]], [1, 2], num_segments=2, test_mode=True, twice_sample=True)
    frames, label = mem[0]
    idx = dataset.segment_indices(9, 2, "test", twice_sample=True)
    assert idx.size == 4 and np.array_equal(frames.numpy(), arrays["a"][idx - 1]) and label == 1
    assert mem.frame_numbers(6) == dataset.segment_indices(6, 2, "test", twice_sample=True).tolist()
    with pytest.raises(ValueError, match="uint8"):
        dataset.InMemoryVideos([torch.zeros(2, 3, 3, 3)], [0])


# ------------------------------------------------------------------------------------------------- argument checks
def _tables():
    clips = torch.tensor([[0, 6, 8, 3], [433, 5, 7, 2]], dtype=torch.int64)              # 432 bytes, one spare, 210 bytes
    frame_idx = torch.tensor([[0, 2], [1, 1], [1, 0], [0, 0]], dtype=torch.int32)
    boxes = torch.tensor([(0, 0, 8, 6, 4, 4, 0, 0, 0), (1, 1, 4, 4, 4, 4, 0, 0, 1), (0, 0, 7, 5, 4, 4, 0, 0, 0),
                          (2, 0, 5, 5, 4, 4, 0, 0, 0)], dtype=torch.int32)
    return 643, clips, frame_idx, boxes


def test_check_ragged_accepts_and_names_what_is_wrong():
    n, clips, frame_idx, boxes = _tables()
    assert augment.check_ragged(n, clips, frame_idx, boxes, 4, views=2) == (2, 2)

    def bad(match, n=n, clips=clips, frame_idx=frame_idx, boxes=boxes, views=2, exc=ValueError):
        with pytest.raises(exc, match=match):
            augment.check_ragged(n, clips, frame_idx, boxes, 4, views=views)

    bad("outside the arena", n=642)
    edit = clips.clone(); edit[0, 0] = -1
    bad("outside the arena", clips=edit)
    edit = clips.clone(); edit[1, 3] = 3
    bad("outside the arena", clips=edit)
    edit = clips.clone(); edit[1, 3] = 0
    bad("0 frames", clips=edit)
    edit = clips.clone(); edit[0, 2] = 16385
    bad("outside \\[1, 16384\\]", clips=edit)
    edit = frame_idx.clone(); edit[3, 1] = 2
    bad("clip 1: frame index", frame_idx=edit)
    edit = frame_idx.clone(); edit[0, 0] = -1
    bad("clip 0: frame index", frame_idx=edit)
    bad("clip 1: box 1 .*crop outside the frame", boxes=boxes[[0, 1, 2, 0]])     # valid for clip 0's 6x8, not for 5x7
    bad("int64 \\[B, 4\\]", clips=clips.int())
    bad("frame_idx must be int32", frame_idx=frame_idx.long())
    bad("frame_idx must be int32 \\[B \\* views, T\\] = \\[2, T\\]", views=1)
    bad("boxes must be int32 \\[B \\* views, 9\\]", boxes=boxes[:3])
    bad("views", views=0)


def test_ragged_entry_checks_its_arguments_before_it_needs_a_device():
    n, clips, frame_idx, boxes = _tables()
    arena = torch.zeros(n, dtype=torch.uint8)
    with pytest.raises(ValueError, match="dtype"):
        augment.ragged_u8_to_clips(arena, clips, frame_idx, boxes, 4, views=2, dtype=torch.float16)
    with pytest.raises(ValueError, match="arena must be a uint8"):
        augment.ragged_u8_to_clips(arena.float(), clips, frame_idx, boxes, 4, views=2)
    with pytest.raises(ValueError, match="outside the arena"):
        augment.ragged_u8_to_clips(arena[:-1], clips, frame_idx, boxes, 4, views=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # valid tables, but the arena is not on a GPU
        augment.ragged_u8_to_clips(arena, clips, frame_idx, boxes, 4, views=2)


def test_per_clip_boxes_calls_the_builder_with_each_clips_size():
    sizes = [(240, 320), (240, 427), (256, 340)]
    got = augment.per_clip_boxes(sizes, lambda hw: augment.full_res_boxes(1, hw, 224, flip=False))
    assert got.dtype == torch.int32 and tuple(got.shape) == (9, 9)
    for i, hw in enumerate(sizes):
        assert torch.equal(got[3 * i:3 * i + 3], augment.full_res_boxes(1, hw, 224, flip=False))
        augment.check_boxes(got[3 * i:3 * i + 3], hw, 224)
    assert tuple(augment.per_clip_boxes([], lambda hw: None).shape) == (0, 9)
    with pytest.raises(ValueError, match="int32 \\[views, 9\\]"):
        augment.per_clip_boxes(sizes, lambda hw: torch.zeros(1, 9))
    with pytest.raises(ValueError, match="views for clip 1"):
        augment.per_clip_boxes(sizes, lambda hw: augment.full_res_boxes(1, hw, 224, flip=hw[1] == 427))


def test_abi_argument_validation_without_a_device():
    import ctypes
    from rubiksnet_amd import _native
    L = _native.lib()
    one = ctypes.c_void_p(16)
    for sfx in ("f32", "bf16"):
        fn = getattr(L, "rk_clip_resample_ragged_u8_" + sfx)
        assert fn(None, 64, one, one, one, one, one, one, 1, 1, 1, 8, 8, None) == -1
        assert fn(one, 64, one, None, one, one, one, one, 1, 1, 1, 8, 8, None) == -1
        assert fn(one, 0, one, one, one, one, one, one, 1, 1, 1, 8, 8, None) == -2
        assert fn(one, 64, one, one, one, one, one, one, 1, 0, 1, 8, 8, None) == -2
        assert fn(one, 64, one, one, one, one, one, one, 40000, 2, 1, 8, 8, None) == -2
