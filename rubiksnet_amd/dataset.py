"""Real video datasets: the reference's `rubiksnet.dataset` (dataset/core.py, dataset/config.py) and two feeders.

The reference decodes the sampled frames of a video with PIL in a DataLoader worker and augments them there.  Here a
worker only decodes: `RubiksDataset` with `transform=None` returns the chosen frames as uint8 [K, H, W, 3], `pack_clips`
lays the videos of a batch -- of whatever sizes -- back to back into one byte arena with a record per video, and the
device does the rest in one launch (augment.ragged_u8_to_clips, rk_clip_resample_ragged_u8_*).

  segment_indices   the frame sampling of core.py:89-265, every branch, as one function of (num_frames, split, flags)
  RubiksDataset     list file + frame folders (core.py:11-87, :267-325); VideoRecord
  InMemoryVideos    the same sampling over decoded videos held in memory
  return_dataset    the five values of dataset/config.py, as a table
  pack_clips        the collate function: arena [bytes], clips int64 [B, 4], labels
  FrameLoader       DataLoader workers -> pinned staging arena -> side-stream copy + ragged launch
                    (decode="device": the workers ship the JPEG files' bytes, jpeg.pack_jpeg_clips packs them and
                    rk_jpeg_decode_u8 decodes them on the side stream in front of the ragged launch; entropy="rows":
                    by MCU row, through the chunked index build and rk_jpeg_decode_indexed_u8)
  DeviceFrameCache  a small set decoded once and resident in HBM; only the three small tables travel per batch

The random draws come from a `torch.Generator` (or torch's global generator, which a DataLoader seeds per worker): the
set of choices is the reference's, the stream is not numpy's.
"""
import collections
import os
import warnings

import numpy as np
import torch
import torch.utils.data as data

from . import augment, jpeg
from .input_pipeline import IMAGENET_MEAN, IMAGENET_STD, _mean_std_on, _near_gpu

__all__ = ["segment_indices", "VideoRecord", "RubiksDataset", "InMemoryVideos", "return_dataset", "pack_clips",
           "FrameLoader", "DeviceFrameCache", "SPLITS"]

SPLITS = ("train", "val", "test")


# ------------------------------------------------------------------------------------------------- sampling
def _draw(bound, size, generator=None):
    """The one source of randomness of segment_indices: `size` integers (one when size is None) uniform in [0, bound),
    as numpy.random.randint(bound, size=size).  A test replaces this to inject the reference's draws."""
    if bound <= 0:
        raise ValueError("nothing to draw from: bound %d" % bound)
    return torch.randint(int(bound), (1 if size is None else int(size),), generator=generator).numpy()


def _start(sample_pos, generator):
    # core.py:99-101: np.random.randint(0, sample_pos - 1) -- the upper bound is sample_pos - 1, exclusive
    return 0 if sample_pos == 1 else int(_draw(sample_pos - 1, None, generator)[0])


def _ticks(span, num_segments, new_length):
    tick = (span - new_length + 1) / float(num_segments)
    return [int(tick / 2.0 + tick * x) for x in range(num_segments)], tick


def segment_indices(num_frames, num_segments, split, *, new_length=1, dense_sample=False, all_sample=False,
                    twice_sample=False, only_even_indices=True, generator=None):
    """The 1-based frame numbers RubiksDataset reads for a video of `num_frames` frames, int64 (always: the reference
    returns floats where a short video falls back to the constant index).  split "train" is _sample_indices (core.py:89-164),
    "val" _get_val_indices (:166-220), "test" _get_test_indices (:222-265), quirks included: "test" looks at
    only_even_indices under dense sampling only; "val" with dense_sample or all_sample still draws a random start; that
    draw's upper bound is sample_pos - 1; twice_sample matters to "test" alone (2 * num_segments numbers: the half-tick clip,
    then the tick clip)."""
    if split not in SPLITS:
        raise ValueError("split must be one of %r, got %r" % (SPLITS, split))
    n, S, L = int(num_frames), int(num_segments), int(new_length)
    half = n // 2
    seg = range(S)
    if dense_sample:                                            # i3d dense sample: the same three ways in every split
        span, window, mul = (half, 32, 2) if only_even_indices else (n, 64, 1)
        sample_pos = max(1, 1 + span - window)
        t_stride = window // S
        if split == "test":
            starts = np.linspace(0, sample_pos - 1, num=10, dtype=int).tolist()
        else:
            starts = [_start(sample_pos, generator)]
        offsets = [(idx * t_stride + s) % span for s in starts for idx in seg]
        return (np.asarray(offsets, dtype=np.int64) + 1) * mul
    if split == "test":
        if twice_sample:
            first, tick = _ticks(n, S, L)
            return np.asarray(first + [int(tick * x) for x in seg], dtype=np.int64) + 1
        if all_sample:
            return np.arange(n, dtype=np.int64) + 1
        return np.asarray(_ticks(n, S, L)[0], dtype=np.int64) + 1
    if all_sample:
        s = _start(max(1, 1 + n - S), generator)
        return np.asarray([(idx + s) % n for idx in seg], dtype=np.int64) + 1
    span, mul = (half, 2) if only_even_indices else (n, 1)
    if split == "train":
        average_duration = (span - L + 1) // S
        if average_duration > 0:
            offsets = np.arange(S, dtype=np.int64) * average_duration + np.asarray(_draw(average_duration, S, generator))
        elif span > S:
            offsets = np.sort(np.asarray(_draw(span - L + 1, S, generator)))
        else:
            offsets = np.zeros(S)
    elif span > S + L - 1:
        offsets = _ticks(span, S, L)[0]
    else:
        offsets = np.zeros(S)
    return (np.asarray(offsets).astype(np.int64) + 1) * mul


def _frame_numbers(indices, num_frames, new_length):
    """core.py:310-319: new_length consecutive frames from every index, the number advancing only while p < num_frames."""
    out = []
    for seg_ind in indices:
        p = int(seg_ind)
        for _ in range(new_length):
            out.append(p)
            if p < num_frames:
                p += 1
    return out


class _Sampled(data.Dataset):
    """What RubiksDataset and InMemoryVideos share: the sampling flags and the split they select."""

    def _init_sampling(self, num_segments, new_length, random_shift, test_mode, dense_sample, all_sample, twice_sample,
                       only_even_indices, generator):
        self.num_segments, self.new_length = int(num_segments), int(new_length)
        self.random_shift, self.test_mode = random_shift, test_mode
        self.dense_sample, self.all_sample, self.twice_sample = dense_sample, all_sample, twice_sample
        self.only_even_indices, self.generator = only_even_indices, generator

    @property
    def split(self):
        return "test" if self.test_mode else ("train" if self.random_shift else "val")

    def sample(self, num_frames, generator=None):
        return segment_indices(num_frames, self.num_segments, self.split, new_length=self.new_length,
                               dense_sample=self.dense_sample, all_sample=self.all_sample, twice_sample=self.twice_sample,
                               only_even_indices=self.only_even_indices, generator=generator or self.generator)

    def frame_numbers(self, num_frames, generator=None):
        """The 1-based frames one sample of a video of num_frames frames reads, new_length included."""
        return _frame_numbers(self.sample(num_frames, generator), num_frames, self.new_length)


# ------------------------------------------------------------------------------------------------- frame folders
class VideoRecord(object):
    """One line of a list file: `<folder> <num_frames> <label>` (core.py:328-342)."""

    def __init__(self, row):
        self._data = row

    @property
    def path(self):
        return self._data[0]

    @property
    def num_frames(self):
        return int(self._data[1])

    @property
    def label(self):
        return int(self._data[2])


class RubiksDataset(_Sampled):
    """The reference's RubiksDataset (core.py:11-87, :267-325) with its constructor arguments.  With a `transform` a
    sample is `(transform(list of PIL images), label)` as there; with `transform=None` it is `(uint8 [K, H, W, 3], label)`,
    the decoded frames for the device path.  `generator`: a torch.Generator for the draws; None uses torch's global
    generator, which a DataLoader seeds differently in every worker.  decode="device" (with transform=None): a sample is
    `(list of frames, label)`, a frame being the bytes of its file, undecoded, for jpeg.pack_jpeg_clips and the device
    decoder -- or uint8 [H, W, 3] decoded here as ever where jpeg.parse_jpeg refuses the file."""

    def __init__(self, root_path, list_file, num_segments=3, new_length=1, image_tmpl="img_{:05d}.jpg", transform=None,
                 random_shift=True, test_mode=False, remove_missing=False, dense_sample=False, all_sample=False,
                 twice_sample=False, only_even_indices=True, logger=None, generator=None, decode="host"):
        if decode not in ("host", "device"):
            raise ValueError("decode must be 'host' or 'device', got %r" % (decode,))
        if decode == "device" and transform is not None:
            raise ValueError("decode='device' hands out undecoded files: it goes with transform=None")
        self.decode = decode
        if image_tmpl == "{:06d}-{}_{:05d}.jpg":
            raise NotImplementedError("the %r naming (halved frame counts, core.py:84-86) is not supported" % image_tmpl)
        self.verbose = logger is not None
        self.root_path, self.list_file, self.image_tmpl = root_path, list_file, image_tmpl
        self.transform, self.remove_missing = transform, remove_missing
        self._init_sampling(num_segments, new_length, random_shift, test_mode, dense_sample, all_sample, twice_sample,
                            only_even_indices, generator)
        self._parse_list()

    def _parse_list(self):
        with open(self.list_file) as fh:
            tmp = [x.strip().split(" ") for x in fh]
        if not self.test_mode or self.remove_missing:                  # core.py:79-81: videos under 3 frames go
            tmp = [item for item in tmp if int(item[1]) >= 3]
        self.video_list = [VideoRecord(item) for item in tmp]
        if self.verbose:
            print("video number:%d" % len(self.video_list))

    def _path(self, directory, idx):
        return os.path.join(self.root_path, directory, self.image_tmpl.format(idx))

    def _load_image(self, directory, idx):
        from PIL import Image
        try:
            with Image.open(self._path(directory, idx)) as im:
                return [im.convert("RGB")]
        except Exception:
            warnings.warn("error loading image: %s (frame 2 stands in)" % self._path(directory, idx))
            with Image.open(self._path(directory, 2)) as im:
                return [im.convert("RGB")]

    def _load_bytes(self, directory, idx):
        """A frame for the device decoder: the file's bytes; decoded here (uint8 [H, W, 3]) where the file is missing,
        unreadable or outside what the device decodes -- by _load_image, with its stand-in rule."""
        try:
            with open(self._path(directory, idx), "rb") as fh:
                raw = fh.read()
            if jpeg.parse_jpeg(raw) is not None:
                return raw
        except OSError:
            pass
        return np.asarray(self._load_image(directory, idx)[0], dtype=np.uint8)

    def __getitem__(self, index):
        record = self.video_list[index]
        first = self._path(record.path, 2 if self.only_even_indices else 1)
        if not os.path.exists(first):
            raise ValueError("not found: %s" % first)
        return self.get(record, self.sample(record.num_frames))

    def get(self, record, indices):
        if self.decode == "device":
            numbers = _frame_numbers(indices, record.num_frames, self.new_length)
            return [self._load_bytes(record.path, p) for p in numbers], record.label
        images = []
        for p in _frame_numbers(indices, record.num_frames, self.new_length):
            images.extend(self._load_image(record.path, p))
        if self.transform is not None:
            return self.transform(images), record.label
        return torch.from_numpy(np.stack([np.asarray(im, dtype=np.uint8) for im in images])), record.label

    def __len__(self):
        return len(self.video_list)

    # what DeviceFrameCache asks of a source
    def num_frames_of(self, index):
        return self.video_list[index].num_frames

    def whole(self, index):
        """Every frame of a video, 1 .. num_frames, uint8 [F, H, W, 3], and its label."""
        record = self.video_list[index]
        images = [self._load_image(record.path, p)[0] for p in range(1, record.num_frames + 1)]
        return torch.from_numpy(np.stack([np.asarray(im, dtype=np.uint8) for im in images])), record.label

    def whole_bytes(self, index):
        """whole() for the device decoder: every frame of a video as _load_bytes gives it (the file's bytes, or uint8
        [H, W, 3] where the host had to decode it, with the same stand-in rule), and its label."""
        record = self.video_list[index]
        return [self._load_bytes(record.path, p) for p in range(1, record.num_frames + 1)], record.label


class InMemoryVideos(_Sampled):
    """RubiksDataset's sampling over videos that are already decoded: `videos` a list of uint8 [F, H, W, 3] tensors (of
    any sizes), frame number p of the reference being videos[i][p - 1]."""

    def __init__(self, videos, labels, num_segments=3, new_length=1, random_shift=True, test_mode=False, dense_sample=False,
                 all_sample=False, twice_sample=False, only_even_indices=True, generator=None):
        self.videos = [torch.as_tensor(v) for v in videos]
        self.labels = [int(l) for l in labels]
        if len(self.videos) != len(self.labels):
            raise ValueError("%d videos and %d labels" % (len(self.videos), len(self.labels)))
        for v in self.videos:
            if v.dtype != torch.uint8 or v.dim() != 4 or v.shape[-1] != 3 or v.shape[0] < 1:
                raise ValueError("a video must be uint8 [F, H, W, 3], got %s %s" % (v.dtype, tuple(v.shape)))
        self._init_sampling(num_segments, new_length, random_shift, test_mode, dense_sample, all_sample, twice_sample,
                            only_even_indices, generator)

    def __getitem__(self, index):
        v = self.videos[index]
        p = torch.tensor(self.frame_numbers(v.shape[0])).clamp_(1, v.shape[0]) - 1
        return v[p], self.labels[index]

    def __len__(self):
        return len(self.videos)

    def num_frames_of(self, index):
        return self.videos[index].shape[0]

    def whole(self, index):
        return self.videos[index], self.labels[index]


# ------------------------------------------------------------------------------------------------- dataset/config.py
# name -> (classes: a count or a category file, train list, val list, frame root, frame name template)
_DATASETS = {
    "ucf101": (101, "ucf101/label/train.txt", "ucf101/label/val.txt", "ucf101/rgb", "img_{:05d}.jpg"),
    "hmdb": (51, "hmdb/label/train.txt", "hmdb/label/val.txt", "hmdb/rgb", "img_{:05d}.jpg"),
    "somethingv1": ("somethingv1/label/category.txt", "somethingv1/label/train_videofolder.txt",
                    "somethingv1/label/val_videofolder.txt", "somethingv1/rgb", "{:05d}.jpg"),
    "somethingv2": ("somethingv2/label/category.txt", "somethingv2/label/train_videofolder.txt",
                    "somethingv2/label/val_videofolder.txt", "somethingv2/rgb", "{:06d}.jpg"),
    "kinetics": (400, "kinetics/labels/train_videofolder.txt", "kinetics/labels/val_videofolder.txt", "kinetics/images",
                 "img_{:05d}.jpg"),
}
_DATASETS["something"] = _DATASETS["somethingv2"]


def return_dataset(dataset, root_path):
    """(n_class, train list, val list, frame root, frame name template) as the reference's dataset/config.py returns
    them; a dataset with a category file has as many classes as the file has lines."""
    if dataset not in _DATASETS:
        raise ValueError("Unknown dataset " + dataset)
    classes, train, val, root, prefix = _DATASETS[dataset]
    if isinstance(classes, str):
        with open(os.path.join(root_path, classes)) as fh:
            classes = len(fh.readlines())
    return classes, os.path.join(root_path, train), os.path.join(root_path, val), os.path.join(root_path, root), prefix


# ------------------------------------------------------------------------------------------------- collate
def pack_clips(samples):
    """The collate function of the device path.  samples: [(uint8 [K, H, W, 3], label)], sizes and K differing freely.
    Returns (arena uint8 [bytes], clips int64 [B, 4], labels int64 [B]): the videos back to back, no padding, a record
    (byte offset of the first frame, Hs, Ws, F) each; frames contiguous, rows Ws * 3 bytes apart."""
    rows, off = [], 0
    for frames, _ in samples:
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError("a sample must be uint8 [K, H, W, 3], got %s %s" % (frames.dtype, tuple(frames.shape)))
        rows.append((off, frames.shape[1], frames.shape[2], frames.shape[0]))
        off += frames.numel()
    arena = torch.empty(off, dtype=torch.uint8)
    for (o, h, w, k), (frames, _) in zip(rows, samples):
        arena[o:o + k * h * w * 3].view(k, h, w, 3).copy_(frames)
    return (arena, torch.tensor(rows, dtype=torch.int64).reshape(-1, 4),
            torch.tensor([int(label) for _, label in samples], dtype=torch.int64))


# ------------------------------------------------------------------------------------------------- feeders
def _default_box_fn(split, size, flip_p):
    """Training: one multiscale crop + flip per clip (GroupMultiScaleCrop + GroupRandomHorizontalFlip).  Evaluation: the
    centre crop of the frame scaled to size * 256 // 224 on its short edge (scripts/test_models.py, one crop)."""
    if split == "train":
        return lambda hw, gen: augment.multiscale_crop_boxes(1, hw, size, flip_p=flip_p, generator=gen)
    return lambda hw, gen: augment.center_crop_boxes(1, hw, size[0] * 256 // 224, size)


def _temporal_index(K, temporal_clips, crops):
    """frame_idx rows of one video whose sample holds K frames = temporal_clips clips of T: crop-major, temporal clip
    minor, the reference's order (its view(-1, T, 3, H, W) of crops x 2T frames, scripts/test_models.py:159-162)."""
    if K % temporal_clips:
        raise ValueError("%d frames do not split into %d temporal clips" % (K, temporal_clips))
    T = K // temporal_clips
    one = torch.arange(K, dtype=torch.int32).view(temporal_clips, T)
    return one.repeat(crops, 1)


class _Feeder:
    """What the two feeders share: the split, the box function and how boxes and frame indices are laid out."""

    def _init_feeder(self, source, batch, split, device, dtype, size, views, box_fn, temporal_clips, seed, flip_p):
        if split not in SPLITS:
            raise ValueError("split must be one of %r, got %r" % (SPLITS, split))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("%s feeds a GPU (no CPU path)" % type(self).__name__)
        self.batch, self.split, self.dtype, self.size = int(batch), split, dtype, augment._hw(size)
        self.crops = int(views)
        if temporal_clips is None:
            temporal_clips = 2 if (split == "test" and getattr(source, "twice_sample", False)
                                   and not getattr(source, "dense_sample", False)) else 1
        self.temporal_clips = int(temporal_clips)
        self.views = self.crops * self.temporal_clips
        self._box_fn = box_fn or _default_box_fn(split, self.size, flip_p)
        self._gen = torch.Generator().manual_seed(seed)
        self.tables = None          # host tables of the batch handed out last: clips, frame_idx, boxes (+ arena / videos)

    def _boxes(self, sizes):
        """[len(sizes) * views, 9]: every crop's box repeated for its temporal clips."""
        boxes = augment.per_clip_boxes(sizes, lambda hw: self._box_fn(hw, self._gen))
        if boxes.shape[0] != len(sizes) * self.crops:
            raise ValueError("box_fn returned %d boxes per clip, views=%d" % (boxes.shape[0] // max(len(sizes), 1), self.crops))
        return boxes.repeat_interleave(self.temporal_clips, dim=0)


class FrameLoader(_Feeder):
    """One epoch per iteration of (clips [B * views, T, 3, size, size] normalised, labels [B]) on `device` from a dataset
    of (uint8 [K, H, W, 3], label) samples -- RubiksDataset(transform=None), InMemoryVideos.

    A torch DataLoader's workers decode and pack (pack_clips) and never touch the GPU.  The parent copies a batch's arena
    into a pinned staging arena (one per slot, grown on demand), draws the boxes for the sizes the batch turned out to
    have, and queues copy + rk_clip_resample_ragged_u8_* on a side stream under SyntheticFrameLoader's event protocol:
    `ready` / `consumed` per slot, the caller's stream waits on the device, a slot's pinned memory is rewritten only after
    the copy that last read it has completed.  A batch stays valid until the next one is asked for.

    `views` spatial crops per video come from `box_fn((H, W), generator)` -> int32 [views, 9]; default: a multiscale crop
    + flip for split "train", the centre crop otherwise.  With a twice_sample test dataset the 2T decoded frames become
    two temporal clips through frame_idx; rows are crop-major, temporal clip minor, so
    `clips.view(B, -1, size, size)` is what evaluation.fold_views(..., views=loader.views) takes.

    decode="device" (with a RubiksDataset(..., decode="device")): the workers read the files and pack their bytes
    (jpeg.pack_jpeg_clips); the compressed arena and its tables travel through the same pinned slot, rk_jpeg_decode_u8
    decodes them into a per-slot RGB arena on the side stream, and the unchanged ragged launch follows on that arena.
    Boxes are drawn from the sizes in the headers, so nothing waits for the device; the clips are bit-identical to the
    host path's.  `fallback_frames` counts the frames that travelled decoded (files the device does not decode);
    `decode_errors()` reads, on request, how many frames the device refused (they come out as zero frames).
    entropy="rows" (with decode="device") decodes by MCU row instead of one Huffman chain per frame: the index tables of a
    batch's own records (jpeg.row_tables, made in the parent from the headers' sizes) travel with the blob,
    rk_jpeg_build_index_chunked finds the rows' entries on the side stream and rk_jpeg_decode_indexed_u8 decodes by them,
    in front of the same ragged launch; the clips are the same bits.  `chain_frames()` reads, on request, how many frames
    the chunked build left to the sequential walk."""

    def __init__(self, dataset, batch, split, device="cuda:0", dtype=torch.float32, size=224, views=1, box_fn=None,
                 num_workers=0, depth=2, seed=0, temporal_clips=None, shuffle=None, drop_last=False, flip_p=0.5,
                 decode="host", entropy="chain", chunk_bytes=256, max_rounds=32):
        if decode not in ("host", "device"):
            raise ValueError("decode must be 'host' or 'device', got %r" % (decode,))
        if entropy not in ("chain", "rows"):
            raise ValueError("entropy must be 'chain' or 'rows', got %r" % (entropy,))
        if entropy == "rows" and decode != "device":
            raise ValueError("entropy='rows' is a way to decode on the device: it goes with decode='device', not %r" % (decode,))
        if entropy == "rows":
            jpeg._check_chunking(chunk_bytes, max_rounds)
        if getattr(dataset, "decode", "host") != decode:
            raise ValueError("the dataset hands out %s-decoded samples, the loader was asked for decode=%r"
                             % (getattr(dataset, "decode", "host"), decode))
        self._init_feeder(dataset, batch, split, device, dtype, size, views, box_fn, temporal_clips, seed, flip_p)
        self.depth = int(depth)
        self.decode, self.fallback_frames = decode, 0
        self.entropy, self.chunk_bytes, self.max_rounds = entropy, int(chunk_bytes), int(max_rounds)
        shuffle = (split == "train") if shuffle is None else shuffle
        self._dl = data.DataLoader(dataset, batch_size=self.batch, shuffle=shuffle, num_workers=num_workers,
                                   collate_fn=pack_clips if decode == "host" else jpeg.pack_jpeg_clips, drop_last=drop_last,
                                   generator=torch.Generator().manual_seed(seed + 1), persistent_workers=num_workers > 0)
        self._stream = torch.cuda.Stream(self.device)
        self._pinned = [None] * self.depth                 # staging arenas, host
        self._arena = [None] * self.depth                  # staging arenas, device
        self._tab = [None] * self.depth                    # (pinned, device) tables, sized by the first batch's T
        self._out = [None] * self.depth
        self._ready = [torch.cuda.Event() for _ in range(self.depth)]
        self._consumed = [torch.cuda.Event() for _ in range(self.depth)]
        self._copied = [None] * self.depth
        self._host = [None] * self.depth
        if decode == "device":
            self._rgb = [None] * self.depth                # decoded frames, device
            self._ws = [None] * self.depth                 # the decoder's workspace, device
            self._status = [None] * self.depth             # its per-frame codes, device
            self._rows = [None] * self.depth               # entropy="rows": entries, build workspace, build codes, route
            with torch.cuda.stream(self._stream):
                self._errors = torch.zeros((), dtype=torch.int64, device=self.device)
                self._chain = torch.zeros((), dtype=torch.int64, device=self.device)
        _mean_std_on(self.device, IMAGENET_MEAN, IMAGENET_STD)      # the one blocking upload happens here, not per batch
        for ev in self._consumed:
            ev.record(torch.cuda.current_stream(self.device))

    def __len__(self):
        return len(self._dl)

    def _tables_for(self, slot, n, T):
        V = self.views
        tab = self._tab[slot]
        if tab is None or tab[0]["frame_idx"].shape[1] != T:
            with _near_gpu(self.device):
                host = {"clips": torch.zeros(self.batch, 4, dtype=torch.int64).pin_memory(),
                        "frame_idx": torch.zeros(self.batch * V, T, dtype=torch.int32).pin_memory(),
                        "boxes": torch.zeros(self.batch * V, 9, dtype=torch.int32).pin_memory(),
                        "labels": torch.zeros(self.batch, dtype=torch.int64).pin_memory()}
            with torch.cuda.stream(self._stream):
                dev = {k: torch.empty_like(v, device=self.device) for k, v in host.items()}
                self._out[slot] = torch.empty(self.batch * V, T, 3, *self.size, dtype=self.dtype, device=self.device)
            tab = self._tab[slot] = (host, dev)
        return tab

    def decode_errors(self):
        """Frames the device decoder refused so far (each came out as a zero frame).  Waits for the side stream: ask
        once, at the end of an epoch."""
        if self.decode != "device":
            return 0
        self._stream.synchronize()
        return int(self._errors.item())

    def chain_frames(self):
        """entropy="rows": frames the chunked index build left to the sequential walk so far (restart intervals, no fixed
        point within max_rounds, refused streams).  Waits for the side stream: ask once, at the end of an epoch."""
        if self.decode != "device" or self.entropy != "rows":
            return 0
        self._stream.synchronize()
        return int(self._chain.item())

    @staticmethod
    def _grown(t, need, make):
        """t if it holds `need` elements, else a new tensor with headroom (batches of a ragged set differ in size)."""
        return t if t is not None and t.numel() >= need else make(need + need // 4)

    def _launch_jpeg(self, slot, packed):
        """_launch for a jpeg.PackedJpeg: the blob and the host-decoded frames are staged, the decode launch fills the
        slot's RGB arena, the host-decoded frames are copied into their places, the ragged launch follows."""
        clips, labels, rgb_bytes = packed.clips, packed.labels, int(packed.rgb_bytes)
        n, V = clips.shape[0], self.views
        sizes = [(int(h), int(w)) for h, w in clips[:, 1:3].tolist()]
        frame_idx = torch.cat([_temporal_index(int(k), self.temporal_clips, self.crops) for k in clips[:, 3].tolist()])
        boxes = self._boxes(sizes)
        B, T = augment.check_ragged(rgb_bytes, clips, frame_idx, boxes, self.size, V)
        blob_bytes = nbytes = packed.blob.numel()
        spots = []                                          # (offset in the staging arena, offset in the RGB arena, bytes)
        for off, frame in packed.fallback:
            nbytes = (nbytes + 15) & ~15
            spots.append((nbytes, int(off), frame.numel()))
            nbytes += frame.numel()
        nj = int(packed.layout[0])
        rows = None
        if nj and self.entropy == "rows":                   # the batch's index tables travel behind the host-decoded frames
            rows = jpeg.row_tables(jpeg.records(packed.blob, packed.layout), self.chunk_bytes)
            rows_at = nbytes = (nbytes + 15) & ~15
            nbytes += rows.tables.numel()
        if self._copied[slot] is not None:
            self._copied[slot].synchronize()                # as in _launch: the copies that last read this slot are done
        if self._pinned[slot] is None or self._pinned[slot].numel() < nbytes:
            cap = nbytes + nbytes // 4
            with _near_gpu(self.device):
                self._pinned[slot] = torch.empty(cap, dtype=torch.uint8).pin_memory()
            with torch.cuda.stream(self._stream):
                self._arena[slot] = torch.empty(cap, dtype=torch.uint8, device=self.device)
        with torch.cuda.stream(self._stream):
            self._rgb[slot] = self._grown(self._rgb[slot], rgb_bytes,
                                          lambda m: torch.empty(m, dtype=torch.uint8, device=self.device))
            self._ws[slot] = self._grown(self._ws[slot], int(packed.workspace_bytes) if rows is None else rows.decode_bytes,
                                         lambda m: torch.empty(m, dtype=torch.uint8, device=self.device))
            if rows is not None:
                old = self._rows[slot] or (None, None, None, None)
                self._rows[slot] = (
                    self._grown(old[0], max(rows.n_entries, 1) * 2, lambda m: torch.empty(m, dtype=torch.int64, device=self.device)),
                    self._grown(old[1], rows.build_bytes, lambda m: torch.empty(m, dtype=torch.uint8, device=self.device)),
                    self._grown(old[2], nj + 1, lambda m: torch.zeros(m, dtype=torch.int32, device=self.device)),
                    self._grown(old[3], nj, lambda m: torch.zeros(m, dtype=torch.int32, device=self.device)))
            self._status[slot] = self._grown(self._status[slot], nj + 1,
                                             lambda m: torch.zeros(m, dtype=torch.int32, device=self.device))
        host, dev = self._tables_for(slot, n, T)
        self._pinned[slot][:blob_bytes].copy_(packed.blob)
        for (at, _, m), (_, frame) in zip(spots, packed.fallback):
            self._pinned[slot][at:at + m].copy_(frame.reshape(-1))
        if rows is not None:
            self._pinned[slot][rows_at:nbytes].copy_(rows.tables)
        for name, t in (("clips", clips), ("frame_idx", frame_idx), ("boxes", boxes), ("labels", labels)):
            host[name][:t.shape[0]].copy_(t)
        self._host[slot] = {"packed": packed, "clips": clips, "frame_idx": frame_idx, "boxes": boxes, "labels": labels}
        self.fallback_frames += len(packed.fallback)
        with torch.cuda.stream(self._stream):
            self._stream.wait_event(self._consumed[slot])
            self._arena[slot][:nbytes].copy_(self._pinned[slot][:nbytes], non_blocking=True)
            for name in host:
                dev[name].copy_(host[name], non_blocking=True)
            if self._copied[slot] is None:
                self._copied[slot] = torch.cuda.Event()
            self._copied[slot].record(self._stream)
            rgb = self._rgb[slot][:rgb_bytes]
            if nj:
                (frames, htabs, qtabs, streams), (_, nh, nq) = jpeg.sections(self._arena[slot], packed.layout)
                status = self._status[slot][:nj + 1]
                if rows is None:
                    jpeg.launch_decode(streams, frames, qtabs, htabs, nj, rgb, self._ws[slot], status, nq, nh)
                else:
                    entries, build_ws, build_status, route = self._rows[slot]
                    jpeg.launch_decode_rows(streams, frames, qtabs, htabs, nq, nh, rows, self._arena[slot][rows_at:nbytes],
                                            entries.view(torch.uint8), build_ws, build_status, route, rgb, self._ws[slot], status,
                                            self.chunk_bytes, self.max_rounds)
                    self._chain += (route[:nj] == 0).sum()
                self._errors += status[nj]
            for at, off, m in spots:
                rgb[off:off + m].copy_(self._arena[slot][at:at + m])
            augment.ragged_u8_to_clips(rgb, dev["clips"][:n], dev["frame_idx"][:n * V], dev["boxes"][:n * V], self.size,
                                       views=V, dtype=self.dtype, out=self._out[slot][:n * V])
            self._ready[slot].record(self._stream)
        return n

    def _launch(self, slot, packed):
        """Stage one packed batch into `slot` and queue its copies and the kernel on the side stream."""
        if self.decode == "device":
            return self._launch_jpeg(slot, packed)
        arena, clips, labels = packed
        n, nbytes, V = clips.shape[0], arena.numel(), self.views
        sizes = [(int(h), int(w)) for h, w in clips[:, 1:3].tolist()]
        frame_idx = torch.cat([_temporal_index(int(k), self.temporal_clips, self.crops) for k in clips[:, 3].tolist()])
        boxes = self._boxes(sizes)
        B, T = augment.check_ragged(nbytes, clips, frame_idx, boxes, self.size, V)
        if self._copied[slot] is not None:
            self._copied[slot].synchronize()                # the copies queued `depth` batches ago: long done in steady state
        if self._pinned[slot] is None or self._pinned[slot].numel() < nbytes:
            cap = nbytes + nbytes // 4                      # grow with headroom: batches of a ragged set differ in size
            with _near_gpu(self.device):
                self._pinned[slot] = torch.empty(cap, dtype=torch.uint8).pin_memory()
            with torch.cuda.stream(self._stream):
                self._arena[slot] = torch.empty(cap, dtype=torch.uint8, device=self.device)
        host, dev = self._tables_for(slot, n, T)
        self._pinned[slot][:nbytes].copy_(arena)
        for name, t in (("clips", clips), ("frame_idx", frame_idx), ("boxes", boxes), ("labels", labels)):
            host[name][:t.shape[0]].copy_(t)
        self._host[slot] = {"arena": arena, "clips": clips, "frame_idx": frame_idx, "boxes": boxes, "labels": labels}
        with torch.cuda.stream(self._stream):
            self._stream.wait_event(self._consumed[slot])
            self._arena[slot][:nbytes].copy_(self._pinned[slot][:nbytes], non_blocking=True)
            for name in host:
                dev[name].copy_(host[name], non_blocking=True)
            if self._copied[slot] is None:
                self._copied[slot] = torch.cuda.Event()
            self._copied[slot].record(self._stream)
            augment.ragged_u8_to_clips(self._arena[slot][:nbytes], dev["clips"][:n], dev["frame_idx"][:n * V],
                                       dev["boxes"][:n * V], self.size, views=V, dtype=self.dtype,
                                       out=self._out[slot][:n * V])
            self._ready[slot].record(self._stream)
        return n

    def __iter__(self):
        queue = collections.deque()

        def hand_out():
            slot, n = queue.popleft()
            torch.cuda.current_stream(self.device).wait_event(self._ready[slot])   # device-side wait, the host does not block
            self.tables = self._host[slot]
            return slot, (self._out[slot][:n * self.views], self._tab[slot][1]["labels"][:n])

        i = 0
        for packed in self._dl:
            slot = i % self.depth
            if len(queue) == self.depth:                    # the slot is the oldest batch in flight: hand it out first
                s, item = hand_out()
                yield item
                self._consumed[s].record(torch.cuda.current_stream(self.device))   # queued on the caller's stream by now
            queue.append((slot, self._launch(slot, packed)))
            i += 1
        while queue:
            s, item = hand_out()
            yield item
            self._consumed[s].record(torch.cuda.current_stream(self.device))


class DeviceFrameCache(_Feeder):
    """FrameLoader for a set small enough to live in HBM: every video is decoded once, whole, into one arena on the
    device; an epoch draws segment_indices and boxes on the host, so per batch only clips / frame_idx / boxes travel.

    source: a RubiksDataset or InMemoryVideos (its sampling flags are used), or a list of (uint8 [F, H, W, 3], label) with
    the sampling given by `num_segments` and the other keywords.  budget_bytes: the most HBM the arena may take; a set
    that needs more raises.  Iteration, output shapes and row order are FrameLoader's; work runs on the caller's stream.

    resident="jpeg" (with a RubiksDataset(..., decode="device")) keeps the FILES' bytes in HBM instead of the decoded
    frames, about a sixth of the bytes for ordinary video frames: the files are read and parsed on the host once, their
    entropy-coded segments, tables and a scan index (jpeg.pack_resident; one entry per MCU row) go to the device, and
    rk_jpeg_build_index walks every scan there once.  Per batch the sampling and the boxes are drawn exactly as for "rgb"
    (the same generator calls in the same order), jpeg.pick_tables names the frames the batch reads, one
    rk_jpeg_decode_indexed_u8 launch decodes them -- a chain per MCU row -- into the batch's RGB arena, and the unchanged
    ragged launch follows: with equal seeds clips and labels are bit-identical to "rgb".  budget_bytes counts the blob, the
    entries, the host-decoded frames and one batch's RGB arena and workspace (grown on demand).  Files jpeg.parse_jpeg
    refuses are decoded once with Pillow, stay resident as RGB and are copied into place per batch (`fallback_frames`
    counts them); frames the index build refused come out as zero frames, `decode_errors()` reads how many such frames
    went out so far.  index_build="chunked" (with resident="jpeg") builds the same index with
    rk_jpeg_build_index_chunked instead of one frame-long walk per frame (jpeg.build_index(method="chunked")); `index.route`
    says which frames took which way.

    resident="coef" (the same sources) keeps what the Huffman stage leaves instead of the files: at construction
    jpeg.build_coef transcodes the set once on the device, slab_frames frames at a time, into packed DCT coefficients (per
    block an offset, a 64-bit mask, the DC and the non-zero AC values; index_build chooses the slabs' entropy stage), and
    per batch one rk_jpeg_decode_coef_u8 launch -- no Huffman stage, the same IDCT on the same coefficients -- fills the
    RGB arena: the same sampling, boxes, fallback frames and bit-identical clips, a batch launch some tens of times
    shorter than "jpeg"'s, a footprint between the two others' (content decides: noisy frames pack poorly), and a
    construction that takes the transcode's time.  budget_bytes counts the packed blob, its tables, the records, the
    host-decoded frames, the batch buffers and, while the build runs, a slab's buffers; it is asked before every
    allocation of the build.  coef_record="dense" (with resident="coef") keeps the denser records of
    jpeg.build_coef(record="dense") -- a nibble per small AC value, about two thirds of the "wide" bytes on video frames
    -- decoded by the same launch with another expansion per block; clips stay bit-identical.  A batch stays valid until
    the next one is asked for."""

    def __init__(self, source, batch, split, device="cuda:0", dtype=torch.float32, size=224, views=1, box_fn=None, seed=0,
                 temporal_clips=None, shuffle=None, drop_last=False, flip_p=0.5, budget_bytes=4 << 30, resident="rgb",
                 index_build="chain", slab_frames=256, coef_record="wide", **sampling):
        self.slab_frames = int(slab_frames)
        if resident not in ("rgb", "jpeg", "coef"):
            raise ValueError("resident must be 'rgb' or 'jpeg' or 'coef', got %r" % (resident,))
        if index_build not in ("chain", "chunked"):
            raise ValueError("index_build must be 'chain' or 'chunked', got %r" % (index_build,))
        if index_build == "chunked" and resident not in ("jpeg", "coef"):
            raise ValueError("index_build='chunked' builds the scan index of resident files: it goes with resident='jpeg' or "
                             "'coef', not %r" % (resident,))
        if coef_record not in jpeg.COEF_RECORDS:
            raise ValueError("coef_record must be 'wide' or 'dense', got %r" % (coef_record,))
        if coef_record != "wide" and resident != "coef":
            raise ValueError("coef_record=%r chooses the records of resident='coef': it does not go with resident=%r"
                             % (coef_record, resident))
        self.index_build, self.coef_record = index_build, coef_record
        if resident in ("jpeg", "coef") and not (isinstance(source, RubiksDataset) and source.decode == "device"):
            raise ValueError("resident=%r %s: it needs a RubiksDataset(..., decode='device'), not "
                             "%s" % (resident, "keeps the files' bytes" if resident == "jpeg" else "transcodes the files",
                                     "in-memory videos, which are decoded already" if not isinstance(source, RubiksDataset)
                                     else "a decode='host' dataset"))
        if not isinstance(source, _Sampled):
            videos, labels = zip(*source) if len(source) else ((), ())
            sampling.setdefault("random_shift", split == "train")
            sampling.setdefault("test_mode", split == "test")
            source = InMemoryVideos(list(videos), list(labels), **sampling)
        elif sampling:
            raise ValueError("sampling keywords %r go with in-memory videos; a dataset brings its own" % sorted(sampling))
        if source.split != split:
            raise ValueError("the source samples for split %r, the cache was asked for %r" % (source.split, split))
        self._init_feeder(source, batch, split, device, dtype, size, views, box_fn, temporal_clips, seed, flip_p)
        self.source, self.drop_last = source, drop_last
        self.shuffle = (split == "train") if shuffle is None else shuffle
        self.resident, self.budget_bytes, self.fallback_frames = resident, int(budget_bytes), 0
        if resident in ("jpeg", "coef"):
            self._init_jpeg()
            return
        need, whole = 0, []
        for i in range(len(source)):            # the budget is checked as the videos come, before the device sees a byte
            whole.append(source.whole(i))
            need += whole[-1][0].numel()
            if need > budget_bytes:
                raise RuntimeError("DeviceFrameCache: the first %d of %d videos take %d bytes decoded, over the budget of %d "
                                   "bytes; raise budget_bytes or stream with FrameLoader" % (i + 1, len(source), need,
                                                                                             budget_bytes))
        arena, self.records, self.labels = pack_clips(whole)
        self.arena = arena.pin_memory().to(self.device, non_blocking=True) if arena.numel() else arena.to(self.device)
        self._dev_labels = self.labels.to(self.device)
        _mean_std_on(self.device, IMAGENET_MEAN, IMAGENET_STD)

    def _init_jpeg(self):
        source = self.source
        self.packed = jpeg.pack_resident([source.whole_bytes(i) for i in range(len(source))])
        res = self.packed
        self.labels, self.fallback_frames = res.labels, len(res.fallback)
        self.records = torch.cat([torch.zeros(len(res.videos), 1, dtype=torch.int64), res.videos[:, [2, 3, 1]]], dim=1)
        sizes = [f.numel() for f in res.fallback]
        self._fallback_off = [0] + np.cumsum(sizes).tolist()
        if self.resident == "coef":
            self._init_coef(sizes)
            return
        n_entries = int(res.entry_off[-1])
        tables = res.seg_mcus.numel() * 4 + res.entry_off.numel() * 8 + (int(res.layout[0]) + 1) * 4
        if self.index_build == "chunked":
            tables += int(res.layout[0]) * 4                # the route array stays with the index
        self._fixed_bytes = res.blob.numel() + max(n_entries, 1) * 16 + tables + sum(sizes)
        if self._fixed_bytes > self.budget_bytes:
            raise RuntimeError("DeviceFrameCache: the %d videos take %d bytes as files, over the budget of %d bytes; raise "
                               "budget_bytes or stream with FrameLoader" % (len(source), self._fixed_bytes, self.budget_bytes))
        self.index = jpeg.build_index(res, self.device, method=self.index_build)
        self._fallback = torch.empty(sum(sizes), dtype=torch.uint8, device=self.device)
        for frame, at in zip(res.fallback, self._fallback_off):
            self._fallback[at:at + frame.numel()].copy_(frame.reshape(-1))
        self._host_frames = jpeg.records(res.blob, res.layout).copy()
        self._frame_ws = jpeg.frame_workspace_bytes(self._host_frames)
        self._rgb = self._ws = self._status = None
        self._errors = torch.zeros((), dtype=torch.int64, device=self.device)
        self._dev_labels = self.labels.to(self.device)
        _mean_std_on(self.device, IMAGENET_MEAN, IMAGENET_STD)

    def _init_coef(self, sizes):
        """resident="coef": the files transcoded once, slab by slab, into packed coefficients (jpeg.build_coef).  The budget
        is asked before every allocation of the build -- the finished parts of the blob, the slab's buffers, the
        host-decoded frames -- so a set that does not fit raises before the device holds it."""
        res, fallback = self.packed, sum(sizes)

        self.build_peak_bytes = 0

        def admit(held):
            self.build_peak_bytes = max(self.build_peak_bytes, held + fallback)
            if held + fallback > self.budget_bytes:
                raise RuntimeError("DeviceFrameCache: transcoding the %d videos takes %d bytes on the device, over the budget "
                                   "of %d bytes; raise budget_bytes or stream with FrameLoader"
                                   % (len(self.source), held + fallback, self.budget_bytes))

        self.coef = jpeg.build_coef(res, self.device, method=self.index_build, slab_frames=self.slab_frames, admit=admit,
                                    record=self.coef_record)
        n = self.coef.n
        self._fixed_bytes = self.coef.blob.numel() + n * 64 + self.coef.qtabs.numel() + (n + 1) * 12 + fallback
        self._fallback = torch.empty(fallback, dtype=torch.uint8, device=self.device)
        for frame, at in zip(res.fallback, self._fallback_off):
            self._fallback[at:at + frame.numel()].copy_(frame.reshape(-1))
        self._host_frames = jpeg.records(res.blob, res.layout).copy()
        self._frame_ws = jpeg.frame_plane_bytes(self._host_frames)
        self._rgb = self._ws = self._status = None
        self._errors = torch.zeros((), dtype=torch.int64, device=self.device)
        self._dev_labels = self.labels.to(self.device)
        _mean_std_on(self.device, IMAGENET_MEAN, IMAGENET_STD)

    @property
    def resident_bytes(self):
        """Bytes of HBM the cache holds now: the arena ("rgb"); the blob, the index, the host-decoded frames and the
        batch buffers as far as they have grown ("jpeg"); the packed blob, its tables, the records, the host-decoded frames
        and the batch buffers ("coef"; the build's slab buffers are gone by the time anyone can ask)."""
        if self.resident == "rgb":
            return self.arena.numel()
        return self._fixed_bytes + sum(t.numel() * t.element_size() for t in (self._rgb, self._ws, self._status) if t is not None)

    def decode_errors(self):
        """Frames that went out as zero frames so far because the device refused them (resident="jpeg" or "coef"; 0
        otherwise).  Waits for the device: ask once, at the end of an epoch."""
        return int(self._errors.item()) if self.resident != "rgb" else 0

    def _grown(self, t, need, make):
        """FrameLoader._grown under the budget: the batch buffers grow on demand, and count."""
        if t is not None and t.numel() >= need:
            return t
        new = make(need + need // 4)
        have = self.resident_bytes - (t.numel() * t.element_size() if t is not None else 0)
        if have + new.numel() * new.element_size() > self.budget_bytes:
            raise RuntimeError("DeviceFrameCache: a batch needs a buffer of %d bytes beside the %d resident, over the budget "
                               "of %d bytes" % (new.numel() * new.element_size(), have, self.budget_bytes))
        return new

    def _decode_batch(self, ids, numbers):
        """resident="jpeg": the frames `numbers` (0-based, per video of `ids`) decoded into the batch's RGB arena ->
        (arena, clips rows for it, per-video frame numbers remapped into it)."""
        t = jpeg.pick_tables(self.packed, ids.tolist(), numbers)
        m = t.pick.numel()
        self._rgb = self._grown(self._rgb, t.rgb_bytes, lambda k: torch.empty(k, dtype=torch.uint8, device=self.device))
        rgb = self._rgb[:t.rgb_bytes]
        if m:
            if self.resident == "coef":
                need = jpeg.coef_workspace_bytes_for(self._host_frames, t.pick.numpy(), self._frame_ws)
            else:
                need = jpeg.indexed_workspace_bytes_for(self._host_frames, t.pick.numpy(), t.max_segments, self._frame_ws)
            self._ws = self._grown(self._ws, need, lambda k: torch.empty(k, dtype=torch.uint8, device=self.device))
            self._status = self._grown(self._status, m + 1, lambda k: torch.zeros(k, dtype=torch.int32, device=self.device))
            with _near_gpu(self.device):
                pick, rgb_off = t.pick.pin_memory(), t.rgb_off.pin_memory()
            status = self._status[:m + 1]
            pick, rgb_off = pick.to(self.device, non_blocking=True), rgb_off.to(self.device, non_blocking=True)
            if self.resident == "coef":
                jpeg.launch_decode_coef(self.coef, pick, rgb_off, rgb, self._ws, status)
            else:
                jpeg.launch_decode_indexed(self.index, pick, rgb_off, t.max_segments, rgb, self._ws, status)
            self._errors += status[m]
        for f, off in t.fallback:
            at, k = self._fallback_off[f], self._fallback_off[f + 1] - self._fallback_off[f]
            rgb[off:off + k].copy_(self._fallback[at:at + k])
        return rgb, t.clips, t.frame_idx

    def __len__(self):
        n = len(self.source)
        return n // self.batch if self.drop_last else (n + self.batch - 1) // self.batch

    def __iter__(self):
        n = len(self.source)
        order = torch.randperm(n, generator=self._gen) if self.shuffle else torch.arange(n)
        for b in range(len(self)):
            ids = order[b * self.batch:(b + 1) * self.batch]
            clips = self.records[ids]
            if self.resident != "rgb":
                numbers =[(torch.tensor(self.source.frame_numbers(nf, self._gen), dtype=torch.int64).clamp_(1, nf) - 1).tolist()
                           for nf in clips[:, 3].tolist()]
                boxes = self._boxes([(int(h), int(w)) for h, w in clips[:, 1:3].tolist()])
                arena, clips, local = self._decode_batch(ids, numbers)
                rows = []
                for p in local:
                    p = torch.from_numpy(p).to(torch.int32)
                    T = p.numel() // self.temporal_clips
                    rows.append(p[_temporal_index(p.numel(), self.temporal_clips, self.crops).long()].view(-1, T))
                frame_idx = torch.cat(rows)
                out = augment.ragged_u8_to_clips(arena, clips, frame_idx, boxes, self.size, views=self.views, dtype=self.dtype)
                self.tables = {"videos": ids, "clips": clips, "frame_idx": frame_idx, "boxes": boxes, "labels": self.labels[ids]}
                yield out, self._dev_labels[ids.to(self.device)]
                continue
            rows = []
            for _, _, _, nf in clips.tolist():
                p = torch.tensor(self.source.frame_numbers(nf, self._gen), dtype=torch.int32).clamp_(1, nf) - 1
                T = p.numel() // self.temporal_clips
                rows.append(p[_temporal_index(p.numel(), self.temporal_clips, self.crops).long()].view(-1, T))
            frame_idx = torch.cat(rows)
            boxes = self._boxes([(int(h), int(w)) for h, w in clips[:, 1:3].tolist()])
            out = augment.ragged_u8_to_clips(self.arena, clips, frame_idx, boxes, self.size, views=self.views,
                                             dtype=self.dtype)
            self.tables = {"videos": ids, "clips": clips, "frame_idx": frame_idx, "boxes": boxes, "labels": self.labels[ids]}
            yield out, self._dev_labels[ids.to(self.device)]
