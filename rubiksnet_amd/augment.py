"""Crop, resize and flip on the device: the head of the reference's transform chain.

The reference augments every frame with PIL on CPU workers (rubiksnet/transforms.py): training runs
`GroupMultiScaleCrop` (a crop, then `Image.resize(..., BILINEAR)`) and `GroupRandomHorizontalFlip`; evaluation runs
`GroupScale` + `GroupCenterCrop`, `GroupFullResSample` (3 crops x flip) or `GroupOverSample` (5 crops x flip).  Here
the host only draws BOXES -- nine int32 per output clip, `(x0, y0, cw, ch, rw, rh, ox, oy, flip)` -- and one HIP kernel
(rk_clip_resample_u8_*, csrc/rk_resample.hip) turns decoded uint8 frames [B, T, Hs, Ws, 3] into the network's input
[B * V, T, 3, Sh, Sw]: crop [y0 : y0 + ch, x0 : x0 + cw] -> Pillow-exact bilinear resize to rw x rh -> window
[oy : oy + Sh, ox : ox + Sw] -> mirror if flip -> ((v / 255) - mean) / std.  The fp32 result is bit-identical to the
reference's chain; all T frames of a clip share one box, as in the reference.

Real sets are ragged (one height and many widths, or both) and a clip is a choice of frames of a longer video:
`ragged_u8_to_clips` (rk_clip_resample_ragged_u8_*) is the same pass from a packed byte arena with one record per video
and a per-frame index table; `per_clip_boxes` draws each clip's boxes for its own frame size (dataset.py feeds it).

Sizes follow the project's (height, width) order: `frame_hw`, `out_hw`; an int means a square.  The random draws come
from a `torch.Generator` (the set of choices is the reference's, the stream is not Python's `random`).
"""
import torch

from . import _native
from .input_pipeline import IMAGENET_MEAN, IMAGENET_STD, _SFX, _mean_std_on, _near_gpu

__all__ = ["multiscale_crop_boxes", "center_crop_boxes", "full_res_boxes", "oversample_boxes", "check_boxes",
           "crop_candidates", "fix_offsets", "short_edge_size", "frames_u8_to_clips", "SyntheticFrameLoader",
           "MAX_RATIO", "BOX_FIELDS", "per_clip_boxes", "check_ragged", "ragged_u8_to_clips", "MAX_SIDE"]

BOX_FIELDS = ("x0", "y0", "cw", "ch", "rw", "rh", "ox", "oy", "flip")
MAX_RATIO = 8          # cw / rw and ch / rh: 17 filter taps (csrc/rk_resample.hip kTaps)
MAX_SIDE = 16384       # the largest Hs or Ws a record of the ragged entry may claim (csrc/rk_resample.hip kMaxSide)


def _hw(size):
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


# ------------------------------------------------------------------------------------------------- the reference's rules
def crop_candidates(frame_hw, input_size, scales=(1, .875, .75, .66), max_distort=1):
    """The (crop_w, crop_h) pairs GroupMultiScaleCrop chooses from (transforms.py:217-236): the short edge times every
    scale, snapped to the input size when within 3 of it, width i with height j for |i - j| <= max_distort."""
    hs, ws = _hw(frame_hw)
    sh, sw = _hw(input_size)
    base = min(ws, hs)
    sizes = [int(base * s) for s in scales]
    crop_h = [sh if abs(x - sh) < 3 else x for x in sizes]
    crop_w = [sw if abs(x - sw) < 3 else x for x in sizes]
    return [(w, h) for i, h in enumerate(crop_h) for j, w in enumerate(crop_w) if abs(i - j) <= max_distort]


def fix_offsets(more_fix_crop, image_w, image_h, crop_w, crop_h):
    """The 5 (or 13) fixed (x, y) crop offsets of GroupMultiScaleCrop.fill_fix_offset (transforms.py:255-278)."""
    ws, hs = (image_w - crop_w) // 4, (image_h - crop_h) // 4
    ret = [(0, 0), (4 * ws, 0), (0, 4 * hs), (4 * ws, 4 * hs), (2 * ws, 2 * hs)]      # corners, centre
    if more_fix_crop:
        ret += [(0, 2 * hs), (4 * ws, 2 * hs), (2 * ws, 4 * hs), (2 * ws, 0),           # edge centres
                (ws, hs), (3 * ws, hs), (ws, 3 * hs), (3 * ws, 3 * hs)]                 # quarters
    return ret


def short_edge_size(frame_hw, size):
    """(rh, rw) of GroupScale(size), i.e. torchvision.transforms.Resize(size) with an int: the short edge becomes `size`,
    w <= h: (w, h) -> (size, int(size * h / w)); otherwise: (int(size * w / h), size).  None keeps the frame."""
    hs, ws = _hw(frame_hw)
    if size is None:
        return hs, ws
    size = int(size)
    if ws <= hs:
        return int(size * hs / ws), size
    return size, int(size * ws / hs)


def _randint(n, generator):
    return int(torch.randint(n, (1,), generator=generator))


def _as_boxes(rows):
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 9)


# ------------------------------------------------------------------------------------------------- box builders
def multiscale_crop_boxes(batch, frame_hw, input_size, scales=(1, .875, .75, .66), max_distort=1, fix_crop=True,
                          more_fix_crop=True, flip_p=0.5, generator=None):
    """GroupMultiScaleCrop + GroupRandomHorizontalFlip: one box per clip, int32 [batch, 9] on the CPU.  A crop pair is
    drawn from crop_candidates(), its offset from fix_offsets() (uniform over the frame when fix_crop is off), the flip
    with probability flip_p (0 for direction-labelled datasets such as Something-Something)."""
    hs, ws = _hw(frame_hw)
    sh, sw = _hw(input_size)
    pairs = crop_candidates(frame_hw, input_size, scales, max_distort)
    rows = []
    for _ in range(batch):
        cw, ch = pairs[_randint(len(pairs), generator)]
        if fix_crop:
            offs = fix_offsets(more_fix_crop, ws, hs, cw, ch)
            x0, y0 = offs[_randint(len(offs), generator)]
        else:
            x0, y0 = _randint(ws - cw + 1, generator), _randint(hs - ch + 1, generator)
        flip = int(float(torch.rand((), generator=generator)) < flip_p)
        rows.append((x0, y0, cw, ch, sw, sh, 0, 0, flip))
    return _as_boxes(rows)


def _view_boxes(batch, frame_hw, scale_size, offsets, flip):
    hs, ws = _hw(frame_hw)
    rh, rw = short_edge_size(frame_hw, scale_size)
    views = []
    for ox, oy in offsets:                     # the reference's order: per offset, the plain view, then its flip
        views.append((0, 0, ws, hs, rw, rh, ox, oy, 0))
        if flip:
            views.append((0, 0, ws, hs, rw, rh, ox, oy, 1))
    return _as_boxes(views * batch)


def center_crop_boxes(batch, frame_hw, scale_size, crop_size):
    """GroupScale(scale_size) + GroupCenterCrop(crop_size): V = 1.  The offset is torchvision's CenterCrop one,
    int(round((h - crop_h) / 2.0)), int(round((w - crop_w) / 2.0))."""
    ch, cw = _hw(crop_size)
    rh, rw = short_edge_size(frame_hw, scale_size)
    return _view_boxes(batch, frame_hw, scale_size, [(int(round((rw - cw) / 2.0)), int(round((rh - ch) / 2.0)))], False)


def full_res_boxes(batch, frame_hw, crop_size, scale_size=None, flip=True):
    """GroupFullResSample (transforms.py:141-186): left, right, centre crops at mid height; V = 3, or 6 with flip."""
    ch, cw = _hw(crop_size)
    rh, rw = short_edge_size(frame_hw, scale_size)
    ws, hs = (rw - cw) // 4, (rh - ch) // 4
    return _view_boxes(batch, frame_hw, scale_size, [(0, 2 * hs), (4 * ws, 2 * hs), (2 * ws, 2 * hs)], flip)


def oversample_boxes(batch, frame_hw, crop_size, scale_size=None, flip=True):
    """GroupOverSample (transforms.py:98-138): four corners and the centre; V = 5, or 10 with flip."""
    ch, cw = _hw(crop_size)
    rh, rw = short_edge_size(frame_hw, scale_size)
    return _view_boxes(batch, frame_hw, scale_size, fix_offsets(False, rw, rh, cw, ch), flip)


def check_boxes(boxes, frame_hw, out_hw):
    """Raise ValueError unless every box is one the kernel defines a result for: the crop non-empty and inside the
    frame, rw and rh positive, the window inside rw x rh, cw / rw and ch / rh at most MAX_RATIO.  Pure CPU."""
    hs, ws = _hw(frame_hw)
    sh, sw = _hw(out_hw)
    b = torch.as_tensor(boxes)
    if b.is_cuda:
        raise ValueError("check_boxes checks host boxes (device boxes are trusted)")
    if b.dim() != 2 or b.shape[1] != 9 or b.dtype != torch.int32:
        raise ValueError("boxes must be int32 [n, 9] (%s), got %s %s" % (", ".join(BOX_FIELDS), b.dtype, tuple(b.shape)))
    if sh <= 0 or sw <= 0:
        raise ValueError("empty output size %r" % ((sh, sw),))
    x0, y0, cw, ch, rw, rh, ox, oy, _ = (b[:, i].to(torch.int64) for i in range(9))

    def bad(mask, what):
        if bool(mask.any()):
            i = int(mask.nonzero()[0])
            raise ValueError("box %d %r: %s (frame %dx%d, output %dx%d)" % (i, tuple(b[i].tolist()), what, hs, ws, sh, sw))

    bad((cw <= 0) | (ch <= 0), "empty crop")
    bad((rw <= 0) | (rh <= 0), "empty resize target")
    bad((x0 < 0) | (y0 < 0) | (x0 + cw > ws) | (y0 + ch > hs), "crop outside the frame")
    bad((ox < 0) | (oy < 0) | (ox + sw > rw) | (oy + sh > rh), "window outside the resized crop")
    bad((cw > MAX_RATIO * rw) | (ch > MAX_RATIO * rh), "downscaling ratio above %d" % MAX_RATIO)


# ------------------------------------------------------------------------------------------------- the device entry point
def frames_u8_to_clips(frames, boxes, out_hw, views=1, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=torch.float32,
                       out=None):
    """frames: uint8 [B, T, Hs, Ws, 3] on the GPU, contiguous, RGB.  boxes: int32 [B * views, 9]; on the CPU they are
    checked (check_boxes) and copied through pinned memory without blocking, on the device they are trusted (the kernel
    clamps its reads whatever they hold).  Returns [B * views, T, 3, Sh, Sw] in `dtype` (float32 or bfloat16); view v of
    clip b is row b * views + v, so `.view(B, views * T * 3, Sh, Sw)` is what evaluation.evaluate(..., views=views) takes."""
    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 5 and frames.shape[-1] == 3
            and frames.is_contiguous()):
        raise RuntimeError("frames must be a contiguous CUDA (HIP) uint8 tensor [B, T, Hs, Ws, 3] (no CPU fallback)")
    if dtype not in _SFX:
        raise ValueError("dtype must be float32 or bfloat16, got %s" % dtype)
    B, T, Hs, Ws, _ = frames.shape
    sh, sw = _hw(out_hw)
    views = int(views)
    if views < 1:
        raise ValueError("views must be >= 1")
    if tuple(boxes.shape) != (B * views, 9) or boxes.dtype != torch.int32:
        raise ValueError("boxes must be int32 [B * views, 9] = [%d, 9], got %s %s" % (B * views, boxes.dtype, tuple(boxes.shape)))
    dev = frames.device
    if boxes.is_cuda:
        if boxes.device != dev or not boxes.is_contiguous():
            raise RuntimeError("device boxes must be contiguous and on the frames' device")
    else:
        check_boxes(boxes, (Hs, Ws), (sh, sw))
        boxes = boxes.contiguous().pin_memory().to(dev, non_blocking=True)
    if out is None:
        out = torch.empty(B * views, T, 3, sh, sw, dtype=dtype, device=dev)
    elif tuple(out.shape) != (B * views, T, 3, sh, sw) or out.dtype != dtype or not out.is_contiguous() or out.device != dev:
        raise RuntimeError("out must be a contiguous %s tensor [B * views, T, 3, Sh, Sw] on the frames' device" % dtype)
    ms = _mean_std_on(dev, mean, std)
    if B and T:
        _native.launch("rk_clip_resample_u8_" + _SFX[dtype], dev, frames.data_ptr(), boxes.data_ptr(), ms[0].data_ptr(),
                       ms[1].data_ptr(), out.data_ptr(), B, T, Hs, Ws, views, sh, sw)
    return out


# ------------------------------------------------------------------------------------------------- videos of different sizes
def per_clip_boxes(sizes, fn):
    """Boxes for clips whose frames differ in size: `fn((H, W))` -> int32 [views, 9] is called once per entry of `sizes`
    (an iterable of (H, W)), e.g. `lambda hw: full_res_boxes(1, hw, 224, flip=False)`, and must return the same number of
    views every time.  Returns int32 [len(sizes) * views, 9], clip-major: what ragged_u8_to_clips takes."""
    rows, views = [], None
    for i, hw in enumerate(sizes):
        b = torch.as_tensor(fn(_hw(hw)))
        if b.dim() != 2 or b.shape[1] != 9 or b.dtype != torch.int32 or b.shape[0] < 1:
            raise ValueError("fn must return int32 [views, 9], got %s %s for clip %d" % (b.dtype, tuple(b.shape), i))
        if views is None:
            views = b.shape[0]
        elif b.shape[0] != views:
            raise ValueError("fn returned %d views for clip %d and %d for the clips before it" % (b.shape[0], i, views))
        rows.append(b)
    return torch.cat(rows) if rows else torch.zeros(0, 9, dtype=torch.int32)


def check_ragged(arena_bytes, clips, frame_idx, boxes, out_hw, views=1):
    """Raise ValueError unless the host tables describe a launch rk_clip_resample_ragged_u8_* defines a picture for:
    clips int64 [B, 4] of (byte offset, Hs, Ws, F) with every record inside `arena_bytes`, frame_idx int32 [B * views, T]
    with every index a stored frame of its own video, boxes int32 [B * views, 9] each valid for its own video's frame size
    (check_boxes).  Pure CPU; returns (B, T)."""
    views = int(views)
    if views < 1:
        raise ValueError("views must be >= 1")
    clips, frame_idx, boxes = torch.as_tensor(clips), torch.as_tensor(frame_idx), torch.as_tensor(boxes)
    if clips.is_cuda or frame_idx.is_cuda or boxes.is_cuda:
        raise ValueError("check_ragged checks host tables (device tables are trusted)")
    if clips.dim() != 2 or clips.shape[1] != 4 or clips.dtype != torch.int64:
        raise ValueError("clips must be int64 [B, 4] (byte offset, Hs, Ws, F), got %s %s" % (clips.dtype, tuple(clips.shape)))
    B = clips.shape[0]
    if frame_idx.dim() != 2 or frame_idx.shape[0] != B * views or frame_idx.dtype != torch.int32:
        raise ValueError("frame_idx must be int32 [B * views, T] = [%d, T], got %s %s" % (B * views, frame_idx.dtype,
                                                                                        tuple(frame_idx.shape)))
    if tuple(boxes.shape) != (B * views, 9) or boxes.dtype != torch.int32:
        raise ValueError("boxes must be int32 [B * views, 9] = [%d, 9], got %s %s" % (B * views, boxes.dtype, tuple(boxes.shape)))
    for b, (off, hs, ws, nf) in enumerate(clips.tolist()):
        if not (1 <= hs <= MAX_SIDE and 1 <= ws <= MAX_SIDE):
            raise ValueError("clip %d: frame size %dx%d outside [1, %d]" % (b, hs, ws, MAX_SIDE))
        if nf < 1:
            raise ValueError("clip %d: %d frames" % (b, nf))
        if off < 0 or off + nf * hs * ws * 3 > arena_bytes:
            raise ValueError("clip %d: bytes [%d, %d) lie outside the arena of %d bytes" % (b, off, off + nf * hs * ws * 3,
                                                                                         arena_bytes))
        idx = frame_idx[b * views:(b + 1) * views]
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= nf):
            raise ValueError("clip %d: frame index outside [0, %d)" % (b, nf))
        try:
            check_boxes(boxes[b * views:(b + 1) * views], (hs, ws), out_hw)
        except ValueError as e:
            raise ValueError("clip %d: %s" % (b, e)) from None
    return B, frame_idx.shape[1]


def ragged_u8_to_clips(arena, clips, frame_idx, boxes, out_hw, views=1, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                       dtype=torch.float32, out=None):
    """frames_u8_to_clips for videos of different sizes and chosen frames (rk_clip_resample_ragged_u8_*).  arena: uint8
    [bytes] on the GPU, contiguous: the videos back to back (dataset.pack_clips).  clips: int64 [B, 4], per video (byte
    offset of its first frame, Hs, Ws, F).  frame_idx: int32 [B * views, T], the stored frame (0-based) each output frame
    shows.  boxes: int32 [B * views, 9], each for its own video's frame size.  Tables on the CPU are checked (check_ragged)
    and copied through pinned memory without blocking; tables on the device are trusted (the kernel clamps indices and
    boxes, and writes zeros for a record that does not fit the arena).  Returns [B * views, T, 3, Sh, Sw] in `dtype`."""
    if dtype not in _SFX:
        raise ValueError("dtype must be float32 or bfloat16, got %s" % dtype)
    views = int(views)
    if views < 1:
        raise ValueError("views must be >= 1")
    if not (torch.is_tensor(arena) and arena.dtype == torch.uint8 and arena.dim() == 1):
        raise ValueError("arena must be a uint8 tensor [bytes]")
    sh, sw = _hw(out_hw)
    tables = (clips, frame_idx, boxes)
    if all(not t.is_cuda for t in tables):
        B, T = check_ragged(arena.numel(), clips, frame_idx, boxes, (sh, sw), views)
    elif all(t.is_cuda for t in tables):
        if clips.dim() != 2 or clips.shape[1] != 4 or clips.dtype != torch.int64:
            raise ValueError("clips must be int64 [B, 4], got %s %s" % (clips.dtype, tuple(clips.shape)))
        B = clips.shape[0]
        if frame_idx.dim() != 2 or frame_idx.shape[0] != B * views or frame_idx.dtype != torch.int32:
            raise ValueError("frame_idx must be int32 [B * views, T] = [%d, T], got %s %s" % (B * views, frame_idx.dtype,
                                                                                            tuple(frame_idx.shape)))
        if tuple(boxes.shape) != (B * views, 9) or boxes.dtype != torch.int32:
            raise ValueError("boxes must be int32 [B * views, 9] = [%d, 9], got %s %s" % (B * views, boxes.dtype,
                                                                                         tuple(boxes.shape)))
        T = frame_idx.shape[1]
    else:
        raise ValueError("clips, frame_idx and boxes must be all on the CPU (checked) or all on the device (trusted)")
    if not (arena.is_cuda and arena.is_contiguous()):
        raise RuntimeError("arena must be a contiguous CUDA (HIP) uint8 tensor (no CPU fallback)")
    dev = arena.device
    if clips.is_cuda:
        if any(t.device != dev or not t.is_contiguous() for t in tables):
            raise RuntimeError("device tables must be contiguous and on the arena's device")
    else:
        clips, frame_idx, boxes = (t.contiguous().pin_memory().to(dev, non_blocking=True) for t in tables)
    if out is None:
        out = torch.empty(B * views, T, 3, sh, sw, dtype=dtype, device=dev)
    elif tuple(out.shape) != (B * views, T, 3, sh, sw) or out.dtype != dtype or not out.is_contiguous() or out.device != dev:
        raise RuntimeError("out must be a contiguous %s tensor [B * views, T, 3, Sh, Sw] on the arena's device" % dtype)
    ms = _mean_std_on(dev, mean, std)
    if B and T:
        _native.launch("rk_clip_resample_ragged_u8_" + _SFX[dtype], dev, arena.data_ptr(), arena.numel(), clips.data_ptr(),
                       frame_idx.data_ptr(), boxes.data_ptr(), ms[0].data_ptr(), ms[1].data_ptr(), out.data_ptr(), B, views, T,
                       sh, sw)
    return out


class SyntheticFrameLoader:
    """Endless iterator of (clips [B, T, 3, size, size] normalised, labels [B]) on `device`, augmented on the device.

    SyntheticClipLoader's sibling one step further up the chain: the pinned host buffers hold random decoded FRAMES
    [B, T, Hs, Ws, 3] (default 256 x 340, the reference's), and every batch gets fresh multiscale-crop + flip boxes,
    drawn on the host into a pinned [B, 9] buffer.  The copies and the kernel run on a side stream under the same event
    protocol (`ready` / `consumed` per slot, the caller's stream waits on the device).  A slot's pinned boxes are
    rewritten only after the copy that last read them has completed: the host waits on that copy's event, which was
    queued `depth` batches earlier, so it waits only when it has run more than `depth` batches ahead of the device.

    `box_fn(batch, generator)` -> int32 [batch * views, 9] replaces the training boxes, e.g. with full_res_boxes for an
    evaluation feed; the clips then come as [B * views, T, 3, size, size]."""

    def __init__(self, batch, n_frames=8, frame_hw=(256, 340), size=224, num_classes=174, device="cuda:0",
                 dtype=torch.float32, seed=0, depth=2, flip_p=0.5, views=1, box_fn=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SyntheticFrameLoader feeds a GPU (no CPU path)")
        self._gen = torch.Generator().manual_seed(seed)
        g = self._gen
        hs, ws = _hw(frame_hw)
        self.n_frames, self.dtype, self.frame_hw, self.size, self.flip_p = n_frames, dtype, (hs, ws), _hw(size), flip_p
        self.views = int(views)
        self._box_fn = box_fn or (lambda n, gen: multiscale_crop_boxes(n, self.frame_hw, self.size, flip_p=self.flip_p,
                                                                      generator=gen))
        with _near_gpu(self.device):
            self._host = [torch.randint(0, 256, (batch, n_frames, hs, ws, 3), dtype=torch.uint8, generator=g).pin_memory()
                          for _ in range(depth)]
            self._labels = [torch.randint(0, num_classes, (batch,), generator=g).pin_memory() for _ in range(depth)]
            self._host_boxes = [torch.zeros(batch * self.views, 9, dtype=torch.int32).pin_memory() for _ in range(depth)]
        self._stage = [torch.empty_like(h, device=self.device) for h in self._host]
        self._boxes = [torch.empty_like(b, device=self.device) for b in self._host_boxes]
        self._out = [torch.empty(batch * self.views, n_frames, 3, *self.size, dtype=dtype, device=self.device) for _ in range(depth)]
        self._lab = [torch.empty_like(l, device=self.device) for l in self._labels]
        self._ready = [torch.cuda.Event() for _ in range(depth)]
        self._consumed = [torch.cuda.Event() for _ in range(depth)]
        self._boxes_copied = [None] * depth
        self._stream = torch.cuda.Stream(self.device)
        _mean_std_on(self.device, IMAGENET_MEAN, IMAGENET_STD)      # the one blocking upload happens here, not per batch
        self._i = 0
        for slot in range(depth):
            self._consumed[slot].record(torch.cuda.current_stream(self.device))
            self._launch(slot)

    def _launch(self, slot):
        """Draw the slot's boxes, then queue copies + kernel of its next batch on the side stream."""
        boxes = self._box_fn(self._host[slot].shape[0], self._gen)
        check_boxes(boxes, self.frame_hw, self.size)
        if self._boxes_copied[slot] is not None:
            self._boxes_copied[slot].synchronize()          # the copy queued one round ago: long done in steady state
        self._host_boxes[slot].copy_(boxes)
        with torch.cuda.stream(self._stream):
            self._stream.wait_event(self._consumed[slot])
            self._stage[slot].copy_(self._host[slot], non_blocking=True)
            self._lab[slot].copy_(self._labels[slot], non_blocking=True)
            self._boxes[slot].copy_(self._host_boxes[slot], non_blocking=True)
            if self._boxes_copied[slot] is None:
                self._boxes_copied[slot] = torch.cuda.Event()
            self._boxes_copied[slot].record(self._stream)
            frames_u8_to_clips(self._stage[slot], self._boxes[slot], self.size, views=self.views, dtype=self.dtype,
                               out=self._out[slot])
            self._ready[slot].record(self._stream)

    def __iter__(self):
        return self

    def __next__(self):
        depth = len(self._host)
        slot = self._i % depth
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self._ready[slot])                            # device-side wait, the host does not block
        if self._i > 0:
            prev = (self._i - 1) % depth                             # the batch handed out one call ago is queued on `cur`
            self._consumed[prev].record(cur)
            self._launch(prev)
        self._i += 1
        return self._out[slot], self._lab[slot]
