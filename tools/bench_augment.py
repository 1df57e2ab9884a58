#!/usr/bin/env python
"""Times the device crop / resize / flip kernel (rk_clip_resample_u8_*) beside its nearest yardstick, the transform
tail rk_clip_u8_to_chw_* at the same output size, and beside the bytes it has to move; then the augmenting loader.

    python tools/bench_augment.py [--clips 32] [--frames 8] [--iters 50] [--out profiles/augment_timing.json]
                                  [--ragged-out profiles/ragged_resample_time.txt] [--workers 8]

Device events around `iters` back-to-back launches, after a warm-up, median of 5 windows.  Bytes = the source bytes
under the taps of every output clip (rows x run of columns x 3, per frame) + the output written; the rate is those
bytes over the time, so it is comparable with the tail's (1 B read + 4 or 2 B written per element).

The ragged legs: rk_clip_resample_ragged_u8_* on the same uniform batch, alternated with rk_clip_resample_u8_* in this
process, three runs each (a run = the median of 5 windows), and on a mixed-width batch (height 240, widths 320 .. 427);
then dataset.DeviceFrameCache and dataset.FrameLoader over in-memory videos of those sizes beside SyntheticFrameLoader.
The FrameLoader figure has no JPEG decoding in it: it is what packing, the worker hand-over and the copy can feed."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rubiksnet_amd import augment, dataset  # noqa: E402
from rubiksnet_amd.input_pipeline import SyntheticClipLoader, stacked_u8_to_clips  # noqa: E402


def tap_span(n, m, first, count):
    """Source samples [lo, hi) under the taps of outputs first .. first + count - 1 of an axis resampled n -> m."""
    scale = n / m
    support = max(scale, 1.0)
    lo = max(int((first + 0.5) * scale - support + 0.5), 0)
    hi = min(int((first + count - 0.5) * scale + support + 0.5), n)
    return lo, hi


def source_bytes(boxes, T, out_hw):
    total = 0
    for x0, y0, cw, ch, rw, rh, ox, oy, _ in boxes.tolist():
        xl, xh = tap_span(cw, rw, ox, out_hw[1])
        yl, yh = tap_span(ch, rh, oy, out_hw[0])
        total += (xh - xl) * (yh - yl) * 3 * T
    return total


def time_ms(fn, iters, windows=5):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / iters)
    return statistics.median(times), min(times), max(times)


def ragged_legs(dev, frames, boxes, S, iters, gen):
    """[(label, dtype name, [ms of each run])]: uniform entry and ragged entry alternated on `frames`, then the ragged
    entry on a mixed-width batch of the same clip and frame counts."""
    B, T, hs, ws, _ = frames.shape
    clips = torch.tensor([(b * T * hs * ws * 3, hs, ws, T) for b in range(B)], dtype=torch.int64).to(dev)
    frame_idx = torch.arange(T, dtype=torch.int32).repeat(B, 1).to(dev)
    dboxes = boxes.to(dev)
    widths = [320 + (427 - 320) * b // max(B - 1, 1) for b in range(B)]
    mixed_rows, off = [], 0
    for w in widths:
        mixed_rows.append((off, 240, w, T))
        off += T * 240 * w * 3
    mixed_arena = torch.randint(0, 256, (off,), dtype=torch.uint8, generator=gen).to(dev)
    mixed_boxes = augment.per_clip_boxes([(240, w) for w in widths],
                                         lambda hw: augment.multiscale_crop_boxes(1, hw, S, generator=gen))
    mixed_clips = torch.tensor(mixed_rows, dtype=torch.int64)
    augment.check_ragged(off, mixed_clips, frame_idx.cpu(), mixed_boxes, S)
    mixed_clips, mixed_boxes = mixed_clips.to(dev), mixed_boxes.to(dev)
    legs = []
    for dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        out = torch.empty(B, T, 3, S, S, dtype=dtype, device=dev)
        uniform = lambda: augment.frames_u8_to_clips(frames, dboxes, S, dtype=dtype, out=out)                      # noqa: E731
        ragged = lambda: augment.ragged_u8_to_clips(frames.view(-1), clips, frame_idx, dboxes, S, dtype=dtype, out=out)  # noqa: E731
        mixed = lambda: augment.ragged_u8_to_clips(mixed_arena, mixed_clips, frame_idx, mixed_boxes, S, dtype=dtype, out=out)  # noqa: E731
        want = uniform().clone()
        assert torch.equal(ragged(), want), "the ragged entry differs from the uniform one on the uniform batch"
        runs = {"uniform": [], "ragged": [], "mixed": []}
        for _ in range(3):
            runs["uniform"].append(time_ms(uniform, iters)[0])
            runs["ragged"].append(time_ms(ragged, iters)[0])
        for _ in range(3):
            runs["mixed"].append(time_ms(mixed, iters)[0])
        legs += [("rk_clip_resample_u8_%s, uniform %dx%d" % (name, hs, ws), runs["uniform"]),
                 ("rk_clip_resample_ragged_u8_%s, uniform %dx%d" % (name, hs, ws), runs["ragged"]),
                 ("rk_clip_resample_ragged_u8_%s, 240 x 320..427" % name, runs["mixed"])]
    return legs


def feeder_rates(dev, B, T, S, batches, workers, gen):
    """clips/s of the two real-data feeders over in-memory videos (height 240, widths 320 .. 427, 2 T frames each)."""
    n = 4 * B
    videos = [torch.randint(0, 256, (2 * T, 240, 320 + (427 - 320) * i // (n - 1), 3), dtype=torch.uint8, generator=gen)
              for i in range(n)]
    ds = dataset.InMemoryVideos(videos, [i % 174 for i in range(n)], num_segments=T, only_even_indices=False)
    rates = []
    for label, make in (("DeviceFrameCache", lambda: dataset.DeviceFrameCache(ds, B, "train", device=dev, size=S)),
                        ("FrameLoader, %d workers" % workers,
                         lambda: dataset.FrameLoader(ds, B, "train", device=dev, size=S, num_workers=workers))):
        feeder = make()

        def take(count):
            done = 0
            while done < count:
                for _ in feeder:
                    done += 1
                    if done == count:
                        break

        take(4)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        take(batches)
        b.record()
        b.synchronize()
        rates.append((label, batches * B / (a.elapsed_time(b) / 1e3)))
        del feeder
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--loader-batches", type=int, default=60)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ragged-out", default=None, help="text file for the ragged legs and the feeders' rates")
    ap.add_argument("--workers", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_augment.py needs a GPU"
    dev = torch.device("cuda:0")
    B, T, hw, S = args.clips, args.frames, (256, 340), 224
    gen = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (B, T, hw[0], hw[1], 3), dtype=torch.uint8, generator=gen).to(dev)
    stacked = torch.randint(0, 256, (B, S, S, 3 * T), dtype=torch.uint8, generator=gen).to(dev)
    mixes = {"multiscale_mix": augment.multiscale_crop_boxes(B, hw, S, generator=gen),
             "centre_crop": augment.center_crop_boxes(B, hw, 256, S)}
    result = {"device": torch.cuda.get_device_name(0), "clips": B, "frames": T, "source_hw": list(hw), "output": S,
              "iters": args.iters, "kernels": []}
    for dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        out = torch.empty(B, T, 3, S, S, dtype=dtype, device=dev)
        out_bytes = out.numel() * out.element_size()
        med, lo, hi = time_ms(lambda: stacked_u8_to_clips(stacked, T, dtype=dtype, out=out.view(B, 3 * T, S, S)), args.iters)
        moved = stacked.numel() + out_bytes
        result["kernels"].append({"kernel": "rk_clip_u8_to_chw_" + name, "boxes": None, "ms": med, "ms_min": lo, "ms_max": hi,
                                  "bytes": moved, "TBps": moved / med / 1e9})
        for mix, boxes in mixes.items():
            augment.check_boxes(boxes, hw, S)
            dboxes = boxes.to(dev)
            med, lo, hi = time_ms(lambda: augment.frames_u8_to_clips(frames, dboxes, S, dtype=dtype, out=out), args.iters)
            moved = source_bytes(boxes, T, (S, S)) + out_bytes
            result["kernels"].append({"kernel": "rk_clip_resample_u8_" + name, "boxes": mix, "ms": med, "ms_min": lo,
                                      "ms_max": hi, "bytes": moved, "TBps": moved / med / 1e9})
    for r in result["kernels"]:
        print("%-28s %-15s %8.4f ms (%.4f .. %.4f)  %6.1f MB  %.2f TB/s" % (
            r["kernel"], r["boxes"] or "-", r["ms"], r["ms_min"], r["ms_max"], r["bytes"] / 1e6, r["TBps"]), flush=True)

    # the feeders alone: batches per second with nothing consuming them but an event wait
    result["loaders"] = []
    for label, make in (("SyntheticClipLoader", lambda: SyntheticClipLoader(B, n_frames=T, size=S, device=dev)),
                        ("SyntheticFrameLoader", lambda: augment.SyntheticFrameLoader(B, n_frames=T, frame_hw=hw, size=S, device=dev))):
        loader = make()
        for _ in range(4):
            next(loader)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.loader_batches):
            next(loader)
        b.record()
        b.synchronize()
        rate = args.loader_batches * B / (a.elapsed_time(b) / 1e3)
        result["loaders"].append({"loader": label, "clips_per_s": rate})
        print("%-28s %10.0f clips/s" % (label, rate), flush=True)
        del loader
    # the ragged entry beside the uniform one, and the real-data feeders beside the synthetic one
    lines = ["%s, %d clips x %d frames -> %d, %d launches per window, median of 5 windows per run, 3 runs" % (
        result["device"], B, T, S, args.iters)]
    result["ragged"] = []
    for label, runs in ragged_legs(dev, frames, mixes["multiscale_mix"], S, args.iters, gen):
        result["ragged"].append({"leg": label, "ms_runs": runs})
        lines.append("%-50s %.4f .. %.4f ms   (%s)" % (label, min(runs), max(runs), ", ".join("%.4f" % r for r in runs)))
    for label, rate in feeder_rates(dev, B, T, S, args.loader_batches, args.workers, gen):
        result["loaders"].append({"loader": label, "clips_per_s": rate})
    for r in result["loaders"]:
        lines.append("%-50s %10.0f clips/s" % (r["loader"], r["clips_per_s"]))
    print("\n".join(lines), flush=True)
    if args.ragged_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.ragged_out)), exist_ok=True)
        with open(args.ragged_out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
