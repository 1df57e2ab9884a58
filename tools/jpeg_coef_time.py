#!/usr/bin/env python
"""Times the resident cache of packed DCT coefficients: the per-batch launch beside the indexed decode's on the same
picks, DeviceFrameCache with resident="coef" beside "rgb" and "jpeg", and the packed bytes beside the files'.

    python tools/jpeg_coef_time.py [--out profiles/jpeg_coef_time.txt] [--videos 64] [--frames 32] [--epochs 100]

The workload is tools/jpeg_cache_time.py's: a synthetic frame directory written with Pillow under a temporary directory
(256 x 340, 4:2:0, quality 90), batches of 32 clips x 8 frames.  Every step runs in a child process of its own under a
time limit, the steps are chained (a step that fails ends the run), three alternating runs each:
  1. the decode launch alone for 256 picked frames: rk_jpeg_decode_coef_u8 and, in the same process on the same picks,
     rk_jpeg_decode_indexed_u8 at one segment per MCU row; events around back-to-back launches, median of 5 windows; the
     two arenas are compared byte for byte; the child also times jpeg.build_coef over the whole set (its second call);
  2. clips/s of DeviceFrameCache(resident="rgb"), ("jpeg") and ("coef") over whole epochs, the bytes each keeps in HBM
     and the seconds its construction took;
  3. the packed bytes per frame beside the file's entropy-coded bytes per frame, and bytes per 8x8 block.
At most one process has the GPU open at a time."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from jpeg_cache_time import BATCH, SEGMENTS, _dataset, _window  # noqa: E402
from jpeg_decode_time import span, write_frames  # noqa: E402


def child_launch(a):
    """The whole set resident both ways, then the same 256 picks through both launches."""
    import numpy as np
    import torch
    from rubiksnet_amd import jpeg
    ds = _dataset(a.root)
    res = jpeg.pack_resident([ds.whole_bytes(i) for i in range(len(ds))])
    assert not res.fallback
    index = jpeg.build_index(res, "cuda")
    jpeg.build_coef(res, "cuda")                            # first use: the code object loads, the allocator grows
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    coef = jpeg.build_coef(res, "cuda")
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0                      # the uploads, the entropy stage, the measuring, the packing
    assert index.status.tolist() == [0] * (index.n + 1) and coef.status.tolist() == [0] * (coef.n + 1)
    ids = list(range(BATCH))
    numbers = [[p - 1 for p in ds.frame_numbers(ds.num_frames_of(i))] for i in ids]
    t = jpeg.pick_tables(res, ids, numbers)
    rec = jpeg.records(res.blob, res.layout).copy()
    m = t.pick.numel()
    pick, rgb_off = t.pick.cuda(), t.rgb_off.cuda()
    status = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    rgb_i = torch.empty(t.rgb_bytes, dtype=torch.uint8, device="cuda")
    ws_i = torch.empty(jpeg.indexed_workspace_bytes_for(rec, t.pick.numpy(), t.max_segments), dtype=torch.uint8, device="cuda")
    rgb_c = torch.empty(t.rgb_bytes, dtype=torch.uint8, device="cuda")
    ws_c = torch.empty(jpeg.coef_workspace_bytes_for(rec, t.pick.numpy()), dtype=torch.uint8, device="cuda")
    out = dict(frames=m, resident_frames=coef.n, build_s=build_s, packed_bytes=coef.packed_bytes, file_bytes=coef.file_bytes,
               blocks=int(jpeg._geometry_blocks(rec)[3].sum()), workspace_indexed=ws_i.numel(), workspace_coef=ws_c.numel())
    for k in range(2):                                      # both launches twice, alternating, in one process
        out["indexed_ms_%d" % k] = _window(lambda: jpeg.launch_decode_indexed(index, pick, rgb_off, t.max_segments, rgb_i, ws_i, status))
        assert status.tolist() == [0] * (m + 1)
        out["coef_ms_%d" % k] = _window(lambda: jpeg.launch_decode_coef(coef, pick, rgb_off, rgb_c, ws_c, status))
        assert status.tolist() == [0] * (m + 1)
    out["equal"] = bool(torch.equal(rgb_i, rgb_c))
    print(json.dumps(out))


def child_cache(a):
    import torch
    from rubiksnet_amd import dataset
    ds = dataset.RubiksDataset(a.root, os.path.join(a.root, "list.txt"), num_segments=SEGMENTS, random_shift=True,
                               decode="host" if a.resident == "rgb" else "device")
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cache = dataset.DeviceFrameCache(ds, BATCH, "train", dtype=torch.float32, size=224, seed=1, resident=a.resident)
    torch.cuda.synchronize()
    construct_s = time.perf_counter() - t0
    for _ in cache:                                         # warm-up epoch: the batch buffers grow
        pass
    torch.cuda.synchronize()
    clips, t0 = 0, time.perf_counter()
    for _ in range(a.epochs):
        for out, _ in cache:
            clips += out.shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    fixed = cache.resident_bytes if a.resident == "rgb" else cache._fixed_bytes
    print(json.dumps(dict(clips_per_s=clips / dt, resident_bytes=cache.resident_bytes, set_bytes=fixed, seconds=dt,
                          construct_s=construct_s, build_peak_bytes=getattr(cache, "build_peak_bytes", 0),
                          fallback_frames=cache.fallback_frames, decode_errors=cache.decode_errors())))


def run_child(a, what, limit, **kw):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", what, "--root", a.root,
           "--epochs", str(a.epochs)]
    for k, v in kw.items():
        cmd += ["--" + k, str(v)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        raise SystemExit("step %s %r ended with status %d; stopping\n%s" % (what, kw, done.returncode, done.stderr[-2000:]))
    print("step %s %r done" % (what, kw), file=sys.stderr, flush=True)
    return json.loads(done.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_coef_time.txt"))
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--resident", default="rgb")
    a = ap.parse_args()
    if a.child:
        return {"launch": child_launch, "cache": child_cache}[a.child](a)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as root:
        a.root = root
        mean_file = write_frames(root, a.videos, a.frames)
        say("%d videos x %d frames, 256 x 340, 4:2:0, quality 90 (smooth synthetic pictures with a little noise): %.1f KB a file "
            "(decoded: 261.1 KB)" % (a.videos, a.frames, mean_file / 1000))
        say("every figure is the span of three alternating runs, each step a process of its own")
        launch, runs = [], {"rgb": [], "jpeg": [], "coef": []}
        for _ in range(3):
            launch.append(run_child(a, "launch", 300))
            for resident in runs:
                runs[resident].append(run_child(a, "cache", 600, resident=resident))
        x = launch[0]
        indexed = [r["indexed_ms_%d" % k] for r in launch for k in range(2)]
        coef = [r["coef_ms_%d" % k] for r in launch for k in range(2)]
        say("")
        say("1. the decode launch alone, %d picked frames (two windows of each per run, alternating in one process)" % x["frames"])
        say("   rk_jpeg_decode_indexed_u8, one segment per MCU row:  %s ms   workspace %.1f MB" % (span(indexed, "%.3f"),
                                                                                                x["workspace_indexed"] / 1e6))
        say("   rk_jpeg_decode_coef_u8:                              %s ms   workspace %.1f MB" % (span(coef, "%.3f"),
                                                                                                x["workspace_coef"] / 1e6))
        say("   the coef launch's range lies wholly below the indexed decode's: %s   (slowest coef over fastest indexed: %.3f)"
            % (max(coef) < min(indexed), max(coef) / min(indexed)))
        say("   the two arenas are equal byte for byte: %s" % all(r["equal"] for r in launch))
        say("   jpeg.build_coef over %d frames (second call; uploads, entropy stage, measuring, packing): %s s"
            % (x["resident_frames"], span([r["build_s"] for r in launch], "%.2f")))
        say("")
        say("2. DeviceFrameCache, batch %d x %d frames -> 224 x 224 f32" % (BATCH, SEGMENTS))
        for resident, r in runs.items():
            say("   resident=%-4s clips/s %s   resident %.1f MB, of which the set %.1f MB and one batch's buffers %.1f MB   constructed "
                "in %s s (the build's peak %.1f MB)   (timed %.1f s)   fallback_frames %d decode_errors %d"
                % (resident, span([v["clips_per_s"] for v in r]), r[0]["resident_bytes"] / 1e6, r[0]["set_bytes"] / 1e6,
                   (r[0]["resident_bytes"] - r[0]["set_bytes"]) / 1e6, span([v["construct_s"] for v in r], "%.2f"),
                   r[0]["build_peak_bytes"] / 1e6, r[0]["seconds"], r[0]["fallback_frames"], r[0]["decode_errors"]))
        say("")
        say("3. the footprint, on this content only (quality 90, smooth synthetic pictures; denser or noisier frames pack worse)")
        n = x["resident_frames"]
        say("   packed %.1f KB a frame (%.1f bytes a block, offsets included) against %.1f KB of entropy-coded bytes a frame: %.2f x; "
            "decoded RGB over packed: %.2f x" % (x["packed_bytes"] / n / 1000, x["packed_bytes"] / x["blocks"], x["file_bytes"] / n / 1000,
                                                 x["packed_bytes"] / x["file_bytes"], 256 * 340 * 3 * n / x["packed_bytes"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
