#!/usr/bin/env python
"""Times the dense records of the resident coefficient cache beside the wide ones: the per-batch launch of both on the
same picks, DeviceFrameCache with resident="rgb", "jpeg", "coef" (wide) and "coef" with coef_record="dense", and
jpeg.build_coef in both formats.

    python tools/jpeg_dense_time.py [--out profiles/jpeg_coef_dense_time.txt] [--videos 64] [--frames 32] [--epochs 100]

The workload is tools/jpeg_cache_time.py's: a synthetic frame directory written with Pillow under a temporary directory
(256 x 340, 4:2:0, quality 90), batches of 32 clips x 8 frames.  Every step runs in a child process of its own under a
time limit, the steps are chained (a step that fails ends the run), three alternating runs each:
  1. the decode launch alone for 256 picked frames: rk_jpeg_decode_coef_as_u8 on the wide and on the dense blob, in the
     same process on the same picks, alternated; events around back-to-back launches, median of 5 windows; the two arenas
     are compared byte for byte; the child also times jpeg.build_coef over the whole set in both formats (second calls);
  2. clips/s of DeviceFrameCache for the four caches over whole epochs, the bytes each keeps in HBM and the seconds its
     construction took;
  3. the packed bytes per frame of both formats beside the file's entropy-coded bytes per frame, and bytes per 8x8 block.
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

CACHES = (("rgb", "wide"), ("jpeg", "wide"), ("coef", "wide"), ("coef", "dense"))


def child_launch(a):
    """The whole set packed both ways, then the same 256 picks through the launch on either blob."""
    import torch
    from rubiksnet_amd import jpeg
    ds = _dataset(a.root)
    res = jpeg.pack_resident([ds.whole_bytes(i) for i in range(len(ds))])
    assert not res.fallback
    coefs, build_s = {}, {}
    for record in ("wide", "dense"):
        jpeg.build_coef(res, "cuda", record=record)         # first use: the code object loads, the allocator grows
    for record in ("wide", "dense"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        coefs[record] = jpeg.build_coef(res, "cuda", record=record)
        torch.cuda.synchronize()
        build_s[record] = time.perf_counter() - t0          # the uploads, the entropy stage, the measuring, the packing
        assert coefs[record].status.tolist() == [0] * (coefs[record].n + 1)
    ids = list(range(BATCH))
    numbers = [[p - 1 for p in ds.frame_numbers(ds.num_frames_of(i))] for i in ids]
    t = jpeg.pick_tables(res, ids, numbers)
    rec = jpeg.records(res.blob, res.layout).copy()
    m = t.pick.numel()
    pick, rgb_off = t.pick.cuda(), t.rgb_off.cuda()
    status = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    rgb = {record: torch.empty(t.rgb_bytes, dtype=torch.uint8, device="cuda") for record in coefs}
    ws = torch.empty(jpeg.coef_workspace_bytes_for(rec, t.pick.numpy()), dtype=torch.uint8, device="cuda")
    out = dict(frames=m, resident_frames=coefs["wide"].n, file_bytes=coefs["wide"].file_bytes,
               blocks=int(jpeg._geometry_blocks(rec)[3].sum()), workspace=ws.numel())
    for record in coefs:
        out["build_s_" + record], out["packed_" + record] = build_s[record], coefs[record].packed_bytes
    for k in range(2):                                      # both launches twice, alternating, in one process
        for record in ("wide", "dense"):
            out["%s_ms_%d" % (record, k)] = _window(
                lambda: jpeg.launch_decode_coef(coefs[record], pick, rgb_off, rgb[record], ws, status))
            assert status.tolist() == [0] * (m + 1)
    out["equal"] = bool(torch.equal(rgb["wide"], rgb["dense"]))
    print(json.dumps(out))


def child_cache(a):
    import torch
    from rubiksnet_amd import dataset
    ds = dataset.RubiksDataset(a.root, os.path.join(a.root, "list.txt"), num_segments=SEGMENTS, random_shift=True,
                               decode="host" if a.resident == "rgb" else "device")
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cache = dataset.DeviceFrameCache(ds, BATCH, "train", dtype=torch.float32, size=224, seed=1, resident=a.resident,
                                     coef_record=a.record)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_coef_dense_time.txt"))
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--resident", default="rgb")
    ap.add_argument("--record", default="wide")
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
        launch, runs = [], {c: [] for c in CACHES}
        for _ in range(3):
            launch.append(run_child(a, "launch", 300))
            for resident, record in CACHES:
                runs[resident, record].append(run_child(a, "cache", 600, resident=resident, record=record))
        x = launch[0]
        wide = [r["wide_ms_%d" % k] for r in launch for k in range(2)]
        dense = [r["dense_ms_%d" % k] for r in launch for k in range(2)]
        say("")
        say("1. the decode launch alone, %d picked frames (two windows of each per run, alternating in one process), workspace "
            "%.1f MB for either" % (x["frames"], x["workspace"] / 1e6))
        say("   rk_jpeg_decode_coef_as_u8, wide records:   %s ms" % span(wide, "%.3f"))
        say("   rk_jpeg_decode_coef_as_u8, dense records:  %s ms" % span(dense, "%.3f"))
        say("   dense over wide, slowest over fastest and fastest over slowest: %.3f .. %.3f   the ranges overlap: %s"
            % (min(dense) / max(wide), max(dense) / min(wide), not (min(dense) > max(wide) or max(dense) < min(wide))))
        say("   the two arenas are equal byte for byte: %s" % all(r["equal"] for r in launch))
        for record in ("wide", "dense"):
            say("   jpeg.build_coef(record=%r) over %d frames (second call; uploads, entropy stage, measuring, packing): %s s"
                % (record, x["resident_frames"], span([r["build_s_" + record] for r in launch], "%.2f")))
        say("")
        say("2. DeviceFrameCache, batch %d x %d frames -> 224 x 224 f32" % (BATCH, SEGMENTS))
        for (resident, record), r in runs.items():
            say("   resident=%-4s %-5s clips/s %s   resident %.1f MB, of which the set %.1f MB and one batch's buffers %.1f MB   "
                "constructed in %s s (the build's peak %.1f MB)   (timed %.1f s)   fallback_frames %d decode_errors %d"
                % (resident, record if resident == "coef" else "", span([v["clips_per_s"] for v in r]), r[0]["resident_bytes"] / 1e6,
                   r[0]["set_bytes"] / 1e6, (r[0]["resident_bytes"] - r[0]["set_bytes"]) / 1e6,
                   span([v["construct_s"] for v in r], "%.2f"), r[0]["build_peak_bytes"] / 1e6, r[0]["seconds"],
                   r[0]["fallback_frames"], r[0]["decode_errors"]))
        rate = {c: [v["clips_per_s"] for v in r] for c, r in runs.items()}
        say("   the dense cache's range lies wholly above resident=jpeg's: %s   wholly below the wide cache's: %s"
            % (min(rate["coef", "dense"]) > max(rate["jpeg", "wide"]), max(rate["coef", "dense"]) < min(rate["coef", "wide"])))
        say("")
        say("3. the footprint, on this content only (quality 90, smooth synthetic pictures; denser or noisier frames pack worse)")
        n = x["resident_frames"]
        for record in ("wide", "dense"):
            packed = x["packed_" + record]
            say("   %-5s %.1f KB a frame (%.1f bytes a block, table included) against %.1f KB of entropy-coded bytes a frame: %.2f x; "
                "decoded RGB over packed: %.2f x" % (record, packed / n / 1000, packed / x["blocks"], x["file_bytes"] / n / 1000,
                                                     packed / x["file_bytes"], 256 * 340 * 3 * n / packed))
        say("   dense over wide: %.3f" % (x["packed_dense"] / x["packed_wide"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
