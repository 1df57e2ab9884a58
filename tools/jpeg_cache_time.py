#!/usr/bin/env python
"""Times the resident JPEG cache: the index build, the indexed decode launch beside the sequential one on the same
frames, and DeviceFrameCache with resident="jpeg" beside resident="rgb".

    python tools/jpeg_cache_time.py [--out profiles/jpeg_cache_time.txt] [--videos 64] [--frames 32] [--epochs 100]

The workload is tools/jpeg_decode_time.py's: a synthetic frame directory written with Pillow under a temporary directory
(256 x 340, 4:2:0, quality 90), batches of 32 clips x 8 frames.  Every variant runs in a child process of its own under a
time limit, three alternating runs each:
  1. the decode launch alone for the same 256 frames through rk_jpeg_decode_u8 (one chain per frame) and through
     rk_jpeg_decode_indexed_u8 at one segment per MCU row, and at 2 and 4 rows per segment (what the launch does when the
     chains get longer and fewer says what bounds it); events around back-to-back launches, median of 5 windows; the
     indexed child also times rk_jpeg_build_index over the whole set (its second call), and the decoders' bytes are compared;
  2. clips/s of DeviceFrameCache(resident="rgb") and (resident="jpeg") over whole epochs, and the bytes each keeps in HBM.
With --chunked only the comparisons of the chunked index build (rk_jpeg_build_index_chunked) run, again three alternating
runs, every figure beside the sequential path's re-measured in the same run (default --out profiles/jpeg_chunked_time.txt):
  3. the build launches alone on device-resident data, for the first 256 frames and for all of them: rk_jpeg_build_index
     and the chunked build at 64, 128 and 256 bytes a chunk; the share of frames the chunked build left to the sequential
     walk and the histogram of the rounds the others took;
  4. one batch of 256 frames: chunked build + indexed decode (jpeg.launch_decode_rows) beside rk_jpeg_decode_u8;
  5. the start-up of DeviceFrameCache(resident="jpeg") with either build.
At most one process has the GPU open at a time."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from jpeg_decode_time import span, write_frames  # noqa: E402

BATCH, SEGMENTS = 32, 8


def _window(fn, iters=20):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / iters)
    return statistics.median(times)


def _dataset(root, split="val"):
    from rubiksnet_amd import dataset
    return dataset.RubiksDataset(root, os.path.join(root, "list.txt"), num_segments=SEGMENTS, random_shift=split == "train",
                                 decode="device")


def child_plain(a):
    """The sequential launch on the frames of the first 32 videos' samples: the previous commit's code path."""
    import torch
    from rubiksnet_amd import jpeg
    ds = _dataset(a.root)
    packed = jpeg.pack_jpeg_clips([ds[i] for i in range(BATCH)])
    (frames, htabs, qtabs, streams), (n, nh, nq) = jpeg.sections(packed.blob.cuda(), packed.layout)
    rgb = torch.empty(packed.rgb_bytes, dtype=torch.uint8, device="cuda")
    ws = torch.empty(packed.workspace_bytes, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    ms = _window(lambda: jpeg.launch_decode(streams, frames, qtabs, htabs, n, rgb, ws, status, nq, nh))
    assert status.tolist() == [0] * (n + 1)
    print(json.dumps(dict(frames=n, decode_ms=ms, digest=int(rgb.to(torch.int64).sum().item()))))


def child_indexed(a):
    """The whole set resident, its index built (timed, once), then the same 256 frames through the indexed launch."""
    import numpy as np
    import torch
    from rubiksnet_amd import jpeg
    ds = _dataset(a.root)
    mcux = (340 + 15) // 16
    res = jpeg.pack_resident([ds.whole_bytes(i) for i in range(len(ds))], seg_mcus=a.rows * mcux)
    assert not res.fallback
    jpeg.build_index(res, "cuda")                           # first use: the code object loads, the allocator grows
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    index = jpeg.build_index(res, "cuda")
    e1.record()
    e1.synchronize()
    build_ms = e0.elapsed_time(e1)                          # the upload of the blob and the tables, and the walk
    assert index.status.tolist() == [0] * (index.n + 1)
    ids = list(range(BATCH))
    numbers = [[p - 1 for p in ds.frame_numbers(ds.num_frames_of(i))] for i in ids]
    t = jpeg.pick_tables(res, ids, numbers)
    (frames, _, _, _), _ = jpeg.sections(res.blob, res.layout)
    rec = np.frombuffer(frames.numpy().tobytes(), dtype=jpeg.FRAME_DTYPE)
    rgb = torch.empty(t.rgb_bytes, dtype=torch.uint8, device="cuda")
    ws = torch.empty(jpeg.indexed_workspace_bytes_for(rec, t.pick.numpy(), t.max_segments), dtype=torch.uint8, device="cuda")
    m = t.pick.numel()
    status = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    pick, rgb_off = t.pick.cuda(), t.rgb_off.cuda()
    ms = _window(lambda: jpeg.launch_decode_indexed(index, pick, rgb_off, t.max_segments, rgb, ws, status))
    assert status.tolist() == [0] * (m + 1)
    print(json.dumps(dict(frames=m, segments=t.max_segments, decode_ms=ms, build_ms=build_ms, resident_frames=index.n,
                          digest=int(rgb.to(torch.int64).sum().item()))))


def child_cache(a):
    import torch
    from rubiksnet_amd import dataset
    ds = dataset.RubiksDataset(a.root, os.path.join(a.root, "list.txt"), num_segments=SEGMENTS, random_shift=True,
                               decode="device" if a.resident == "jpeg" else "host")
    cache = dataset.DeviceFrameCache(ds, BATCH, "train", dtype=torch.float32, size=224, seed=1, resident=a.resident)
    for _ in cache:                                         # warm-up epoch: the batch buffers grow
        pass
    torch.cuda.synchronize()
    clips, t0 = 0, time.perf_counter()
    for _ in range(a.epochs):
        for out, _ in cache:
            clips += out.shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    fixed = cache._fixed_bytes if a.resident == "jpeg" else cache.resident_bytes
    print(json.dumps(dict(clips_per_s=clips / dt, resident_bytes=cache.resident_bytes, set_bytes=fixed, seconds=dt,
                          fallback_frames=cache.fallback_frames, decode_errors=cache.decode_errors())))


def child_build(a):
    """The build launches alone: the set resident on the device, the first 256 frames and all of them, either build."""
    import collections

    import numpy as np
    import torch
    from rubiksnet_amd import _native, jpeg
    ds = _dataset(a.root)
    res = jpeg.pack_resident([ds.whole_bytes(i) for i in range(len(ds))])
    assert not res.fallback
    index = jpeg.build_index(res, "cuda")
    (frames, _, _, _), _ = jpeg.sections(res.blob, res.layout)
    rec = np.frombuffer(frames.numpy().tobytes(), dtype=jpeg.FRAME_DTYPE)
    want = index.entries.clone()
    out = {"resident_frames": index.n}
    for k in sorted({min(256, index.n), index.n}):
        status = torch.zeros(k + 1, dtype=torch.int32, device="cuda")
        route = torch.zeros(k, dtype=torch.int32, device="cuda")
        out["chain_ms_%d" % k] = _window(lambda: _native.launch(
            "rk_jpeg_build_index", index.streams.device, index.streams.data_ptr(), index.streams.numel(), index.frames.data_ptr(),
            index.htabs.data_ptr(), index.nq, index.nh, k, index.seg_mcus.data_ptr(), index.entry_off.data_ptr(),
            index.entries.data_ptr(), index.n_entries, status.data_ptr()), iters=5)
        assert status.tolist() == [0] * (k + 1)
        for chunk_bytes in (64, 128, 256):
            ws = torch.empty(jpeg.chunked_workspace_bytes_for(rec[:k], chunk_bytes), dtype=torch.uint8, device="cuda")
            index.entries.zero_()
            out["chunked_ms_%d_%d" % (k, chunk_bytes)] = _window(lambda: jpeg.launch_build_index_chunked(
                index.streams, index.frames, index.htabs, index.nq, index.nh, k, index.seg_mcus, index.entry_off, index.entries,
                index.n_entries, chunk_bytes, a.max_rounds, ws, status, route), iters=5)
            last = int(index.entry_off[k])
            assert status.tolist() == [0] * (k + 1) and torch.equal(index.entries[:last * 16], want[:last * 16])
            hist = collections.Counter(route.tolist())
            out["rounds_%d_%d" % (k, chunk_bytes)] = {str(r): c for r, c in sorted(hist.items())}
    print(json.dumps(out))


def child_batch(a):
    """One batch of 256 frames: rk_jpeg_decode_u8, and the chunked build + the indexed decode of the same records."""
    import numpy as np
    import torch
    from rubiksnet_amd import jpeg
    ds = _dataset(a.root)
    packed = jpeg.pack_jpeg_clips([ds[i] for i in range(BATCH)])
    (frames, htabs, qtabs, streams), (n, nh, nq) = jpeg.sections(packed.blob.cuda(), packed.layout)
    rgb = torch.empty(packed.rgb_bytes, dtype=torch.uint8, device="cuda")
    ws = torch.empty(packed.workspace_bytes, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    out = {"frames": n}
    out["chain_ms"] = _window(lambda: jpeg.launch_decode(streams, frames, qtabs, htabs, n, rgb, ws, status, nq, nh))
    assert status.tolist() == [0] * (n + 1)
    want = rgb.clone()
    (host_frames, _, _, _), _ = jpeg.sections(packed.blob, packed.layout)
    for chunk_bytes in (64, 128, 256):
        rows = jpeg.row_tables(np.frombuffer(host_frames.numpy().tobytes(), dtype=jpeg.FRAME_DTYPE), chunk_bytes)
        tables = rows.tables.cuda()
        entries = torch.zeros(rows.n_entries * 2, dtype=torch.int64, device="cuda").view(torch.uint8)
        build_ws = torch.empty(rows.build_bytes, dtype=torch.uint8, device="cuda")
        decode_ws = torch.empty(rows.decode_bytes, dtype=torch.uint8, device="cuda")
        build_status = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        route = torch.zeros(n, dtype=torch.int32, device="cuda")
        rgb.zero_()
        out["rows_ms_%d" % chunk_bytes] = _window(lambda: jpeg.launch_decode_rows(
            streams, frames, qtabs, htabs, nq, nh, rows, tables, entries, build_ws, build_status, route, rgb, decode_ws, status,
            chunk_bytes, a.max_rounds))
        assert status.tolist() == [0] * (n + 1) and torch.equal(rgb, want)
        out["chain_frames_%d" % chunk_bytes] = int((route == 0).sum())
    print(json.dumps(out))


def child_startup(a):
    """DeviceFrameCache(resident="jpeg") from nothing to its first batch, with either index build."""
    import torch
    from rubiksnet_amd import dataset
    ds = dataset.RubiksDataset(a.root, os.path.join(a.root, "list.txt"), num_segments=SEGMENTS, random_shift=True, decode="device")
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cache = dataset.DeviceFrameCache(ds, BATCH, "train", dtype=torch.float32, size=224, seed=1, resident="jpeg",
                                     index_build=a.index_build)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    next(iter(cache))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(json.dumps(dict(construct_s=t1 - t0, first_batch_s=t2 - t1, build_errors=int(cache.index.status[-1]))))


def run_child(a, what, limit, **kw):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", what, "--root", a.root,
           "--epochs", str(a.epochs), "--max-rounds", str(a.max_rounds)]
    for k, v in kw.items():
        cmd += ["--" + k, str(v)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        raise SystemExit("step %s %r ended with status %d; stopping\n%s" % (what, kw, done.returncode, done.stderr[-2000:]))
    return json.loads(done.stdout.strip().splitlines()[-1])


def chunked_report(a, say):
    """Steps 3 to 5 of the module's text."""
    build, batch, start = [], [], {"chain": [], "chunked": []}
    for _ in range(3):
        build.append(run_child(a, "build", 300))
        batch.append(run_child(a, "batch", 300))
        for index_build in start:
            start[index_build].append(run_child(a, "startup", 300, **{"index-build": index_build}))
    n = build[0]["resident_frames"]
    say("max_rounds %d; every figure is the span of three alternating runs" % a.max_rounds)
    for k in sorted({min(256, n), n}):
        say("index build launches alone, %d frames, rk_jpeg_build_index (one chain per frame): %s ms"
            % (k, span([x["chain_ms_%d" % k] for x in build], "%.3f")))
        for chunk_bytes in (64, 128, 256):
            rounds = build[0]["rounds_%d_%d" % (k, chunk_bytes)]
            say("index build launches alone, %d frames, rk_jpeg_build_index_chunked at %d bytes a chunk: %s ms   frames left to the "
                "sequential walk %d of %d   rounds: frames %s"
                % (k, chunk_bytes, span([x["chunked_ms_%d_%d" % (k, chunk_bytes)] for x in build], "%.3f"),
                   rounds.get("0", 0), k, ", ".join("%s: %d" % rc for rc in rounds.items() if rc[0] != "0")))
    say("one batch, %d frames, rk_jpeg_decode_u8 (one chain per frame): %s ms"
        % (batch[0]["frames"], span([x["chain_ms"] for x in batch], "%.3f")))
    for chunk_bytes in (64, 128, 256):
        say("one batch, %d frames, chunked build at %d bytes a chunk + rk_jpeg_decode_indexed_u8 by MCU row, the same bytes out: %s ms"
            "   frames left to the sequential walk %d"
            % (batch[0]["frames"], chunk_bytes, span([x["rows_ms_%d" % chunk_bytes] for x in batch], "%.3f"),
               batch[0]["chain_frames_%d" % chunk_bytes]))
    for index_build, r in start.items():
        say("DeviceFrameCache(resident='jpeg', index_build=%-9r) of %d frames: constructed in %s s (files read and parsed on the "
            "host, upload, build), first batch after %s s more   build errors %d"
            % (index_build, n, span([x["construct_s"] for x in r], "%.2f"), span([x["first_batch_s"] for x in r], "%.3f"),
               r[0]["build_errors"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chunked", action="store_true")
    ap.add_argument("--max-rounds", type=int, default=32)
    ap.add_argument("--index-build", default="chain")
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--resident", default="rgb")
    ap.add_argument("--rows", type=int, default=1)
    a = ap.parse_args()
    if a.child:
        return {"plain": child_plain, "indexed": child_indexed, "cache": child_cache, "build": child_build, "batch": child_batch,
                "startup": child_startup}[a.child](a)
    a.out = a.out or os.path.join(ROOT, "profiles", "jpeg_chunked_time.txt" if a.chunked else "jpeg_cache_time.txt")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as root:
        a.root = root
        mean_file = write_frames(root, a.videos, a.frames)
        say("%d videos x %d frames, 256 x 340, 4:2:0, quality 90: %.1f KB a file (decoded: 261.1 KB)"
            % (a.videos, a.frames, mean_file / 1000))
        if a.chunked:
            chunked_report(a, say)
        else:
            plain, indexed = [], {1: [], 2: [], 4: []}
            for _ in range(3):
                plain.append(run_child(a, "plain", 300))
                for rows in indexed:
                    indexed[rows].append(run_child(a, "indexed", 300, rows=rows))
            digests = {x["digest"] for x in plain} | {x["digest"] for r in indexed.values() for x in r}
            say("decode launch alone, %d frames, rk_jpeg_decode_u8 (one chain per frame): %s ms"
                % (plain[0]["frames"], span([x["decode_ms"] for x in plain], "%.3f")))
            for rows, r in indexed.items():
                say("decode launch alone, %d frames, rk_jpeg_decode_indexed_u8, %d MCU row(s) per segment (%d chains per frame): %s ms"
                    % (r[0]["frames"], rows, r[0]["segments"], span([x["decode_ms"] for x in r], "%.3f")))
            say("both decoders' output bytes sum to the same number: %s" % (len(digests) == 1))
            say("rk_jpeg_build_index over %d resident frames (second call; the blob's upload included): %s ms"
                % (indexed[1][0]["resident_frames"], span([x["build_ms"] for r in indexed.values() for x in r], "%.1f")))
            runs = {"rgb": [], "jpeg": []}
            for _ in range(3):
                for resident in runs:
                    runs[resident].append(run_child(a, "cache", 600, resident=resident))
            for resident, r in runs.items():
                say("DeviceFrameCache resident=%-4s batch %d x %d frames -> 224 x 224 f32: clips/s %s   resident %.1f MB, of which the "
                    "set %.1f MB and one batch's buffers %.1f MB (timed %.1f s)   fallback_frames %d decode_errors %d"
                    % (resident, BATCH, SEGMENTS, span([x["clips_per_s"] for x in r]), r[0]["resident_bytes"] / 1e6,
                       r[0]["set_bytes"] / 1e6, (r[0]["resident_bytes"] - r[0]["set_bytes"]) / 1e6, r[0]["seconds"],
                       r[0]["fallback_frames"], r[0]["decode_errors"]))
            say("resident bytes, rgb over jpeg: the set %.2f, all %.2f" % (runs["rgb"][0]["set_bytes"] / runs["jpeg"][0]["set_bytes"],
                                                                         runs["rgb"][0]["resident_bytes"] / runs["jpeg"][0]["resident_bytes"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
