#!/usr/bin/env python
"""Times the device JPEG decode (rk_jpeg_decode_u8) and FrameLoader(decode="device") beside the host-decoding FrameLoader.

    python tools/jpeg_decode_time.py [--out profiles/jpeg_decode_time.txt] [--videos 64] [--frames 32] [--epochs 12]
                                     [--parent-dataset FILE]

A synthetic frame directory is written with Pillow under a temporary directory (256 x 340, 4:2:0, quality 90), then,
every GPU step in a child process of its own under a time limit, three alternating runs each:
  1. clips/s of FrameLoader with Pillow decoding in the workers and of decode="device", at 8 and at 16 workers, on the
     same files, 32 clips x 8 frames a batch; 2. the bytes the workers hand over per batch on both paths;
  3. the decode launch alone on 256 frames (events around back-to-back launches, median of 5 windows) and the ragged
     launch behind it;  4. a RubiksNet-Tiny training step fed by each path.
--parent-dataset: a copy of the previous commit's rubiksnet_amd/dataset.py to take the host path from (the host path of
this tree is that code behind one `if`).  The workers never open the GPU: at most one process does at a time.
--chunked: only FrameLoader(decode="device") with entropy="rows" beside entropy="chain", at 8 and at 16 workers, three
alternating runs; the lines are appended to --out (default profiles/jpeg_chunked_time.txt, behind what
tools/jpeg_cache_time.py --chunked wrote)."""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_frames(root, videos, frames):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:256, 0:340].astype(np.float64)
    total = 0
    with open(os.path.join(root, "list.txt"), "w") as lst:
        for v in range(videos):
            os.makedirs(os.path.join(root, "v%03d" % v))
            a, b, c = rng.uniform(0.02, 0.2, 3)
            img = np.stack([128 + 90 * np.sin(a * x) * np.cos(b * y), 128 + 80 * np.cos(c * (x - y)), 60 + 0.5 * x + 0.2 * y],
                           axis=-1) + rng.uniform(-25, 25, (256, 340, 3))
            img = np.clip(img, 0, 255).astype(np.uint8)
            for f in range(frames):                         # the picture drifts to the right, 3 pixels a frame
                path = os.path.join(root, "v%03d" % v, "img_%05d.jpg" % (f + 1))
                Image.fromarray(np.roll(img, 3 * f, axis=1)).save(path, "JPEG", quality=90, subsampling=2)
                total += os.path.getsize(path)
            lst.write("v%03d %d %d\n" % (v, frames, v % 10))
    return total / (videos * frames)


def _dataset_module(parent):
    if not parent:
        from rubiksnet_amd import dataset
        return dataset
    spec = importlib.util.spec_from_file_location("rubiksnet_amd.dataset_parent", parent)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def _loader(root, decode, workers, parent=None, entropy="chain"):
    import torch
    mod = _dataset_module(parent if decode == "host" else None)
    kw = {} if decode == "host" else {"decode": "device"}
    ds = mod.RubiksDataset(root, os.path.join(root, "list.txt"), num_segments=8, random_shift=True, **kw)
    if entropy != "chain":
        kw = dict(kw, entropy=entropy)
    return mod.FrameLoader(ds, 32, "train", dtype=torch.float32, size=224, num_workers=workers, seed=1, **kw)


def child_loader(a):
    import torch
    loader = _loader(a.root, a.decode, a.workers, a.parent_dataset, a.entropy)
    handed, clips = [], 0
    for _ in loader:                                        # warm-up epoch: workers start, arenas grow
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.epochs):
        for out, _ in loader:
            clips += out.shape[0]
            t = loader.tables
            handed.append(t["arena"].numel() if "arena" in t else
                          t["packed"].blob.numel() + sum(f.numel() for _, f in t["packed"].fallback))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    extra = {} if a.decode == "host" else {"fallback_frames": loader.fallback_frames, "decode_errors": loader.decode_errors()}
    if a.entropy == "rows":
        extra["chain_frames"] = loader.chain_frames()
    print(json.dumps(dict(clips_per_s=clips / dt, bytes_per_batch=statistics.mean(handed), **extra)))


def child_kernel(a):
    import torch
    from rubiksnet_amd import augment, dataset, jpeg
    ds = dataset.RubiksDataset(a.root, os.path.join(a.root, "list.txt"), num_segments=8, random_shift=False, decode="device")
    packed = jpeg.pack_jpeg_clips([ds[i] for i in range(32)])
    (frames, htabs, qtabs, streams), (n, nh, nq) = jpeg.sections(packed.blob.cuda(), packed.layout)
    rgb = torch.empty(packed.rgb_bytes, dtype=torch.uint8, device="cuda")
    ws = torch.empty(packed.workspace_bytes, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    clips = packed.clips.cuda()
    frame_idx = torch.arange(8, dtype=torch.int32).repeat(32, 1).cuda()
    boxes = augment.multiscale_crop_boxes(32, (256, 340), (224, 224), generator=torch.Generator().manual_seed(0)).cuda()
    out = torch.empty(32, 8, 3, 224, 224, device="cuda")

    def window(fn, iters=20):
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

    dec = window(lambda: jpeg.launch_decode(streams, frames, qtabs, htabs, n, rgb, ws, status, nq, nh))
    rag = window(lambda: augment.ragged_u8_to_clips(rgb, clips, frame_idx, boxes, (224, 224), out=out))
    assert status.tolist() == [0] * (n + 1)
    print(json.dumps(dict(frames=n, decode_ms=dec, us_per_frame=1000 * dec / n, compressed_MB_per_s=streams.numel() / dec / 1000,
                          compressed_bytes=streams.numel(), ragged_ms=rag)))


def child_train(a):
    import torch
    from rubiksnet_amd import RubiksNet
    loader = _loader(a.root, a.decode, a.workers, a.parent_dataset)
    net = RubiksNet("tiny", num_classes=10, num_frames=8, verbose=False).cuda()
    opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)

    def epoch():
        seen = 0
        for clips, labels in loader:
            loss = torch.nn.functional.cross_entropy(net(clips), labels)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            seen += clips.shape[0]
        return seen

    epoch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seen = sum(epoch() for _ in range(a.epochs))
    torch.cuda.synchronize()
    print(json.dumps(dict(clips_per_s=seen / (time.perf_counter() - t0))))


def run_child(a, what, limit, **kw):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", what, "--root", a.root,
           "--epochs", str(a.epochs)]
    if a.parent_dataset:
        cmd += ["--parent-dataset", a.parent_dataset]
    for k, v in kw.items():
        cmd += ["--" + k, str(v)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        raise SystemExit("step %s %r ended with status %d; stopping\n%s" % (what, kw, done.returncode, done.stderr[-2000:]))
    return json.loads(done.stdout.strip().splitlines()[-1])


def span(values, fmt="%.0f"):
    return (fmt + " .. " + fmt) % (min(values), max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chunked", action="store_true")
    ap.add_argument("--entropy", default="chain")
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=12)
    ap.add_argument("--parent-dataset", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--decode", default="host")
    ap.add_argument("--workers", type=int, default=8)
    a = ap.parse_args()
    if a.child:
        return {"loader": child_loader, "kernel": child_kernel, "train": child_train}[a.child](a)
    a.out = a.out or os.path.join(ROOT, "profiles", "jpeg_chunked_time.txt" if a.chunked else "jpeg_decode_time.txt")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as root:
        a.root = root
        mean_file = write_frames(root, a.videos, a.frames)
        say("%d videos x %d frames, 256 x 340, 4:2:0, quality 90: %.1f KB a file (decoded: 261.1 KB)"
            % (a.videos, a.frames, mean_file / 1000))
        for workers in (8, 16) if a.chunked else ():
            runs = {"chain": [], "rows": []}
            for _ in range(3):
                for entropy in runs:
                    runs[entropy].append(run_child(a, "loader", 300, decode="device", workers=workers, entropy=entropy))
            for entropy, r in runs.items():
                say("loader  workers=%-2d decode=device entropy=%-5s clips/s %s   decode_errors %d%s"
                    % (workers, entropy, span([x["clips_per_s"] for x in r]), r[0]["decode_errors"],
                       "" if entropy == "chain" else "   frames left to the sequential walk %d" % r[0]["chain_frames"]))
        if a.chunked:
            with open(a.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")
            return
        say("host path: %s" % ("the previous commit's dataset.py" if a.parent_dataset else "this tree's decode='host'"))
        for workers in (8, 16):
            runs = {"host": [], "device": []}
            for _ in range(3):
                for decode in ("host", "device"):
                    runs[decode].append(run_child(a, "loader", 300, decode=decode, workers=workers))
            for decode in ("host", "device"):
                r = runs[decode]
                say("loader  workers=%-2d decode=%-6s clips/s %s   bytes handed over per batch %.2f MB%s"
                    % (workers, decode, span([x["clips_per_s"] for x in r]), r[0]["bytes_per_batch"] / 1e6,
                       "" if decode == "host" else "   fallback_frames %d decode_errors %d"
                       % (r[0]["fallback_frames"], r[0]["decode_errors"])))
        k = [run_child(a, "kernel", 120) for _ in range(3)]
        say("decode launch alone, %d frames (%.2f MB compressed): %s ms, %s us a frame, %s MB/s of compressed data"
            % (k[0]["frames"], k[0]["compressed_bytes"] / 1e6, span([x["decode_ms"] for x in k], "%.3f"),
               span([x["us_per_frame"] for x in k], "%.2f"), span([x["compressed_MB_per_s"] for x in k])))
        say("ragged launch behind it (32 clips x 8 frames -> 224 x 224 f32): %s ms" % span([x["ragged_ms"] for x in k], "%.3f"))
        runs = {"host": [], "device": []}
        for _ in range(3):
            for decode in ("host", "device"):
                runs[decode].append(run_child(a, "train", 300, decode=decode, workers=8))
        for decode in ("host", "device"):
            say("Tiny fp32 training step, batch 32, workers=8, fed by decode=%-6s: clips/s %s"
                % (decode, span([x["clips_per_s"] for x in runs[decode]])))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
