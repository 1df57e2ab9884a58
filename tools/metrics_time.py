"""python tools/metrics_time.py [--batches 20]: evaluation.evaluate (two .item() and a copy of the logits to the host per
batch) against evaluation.evaluate_streaming (one StreamMeter launch per batch, the state read once at the end) on
RubiksNet-Tiny in eval mode: 32 videos of 3 views per batch, 174 classes, fed by SyntheticClipLoader.

Both run in this process, alternating, after a warm-up pass of each; a point is the wall time per batch of one pass over
`--batches` batches ending in a device synchronise, three passes each, printed as min..max.  Then the update launch alone
(rk_metrics.hip through StreamMeter.update, 32 x 3 x 174 logits): HIP events around 200 back-to-back calls, three runs (the
host's enqueue or the kernel, whichever is slower), and around a captured replay of the same 200 launches (the kernel)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rubiksnet_amd import RubiksNet  # noqa: E402
from rubiksnet_amd.evaluation import evaluate, evaluate_streaming  # noqa: E402
from rubiksnet_amd.input_pipeline import SyntheticClipLoader  # noqa: E402
from rubiksnet_amd.metrics import StreamMeter  # noqa: E402

DEV = torch.device("cuda:0")
VIDEOS, VIEWS, FRAMES, CLASSES, SIZE = 32, 3, 8, 174, 224


def batches(loader, n):
    for _ in range(n):
        clips, labels = next(loader)                     # [VIDEOS * VIEWS, T, 3, S, S]: a video's views are consecutive clips
        yield clips.view(VIDEOS, VIEWS * FRAMES * 3, SIZE, SIZE), labels[:VIDEOS]


def ms_per_batch(fn, net, loader, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn(net, batches(loader, n), n_frames=FRAMES, views=VIEWS)
    torch.cuda.synchronize()
    assert res["videos"] == n * VIDEOS
    return (time.perf_counter() - t0) / n * 1e3, res


def loops(n):
    torch.manual_seed(0)
    net = RubiksNet("tiny", CLASSES, num_frames=FRAMES, verbose=False).to(DEV).eval()
    loader = SyntheticClipLoader(VIDEOS * VIEWS, n_frames=FRAMES, size=SIZE, num_classes=CLASSES, device=DEV)
    print("RubiksNet-Tiny eval, fp32, %d videos x %d views per batch, %d classes; ms per batch over %d batches, "
          "min..max of 3 alternating passes" % (VIDEOS, VIEWS, CLASSES, n))
    res = {"evaluate": [], "evaluate_streaming": []}
    last = {}
    for name, fn in (("evaluate", evaluate), ("evaluate_streaming", evaluate_streaming)):
        ms_per_batch(fn, net, loader, 3)                 # warm-up
    for _ in range(3):
        for name, fn in (("evaluate", evaluate), ("evaluate_streaming", evaluate_streaming)):
            ms, last[name] = ms_per_batch(fn, net, loader, n)
            res[name].append(ms)
    for name in res:
        print("%-19s %8.3f..%-8.3f ms/batch   top1 %.2f top5 %.2f" % (name, min(res[name]), max(res[name]),
                                                                      last[name]["top1"], last[name]["top5"]))
    old, new = res["evaluate"], res["evaluate_streaming"]
    print("evaluate / evaluate_streaming: %.3fx at best, >= %.3fx%s" % (
        min(old) / min(new), min(old) / max(new), "" if max(new) < min(old) else "   RANGES OVERLAP"), flush=True)


def launch_alone(calls=200):
    print("StreamMeter.update alone, %d x %d x %d logits, confusion matrix on; by HIP events around %d back-to-back calls "
          "(the host's enqueue or the kernel, whichever is slower) and around a captured replay of them, min..max of 3 runs" % (
              VIDEOS, VIEWS, CLASSES, calls))
    labels = torch.randint(0, CLASSES, (VIDEOS,), device=DEV)
    for dtype in (torch.float32, torch.bfloat16):
        logits = torch.randn(VIDEOS * VIEWS, CLASSES, device=DEV).to(dtype)
        meter = StreamMeter(CLASSES, views=VIEWS)
        for _ in range(20):
            meter.update(logits, labels)
        runs = []
        for _ in range(3):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(calls):
                meter.update(logits, labels)
            stop.record()
            stop.synchronize()
            runs.append(start.elapsed_time(stop) / calls * 1e3)
        assert meter.torch_updates == 0 and meter.result()["videos"] == VIDEOS * (20 + 3 * calls)
        # the same `calls` launches captured once and replayed: no host work between them, so this is the kernel's own time
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(calls):
                meter.update(logits, labels)
        torch.cuda.synchronize()
        meter.reset()
        replays = []
        for _ in range(4):                               # (the first replay is the warm-up)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            graph.replay()
            stop.record()
            stop.synchronize()
            replays.append(start.elapsed_time(stop) / calls * 1e3)
        assert meter.result()["videos"] == VIDEOS * 4 * calls
        print("%-9s %7.2f..%-7.2f us/call back to back, %6.2f..%-6.2f us/launch in a captured replay (%d bytes of logits)" % (
            str(dtype).replace("torch.", ""), min(runs), max(runs), min(replays[1:]), max(replays[1:]),
            logits.numel() * logits.element_size()), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    args = ap.parse_args()
    loops(args.batches)
    launch_alone()
