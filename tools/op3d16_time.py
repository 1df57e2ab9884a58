"""python tools/op3d16_time.py [--batch 32] [--step]: RubiksShift3D under bf16 autocast, the cast path against the native
16-bit kernels, on the distinct (shape, stride) shift configurations of RubiksNet-Large and -Tiny.

(a) cast    what rubiks_shift_3d does with RK_SHIFT3D_16=0: widen x to fp32, the fp32 operator, narrow y (and the mirror
            image in the backward), casts included
(b) native  RubiksShift3D16Func on the bf16 tensors (rk3d_*_sf32), whatever family the planner gives it -- also for the
            configurations rubiks_shift_3d does not route to it (column `routed`), so the table shows what they would do
Both run in this process, alternating, warmed up, each point over at least 0.5 s of back-to-back calls on 3 rotating buffer
sets, three times over (min .. max shown).  us, and algorithmic GB/s of the native byte count (forward 4 B, backward 6 B per
element of the larger tensor side) against the 8 TB/s HBM roofline.
--step: one RubiksNet-Large rubiks3d train step under bf16 autocast with RK_SHIFT3D_16 = 1 and 0: ms/step and peak memory."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rubiksnet_amd import RubiksNet, _native, config, dp  # noqa: E402
from rubiksnet_amd.shiftlib import RubiksShift3D  # noqa: E402
from rubiksnet_amd.shiftlib.rubiks3d.primitive import RubiksShift3D16Func, RubiksShift3DFunc  # noqa: E402

DEV = "cuda:0"
ROOF = 8e12


def shift_configs(tier):
    """[(C, H, W, stride)] of the tier's RubiksShift3D layers, distinct, in network order."""
    net = RubiksNet(tier, 8, verbose=False).to(DEV).eval()
    seen = []

    def hook(mod, inp, out):
        key = (tuple(inp[0].shape[2:]), tuple(mod.stride))
        if key not in seen:
            seen.append(key)

    hs = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, RubiksShift3D)]
    with torch.no_grad():
        net(torch.randn(1, 8, 3, 224, 224, device=DEV))
    for h in hs:
        h.remove()
    return seen


def cast_path(x, shift, stride):
    return RubiksShift3DFunc.apply(x.float(), shift.float(), stride, 0, True, 1.0, False).to(x.dtype)


def native_path(x, shift, stride):
    return RubiksShift3D16Func.apply(x, shift, stride, 0, True, 1.0, False)


def us_per_call(fn, min_seconds=0.5):
    for i in range(10):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(20):
        fn(i)
    torch.cuda.synchronize()
    reps = max(20, int(min_seconds / max((time.perf_counter() - t0) / 20, 1e-6)))
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def time_config(N, T, C, H, W, stride):
    torch.manual_seed(0)
    sets = []
    for _ in range(3):
        x = torch.randn(N, T, C, H, W, device=DEV).to(torch.bfloat16).requires_grad_(True)
        shift = (torch.rand(3, C, device=DEV) * 2 - 1).requires_grad_(True)
        with torch.no_grad():
            gy = torch.randn_like(native_path(x, shift, stride))
        sets.append((x, shift, gy))

    def both(path):
        def fn(i):
            x, shift, gy = sets[i % 3]
            x.grad = shift.grad = None
            path(x, shift, stride).backward(gy)
        return fn

    def forward(path):
        def fn(i):
            x, shift, _ = sets[i % 3]
            path(x, shift, stride)
        return fn

    res = {}
    for rep in range(3):
        for name, path in (("cast", cast_path), ("native", native_path)):
            res.setdefault((name, "fwd"), []).append(us_per_call(forward(path)))
            res.setdefault((name, "all"), []).append(us_per_call(both(path)))
    nin, nout = sets[0][0].numel(), sets[0][2].numel()
    return res, 2 * (nin + nout), 2 * (2 * nin + nout) + 2 * (nin + nout)


def op_table(batch):
    L = _native.lib()
    print("RubiksShift3D under bf16 autocast, batch %d, T = 8: cast path (fp32 operator between two casts) vs native 16-bit "
          "kernels; us as min..max of 3 runs of >= 0.5 s each; GB/s = native bytes (fwd 4, fwd+bwd 10 per element) / time; "
          "roofline 8000 GB/s" % batch)
    print("%-6s %-22s %-8s %-7s | %-19s %-19s | %-19s %-19s | %6s %6s | %9s" % (
        "tier", "[N,T,C,H,W]", "stride", "routed", "cast fwd us", "native fwd us", "cast fwd+bwd us", "native fwd+bwd us",
        "GB/s", "% roof", "speed-up"))
    done = set()
    for tier in ("large", "tiny"):
        for (C, H, W), stride in shift_configs(tier):
            if (C, H, W, stride) in done:
                continue
            done.add((C, H, W, stride))
            res, fwd_bytes, all_bytes = time_config(batch, 8, C, H, W, stride)
            routed = L.rk3d_sf32_streams(batch, 8, C, H, W, *stride, 0, 0, 0, 0, 2)
            span = lambda k: "%8.1f..%-8.1f" % (min(res[k]), max(res[k]))  # noqa: E731
            nat, cast = min(res[("native", "all")]), min(res[("cast", "all")])
            worst = min(res[("cast", "all")]) / max(res[("native", "all")])
            print("%-6s %-22s %-8s %-7s | %s %s | %s %s | %6.0f %6.1f | %4.2fx (>= %4.2fx)" % (
                tier, "[%d,8,%d,%d,%d]" % (batch, C, H, W), "".join(map(str, stride)), "yes" if routed else "no",
                span(("cast", "fwd")), span(("native", "fwd")), span(("cast", "all")), span(("native", "all")),
                all_bytes / nat / 1e3, 100 * all_bytes / (nat * 1e-6) / ROOF, cast / nat, worst), flush=True)


def train_step(batch, steps=10, warmup=3):
    print("RubiksNet-Large rubiks3d train step, bf16 autocast, batch %d, %d steps after %d warm-up" % (batch, steps, warmup))
    for on in ("1", "0", "1", "0"):
        config.reload(dict(os.environ, RK_SHIFT3D_16=on))
        torch.manual_seed(0)
        net = RubiksNet("large", 174, verbose=False).to(DEV)
        opt = dp.make_optimizer(net, lr=1e-3)
        clips = torch.randn(batch, 8, 3, 224, 224, device=DEV)
        labels = torch.randint(0, 174, (batch,), device=DEV)
        torch.cuda.reset_peak_memory_stats()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            for _ in range(warmup):
                dp.train_step(net, opt, clips, labels)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                dp.train_step(net, opt, clips, labels)
            torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        print("RK_SHIFT3D_16=%s: %.1f ms/step, peak memory %.2f GiB" % (on, ms, torch.cuda.max_memory_allocated() / 2**30),
              flush=True)
        del net, opt
        torch.cuda.empty_cache()
    config.reload()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--no-ops", action="store_true")
    args = ap.parse_args()
    if not args.no_ops:
        op_table(args.batch)
    if args.step:
        train_step(args.batch)
