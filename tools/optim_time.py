"""python tools/optim_time.py [--step] [--batch 32]: the one-launch optimizer step (rubiksnet_amd.optim, rk_optim.hip) against
what dp.make_optimizer gave before it -- torch.optim.Adam(fused=True) and torch.optim.SGD -- on the parameter sets of
RubiksNet-Large and RubiksNet-Tiny with synthetic gradients, with and without clipping by the global norm (the torch side:
torch.nn.utils.clip_grad_norm_ + step).

Both run in this process, alternating, warmed up; each point is us per step over at least 0.5 s of back-to-back steps ending
in a device synchronise, three runs, printed as min..max.  "launch" is the new step without its pass over the parameters
(the kept job table launched again: hyper-parameters, one or two ctypes calls, the kernels).  GB/s = the bytes the rule has to
move (SGD with momentum 5, Adam 7 dwords per element, one more for the norm's pass over the gradients) over the best launch
time, against 8 TB/s.

--step: one RubiksNet-Large-AQ train step under bf16 autocast with kind="adam" and kind="hip_adam", four alternating runs.

--ext: the rows of the extended step (rk_optim_step_ext_f32) on RubiksNet-Large, same protocol: AdamW against
torch.optim.AdamW(fused=True); Adam + EMA against fused Adam + torch._foreach_lerp_; AdamW + EMA + guard and SGD + guard
(both clipping at the same max norm) against clip_grad_norm_ + an isfinite test of its norm + step (+ lerp).
--against OTHER.so [--against-py OTHER_OPTIM.py]: the plain SGD / Adam rows with this build and with another build of the
library (the parent commit's; with --against-py that commit's rubiksnet_amd/optim.py too) alternating in one process on the
same tensors; SLOWER is printed when this build's range lies wholly above the other's."""
import argparse
import ctypes
import importlib.util
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rubiksnet_amd import RubiksNet, _native, dp, optim  # noqa: E402

DEV = torch.device("cuda:0")
ROOF = 8e12
MAX_NORM = 20.0


def us_per_call(fn, min_seconds=0.5):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    reps = max(20, int(min_seconds / max((time.perf_counter() - t0) / 20, 1e-6)))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def stepper(tier, kind, clip):
    """A closure that runs one optimizer step (with its clipping) on a fresh copy of the tier's parameters."""
    torch.manual_seed(0)
    net = RubiksNet(tier, 174, verbose=False).to(DEV)
    params = [p for p in net.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.randn_like(p) * 1e-2
    native = kind.startswith("hip_")
    opt = dp.make_optimizer(net, lr=1e-5, lr_shift_mult=0.1, kind=kind, momentum=0.9, weight_decay=5e-4,
                            max_grad_norm=MAX_NORM if (clip and native) else None)
    if clip and not native:
        def fn():
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            opt.step()
    else:
        fn = opt.step
    return fn, opt, sum(p.numel() for p in params), len(params)


def table():
    print("optimizer step, fp32 parameters, synthetic gradients; us per step as min..max of 3 alternating runs of >= 0.5 s; "
          "GB/s = rule bytes / best launch time; roofline 8000 GB/s")
    print("%-6s %-5s %-5s %9s %7s | %-21s %-21s %-21s | %7s %6s | %s" % (
        "tier", "rule", "clip", "elements", "tensors", "torch.optim us", "one-launch step us", "launch us", "GB/s", "% roof",
        "speed-up"))
    for tier in ("large", "tiny"):
        for rule, dwords in (("sgd", 5), ("adam", 7)):
            for clip in (False, True):
                old, _, numel, ntensors = stepper(tier, rule, clip)
                new, opt, _, _ = stepper(tier, "hip_" + rule, clip)
                res = {"old": [], "new": [], "launch": []}
                for _ in range(3):
                    res["old"].append(us_per_call(old))
                    res["new"].append(us_per_call(new))
                    res["launch"].append(us_per_call(lambda: opt._launch_table(opt._table)))
                assert opt.torch_steps == 0 and opt.native_steps > 0
                nbytes = 4 * numel * (dwords + (1 if clip else 0))
                best, launch = min(res["new"]), min(res["launch"])
                span = lambda k: "%9.1f..%-9.1f" % (min(res[k]), max(res[k]))  # noqa: E731
                print("%-6s %-5s %-5s %9d %7d | %s %s %s | %7.0f %6.1f | %4.2fx (>= %4.2fx)%s" % (
                    tier, rule, "yes" if clip else "no", numel, ntensors, span("old"), span("new"), span("launch"),
                    nbytes / launch / 1e3, 100 * nbytes / (launch * 1e-6) / ROOF, min(res["old"]) / best,
                    min(res["old"]) / max(res["new"]),
                    "" if max(res["new"]) < min(res["old"]) else "   RANGES OVERLAP"), flush=True)
                del old, new, opt
                torch.cuda.empty_cache()


EMA_DECAY = 0.999
EXT_ROWS = [("AdamW", "hip_adamw", dict(), 7),
            ("Adam + EMA", "hip_adam", dict(ema_decay=EMA_DECAY), 9),
            ("AdamW + EMA + guard (clipping)", "hip_adamw", dict(ema_decay=EMA_DECAY, skip_nonfinite=True, max_grad_norm=MAX_NORM), 10),
            ("SGD + guard (clipping)", "hip_sgd", dict(skip_nonfinite=True, max_grad_norm=MAX_NORM), 6)]


def _large():
    torch.manual_seed(0)
    net = RubiksNet("large", 174, verbose=False).to(DEV)
    params = [p for p in net.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.randn_like(p) * 1e-2
    return net, params


def ext_stepper(kind, kw, native):
    """One step of an extended row: rubiksnet_amd.optim's, or what a user writes around torch.optim for the same effect."""
    net, params = _large()
    common = dict(lr=1e-5, lr_shift_mult=0.1, momentum=0.9, weight_decay=5e-4)
    if native:
        opt = dp.make_optimizer(net, kind=kind, **common, **kw)
        return opt.step, opt, params
    if kind == "hip_adamw":
        shift = [p for n, p in net.named_parameters() if n.endswith("shift")]
        rest = [p for n, p in net.named_parameters() if not n.endswith("shift")]
        opt = torch.optim.AdamW([{"params": shift, "lr": 1e-6}, {"params": rest}], lr=1e-5, weight_decay=5e-4, fused=True)
    else:
        opt = dp.make_optimizer(net, kind=kind[4:], **common)
    shadows = [p.detach().clone() for p in params] if "ema_decay" in kw else None
    guard = kw.get("skip_nonfinite", False)

    def fn():
        if guard:
            if not bool(torch.isfinite(torch.nn.utils.clip_grad_norm_(params, MAX_NORM))):
                return
        opt.step()
        if shadows is not None:
            torch._foreach_lerp_(shadows, [p.detach() for p in params], 1.0 - EMA_DECAY)
    return fn, opt, params


def ext_table():
    print("extended optimizer step, RubiksNet-Large, fp32 parameters, synthetic gradients; us per step as min..max of 3 "
          "alternating runs of >= 0.5 s; GB/s = rule bytes / best launch time; roofline 8000 GB/s")
    print("%-32s %9s | %-21s %-21s %-21s | %7s %6s | %s" % ("row", "elements", "torch us", "one-launch step us", "launch us",
                                                            "GB/s", "% roof", "speed-up"))
    for name, kind, kw, dwords in EXT_ROWS:
        old, _, params = ext_stepper(kind, kw, False)
        new, opt, _ = ext_stepper(kind, kw, True)
        numel = sum(p.numel() for p in params)
        res = {"old": [], "new": [], "launch": []}
        for _ in range(3):
            res["old"].append(us_per_call(old))
            res["new"].append(us_per_call(new))
            res["launch"].append(us_per_call(lambda: opt._launch_table(opt._table)))
        assert opt.torch_steps == 0 and opt.native_steps > 0 and (not opt.skip_nonfinite or opt.skipped_steps == 0)
        nbytes, launch = 4 * numel * dwords, min(res["launch"])
        span = lambda k: "%9.1f..%-9.1f" % (min(res[k]), max(res[k]))  # noqa: E731
        print("%-32s %9d | %s %s %s | %7.0f %6.1f | %4.2fx (>= %4.2fx)" % (
            name, numel, span("old"), span("new"), span("launch"), nbytes / launch / 1e3,
            100 * nbytes / (launch * 1e-6) / ROOF, min(res["old"]) / min(res["new"]), min(res["old"]) / max(res["new"])),
            flush=True)
        del old, new, opt
        torch.cuda.empty_cache()


def against(path, py=None):
    """The plain rows (rk_optim_sgd_many_f32 / rk_optim_adam_many_f32) of this build and of the library at `path` (with
    py: of the classes in that other optim.py too), both stepping the SAME parameters and gradients, in ABBA order."""
    other = ctypes.CDLL(path)
    for name, (res, args) in _native.SIGNATURES.items():
        if name.startswith(("rk_optim", "rk_debug_optim")) and hasattr(other, name):
            fn = getattr(other, name)
            fn.restype, fn.argtypes = res, args
    mod = optim
    if py:
        spec = importlib.util.spec_from_file_location("rubiksnet_amd._optim_other", py)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    print("plain rows, RubiksNet-Large: this build against %s%s, same tensors, ABBA; us as min..max of 4 runs of >= 0.5 s" % (
        path, " + " + py if py else ""))
    print("%-5s %-5s | %-21s %-21s | %-21s %-21s | %s" % ("rule", "clip", "step us (this)", "step us (other)", "launch us (this)",
                                                          "launch us (other)", "verdict"))
    for rule in ("sgd", "adam"):
        for clip in (False, True):
            net, _ = _large()
            new = dp.make_optimizer(net, lr=1e-5, lr_shift_mult=0.1, kind="hip_" + rule, momentum=0.9, weight_decay=5e-4,
                                    max_grad_norm=MAX_NORM if clip else None)
            groups = [{"params": g["params"], "lr_mult": g["lr_mult"]} for g in new.param_groups]
            kw = dict(lr=1e-5, weight_decay=5e-4, max_grad_norm=MAX_NORM if clip else None)
            old = mod.RubiksSGD(groups, momentum=0.9, **kw) if rule == "sgd" else mod.RubiksAdam(groups, **kw)
            old._lib = other
            res = {k: [] for k in ("new", "old", "lnew", "lold")}
            for r in range(4):
                for k, opt in ((("new", new), ("old", old)) if r % 2 == 0 else (("old", old), ("new", new))):
                    res[k].append(us_per_call(opt.step))
                    res["l" + k].append(us_per_call(lambda: opt._launch_table(opt._table)))
            assert new.torch_steps == 0 and old.torch_steps == 0 and old.native_steps > 0
            span = lambda k: "%9.1f..%-9.1f" % (min(res[k]), max(res[k]))  # noqa: E731
            slower = [k for k, o in (("new", "old"), ("lnew", "lold")) if min(res[k]) > max(res[o])]
            print("%-5s %-5s | %s %s | %s %s | %s" % (rule, "yes" if clip else "no", span("new"), span("old"), span("lnew"),
                                                      span("lold"), "SLOWER: " + ", ".join(slower) if slower else "not slower"),
                  flush=True)
            del net, new, old
            torch.cuda.empty_cache()


def train_step(batch, steps=10, warmup=3):
    print("RubiksNet-Large-AQ train step, bf16 autocast, batch %d, %d steps after %d warm-up" % (batch, steps, warmup))
    for kind in ("adam", "hip_adam", "adam", "hip_adam"):
        torch.manual_seed(0)
        net = RubiksNet("large", 174, variant="rubiks3d-aq", verbose=False).to(DEV)
        opt = dp.make_optimizer(net, lr=1e-3, kind=kind)
        clips = torch.randn(batch, 8, 3, 224, 224, device=DEV)
        labels = torch.randint(0, 174, (batch,), device=DEV)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            for _ in range(warmup):
                dp.train_step(net, opt, clips, labels)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = dp.train_step(net, opt, clips, labels)
            torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        print("kind=%-8s: %.2f ms/step (loss %.4f)" % (kind, ms, float(loss.detach())), flush=True)
        del net, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--no-table", action="store_true")
    ap.add_argument("--ext", action="store_true")
    ap.add_argument("--against", metavar="OTHER.so")
    ap.add_argument("--against-py", metavar="OTHER_OPTIM.py")
    args = ap.parse_args()
    if not args.no_table:
        table()
    if args.ext:
        ext_table()
    if args.against:
        against(args.against, args.against_py)
    if args.step:
        train_step(args.batch)
