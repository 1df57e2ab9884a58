"""fp64 host twin of a whole RubiksNet and the comparator of the step-parity tests -- TEST INFRASTRUCTURE.

`host_twin(net)` is a deep copy of the network on the CPU in float64.  On host tensors every product module takes its
stock PyTorch path (each fused entry point -- fused_bn.bn_relu / bn_relu_skip / bn_relu_tshift_* / bn_relu_shift2d,
pointwise.conv1x1 / fork_shortcut / stem_conv / fused_eval_block, train_block.fused_train_block / bn_relu_from_stats,
the SE layer, dp.train_step's step-scoped caches -- is guarded by `is_cuda`), so the twin is nn.BatchNorm2d, nn.Conv2d,
nn.Linear and autograd in fp64.  The three shift modules have no host path; the twin swaps them for the oracles:

    RubiksShift3D   shift_function -> oracle/torch_shift.py::oracle_shift (the C oracle, fp64)
    RubiksShift2D   forward        -> OracleShift2D (the C oracle, fp64, `normalize_grad` honoured)
    AttentionShift  forward        -> the tap softmax as a torch expression (autograd owns it), then the 3-tap filter of
                                      oracle/attention_oracle.py (pinned by tests/golden/attention_*.npz)

`twin_guard()` makes any call into the native library an error while the twin runs, so that nothing of the HIP path
can leak into the reference.

`capture()` snapshots what a training step produced (loss, logits, every parameter gradient, BatchNorm running
statistics, the updated parameters, an input gradient) and `check_step()` compares a fused and a stock GPU snapshot
with the twin's: for every tensor err_fused <= FACTOR * err_stock + floor, and err_stock <= ceiling, where err is the
relative-norm error against fp64 (the max-abs error is reported next to it).
"""
import contextlib
import copy
import functools
import math
import time

import torch
import torch.nn.functional as F

from oracle.torch_shift import OracleShift2D, OracleTemporalShift3, oracle_shift

F64 = torch.float64
DEV = "cuda:0"
FACTOR = 3.0
LR = 0.1
# every fusion switch of config.py off: stock PyTorch modules plus the HIP shift operators
STOCK_SWITCHES = {"RK_FUSED_TRAIN": "0", "RK_FUSED_BN": "0", "RK_PW": "0", "RK_FUSED_EVAL": "0", "RK_PRESOFT": "0",
                  "RK_PREPACK": "0", "RK_BN_SHIFT2D": "0", "RK_BN_TSHIFT_FORK": "0", "RK_PW16_STATS": "0",
                  "RK_WGRAD_OVERLAP": "0"}
SHIFT_NEAR_ZERO = 1e-3          # shift-table gradient components below this (x the row's max) are not compared


def _twin_taps(layer, x):
    """AttentionShift.forward on the host: softmax((w / (std(w, unbiased) + 1e-6)) / T) over the 3 taps, then the filter."""
    w = layer.weight
    z = w / (w.std(dim=1, keepdim=True) + 1e-6) / layer.T
    return OracleTemporalShift3.apply(x, torch.softmax(z, dim=1), layer.n_segment)


def _twin_shift2d(layer, x):
    return OracleShift2D.apply(x, layer.shift, layer.stride, layer.padding, bool(layer.normalize_grad), bool(layer.quantize))


def host_twin(net):
    """Deep copy of `net` (a RubiksNet, or any module built of its parts) on the CPU in float64, its shift modules
    evaluated by the oracles."""
    from rubiksnet_amd.attention_shift import AttentionShift
    from rubiksnet_amd.shiftlib import RubiksShift2D, RubiksShift3D

    twin = copy.deepcopy(net).cpu().to(F64)
    for m in twin.modules():
        for cached in ("_rk_presoft_plan", "_rk_prefold_plan", "_rk_prepack_plan"):
            m.__dict__.pop(cached, None)
        if isinstance(m, RubiksShift3D):
            m.shift_function = oracle_shift
        elif isinstance(m, RubiksShift2D):
            m.forward = functools.partial(_twin_shift2d, m)
        elif isinstance(m, AttentionShift):
            assert m.weight is not None, "AttentionShift without weights: run one forward before making the twin"
            m.forward = functools.partial(_twin_taps, m)
    return twin


@contextlib.contextmanager
def twin_guard():
    """Inside the block any use of librubiks_hip raises: the twin must never reach the HIP path."""
    from rubiksnet_amd import _native

    def refuse(*_args, **_kw):
        raise AssertionError("the fp64 host twin reached the native HIP library")

    saved = _native.lib
    _native.lib = refuse
    try:
        yield
    finally:
        _native.lib = saved


# ------------------------------------------------------------------------------------------------ snapshots
def capture(net, loss, logits, inputs=None):
    """What a step left behind, as float64 host tensors keyed by name, plus the exact integer counters."""
    rec = {"loss": loss.detach().to("cpu", F64).reshape(1), "logits": logits.detach().to("cpu", F64)}
    grads, trainable = set(), set()
    for name, p in net.named_parameters():
        if p.requires_grad:
            trainable.add(name)
        if p.grad is not None:
            grads.add(name)
            rec["grad:" + name] = p.grad.detach().to("cpu", F64)
        rec["param:" + name] = p.detach().to("cpu", F64)
    counters = {}
    for name, m in net.named_modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.running_mean is not None:
            rec["running_mean:" + name] = m.running_mean.detach().to("cpu", F64)
            rec["running_var:" + name] = m.running_var.detach().to("cpu", F64)
            counters["num_batches_tracked:" + name] = int(m.num_batches_tracked)
    if inputs is not None:
        rec["input_grad"] = None if inputs.grad is None else inputs.grad.detach().to("cpu", F64)
    return {"tensors": rec, "grads": grads, "trainable": trainable, "counters": counters}


def _is_shift_grad(key):
    return key.startswith("grad:") and key.endswith("shift")


def errors(got, ref, key=""):
    """(relative-norm error, max-abs error) of `got` against `ref`.  Shift-table gradients are unit vectors after the
    normalisation of the backward: their near-zero components are left out."""
    if got is None or ref is None:
        return (math.inf, math.inf) if (got is None) != (ref is None) else (0.0, 0.0)
    if tuple(got.shape) != tuple(ref.shape):
        return math.inf, math.inf
    if not bool(torch.isfinite(got).all()):
        return math.inf, math.inf
    if _is_shift_grad(key):                          # [D, C]: one row per shifted axis
        keep = ref.abs() >= SHIFT_NEAR_ZERO * ref.abs().amax(dim=1, keepdim=True)
        got, ref = got[keep], ref[keep]
    diff = got - ref
    den = float(ref.norm())
    rel = float(diff.norm()) / den if den > 0 else float(diff.norm())
    return rel, float(diff.abs().max()) if diff.numel() else 0.0


# The floor of the bar, by the storage precision of the activations and by where the tensor sits.  Forward quantities
# (loss, logits, running statistics) and the classifier head's parameters have no ReLU between them and the loss: fp32
# round-off.  Every other gradient sits behind ReLU kinks, and a handful of the ~10^6 activations of a step lie within
# fp32 round-off of zero: which side they fall on is arbitrary, and the fused BatchNorm (y = a x + b, a = gamma invstd,
# b = beta - mean a) decides a few of them differently from both fp64 and stock PyTorch ((x - mean) invstd gamma + beta).
# Each flip moves one element's gradient by O(1); upstream of it a whole-network gradient moves by ~1e-3 relative
# (measured: at most 7.8e-3, a shift-table gradient of the last RubiksNet-Large block, where stock is at 1.4e-5).
_PRECISE = {torch.float32: 1e-5, torch.bfloat16: 1e-2}
_KINK = {torch.float32: 1.5e-2, torch.bfloat16: 5e-2}


# err_stock stays under this whatever the tensor (measured: 1.8e-2 fp32, a shift-table gradient of RubiksNet-Small; in
# bf16 the gradients of a 50-block network have decorrelated from fp64 -- up to 1.6 -- and only garbage is caught)
CEILING = {torch.float32: 5e-2, torch.bfloat16: 2.5}


def floor_for(dtype, key):
    if key in ("loss", "logits") or key.startswith(("running_mean:", "running_var:", "grad:new_fc.", "param:new_fc.")):
        return _PRECISE[dtype]
    return _KINK[dtype]


def check_step(fused, stock, twin, *, dtype, ceiling=None, label=""):
    """Compare two GPU snapshots with the twin's.  Returns the rows (key, err_stock, err_fused, maxabs_stock,
    maxabs_fused); raises AssertionError naming every tensor that misses its bar, a missing / extra gradient and a
    counter that differs."""
    ceiling = CEILING[dtype] if ceiling is None else ceiling
    problems = []
    for which, snap in (("fused", fused), ("stock", stock), ("twin", twin)):
        frozen = sorted(snap["grads"] - snap["trainable"])
        if frozen:
            problems.append("%s: gradient on a frozen parameter %s" % (which, ", ".join(frozen)))
    if twin["grads"] != twin["trainable"]:
        problems.append("twin: no gradient for %s" % ", ".join(sorted(twin["trainable"] - twin["grads"])))
    for which, snap in (("fused", fused), ("stock", stock)):
        missing = sorted(twin["grads"] - snap["grads"])
        extra = sorted(snap["grads"] - twin["grads"])
        if missing:
            problems.append("%s: no gradient for %s" % (which, ", ".join(missing)))
        if extra:
            problems.append("%s: gradient the twin does not have for %s" % (which, ", ".join(extra)))
        for k, v in twin["counters"].items():
            if snap["counters"].get(k) != v:
                problems.append("%s: %s = %s, the twin has %d" % (which, k, snap["counters"].get(k), v))
    rows = []
    for key, ref in twin["tensors"].items():
        rs, ms = errors(stock["tensors"].get(key), ref, key)
        rf, mf = errors(fused["tensors"].get(key), ref, key)
        rows.append((key, rs, rf, ms, mf))
        if not rs <= ceiling:
            problems.append("stock %s: err %.3e over the ceiling %.1e (max abs %.3e)" % (key, rs, ceiling, ms))
        bar = FACTOR * rs + floor_for(dtype, key)
        if not rf <= bar:
            problems.append("fused %s: err %.3e over the bar %.3e (stock %.3e; max abs fused %.3e stock %.3e)"
                            % (key, rf, bar, rs, mf, ms))
    for key in sorted(set(fused["tensors"]) - set(twin["tensors"])):
        problems.append("fused %s: not in the twin's snapshot" % key)
    if problems:
        raise AssertionError("%s: %d mismatch(es) against the fp64 twin:\n  %s\n%s"
                             % (label, len(problems), "\n  ".join(problems), summary(rows, label)))
    return rows


def summary(rows, label):
    """One line per tensor family: the worst err_stock / err_fused (relative norm) and the worst fused max-abs."""
    fams = {}
    for key, rs, rf, ms, mf in rows:
        fam = key.split(":")[0]
        if fam == "grad" and key.endswith("shift"):
            fam = "grad(shift)"
        a = fams.setdefault(fam, [0.0, 0.0, 0.0])
        a[0], a[1], a[2] = max(a[0], rs), max(a[1], rf), max(a[2], mf)
    return "\n".join("%s %-16s err_stock %.2e  err_fused %.2e  maxabs_fused %.2e" % (label, f, *v) for f, v in fams.items())


# ------------------------------------------------------------------------------------------------ procedures
def sgd_step(net, clips, labels):
    """One dp.train_step with plain SGD (no momentum) over the trainable parameters; returns (loss, logits).  A network
    with nothing to train gets forward + backward only."""
    from rubiksnet_amd import dp

    seen = {}

    def criterion(out, y):
        seen["logits"] = out
        return F.cross_entropy(out, y)

    params = [p for p in net.parameters() if p.requires_grad]
    if not params:
        loss = criterion(net(clips), labels)
        loss.backward()
        return loss, seen["logits"]
    loss = dp.train_step(net, torch.optim.SGD(params, lr=LR, momentum=0.0), clips, labels, criterion=criterion)
    return loss, seen["logits"]


def run_three(monkeypatch, net0, clips, labels, procedure=sgd_step, *, bf16=False, input_grad=False):
    """`procedure(net, clips, labels) -> (loss, logits)` on three deep copies of the host model `net0`: "fused" (GPU,
    default switches), "stock" (GPU, STOCK_SWITCHES) and "twin" (host_twin, fp64, the native library locked away).
    bf16: the GPU runs under bf16 autocast.  Returns {mode: capture(...)}, with the seconds each took under "secs" and
    the growth of train_block.stats_fallbacks() under "fallbacks"."""
    from rubiksnet_amd import config, train_block

    out = {}
    for mode in ("fused", "stock"):
        with monkeypatch.context() as mp:
            for k, v in (STOCK_SWITCHES.items() if mode == "stock" else ()):
                mp.setenv(k, v)
            config.reload()
            net = copy.deepcopy(net0).to(DEV)
            x = clips.detach().to(DEV, copy=True).requires_grad_(input_grad)
            before = train_block.stats_fallbacks()
            t0 = time.perf_counter()
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
                loss, logits = procedure(net, x, labels.to(DEV))
            if x.is_cuda:
                torch.cuda.synchronize()
            out[mode] = capture(net, loss, logits, x if input_grad else None)
            out[mode]["secs"] = time.perf_counter() - t0
            out[mode]["fallbacks"] = train_block.stats_fallbacks() - before
        config.reload()
    twin = host_twin(net0)
    x = clips.detach().to(F64, copy=True).requires_grad_(input_grad)
    t0 = time.perf_counter()
    with twin_guard():
        loss, logits = procedure(twin, x, labels)
    out["twin"] = capture(twin, loss, logits, x if input_grad else None)
    out["twin"]["secs"] = time.perf_counter() - t0
    return out
