"""Generates tests/golden/binding_trace_parent.json.gz: what the Python bindings of the 1x1 convolutions, the stem, the
fused BatchNorms and the fused blocks ask of librubiks_hip, and what comes back.

For each scenario below (one per route of `conv1x1`, the stem, `bn_relu*`, the fused blocks, one whole-model train step
and eval forward) a recording proxy in the place of `_native._lib` stores every call into the library -- the entry
name, every integer and float argument verbatim, each pointer as "null" / "ptr", the stream of a launch as "current" /
"other", the value a query (`*_bytes`, `*_tiles`, `*_supported`, ...) returned -- and a SHA-256 of every output and
gradient is taken.  tests/test_binding_trace_gpu.py replays the scenarios and asserts the identical call list and the
identical digests: a refactor of the binding layer must not change what runs on the device.

Run on a GPU, on the commit whose behaviour is to be kept, with only this file added:

    python tests/golden/gen_binding_trace_golden.py [output path]

Every scenario runs twice; the golden is not written when the two runs differ (the kernels sum in a fixed order
without atomics, so a difference is a finding).  Only functions the package exports on both sides of a refactor are
used: conv1x1, fork_shortcut, stem_conv, bn_relu, bn_relu_skip, fused_eval_block, fused_train_block, RubiksNet,
dp.train_step."""
import contextlib
import ctypes
import gzip
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _path in (os.path.dirname(TESTS), TESTS):
    if _path not in sys.path:
        sys.path.insert(0, _path)

from _util import DEV, seed_of  # noqa: E402

GOLDEN = os.path.join(HERE, "binding_trace_parent.json.gz")
F32, BF16 = torch.float32, torch.bfloat16

# entry points that launch nothing: their return value is part of the trace, and a trailing pointer is no stream
_QUERY_SUFFIXES = ("_bytes", "_tiles", "_supported", "_shape", "_streams")
_QUERY_NAMES = ("rk_version", "rk_error_string", "rk_out_len", "rk_device_count", "rk_fin_status_register")


def _is_query(name, restype):
    return (restype is not ctypes.c_int or name.endswith(_QUERY_SUFFIXES) or name in _QUERY_NAMES
            or name.startswith("rk_debug"))


class Recorder:
    """Stands in for the ctypes handle `_native.lib()` returns; `calls` is the trace."""

    def __init__(self, real, signatures):
        self._real, self._signatures, self._fns, self.calls = real, signatures, {}, []

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            fn = self._fns[name] = self._wrap(name)
        return fn

    def _wrap(self, name):
        real = getattr(self._real, name)
        restype, argtypes = self._signatures[name]
        query = _is_query(name, restype)

        def call(*args):
            rc = real(*args)
            assert len(args) == len(argtypes), name
            rec = []
            for k, (a, t) in enumerate(zip(args, argtypes)):
                if t is ctypes.c_void_p or isinstance(a, ctypes._Pointer) or hasattr(a, "_obj"):
                    a = getattr(a, "value", a)
                    if not query and k == len(args) - 1:
                        rec.append("current" if (a or 0) == torch.cuda.current_stream().cuda_stream else "other")
                    else:
                        rec.append("null" if not a else "ptr")
                elif isinstance(a, float):
                    rec.append(a)
                else:
                    rec.append(int(a))
            if query:
                rc_rec = rc.decode() if isinstance(rc, bytes) else int(rc)
                self.calls.append([name, rec, rc_rec])
            else:
                self.calls.append([name, rec])
            return rc

        return call


@contextlib.contextmanager
def recording():
    from rubiksnet_amd import _native, fin_status

    real = _native.lib()
    fin_status.ensure(torch.device(DEV))     # once per process: registered before the trace starts, whatever ran earlier
    rec = Recorder(real, _native.SIGNATURES)
    _native._lib = rec
    try:
        yield rec
    finally:
        _native._lib = real


def digest(t):
    return hashlib.sha256(t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


# ---- inputs ----------------------------------------------------------------------------------------------------

def _tensor(rng, shape, dtype=F32, grad=False):
    t = torch.from_numpy(rng.uniform(-1, 1, size=shape).astype(np.float32)).to(DEV).to(dtype)
    return t.requires_grad_(grad)


def _conv(rng, K, M, stride=1, kernel=1):
    conv = torch.nn.Conv2d(K, M, kernel, stride=stride, padding=kernel // 2, bias=False)
    w = rng.standard_normal((M, K, kernel, kernel)).astype(np.float32) / np.sqrt(K * kernel * kernel)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w))
    return conv.to(DEV)


def _fill_bn(rng, bn):
    C = bn.num_features
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)))
        bn.bias.copy_(torch.from_numpy((0.3 * rng.standard_normal(C)).astype(np.float32)))
        bn.running_mean.copy_(torch.from_numpy(rng.standard_normal(C).astype(np.float32)))
        bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)))
    return bn


def _bn(rng, C):
    return _fill_bn(rng, torch.nn.BatchNorm2d(C)).to(DEV)


def _autocast(dtype):
    return torch.autocast("cuda", dtype=BF16) if dtype == BF16 else contextlib.nullcontext()


@contextlib.contextmanager
def _switch(name, value):
    """An RK_* switch of config.py set for the block (None: left as it is)."""
    from rubiksnet_amd import config

    old = os.environ.get(name)
    if value is not None:
        os.environ[name] = value
    config.reload()
    try:
        yield
    finally:
        if value is not None:
            os.environ.pop(name) if old is None else os.environ.__setitem__(name, old)
        config.reload()


def _bn_state(prefix, bn):
    return {prefix + ".dgamma": bn.weight.grad, prefix + ".dbeta": bn.bias.grad, prefix + ".running_mean": bn.running_mean,
            prefix + ".running_var": bn.running_var, prefix + ".num_batches_tracked": bn.num_batches_tracked}


# ---- scenarios: each returns {name: tensor} ----------------------------------------------------------------------

def conv_case(rng, Fr, K, M, H, W, stride=1, res=False, dtype=F32, train=True, stats=None, stock=False):
    from rubiksnet_amd import pointwise

    conv = _conv(rng, K, M, stride).train(train)
    x = _tensor(rng, (Fr, K, H, W), dtype, True)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = _tensor(rng, (Fr, M, Ho, Wo), dtype, True) if res else None
    gy = _tensor(rng, (Fr, M, Ho, Wo), dtype)
    with _autocast(dtype), _switch("RK_PW16_STATS", stats):
        y = pointwise.conv1x1(conv, x, residual=r)
    y.backward(gy)
    out = {"y": y, "dx": x.grad, "dw": conv.weight.grad}
    if res:
        out["dr"] = r.grad
    if stock:
        # the stock path is MIOpen's, whose bits depend on the solver it picks (d(input) of this layer differed between two
        # processes of one commit, and within one process after other convolutions had run): no digest; what is held is that
        # no node of ours is in the graph and (by the caller) that no call was recorded
        assert not isinstance(y.grad_fn, torch.autograd.function.BackwardCFunction), type(y.grad_fn).__name__
    return out


def fork_case(rng, Fr, K, M, H, W):
    from rubiksnet_amd import pointwise

    conv = _conv(rng, K, M, 2)
    x = _tensor(rng, (Fr, K, H, W), BF16, True)
    gm = _tensor(rng, (Fr, K, H, W), BF16)
    gs = _tensor(rng, (Fr, M, H // 2, W // 2), BF16)
    with _autocast(BF16):
        main, y = pointwise.fork_shortcut(conv, x * 1.0)           # a non-leaf, as relu(bn1(.)) is
    torch.autograd.backward([main, y], [gm, gs])
    return {"y": y, "dx": x.grad, "dw": conv.weight.grad}


def stem_case(rng, train, dtype=F32, W=40):
    from rubiksnet_amd import pointwise

    conv = _conv(rng, 3, 54, 2, kernel=3).train(train)
    x = _tensor(rng, (2, 3, 32, W))
    gy = _tensor(rng, (2, 54, 16, W // 2), dtype)
    with _autocast(dtype):
        y = pointwise.stem_conv(conv, x)
    y.backward(gy)
    return {"y": y, "dw": conv.weight.grad}


def bn_case(rng, skip=False, train=True, relu=True):
    from rubiksnet_amd import fused_bn

    bn = _bn(rng, 16).train(train)
    x = _tensor(rng, (3, 16, 8, 8), F32, train)
    gy = _tensor(rng, (3, 16, 8, 8))
    if not train:
        with torch.no_grad():
            return {"y": fused_bn.bn_relu(bn, x, relu=relu)}
    if skip:
        y, same = fused_bn.bn_relu_skip(bn, x * 1.0)
        (y + 0.5 * same).backward(gy)
    else:
        y = fused_bn.bn_relu(bn, x, relu=relu)
        y.backward(gy)
    return dict(_bn_state("bn", bn), y=y, dx=x.grad)


def bn_stats_case(rng):
    """bn_relu on a tensor that carries the tile statistics of the bf16 GEMM that made it."""
    from rubiksnet_amd import fused_bn, pointwise

    conv, bn = _conv(rng, 72, 144).train(), _bn(rng, 144).train()
    x = _tensor(rng, (4, 72, 8, 8), BF16, True)
    gy = _tensor(rng, (4, 144, 8, 8), BF16)
    with _autocast(BF16), _switch("RK_PW16_STATS", "1"):
        z = pointwise.conv1x1(conv, x)
        assert getattr(z, "_rk_stats", None) is not None
        y = fused_bn.bn_relu(bn, z)
    y.backward(gy)
    return dict(_bn_state("bn", bn), y=y, dx=x.grad, dw=conv.weight.grad)


def _block(rng, cin, cout, stride, T):
    from rubiksnet_amd.backbone import RubiksShiftBlock
    from rubiksnet_amd.models import _Rubiks3DWrap

    class Parent:
        expansion, normalize_grad, quantize, init_shift, use_se = 1, True, False, "uniform", False

    torch.manual_seed(0)
    block = RubiksShiftBlock(cin, cout, stride=stride, parent=Parent())
    block.as3 = _Rubiks3DWrap(block.as3, n_segment=T)
    with torch.no_grad():
        for name, p in sorted(block.named_parameters()):
            if p.dim() == 4:
                p.copy_(torch.from_numpy((rng.standard_normal(tuple(p.shape)) * (2.0 / p.shape[1]) ** 0.5).astype(np.float32)))
            elif name.endswith("shift"):
                p.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(p.shape)).astype(np.float32)))
        for m in (block.bn1, block.bn2):
            _fill_bn(rng, m)
    return block.to(DEV)


def train_block_case(rng, cin, cout, stride, dims):
    from rubiksnet_amd import train_block

    N, T, H, W = dims
    block = _block(rng, cin, cout, stride, T).train()
    x = _tensor(rng, (N * T, cin, H, W), F32, True)
    dout = _tensor(rng, (N * T, cout, (H - 1) // stride + 1, (W - 1) // stride + 1))
    out = train_block.fused_train_block(block, x)
    assert out is not None, "the block must qualify for the fused training path"
    out.backward(dout)
    res = {"out": out, "dx": x.grad}
    res.update({"d." + name: p.grad for name, p in block.named_parameters()})
    res.update({name: b for name, b in block.named_buffers()})
    return res


def eval_block_case(rng, cin, cout, stride, dims):
    from rubiksnet_amd import pointwise

    N, T, H, W = dims
    block = _block(rng, cin, cout, stride, T).eval()
    x = _tensor(rng, (N * T, cin, H, W))
    with torch.no_grad():
        out = pointwise.fused_eval_block(block, x)
    assert out is not None, "the block must qualify for the fused inference path"
    return {"out": out}


def model_case(rng, train, dtype=F32):
    """RubiksNet-Tiny at the smallest input of tests/test_step_parity_gpu.py; the trace only (its numerics are held by
    test_step_parity_gpu.py and test_model_configs_gpu.py)."""
    from rubiksnet_amd import RubiksNet, dp

    torch.manual_seed(11)
    net = RubiksNet("tiny", 11, num_frames=8, verbose=False).to(DEV)
    clips = _tensor(rng, (2, 8, 3, 224, 224))
    labels = torch.from_numpy(rng.integers(0, 11, 2)).to(DEV)
    with _autocast(dtype):
        if train:
            dp.train_step(net.train(), torch.optim.SGD(net.parameters(), lr=0.05), clips, labels)
        else:
            with torch.no_grad():
                net.eval()(clips)
    torch.cuda.synchronize()
    return None


# name -> (function, arguments, an entry point the route must reach -- None: no call at all)
SCENARIOS = {
    "conv-f32-s1": (conv_case, dict(Fr=3, K=54, M=108, H=8, W=8), "rk_pw_gemm_f32"),
    "conv-f32-s1-res": (conv_case, dict(Fr=3, K=54, M=108, H=8, W=8, res=True), "rk_pw_gemm_f32"),
    "conv-f32-s2": (conv_case, dict(Fr=3, K=6, M=10, H=16, W=24, stride=2), "rk_pw_s2_forward_f32"),
    "conv-f32-7x7": (conv_case, dict(Fr=3, K=8, M=12, H=7, W=7), "rk_pw_gemm_odd_f32"),
    "conv-f32-7x7-res": (conv_case, dict(Fr=3, K=8, M=12, H=7, W=7, res=True), "rk_pw_gemm_odd_f32"),
    "conv-f32-14to7": (conv_case, dict(Fr=3, K=8, M=12, H=14, W=14, stride=2), "rk_pw_s2_forward_odd_f32"),
    "conv-bf16-s1-train": (conv_case, dict(Fr=4, K=72, M=144, H=8, W=8, dtype=BF16, stats="1"),
                           "rk_pw_gemm_packed_stats_bf16"),
    "conv-bf16-s1-eval": (conv_case, dict(Fr=4, K=72, M=144, H=8, W=8, dtype=BF16, train=False), "rk_pw_gemm_packed_bf16"),
    "conv-bf16-s1-res": (conv_case, dict(Fr=4, K=72, M=144, H=8, W=8, dtype=BF16, res=True), "rk_pw_gemm_packed_bf16"),
    "conv-bf16-s2": (conv_case, dict(Fr=4, K=72, M=144, H=8, W=8, stride=2, dtype=BF16), "rk_pw_gemm_packed_bf16"),
    "conv-bf16-7x7-res": (conv_case, dict(Fr=5, K=64, M=96, H=7, W=7, res=True, dtype=BF16), "rk_pw_gemm_packed_odd_bf16"),
    "conv-bf16-14to7": (conv_case, dict(Fr=4, K=64, M=96, H=10, W=14, stride=2, dtype=BF16), "rk_pw_gemm_packed_odd_bf16"),
    "fork-pw16": (fork_case, dict(Fr=2, K=16, M=32, H=16, W=24), "rk_scatter2x2_add_bf16"),
    "fork-odd16": (fork_case, dict(Fr=3, K=32, M=64, H=10, W=6), "rk_scatter2x2_add_bf16"),
    "conv-ineligible": (conv_case, dict(Fr=3, K=7, M=9, H=8, W=8, stock=True), None),
    "stem-f32-stats": (stem_case, dict(train=True), "rk_stem_conv3x3s2_stats_f32"),
    "stem-f32": (stem_case, dict(train=False), "rk_stem_conv3x3s2_f32"),
    # (rk_stem16.hip wants whole 16-column blocks of output: W % 32 == 0)
    "stem-bf16": (stem_case, dict(train=True, dtype=BF16, W=64), "rk_stem_conv3x3s2_bf16out"),
    "bn-relu": (bn_case, dict(), "rk_bn_relu_forward_counted_f32"),
    "bn-no-relu": (bn_case, dict(relu=False), "rk_bn_relu_forward_counted_f32"),
    "bn-relu-skip": (bn_case, dict(skip=True), "rk_bn_relu_forward_counted_f32"),
    "bn-relu-eval": (bn_case, dict(train=False), "rk_bn_relu_forward_f32"),
    "bn-relu-stats": (bn_stats_case, dict(), "rk_bn_apply_affine_bf16"),
    "train-block-identity": (train_block_case, dict(cin=16, cout=16, stride=1, dims=(2, 4, 14, 14)), "rk_pw_gemm_stats_f32"),
    "train-block-down": (train_block_case, dict(cin=16, cout=32, stride=2, dims=(2, 4, 28, 32)), "rk_pw_s2_forward_fused_f32"),
    "eval-block-identity": (eval_block_case, dict(cin=16, cout=16, stride=1, dims=(2, 4, 14, 14)), "rk_pw_gemm_fused_f32"),
    "eval-block-down": (eval_block_case, dict(cin=16, cout=32, stride=2, dims=(2, 4, 28, 32)), "rk_pw_s2_forward_fused_f32"),
    "tiny-train-f32": (model_case, dict(train=True), "rk_pw_gemm_stats_f32"),
    "tiny-train-bf16": (model_case, dict(train=True, dtype=BF16), "rk_pw_pack_many_bf16"),
    "tiny-eval-f32": (model_case, dict(train=False), "rk_bn_fold_many_f32"),
    "tiny-eval-bf16": (model_case, dict(train=False, dtype=BF16), "rk_pw_gemm_packed_bf16"),
}
# no digest: the whole-model scenarios (their numerics are held elsewhere) and the stock path (checked in place, above)
TRACE_ONLY = ("tiny-train-f32", "tiny-train-bf16", "tiny-eval-f32", "tiny-eval-bf16", "conv-ineligible")


def run(name):
    """One scenario under the recorder: {"calls": [...], "digests": {output: sha256} or None}."""
    fn, kwargs, expect = SCENARIOS[name]
    rng = np.random.default_rng(seed_of("binding-trace", name))
    with recording() as rec:
        tensors = fn(rng, **kwargs)
        torch.cuda.synchronize()
    names = [c[0] for c in rec.calls]
    if expect is None:
        assert not names, "%s: expected the stock path, recorded %r" % (name, names)
    else:
        assert expect in names, "%s: %s was not called (%r)" % (name, expect, sorted(set(names)))
    digests = None
    if name not in TRACE_ONLY:
        assert tensors and all(t is not None for t in tensors.values()), (name, [k for k, t in tensors.items() if t is None])
        digests = {k: digest(t) for k, t in sorted(tensors.items())}
    return {"calls": rec.calls, "digests": digests}


def load(path=GOLDEN):
    with gzip.open(path, "rt") as f:
        return json.load(f)


def main(path):
    golden, failed = {}, []
    for name in SCENARIOS:
        try:
            first, second = run(name), run(name)
        except Exception as e:           # (every scenario is tried before giving up: one GPU visit shows them all)
            failed.append("%s: %s: %s" % (name, type(e).__name__, e))
            continue
        if first != second:
            failed.append("%s: two runs differ in their %s" % (name, "digests" if first["digests"] != second["digests"] else "calls"))
            continue
        golden[name] = first
        print("%-24s %4d calls, %s outputs" % (name, len(first["calls"]), len(first["digests"] or ())))
    if failed:
        raise SystemExit("no golden written:\n" + "\n".join(failed))
    text = json.dumps(golden, separators=(",", ":"), sort_keys=True)
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(text.encode())
    print("wrote %s (%d bytes of JSON)" % (path, len(text)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
