"""RubiksSGD / RubiksAdam / RubiksAdamW: torch.optim.SGD's, Adam's and AdamW's update rules with the whole network's step in
ONE HIP launch (rk_optim.hip), the `lr_mult` / `decay_mult` keys of `RubiksNetBackbone.get_optim_policy()` honoured, and
optional clipping by the global gradient norm (one more launch, no host wait).

    opt = RubiksSGD(net.get_optim_policy(), lr=0.01, momentum=0.9, weight_decay=5e-4, max_grad_norm=20.0)

A group's effective rate is lr * lr_mult, its effective decay weight_decay * decay_mult (both default 1).  State keys and
layout are torch's (`momentum_buffer`; `step`, `exp_avg`, `exp_avg_sq`), so a state_dict() moves between these classes
and torch.optim.SGD / Adam in both directions.  Parameters whose .grad is None are skipped, as torch skips them.

The native path takes fp32 CUDA parameters (contiguous, one device, at most 8 groups).  Anything else -- CPU parameters,
another dtype, a ninth group, no built library -- runs the same rule, in the same order of operations, written with
torch ops: the classes work in the gloo / CPU tests and on a box without a GPU.  `native_steps` / `torch_steps` count which
path each step took.

The job table the kernels read (one 48-byte record per tensor: include/rubiks_hip.h) is built in pinned host memory,
uploaded asynchronously and kept until a parameter or gradient pointer changes or the set of parameters with a gradient
does (zero_grad(set_to_none=True) re-allocates the gradients; the caching allocator mostly hands the same blocks back);
load_state_dict and add_param_group drop it.  The hyper-parameters travel in the kernel arguments: an lr schedule never
causes an upload.  A step on a kept table costs the host one pass over the parameters (two data_ptr() each) and one or two
ctypes calls: the state tensors are the table's, and Adam's per-parameter `step` counters are 0-dim views of ONE host
tensor, advanced with one add.

Two opt-in keyword arguments of all three classes (both off: the entry points, state keys and table handling above, unchanged):

ema_decay=d keeps an exponential moving average of every parameter for evaluation, updated inside the step launch from
the new parameter it holds in registers: e = d e + (1 - d) p_new.  state[p]["ema"] is created as a clone of p when the
parameter's state is first made; `opt.ema_decay` is read at every step and travels by value (a warm-up schedule uploads
nothing).  `ema_parameters()` returns the shadows in parameter order and `with opt.swap_ema(): ...` exchanges every p.data
with its shadow and back, so `with opt.swap_ema(): evaluation.evaluate_streaming(...)` scores the averaged weights.
Only parameters are averaged: BatchNorm's running statistics are buffers and stay the live model's.

skip_nonfinite=True guards the step against a non-finite gradient: the sum-of-squares launch runs (with or without
max_grad_norm) and when its fp64 sum is NaN or an infinity the step writes no parameter, no state and no shadow
(zero_grads still zeroes the gradients).  `opt.skipped` is an int64 device counter of such steps (no host wait),
`opt.skipped_steps` reads it (waits for the device), `opt.last_grad_norm` holds the non-finite norm and
`opt.nonfinite_parameters()` names the tensors that caused it (from `opt.grad_norms()`, one fp64 norm per tensor of the
last step that formed the norm).  Gradients of 1e25 overflow an fp32 square but not the fp64 sum: no skip.
A deviation from torch's fused Adam, which keeps `step` on the device for this reason: Adam's per-parameter `step` counters
live on the host and advance on a skipped step too, so after k skipped steps the bias corrections run k steps ahead.
The one wait the guard can cost the native path: a step that initialises an SGD momentum buffer reads the counter back,
since the host must know whether the buffer was written.
"""
import contextlib
import ctypes
import math
import struct

import torch
from torch.optim import Optimizer

from . import _native

__all__ = ["RubiksSGD", "RubiksAdam", "RubiksAdamW", "MAX_GROUPS"]

MAX_GROUPS = 8           # RK_OPTIM_MAX_GROUPS
_FIRST_STEP = 1 << 8     # Job::group_flags
_ptr = torch.Tensor.data_ptr


class _SgdHyper(ctypes.Structure):       # rk_optim_sgd_hyper
    _fields_ = [("lr", ctypes.c_float), ("weight_decay", ctypes.c_float), ("momentum", ctypes.c_float),
                ("one_minus_dampening", ctypes.c_float), ("nesterov", ctypes.c_int)]


class _AdamHyper(ctypes.Structure):      # rk_optim_adam_hyper
    _fields_ = [(k, ctypes.c_float) for k in ("step_size", "weight_decay", "beta1", "one_minus_beta1", "beta2",
                                              "one_minus_beta2", "eps", "bc2_sqrt")]


class _AdamWHyper(ctypes.Structure):     # rk_optim_adamw_hyper
    _fields_ = [(k, ctypes.c_float) for k in ("step_size", "decay_factor", "beta1", "one_minus_beta1", "beta2",
                                              "one_minus_beta2", "eps", "bc2_sqrt")]


def chunk_partition(numels):
    """(chunk size, chunks in all, first chunk of every tensor) as the kernels cut `numels` (rk_debug_optim_chunks)."""
    n = len(numels)
    out = (ctypes.c_int * (n + 2))()
    _native.call("rk_debug_optim_chunks", (ctypes.c_longlong * n)(*numels), n, out)
    return out[0], out[1], list(out[2:])


class _Table:
    """The uploaded job table of one step geometry and what belongs to it."""
    __slots__ = ("key", "n", "chunks", "jobs", "host", "partials", "first_step", "device", "shape", "params", "offsets",
                 "chunk_tensor", "shadows")


class _RubiksOptimizer(Optimizer):
    _STATE_KEYS = ()

    _RULE = None                         # RK_OPTIM_RULE_* of rk_optim_step_ext_f32
    _ALWAYS_EXT = False                  # the rule has no entry point of its own

    def __init__(self, params, defaults, max_grad_norm, zero_grads, ema_decay=None, skip_nonfinite=False):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive or None, got %r" % (max_grad_norm,))
        if ema_decay is not None and not 0.0 <= float(ema_decay) <= 1.0:
            raise ValueError("ema_decay must lie in [0, 1] or be None, got %r" % (ema_decay,))
        defaults = dict(defaults, lr_mult=1.0, decay_mult=1.0)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        # zero_grads: the step stores 0 to every gradient it consumed (in the same launch on the native path), so a training
        # loop that accumulates into kept gradients needs no zero_grad(set_to_none=False) launch of its own
        self.zero_grads = bool(zero_grads)
        self.last_grad_norm = None       # 0-dim fp32 tensor on the parameters' device once a clipped / guarded step ran (no host wait)
        self.native_steps = 0
        self.torch_steps = 0
        self._table = None
        self._lib = None
        self._uninit = set()             # parameters whose momentum buffer is allocated but not yet written (RubiksSGD)
        self._steps_flat = None          # the host tensor behind every state[p]["step"] (RubiksAdam)
        self.ema_decay = None if ema_decay is None else float(ema_decay)     # read at every step
        self._ema = ema_decay is not None                                    # (whether state[p] holds "ema" is fixed here)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._ext = self._ALWAYS_EXT or self._ema or self.skip_nonfinite
        self._skipped = None             # the int64 device counter of skipped steps
        self._norm_src = None            # what grad_norms() reads: (table,) or (fp64 sums of squares, parameters)

    # ---- the guard's counter, the per-tensor norms, the EMA shadows ---------------------------------------------------
    def _counter(self, dev):
        if self._skipped is None or self._skipped.device != dev:
            old = 0 if self._skipped is None else int(self._skipped)
            self._skipped = torch.full((), old, dtype=torch.int64, device=dev)
        return self._skipped

    @property
    def skipped(self):
        """0-dim int64 tensor on the parameters' device: the steps the guard skipped (reading it here waits for nothing)."""
        for group in self.param_groups:
            for p in group["params"]:
                return self._counter(p.device)
        return self._counter(torch.device("cpu"))

    @property
    def skipped_steps(self):
        """The number of skipped steps as an int (waits for the device)."""
        return int(self.skipped)

    def grad_norms(self):
        """fp64 tensor on the parameters' device: ||g|| of every tensor that had a gradient in the last step that formed the
        norm (max_grad_norm or skip_nonfinite), in parameter order; the native path sums the step's per-chunk partials."""
        src = self._norm_src
        if src is None:
            raise RuntimeError("grad_norms() needs a step with max_grad_norm or skip_nonfinite")
        if len(src) == 2:
            return src[0].sqrt()
        table = src[0]
        if table.chunk_tensor is None:
            counts = torch.tensor(table.offsets[1:] + [table.chunks]) - torch.tensor(table.offsets)
            table.chunk_tensor = torch.repeat_interleave(torch.arange(table.n), counts).to(table.device)
        sq = torch.zeros(table.n, dtype=torch.float64, device=table.device)
        if table.chunks:
            sq.index_add_(0, table.chunk_tensor, table.partials[:table.chunks])
        return sq.sqrt()

    def nonfinite_parameters(self):
        """The parameters whose gradient norm of that step is NaN or an infinity (waits for the device)."""
        bad = (~torch.isfinite(self.grad_norms())).tolist()
        src = self._norm_src
        return [p for p, b in zip(src[1] if len(src) == 2 else src[0].params, bad) if b]

    def _ensure_ema(self, p):
        if self._ema and self.state[p].get("ema") is None:
            self.state[p]["ema"] = p.detach().clone(memory_format=torch.preserve_format)

    def ema_parameters(self):
        """The EMA shadows in parameter order (None where a parameter has not met a step yet)."""
        return [self.state[p].get("ema") if p in self.state else None for group in self.param_groups for p in group["params"]]

    @contextlib.contextmanager
    def swap_ema(self):
        """Exchanges every p.data with its shadow on entry and back on exit (pointers, no copy); the cached table is
        dropped both times.  BatchNorm's running statistics are buffers, not parameters: they stay the live model's."""
        def exchange():
            for group in self.param_groups:
                for p in group["params"]:
                    st = self.state.get(p)
                    if st is not None and st.get("ema") is not None:
                        p.data, st["ema"] = st["ema"], p.data
            self._table = None
        exchange()
        try:
            yield self
        finally:
            exchange()

    # ---- what invalidates the cached table besides a moved pointer ------------------------------------------------
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._table = None
        self._uninit = set()
        self._steps_flat = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._table = None
        self._steps_flat = None

    @staticmethod
    def _effective(group):
        return (float(group["lr"]) * float(group.get("lr_mult", 1.0)),
                float(group["weight_decay"]) * float(group.get("decay_mult", 1.0)))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # (p, g) addresses of every parameter with a gradient: what the uploaded table was built from
        key = [x for group in self.param_groups for p in group["params"] if (g := p.grad) is not None
               for x in (_ptr(p), _ptr(g))]
        if not key:
            return loss
        table = self._table
        if table is not None and self._ema and any(st.get("ema") is not e for st, e in table.shadows):
            table = None                 # a shadow was replaced by hand: its pointer is the table's too
        if table is None or table.key != key or table.shape != self._table_shape():
            work = [(gi, p) for gi, group in enumerate(self.param_groups) for p in group["params"] if p.grad is not None]
            table = self._table = self._build_table(work) if self._native_ok(work) else None
            if table is None:
                self._step_torch(work)   # (it creates and advances state on its own: the next native step starts afresh)
                self.torch_steps += 1
                return loss
        self._launch_table(table)
        self.native_steps += 1
        return loss

    # ---- native path ----------------------------------------------------------------------------------------------
    def _library(self):
        if self._lib is None:
            try:
                self._lib = _native.lib()
            except (RuntimeError, OSError, AttributeError):
                self._lib = False
        return self._lib

    def _native_ok(self, work):
        return len(self.param_groups) <= MAX_GROUPS and work[0][1].is_cuda and bool(self._library())

    def _launch_table(self, table):
        if self._ext:
            return self._launch_table_ext(table)
        hyper = self._hyper(table)
        L, dev = self._lib, table.device
        clip = self.max_grad_norm is not None
        if clip and (self.last_grad_norm is None or self.last_grad_norm.device != dev):
            self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
        if clip and table.partials is None:
            table.partials = torch.empty(max(table.chunks, 1), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if clip and table.chunks:
                _native.check(L.rk_optim_sqnorm_many_f32(table.jobs.data_ptr(), table.n, table.chunks,
                                                         table.partials.data_ptr(), stream), "rk_optim_sqnorm_many_f32")
            elif clip:
                self.last_grad_norm.zero_()
            _native.check(self._launch(L)(table.jobs.data_ptr(), table.n, table.chunks, hyper, len(self.param_groups),
                                          table.partials.data_ptr() if clip and table.chunks else None, table.chunks,
                                          self.max_grad_norm if clip else 0.0,
                                          self.last_grad_norm.data_ptr() if clip else None, int(self.zero_grads), stream),
                          self._ENTRY)
        if clip:
            self._norm_src = (table,)
        self._after_native(table)

    def _launch_table_ext(self, table):
        """rk_optim_step_ext_f32: the rule by number, the shadows' pointers behind the records, the guard's counter."""
        hyper = self._hyper(table)
        L, dev = self._lib, table.device
        clip, guard = self.max_grad_norm is not None, self.skip_nonfinite
        norm = clip or guard
        if norm and (self.last_grad_norm is None or self.last_grad_norm.device != dev):
            self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
        if norm and table.partials is None:
            table.partials = torch.empty(max(table.chunks, 1), dtype=torch.float64, device=dev)
        decay = float(self.ema_decay) if self._ema else 0.0
        counter = self._counter(dev) if guard else None
        first = guard and table.first_step and table.chunks
        seen = int(counter) if first else 0          # (a host wait, on steps that initialise a momentum buffer only)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if norm and table.chunks:
                _native.check(L.rk_optim_sqnorm_many_f32(table.jobs.data_ptr(), table.n, table.chunks,
                                                         table.partials.data_ptr(), stream), "rk_optim_sqnorm_many_f32")
            elif norm:
                self.last_grad_norm.zero_()
            _native.check(L.rk_optim_step_ext_f32(
                self._RULE, table.jobs.data_ptr(), table.n, table.chunks, hyper, len(self.param_groups),
                table.partials.data_ptr() if norm and table.chunks else None, table.chunks,
                self.max_grad_norm if clip else math.inf, self.last_grad_norm.data_ptr() if norm else None,
                int(self.zero_grads), table.jobs.data_ptr() + 48 * table.n if self._ema else None, decay, 1.0 - decay,
                int(guard), counter.data_ptr() if guard else None, stream), "rk_optim_step_ext_f32")
        if norm:
            self._norm_src = (table,)
        # a skipped step wrote no momentum buffer: the host has to know before it spends the records' first-step bits
        self._after_native(table, skipped=bool(first) and int(counter) != seen)

    def _build_table(self, work):
        """State for new parameters, then the records; None when a tensor is not the native path's to take."""
        dev = work[0][1].device
        for _, p in work:
            g = p.grad
            if not (p.device == dev and g.device == dev and p.dtype == torch.float32 and g.dtype == torch.float32
                    and g.layout == torch.strided and p.is_contiguous() and g.is_contiguous()):
                return None
        if not self._prepare_state(work):
            return None
        keys = self._STATE_KEYS
        if self._ema:
            keys = keys + ("ema",)
            for _, p in work:
                self._ensure_ema(p)
        for _, p in work:
            for k in keys:
                t = self.state[p].get(k)
                if t is not None and not (t.device == dev and t.dtype == torch.float32 and t.is_contiguous()
                                          and t.numel() == p.numel()):
                    return None
        table = _Table()
        table.device, table.n = dev, len(work)
        _, table.chunks, offsets = chunk_partition([p.numel() for _, p in work])
        recs, key, table.first_step = [], [], False
        for (gi, p), chunk0 in zip(work, offsets):
            st = self.state[p]
            ptrs = [st[k].data_ptr() if st.get(k) is not None else 0 for k in self._STATE_KEYS]
            first = self._first_step(gi, p)
            table.first_step |= first
            recs.append(struct.pack("<QQQQqii", p.data_ptr(), p.grad.data_ptr(), *(ptrs + [0, 0])[:2], p.numel(), chunk0,
                                    gi | (_FIRST_STEP if first else 0)))
            key += [p.data_ptr(), p.grad.data_ptr()]
        table.shadows = None
        if self._ema:                    # the shadows' pointers: n more 8-byte words behind the records, one upload
            table.shadows = [(self.state[p], self.state[p]["ema"]) for _, p in work]
            recs.append(struct.pack("<%dQ" % len(work), *(e.data_ptr() for _, e in table.shadows)))
        table.key, table.shape = key, self._table_shape()
        table.params, table.offsets, table.chunk_tensor = [p for _, p in work], list(offsets), None
        blob = b"".join(recs)
        table.host = torch.empty(len(blob), dtype=torch.uint8, pin_memory=True)
        table.host.copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
        table.jobs = torch.empty(len(blob), dtype=torch.uint8, device=dev)
        table.jobs.copy_(table.host, non_blocking=True)
        table.partials = None            # the clipping workspace: allocated by the first clipped step
        return table

    def _first_step(self, gi, p):
        return False

    def _table_shape(self):
        """What besides the pointers decides the records' contents (compared on every step)."""
        return None

    def _after_native(self, table, skipped=False):
        if table.first_step and not skipped:             # the records' first-step bits are spent
            self._table = None

    # ---- torch-op path: the same rule, any device and dtype -------------------------------------------------------
    def _step_torch(self, work):
        coef = self._clip_coef(work)
        if self.skip_nonfinite and not bool(torch.isfinite(self._norm_src[0].sum())):      # (waits for the device)
            self._counter(work[0][1].device).add_(1)
            self._skip_torch(work)
            if self.zero_grads:
                for _, p in work:
                    p.grad.zero_()
            return
        self._rule_torch(work, coef)

    def _skip_torch(self, work):
        pass

    def _ema_torch(self, p):
        """The shadow's update from the new p, in the kernel's order: two products, one sum."""
        if self._ema:
            decay = float(self.ema_decay)
            self.state[p]["ema"].mul_(decay).add_(p * (1.0 - decay))

    def _clip_coef(self, work):
        """min(1, max_norm / (norm + 1e-6)) with the norm summed in fp64, as the kernels form it; None without clipping
        (the guard alone forms the norm and scales nothing)."""
        if self.max_grad_norm is None and not self.skip_nonfinite:
            return None
        dev = work[0][1].device
        for _, p in work:
            if p.grad.is_sparse:
                raise RuntimeError("%s does not support sparse gradients" % type(self).__name__)
        each = torch.stack([p.grad.detach().double().pow(2).sum().to(dev) for _, p in work])
        self._norm_src = (each, [p for _, p in work])
        norm = each.sum().sqrt()
        self.last_grad_norm = norm.to(torch.float32)
        if self.max_grad_norm is None:
            return None
        return torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0)

    @staticmethod
    def _decayed_grad(p, coef, wd):
        g = p.grad
        gp = g * coef.to(device=g.device, dtype=g.dtype) if coef is not None else g
        return gp + wd * p if wd != 0.0 else gp


class RubiksSGD(_RubiksOptimizer):
    """torch.optim.SGD's rule (momentum, dampening, nesterov, L2 weight decay).  Per group: g' = coef g + wd p;
    buf = g' on a tensor's first step, else momentum buf + (1 - dampening) g'; p -= lr buf (nesterov: lr (g' + momentum buf)).
    momentum 0 keeps no buffer."""
    _STATE_KEYS = ("momentum_buffer",)
    _ENTRY = "rk_optim_sgd_many_f32"
    _RULE = 0

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, max_grad_norm=None,
                 zero_grads=False, ema_decay=None, skip_nonfinite=False):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("lr, momentum and weight_decay must not be negative")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov), max_grad_norm, zero_grads, ema_decay, skip_nonfinite)

    @staticmethod
    def _launch(L):
        return L.rk_optim_sgd_many_f32

    def _prepare_state(self, work):
        for gi, p in work:
            if self.param_groups[gi]["momentum"] != 0 and self.state[p].get("momentum_buffer") is None:
                self.state[p]["momentum_buffer"] = torch.empty_like(p)       # filled by its first step
                self._uninit.add(p)
        return True

    def _first_step(self, gi, p):
        return p in self._uninit

    def _table_shape(self):
        return [group["momentum"] != 0 for group in self.param_groups]     # (a record holds a buffer only where it is used)

    def _after_native(self, table, skipped=False):
        if table.first_step and not skipped:
            self._uninit.clear()         # (a table covers every parameter with a gradient, so every flagged one was written)
        super()._after_native(table, skipped)

    def _hyper(self, table):
        arr = (_SgdHyper * len(self.param_groups))()
        for h, group in zip(arr, self.param_groups):
            lr, wd = self._effective(group)
            h.lr, h.weight_decay, h.momentum = lr, wd, float(group["momentum"])
            h.one_minus_dampening, h.nesterov = 1.0 - float(group["dampening"]), int(bool(group["nesterov"]))
        return arr

    def _rule_torch(self, work, coef):
        for gi, p in work:
            group = self.param_groups[gi]
            lr, wd = self._effective(group)
            mu = float(group["momentum"])
            self._ensure_ema(p)
            gp = self._decayed_grad(p, coef, wd)
            if mu != 0.0:
                st = self.state[p]
                buf = st.get("momentum_buffer")
                if buf is None or p in self._uninit:
                    self._uninit.discard(p)
                    buf = st["momentum_buffer"] = gp.clone()
                else:
                    buf.mul_(mu).add_(gp * (1.0 - float(group["dampening"])))
                gp = gp + mu * buf if group["nesterov"] else buf
            p.sub_(lr * gp)
            self._ema_torch(p)
            if self.zero_grads:
                p.grad.zero_()


class RubiksAdam(_RubiksOptimizer):
    """torch.optim.Adam's rule (L2 weight decay, not AdamW; no amsgrad).  g' = coef g + wd p; m = beta1 m + (1 - beta1) g';
    v = beta2 v + (1 - beta2) g'^2; p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), the bias corrections evaluated on the
    host in double."""
    _STATE_KEYS = ("exp_avg", "exp_avg_sq")
    _ENTRY = "rk_optim_adam_many_f32"
    _RULE = 1
    _DECOUPLED = False
    _HYPER = _AdamHyper

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 zero_grads=False, ema_decay=None, skip_nonfinite=False):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), max_grad_norm,
                         zero_grads, ema_decay, skip_nonfinite)

    @staticmethod
    def _launch(L):
        return L.rk_optim_adam_many_f32

    @staticmethod
    def _new_state(st, p):
        st["step"] = torch.tensor(0.0, dtype=torch.float32)      # torch's layout: a 0-dim fp32 tensor on the host
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _prepare_state(self, work):
        """Creates missing state and homes every `step` counter in one host tensor (state[p]["step"] is a 0-dim view of it:
        torch's layout, advanced with ONE add per step instead of one per parameter).  The native path wants one step count
        per group, the bias corrections being per group; False otherwise."""
        flat = self._steps_flat
        if flat is None:
            params = [p for group in self.param_groups for p in group["params"]]
            flat = self._steps_flat = torch.zeros(len(params), dtype=torch.float32)
            self._slot = {id(p): i for i, p in enumerate(params)}
        home = flat.untyped_storage().data_ptr()
        self._group_steps, mask = {}, torch.zeros_like(flat)
        for gi, p in work:
            st, slot = self.state[p], self._slot[id(p)]
            if "step" not in st:
                self._new_state(st, p)
            s = st["step"]
            if not (torch.is_tensor(s) and not s.is_cuda and s.untyped_storage().data_ptr() == home):
                flat[slot] = float(s)    # (made by the torch path, or loaded: also a fused torch Adam's device counter)
                s = st["step"] = flat[slot]
            t = int(s)
            if self._group_steps.setdefault(gi, t) != t:
                return False
            mask[slot] = 1.0
        self._step_mask = mask
        return True

    def _hyper(self, table):
        arr = (self._HYPER * len(self.param_groups))()
        for gi, (h, group) in enumerate(zip(arr, self.param_groups)):
            lr, wd = self._effective(group)
            b1, b2 = (float(b) for b in group["betas"])
            t = self._group_steps.get(gi, 0) + 1
            h.step_size = lr / (1.0 - b1 ** t)
            if self._DECOUPLED:
                h.decay_factor = 1.0 - lr * wd       # in double, rounded once by the assignment
            else:
                h.weight_decay = wd
            h.beta1, h.one_minus_beta1, h.beta2, h.one_minus_beta2 = b1, 1.0 - b1, b2, 1.0 - b2
            h.eps, h.bc2_sqrt = float(group["eps"]), math.sqrt(1.0 - b2 ** t)
        return arr

    def _after_native(self, table, skipped=False):
        self._steps_flat.add_(self._step_mask)           # (on a skipped step too: the host does not wait to find out)
        for gi in self._group_steps:
            self._group_steps[gi] += 1
        super()._after_native(table)

    def _skip_torch(self, work):
        for _, p in work:                                # the counters advance as on the native path
            st = self.state[p]
            if "step" not in st:
                self._new_state(st, p)
            self._ensure_ema(p)
            st["step"] += 1

    def _rule_torch(self, work, coef):
        for gi, p in work:
            group = self.param_groups[gi]
            lr, wd = self._effective(group)
            b1, b2 = (float(b) for b in group["betas"])
            st = self.state[p]
            if "step" not in st:
                self._new_state(st, p)
            self._ensure_ema(p)
            st["step"] += 1
            t = float(st["step"])
            if self._DECOUPLED:
                p.mul_(1.0 - lr * wd)
                wd = 0.0
            gp = self._decayed_grad(p, coef, wd)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            m.mul_(b1).add_(gp * (1.0 - b1))
            v.mul_(b2).add_((gp * gp) * (1.0 - b2))
            p.sub_((lr / (1.0 - b1 ** t)) * (m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + float(group["eps"]))))
            self._ema_torch(p)
            if self.zero_grads:
                p.grad.zero_()


class RubiksAdamW(RubiksAdam):
    """torch.optim.AdamW's rule (decoupled weight decay; no amsgrad).  p1 = (1 - lr wd) p, the factor formed on the host in
    double; g' = coef g; m, v and the update as RubiksAdam, starting from p1.  State keys and layout are torch's: a
    state_dict() moves between this class and torch.optim.AdamW in both directions."""
    _ENTRY = "rk_optim_step_ext_f32"
    _RULE = 2
    _DECOUPLED = True
    _HYPER = _AdamWHyper
    _ALWAYS_EXT = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 zero_grads=False, ema_decay=None, skip_nonfinite=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                         zero_grads=zero_grads, ema_decay=ema_decay, skip_nonfinite=skip_nonfinite)
