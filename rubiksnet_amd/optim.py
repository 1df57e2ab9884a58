"""RubiksSGD / RubiksAdam: torch.optim.SGD's and torch.optim.Adam's update rules with the whole network's step in ONE HIP
launch (rk_optim.hip), the `lr_mult` / `decay_mult` keys of `RubiksNetBackbone.get_optim_policy()` honoured, and optional
clipping by the global gradient norm (one more launch, no host wait).

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
"""
import ctypes
import math
import struct

import torch
from torch.optim import Optimizer

from . import _native

__all__ = ["RubiksSGD", "RubiksAdam", "MAX_GROUPS"]

MAX_GROUPS = 8           # RK_OPTIM_MAX_GROUPS
_FIRST_STEP = 1 << 8     # Job::group_flags
_ptr = torch.Tensor.data_ptr


class _SgdHyper(ctypes.Structure):       # rk_optim_sgd_hyper
    _fields_ = [("lr", ctypes.c_float), ("weight_decay", ctypes.c_float), ("momentum", ctypes.c_float),
                ("one_minus_dampening", ctypes.c_float), ("nesterov", ctypes.c_int)]


class _AdamHyper(ctypes.Structure):      # rk_optim_adam_hyper
    _fields_ = [(k, ctypes.c_float) for k in ("step_size", "weight_decay", "beta1", "one_minus_beta1", "beta2",
                                              "one_minus_beta2", "eps", "bc2_sqrt")]


def chunk_partition(numels):
    """(chunk size, chunks in all, first chunk of every tensor) as the kernels cut `numels` (rk_debug_optim_chunks)."""
    n = len(numels)
    out = (ctypes.c_int * (n + 2))()
    _native.check(_native.lib().rk_debug_optim_chunks((ctypes.c_longlong * n)(*numels), n, out), "rk_debug_optim_chunks")
    return out[0], out[1], list(out[2:])


class _Table:
    """The uploaded job table of one step geometry and what belongs to it."""
    __slots__ = ("key", "n", "chunks", "jobs", "host", "partials", "first_step", "device", "shape")


class _RubiksOptimizer(Optimizer):
    _STATE_KEYS = ()

    def __init__(self, params, defaults, max_grad_norm, zero_grads):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive or None, got %r" % (max_grad_norm,))
        defaults = dict(defaults, lr_mult=1.0, decay_mult=1.0)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        # zero_grads: the step stores 0 to every gradient it consumed (in the same launch on the native path), so a training
        # loop that accumulates into kept gradients needs no zero_grad(set_to_none=False) launch of its own
        self.zero_grads = bool(zero_grads)
        self.last_grad_norm = None       # 0-dim fp32 tensor on the parameters' device once a clipped step ran (no host wait)
        self.native_steps = 0
        self.torch_steps = 0
        self._table = None
        self._lib = None
        self._uninit = set()             # parameters whose momentum buffer is allocated but not yet written (RubiksSGD)
        self._steps_flat = None          # the host tensor behind every state[p]["step"] (RubiksAdam)

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
        self._after_native(table)

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
        for _, p in work:
            for k in self._STATE_KEYS:
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
        table.key, table.shape = key, self._table_shape()
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

    def _after_native(self, table):
        if table.first_step:             # the records' first-step bits are spent
            self._table = None

    # ---- torch-op path: the same rule, any device and dtype -------------------------------------------------------
    def _clip_coef(self, work):
        """min(1, max_norm / (norm + 1e-6)) with the norm summed in fp64, as the kernels form it; None without clipping."""
        if self.max_grad_norm is None:
            return None
        dev = work[0][1].device
        for _, p in work:
            if p.grad.is_sparse:
                raise RuntimeError("%s does not support sparse gradients" % type(self).__name__)
        sq = torch.stack([p.grad.detach().double().pow(2).sum().to(dev) for _, p in work]).sum()
        norm = sq.sqrt()
        self.last_grad_norm = norm.to(torch.float32)
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

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, max_grad_norm=None,
                 zero_grads=False):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("lr, momentum and weight_decay must not be negative")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov), max_grad_norm, zero_grads)

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

    def _after_native(self, table):
        if table.first_step:
            self._uninit.clear()         # (a table covers every parameter with a gradient, so every flagged one was written)
        super()._after_native(table)

    def _hyper(self, table):
        arr = (_SgdHyper * len(self.param_groups))()
        for h, group in zip(arr, self.param_groups):
            lr, wd = self._effective(group)
            h.lr, h.weight_decay, h.momentum = lr, wd, float(group["momentum"])
            h.one_minus_dampening, h.nesterov = 1.0 - float(group["dampening"]), int(bool(group["nesterov"]))
        return arr

    def _step_torch(self, work):
        coef = self._clip_coef(work)
        for gi, p in work:
            group = self.param_groups[gi]
            lr, wd = self._effective(group)
            mu = float(group["momentum"])
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
            if self.zero_grads:
                p.grad.zero_()


class RubiksAdam(_RubiksOptimizer):
    """torch.optim.Adam's rule (L2 weight decay, not AdamW; no amsgrad).  g' = coef g + wd p; m = beta1 m + (1 - beta1) g';
    v = beta2 v + (1 - beta2) g'^2; p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), the bias corrections evaluated on the
    host in double."""
    _STATE_KEYS = ("exp_avg", "exp_avg_sq")
    _ENTRY = "rk_optim_adam_many_f32"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 zero_grads=False):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), max_grad_norm,
                         zero_grads)

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
        arr = (_AdamHyper * len(self.param_groups))()
        for gi, (h, group) in enumerate(zip(arr, self.param_groups)):
            lr, wd = self._effective(group)
            b1, b2 = (float(b) for b in group["betas"])
            t = self._group_steps.get(gi, 0) + 1
            h.step_size, h.weight_decay = lr / (1.0 - b1 ** t), wd
            h.beta1, h.one_minus_beta1, h.beta2, h.one_minus_beta2 = b1, 1.0 - b1, b2, 1.0 - b2
            h.eps, h.bc2_sqrt = float(group["eps"]), math.sqrt(1.0 - b2 ** t)
        return arr

    def _after_native(self, table):
        self._steps_flat.add_(self._step_mask)
        for gi in self._group_steps:
            self._group_steps[gi] += 1
        super()._after_native(table)

    def _step_torch(self, work):
        coef = self._clip_coef(work)
        for gi, p in work:
            group = self.param_groups[gi]
            lr, wd = self._effective(group)
            b1, b2 = (float(b) for b in group["betas"])
            st = self.state[p]
            if "step" not in st:
                self._new_state(st, p)
            st["step"] += 1
            t = float(st["step"])
            gp = self._decayed_grad(p, coef, wd)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            m.mul_(b1).add_(gp * (1.0 - b1))
            v.mul_(b2).add_((gp * gp) * (1.0 - b2))
            p.sub_((lr / (1.0 - b1 ** t)) * (m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + float(group["eps"]))))
            if self.zero_grads:
                p.grad.zero_()
