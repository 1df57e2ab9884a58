"""StreamMeter: loss, top-k and per-class accuracy of a run, accumulated ON THE DEVICE and read once, at the end.

    meter = StreamMeter(174, topk=(1, 5), views=3)
    for data, label in loader:
        meter.update(model(fold_views(data, 8, 3)), label)       # one launch, no host wait
    print(meter.result())                                        # the single host read

update() scores a batch in ONE HIP launch (rk_metrics.hip; the rules are written out in include/rubiks_hip.h): the mean
of a video's `views` rows of logits (the reference's `.mean(1)`), the rank of the label in it -- hence top-k for any k,
ties counted against the label as `rank = #{z > z[y]} + #{j < y : z[j] == z[y]}` --, the cross-entropy, per-class counts and
hits and, optionally, the confusion matrix.  Everything lands in one int64 tensor, `state`, added with integer atomics:

    [0] videos   [1] loss sum, unit 2^-32   [2] nonfinite   [3] bad_labels   [4..8) hits per k of `topk`
    [8..8+K) videos per label   [8+K..8+2K) top-1 hits per label   [8+2K..8+2K+K*K) confusion[label][pred]

so two meters merge by adding their states and the ranks of a job with one all_reduce(SUM), bit for bit whatever the order.
A label outside [0, K) counts in `bad_labels` only; a video with a NaN or an infinity in its mean logits counts as a video of
its class and a miss at every k (`nonfinite`), and adds nothing to the loss or the confusion matrix.

The native path takes CUDA logits in fp32 / bf16 / fp16.  CPU tensors, another dtype (computed in fp32) and a box without the
built library run the same rules written with torch ops, on the same state layout, with the loss in fp32 by the kernel's
formula and the same fixed point: states of the two paths merge.  `native_updates` / `torch_updates` count which path
each update took.
"""
import torch

from . import _native

__all__ = ["StreamMeter", "HEAD_WORDS", "MAX_TOPK", "MAX_VIEWS", "MAX_CLASSES", "OUTPUTS"]

HEAD_WORDS = 8           # RK_METRICS_HEAD_WORDS
MAX_TOPK = 4             # RK_METRICS_MAX_TOPK
MAX_VIEWS = 64           # RK_METRICS_MAX_VIEWS
MAX_CLASSES = 65536      # RK_METRICS_MAX_CLASSES
OUTPUTS = ("consensus", "pred", "rank", "loss")
_LOSS_UNIT = float(1 << 32)
_LOSS_MAX = float(1 << 20)
_NATIVE = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}


class StreamMeter:
    def __init__(self, num_classes, topk=(1, 5), views=1, confusion=True):
        topk = tuple(int(k) for k in topk)
        if not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError("num_classes must be in [1, %d], got %r" % (MAX_CLASSES, num_classes))
        if not 1 <= int(views) <= MAX_VIEWS:
            raise ValueError("views must be in [1, %d], got %r" % (MAX_VIEWS, views))
        if len(topk) > MAX_TOPK or any(k < 1 for k in topk) or len(set(topk)) != len(topk):
            raise ValueError("topk: at most %d distinct values, each >= 1, got %r" % (MAX_TOPK, topk))
        self.num_classes, self.views, self.topk, self.confusion = int(num_classes), int(views), topk, bool(confusion)
        self.native = True               # False: the torch-op path for CUDA tensors too
        self.native_updates = 0
        self.torch_updates = 0
        self._state = None
        self._lib = None

    # ---- the state --------------------------------------------------------------------------------------------------
    @property
    def words(self):
        K = self.num_classes
        return HEAD_WORDS + 2 * K + (K * K if self.confusion else 0)

    @property
    def state(self):
        """The int64 tensor (None until the first update, merge or all_reduce put it on a device)."""
        return self._state

    @state.setter
    def state(self, tensor):
        """Adopts `tensor` as the state (a restored one, or a caller's slice of a larger buffer): it is used in place."""
        if not (torch.is_tensor(tensor) and tensor.dtype == torch.int64 and tensor.dim() == 1
                and tensor.numel() == self.words and tensor.is_contiguous()):
            raise ValueError("the state is a contiguous int64 tensor of %d words" % self.words)
        self._state = tensor

    def _state_on(self, device):
        if self._state is None:
            self._state = torch.zeros(self.words, dtype=torch.int64, device=device)
        elif self._state.device != device:
            raise ValueError("this meter's state is on %s, the update on %s" % (self._state.device, device))
        return self._state

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    def _same_shape(self, other):
        if (self.num_classes, self.views, self.topk, self.confusion) != (other.num_classes, other.views, other.topk,
                                                                         other.confusion):
            raise ValueError("meters of different configurations do not merge")

    def merge(self, other):
        """Adds `other`'s state to this one (no host wait)."""
        self._same_shape(other)
        if other._state is not None:
            state = self._state_on(other._state.device if self._state is None else self._state.device)
            state.add_(other._state.to(state.device, non_blocking=True))
        return self

    def all_reduce(self, group=None, device=None):
        """Sums the states of every rank of `group` into each (one collective).  A rank that has seen no batch yet joins with
        zeros, on `device` (default: the current CUDA device under an NCCL group, else the CPU)."""
        import torch.distributed as dist
        if self._state is None:
            if device is None:
                device = (torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl"
                          else torch.device("cpu"))
            self._state_on(torch.device(device))
        dist.all_reduce(self._state, op=dist.ReduceOp.SUM, group=group)
        return self

    # ---- one batch --------------------------------------------------------------------------------------------------
    def update(self, logits, labels, outputs=()):
        """logits [B * views, K] or [B, views, K], labels [B].  Enqueues on the current stream and never waits on the host.
        outputs: names out of ("consensus", "pred", "rank", "loss"); returns a dict of those per-video tensors
        (consensus fp32 [B, K]; pred, rank int32 and loss fp32 [B]; rank -1 and loss NaN for a video with a bad label or
        non-finite logits, pred -1 for the latter)."""
        K, V = self.num_classes, self.views
        outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
        for name in outputs:
            if name not in OUTPUTS:
                raise ValueError("outputs are out of %r, got %r" % (OUTPUTS, name))
        if logits.dim() == 3:
            if logits.size(1) != V:
                raise ValueError("logits [B, views, K] with %d views, the meter has %d" % (logits.size(1), V))
            logits = logits.reshape(-1, logits.size(2))
        if logits.dim() != 2 or logits.size(1) != K or logits.size(0) % V:
            raise ValueError("logits must be [B * %d, %d] or [B, %d, %d], got %r" % (V, K, V, K, tuple(logits.shape)))
        B = logits.size(0) // V
        if labels.numel() != B:
            raise ValueError("%d labels for %d videos" % (labels.numel(), B))
        dev = logits.device
        logits = logits.detach().contiguous()
        labels = labels.detach().reshape(-1).to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
        state = self._state_on(dev)
        if B == 0:
            z = torch.empty(0, K, dtype=torch.float32, device=dev)
            empty = {"consensus": z, "pred": z.new_empty(0, dtype=torch.int32), "rank": z.new_empty(0, dtype=torch.int32),
                     "loss": z.new_empty(0)}
            return {name: empty[name] for name in outputs}
        if self.native and dev.type == "cuda" and logits.dtype in _NATIVE and self._library():
            out = self._update_native(logits, labels, state, B, outputs)
            self.native_updates += 1
        else:
            out = self._update_torch(logits, labels, state, B)
            self.torch_updates += 1
        return {name: out[name] for name in outputs}

    def _library(self):
        if self._lib is None:
            try:
                self._lib = _native.lib()
            except (RuntimeError, OSError, AttributeError):
                self._lib = False
        return self._lib

    def _update_native(self, logits, labels, state, B, outputs):
        K, dev = self.num_classes, logits.device
        out = {}
        if "consensus" in outputs:
            out["consensus"] = torch.empty(B, K, dtype=torch.float32, device=dev)
        for name in ("pred", "rank"):
            if name in outputs:
                out[name] = torch.empty(B, dtype=torch.int32, device=dev)
        if "loss" in outputs:
            out["loss"] = torch.empty(B, dtype=torch.float32, device=dev)
        entry = "rk_metrics_update_" + _NATIVE[logits.dtype]
        ks = (self.topk + (1,) * MAX_TOPK)[:MAX_TOPK]
        _native.launch(entry, dev, logits.data_ptr(), labels.data_ptr(), state.data_ptr(), B, self.views, K, int(self.confusion),
                       len(self.topk), *ks, *(_native.ptr(out.get(name)) for name in OUTPUTS))
        return out

    def _update_torch(self, logits, labels, state, B):
        """The kernel's rules in torch ops (fp32, the same order of operations), on any device; no host wait."""
        K, V, dev = self.num_classes, self.views, logits.device
        x = logits.view(B, V, K)
        acc = x[:, 0].float()
        for v in range(1, V):
            acc = acc + x[:, v].float()
        z = acc / torch.full((1, 1), float(V), dtype=torch.float32, device=dev)      # (a tensor divisor: one true division)
        ar = torch.arange(K, device=dev)
        valid = (labels >= 0) & (labels < K)
        finite = torch.isfinite(z).all(1)
        ok = valid & finite
        y = labels.clamp(0, K - 1)
        m = z.max(1, keepdim=True).values
        zy = z.gather(1, y[:, None])
        pred = torch.where(z == m, ar, K).min(1).values.clamp(max=K - 1)
        rank = ((z > zy) | ((z == zy) & (ar < y[:, None]))).sum(1)
        loss = ((m[:, 0] + torch.log(torch.exp(z - m).sum(1))) - zy[:, 0]).clamp(0.0, _LOSS_MAX)
        fixed = torch.where(ok, torch.round(loss.double() * _LOSS_UNIT), 0.0).to(torch.int64)
        head = [valid.sum(), fixed.sum(), (valid & ~finite).sum(), (~valid).sum()]
        head += [(ok & (rank < k)).sum() for k in self.topk]
        state[:len(head)] += torch.stack(head)
        state[HEAD_WORDS:HEAD_WORDS + K].index_add_(0, y, valid.to(torch.int64))
        state[HEAD_WORDS + K:HEAD_WORDS + 2 * K].index_add_(0, y, (ok & (rank == 0)).to(torch.int64))
        if self.confusion:
            state[HEAD_WORDS + 2 * K:].index_add_(0, y * K + pred, ok.to(torch.int64))
        return {"consensus": z, "pred": torch.where(finite, pred, -1).to(torch.int32),
                "rank": torch.where(ok, rank, -1).to(torch.int32),
                "loss": torch.where(ok, loss, float("nan"))}

    # ---- the single host read ---------------------------------------------------------------------------------------
    def result(self):
        """dict(videos, loss: mean over the finite videos, top{k} in percent for every k of `topk`, per_class_acc [K] fp64
        (NaN where a class was never seen), mean_class_acc over the classes seen (the reference's diag / row-sum mean),
        confusion [K, K] int64 or None, nonfinite, bad_labels).  NaN where nothing was counted."""
        K = self.num_classes
        s = torch.zeros(self.words, dtype=torch.int64) if self._state is None else self._state.cpu()
        videos, fixed, nonfinite, bad = (int(v) for v in s[:4])
        nan = float("nan")
        out = {"videos": videos, "loss": fixed / _LOSS_UNIT / (videos - nonfinite) if videos > nonfinite else nan}
        for slot, k in enumerate(self.topk):
            out["top%d" % k] = 100.0 * int(s[4 + slot]) / videos if videos else nan
        count = s[HEAD_WORDS:HEAD_WORDS + K].double()
        hits = s[HEAD_WORDS + K:HEAD_WORDS + 2 * K].double()
        seen = count > 0
        per_class = torch.where(seen, hits / count.clamp(min=1.0), torch.full_like(count, nan))
        out["per_class_acc"] = per_class
        out["mean_class_acc"] = float(per_class[seen].mean()) if bool(seen.any()) else nan
        out["confusion"] = s[HEAD_WORDS + 2 * K:].view(K, K).clone() if self.confusion else None
        out["nonfinite"], out["bad_labels"] = nonfinite, bad
        return out
