"""The CPU oracle as torch.autograd.Functions -- the shift operators of RubiksNet on host tensors.

TEST INFRASTRUCTURE -- NOT PRODUCT CODE (the product has no CPU path: rubiksnet_amd raises on a CPU tensor).  Used by
tests/_host_reference.py (the fp64 host twin of a whole network: OracleShift3D, OracleShift2D and OracleTemporalShift3),
tests/test_dist_gloo.py (the data-parallel harness on CPU ranks) and by bench.py's cpu_baseline leg (the model-level CPU
column: RubiksNet-Tiny forward + backward on the host cores with this function plugged into every RubiksShift3D layer as
its `shift_function`).  Same argument list as rubiksnet/shiftlib/rubiks3d/primitive.py:193-215 (`rubiks_shift_3d`)."""
import torch

from . import attention_oracle
from . import oracle as orc


class OracleShift3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, shift, stride, padding, normalize_grad, normalize_t_factor, quantize):
        ctx.save_for_backward(x, shift)
        if normalize_t_factor == "auto":                     # primitive.py:206-210 (T / H of the input)
            normalize_t_factor = float(x.shape[1]) / float(x.shape[3])
        ctx.cfg = (stride, padding, normalize_grad, normalize_t_factor, quantize)
        return torch.from_numpy(orc.rk3d_forward(x.detach().contiguous().numpy(), shift.detach().contiguous().numpy(), stride, padding,
                                                 quantize))

    @staticmethod
    def backward(ctx, gy):
        x, shift = ctx.saved_tensors
        stride, padding, ng, tf, q = ctx.cfg
        gx, gs = orc.rk3d_backward(gy.contiguous().numpy(), x.detach().contiguous().numpy(), shift.detach().contiguous().numpy(), stride,
                                   padding, ng, tf, q)
        return torch.from_numpy(gx), torch.from_numpy(gs), None, None, None, None, None


class OracleShift2D(torch.autograd.Function):
    """RubiksShift2D on host tensors (float32 / float64): x [N, C, H, W], shift [2, C]; d(shift) always computed, as the
    module asks for it (L2-normalised when `normalize_grad`)."""

    @staticmethod
    def forward(ctx, x, shift, stride, padding, normalize_grad, quantize):
        ctx.save_for_backward(x, shift)
        ctx.cfg = (stride, padding, normalize_grad, quantize)
        return torch.from_numpy(orc.rk2d_forward(x.detach().contiguous().numpy(), shift.detach().contiguous().numpy(), stride,
                                                 padding, quantize))

    @staticmethod
    def backward(ctx, gy):
        x, shift = ctx.saved_tensors
        stride, padding, ng, q = ctx.cfg
        gx, gs = orc.rk2d_backward(gy.contiguous().numpy(), x.detach().contiguous().numpy(), shift.detach().contiguous().numpy(),
                                   stride, padding, ng, True, q)
        return torch.from_numpy(gx), torch.from_numpy(gs), None, None, None, None


class OracleTemporalShift3(torch.autograd.Function):
    """AttentionShift's 3-tap temporal filter on host tensors through oracle/attention_oracle.py: x [N*T, C, H, W] and
    already soft-maxed taps [C, 3] -> y; the tap sums of the backward are float64."""

    @staticmethod
    def forward(ctx, x, taps, n_segment):
        ctx.save_for_backward(x, taps)
        ctx.n_segment = n_segment
        return torch.from_numpy(attention_oracle.taps_forward(x.detach().contiguous().numpy(), taps.detach().numpy(), n_segment))

    @staticmethod
    def backward(ctx, gy):
        x, taps = ctx.saved_tensors
        gx, gtaps = attention_oracle.taps_backward(gy.contiguous().numpy(), x.detach().contiguous().numpy(),
                                                   taps.detach().numpy(), ctx.n_segment)
        return torch.from_numpy(gx), torch.from_numpy(gtaps).to(taps.dtype), None


def oracle_shift(x, shift, stride=1, padding=0, normalize_grad=True, normalize_t_factor=1.0, quantize=False):
    return OracleShift3D.apply(x, shift, stride, padding, normalize_grad, normalize_t_factor, quantize)


def plug_into(model):
    """Every RubiksShift3D layer of `model` evaluates through the oracle from now on (host tensors only).  Returns the count."""
    n = 0
    for m in model.modules():
        if type(m).__name__ == "RubiksShift3D" and hasattr(m, "shift_function"):
            m.shift_function = oracle_shift
            n += 1
    return n
