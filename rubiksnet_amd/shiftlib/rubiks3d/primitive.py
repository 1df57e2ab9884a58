"""RubiksShift3D functional layer on top of the HIP library.

Counterpart of rubiksnet/shiftlib/rubiks3d/primitive.py:13-236 with the same public names
and signatures:

    rubiks_shift_3d_forward(x, shift, stride, padding, quantize=False, output=None)
    rubiks_shift_3d_backward(upstream_grad, x, shift, stride, padding, normalize_grad,
                             normalize_t_factor=1.0, quantize=False,
                             x_grad_output=None, shift_grad_output=None)
    rubiks_shift_3d(x, shift, stride=1, padding=0, normalize_grad=True,
                    normalize_t_factor=1.0, quantize=False)          # autograd-aware

x is [N, T, C, H, W] (NOT NCTHW), shift is [3, C] with rows (T, H, W).
"""
import torch

from rubiksnet_amd import _native, config, rubiksnet_cuda
from rubiksnet_amd.utils import allocate_output, make_tuple

__all__ = [
    "rubiks_shift_3d_forward",
    "rubiks_shift_3d_backward",
    "rubiks_shift_3d",
]

_DIM = 3


def _per_axis(value, naxes=_DIM):
    """One integer per moving axis: a bare int applies to all of them."""
    return make_tuple(value, naxes)


def compute_output_shape(x, stride, padding, shift_dim=_DIM):
    """Shape of the shifted tensor for x [N, T, C, H, W].

    The last `shift_dim` of the three (T, H, W) axes move -- 3: all of them, 2: (H, W), 1: T alone,
    which is how the reference numbers them (rubiks3d/primitive.py:29-48).  A moving axis of length L
    comes out `(L + 2*pad - 1) // stride + 1` long: that is `rk_out_len`, the library's own rule
    (cuda_src/rubiks.cpp:166), so Python and the kernels cannot disagree.
    """
    if shift_dim not in (1, 2, 3):
        raise NotImplementedError("only 1D, 2D, 3D shifts supported")
    n, t, c, h, w = (int(v) for v in x.size())
    lengths = {"t": t, "h": h, "w": w}
    moving = {1: "t", 2: "hw", 3: "thw"}[shift_dim]
    out_len = _native.lib().rk_out_len
    for axis, s, p in zip(moving, _per_axis(stride, shift_dim), _per_axis(padding, shift_dim)):
        lengths[axis] = int(out_len(lengths[axis], s, p))
    return n, lengths["t"], c, lengths["h"], lengths["w"]


def _pick(x, f32, f64):
    if x.dtype == torch.float32:
        return f32
    if x.dtype == torch.float64:
        return f64
    raise ValueError("rubiks_shift_{}d only supports float32 and float64 (double) dtypes.".format(_DIM))


def rubiks_shift_3d_forward(x, shift, stride, padding, quantize=False, output=None):
    """Pure forward primitive, no autograd (rubiks3d/primitive.py:54-80)."""
    strides = _per_axis(stride)
    paddings = _per_axis(padding)
    assert x.is_cuda, "rubiks shift only works on CUDA tensors"
    assert x.size(2) == shift.size(1), "x tensor channel dim[2] must match shift channel dim[1]"
    assert x.dtype == shift.dtype, "x and shift must have the same dtype"
    func = _pick(x, rubiksnet_cuda.rubiks_shift_3d_forward_float, rubiksnet_cuda.rubiks_shift_3d_forward_double)
    out_shape = compute_output_shape(x, strides, paddings, shift_dim=_DIM)
    # the 3D kernels write every output element, so a fresh buffer need not be zeroed
    output = allocate_output(output, x, out_shape, zero=False)
    ret = func(x.contiguous(), shift.contiguous(), strides, paddings, quantize, output)
    assert ret == 0, "HIP kernel return code {} != 0, error".format(ret)
    return output


def rubiks_shift_3d_backward(
    upstream_grad,
    x,
    shift,
    stride,
    padding,
    normalize_grad,
    normalize_t_factor=1.0,
    quantize=False,
    x_grad_output=None,
    shift_grad_output=None,
    need_x_grad=True,
    need_shift_grad=True,
):
    """Pure backward primitive (rubiks3d/primitive.py:90-140): returns (x_grad, shift_grad).

    `need_x_grad` / `need_shift_grad` are additions: the reference always computes both;
    a skipped half comes back as None.
    """
    strides = _per_axis(stride)
    paddings = _per_axis(padding)
    assert x.is_cuda and upstream_grad.is_cuda, "rubiks shift only works on CUDA tensors"
    func = _pick(x, rubiksnet_cuda.rubiks_shift_3d_backward_float, rubiksnet_cuda.rubiks_shift_3d_backward_double)
    x_grad = allocate_output(x_grad_output, x, x.size(), zero=False) if need_x_grad else None
    shift_grad = allocate_output(shift_grad_output, shift, shift.size(), zero=False) if need_shift_grad else None
    # the reference hands a non-contiguous upstream grad to raw-pointer kernels unchecked
    # (SURVEY 3.2); make it dense instead of misreading it
    ret = func(
        x.contiguous(),
        shift.contiguous(),
        upstream_grad.contiguous(),
        strides,
        paddings,
        x_grad,
        shift_grad,
        normalize_grad,
        normalize_t_factor,
        quantize,
    )
    assert ret == 0, "HIP return code {} != 0, error".format(ret)
    return x_grad, shift_grad


class RubiksShift3DFunc(torch.autograd.Function):
    """autograd wiring, 7 inputs -> grads for the first two (rubiks3d/primitive.py:146-188)."""

    @staticmethod
    def forward(ctx, x, shift, stride, padding, normalize_grad, normalize_t_factor, quantize):
        assert isinstance(normalize_grad, bool)
        ctx.stride = stride
        ctx.padding = padding
        ctx.normalize_grad = normalize_grad
        ctx.normalize_t_factor = normalize_t_factor
        ctx.quantize = quantize
        ctx.save_for_backward(x, shift)
        return rubiks_shift_3d_forward(x, shift, stride, padding, quantize=quantize)

    @staticmethod
    def backward(ctx, grad_output):
        x, shift = ctx.saved_tensors
        x_grad = shift_grad = None
        if any(ctx.needs_input_grad):
            x_grad, shift_grad = rubiks_shift_3d_backward(
                grad_output,
                x,
                shift,
                stride=ctx.stride,
                padding=ctx.padding,
                normalize_grad=ctx.normalize_grad,
                normalize_t_factor=ctx.normalize_t_factor,
                quantize=ctx.quantize,
                need_x_grad=ctx.needs_input_grad[0],
                need_shift_grad=ctx.needs_input_grad[1],
            )
        return x_grad, shift_grad, None, None, None, None, None


class RubiksShift3D16Func(torch.autograd.Function):
    """The same node on 16-bit activations next to an fp32 shift (rubiksnet_cuda.rubiks_shift_3d_*_sf32): saves the 16-bit
    x and the fp32 shift, returns d(x) in x's dtype and d(shift) in fp32."""

    @staticmethod
    def forward(ctx, x, shift, stride, padding, normalize_grad, normalize_t_factor, quantize):
        assert isinstance(normalize_grad, bool)
        ctx.stride = _per_axis(stride)
        ctx.padding = _per_axis(padding)
        ctx.normalize_grad = normalize_grad
        ctx.normalize_t_factor = normalize_t_factor
        ctx.quantize = quantize
        x = x.contiguous()
        shift = shift.contiguous()
        ctx.save_for_backward(x, shift)
        y = x.new_empty(compute_output_shape(x, ctx.stride, ctx.padding, shift_dim=_DIM))
        rubiksnet_cuda.rubiks_shift_3d_forward_sf32(x, shift, ctx.stride, ctx.padding, quantize, y)
        return y

    @staticmethod
    def backward(ctx, grad_output):
        x, shift = ctx.saved_tensors
        x_grad = shift_grad = None
        if any(ctx.needs_input_grad[:2]):
            x_grad = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            shift_grad = torch.empty_like(shift) if ctx.needs_input_grad[1] else None
            rubiksnet_cuda.rubiks_shift_3d_backward_sf32(
                x, shift, grad_output.contiguous(), ctx.stride, ctx.padding, x_grad, shift_grad, ctx.normalize_grad,
                ctx.normalize_t_factor, ctx.quantize)
        return x_grad, shift_grad, None, None, None, None, None


def _native16(x, shift, stride, padding, quantize):
    """True when the 16-bit kernels take this call: bf16 / f16 activations next to an fp32 shift, RK_SHIFT3D_16 on, and a
    configuration of one of the streaming 16-bit families, stride 1 or stride (1,2,2) (rk3d_sf32_streams) -- the ones
    measured faster than the cast path."""
    if shift.dtype != torch.float32 or not x.is_cuda or not config.switches().shift3d_16:
        return False
    if x.numel() == 0:
        return False
    dims = [int(v) for v in x.size()] + list(_per_axis(stride)) + list(_per_axis(padding))
    return _native.lib().rk3d_sf32_streams(*dims, int(bool(quantize)), 2) == 1


def rubiks_shift_3d(x, shift, stride=1, padding=0, normalize_grad=True, normalize_t_factor=1.0, quantize=False):
    """User-facing functional (rubiks3d/primitive.py:193-215)."""
    assert len(x.size()) == 5, "x must be [N, T, C, H, W]"
    _, T, C, H, _ = x.size()
    assert C == shift.size(1), "group shift is deprecated. Now C dim must match."
    if normalize_t_factor == "auto":
        normalize_t_factor = T / H
    else:
        assert isinstance(normalize_t_factor, (int, float))
    if x.dtype in (torch.float16, torch.bfloat16):
        if _native16(x, shift, stride, padding, quantize):
            return RubiksShift3D16Func.apply(x, shift, stride, padding, normalize_grad, normalize_t_factor, quantize)
        # autocast hands half activations to an fp32 parameter.  The reference's 3D op exists in fp32/fp64 only
        # (primitive.py:66-75): run it in fp32 and hand back the caller's dtype (the explicit-dtype primitives
        # below still raise for half inputs, as the reference does).
        y = RubiksShift3DFunc.apply(x.float(), shift.float(), stride, padding, normalize_grad, normalize_t_factor,
                                    quantize)
        return y.to(x.dtype)
    return RubiksShift3DFunc.apply(x, shift, stride, padding, normalize_grad, normalize_t_factor, quantize)
