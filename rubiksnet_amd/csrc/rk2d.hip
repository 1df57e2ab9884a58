// rk2d.hip -- RubiksShift2D for gfx950: kernels + C-ABI entry points (include/rubiks_hip.h).
//
// Semantics follow the reference's K6-K9 (cuda_src/rubiks2d_kernels.cu:94-397) and its
// host glue (cuda_src/rubiks.cpp:44-155).  Layout [N,C,H,W], shift [2,C] = (H,W).
// Same mapping idea as rk3d_generic.hpp: one (n, c) plane per group of E = 64/128/256
// threads, per-channel quantities hoisted, no per-element division, no float atomics:
// d(shift) goes wave-shuffle -> LDS -> one partial per plane -> fixed-order fp64 finalize.
// f16 / bf16 tensors are computed in fp32 and rounded once on store; only the quantize
// position arithmetic is done in the storage type, because it decides WHICH element is
// gathered (the reference instantiates the whole kernel at c10::Half).
#include "rk2d_plan.hpp"

using namespace rk;
using namespace rk::g2d;
using namespace rk::plan2d;

namespace {

int make_dims2(Dims2& d, int N, int C, int H, int W, int sH, int sW, int pH, int pW) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return RK_ERR_BAD_DIMS;
    if (sH <= 0 || sW <= 0 || pH < 0 || pW < 0) return RK_ERR_BAD_STRIDE;
    d.N = N; d.C = C; d.H = H; d.W = W; d.sH = sH; d.sW = sW; d.pH = pH; d.pW = pW;
    d.Ho = out_len(H, sH, pH); d.Wo = out_len(W, sW, pW);
    if (d.Ho <= 0 || d.Wo <= 0) return RK_ERR_BAD_DIMS;
    // the reference's accessors index with uint32 (utils_cuda.h:12-13)
    if ((long long)N * C * H * W > 0x7fffffffLL || (long long)N * C * d.Ho * d.Wo > 0x7fffffffLL)
        return RK_ERR_BAD_DIMS;
    return RK_OK;
}

// the process's RK_SHIFT_KERNELS (rk_common.hpp), read once, and the current device's compute units
Switches env_switches() { return Switches{shift_kernels(), device_cus()}; }
// the shape-only answers (workspace sizes, rk2d_bn_fused_shape) make no device call: the CU count moves the frames per wave
// of the 16-bit 14x14 backward (rk2d_tile.hpp), never eligibility, and the workspace bound is taken at the least frames per wave
Switches shape_switches() { return Switches{shift_kernels(), 256}; }
// what plan2d::Call::align holds for an operand
int al(const void* p) { return ((uintptr_t)p & 15) == 0 ? 16 : ((uintptr_t)p & 7) == 0 ? 8 : 0; }

// the operands of a call, by the names the launchers use.  T: storage type of the activations; S: storage type of the shift
// table and of d(shift).  S == T is the reference's instantiation (the whole kernel at one scalar type,
// rubiks2d_kernels.cu:422); S = float next to 16-bit activations keeps the fp32 parameter of an autocast network un-rounded
// (and returns d(shift) in fp32).
template <typename T, typename S> struct Ops {
    const T* x; const S* shift; const T* gy; T* y; T* gx; S* gshift; void* ws;
    int normalize;
    const float* ab;              // the BN forward's [2][C]
    dma2d::BnFuse2 bn;            // the BN backward's pack and outputs
};

// runs one planned launch
template <typename T, typename S>
void run(const Launch& l, const Dims2& d, int P, const Ops<T, S>& o, hipStream_t stream) {
    using CT = typename Compute<T>::type;
    const Cfg2& c = l.c;
    const T* src = c.negate ? o.gy : o.x;                              // forward / d(x)-only families
    T* dst = c.negate ? o.gx : o.y;
    const dim3 grid(c.grid), block(kBlock);
    if constexpr (!std::is_same<T, double>::value) {                   // the streaming families; a fused backward's finalizers
        const bool fused = l.family == kDmaBwd || l.family == kStageBwd || l.family == kRawBwd || l.family == kTileBwd;
        const dma2d::Fin2<S> fin = fused ? dma2d::make_fin2(o.ws, (int)c.grid - d.C, o.gshift, o.normalize) : dma2d::Fin2<S>{};
        if (l.family == kTileInterp) return tile2d::launch_interp(c, l.g.tile, src, o.shift, dst, o.ab, stream);
        if (l.family == kTileBwd) return tile2d::launch_backward(c, l.g.tile, o.gy, o.x, o.shift, o.gx, fin, o.bn, stream);
        if constexpr (std::is_same<T, float>::value) {
            if (l.family == kDmaInterp) return dma2d::launch_interp(c, l.g.band, src, o.shift, dst, stream);
            if (l.family == kDmaBwd) return dma2d::launch_backward(c, l.g.band, d, o.gy, o.x, o.shift, o.gx, fin, stream);
        } else {
            if (l.family == kRawInterp) return raw16::launch_interp(c, l.g.band, src, o.shift, dst, o.ab, stream);
            if (l.family == kRawBwd) return raw16::launch_backward(c, l.g.band, o.gy, o.x, o.shift, o.gx, fin, o.bn, stream);
            if (l.family == kStageInterp) return stage2d::launch_interp(c, l.g.band, src, o.shift, dst, o.ab, stream);
            if (l.family == kStageBwd) return stage2d::launch_backward(c, l.g.band, d, o.gy, o.x, o.shift, o.gx, fin, o.bn, stream);
        }
    }
    switch (l.family) {
        case kColFwd: return col2d::launch_forward(c, l.g.col, o.x, o.shift, o.y, o.ab, stream);
        case kColBwd: return col2d::launch_backward(c, l.g.col, o.gy, o.x, o.shift, o.gx, (CT*)o.ws, o.bn.abmi, stream);
        case kGenFwd:
            if (c.quant) hipLaunchKernelGGL((k2d_forward<T, S, true>), grid, block, 0, stream, o.x, o.shift, o.y, l.g.gen);
            else hipLaunchKernelGGL((k2d_forward<T, S, false>), grid, block, 0, stream, o.x, o.shift, o.y, l.g.gen);
            return;
        case kGenBwdX:
            if (c.quant) hipLaunchKernelGGL((k2d_backward_input<T, S, true>), grid, block, 0, stream, o.gy, o.shift, o.gx, l.g.gen);
            else hipLaunchKernelGGL((k2d_backward_input<T, S, false>), grid, block, 0, stream, o.gy, o.shift, o.gx, l.g.gen);
            return;
        case kGenBwdS:
            hipLaunchKernelGGL((k2d_backward_shift<T, S>), grid, block, 0, stream, o.gy, o.x, o.shift, (CT*)o.ws, l.g.gen);
            return;
        case kFinalize:
            hipLaunchKernelGGL((k2d_finalize<T, S>), grid, dim3(finalize_block(P)), 0, stream, (const CT*)o.ws, o.gshift, d.C, P,
                               o.normalize);
            return;
        case kFinalizeBn:
            if constexpr (kBnVariant<T, S>)
                hipLaunchKernelGGL(col2d::k2d_finalize_bn, grid, dim3(finalize_block(P)), 0, stream, (const float*)o.ws, o.gshift,
                                   o.bn.k12, o.bn.dgamma, o.bn.dbeta, d.C, P, o.normalize, o.bn.inv_count);
            return;
        default: return;
    }
}
template <typename T, typename S>
int run(const Call& c, const Ops<T, S>& o, rk_stream_t stream) {
    const Plan pl = plan(c, env_switches());
    if (pl.rc) return pl.rc;
    for (int i = 0; i < pl.n; ++i) run<T, S>(pl.l[i], c.d, pl.P, o, (hipStream_t)stream);
    return launch_status();
}

template <typename T, typename S>
int forward2(const void* x, const void* shift, void* y, int N, int C, int H, int W, int sH, int sW, int pH, int pW, int quantize,
             rk_stream_t stream) {
    if (!x || !shift || !y) return RK_ERR_NULL_POINTER;
    Call c{};
    if (int rc = make_dims2(c.d, N, C, H, W, sH, sW, pH, pW)) return rc;
    c.form = kForward; c.elem = (int)sizeof(T); c.quantize = quantize;
    c.align[kX] = al(x); c.align[kY] = al(y); c.align[kGx] = c.align[kBn] = 16;
    Ops<T, S> o{};
    o.x = (const T*)x; o.shift = (const S*)shift; o.y = (T*)y;
    return run(c, o, stream);
}

template <typename T, typename S>
int backward2(const void* gy, const void* x, const void* shift, void* gx, void* gshift, int N, int C, int H, int W, int sH, int sW,
              int pH, int pW, int normalize_grad, int enable_shift_grad, int quantize, void* ws, size_t ws_bytes,
              rk_stream_t stream) {
    if (!gy || !shift || !gx) return RK_ERR_NULL_POINTER;
    if (enable_shift_grad && (!x || !gshift)) return RK_ERR_NULL_POINTER;
    Call c{};
    if (int rc = make_dims2(c.d, N, C, H, W, sH, sW, pH, pW)) return rc;
    if (enable_shift_grad && (!ws || ws_bytes < workspace_bytes(c.d, shape_switches()))) return RK_ERR_WORKSPACE;
    c.form = kBackward; c.elem = (int)sizeof(T); c.quantize = quantize; c.gshift = enable_shift_grad;
    c.align[kX] = al(x); c.align[kY] = al(gy); c.align[kGx] = al(gx); c.align[kBn] = 16;
    Ops<T, S> o{};
    o.gy = (const T*)gy; o.x = (const T*)x; o.shift = (const S*)shift; o.gx = (T*)gx; o.gshift = (S*)gshift; o.ws = ws;
    o.normalize = normalize_grad;
    return run(c, o, stream);
}

// ---- training fusion (round 5): the shift applied to relu(bn2(z)) without the activation ever being stored
// (fused_bn.bn_relu_shift2d; backbone.py:129-131 under models.py:71-79's 2-D variant).  RK_ERR_UNSUPPORTED (nothing launched) when
// no fused kernel covers the configuration (quantize; column kernels switched off and a shape the streaming kernels do not take); the caller then normalises
// with rk_bn_apply_affine_* and calls the plain entry points.
template <typename T>
int forward2_bn(const void* z, const float* ab, const float* shift, void* y, int N, int C, int H, int W, int sH, int sW, int pH,
                int pW, int quantize, rk_stream_t stream) {
    if (!z || !ab || !shift || !y) return RK_ERR_NULL_POINTER;
    Call c{};
    if (int rc = make_dims2(c.d, N, C, H, W, sH, sW, pH, pW)) return rc;
    c.form = kForwardBn; c.elem = (int)sizeof(T); c.quantize = quantize;
    c.align[kX] = al(z); c.align[kY] = al(y); c.align[kGx] = 16; c.align[kBn] = al(ab);
    Ops<T, float> o{};
    o.x = (const T*)z; o.shift = shift; o.y = (T*)y; o.ab = ab;
    return run(c, o, stream);
}
template <typename T>
int backward2_bn(const void* gy, const void* z, const float* abmi, const float* shift, void* dz, float* gshift, float* k12,
                 float* dgamma, float* dbeta, int N, int C, int H, int W, int sH, int sW, int pH, int pW, int normalize_grad,
                 int quantize, void* ws, size_t ws_bytes, rk_stream_t stream) {
    if (!gy || !z || !abmi || !shift || !dz || !gshift || !k12 || !dgamma || !dbeta) return RK_ERR_NULL_POINTER;
    Call c{};
    if (int rc = make_dims2(c.d, N, C, H, W, sH, sW, pH, pW)) return rc;
    if (quantize) return RK_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < 2 * workspace_bytes(c.d, shape_switches())) return RK_ERR_WORKSPACE;
    c.form = kBackwardBn; c.elem = (int)sizeof(T); c.gshift = true;
    c.align[kX] = al(z); c.align[kY] = al(gy); c.align[kGx] = al(dz); c.align[kBn] = al(abmi);
    Ops<T, float> o{};
    o.gy = (const T*)gy; o.x = (const T*)z; o.shift = shift; o.gx = (T*)dz; o.gshift = gshift; o.ws = ws;
    o.normalize = normalize_grad;
    o.bn.abmi = reinterpret_cast<const float4*>(abmi);
    o.bn.k12 = k12; o.bn.dgamma = dgamma; o.bn.dbeta = dbeta;
    o.bn.inv_count = (float)(1.0 / ((double)N * H * W));
    return run(c, o, stream);
}

}  // namespace

extern "C" {

size_t rk2d_backward_workspace_bytes(int N, int C, int H, int W, int sH, int sW, int pH, int pW, int elem_size) {
    Dims2 d;
    if (make_dims2(d, N, C, H, W, sH, sW, pH, pW)) return 0;
    (void)elem_size;                                               // fp32 and fp64 partials share the 16-byte slot
    return workspace_bytes(d, shape_switches());
}

#define RK_DEF_2D(SFX, TYPE, CTYPE)                                                                              \
    int rk2d_forward_##SFX(const CTYPE* x, const CTYPE* shift, CTYPE* y, int N, int C, int H, int W, int sH,     \
                           int sW, int pH, int pW, int quantize, rk_stream_t stream) {                           \
        return forward2<TYPE, TYPE>(x, shift, y, N, C, H, W, sH, sW, pH, pW, quantize, stream);                      \
    }                                                                                                            \
    int rk2d_backward_##SFX(const CTYPE* gy, const CTYPE* x, const CTYPE* shift, CTYPE* gx, CTYPE* gshift,       \
                            int N, int C, int H, int W, int sH, int sW, int pH, int pW, int normalize_grad,     \
                            int enable_shift_grad, int quantize, void* ws, size_t ws_bytes, rk_stream_t stream) { \
        return backward2<TYPE, TYPE>(gy, x, shift, gx, gshift, N, C, H, W, sH, sW, pH, pW, normalize_grad,             \
                               enable_shift_grad, quantize, ws, ws_bytes, stream);                               \
    }
RK_DEF_2D(f32, float, float)
RK_DEF_2D(f64, double, double)
RK_DEF_2D(f16, __half, void)
RK_DEF_2D(bf16, __hip_bfloat16, void)
#undef RK_DEF_2D

// 16-bit activations with the shift table / d(shift) in fp32 (what autocast hands the operator: bf16 activations next
// to an fp32 nn.Parameter).  Everything that depends on the shift -- floor / remainder, the 1e-7 integer test, the
// quantize position arithmetic -- is then evaluated in fp32 exactly as by rk2d_*_f32.
#define RK_DEF_2D_MIXED(SFX, TYPE)                                                                               \
    int rk2d_forward_##SFX##_sf32(const void* x, const float* shift, void* y, int N, int C, int H, int W, int sH, \
                                  int sW, int pH, int pW, int quantize, rk_stream_t stream) {                    \
        return forward2<TYPE, float>(x, shift, y, N, C, H, W, sH, sW, pH, pW, quantize, stream);                 \
    }                                                                                                            \
    int rk2d_backward_##SFX##_sf32(const void* gy, const void* x, const float* shift, void* gx, float* gshift,   \
                                   int N, int C, int H, int W, int sH, int sW, int pH, int pW,                   \
                                   int normalize_grad, int enable_shift_grad, int quantize, void* ws,            \
                                   size_t ws_bytes, rk_stream_t stream) {                                        \
        return backward2<TYPE, float>(gy, x, shift, gx, gshift, N, C, H, W, sH, sW, pH, pW, normalize_grad,      \
                                      enable_shift_grad, quantize, ws, ws_bytes, stream);                        \
    }
RK_DEF_2D_MIXED(f16, __half)
RK_DEF_2D_MIXED(bf16, __hip_bfloat16)
#undef RK_DEF_2D_MIXED

// 1 when rk2d_forward_bn_* / rk2d_backward_bn_* have a fused kernel for this shape and storage size (4: fp32, 2: bf16), else 0:
// lets a caller decide BEFORE it runs bn2's statistics (whose side effects -- running statistics -- must happen once).  The answer
// is the planner's: both BN forms plan to RK_OK with every operand aligned.
int rk2d_bn_fused_shape(int N, int C, int H, int W, int sH, int sW, int pH, int pW, int elem_size) {
    Call c{};
    if (make_dims2(c.d, N, C, H, W, sH, sW, pH, pW)) return 0;
    if (elem_size != 4 && elem_size != 2) return 0;
    c.elem = elem_size; c.gshift = true;
    for (int& a : c.align) a = 16;
    c.form = kForwardBn;
    if (plan(c, shape_switches()).rc) return 0;
    c.form = kBackwardBn;
    return plan(c, shape_switches()).rc ? 0 : 1;
}
size_t rk2d_backward_bn_workspace_bytes(int N, int C, int H, int W, int sH, int sW, int pH, int pW) {
    Dims2 d;
    if (make_dims2(d, N, C, H, W, sH, sW, pH, pW)) return 0;
    return 2 * workspace_bytes(d, shape_switches());               // four partials per (channel, group) instead of two
}
int rk2d_forward_bn_f32(const float* z, const float* ab, const float* shift, float* y, int N, int C, int H, int W, int sH,
                        int sW, int pH, int pW, int quantize, rk_stream_t stream) {
    return forward2_bn<float>(z, ab, shift, y, N, C, H, W, sH, sW, pH, pW, quantize, stream);
}
int rk2d_forward_bn_bf16_sf32(const void* z, const float* ab, const float* shift, void* y, int N, int C, int H, int W, int sH,
                              int sW, int pH, int pW, int quantize, rk_stream_t stream) {
    return forward2_bn<__hip_bfloat16>(z, ab, shift, y, N, C, H, W, sH, sW, pH, pW, quantize, stream);
}
int rk2d_backward_bn_f32(const float* gy, const float* z, const float* abmi, const float* shift, float* dz, float* gshift,
                         float* k12, float* dgamma, float* dbeta, int N, int C, int H, int W, int sH, int sW, int pH, int pW,
                         int normalize_grad, int quantize, void* ws, size_t ws_bytes, rk_stream_t stream) {
    return backward2_bn<float>(gy, z, abmi, shift, dz, gshift, k12, dgamma, dbeta, N, C, H, W, sH, sW, pH, pW, normalize_grad,
                               quantize, ws, ws_bytes, stream);
}
int rk2d_backward_bn_bf16_sf32(const void* gy, const void* z, const float* abmi, const float* shift, void* dz, float* gshift,
                               float* k12, float* dgamma, float* dbeta, int N, int C, int H, int W, int sH, int sW, int pH,
                               int pW, int normalize_grad, int quantize, void* ws, size_t ws_bytes, rk_stream_t stream) {
    return backward2_bn<__hip_bfloat16>(gy, z, abmi, shift, dz, gshift, k12, dgamma, dbeta, N, C, H, W, sH, sW, pH, pW,
                                        normalize_grad, quantize, ws, ws_bytes, stream);
}

// Test hook: the planner with explicit switches and alignments (no device call).  form: 0 forward, 1 backward, 2 rk2d_forward_bn_*,
// 3 rk2d_backward_bn_*; elem_size 4 / 8 / 2; aligned: two bits per operand (x / z, y or gy, gx / dz, the BN pack, from bit 0):
// 2 = a multiple of 16 bytes, 1 = of 8, 0 = neither; shift_kernels: 0 auto, 1 column, 2 generic; cus: compute units.
// out[0] = launches, out[1] = P, out[2] = k2d_finalize / k2d_finalize_bn follows as a launch of its own, then 11 ints per launch:
// family (rk2d_plan.hpp), negate, bn, rounds, M, single, vec, quant, grid, block, dynamic LDS bytes.  Returns the call's status
// as far as it does not depend on pointers.
int rk_debug_2d_plan(int form, int elem_size, int N, int C, int H, int W, int sH, int sW, int pH, int pW, int quantize,
                     int want_gshift, int aligned, int shift_kernels, int cus, int* out) {
    Call c{};
    if (int rc = make_dims2(c.d, N, C, H, W, sH, sW, pH, pW)) return rc;
    c.form = (Form)form; c.elem = elem_size; c.quantize = quantize; c.gshift = want_gshift || form == kBackwardBn;
    for (int i = 0; i < 4; ++i) c.align[i] = 8 * ((aligned >> (2 * i)) & 3);
    const Plan pl = plan(c, Switches{(ShiftKernels)shift_kernels, cus});
    if (!out) return pl.rc;
    out[0] = pl.n; out[1] = pl.P; out[2] = pl.finalize;
    for (int i = 0; i < 3; ++i) {
        const Launch& l = pl.l[i];
        const bool fin = l.family == kFinalize || l.family == kFinalizeBn;
        const int v[11] = {l.family, l.c.negate, l.c.bn, l.c.rounds, l.c.M, l.c.single, l.c.vec, l.c.quant, (int)l.c.grid,
                           i >= pl.n ? 0 : fin ? finalize_block(pl.P) : kBlock, (int)l.c.lds};
        for (int k = 0; k < 11; ++k) out[3 + 11 * i + k] = v[k];
    }
    return pl.rc;
}

}  // extern "C"
