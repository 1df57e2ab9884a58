// rk3d.hip -- C-ABI entry points of the RubiksShift3D operator (include/rubiks_hip.h).
// Host glue restating cuda_src/rubiks.cpp:161-379 (shape math, dispatch) without ATen:
// caller-owned buffers and workspace, explicit stream, error codes instead of exit().
#include "rk3d_plan.hpp"

#include <type_traits>

using namespace rk;
using namespace rk::plan3d;

namespace {

__global__ __launch_bounds__(kWave) void k3d_debug_finalize_only(dma3d::Fin3 fin, int C, int P) {
    dma3d::finalizer_wave<3>(fin, (int)blockIdx.x, C, P);
}

int make_dims(Dims3& d, int N, int T, int C, int H, int W, int sT, int sH, int sW, int pT, int pH, int pW) {
    if (N <= 0 || T <= 0 || C <= 0 || H <= 0 || W <= 0) return RK_ERR_BAD_DIMS;
    if (sT <= 0 || sH <= 0 || sW <= 0 || pT < 0 || pH < 0 || pW < 0) return RK_ERR_BAD_STRIDE;
    d.N = N; d.T = T; d.C = C; d.H = H; d.W = W;
    d.sT = sT; d.sH = sH; d.sW = sW; d.pT = pT; d.pH = pH; d.pW = pW;
    d.To = out_len(T, sT, pT); d.Ho = out_len(H, sH, pH); d.Wo = out_len(W, sW, pW);
    if (d.To <= 0 || d.Ho <= 0 || d.Wo <= 0) return RK_ERR_BAD_DIMS;
    // the reference indexes with int (rubiks3d_kernels.cu:34-36); keep the same limit
    const long long nin = (long long)N * T * C * H * W, nout = (long long)N * d.To * C * d.Ho * d.Wo;
    if (nin > 0x7fffffffLL || nout > 0x7fffffffLL) return RK_ERR_BAD_DIMS;
    return RK_OK;
}

// the process's switches, read once: RK_SHIFT_KERNELS (rk_common.hpp) and RK_SLAB14 (rk3d_plan.hpp)
const Switches& env_switches() {
    static const Switches sw = [] {
        const char* e = getenv("RK_SLAB14");
        return Switches{shift_kernels(), e ? (e[0] == '1' ? 1 : 0) : -1};
    }();
    return sw;
}
// the Aligned bit `bit` of an operand (NULL: the call does not have it)
int al(const void* p, int bit) { return ((uintptr_t)p & 15) == 0 ? bit : 0; }

// the operands of a call, by the names the launchers use
template <typename T> struct Ops {
    const T* x; const T* shift; const T* gy; T* y; T* gx; T* gshift; T* ws;
    int normalize; T t_factor;
    dma3d::BnFuse bn;
};

// runs one planned launch
template <typename T>
void run(const Launch& l, const Dims3& d, int P, const Ops<T>& o, hipStream_t stream) {
    const Cfg3& c = l.c;
    if constexpr (std::is_same<T, float>::value) {
        const bool negate = c.v[0];                                    // forward / d(x)-only families
        const float* src = negate ? o.gy : o.x;
        float* dst = negate ? o.gx : o.y;
        const bool bwd = l.family == kDmaBwd || l.family == kTileBwd || l.family == kSlabBwd || l.family == kS2Bwd ||
                         l.family == kSlabS2Bwd || l.family == kColBwd;
        float* gx = bwd && c.v[0] ? o.gx : nullptr;                    // (the d(shift) half behind a translation writes no d(x))
        const dma3d::Fin3 fin = bwd && c.v[1] ? dma3d::make_fin3(o.ws, (int)c.grid - d.C, o.gshift, o.normalize, o.t_factor) : dma3d::Fin3{};
        switch (l.family) {
            case kPlane: return plane3d::launch(c, l.g.plane, src, o.shift, dst, o.bn.abmi, stream);
            case kDmaInterp:
                if (c.v[1]) return dma3d::launch_forward_bn(c, l.g.band, src, o.shift, dst, o.bn.abmi, stream);
                if (negate) return dma3d::launch_interp<true>(c, l.g.band, src, o.shift, dst, stream);
                return dma3d::launch_interp<false>(c, l.g.band, src, o.shift, dst, stream);
            case kTileInterp: return tile3d::launch_interp(c, d, src, o.shift, dst, o.bn.abmi, stream);
            case kSlabInterp: return slab3d::launch_interp(c, l.g.slab, d, src, o.shift, dst, stream);
            case kXlate: return xlate3d::launch(c, l.g.gen, src, o.shift, dst, stream);
            case kS2Fwd: return s2::launch_forward(c, l.g.s2, o.x, o.shift, o.y, o.bn.abmi, stream);
            case kSlabS2Fwd: return slab3d::launch_fwd_s2(c, l.g.slab2, d, o.x, o.shift, o.y, stream);
            case kDmaBwd: return dma3d::launch_bwd(c, l.g.band, d, o.x, o.shift, o.gy, gx, o.ws, fin, o.bn, stream);
            case kTileBwd: return tile3d::launch_bwd(c, d, o.x, o.shift, o.gy, gx, o.ws, fin, o.bn, stream);
            case kSlabBwd: return slab3d::launch_bwd(c, l.g.slab, d, o.x, o.shift, o.gy, gx, o.ws, fin, stream);
            case kS2Bwd: return s2::launch_backward(c, l.g.s2, d, o.x, o.shift, o.gy, gx, o.ws, fin, o.bn, stream);
            case kSlabS2Bwd: return slab3d::launch_bwd_s2(c, l.g.slab2, d, o.x, o.shift, o.gy, gx, o.ws, fin, stream);
            case kColBwd: return col3d::launch_backward<T>(c, l.g.col, o.x, o.shift, o.gy, gx, o.ws, fin, stream);
            default: break;
        }
    }
    const dim3 grid(c.grid), block(kBlock);
    switch (l.family) {
        case kColFwd: return col3d::launch_forward<T>(c, l.g.col, o.x, o.shift, o.y, stream);
        case kColBwd: return col3d::launch_backward<T>(c, l.g.col, o.x, o.shift, o.gy, o.gx, o.ws, dma3d::Fin3{}, stream);
        case kGenFwd:
            if (c.v[0]) hipLaunchKernelGGL((k3d_forward_generic<T, true>), grid, block, 0, stream, o.x, o.shift, o.y, l.g.gen);
            else hipLaunchKernelGGL((k3d_forward_generic<T, false>), grid, block, 0, stream, o.x, o.shift, o.y, l.g.gen);
            return;
        case kGenBwdX:
            if (c.v[0]) hipLaunchKernelGGL((k3d_backward_input_generic<T, true>), grid, block, 0, stream, o.shift, o.gy, o.gx, l.g.gen);
            else hipLaunchKernelGGL((k3d_backward_input_generic<T, false>), grid, block, 0, stream, o.shift, o.gy, o.gx, l.g.gen);
            return;
        case kGenBwdS:
            hipLaunchKernelGGL((k3d_backward_shift_generic<T>), grid, block, 0, stream, o.x, o.shift, o.gy, o.ws, l.g.gen);
            return;
        case kFinalize:
            hipLaunchKernelGGL((k3d_finalize<T>), grid, dim3(finalize_block(P)), 0, stream, (const T*)o.ws, o.gshift, d.C, P,
                               o.normalize, o.t_factor);
            return;
        default: return;
    }
}
template <typename T>
int run(const Plan& pl, const Dims3& d, const Ops<T>& o, rk_stream_t stream) {
    if (pl.rc) return pl.rc;
    for (int i = 0; i < pl.n; ++i) run<T>(pl.l[i], d, pl.P, o, (hipStream_t)stream);
    return launch_status();
}

template <typename T>
int forward_impl(const T* x, const T* shift, T* y, int N, int Tn, int C, int H, int W, int sT, int sH, int sW,
                 int pT, int pH, int pW, int quantize, rk_stream_t stream) {
    if (!x || !shift || !y) return RK_ERR_NULL_POINTER;
    Call c{};
    if (int rc = make_dims(c.d, N, Tn, C, H, W, sT, sH, sW, pT, pH, pW)) return rc;
    c.form = kForward; c.elem = (int)sizeof(T); c.quantize = quantize;
    c.aligned = al(x, kAlX) | al(y, kAlY);
    Ops<T> o{};
    o.x = x; o.shift = shift; o.y = y;
    return run<T>(plan(c, env_switches()), c.d, o, stream);
}

// `P_out` != nullptr: two-phase use -- stop after the partials (ws[C][3][*P_out]) and report their count instead of
// running the row-sum + K5 (rk3d_backward_finalize_* does that).
template <typename T>
int backward_impl(const T* x, const T* shift, const T* gy, T* gx, T* gshift, int N, int Tn, int C, int H, int W,
                  int sT, int sH, int sW, int pT, int pH, int pW, int normalize_grad, T t_factor, int quantize,
                  void* ws, size_t ws_bytes, rk_stream_t stream, int* P_out = nullptr) {
    if (!shift || !gy || (!gx && !gshift)) return RK_ERR_NULL_POINTER;
    if (gshift && !x) return RK_ERR_NULL_POINTER;
    Call c{};
    if (int rc = make_dims(c.d, N, Tn, C, H, W, sT, sH, sW, pT, pH, pW)) return rc;
    if (gshift) {
        const size_t need = rk3d_backward_workspace_bytes(N, Tn, C, H, W, sT, sH, sW, pT, pH, pW, (int)sizeof(T));
        if (!ws || ws_bytes < need) return RK_ERR_WORKSPACE;
    }
    c.form = kBackward; c.elem = (int)sizeof(T); c.quantize = quantize;
    c.gx = gx; c.gshift = gshift; c.two_phase = P_out;
    c.aligned = al(x, kAlX) | al(gy, kAlY) | al(gx, kAlGx);
    const Plan pl = plan(c, env_switches());
    Ops<T> o{};
    o.x = x; o.shift = shift; o.gy = gy; o.gx = gx; o.gshift = gshift; o.ws = (T*)ws;
    o.normalize = normalize_grad; o.t_factor = t_factor;
    if (P_out) *P_out = pl.P;
    return run<T>(pl, c.d, o, stream);
}

// ---- 16-bit activations (bf16 / f16) next to an fp32 shift table: the kernels of rk3d_16.hip ----
struct Ops16 {
    const void* x; const float* shift; const void* gy; void* y; void* gx; float* gshift; float* ws;
    int normalize; float t_factor;
};
int run16(const Plan& pl, const Dims3& d, bool bf16, const Ops16& o, rk_stream_t stream_) {
    if (pl.rc) return pl.rc;
    hipStream_t stream = (hipStream_t)stream_;
    for (int i = 0; i < pl.n; ++i) {
        const Launch& l = pl.l[i];
        switch (l.family) {
            case kStream16Fwd: s16::launch_stream_forward(l.c, l.g.s16, bf16, o.x, o.shift, o.y, stream); break;
            case kStream16Bwd: s16::launch_stream_backward(l.c, l.g.s16, bf16, o.x, o.shift, o.gy, o.gx, o.ws, stream); break;
            case kStream16S2Fwd: s16::launch_s2_forward(l.c, l.g.s16s2, bf16, o.x, o.shift, o.y, stream); break;
            case kStream16S2Bwd: s16::launch_s2_backward(l.c, l.g.s16s2, bf16, o.x, o.shift, o.gy, o.gx, o.ws, stream); break;
            case kGen16Fwd: s16::launch_generic_forward(l.c, l.g.gen, bf16, o.x, o.shift, o.y, stream); break;
            case kGen16BwdX: s16::launch_generic_backward_input(l.c, l.g.gen, bf16, o.shift, o.gy, o.gx, stream); break;
            case kGen16BwdS: s16::launch_generic_backward_shift(l.c, l.g.gen, bf16, o.x, o.shift, o.gy, o.ws, stream); break;
            case kFinalize:
                hipLaunchKernelGGL((k3d_finalize<float>), dim3(l.c.grid), dim3(finalize_block(pl.P)), 0, stream, (const float*)o.ws,
                                   o.gshift, d.C, pl.P, o.normalize, o.t_factor);
                break;
            default: break;
        }
    }
    return launch_status();
}
int forward16_impl(bool bf16, const void* x, const float* shift, void* y, int N, int Tn, int C, int H, int W, int sT, int sH,
                   int sW, int pT, int pH, int pW, int quantize, rk_stream_t stream) {
    if (!x || !shift || !y) return RK_ERR_NULL_POINTER;
    Call c{};
    if (int rc = make_dims(c.d, N, Tn, C, H, W, sT, sH, sW, pT, pH, pW)) return rc;
    c.form = kForward; c.elem = 2; c.quantize = quantize;
    c.aligned = al(x, kAlX) | al(y, kAlY) | kAlGx;
    Ops16 o{};
    o.x = x; o.shift = shift; o.y = y;
    return run16(plan(c, env_switches()), c.d, bf16, o, stream);
}
int backward16_impl(bool bf16, const void* x, const float* shift, const void* gy, void* gx, float* gshift, int N, int Tn, int C,
                    int H, int W, int sT, int sH, int sW, int pT, int pH, int pW, int normalize_grad, float t_factor,
                    int quantize, void* ws, size_t ws_bytes, rk_stream_t stream) {
    if (!shift || !gy || (!gx && !gshift)) return RK_ERR_NULL_POINTER;
    if (gshift && !x) return RK_ERR_NULL_POINTER;
    Call c{};
    if (int rc = make_dims(c.d, N, Tn, C, H, W, sT, sH, sW, pT, pH, pW)) return rc;
    if (gshift) {
        const size_t need = rk3d_backward_workspace_bytes(N, Tn, C, H, W, sT, sH, sW, pT, pH, pW, 2);
        if (!ws || ws_bytes < need) return RK_ERR_WORKSPACE;
    }
    c.form = kBackward; c.elem = 2; c.quantize = quantize;
    c.gx = gx; c.gshift = gshift;
    c.aligned = al(x, kAlX) | al(gy, kAlY) | al(gx, kAlGx);
    Ops16 o{};
    o.x = x; o.shift = shift; o.gy = gy; o.gx = gx; o.gshift = gshift; o.ws = (float*)ws;
    o.normalize = normalize_grad; o.t_factor = t_factor;
    return run16(plan(c, env_switches()), c.d, bf16, o, stream);
}

}  // namespace

extern "C" {

size_t rk3d_backward_workspace_bytes(int N, int T, int C, int H, int W, int sT, int sH, int sW, int pT, int pH,
                                     int pW, int elem_size) {
    (void)sH; (void)sW; (void)pH; (void)pW;
    if (N <= 0 || T <= 0 || C <= 0 || sT <= 0 || pT < 0) return 0;
    // partials part[C][3][P]: P = N*To for the generic kernels, N*nbands (row bands) for the streaming ones
    size_t per_n = (size_t)out_len(T, sT, pT);
    if (H > 0 && (size_t)H > per_n) per_n = (size_t)H;    // row bands: nbands <= H
    if (H > 0 && W > 0) {                                 // column kernels: 256-element chunks at most
        const size_t chunks = ((size_t)H * (size_t)W + 255) / 256;
        if (chunks > per_n) per_n = chunks;
    }
    const size_t P = (size_t)N * per_n;
    // fp32: the streaming backward keeps its partials as 16-byte granule pairs (rk_dma.hpp: fin_publish)
    // 16-bit activations (elem_size 2): plain fp32 partials
    return (size_t)C * 3 * P * (size_t)(elem_size == 4 ? 16 : elem_size == 2 ? 4 : elem_size);
}

// ---- training fusion: the shift applied to relu(bn(z)) without the activation ever being stored (train_block.py) ----
// Both return RK_ERR_UNSUPPORTED (no launch, nothing touched) when no fused kernel covers the configuration; the caller
// then normalises with rk_bn_apply_affine_f32 and calls the plain entry points.
int rk3d_forward_bn_f32(const float* z, const float* abmi, const float* shift, float* y, int N, int T, int C, int H,
                        int W, int sT, int sH, int sW, int pT, int pH, int pW, int quantize, rk_stream_t stream) {
    if (!z || !abmi || !shift || !y) return RK_ERR_NULL_POINTER;
    Call c{};
    if (int rc = make_dims(c.d, N, T, C, H, W, sT, sH, sW, pT, pH, pW)) return rc;
    c.form = kForwardBn; c.elem = 4; c.quantize = quantize;
    c.aligned = al(z, kAlX) | al(y, kAlY) | al(abmi, kAlBn);
    Ops<float> o{};
    o.x = z; o.shift = shift; o.y = y;
    o.bn.abmi = reinterpret_cast<const float4*>(abmi);
    return run<float>(plan(c, env_switches()), c.d, o, stream);
}
size_t rk3d_backward_bn_workspace_bytes(int N, int T, int C, int H, int W, int sT, int sH, int sW, int pT, int pH, int pW) {
    // five partials per (channel, column-band) instead of three, as 16-byte granule pairs
    return rk3d_backward_workspace_bytes(N, T, C, H, W, sT, sH, sW, pT, pH, pW, 4) / 3 * 5;
}
int rk3d_backward_bn_f32(const float* z, const float* abmi, const float* shift, const float* gy, float* dz, float* gshift,
                         float* k12, float* dgamma, float* dbeta, int N, int T, int C, int H, int W, int sT, int sH,
                         int sW, int pT, int pH, int pW, int normalize_grad, float t_factor, int quantize, void* ws,
                         size_t ws_bytes, rk_stream_t stream) {
    if (!z || !abmi || !shift || !gy || !dz || !gshift || !k12 || !dgamma || !dbeta) return RK_ERR_NULL_POINTER;
    Call c{};
    if (int rc = make_dims(c.d, N, T, C, H, W, sT, sH, sW, pT, pH, pW)) return rc;
    if (!ws || ws_bytes < rk3d_backward_bn_workspace_bytes(N, T, C, H, W, sT, sH, sW, pT, pH, pW)) return RK_ERR_WORKSPACE;
    c.form = kBackwardBn; c.elem = 4; c.quantize = quantize; c.gx = c.gshift = true;
    c.aligned = al(z, kAlX) | al(gy, kAlY) | al(dz, kAlGx) | al(abmi, kAlBn);
    Ops<float> o{};
    o.x = z; o.shift = shift; o.gy = gy; o.gx = dz; o.gshift = gshift; o.ws = (float*)ws;
    o.normalize = normalize_grad; o.t_factor = t_factor;
    o.bn.abmi = reinterpret_cast<const float4*>(abmi);
    o.bn.k12 = k12; o.bn.dgamma = dgamma; o.bn.dbeta = dbeta;
    o.bn.inv_count = (float)(1.0 / ((double)N * T * H * W));
    return run<float>(plan(c, env_switches()), c.d, o, stream);
}

int rk3d_forward_f32(const float* x, const float* shift, float* y, int N, int T, int C, int H, int W, int sT,
                     int sH, int sW, int pT, int pH, int pW, int quantize, rk_stream_t stream) {
    return forward_impl<float>(x, shift, y, N, T, C, H, W, sT, sH, sW, pT, pH, pW, quantize, stream);
}
int rk3d_forward_f64(const double* x, const double* shift, double* y, int N, int T, int C, int H, int W, int sT,
                     int sH, int sW, int pT, int pH, int pW, int quantize, rk_stream_t stream) {
    return forward_impl<double>(x, shift, y, N, T, C, H, W, sT, sH, sW, pT, pH, pW, quantize, stream);
}
int rk3d_backward_f32(const float* x, const float* shift, const float* gy, float* gx, float* gshift, int N, int T,
                      int C, int H, int W, int sT, int sH, int sW, int pT, int pH, int pW, int normalize_grad,
                      float t_factor, int quantize, void* ws, size_t ws_bytes, rk_stream_t stream) {
    return backward_impl<float>(x, shift, gy, gx, gshift, N, T, C, H, W, sT, sH, sW, pT, pH, pW, normalize_grad,
                                t_factor, quantize, ws, ws_bytes, stream);
}
int rk3d_backward_f64(const double* x, const double* shift, const double* gy, double* gx, double* gshift, int N,
                      int T, int C, int H, int W, int sT, int sH, int sW, int pT, int pH, int pW,
                      int normalize_grad, double t_factor, int quantize, void* ws, size_t ws_bytes,
                      rk_stream_t stream) {
    return backward_impl<double>(x, shift, gy, gx, gshift, N, T, C, H, W, sT, sH, sW, pT, pH, pW, normalize_grad,
                                 t_factor, quantize, ws, ws_bytes, stream);
}

int rk3d_forward_bf16_sf32(const void* x, const float* shift, void* y, int N, int T, int C, int H, int W, int sT, int sH,
                           int sW, int pT, int pH, int pW, int quantize, rk_stream_t stream) {
    return forward16_impl(true, x, shift, y, N, T, C, H, W, sT, sH, sW, pT, pH, pW, quantize, stream);
}
int rk3d_forward_f16_sf32(const void* x, const float* shift, void* y, int N, int T, int C, int H, int W, int sT, int sH,
                          int sW, int pT, int pH, int pW, int quantize, rk_stream_t stream) {
    return forward16_impl(false, x, shift, y, N, T, C, H, W, sT, sH, sW, pT, pH, pW, quantize, stream);
}
int rk3d_backward_bf16_sf32(const void* x, const float* shift, const void* gy, void* gx, float* gshift, int N, int T, int C,
                            int H, int W, int sT, int sH, int sW, int pT, int pH, int pW, int normalize_grad, float t_factor,
                            int quantize, void* ws, size_t ws_bytes, rk_stream_t stream) {
    return backward16_impl(true, x, shift, gy, gx, gshift, N, T, C, H, W, sT, sH, sW, pT, pH, pW, normalize_grad, t_factor,
                           quantize, ws, ws_bytes, stream);
}
int rk3d_backward_f16_sf32(const void* x, const float* shift, const void* gy, void* gx, float* gshift, int N, int T, int C,
                           int H, int W, int sT, int sH, int sW, int pT, int pH, int pW, int normalize_grad, float t_factor,
                           int quantize, void* ws, size_t ws_bytes, rk_stream_t stream) {
    return backward16_impl(false, x, shift, gy, gx, gshift, N, T, C, H, W, sT, sH, sW, pT, pH, pW, normalize_grad, t_factor,
                           quantize, ws, ws_bytes, stream);
}
// 1 when one of the streaming 16-bit families (rk3d_16.hpp: stride 1, stride (1,2,2)) takes the configuration, pointer
// alignment aside: a pure host predicate
int rk3d_sf32_streams(int N, int T, int C, int H, int W, int sT, int sH, int sW, int pT, int pH, int pW, int quantize,
                      int elem_size) {
    Dims3 d;
    if (elem_size != 2 || quantize || make_dims(d, N, T, C, H, W, sT, sH, sW, pT, pH, pW)) return 0;
    s16::SDims s;
    s16::S2Dims s2;
    Cfg3 c{};
    return s16::geometry(s, c, d) || s16::geometry_s2(s2, c, d, false) ? 1 : 0;
}

// Two-phase form of the fp32 backward (the reference's own host glue has these phases, rubiks.cpp:324-376: K2 + K3/K4,
// then addmv row-sum + K5): phase 1 writes d(x) and the per-channel partials ws[C][3][P] and returns P through
// *partials; phase 2 sums them and normalises.  rk3d_backward_f32 == phase 1 + phase 2.
int rk3d_backward_partials_f32(const float* x, const float* shift, const float* gy, float* gx, int N, int T, int C,
                               int H, int W, int sT, int sH, int sW, int pT, int pH, int pW, int quantize, void* ws,
                               size_t ws_bytes, int* partials, rk_stream_t stream) {
    if (!partials || !ws) return RK_ERR_NULL_POINTER;
    float* not_null = (float*)ws;        // "d(shift) wanted": the partials land in ws, nothing is written through this
    return backward_impl<float>(x, shift, gy, gx, not_null, N, T, C, H, W, sT, sH, sW, pT, pH, pW, 0, 1.0f, quantize, ws,
                                ws_bytes, stream, partials);
}
int rk3d_backward_finalize_f32(const void* ws, int C, int partials, float* gshift, int normalize_grad, float t_factor,
                               rk_stream_t stream) {
    if (!ws || !gshift) return RK_ERR_NULL_POINTER;
    if (C <= 0 || partials <= 0) return RK_ERR_BAD_DIMS;
    hipLaunchKernelGGL((k3d_finalize<float>), dim3(C), dim3(finalize_block(partials)), 0, (hipStream_t)stream,
                       (const float*)ws, gshift, C, partials, normalize_grad, t_factor);
    return launch_status();
}

// Test hook: ONLY the finalizer waves of a fused 3-D backward (rk3d_dma.hpp, finalizer_wave<3>) on a workspace no producer
// will ever publish to -- the give-up path: every channel must come back NaN once the poll budget
// (rk_debug_set_finalize_spins) is spent, and the launch must end.  No product code calls it.  The give-up record is the
// one given (NULL: none), never the registered one: a deliberate give-up must not dirty the record product launches use.
int rk3d_debug_finalize_only_status_f32(void* ws, size_t ws_bytes, int C, int partials, float* gshift, int normalize_grad,
                                        float t_factor, void* record, rk_stream_t stream) {
    if (!ws || !gshift) return RK_ERR_NULL_POINTER;
    if (C <= 0 || partials <= 0) return RK_ERR_BAD_DIMS;
    if ((uintptr_t)record & (RK_FIN_STATUS_BYTES - 1)) return RK_ERR_BAD_DIMS;
    if (ws_bytes < (size_t)C * 3 * partials * 16) return RK_ERR_WORKSPACE;
    dma3d::Fin3 fin = dma3d::make_fin3(ws, 0, gshift, normalize_grad, t_factor);
    fin.f.status = static_cast<unsigned*>(record);
    hipLaunchKernelGGL(k3d_debug_finalize_only, dim3((unsigned)C), dim3(kWave), 0, (hipStream_t)stream, fin, C, partials);
    return launch_status();
}
int rk3d_debug_finalize_only_f32(void* ws, size_t ws_bytes, int C, int partials, float* gshift, int normalize_grad,
                                 float t_factor, rk_stream_t stream) {
    return rk3d_debug_finalize_only_status_f32(ws, ws_bytes, C, partials, gshift, normalize_grad, t_factor, nullptr, stream);
}


// Test hook: the planner with explicit switches and alignment bits (no device call).  form: 0 forward, 1 backward,
// 2 rk3d_forward_bn_f32, 3 rk3d_backward_bn_f32; shift_kernels: 0 auto, 1 column, 2 generic; slab14: -1 unset, 0, 1;
// aligned: 1 x / z, 2 y or gy, 4 gx / dz, 8 the BN pack.  out[0] = launches, out[1] = P, out[2] = a separate finalize
// follows, then 9 ints per launch: family (rk3d_plan.hpp), its variant x 5, grid, block, dynamic LDS bytes.  Returns the
// call's status as far as it does not depend on pointers.
int rk_debug_3d_plan(int form, int elem_size, int N, int T, int C, int H, int W, int sT, int sH, int sW, int pT, int pH, int pW,
                     int quantize, int want_gx, int want_gshift, int two_phase, int aligned, int shift_kernels, int slab14,
                     int* out) {
    Call c{};
    if (int rc = make_dims(c.d, N, T, C, H, W, sT, sH, sW, pT, pH, pW)) return rc;
    c.form = (Form)form; c.elem = elem_size; c.quantize = quantize;
    c.gx = want_gx; c.gshift = want_gshift; c.two_phase = two_phase; c.aligned = aligned;
    const Plan pl = plan(c, Switches{(ShiftKernels)shift_kernels, slab14});
    if (!out) return pl.rc;
    out[0] = pl.n; out[1] = pl.P; out[2] = pl.finalize;
    for (int i = 0; i < 3; ++i) {
        const Launch& l = pl.l[i];
        int* o = out + 3 + 9 * i;
        o[0] = l.family;
        for (int k = 0; k < 5; ++k) o[1 + k] = l.c.v[k];
        o[6] = (int)l.c.grid; o[7] = i >= pl.n ? 0 : l.family == kFinalize ? finalize_block(pl.P) : kBlock; o[8] = (int)l.c.lds;
    }
    return pl.rc;
}

}  // extern "C"
