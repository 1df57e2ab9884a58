// rk3d_16.hip -- RubiksShift3D kernels for 16-bit activations (bf16 / f16) next to an fp32 shift table (rk3d_16.hpp).
//
// Generic family: the plane kernels of rk3d_generic.hpp instantiated at <float, ., S>.
//
// Streaming family (stride 1 / pad 0, quantize off).  A workgroup of 256 threads owns the channels c0 .. c0+G-1 of one
// clip n and walks the source planes s (x planes in the forward, gy planes in the backward).  The G planes of (n, s) are one
// contiguous slab: it is fetched with 16-byte loads into registers one step ahead and written to the other half of a
// double-buffered LDS slab with 16-byte LDS writes, so a plane is read from HBM once and one barrier ends a step.  A thread
// owns the same packs of 4 consecutive slab elements for the whole walk; per element it keeps the LDS offset of its tap
// (0,0), the validity of its 4 taps and its channel, the channel's remainders come from a small LDS table.
//   forward : B(s) = bilinear of the 4 taps; element of a channel with floor flT emits y[s - flT - 1] =
//             (1-rT) B(s-1) + rT B(s) -- the tree of trilerp (rk3d_generic.hpp), B(s-1) kept in registers.
//   backward: the adjoint form on the input side with the negated shift (fl', r'), as k3d_backward_column has it:
//             gx[k-1] = (1-r'T) Q(s-1) + r'T Q(s) with k = s - fl'T, and the d(shift) terms from Q, its row / column
//             differences and the thread's own x elements, which are loaded directly (8-byte loads), never through LDS.
// The channels of a group have different temporal floors, so the walk covers min(fl) .. max(fl) + T and every element is
// active for the T + 1 steps of its own window (a floor beyond +-T is clamped: everything it reaches is zero anyway).
// When H*W % 4 != 0 (7x7) a pack can straddle two channels: such a pack loads and stores element by element.
// Channels with an exactly-integer shift component take the per-element reference formulation for d(x) and d(shift)
// (backward_input_plane / shift_grad_plane), after the walk, the whole workgroup on one channel at a time.
// d(shift): one fp32 partial per (n, c) and component, ws[C][3][N], summed in a fixed order (no atomics); k3d_finalize<float>
// follows as a launch of its own.
// A plane too large for a slab (112x112) is split into bands of R rows: a workgroup owns one channel (G = 1) and one band,
// the slab is the band's source rows r0 + fl .. r0 + R + fl of that channel, clipped to the plane (R + 1 rows at most), and
// there is one partial per (n, c, band), ws[C][3][N * bands]; band 0 does the whole column of an integer-shift channel.
//
// Streaming family for stride (1,2,2) / pad 0: the same walk with another cell, further down (k3d16_s2_*).
#include "rk3d_16.hpp"

namespace rk {
namespace s16 {

template <typename S> __device__ __forceinline__ float widen1(unsigned short v);
template <> __device__ __forceinline__ float widen1<__hip_bfloat16>(unsigned short v) { return __uint_as_float((unsigned)v << 16); }
template <> __device__ __forceinline__ float widen1<__half>(unsigned short v) { return __half2float(__builtin_bit_cast(__half, v)); }

// element meta word: bits 0-3 validity of taps (0,0) (0,1) (1,0) (1,1), bits 4-9 channel within the group, bit 10 active
constexpr unsigned kActive = 1u << 10;

// per channel of the group: (rT, rH, rW, temporal floor) and (flH, flW, integer component, -)
struct ChanTab {
    float4 f[kMaxG];
    int4 i[kMaxG];
};

// fills the table for channels c0 .. c0+Gl-1 (NEG: of the negated shift) and returns the walk's range over the channels that
// stream (backward: those without an integer component)
template <bool NEG>
__device__ __forceinline__ void channel_table(ChanTab& tab, const float* __restrict__ shift, int C, int c0, int Gl, int T,
                                              int& s_lo, int& s_hi) {
    const int tid = threadIdx.x;
    if (tid < Gl) {
        const float s0 = shift[c0 + tid], s1 = shift[C + c0 + tid], s2 = shift[2 * C + c0 + tid];
        const bool slow = NEG && (split_shift(s0).r == 0 || split_shift(s1).r == 0 || split_shift(s2).r == 0);
        const Frac<float> fT = split_shift(NEG ? -s0 : s0), fH = split_shift(NEG ? -s1 : s1), fW = split_shift(NEG ? -s2 : s2);
        const int fl = fT.fl > T ? T : (fT.fl < -(T + 1) ? -(T + 1) : fT.fl);
        tab.f[tid] = make_float4(fT.r, fH.r, fW.r, __int_as_float(fl));
        tab.i[tid] = make_int4(fH.fl, fW.fl, slow ? 1 : 0, 0);
    }
    __syncthreads();
    s_lo = 0x7fffffff; s_hi = -0x7fffffff;
    for (int g = 0; g < Gl; ++g) {
        if (tab.i[g].z) continue;
        const int fl = __float_as_int(tab.f[g].w);
        s_lo = fl < s_lo ? fl : s_lo;
        s_hi = fl > s_hi ? fl : s_hi;
    }
    s_hi += T;
}

// what a workgroup owns: channels c0 .. c0+Gl-1 of clip n, rows r0 .. r0+rows-1 of their planes (all of them unless the plane
// is split into bands)
struct Owned { int n, c0, Gl, band, r0, rows; };
__device__ __forceinline__ Owned owned(const SDims& sd) {
    Owned o;
    int id = (int)blockIdx.x;
    o.band = id % sd.bands; id /= sd.bands;
    o.n = id / sd.groups;
    o.c0 = (id - o.n * sd.groups) * sd.G;
    o.Gl = sd.d.C - o.c0 < sd.G ? sd.d.C - o.c0 : sd.G;
    o.r0 = o.band * sd.R;
    o.rows = sd.d.H - o.r0 < sd.R ? sd.d.H - o.r0 : sd.R;
    return o;
}
// the slab of source rows, in elements from the start of the group's planes: everything, or a band's rows r0 + fl ..
// r0 + rows + fl of its one channel, clipped
__device__ __forceinline__ void source_rows(const SDims& sd, const Owned& o, const ChanTab& tab, int& src0, int& src_elems) {
    src0 = 0; src_elems = o.Gl * sd.HW;
    if (sd.bands > 1) {
        const int H = sd.d.H, fl = tab.i[0].x;
        int rs = o.r0 + fl, re = o.r0 + o.rows + fl + 1;
        rs = rs < 0 ? 0 : (rs > H ? H : rs);
        re = re < 0 ? 0 : (re > H ? H : re);
        src0 = rs * sd.d.W; src_elems = (re - rs) * sd.d.W;
    }
}

// the thread's elements: LDS offset of tap (0,0) and the meta word.  Pack k of the thread is pack tid + k * 256 of the
// workgroup's rows (per channel `rowsW` elements from row r0 on); the slab in LDS starts src0 elements into the planes.
template <int NP>
__device__ __forceinline__ void element_setup(const ChanTab& tab, int H, int W, int HW, int packs, int rowsW, int r0, int src0,
                                              int (&o00)[NP * 4], unsigned (&meta)[NP * 4]) {
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int p = (int)threadIdx.x + k * kBlock;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = k * 4 + j;
            o00[e] = 0; meta[e] = 0;
            if (p >= packs) continue;
            const int i = 4 * p + j;
            const int cl = i / rowsW, rem = i - cl * rowsW;
            const int hb = rem / W, h = r0 + hb, w = rem - hb * W;
            const int4 ti = tab.i[cl];
            const int h0 = h + ti.x, w0 = w + ti.y;
            const bool mh0 = h0 >= 0 && h0 < H, mh1 = h0 + 1 >= 0 && h0 + 1 < H;
            const bool mw0 = w0 >= 0 && w0 < W, mw1 = w0 + 1 >= 0 && w0 + 1 < W;
            o00[e] = cl * HW + h0 * W + w0 - src0;
            meta[e] = (mh0 && mw0 ? 1u : 0u) | (mh0 && mw1 ? 2u : 0u) | (mh1 && mw0 ? 4u : 0u) | (mh1 && mw1 ? 8u : 0u) |
                      ((unsigned)cl << 4) | (ti.z ? 0u : kActive);
        }
    }
}

// one plane's slab, global -> registers -> LDS, 16 bytes per access; chunk q of the thread is chunk tid + q * 256
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 chunk_load(const void* plane, int ch, int chunks) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (ch < chunks) v = reinterpret_cast<const u32x4*>(plane)[ch];
    return v;
}
__device__ __forceinline__ void chunk_store(unsigned short* lds, int ch, int chunks, u32x4 v) {
    if (ch < chunks) reinterpret_cast<u32x4*>(lds)[ch] = v;
}
#define RK16_SLAB_LOAD(plane) do { r0 = chunk_load(plane, (int)threadIdx.x, chunks); r1 = chunk_load(plane, (int)threadIdx.x + kBlock, chunks); } while (0)
#define RK16_SLAB_STORE(lds) do { chunk_store(lds, (int)threadIdx.x, chunks, r0); chunk_store(lds, (int)threadIdx.x + kBlock, chunks, r1); } while (0)

template <typename S>
__device__ __forceinline__ void taps(const unsigned short* pl, int o, unsigned mk, int W, float& q00, float& q01, float& q10,
                                     float& q11) {
    // all four reads issued unconditionally (a tap that does not exist reads element 0 and is masked at use): predicated
    // reads would each wait for their own LDS round trip
    const unsigned short v00 = pl[(mk & 1u) ? o : 0], v01 = pl[(mk & 2u) ? o + 1 : 0];
    const unsigned short v10 = pl[(mk & 4u) ? o + W : 0], v11 = pl[(mk & 8u) ? o + W + 1 : 0];
    q00 = (mk & 1u) ? widen1<S>(v00) : 0.f;
    q01 = (mk & 2u) ? widen1<S>(v01) : 0.f;
    q10 = (mk & 4u) ? widen1<S>(v10) : 0.f;
    q11 = (mk & 8u) ? widen1<S>(v11) : 0.f;
}
// the table entry of element e's channel: pack-mates share a channel unless H*W % 4 != 0
template <bool ODD>
__device__ __forceinline__ float4 entry(const ChanTab& tab, unsigned meta_e, unsigned meta_0, const float4& first) {
    if (!ODD || ((meta_e ^ meta_0) & (63u << 4)) == 0) return first;
    return tab.f[(meta_e >> 4) & 63u];
}

// ------------------------------------------------------------------------------------ forward
template <typename S, int NP, bool ODD>
__global__ __launch_bounds__(kBlock) void k3d16_stream_forward(const S* __restrict__ x, const float* __restrict__ shift,
                                                               S* __restrict__ y, SDims sd) {
    __shared__ __attribute__((aligned(16))) unsigned short slab[2][NP * 4 * kBlock];
    __shared__ ChanTab tab;
    const Dims3& d = sd.d;
    const Owned own = owned(sd);
    const int n = own.n, c0 = own.c0, Gl = own.Gl;
    const int HW = sd.HW, T = d.T, W = d.W, rowsW = own.rows * W;
    const int packs = Gl * rowsW >> 2;
    const size_t tstride = (size_t)d.C * HW;

    int s_lo, s_hi;
    channel_table<false>(tab, shift, d.C, c0, Gl, T, s_lo, s_hi);
    int src0, src_elems;
    source_rows(sd, own, tab, src0, src_elems);
    const int chunks = src_elems >> 3;
    const S* xg = x + ((size_t)n * T * d.C + c0) * HW + src0;            // the slab of (n, t = 0)
    S* yg = y + ((size_t)n * T * d.C + c0) * HW + own.r0 * W;           // the workgroup's rows of (n, t = 0)
    int o00[NP * 4];
    unsigned meta[NP * 4];
    element_setup<NP>(tab, d.H, W, HW, packs, rowsW, own.r0, src0, o00, meta);
    float Bprev[NP * 4];
#pragma unroll
    for (int e = 0; e < NP * 4; ++e) Bprev[e] = 0.f;

    u32x4 r0 = {0u, 0u, 0u, 0u}, r1 = r0;
    int buf = 0;
    if (s_lo >= 0 && s_lo < T) {
        RK16_SLAB_LOAD(xg + (size_t)s_lo * tstride);
        RK16_SLAB_STORE(slab[0]);
    }
    __syncthreads();
    for (int s = s_lo; s <= s_hi; ++s, buf ^= 1) {
        const bool next = s + 1 >= 0 && s + 1 < T && s + 1 <= s_hi;
        if (next) RK16_SLAB_LOAD(xg + (size_t)(s + 1) * tstride);
        const bool valid = s >= 0 && s < T;
        const unsigned short* pl = slab[buf];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int p = (int)threadIdx.x + k * kBlock;
            if (p >= packs) continue;
            float res[4];
            int to[4];
            const float4 tf0 = tab.f[(meta[k * 4] >> 4) & 63u];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = k * 4 + j;
                const float4 tf = entry<ODD>(tab, meta[e], meta[k * 4], tf0);
                const float rT = tf.x, rH = tf.y, rW = tf.z;
                float B = 0.f;
                if (valid) {
                    float q00, q01, q10, q11;
                    taps<S>(pl, o00[e], meta[e], W, q00, q01, q10, q11);
                    B = (1 - rH) * (q00 * (1 - rW) + q01 * rW) + rH * (q10 * (1 - rW) + q11 * rW);
                }
                res[j] = (1 - rT) * Bprev[e] + rT * B;
                Bprev[e] = B;
                to[j] = s - __float_as_int(tf.w) - 1;
            }
            const bool whole = !ODD || ((meta[k * 4] ^ meta[k * 4 + 3]) & (63u << 4)) == 0;     // one channel: one output plane
            if (whole) {
                if (to[0] >= 0 && to[0] < T)
                    *reinterpret_cast<uint2*>(yg + (size_t)to[0] * tstride + 4 * p) = Cell4<S>::narrow(res[0], res[1], res[2], res[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (to[j] >= 0 && to[j] < T) st(yg + (size_t)to[j] * tstride + 4 * p + j, res[j]);
            }
        }
        if (next) RK16_SLAB_STORE(slab[buf ^ 1]);
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------------- backward
template <typename S, int NP, bool ODD, bool WRITE_GX, bool WANT_GS>
__global__ __launch_bounds__(kBlock) void k3d16_stream_backward(const S* __restrict__ x, const float* __restrict__ shift,
                                                                const S* __restrict__ gy, S* __restrict__ gx,
                                                                float* __restrict__ part, SDims sd) {
    // the gy slab twice; after the walk the same memory holds the d(shift) terms, one per pack (ODD: per element)
    constexpr int NA = ODD ? NP * 4 : NP;                        // accumulator triples per thread
    constexpr int kSlabBytes = 2 * NP * 4 * kBlock * 2, kSumBytes = 3 * NA * kBlock * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[kSlabBytes > kSumBytes ? kSlabBytes : kSumBytes];
    __shared__ ChanTab tab;
    __shared__ float red[3][kBlock / kWave];
    unsigned short (*slab)[NP * 4 * kBlock] = reinterpret_cast<unsigned short (*)[NP * 4 * kBlock]>(smem);
    float (*sums)[NA * kBlock] = reinterpret_cast<float (*)[NA * kBlock]>(smem);
    const Dims3& d = sd.d;
    const int tid = threadIdx.x;
    const Owned own = owned(sd);
    const int n = own.n, c0 = own.c0, Gl = own.Gl;
    const int HW = sd.HW, T = d.T, W = d.W, rowsW = own.rows * W;
    const int packs = Gl * rowsW >> 2, P = d.N * sd.bands;
    const size_t tstride = (size_t)d.C * HW;
    const size_t base = ((size_t)n * T * d.C + c0) * HW + own.r0 * W;    // the workgroup's rows of (n, t = 0)

    int s_lo, s_hi;
    channel_table<true>(tab, shift, d.C, c0, Gl, T, s_lo, s_hi);
    int src0, src_elems;
    source_rows(sd, own, tab, src0, src_elems);
    const int chunks = src_elems >> 3;
    const S* gg = gy + ((size_t)n * T * d.C + c0) * HW + src0;           // the slab of (n, t = 0)
    int o00[NP * 4];
    unsigned meta[NP * 4];
    element_setup<NP>(tab, d.H, W, HW, packs, rowsW, own.r0, src0, o00, meta);
    float Qprev[WRITE_GX ? NP * 4 : 1], xa[WANT_GS ? NP * 4 : 1], xb[WANT_GS ? NP * 4 : 1];
    float aT[WANT_GS ? NA : 1], aH[WANT_GS ? NA : 1], aW[WANT_GS ? NA : 1];
    if constexpr (WRITE_GX) {
#pragma unroll
        for (int e = 0; e < NP * 4; ++e) Qprev[e] = 0.f;
    }
    if constexpr (WANT_GS) {
#pragma unroll
        for (int e = 0; e < NP * 4; ++e) xa[e] = xb[e] = 0.f;
#pragma unroll
        for (int a = 0; a < NA; ++a) aT[a] = aH[a] = aW[a] = 0.f;
    }

    if (s_lo <= s_hi) {
        --s_lo;                                                  // the step before an element's window fetches its x[0]
        u32x4 r0 = {0u, 0u, 0u, 0u}, r1 = r0;
        int buf = 0;
        if (s_lo >= 0 && s_lo < T) {
            RK16_SLAB_LOAD(gg + (size_t)s_lo * tstride);
            RK16_SLAB_STORE(slab[0]);
        }
        __syncthreads();
        for (int s = s_lo; s <= s_hi; ++s, buf ^= 1) {
            const bool next = s + 1 >= 0 && s + 1 < T && s + 1 <= s_hi;
            if (next) RK16_SLAB_LOAD(gg + (size_t)(s + 1) * tstride);
            const bool valid = s >= 0 && s < T;
            const unsigned short* pl = slab[buf];
            // x[k + 1] of every pack enters its window at the end of this step: requested here, all packs at once, as packed bits
            uint2 xnp[WANT_GS ? NP : 1];
            if constexpr (WANT_GS) {
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    const int p = tid + k * kBlock;
                    xnp[k] = make_uint2(0u, 0u);
                    if (p >= packs) continue;
                    const bool whole = !ODD || ((meta[k * 4] ^ meta[k * 4 + 3]) & (63u << 4)) == 0;
                    const float4 tf0 = tab.f[(meta[k * 4] >> 4) & 63u];
                    if (whole) {
                        const int k1 = (meta[k * 4] & kActive) ? s - __float_as_int(tf0.w) + 1 : -1;
                        if (k1 >= 0 && k1 < T) xnp[k] = *reinterpret_cast<const uint2*>(x + base + (size_t)k1 * tstride + 4 * p);
                    } else {
                        unsigned b[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const unsigned m = meta[k * 4 + j];
                            const int k1 = (m & kActive) ? s - __float_as_int(entry<ODD>(tab, m, meta[k * 4], tf0).w) + 1 : -1;
                            b[j] = 0u;
                            if (k1 >= 0 && k1 < T)
                                b[j] = *reinterpret_cast<const unsigned short*>(x + base + (size_t)k1 * tstride + 4 * p + j);
                        }
                        xnp[k] = make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16));
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int p = tid + k * kBlock;
                if (p >= packs) continue;
                const bool whole = !ODD || ((meta[k * 4] ^ meta[k * 4 + 3]) & (63u << 4)) == 0;
                const float4 tf0 = tab.f[(meta[k * 4] >> 4) & 63u];
                float res[4], xn[4];
                int kk[4];                                       // position in the element's window: active for 0 .. T
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = k * 4 + j;
                    kk[j] = (meta[e] & kActive) ? s - __float_as_int(entry<ODD>(tab, meta[e], meta[k * 4], tf0).w) : -2;
                }
                if constexpr (WANT_GS) {
                    const float4 v = Cell4<S>::widen(xnp[k]);
                    xn[0] = v.x; xn[1] = v.y; xn[2] = v.z; xn[3] = v.w;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // every element runs the step's arithmetic (no divergent branch around the LDS reads: they would each
                    // wait for their own round trip); outside its window an element's results are dropped
                    const int e = k * 4 + j, a = ODD ? e : k;
                    const bool act = kk[j] >= 0 && kk[j] <= T;
                    const float4 tf = entry<ODD>(tab, meta[e], meta[k * 4], tf0);
                    const float rT = tf.x, rH = tf.y, rW = tf.z;
                    float q00 = 0.f, q01 = 0.f, q10 = 0.f, q11 = 0.f;
                    if (valid) taps<S>(pl, o00[e], meta[e], W, q00, q01, q10, q11);
                    const float la = q00 * (1 - rW) + q01 * rW, lb = q10 * (1 - rW) + q11 * rW;
                    const float Q = (1 - rH) * la + rH * lb;              // the reference's tree, contraction off
                    if constexpr (WANT_GS) {
                        const float QH = la - lb;
                        const float QW = ((1 - rH) * q00 + rH * q10) - ((1 - rH) * q01 + rH * q11);
                        const float dx = xb[e] - xa[e];
                        const float mx = (1 - rT) * xb[e] + rT * xa[e];
                        aT[a] += act ? Q * dx : 0.f;
                        aH[a] += act ? QH * mx : 0.f;
                        aW[a] += act ? QW * mx : 0.f;
                        const bool slide = kk[j] >= -1 && kk[j] <= T;
                        xa[e] = slide ? xb[e] : xa[e];
                        xb[e] = slide ? xn[j] : xb[e];
                    }
                    res[j] = 0.f;
                    if constexpr (WRITE_GX) {
                        res[j] = (1 - rT) * Qprev[e] + rT * Q;
                        Qprev[e] = act ? Q : Qprev[e];
                    }
                }
                if constexpr (WRITE_GX) {
                    if (whole) {
                        if (kk[0] >= 1 && kk[0] <= T)
                            *reinterpret_cast<uint2*>(gx + base + (size_t)(kk[0] - 1) * tstride + 4 * p) =
                                Cell4<S>::narrow(res[0], res[1], res[2], res[3]);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (kk[j] >= 1 && kk[j] <= T) st(gx + base + (size_t)(kk[j] - 1) * tstride + 4 * p + j, res[j]);
                    }
                }
            }
            if (next) RK16_SLAB_STORE(slab[buf ^ 1]);
            __syncthreads();
        }
    }

    if constexpr (WANT_GS) {
        // the terms of a channel are consecutive entries: summed by one wave in a fixed order
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int p = tid + k * kBlock;
            if (p >= packs) continue;
            if constexpr (ODD) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sums[0][4 * p + j] = aT[k * 4 + j]; sums[1][4 * p + j] = aH[k * 4 + j]; sums[2][4 * p + j] = aW[k * 4 + j];
                }
            } else {
                sums[0][p] = aT[k]; sums[1][p] = aH[k]; sums[2][p] = aW[k];
            }
        }
        __syncthreads();
        const int per = ODD ? rowsW : rowsW >> 2, lane = tid & (kWave - 1);
        for (int cl = tid / kWave; cl < Gl; cl += kBlock / kWave) {
            if (tab.i[cl].z) continue;
            float v[3] = {0.f, 0.f, 0.f};
            for (int i = lane; i < per; i += kWave)
#pragma unroll
                for (int q = 0; q < 3; ++q) v[q] += sums[q][cl * per + i];
#pragma unroll
            for (int q = 0; q < 3; ++q) v[q] = wave_sum(v[q]);
            if (lane == 0) {
                float* o = part + (size_t)(c0 + cl) * 3 * P + n * sd.bands + own.band;
                o[0] = v[0]; o[P] = v[1]; o[2 * P] = v[2];
            }
        }
    }
    // integer component: the reference's per-element formulation, the whole workgroup on one channel at a time (of a split
    // plane: band 0 does the column, the other bands contribute zero)
    for (int cl = 0; cl < Gl; ++cl) {
        if (!tab.i[cl].z) continue;
        const int c = c0 + cl;
        const bool mine = own.band == 0;
        if constexpr (WRITE_GX) {
            if (mine)
                for (int t = 0; t < T; ++t) backward_input_plane<float, false, S>(shift, gy, gx, d, n, t, c, tid, kBlock);
        }
        if constexpr (WANT_GS) {
            float bT = 0.f, bH = 0.f, bW = 0.f;
            if (mine)
                for (int to = 0; to < T; ++to) shift_grad_plane<float, NoAct, S>(x, shift, gy, d, n, to, c, tid, kBlock, bT, bH, bW);
            bT = group_sum(bT, kBlock, red[0]);
            bH = group_sum(bH, kBlock, red[1]);
            bW = group_sum(bW, kBlock, red[2]);
            if (tid == 0) {
                float* o = part + (size_t)c * 3 * P + n * sd.bands + own.band;
                o[0] = bT; o[P] = bH; o[2 * P] = bW;
            }
        }
    }
}

// ==================================================================================== stride (1,2,2)
// The 2x2 tap windows of a stride-2 layer tile the source plane at offset (flH, flW) (rk3d_stride2.hpp): every x element is a
// tap of exactly one output per source plane.
//   forward : the walk of k3d16_stream_forward over x slabs; a thread owns ONE pack of 4 consecutive outputs of the group's
//             Ho x Wo planes (a slab of 4096 source elements is 1024 outputs at most), tap (0,0) of output j at
//             cl*H*W + (2 ho + flH)*W + 2 (wo + j) + flW; a band of R output rows needs the 2R source rows 2 r0 + flH ..
//   backward: the walk of k3d16_stream_backward over gy slabs, on the INPUT side: a thread owns packs of 4 consecutive source
//             elements.  Through the stride un-mapping (unmap, rk3d_generic.hpp) an element (hi, wi) has at most one gy tap
//             per plane: with the negated shift (fl', r') and p = hi + fl'H, p even -> tap h0 = p / 2 with weight 1 - r'H
//             (the lower row of a window), p odd -> tap h1 = (p + 1) / 2 with weight r'H (the upper row); columns alike.  The
//             reference's trilinear tree with its seven zero taps is then  Q = wH (g wW),  gx[k-1] = (1-r'T) Q(s-1) + r'T Q(s)
//             (same roundings, as s2::backward_loop has it), and the face differences of d(shift) are -/+ (g wW) and
//             -/+ (wH g) times the x pairing of the stride-1 kernel.  An element no window covers has no tap: it stores zero
//             and adds nothing.  A band is 2R source rows; their taps lie in R + 1 gy rows at most.
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// a spatial floor beyond +-(2L + 4) reaches nothing, like any floor out there: clamped, index arithmetic cannot overflow
__device__ __forceinline__ int near_floor(int fl, int L) { return clampi(fl, -2 * L - 4, 2 * L + 4); }

struct S2Owned { int n, c0, Gl, band; };
__device__ __forceinline__ S2Owned s2_owned(const S2Dims& sd) {
    S2Owned o;
    int id = (int)blockIdx.x;
    o.band = id % sd.bands; id /= sd.bands;
    o.n = id / sd.groups;
    o.c0 = (id - o.n * sd.groups) * sd.G;
    o.Gl = sd.d.C - o.c0 < sd.G ? sd.d.C - o.c0 : sd.G;
    return o;
}

template <typename S>
__global__ __launch_bounds__(kBlock) void k3d16_s2_forward(const S* __restrict__ x, const float* __restrict__ shift,
                                                           S* __restrict__ y, S2Dims sd) {
    __shared__ __attribute__((aligned(16))) unsigned short slab[2][kSlabElems];
    __shared__ ChanTab tab;
    const Dims3& d = sd.d;
    const S2Owned own = s2_owned(sd);
    const int n = own.n, c0 = own.c0, Gl = own.Gl;
    const int HW = sd.HW, HWo = sd.HWo, T = d.T, H = d.H, W = d.W, Wo = d.Wo;
    const int ho0 = own.band * sd.R, rows = d.Ho - ho0 < sd.R ? d.Ho - ho0 : sd.R;     // output rows
    const int rowsWo = rows * Wo, packs = Gl * rowsWo >> 2;
    const size_t tin = (size_t)d.C * HW, tout = (size_t)d.C * HWo;

    int s_lo, s_hi;
    channel_table<false>(tab, shift, d.C, c0, Gl, T, s_lo, s_hi);
    int src0 = 0, src_elems = Gl * HW;
    if (sd.bands > 1) {                                              // one channel: the band's 2 * rows source rows, clipped
        const int fl = near_floor(tab.i[0].x, H);
        const int rs = clampi(2 * ho0 + fl, 0, H), re = clampi(2 * (ho0 + rows) + fl, 0, H);
        src0 = rs * W; src_elems = (re - rs) * W;
    }
    const int chunks = src_elems >> 3;
    const S* xg = x + ((size_t)n * T * d.C + c0) * HW + src0;            // the slab of (n, t = 0)
    S* yg = y + ((size_t)n * T * d.C + c0) * HWo + ho0 * Wo;             // the workgroup's rows of (n, t = 0)

    // the thread's pack: LDS offset of tap (0,0) of output 0 (output j: + 2 j), 4 validity bits per output, the channel
    const int p = (int)threadIdx.x;
    const bool mine = p < packs;
    int o00 = 0, flT = 0;
    unsigned mask = 0;
    float rT = 0.f, rH = 0.f, rW = 0.f;
    if (mine) {
        const int i = 4 * p;
        const int cl = i / rowsWo, rem = i - cl * rowsWo;
        const int hb = rem / Wo, wo = rem - hb * Wo;
        const int4 ti = tab.i[cl];
        const float4 tf = tab.f[cl];
        rT = tf.x; rH = tf.y; rW = tf.z; flT = __float_as_int(tf.w);
        const int h0 = 2 * (ho0 + hb) + near_floor(ti.x, H), wb = 2 * wo + near_floor(ti.y, W);
        const bool mh0 = h0 >= 0 && h0 < H, mh1 = h0 + 1 >= 0 && h0 + 1 < H;
        o00 = cl * HW + h0 * W + wb - src0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int w0 = wb + 2 * j;
            const bool mw0 = w0 >= 0 && w0 < W, mw1 = w0 + 1 >= 0 && w0 + 1 < W;
            mask |= ((mh0 && mw0 ? 1u : 0u) | (mh0 && mw1 ? 2u : 0u) | (mh1 && mw0 ? 4u : 0u) | (mh1 && mw1 ? 8u : 0u)) << (4 * j);
        }
    }
    float Bprev[4] = {0.f, 0.f, 0.f, 0.f};

    u32x4 r0 = {0u, 0u, 0u, 0u}, r1 = r0;
    int buf = 0;
    if (s_lo >= 0 && s_lo < T) {
        RK16_SLAB_LOAD(xg + (size_t)s_lo * tin);
        RK16_SLAB_STORE(slab[0]);
    }
    __syncthreads();
    for (int s = s_lo; s <= s_hi; ++s, buf ^= 1) {
        const bool next = s + 1 >= 0 && s + 1 < T && s + 1 <= s_hi;
        if (next) RK16_SLAB_LOAD(xg + (size_t)(s + 1) * tin);
        const bool valid = s >= 0 && s < T;
        const unsigned short* pl = slab[buf];
        if (mine) {
            float res[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float B = 0.f;
                if (valid) {
                    float q00, q01, q10, q11;
                    taps<S>(pl, o00 + 2 * j, (mask >> (4 * j)) & 15u, W, q00, q01, q10, q11);
                    B = (1 - rH) * (q00 * (1 - rW) + q01 * rW) + rH * (q10 * (1 - rW) + q11 * rW);
                }
                res[j] = (1 - rT) * Bprev[j] + rT * B;
                Bprev[j] = B;
            }
            const int to = s - flT - 1;
            if (to >= 0 && to < T)
                *reinterpret_cast<uint2*>(yg + (size_t)to * tout + 4 * p) = Cell4<S>::narrow(res[0], res[1], res[2], res[3]);
        }
        if (next) RK16_SLAB_STORE(slab[buf ^ 1]);
        __syncthreads();
    }
}

// element meta word of the backward: bit 0 the gy tap exists, bit 1 lower row of its window (tap h0, weight 1 - r'H),
// bit 2 right column (tap w0, weight 1 - r'W), bits 4-9 channel within the group, bit 10 active (kActive)
template <typename S, int NP, bool WRITE_GX, bool WANT_GS>
__global__ __launch_bounds__(kBlock) void k3d16_s2_backward(const S* __restrict__ x, const float* __restrict__ shift,
                                                            const S* __restrict__ gy, S* __restrict__ gx,
                                                            float* __restrict__ part, S2Dims sd) {
    // the gy slab twice; after the walk the same memory holds the d(shift) terms, one per pack
    constexpr int kSlabBytes = 2 * kS2GySlab * 2, kSumBytes = 3 * NP * kBlock * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[kSlabBytes > kSumBytes ? kSlabBytes : kSumBytes];
    __shared__ ChanTab tab;
    __shared__ float red[3][kBlock / kWave];
    unsigned short (*slab)[kS2GySlab] = reinterpret_cast<unsigned short (*)[kS2GySlab]>(smem);
    float (*sums)[NP * kBlock] = reinterpret_cast<float (*)[NP * kBlock]>(smem);
    const Dims3& d = sd.d;
    const int tid = threadIdx.x;
    const S2Owned own = s2_owned(sd);
    const int n = own.n, c0 = own.c0, Gl = own.Gl;
    const int HW = sd.HW, HWo = sd.HWo, T = d.T, H = d.H, W = d.W, Ho = d.Ho, Wo = d.Wo;
    const int r0 = 2 * own.band * sd.R, rows = H - r0 < 2 * sd.R ? H - r0 : 2 * sd.R;   // source rows
    const int rowsW = rows * W, packs = Gl * rowsW >> 2, P = d.N * sd.bands;
    const size_t tin = (size_t)d.C * HW, tout = (size_t)d.C * HWo;
    const size_t base = ((size_t)n * T * d.C + c0) * HW + r0 * W;        // the workgroup's rows of (n, t = 0)

    int s_lo, s_hi;
    channel_table<true>(tab, shift, d.C, c0, Gl, T, s_lo, s_hi);
    int src0 = 0, src_elems = Gl * HWo;
    if (sd.bands > 1) {                                              // one channel: the gy rows the band's taps lie in, clipped
        const int fl = near_floor(tab.i[0].x, H);
        const int gs = clampi((r0 + fl + 1) >> 1, 0, Ho), ge = clampi(((r0 + rows + fl) >> 1) + 1, 0, Ho);
        src0 = gs * Wo; src_elems = (ge - gs) * Wo;
    }
    const int chunks = src_elems >> 3;
    const S* gg = gy + ((size_t)n * T * d.C + c0) * HWo + src0;          // the slab of (n, t = 0)
    int og[NP * 4];
    unsigned meta[NP * 4];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int p = tid + k * kBlock;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = k * 4 + j;
            og[e] = 0; meta[e] = 0;
            if (p >= packs) continue;
            const int i = 4 * p + j;
            const int cl = i / rowsW, rem = i - cl * rowsW;
            const int hb = rem / W, hi = r0 + hb, wi = rem - hb * W;
            const int4 ti = tab.i[cl];
            const int ph = hi + near_floor(ti.x, H), pw = wi + near_floor(ti.y, W);
            const int ho = (ph + 1) >> 1, wo = (pw + 1) >> 1;
            const bool ok = ho >= 0 && ho < Ho && wo >= 0 && wo < Wo;
            og[e] = ok ? cl * HWo + ho * Wo + wo - src0 : 0;
            meta[e] = (ok ? 1u : 0u) | ((ph & 1) ? 0u : 2u) | ((pw & 1) ? 0u : 4u) | ((unsigned)cl << 4) | (ti.z ? 0u : kActive);
        }
    }
    float Qprev[WRITE_GX ? NP * 4 : 1], xa[WANT_GS ? NP * 4 : 1], xb[WANT_GS ? NP * 4 : 1];
    float aT[WANT_GS ? NP : 1], aH[WANT_GS ? NP : 1], aW[WANT_GS ? NP : 1];
    if constexpr (WRITE_GX) {
#pragma unroll
        for (int e = 0; e < NP * 4; ++e) Qprev[e] = 0.f;
    }
    if constexpr (WANT_GS) {
#pragma unroll
        for (int e = 0; e < NP * 4; ++e) xa[e] = xb[e] = 0.f;
#pragma unroll
        for (int a = 0; a < NP; ++a) aT[a] = aH[a] = aW[a] = 0.f;
    }

    if (s_lo <= s_hi) {
        --s_lo;                                                  // the step before an element's window fetches its x[0]
        u32x4 ahead = {0u, 0u, 0u, 0u};
        int buf = 0;
        if (s_lo >= 0 && s_lo < T) {
            ahead = chunk_load(gg + (size_t)s_lo * tout, tid, chunks);
            chunk_store(slab[0], tid, chunks, ahead);
        }
        __syncthreads();
        for (int s = s_lo; s <= s_hi; ++s, buf ^= 1) {
            const bool next = s + 1 >= 0 && s + 1 < T && s + 1 <= s_hi;
            if (next) ahead = chunk_load(gg + (size_t)(s + 1) * tout, tid, chunks);
            const bool valid = s >= 0 && s < T;
            const unsigned short* pl = slab[buf];
            // x[k + 1] of every pack enters its window at the end of this step: requested here, all packs at once, as packed bits
            uint2 xnp[WANT_GS ? NP : 1];
            if constexpr (WANT_GS) {
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    const int p = tid + k * kBlock;
                    xnp[k] = make_uint2(0u, 0u);
                    if (p >= packs) continue;
                    const float4 tf = tab.f[(meta[k * 4] >> 4) & 63u];
                    const int k1 = (meta[k * 4] & kActive) ? s - __float_as_int(tf.w) + 1 : -1;
                    if (k1 >= 0 && k1 < T) xnp[k] = *reinterpret_cast<const uint2*>(x + base + (size_t)k1 * tin + 4 * p);
                }
            }
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int p = tid + k * kBlock;
                if (p >= packs) continue;
                const float4 tf = tab.f[(meta[k * 4] >> 4) & 63u];
                const float rT = tf.x, rH = tf.y, rW = tf.z;
                const int kk = (meta[k * 4] & kActive) ? s - __float_as_int(tf.w) : -2;    // position in the pack's window: active for 0 .. T
                const bool act = kk >= 0 && kk <= T;
                float res[4], xn[4];
                if constexpr (WANT_GS) {
                    const float4 v = Cell4<S>::widen(xnp[k]);
                    xn[0] = v.x; xn[1] = v.y; xn[2] = v.z; xn[3] = v.w;
                }
                // the pack's four taps, issued together (one that does not exist reads element 0 and is masked at use)
                unsigned short gv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) gv[j] = pl[og[k * 4 + j]];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = k * 4 + j;
                    const unsigned m = meta[e];
                    const float g = (valid && (m & 1u)) ? widen1<S>(gv[j]) : 0.f;
                    const float wH = (m & 2u) ? 1 - rH : rH, wW = (m & 4u) ? 1 - rW : rW;
                    const float gw = g * wW;
                    const float Q = wH * gw;                              // the reference's tree with its one live tap
                    if constexpr (WANT_GS) {
                        const float QH = (m & 2u) ? gw : -gw;             // lower row: the large face
                        const float gh = wH * g;
                        const float QW = (m & 4u) ? gh : -gh;
                        const float dx = xb[e] - xa[e];
                        const float mx = (1 - rT) * xb[e] + rT * xa[e];
                        aT[k] += act ? Q * dx : 0.f;
                        aH[k] += act ? QH * mx : 0.f;
                        aW[k] += act ? QW * mx : 0.f;
                        const bool slide = kk >= -1 && kk <= T;
                        xa[e] = slide ? xb[e] : xa[e];
                        xb[e] = slide ? xn[j] : xb[e];
                    }
                    res[j] = 0.f;
                    if constexpr (WRITE_GX) {
                        res[j] = (1 - rT) * Qprev[e] + rT * Q;
                        Qprev[e] = act ? Q : Qprev[e];
                    }
                }
                if constexpr (WRITE_GX) {
                    if (kk >= 1 && kk <= T)
                        *reinterpret_cast<uint2*>(gx + base + (size_t)(kk - 1) * tin + 4 * p) =
                            Cell4<S>::narrow(res[0], res[1], res[2], res[3]);
                }
            }
            if (next) chunk_store(slab[buf ^ 1], tid, chunks, ahead);
            __syncthreads();
        }
    }

    if constexpr (WANT_GS) {
        // the terms of a channel are consecutive entries: summed by one wave in a fixed order
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int p = tid + k * kBlock;
            if (p >= packs) continue;
            sums[0][p] = aT[k]; sums[1][p] = aH[k]; sums[2][p] = aW[k];
        }
        __syncthreads();
        const int per = rowsW >> 2, lane = tid & (kWave - 1);
        for (int cl = tid / kWave; cl < Gl; cl += kBlock / kWave) {
            if (tab.i[cl].z) continue;
            float v[3] = {0.f, 0.f, 0.f};
            for (int i = lane; i < per; i += kWave)
#pragma unroll
                for (int q = 0; q < 3; ++q) v[q] += sums[q][cl * per + i];
#pragma unroll
            for (int q = 0; q < 3; ++q) v[q] = wave_sum(v[q]);
            if (lane == 0) {
                float* o = part + (size_t)(c0 + cl) * 3 * P + n * sd.bands + own.band;
                o[0] = v[0]; o[P] = v[1]; o[2 * P] = v[2];
            }
        }
    }
    // integer component: the reference's per-element formulation, as in the stride-1 kernel
    for (int cl = 0; cl < Gl; ++cl) {
        if (!tab.i[cl].z) continue;
        const int c = c0 + cl;
        const bool mine = own.band == 0;
        if constexpr (WRITE_GX) {
            if (mine)
                for (int t = 0; t < T; ++t) backward_input_plane<float, false, S>(shift, gy, gx, d, n, t, c, tid, kBlock);
        }
        if constexpr (WANT_GS) {
            float bT = 0.f, bH = 0.f, bW = 0.f;
            if (mine)
                for (int to = 0; to < T; ++to) shift_grad_plane<float, NoAct, S>(x, shift, gy, d, n, to, c, tid, kBlock, bT, bH, bW);
            bT = group_sum(bT, kBlock, red[0]);
            bH = group_sum(bH, kBlock, red[1]);
            bW = group_sum(bW, kBlock, red[2]);
            if (tid == 0) {
                float* o = part + (size_t)c * 3 * P + n * sd.bands + own.band;
                o[0] = bT; o[P] = bH; o[2 * P] = bW;
            }
        }
    }
}

#undef RK16_SLAB_LOAD
#undef RK16_SLAB_STORE

// ----------------------------------------------------------------------------------- launchers
namespace {

template <typename S>
void stream_forward(const Cfg3& c, const SDims& s, const S* x, const float* shift, S* y, hipStream_t stream) {
    const dim3 grid(c.grid), block(kBlock);
    if (c.v[3]) hipLaunchKernelGGL((k3d16_stream_forward<S, 2, true>), grid, block, 0, stream, x, shift, y, s);
    else if (c.v[2] == 2) hipLaunchKernelGGL((k3d16_stream_forward<S, 2, false>), grid, block, 0, stream, x, shift, y, s);
    else hipLaunchKernelGGL((k3d16_stream_forward<S, 4, false>), grid, block, 0, stream, x, shift, y, s);
}

template <typename S, bool GX, bool GS>
void stream_backward(const Cfg3& c, const SDims& s, const S* x, const float* shift, const S* gy, S* gx, float* ws, hipStream_t stream) {
    const dim3 grid(c.grid), block(kBlock);
    if (c.v[3]) hipLaunchKernelGGL((k3d16_stream_backward<S, 2, true, GX, GS>), grid, block, 0, stream, x, shift, gy, gx, ws, s);
    else if (c.v[2] == 2) hipLaunchKernelGGL((k3d16_stream_backward<S, 2, false, GX, GS>), grid, block, 0, stream, x, shift, gy, gx, ws, s);
    else hipLaunchKernelGGL((k3d16_stream_backward<S, 4, false, GX, GS>), grid, block, 0, stream, x, shift, gy, gx, ws, s);
}
template <typename S>
void stream_backward(const Cfg3& c, const SDims& s, const S* x, const float* shift, const S* gy, S* gx, float* ws, hipStream_t stream) {
    if (c.v[0] && c.v[1]) stream_backward<S, true, true>(c, s, x, shift, gy, gx, ws, stream);
    else if (c.v[0]) stream_backward<S, true, false>(c, s, x, shift, gy, gx, ws, stream);
    else stream_backward<S, false, true>(c, s, x, shift, gy, gx, ws, stream);
}

template <typename S, bool GX, bool GS>
void s2_backward(const Cfg3& c, const S2Dims& s, const S* x, const float* shift, const S* gy, S* gx, float* ws, hipStream_t stream) {
    const dim3 grid(c.grid), block(kBlock);
    if (c.v[2] == 2) hipLaunchKernelGGL((k3d16_s2_backward<S, 2, GX, GS>), grid, block, 0, stream, x, shift, gy, gx, ws, s);
    else hipLaunchKernelGGL((k3d16_s2_backward<S, 4, GX, GS>), grid, block, 0, stream, x, shift, gy, gx, ws, s);
}
template <typename S>
void s2_backward(const Cfg3& c, const S2Dims& s, const S* x, const float* shift, const S* gy, S* gx, float* ws, hipStream_t stream) {
    if (c.v[0] && c.v[1]) s2_backward<S, true, true>(c, s, x, shift, gy, gx, ws, stream);
    else if (c.v[0]) s2_backward<S, true, false>(c, s, x, shift, gy, gx, ws, stream);
    else s2_backward<S, false, true>(c, s, x, shift, gy, gx, ws, stream);
}

template <typename S>
void generic_forward(const Cfg3& c, const Dims3& d, const S* x, const float* shift, S* y, hipStream_t stream) {
    const dim3 grid(c.grid), block(kBlock);
    if (c.v[0]) hipLaunchKernelGGL((k3d_forward_generic<float, true, S>), grid, block, 0, stream, x, shift, y, d);
    else hipLaunchKernelGGL((k3d_forward_generic<float, false, S>), grid, block, 0, stream, x, shift, y, d);
}
template <typename S>
void generic_backward_input(const Cfg3& c, const Dims3& d, const float* shift, const S* gy, S* gx, hipStream_t stream) {
    const dim3 grid(c.grid), block(kBlock);
    if (c.v[0]) hipLaunchKernelGGL((k3d_backward_input_generic<float, true, S>), grid, block, 0, stream, shift, gy, gx, d);
    else hipLaunchKernelGGL((k3d_backward_input_generic<float, false, S>), grid, block, 0, stream, shift, gy, gx, d);
}

}  // namespace

using bf16_t = __hip_bfloat16;

void launch_stream_forward(const Cfg3& c, const SDims& s, bool bf16, const void* x, const float* shift, void* y, hipStream_t stream) {
    if (bf16) stream_forward<bf16_t>(c, s, (const bf16_t*)x, shift, (bf16_t*)y, stream);
    else stream_forward<__half>(c, s, (const __half*)x, shift, (__half*)y, stream);
}
void launch_stream_backward(const Cfg3& c, const SDims& s, bool bf16, const void* x, const float* shift, const void* gy, void* gx,
                            float* ws, hipStream_t stream) {
    if (bf16) stream_backward<bf16_t>(c, s, (const bf16_t*)x, shift, (const bf16_t*)gy, (bf16_t*)gx, ws, stream);
    else stream_backward<__half>(c, s, (const __half*)x, shift, (const __half*)gy, (__half*)gx, ws, stream);
}
void launch_s2_forward(const Cfg3& c, const S2Dims& s, bool bf16, const void* x, const float* shift, void* y, hipStream_t stream) {
    const dim3 grid(c.grid), block(kBlock);
    if (bf16) hipLaunchKernelGGL((k3d16_s2_forward<bf16_t>), grid, block, 0, stream, (const bf16_t*)x, shift, (bf16_t*)y, s);
    else hipLaunchKernelGGL((k3d16_s2_forward<__half>), grid, block, 0, stream, (const __half*)x, shift, (__half*)y, s);
}
void launch_s2_backward(const Cfg3& c, const S2Dims& s, bool bf16, const void* x, const float* shift, const void* gy, void* gx,
                        float* ws, hipStream_t stream) {
    if (bf16) s2_backward<bf16_t>(c, s, (const bf16_t*)x, shift, (const bf16_t*)gy, (bf16_t*)gx, ws, stream);
    else s2_backward<__half>(c, s, (const __half*)x, shift, (const __half*)gy, (__half*)gx, ws, stream);
}
void launch_generic_forward(const Cfg3& c, const Dims3& d, bool bf16, const void* x, const float* shift, void* y, hipStream_t stream) {
    if (bf16) generic_forward<bf16_t>(c, d, (const bf16_t*)x, shift, (bf16_t*)y, stream);
    else generic_forward<__half>(c, d, (const __half*)x, shift, (__half*)y, stream);
}
void launch_generic_backward_input(const Cfg3& c, const Dims3& d, bool bf16, const float* shift, const void* gy, void* gx,
                                   hipStream_t stream) {
    if (bf16) generic_backward_input<bf16_t>(c, d, shift, (const bf16_t*)gy, (bf16_t*)gx, stream);
    else generic_backward_input<__half>(c, d, shift, (const __half*)gy, (__half*)gx, stream);
}
void launch_generic_backward_shift(const Cfg3& c, const Dims3& d, bool bf16, const void* x, const float* shift, const void* gy,
                                   float* ws, hipStream_t stream) {
    const dim3 grid(c.grid), block(kBlock);
    if (bf16)
        hipLaunchKernelGGL((k3d_backward_shift_generic<float, bf16_t>), grid, block, 0, stream, (const bf16_t*)x, shift,
                           (const bf16_t*)gy, ws, d);
    else
        hipLaunchKernelGGL((k3d_backward_shift_generic<float, __half>), grid, block, 0, stream, (const __half*)x, shift,
                           (const __half*)gy, ws, d);
}

}  // namespace s16
}  // namespace rk
