// rk3d_16.hpp -- RubiksShift3D on 16-bit activations (bf16 / f16) with the shift table and d(shift) in fp32: the geometry
// plan3d::plan (rk3d_plan.hpp) asks for and the launchers rk3d.hip calls.  The kernels are in rk3d_16.hip.
//
// Three families, the same fp32 arithmetic as the fp32 operator (the trees of rk3d_generic.hpp, contraction off), the result
// rounded to the storage type once, on store:
//   generic    the K1 / K3-K4 / K2 plane kernels of rk3d_generic.hpp at storage S, compute float: any stride / padding,
//              quantize, misaligned tensors; d(shift) as fp32 partials ws[C][3][N * To]
//   streaming  stride 1 / pad 0, quantize off, 16-byte aligned tensors: a workgroup owns one (n, c0 .. c0+G-1) channel
//              group and walks t; for fixed (n, t) the G planes are one contiguous slab of G*H*W*2 bytes, fetched with
//              16-byte loads, held in LDS twice over (plane t+1 lands while plane t is consumed); one partial per (n, c)
//              and component, ws[C][3][N].  A plane too large for a slab (112x112) is split into bands of R rows, one
//              channel and one band per workgroup, the band's R + 1 source rows in LDS: ws[C][3][N * bands]
//   streaming, stride (1,2,2) / pad 0, quantize off, 16-byte aligned tensors, W % 8 == 0 and even H (112 -> 56 and 56 -> 28
//              in the networks): the same walk over the planes of a channel group or of one channel's row band.  The 2x2 tap
//              windows of such a layer tile the source plane, so a band of R output rows is exactly 2R source rows.
//              forward : the slab is the x planes, a thread owns 4 consecutive outputs
//              backward: the slab is the gy planes (a quarter of the size), a thread owns packs of 4 consecutive SOURCE
//                        elements, each of which has one gy tap per plane at most -- x is loaded and d(x) stored in aligned
//                        8-byte packs, an element no window covers gets its zero like any other
//              Partials ws[C][3][N * bands] as above.
// All leave the row-sum + K5 to k3d_finalize<float>, a launch of its own.
#pragma once
#include "rk3d_generic.hpp"

namespace rk {
namespace s16 {

constexpr int kMaxG = 32;            // channels of a group at most
constexpr int kSlabElems = 4096;     // elements of a slab at most: 16 per thread, as 4 packs of 4 consecutive elements
constexpr int kSlabElemsOdd = 2048;  // ... when H*W % 4 != 0 (packs straddle channels: per-element d(shift) sums)
// Small planes take smaller groups than would fit: a group is one workgroup's serial walk, and [32,8,288,14,14] in groups
// of 16 is 576 workgroups for 256 CUs.  Planes of <= 256 elements: groups of <= 2048 elements (G = 8 at 14x14), <= 1024 when
// H*W % 4 != 0 (G = 16 at 7x7).
constexpr int kSmallPlane = 256;

struct SDims {
    Dims3 d;
    int HW, G, groups;               // G channels per workgroup, groups = ceil(C / G) per clip
    int R, bands;                    // rows per workgroup and workgroups per plane: H, 1 unless the plane is split (then G = 1)
};

// false: not for the streaming kernels (pointer alignment aside, which the planner checks).  v[2] = packs per thread
// (2 or 4), v[3] = H*W % 4 != 0.  Every slab -- the ragged last group's too -- starts 16-byte aligned and is a whole number
// of 16-byte chunks: C*H*W and G*H*W are multiples of 8 elements (split planes: W is).
inline bool geometry(SDims& s, Cfg3& c, const Dims3& d) {
    if (!s1p0(d)) return false;
    const long long HW = (long long)d.H * d.W;
    const int cap = HW % 4 == 0 ? kSlabElems : kSlabElemsOdd;
    int G = 1, R = d.H, bands = 1, slab;
    if (HW > cap) {                                       // row bands: R + 1 source rows of one channel fit the slab
        if (d.W % 8 != 0 || 2 * d.W > kSlabElems) return false;
        bands = (d.H + kSlabElems / d.W - 2) / (kSlabElems / d.W - 1);
        R = (d.H + bands - 1) / bands;
        bands = (d.H + R - 1) / R;
        slab = (R + 1) * d.W;
    } else {
        const int fill = HW > kSmallPlane ? cap : cap / 2;
        while (G * 2 <= kMaxG && G * 2 * HW <= fill) G *= 2;
        if (G * HW % 8 != 0 || (long long)d.C * HW % 8 != 0) return false;
        slab = G * (int)HW;
    }
    s.d = d;
    s.HW = (int)HW; s.G = G; s.groups = (d.C + G - 1) / G;
    s.R = R; s.bands = bands;
    const long long grid = (long long)d.N * s.groups * bands;
    if (grid > 0x7fffffffLL) return false;
    c.v[2] = slab / 4 <= 2 * kBlock ? 2 : 4;
    c.v[3] = HW % 4 != 0;
    c.grid = (unsigned)grid;
    c.lds = 0;
    return true;
}

// The stride (1,2,2) streaming family.  R: output rows per band (the backward's band is the 2R source rows under them).
struct S2Dims {
    Dims3 d;
    int HW, HWo, G, groups;
    int R, bands;
};
constexpr int kS2GySlab = 2048;      // elements of a gy slab at most: a quarter of kSlabElems, or the R + 1 rows a band can touch

// false: not for these kernels (pointer alignment aside).  v[2] = packs per thread (forward: 1 pack of 4 outputs, backward:
// 2 or 4 packs of 4 source elements), v[3] = channels per group.  Every slab of x and of gy starts 16-byte aligned and is
// whole 16-byte chunks: H*W is a multiple of 8 elements, C*Ho*Wo and G*Ho*Wo must be (split planes: Wo must be).
inline bool geometry_s2(S2Dims& s, Cfg3& c, const Dims3& d, bool backward) {
    if (!s122p0(d) || d.W % 8 != 0 || d.Wo % 4 != 0 || d.H % 2 != 0) return false;
    const long long HW = (long long)d.H * d.W, HWo = (long long)d.Ho * d.Wo;
    int G = 1, R = d.Ho, bands = 1, owned;
    if (HW > kSlabElems) {                                // row bands: the 2R source rows of one channel fit the slab
        if (d.Wo % 8 != 0 || 2 * d.W > kSlabElems) return false;
        const int rmax = kSlabElems / (2 * d.W);
        bands = (d.Ho + rmax - 1) / rmax;
        R = (d.Ho + bands - 1) / bands;
        bands = (d.Ho + R - 1) / R;
        owned = 2 * R * d.W;
    } else {
        const int fill = HW > kSmallPlane ? kSlabElems : kSlabElems / 2;
        while (G * 2 <= kMaxG && G * 2 * HW <= fill) G *= 2;
        if (G * HWo % 8 != 0 || (long long)d.C * HWo % 8 != 0) return false;
        owned = G * (int)HW;
    }
    const long long grid = (long long)d.N * ((d.C + G - 1) / G) * bands;
    if (grid > 0x7fffffffLL) return false;
    s.d = d;
    s.HW = (int)HW; s.HWo = (int)HWo; s.G = G; s.groups = (d.C + G - 1) / G;
    s.R = R; s.bands = bands;
    c.v[2] = !backward ? 1 : (owned / 4 <= 2 * kBlock ? 2 : 4);
    c.v[3] = G;
    c.grid = (unsigned)grid;
    c.lds = 0;
    return true;
}

// The launchers run the configuration they are given.  bf16: the storage type is bf16, else f16.
// streaming forward; v = -, -, packs per thread, odd
void launch_stream_forward(const Cfg3& c, const SDims& s, bool bf16, const void* x, const float* shift, void* y, hipStream_t stream);
// streaming backward; v = WRITE_GX, d(shift) wanted, packs per thread, odd; partials ws[C][3][N * bands]
void launch_stream_backward(const Cfg3& c, const SDims& s, bool bf16, const void* x, const float* shift, const void* gy, void* gx,
                            float* ws, hipStream_t stream);
// stride (1,2,2) streaming forward / backward; v = WRITE_GX, d(shift) wanted (backward), packs per thread, channels per group
void launch_s2_forward(const Cfg3& c, const S2Dims& s, bool bf16, const void* x, const float* shift, void* y, hipStream_t stream);
void launch_s2_backward(const Cfg3& c, const S2Dims& s, bool bf16, const void* x, const float* shift, const void* gy, void* gx,
                        float* ws, hipStream_t stream);
// generic kernels; v[0] = QUANT (forward, d(x)); partials ws[C][3][N * To]
void launch_generic_forward(const Cfg3& c, const Dims3& d, bool bf16, const void* x, const float* shift, void* y, hipStream_t stream);
void launch_generic_backward_input(const Cfg3& c, const Dims3& d, bool bf16, const float* shift, const void* gy, void* gx,
                                   hipStream_t stream);
void launch_generic_backward_shift(const Cfg3& c, const Dims3& d, bool bf16, const void* x, const float* shift, const void* gy,
                                   float* ws, hipStream_t stream);

}  // namespace s16
}  // namespace rk
