// rk3d_slab.hpp -- host entry points of the small-plane RubiksShift3D kernels (rk3d_slab.hip) for plan3d (rk3d_plan.hpp) and
// rk3d.hip: geometry functions (false = not for these kernels; the planner has checked stride / padding, alignment and the
// switches) and launchers, which run the configuration they are given.
#pragma once
#include "rk3d_dma.hpp"

namespace rk {
namespace slab3d {

struct SDims {
    int N, T, C, H, W, HW;
    int slab;                     // C * HW: elements of one (n, t)
    int nchunks;                  // ceil(slab / (256 M))
};
struct S2Dims {
    int N, T, C, H, W, HW, Wo, HWo;
    int slab_in, slab_out;        // C * HW, C * HWo
    int nchunks;                  // ceil(slab_in / 1024)
};

// stride 1 / pad 0, planes of 16 .. 256 elements up to 15 wide, T <= 8.  c: v[2] = HALO, grid (the producers: a FUSED
// backward launch adds C finalizer blocks), lds; P = 2 * N
bool geometry(SDims& s, Cfg3& c, const Dims3& d, bool backward);
// v = NEGATE (false: src = x, dst = y; true, d(x) alone: src = gy, dst = gx), -, HALO
void launch_interp(const Cfg3& c, const SDims& s, const Dims3& d, const float* src, const float* shift, float* dst, hipStream_t stream);
// v = WRITE_GX, FUSED (row-sum + K5 inside the launch, ws = granule pairs; else plain partials ws[C][3][P]), HALO
void launch_bwd(const Cfg3& c, const SDims& s, const Dims3& d, const float* x, const float* shift, const float* gy, float* gx, float* ws,
                const dma3d::Fin3& fin, hipStream_t stream);

// the same for stride (1,2,2) / pad 0 on even planes up to 56 wide (the layers rk3d_stride2.hpp does not take: 28 -> 14, 14 -> 7)
bool geometry_s2(S2Dims& s, Cfg3& c, const Dims3& d, bool backward);
void launch_fwd_s2(const Cfg3& c, const S2Dims& s, const Dims3& d, const float* x, const float* shift, float* y, hipStream_t stream);
void launch_bwd_s2(const Cfg3& c, const S2Dims& s, const Dims3& d, const float* x, const float* shift, const float* gy, float* gx,
                   float* ws, const dma3d::Fin3& fin, hipStream_t stream);

}  // namespace slab3d
}  // namespace rk
