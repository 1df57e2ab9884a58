// rk2d_plan.hpp -- which kernels run a RubiksShift2D call.  plan2d::plan holds every eligibility rule and the order in which
// the families are considered; it is a pure host function (no HIP call, no environment, no pointers: the alignment of each
// operand, the switch and the CU count as arguments), so rk_debug_2d_plan can show the choice on a machine without a device
// and tests/test_plan2d.py holds it against the dispatch it replaced.  The families' headers supply the geometry (false = not
// for these kernels) and launchers that run what they are given; rk2d.hip validates, plans and switches over the plan.
#pragma once
#include "rk2d_generic.hpp"
#include "rk2d_dma.hpp"
#include "rk2d_stage.hpp"
#include "rk2d_raw16.hpp"
#include "rk2d_tile.hpp"
#include "rk2d_column.hpp"

namespace rk {
namespace plan2d {

using g2d::Cfg2;
using g2d::Dims2;

enum Family {                 // the kernel template of a launch; Launch::c holds its variant
    kNone, kGenFwd, kGenBwdX, kGenBwdS, kFinalize, kFinalizeBn, kDmaInterp, kDmaBwd, kStageInterp, kStageBwd, kRawInterp, kRawBwd,
    kTileInterp, kTileBwd, kColFwd, kColBwd
};
enum Form { kForward, kBackward, kForwardBn, kBackwardBn };
enum Operand { kX, kY, kGx, kBn };            // x / z, y (forward) or gy, gx / dz, the BN pack (backward: abmi)

struct Switches { ShiftKernels kernels; int cus; };     // RK_SHIFT_KERNELS (rk_common.hpp), the device's compute units

struct Call {
    Dims2 d;
    Form form;
    int elem;                 // 4: fp32, 8: fp64, 2: bf16 / f16 activations (shift table of the same type or, rk2d_*_sf32, fp32)
    bool quantize, gshift;    // backward: d(shift) wanted (the BN backward always wants it)
    int align[4];             // per Operand: 16, 8 or 0 -- the largest of these its address is a multiple of; an operand the
                              // call does not have counts as 16
};
struct Launch {
    Family family;
    Cfg2 c;
    union { dma2d::FDims band; tile2d::TDims2 tile; col2d::C2Dims col; Dims2 gen; } g;
};
struct Plan {
    int rc;                   // RK_OK, or RK_ERR_UNSUPPORTED (the BN forms: no fused kernel covers the call)
    int n;
    Launch l[3];              // in launch order
    int P;                    // partials per channel and sum of the d(shift) launch: ws[C][2 or 4][P]; 0: no d(shift)
    bool finalize;            // k2d_finalize / k2d_finalize_bn is a launch of its own (else: inside the d(shift) launch)
};

inline void set_group(Dims2& d, int plane_elems) {
    d.E = pow2_at_least(plane_elems, kWave, kBlock);
    d.logE = (d.E == 64) ? 6 : (d.E == 128 ? 7 : 8);
}
inline unsigned grid_for(const Dims2& d) {
    const int per_block = kBlock / d.E;
    return (unsigned)(((long long)d.N * d.C + per_block - 1) / per_block);
}
// the fp32 LDS-DMA backward streams this shape (its ring within 64 KB)
inline bool dma_backward_geometry(dma2d::FDims& f, const Dims2& d) {
    return dma2d::make_fdims(f, d, dma2d::kFramesF32, true) && dma::bwd_ring_bytes(f.b, 1, 1) <= 64 * 1024;
}

// (a geometry function writes to the launch only when it takes the call)
inline Plan plan(const Call& c, const Switches& sw) {
    const Dims2& d = c.d;
    Plan pl{};
    const bool bn = c.form == kForwardBn || c.form == kBackwardBn, backward = c.form == kBackward || c.form == kBackwardBn;
    const bool fused = backward && (c.gshift || bn);                   // d(x) + d(shift) in one launch
    const bool streaming = sw.kernels == ShiftKernels::Auto && !c.quantize && c.elem != 8;
    const bool column = sw.kernels != ShiftKernels::Generic && !c.quantize;     // rk2d_column.hpp
    auto take = [&pl](Family f, Launch& l) { l.family = f; pl.l[pl.n++] = l; return true; };
    // every operand the streaming kernel of this form touches is a multiple of `bytes` (the BN backward's pack: of 16)
    auto aligned = [&](int bytes) {
        if (!backward) return c.align[kX] >= bytes && c.align[kY] >= bytes;
        if (!fused) return c.align[kY] >= bytes && c.align[kGx] >= bytes;
        return c.align[kX] >= bytes && c.align[kY] >= bytes && c.align[kGx] >= bytes && (!bn || c.align[kBn] >= 16);
    };
    // forward (src = x, dst = y), d(x) alone (negate: src = gy, dst = gx) or the fused backward (row-sum + K9 inside the launch;
    // sets P) in one streaming launch, stride 1 / pad 0
    auto streams = [&] {
        if (!streaming) return false;
        Launch l{};
        l.c.negate = backward && !fused; l.c.bn = bn;
        auto done = [&](Family f, int producers, int P, size_t lds) {
            l.c.lds = lds;
            l.c.grid = (unsigned)(producers + (fused ? d.C : 0));      // the finalizer blocks
            if (fused) pl.P = P;
            return take(f, l);
        };
        auto bands = [&](Family f, size_t lds) {
            const dma2d::FDims& b = l.g.band;
            const int r = dma::rounds_of(b.b);
            l.c.rounds = r >= 1 && r <= 3 ? r : 4;
            return done(f, b.ngroups * b.b.C * b.b.nbands, b.ngroups * b.b.nbands, lds);
        };
        auto ring = [&] { return fused ? dma::bwd_ring_bytes(l.g.band.b, 1, 1) : dma::interp_ring_bytes(l.g.band.b, dma2d::kInterpDepth); };
        // 14x14 planes
        if (aligned(16) && (c.elem == 4 ? tile2d::make_tdims<float, 14, 14>(l.g.tile, d, fused, sw.cus)
                                        : tile2d::make_tdims<__hip_bfloat16, 14, 14>(l.g.tile, d, fused, sw.cus))) {
            const long long waves = (long long)l.g.tile.NG * l.g.tile.ngroups;
            return done(fused ? kTileBwd : kTileInterp, (int)((waves + 3) / 4), l.g.tile.ngroups,
                        fused ? tile2d::backward_lds() : tile2d::interp_lds());
        }
        if (c.elem == 4)                                               // W % 4 == 0 (no BN variant: rk_bn_apply_affine_* + these win)
            return !bn && aligned(16) && dma2d::make_fdims(l.g.band, d, dma2d::kFramesF32, fused) && ring() <= 64 * 1024 &&
                   bands(fused ? kDmaBwd : kDmaInterp, ring());
        if (aligned(16) && raw16::make_fdims8(l.g.band, d, fused ? raw16::kFramesRaw16 : raw16::kFramesRaw16Fwd) && ring() <= 64 * 1024)
            return bands(fused ? kRawBwd : kRawInterp, ring());        // raw 16-bit planes, W % 8 == 0: 56 x 56, 112 x 112
        return aligned(8) && dma2d::make_fdims(l.g.band, d, dma2d::kFrames16) &&    // register-staged: other W % 4 == 0 (28 x 28)
               bands(fused ? kStageBwd : kStageInterp, stage2d::ring_bytes(l.g.band.b));
    };
    auto generic = [&](Family f, int plane_elems, int quant) {
        Launch l{};
        l.c.quant = quant;
        l.g.gen = d;
        set_group(l.g.gen, plane_elems);
        l.c.grid = grid_for(l.g.gen);
        return take(f, l);
    };
    auto col_forward = [&] {
        Launch l{};
        l.g.col = col2d::make_c2dims(d, d.Ho * d.Wo);
        l.c.bn = bn; l.c.M = l.g.col.M;
        l.c.vec = l.g.col.M == 4 && (d.Ho * d.Wo) % 4 == 0 && c.align[kY] >= 16;
        l.c.grid = col2d::grid_of(l.g.col);
        return take(kColFwd, l);
    };
    auto finalize = [&](Family f) {                                    // row-sum of the P partials per channel + K9
        Launch l{};
        l.c.grid = (unsigned)d.C;
        pl.finalize = true;
        return take(f, l);
    };
    auto col_backward = [&] {                                          // fused d(x) + d(shift), any stride / H x W
        Launch l{};
        l.g.col = col2d::make_c2dims(d, d.H * d.W);
        l.c.bn = bn; l.c.M = l.g.col.M;
        l.c.single = d.sH >= 2 && d.sW >= 2;
        l.c.vec = l.g.col.M == 4 && (d.H * d.W) % 4 == 0 && c.align[kX] >= 16 && c.align[kGx] >= 16;
        l.c.grid = col2d::grid_of(l.g.col);
        pl.P = l.g.col.ngroups * l.g.col.nchunks;
        take(kColBwd, l);
        return finalize(bn ? kFinalizeBn : kFinalize);
    };

    if (bn) {
        // the column kernels' fused variants take what no streaming kernel does (fp32 planes the LDS-DMA kernels stream keep the
        // normalise pass + those kernels: they are the faster pair there)
        dma2d::FDims f;
        const bool col_bn_takes = column && !(c.elem == 4 && sw.kernels == ShiftKernels::Auto && dma_backward_geometry(f, d));
        if (c.quantize || !(streams() || (col_bn_takes && (backward ? col_backward() : col_forward())))) pl.rc = RK_ERR_UNSUPPORTED;
        return pl;
    }
    if (streams()) return pl;
    if (!backward) {
        // small planes only: on larger ones the per-plane kernel below is the faster forward (stride-2 56x56 ->
        // 28x28: 85 vs 102 us); the column BACKWARD wins everywhere (fused, single-tap)
        // (16-bit strided layers: the column kernel with 8-byte stores also wins on the large planes, 108 -> 84 us at
        // [256,108,56,56] bf16; in fp32 it loses there, 84 -> 97 us)
        if (column && (d.Ho * d.Wo <= kBlock || (c.elem == 2 && (d.sH > 1 || d.sW > 1)))) col_forward();
        else generic(kGenFwd, d.Ho * d.Wo, c.quantize);
        return pl;
    }
    if (c.gshift && column) return col_backward(), pl;
    if (c.gshift) {                                                    // rubiks.cpp:126-149
        generic(kGenBwdS, d.Ho * d.Wo, 0);
        pl.P = d.N;
        finalize(kFinalize);
    }
    generic(kGenBwdX, d.H * d.W, c.quantize);                                      // rubiks.cpp:151-153
    return pl;
}

// bytes of d(shift) partials a caller provides before the call (the BN backward: twice that -- four sums per partial instead
// of two): [C][2][P] with P the most any family writes for this shape, P = N for the generic kernels; 16 bytes per partial --
// the streaming backwards keep their fp32 partials as 16-byte granule pairs (rk_dma.hpp: fin_publish)
inline size_t workspace_bytes(const Dims2& d, const Switches& sw) {
    int P = d.N;
    auto upto = [&P](int p) { P = p > P ? p : P; };
    const col2d::C2Dims cd = col2d::make_c2dims(d, d.H * d.W);
    upto(cd.ngroups * cd.nchunks);
    if (sw.kernels == ShiftKernels::Auto) {
        dma2d::FDims f;
        tile2d::TDims2 t;
        // the smaller group size gives the larger partial count: an upper bound for every storage type
        if (dma2d::make_fdims(f, d, dma2d::kFramesF32 < dma2d::kFrames16 ? dma2d::kFramesF32 : dma2d::kFrames16, true)) upto(f.ngroups * f.b.nbands);
        if (raw16::make_fdims8(f, d, raw16::kFramesRaw16)) upto(f.ngroups * f.b.nbands);
        // (fp32's frames per wave, kTileFrames, is the least the 16-bit backward's CU-dependent count takes: the most groups)
        if (tile2d::make_tdims<float, 14, 14>(t, d, true, sw.cus)) upto(t.ngroups);
    }
    return (size_t)d.C * 2 * (size_t)P * 16;
}

}  // namespace plan2d
}  // namespace rk
