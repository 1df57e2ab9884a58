// rk3d_plan.hpp -- which kernels run a RubiksShift3D call.  plan3d() holds every eligibility rule and the order in which the
// families are considered; it is a pure host function (no HIP call, no environment, no pointers: one alignment bit per
// operand, the switches as arguments), so rk_debug_3d_plan can show the choice on a machine without a device and
// tests/test_plan3d.py holds it against the dispatch it replaced.  The families' headers supply the geometry (false = not
// for these kernels) and launchers that run what they are given; rk3d.hip validates, plans and switches over the plan.
#pragma once
#include "rk3d_generic.hpp"
#include "rk3d_dma.hpp"
#include "rk3d_plane.hpp"
#include "rk3d_tile.hpp"
#include "rk3d_translate.hpp"
#include "rk3d_stride2.hpp"
#include "rk3d_column.hpp"
#include "rk3d_slab.hpp"
#include "rk3d_16.hpp"

namespace rk {
namespace plan3d {

enum Family {                 // the kernel template of a launch; Cfg3::v holds its variant
    kNone, kPlane, kDmaInterp, kDmaBwd, kTileInterp, kTileBwd, kSlabInterp, kSlabBwd, kXlate, kS2Fwd, kS2Bwd, kSlabS2Fwd,
    kSlabS2Bwd, kColFwd, kColBwd, kGenFwd, kGenBwdX, kGenBwdS, kFinalize,
    kGen16Fwd, kGen16BwdX, kGen16BwdS, kStream16Fwd, kStream16Bwd,         // 16-bit activations, fp32 shift (rk3d_16.hpp)
    kStream16S2Fwd, kStream16S2Bwd                                         // ... their stride (1,2,2) streaming family
};
enum Form { kForward, kBackward, kForwardBn, kBackwardBn };
enum Aligned { kAlX = 1, kAlY = 2, kAlGx = 4, kAlBn = 8 };     // 16-byte aligned: x / z, y (forward) or gy, gx / dz, the BN pack

// RK_SHIFT_KERNELS (rk_common.hpp) and RK_SLAB14: 14x14 planes on the slab kernels instead of the tile kernels -- unset
// (-1): the forward and d(x) alone, 1: the fused backward too, 0: neither.  (The slab forward / d(x)-only kernels are level
// with the tile kernels at C = 216 and 10 % faster at C = 288, 22.0 vs 24.7 us; the fused backward is level, 29.2 vs 29.1 us,
// and rk3d_tile.hpp has the BatchNorm-fused variants.)
struct Switches { ShiftKernels kernels; int slab14; };

struct Call {
    Dims3 d;
    Form form;
    int elem;                 // 4: fp32, 8: fp64, 2: bf16 / f16 activations next to an fp32 shift table (rk3d_*_sf32)
    bool quantize, gx, gshift, two_phase;     // backward: the gradients wanted; two_phase: stop after the partials
    int aligned;              // Aligned bits; an operand the call does not have counts as aligned
};
struct Launch {
    Family family;
    Cfg3 c;
    union { plane3d::PDims plane; dma::BDims band; s2::SDims s2; slab3d::SDims slab; slab3d::S2Dims slab2; col3d::CDims col; Dims3 gen; s16::SDims s16; s16::S2Dims s16s2; } g;
};
struct Plan {
    int rc;                   // RK_OK, or RK_ERR_UNSUPPORTED (the BN forms: no fused kernel covers the call; 16-bit: no such form)
    int n;
    Launch l[3];              // in launch order; a separate finalize (k3d_finalize) is the last of them
    int P;                    // partials per channel and sum of the d(shift) launch: ws[C][3 or 5][P]; 0: no d(shift)
    bool finalize;            // the row-sum + K5 is a launch of its own (else: inside the d(shift) launch, or two-phase)
};

inline void set_group(Dims3& d, int plane_elems) {
    d.E = pow2_at_least(plane_elems, kWave, kBlock);
    d.logE = (d.E == 64) ? 6 : (d.E == 128 ? 7 : 8);
}
inline unsigned grid_for(const Dims3& d, long long planes) {
    const int per_block = kBlock / d.E;
    return (unsigned)((planes + per_block - 1) / per_block);
}

// (a geometry function writes to the launch only when it takes the call)
inline Plan plan(const Call& c, const Switches& sw) {
    const Dims3& d = c.d;
    Plan pl{};
    auto variant = [](int v0, int v1) { Launch l{}; l.c.v[0] = v0; l.c.v[1] = v1; return l; };
    auto take = [&pl](Family f, Launch& l) { l.family = f; pl.l[pl.n++] = l; return true; };
    auto generic = [&](Family f, int quant, int plane_elems, int planes_t) {
        Launch l = variant(quant, 0);
        l.g.gen = d;
        set_group(l.g.gen, plane_elems);
        l.c.grid = grid_for(l.g.gen, (long long)d.N * planes_t * d.C);
        return take(f, l);
    };
    auto finalize = [&] {                                              // k3d_finalize: row-sum of the P partials per channel + K5
        Launch l = variant(0, 0);
        l.c.grid = (unsigned)d.C;
        pl.finalize = true;
        return take(kFinalize, l);
    };
    if (c.elem == 2) {
        // 16-bit activations: the streaming kernels of rk3d_16.hpp (stride 1, or stride (1,2,2)) where they apply and every
        // operand they touch is 16-byte aligned, else the generic plane kernels at 16-bit storage; fp32 partials, the finalize
        // always a launch of its own.  No BN form, no two-phase form.
        if (c.form == kForwardBn || c.form == kBackwardBn || c.two_phase) return pl.rc = RK_ERR_UNSUPPORTED, pl;
        const bool al16 = (c.aligned & (kAlX | kAlY | kAlGx)) == (kAlX | kAlY | kAlGx);
        Launch l = variant(c.form == kBackward && c.gx, c.form == kBackward && c.gshift);
        const bool may = !c.quantize && sw.kernels == ShiftKernels::Auto && al16;
        const bool streams = may && s16::geometry(l.g.s16, l.c, d);                                   // stride 1
        const bool streams2 = may && !streams && s16::geometry_s2(l.g.s16s2, l.c, d, c.form == kBackward);   // stride (1,2,2)
        if (c.form == kForward) {
            if (streams) take(kStream16Fwd, l);
            else if (streams2) take(kStream16S2Fwd, l);
            else generic(kGen16Fwd, c.quantize, d.Ho * d.Wo, d.To);
            return pl;
        }
        if (streams || streams2) {
            const int bands = streams ? l.g.s16.bands : l.g.s16s2.bands;
            take(streams ? kStream16Bwd : kStream16S2Bwd, l);
            if (c.gshift) pl.P = d.N * bands;
        } else {
            if (c.gx) generic(kGen16BwdX, c.quantize, d.H * d.W, d.T);
            if (c.gshift) {
                generic(kGen16BwdS, 0, d.Ho * d.Wo, d.To);
                pl.P = d.N * d.To;
            }
        }
        if (c.gshift) finalize();
        return pl;
    }
    const bool f32 = c.elem == 4, bn = c.form == kForwardBn || c.form == kBackwardBn;
    const bool streaming = f32 && sw.kernels == ShiftKernels::Auto, column = sw.kernels != ShiftKernels::Generic;
    const bool band_ok = s1p0(d) && d.W % 4 == 0 && d.W >= 4;                   // rk3d_plane.hpp, rk3d_dma.hpp
    const bool p14 = d.H == 14 && d.W == 14;
    const bool al_x = c.aligned & kAlX, al_y = c.aligned & kAlY, al_gx = c.aligned & kAlGx, al_bn = !bn || (c.aligned & kAlBn);

    // forward (src = x, dst = y) or d(x) alone (negate: src = gy, dst = gx) in one streaming launch, stride 1 / pad 0
    auto interp = [&](bool negate) {
        if (!streaming || !s1p0(d)) return false;
        Launch l = variant(negate, bn);
        if (c.quantize) {                                              // a plane translation (rk3d_translate.hpp)
            if (d.W % 4 != 0 || !(negate ? al_gx : al_y)) return false;
            l.g.gen = d;
            xlate3d::geometry(l.g.gen, l.c);
            return take(kXlate, l);
        }
        if (!(negate ? al_gx : al_x) || !al_y || !al_bn) return false;
        if (band_ok && plane3d::geometry(l.g.plane, l.c, d)) return take(kPlane, l);
        if (band_ok && dma3d::interp_geometry(l.g.band, l.c, d)) return take(kDmaInterp, l);
        // 14x14: the slab kernels unless RK_SLAB14=0 or they do not take it (T > 8), then the tile kernels, which also
        // have the BN variant; other small planes: the slab kernels
        if (!bn && (!p14 || sw.slab14 != 0) && slab3d::geometry(l.g.slab, l.c, d, false)) return take(kSlabInterp, l);
        if (!p14) return false;
        tile3d::geometry(l.c, d, false);
        return take(kTileInterp, l);
    };
    // the forward of the stride (1,2,2) / pad 0 layers
    auto forward_s2 = [&] {
        if (c.quantize || !streaming || !s122p0(d) || !al_x || !al_y || !al_bn) return false;
        Launch l = variant(0, bn);
        if (s2::geometry(l.g.s2, l.c, d, false)) return take(kS2Fwd, l);
        return !bn && slab3d::geometry_s2(l.g.slab2, l.c, d, false) && take(kSlabS2Fwd, l);
    };
    // d(shift) (+ d(x)) in one streaming launch, the row-sum + K5 inside it unless two-phase; sets P.
    // quant: the QUANT walk of rk3d_dma.hpp or nothing; dma_tile_only: the d(shift) half behind a translation
    auto fused_bwd = [&](bool gx, bool quant, bool dma_tile_only) {
        if (!streaming || !al_x || !al_y || (gx && !al_gx) || !al_bn) return false;
        const bool fused = !c.two_phase, slab = !dma_tile_only && !bn;
        Launch l = variant(gx, fused);
        auto done = [&](Family f, int P) {
            if (fused) l.c.grid += (unsigned)d.C;                      // the finalizer blocks
            pl.P = P;
            return take(f, l);
        };
        if (band_ok && dma3d::bwd_geometry(l.g.band, l.c, d)) {
            l.c.v[3] = quant; l.c.v[4] = bn;
            return done(kDmaBwd, d.N * l.g.band.nbands);
        }
        if (quant) return false;
        if (s1p0(d) && p14) {          // the tile kernels (or, RK_SLAB14=1, the slab kernels first)
            if (slab && sw.slab14 == 1 && slab3d::geometry(l.g.slab, l.c, d, true)) return done(kSlabBwd, 2 * d.N);
            tile3d::geometry(l.c, d, true);
            l.c.v[2] = bn;
            return done(kTileBwd, d.N);
        }
        if (s1p0(d)) return slab && slab3d::geometry(l.g.slab, l.c, d, true) && done(kSlabBwd, 2 * d.N);
        if (!s122p0(d) || dma_tile_only) return false;
        if (s2::geometry(l.g.s2, l.c, d, true)) {
            l.c.v[2] = bn;
            return done(kS2Bwd, d.N * l.g.s2.nbands);
        }
        return slab && slab3d::geometry_s2(l.g.slab2, l.c, d, true) && done(kSlabS2Bwd, 2 * d.N);   // 28 -> 14 and 14 -> 7
    };
    const bool col_ok = column && !c.quantize && d.sT == 1 && d.pT == 0;   // rk3d_column.hpp

    switch (c.form) {
        case kForwardBn:
            pl.rc = !c.quantize && (interp(false) || forward_s2()) ? RK_OK : RK_ERR_UNSUPPORTED;
            return pl;
        case kBackwardBn:
            pl.rc = fused_bwd(true, c.quantize, false) ? RK_OK : RK_ERR_UNSUPPORTED;
            return pl;
        case kForward: {
            if (interp(false) || forward_s2()) return pl;
            if (!col_ok) return generic(kGenFwd, c.quantize, d.Ho * d.Wo, d.To), pl;
            Launch l = variant(0, 0);
            l.g.col = col3d::make_cdims(d, d.Ho * d.Wo);
            l.c.v[2] = l.g.col.M;
            l.c.grid = col3d::grid_of(l.g.col);
            return take(kColFwd, l), pl;
        }
        case kBackward: break;
    }
    bool gx = c.gx;
    if (c.quantize && c.gx) {
        // d(x) is a plane translation; d(shift) does not depend on quantize (K2 takes the fractional shift, rubiks.cpp:324-358):
        // both from the QUANT walk in the one-call form, else the translation and a streaming backward without its d(x) half
        if (c.gshift && !c.two_phase && fused_bwd(true, true, false)) return pl;
        if (interp(true)) {
            if (!c.gshift || fused_bwd(false, false, true)) return pl;
            gx = false;
        }
    } else if (!c.quantize && (c.gshift ? fused_bwd(c.gx, false, false) : interp(true))) {
        return pl;
    }
    if (c.gshift && col_ok) {
        // fp32 one-call form: row-sum + K5 inside the launch; two-phase form / fp64 / no streaming kernels: partials
        Launch l = variant(c.gx, !c.two_phase && streaming);
        l.g.col = col3d::make_cdims(d, d.H * d.W);
        l.c.v[2] = l.g.col.M;
        l.c.v[3] = d.sH >= 2 && d.sW >= 2;
        l.c.v[4] = l.g.col.M == 4 && f32 && d.H * d.W % 4 == 0 && al_x && (!c.gx || al_gx);
        l.c.grid = col3d::grid_of(l.g.col) + (l.c.v[1] ? (unsigned)d.C : 0u);
        pl.P = d.N * l.g.col.nchunks;
        pl.finalize = !l.c.v[1] && !c.two_phase;
        take(kColBwd, l);
    } else {
        if (gx) generic(kGenBwdX, c.quantize, d.H * d.W, d.T);        // rubiks.cpp:363-376
        if (c.gshift) {                                                // rubiks.cpp:324-358
            generic(kGenBwdS, 0, d.Ho * d.Wo, d.To);
            pl.P = d.N * d.To;
            pl.finalize = !c.two_phase;
        }
    }
    if (pl.finalize) finalize();
    return pl;
}

}  // namespace plan3d
}  // namespace rk
