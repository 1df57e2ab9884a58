// rk_resample.hip -- the head of the input side on the device: crop -> Pillow-exact bilinear resize -> window -> flip ->
// normalise, uint8 frames in, network input out (include/rubiks_hip.h, "crop, resize and flip").
//
// The reference does this per frame with PIL on CPU workers (rubiksnet/transforms.py: GroupMultiScaleCrop :189-278,
// GroupRandomHorizontalFlip :45-63, GroupScale / GroupCenterCrop / GroupFullResSample / GroupOverSample :37-186) and
// only then Stack -> ToTorchFormatTensor -> GroupNormalize.  Here one launch takes decoded frames [B, T, Hs, Ws, 3] and
// one box per output clip and writes [B * V, T, 3, Sh, Sw].
//
// Pillow's 8-bit resampler (ImagingResample, BILINEAR) is two separable integer passes, horizontal first, each
// producing uint8: out = clip8((2^21 + sum_j in[xmin + j] * k_j) >> 22), k_j = (int)(w_j * 2^22 + 0.5), the w_j a
// triangle filter of support max(in / out, 1) normalised by its left-to-right sum -- a handful of IEEE double
// operations per tap.  resample_coeffs() below repeats those operations in the same order in fp64 (the library is
// built with -ffp-contract=off; fp64 division on gfx950 is correctly rounded), so the integer weights, and with them
// every output byte, are Pillow's.  An axis whose lengths are equal needs no special case: the formula gives the
// weights (2^22, 0), the identity.
//
// One workgroup per (output clip, frame, band of kBandRows output rows).  Prologue: every column's and every band
// row's (first tap, tap count, integer weights) into LDS, plus the 3 x 256 table of normalised values (the tail's
// ((v / 255) - mean) / std has 256 possible inputs per channel: two fp32 divisions per table entry instead of per
// element, same roundings).  Then, for as many band rows as fit kHRows source rows at a time: the horizontal pass of
// the source rows they need into LDS as uint8 (a lane owns a pixel: its three channels share the taps), and the vertical
// pass + table lookup + store (a lane owns an output pixel: consecutive lanes -> consecutive elements of each plane).  The
// flip is folded into the column table (entry x describes window column Sw - 1 - x).
//
// Boxes are device data the launcher cannot see.  Tap counts are clamped to kTaps; a column's first source column is
// clamped into the frame and its tap count to what is left of the row when the table is built; a source row index is
// clamped into the frame where it is formed; the rows of a vertical pass are chosen so that their taps lie inside the
// LDS row buffer.  None of this changes a valid box's result, and a meaningless box gives a meaningless picture and
// nothing else.
//
// rk_clip_resample_ragged_u8_* is the same pass for real datasets, whose videos differ in size and whose clips are
// chosen frames of longer videos: the source is a packed arena, a record per video says where its frames lie and how
// large they are, and a per-frame index table says which stored frame each output frame shows (k_clip_resample_ragged).
#include "rk_common.hpp"

using namespace rk;

namespace {

constexpr int kTaps = 17;          // 2 * 8 + 1: a ratio of 8 is the largest supported (1080p -> 256 is 4.2)
constexpr int kBandRows = 16;      // output rows per workgroup
constexpr int kHRows = 32;         // horizontally resampled source rows held in LDS (>= kTaps: one output row always fits)
constexpr int kRowsPerIter = 4;    // source rows a lane resamples together in the horizontal pass
constexpr int kPrec = 22;          // Pillow's PRECISION_BITS for 8-bit data (32 - 8 - 2)
constexpr int kMaxSide = 16384;    // the largest Hs or Ws a record of the ragged entry may claim

__device__ __forceinline__ double tri(double a) {
    if (a < 0.0) a = -a;
    return a < 1.0 ? 1.0 - a : 0.0;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for output index i of an axis resampled from n to m samples
// (n, m >= 1).  i is a double so that a meaningless window offset cannot overflow an int on the way in.
__device__ __forceinline__ void resample_coeffs(int n, int m, double i, int* first, int* count, int* k) {
    const double scale = (double)n / (double)m;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs, ss = 1.0 / fs;
    const double center = (i + 0.5) * scale;
    const double lo = center - support + 0.5, hi = center + support + 0.5;
    const int xmin = lo < 0.0 ? 0 : (lo > (double)n ? n : (int)lo);             // (int) truncates, as in C
    const int xmax = hi > (double)n ? n : (hi < 0.0 ? 0 : (int)hi);
    int cnt = xmax - xmin;
    cnt = cnt < 0 ? 0 : (cnt > kTaps ? kTaps : cnt);
    double ww = 0.0;
    for (int j = 0; j < cnt; ++j) ww += tri(((double)(j + xmin) - center + 0.5) * ss);
    for (int j = 0; j < cnt; ++j) {
        double w = tri(((double)(j + xmin) - center + 0.5) * ss);               // the same value the sum above saw
        if (ww != 0.0) w /= ww;
        k[j] = (int)(w * (double)(1 << kPrec) + 0.5);
    }
    *first = xmin;
    *count = cnt;
}

__device__ __forceinline__ int clampi(long long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }
__device__ __forceinline__ unsigned clip8(unsigned acc) {      // Pillow's clip8 of a non-negative accumulator
    acc >>= kPrec;
    return acc > 255u ? 255u : acc;
}

__host__ __device__ inline size_t resample_lds_bytes(int Sw) {
    return ((size_t)Sw * (2 + kTaps) + (size_t)kBandRows * (2 + kTaps)) * sizeof(int) + 3 * 256 * sizeof(float) +
           (size_t)kHRows * Sw * 3;
}

// One workgroup's share of the work: band blockIdx.x of output frame t of output clip oc, from the source frame at fbase
// (Hs x Ws x 3, rows Ws * 3 bytes apart).  Both kernels below are this body behind a different way of finding fbase.
template <typename T>
__device__ __forceinline__ void resample_band(const unsigned char* __restrict__ fbase, const int* __restrict__ boxes,
                                              const float* __restrict__ mean3, const float* __restrict__ std3,
                                              T* __restrict__ out, int Tn, int Hs, int Ws, int Sh, int Sw) {
    extern __shared__ __align__(16) unsigned char smem[];
    int* xsrc_s = reinterpret_cast<int*>(smem);        // [Sw] first tap as a column of the source FRAME
    int* xcnt_s = xsrc_s + Sw;                         // [Sw]
    int* kx_s = xcnt_s + Sw;                           // [Sw][kTaps]
    int* ymin_s = kx_s + Sw * kTaps;                   // [kBandRows]
    int* ycnt_s = ymin_s + kBandRows;                  // [kBandRows]
    int* ky_s = ycnt_s + kBandRows;                    // [kBandRows][kTaps]
    float* lut = reinterpret_cast<float*>(ky_s + kBandRows * kTaps);     // [3][256]
    unsigned char* hbuf = reinterpret_cast<unsigned char*>(lut + 3 * 256);   // [kHRows][Sw * 3]

    const int band = blockIdx.x, t = blockIdx.y, oc = blockIdx.z, tid = threadIdx.x;
    const int* box = boxes + (long long)oc * 9;
    const int x0 = box[0], y0 = box[1], ox = box[6], oy = box[7], flip = box[8];
    const int cw = box[2] < 1 ? 1 : box[2], ch = box[3] < 1 ? 1 : box[3];
    const int rw = box[4] < 1 ? 1 : box[4], rh = box[5] < 1 ? 1 : box[5];
    const int row0 = band * kBandRows;
    const int rows_here = (Sh - row0) < kBandRows ? (Sh - row0) : kBandRows;
    const int rowelems = Sw * 3;

    for (int i = tid; i < Sw + kBandRows; i += kBlock) {
        if (i < Sw) {
            const int wcol = flip ? Sw - 1 - i : i;
            int first, count;
            resample_coeffs(cw, rw, (double)ox + (double)wcol, &first, &count, kx_s + i * kTaps);
            // clamped into the frame HERE, once: x0 + first + count <= x0 + cw <= Ws for a valid box, which this leaves
            // alone; whatever else a box holds, the taps below stay inside the source row
            const int xs = clampi((long long)x0 + first, 0, Ws - 1);
            xsrc_s[i] = xs;
            xcnt_s[i] = count < Ws - xs ? count : Ws - xs;
        } else if (i - Sw < rows_here) {
            const int r = i - Sw;
            resample_coeffs(ch, rh, (double)oy + (double)(row0 + r), ymin_s + r, ycnt_s + r, ky_s + r * kTaps);
        }
    }
    for (int i = tid; i < 3 * 256; i += kBlock) {
        const int c = i >> 8;
        const float v = (float)(i & 255) / 255.0f;                 // ToTorchFormatTensor: .float().div(255)
        lut[i] = (v - mean3[c]) / std3[c];                         // GroupNormalize: sub_(m).div_(s)
    }
    __syncthreads();

    T* obase = out + (((long long)oc * Tn + t) * 3 * Sh + row0) * (long long)Sw;
    const long long plane = (long long)Sh * Sw;

    for (int o = 0; o < rows_here;) {
        // as many further rows as the kHRows source rows starting at this row's first tap cover
        const int base = ymin_s[o];
        int top = base + ycnt_s[o], k = 1;
        while (o + k < rows_here) {
            const int lo = ymin_s[o + k], hi = lo + ycnt_s[o + k];
            if (lo < base || hi - base > kHRows) break;
            top = hi > top ? hi : top;
            ++k;
        }
        const int nsrc = top - base;                               // <= kHRows: ycnt <= kTaps <= kHRows
        // horizontal pass, uint8 result: a lane owns one pixel (its three channels share the taps) of kRowsPerIter source
        // rows at once -- the rows share the column's taps and weights, and their loads are independent, so 3 *
        // kRowsPerIter byte loads are in flight per tap instead of 3 (the pass waits on global loads, not on arithmetic).
        // A row index past the last one repeats the last row and is not stored.
        for (int r = 0; r < nsrc; r += kRowsPerIter) {
            const unsigned char* rowp[kRowsPerIter];
#pragma unroll
            for (int i = 0; i < kRowsPerIter; ++i) {
                const int rr = r + i < nsrc ? r + i : nsrc - 1;
                rowp[i] = fbase + (long long)clampi((long long)y0 + base + rr, 0, Hs - 1) * Ws * 3;
            }
            for (int x = tid; x < Sw; x += kBlock) {
                const int cn = xcnt_s[x];
                const int* kk = kx_s + x * kTaps;
                int off = xsrc_s[x] * 3;                            // xsrc + cn <= Ws: see the prologue
                unsigned acc[kRowsPerIter][3];
#pragma unroll
                for (int i = 0; i < kRowsPerIter; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 1u << (kPrec - 1);
                for (int j = 0; j < cn; ++j, off += 3) {
                    const unsigned w = (unsigned)kk[j];
#pragma unroll
                    for (int i = 0; i < kRowsPerIter; ++i) {
                        acc[i][0] += rowp[i][off + 0] * w;
                        acc[i][1] += rowp[i][off + 1] * w;
                        acc[i][2] += rowp[i][off + 2] * w;
                    }
                }
#pragma unroll
                for (int i = 0; i < kRowsPerIter; ++i) {
                    if (r + i < nsrc) {
                        unsigned char* h = hbuf + (r + i) * rowelems + x * 3;
                        h[0] = clip8(acc[i][0]);
                        h[1] = clip8(acc[i][1]);
                        h[2] = clip8(acc[i][2]);
                    }
                }
            }
        }
        __syncthreads();
        // vertical pass + normalise: a lane owns one pixel of an output row, consecutive lanes -> consecutive elements of
        // each channel plane.  Rows of this pass satisfy base <= ymin and ymin + ycnt - base <= kHRows (the loop above),
        // so every hbuf row read here was written by the horizontal pass just done.
        for (int r = 0; r < k; ++r) {
            const int cn = ycnt_s[o + r];
            const int* kk = ky_s + (o + r) * kTaps;
            const unsigned char* hfirst = hbuf + (ymin_s[o + r] - base) * rowelems;
            T* orow = obase + (long long)(o + r) * Sw;
            for (int x = tid; x < Sw; x += kBlock) {
                const unsigned char* h = hfirst + x * 3;
                unsigned a0 = 1u << (kPrec - 1), a1 = a0, a2 = a0;
                for (int j = 0; j < cn; ++j, h += rowelems) {
                    const unsigned w = (unsigned)kk[j];
                    a0 += h[0] * w;
                    a1 += h[1] * w;
                    a2 += h[2] * w;
                }
                st(orow + x, lut[clip8(a0)]);
                st(orow + plane + x, lut[256 + clip8(a1)]);
                st(orow + 2 * plane + x, lut[512 + clip8(a2)]);
            }
        }
        __syncthreads();
        o += k;
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_clip_resample(const unsigned char* __restrict__ frames,
                                                          const int* __restrict__ boxes, const float* __restrict__ mean3,
                                                          const float* __restrict__ std3, T* __restrict__ out, int Tn,
                                                          int Hs, int Ws, int V, int Sh, int Sw) {
    const int t = blockIdx.y, oc = blockIdx.z;
    resample_band<T>(frames + ((long long)(oc / V) * Tn + t) * Hs * (long long)Ws * 3, boxes, mean3, std3, out, Tn, Hs, Ws,
                     Sh, Sw);
}

// The same pass over a packed arena of videos of different sizes.  clips [B][4] int64: (byte offset of the video's first
// frame, Hs, Ws, F), its F frames back to back, rows Ws * 3 bytes apart, any alignment.  frame_idx [B * V][Tn] int32: the
// stored frame output frame t of output clip oc shows, clamped into [0, F - 1].  Sizes, offset and indices are device data
// the launcher cannot see: a record that does not describe F whole frames inside [arena, arena + arena_bytes) is decided
// here, from values every lane of the workgroup reads alike, before any byte of the arena is read, and its clip is written
// as zeros.  A record that passes keeps every read of the body inside its own video: the body clamps rows into [0, Hs) and
// column runs into [0, Ws).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_clip_resample_ragged(const unsigned char* __restrict__ arena, long long arena_bytes,
                                                                 const long long* __restrict__ clips,
                                                                 const int* __restrict__ frame_idx,
                                                                 const int* __restrict__ boxes, const float* __restrict__ mean3,
                                                                 const float* __restrict__ std3, T* __restrict__ out, int Tn,
                                                                 int V, int Sh, int Sw) {
    const int band = blockIdx.x, t = blockIdx.y, oc = blockIdx.z;
    const long long* rec = clips + (long long)(oc / V) * 4;
    const long long off = rec[0], hs = rec[1], ws = rec[2], nf = rec[3];
    // read beside the record, not after the verdict: the table has a row per output clip whatever the records say, and
    // one wait covers both loads
    int fraw = frame_idx[(long long)oc * Tn + t];
    int touch = boxes[(long long)oc * 9];                          // the body's box reads then hit the scalar cache
    asm volatile("" : "+s"(fraw), "+s"(touch));                    // keeps both loads here: the compiler would sink them below the verdict
    long long f = fraw;
    bool ok = hs >= 1 && hs <= kMaxSide && ws >= 1 && ws <= kMaxSide && nf >= 1 && off >= 0 && off <= arena_bytes;
    const long long fbytes = ok ? hs * ws * 3 : 3;                 // at most 3 * 2^28 once the sides passed
    // off + nf * fbytes <= arena_bytes without a 64-bit division: nf <= room bounds nf below 2^63, the high half of the
    // 128-bit product says whether the low half is all of it
    const unsigned long long room = (unsigned long long)arena_bytes - (unsigned long long)off;   // meaningful once ok
    if (ok) ok = (unsigned long long)nf <= room && __umul64hi((unsigned long long)nf, (unsigned long long)fbytes) == 0 &&
                 (unsigned long long)nf * (unsigned long long)fbytes <= room;
    if (!ok) {
        const int row0 = band * kBandRows;
        const int rows_here = (Sh - row0) < kBandRows ? (Sh - row0) : kBandRows;
        T* obase = out + (((long long)oc * Tn + t) * 3 * Sh + row0) * (long long)Sw;
        const long long plane = (long long)Sh * Sw;
        for (int c = 0; c < 3; ++c)
            for (int i = threadIdx.x; i < rows_here * Sw; i += kBlock) st(obase + c * plane + i, 0.0f);
        return;
    }
    f = f < 0 ? 0 : (f > nf - 1 ? nf - 1 : f);
    resample_band<T>(arena + off + f * fbytes, boxes, mean3, std3, out, Tn, (int)hs, (int)ws, Sh, Sw);
}

template <typename T>
int resample_impl(const unsigned char* frames, const int* boxes, const float* mean3, const float* std3, void* out, int B,
                  int Tn, int Hs, int Ws, int V, int Sh, int Sw, rk_stream_t stream) {
    if (!frames || !boxes || !mean3 || !std3 || !out) return RK_ERR_NULL_POINTER;
    if (B <= 0 || Tn <= 0 || Hs <= 0 || Ws <= 0 || V <= 0 || Sh <= 0 || Sw <= 0) return RK_ERR_BAD_DIMS;
    if ((long long)B * V > 65535 || Tn > 65535 || (long long)Ws * 3 > 0x7fffffffLL) return RK_ERR_BAD_DIMS;   // grid.z, grid.y
    const size_t lds = resample_lds_bytes(Sw);
    static DynLdsRaised raised;
    const int rc = raise_dynamic_lds(reinterpret_cast<const void*>(&k_clip_resample<T>), lds, raised);   // more than 160 KB (Sw above ~920): RK_ERR_UNSUPPORTED
    if (rc != RK_OK) return rc;
    const dim3 grid((unsigned)((Sh + kBandRows - 1) / kBandRows), (unsigned)Tn, (unsigned)(B * V));
    hipLaunchKernelGGL((k_clip_resample<T>), grid, dim3(kBlock), lds, (hipStream_t)stream, frames, boxes, mean3, std3, (T*)out,
                       Tn, Hs, Ws, V, Sh, Sw);
    return launch_status();
}

template <typename T>
int resample_ragged_impl(const unsigned char* arena, long long arena_bytes, const long long* clips, const int* frame_idx,
                         const int* boxes, const float* mean3, const float* std3, void* out, int B, int V, int Tn, int Sh,
                         int Sw, rk_stream_t stream) {
    if (!arena || !clips || !frame_idx || !boxes || !mean3 || !std3 || !out) return RK_ERR_NULL_POINTER;
    if (arena_bytes <= 0 || B <= 0 || V <= 0 || Tn <= 0 || Sh <= 0 || Sw <= 0) return RK_ERR_BAD_DIMS;
    if ((long long)B * V > 65535 || Tn > 65535) return RK_ERR_BAD_DIMS;                                      // grid.z, grid.y
    const size_t lds = resample_lds_bytes(Sw);                     // the source sizes do not enter: Sw alone, as above
    static DynLdsRaised raised;
    const int rc = raise_dynamic_lds(reinterpret_cast<const void*>(&k_clip_resample_ragged<T>), lds, raised);
    if (rc != RK_OK) return rc;
    const dim3 grid((unsigned)((Sh + kBandRows - 1) / kBandRows), (unsigned)Tn, (unsigned)(B * V));
    hipLaunchKernelGGL((k_clip_resample_ragged<T>), grid, dim3(kBlock), lds, (hipStream_t)stream, arena, arena_bytes, clips,
                       frame_idx, boxes, mean3, std3, (T*)out, Tn, V, Sh, Sw);
    return launch_status();
}

}  // namespace

extern "C" {

int rk_clip_resample_u8_f32(const unsigned char* frames, const int* boxes, const float* mean3, const float* std3, float* out,
                            int B, int T, int Hs, int Ws, int V, int Sh, int Sw, rk_stream_t stream) {
    return resample_impl<float>(frames, boxes, mean3, std3, out, B, T, Hs, Ws, V, Sh, Sw, stream);
}
int rk_clip_resample_u8_bf16(const unsigned char* frames, const int* boxes, const float* mean3, const float* std3, void* out,
                             int B, int T, int Hs, int Ws, int V, int Sh, int Sw, rk_stream_t stream) {
    return resample_impl<__hip_bfloat16>(frames, boxes, mean3, std3, out, B, T, Hs, Ws, V, Sh, Sw, stream);
}

int rk_clip_resample_ragged_u8_f32(const unsigned char* arena, long long arena_bytes, const long long* clips,
                                   const int* frame_idx, const int* boxes, const float* mean3, const float* std3, float* out,
                                   int B, int V, int T, int Sh, int Sw, rk_stream_t stream) {
    return resample_ragged_impl<float>(arena, arena_bytes, clips, frame_idx, boxes, mean3, std3, out, B, V, T, Sh, Sw, stream);
}
int rk_clip_resample_ragged_u8_bf16(const unsigned char* arena, long long arena_bytes, const long long* clips,
                                    const int* frame_idx, const int* boxes, const float* mean3, const float* std3, void* out,
                                    int B, int V, int T, int Sh, int Sw, rk_stream_t stream) {
    return resample_ragged_impl<__hip_bfloat16>(arena, arena_bytes, clips, frame_idx, boxes, mean3, std3, out, B, V, T, Sh, Sw,
                                                stream);
}

}  // extern "C"
