// rk_jpeg.hip -- baseline JPEG frames decoded on the device (rk_jpeg_decode_u8, include/rubiks_hip.h).
//
// The decode itself is rk_jpeg_core.hpp, the same text the CPU test runs under sanitizers; this file lays it over the
// machine in five launches that the stream orders (no hand-off inside a launch, no atomics, no polling):
//
//   k_jpeg_plan     one workgroup: every record checked from its own fields, the frames' workspace regions laid out
//                   (an exclusive sum of their sizes into the offset table that heads the workspace), status[i] set
//   k_jpeg_entropy  one wave per frame.  The Huffman walk is one dependent chain, so the wave runs it once for all 64
//                   lanes in uniform control flow: the frame's tables sit in LDS, the stream comes through a 2 KB LDS
//                   window that all lanes refill together (a lane pulling single bytes from global memory would pay a
//                   full memory round trip per byte; an LDS read is ~64 cycles and broadcasts).  Lane p keeps
//                   coefficient p of the current block in a register, so a finished block leaves as one 128-byte store
//                   and no coefficient memory needs clearing.
//   k_jpeg_idct     a lane per 8x8 block: dequantise, jidctint ISLOW, range limit, into the component planes
//   k_jpeg_colour   a lane per output pixel: fancy upsampling + YCbCr -> RGB, HWC bytes; a failed frame is zeroed here
//   k_jpeg_count    status[n] = frames with a non-zero code
//
// The launcher knows n and the byte counts only, so every grid is sized by n and strides over a frame's work.
#include "rk_common.hpp"
#include "rk_jpeg_core.hpp"

namespace rk {
namespace {

constexpr int kJpegWindow = 2048;       // bytes of a frame's stream staged in LDS at a time
constexpr int kIdctSlices = 16;         // workgroups per frame in k_jpeg_idct
constexpr int kColourSlices = 32;       // workgroups per frame in k_jpeg_colour

__global__ __launch_bounds__(kBlock) void k_jpeg_plan(const rk_jpeg_frame* __restrict__ frames, int n, long long stream_bytes,
                                                      long long rgb_bytes, int nq, int nh, long long* __restrict__ offsets,
                                                      long long workspace_bytes, int* __restrict__ status) {
    __shared__ long long part[kBlock];
    const int t = threadIdx.x, per = (n + kBlock - 1) / kBlock;
    const int lo = min(n, t * per), hi = min(n, lo + per);
    long long sum = 0;
    for (int i = lo; i < hi; ++i) sum += rkjpeg::frame_workspace_bytes(frames[i]);
    part[t] = sum;
    __syncthreads();
    long long at = rkjpeg::offset_table_bytes(n);
    for (int k = 0; k < t; ++k) at += part[k];
    for (int i = lo; i < hi; ++i) {
        const rk_jpeg_frame f = frames[i];
        offsets[i] = at;
        at += rkjpeg::frame_workspace_bytes(f);
        status[i] = rkjpeg::check_record(f, stream_bytes, rgb_bytes, nq, nh, at, workspace_bytes);
    }
    if (t == kBlock - 1) offsets[n] = at;               // the last thread's end is the total (its own chunk may be empty)
}

// The frame's segment through an LDS window; every lane of the wave calls byte() with the same position.
struct WindowSrc {
    const unsigned char* g;         // the segment in global memory
    unsigned char* win;
    long long base, len;
    int lane;
    __device__ __forceinline__ int byte(long long p) {
        if (p < base || p >= base + kJpegWindow) {
            __syncthreads();        // one wave per workgroup: orders the LDS traffic, cannot wait on anyone
            base = p;
            for (int k = lane; k < kJpegWindow; k += kWave) win[k] = (base + k < len) ? g[base + k] : (unsigned char)0;
            __syncthreads();
        }
        return win[(int)(p - base)];
    }
};

// Lane p holds coefficient p (natural order) of the block being decoded; `zigzag` is that coefficient's place in the
// scan, looked up once per lane, so that a decoded coefficient costs one compare and no table access.
struct LaneSink {
    short* coefs;
    int lane, zigzag, mine;
    __device__ __forceinline__ void put(int k, int v) { mine = (k == zigzag) ? v : mine; }
    __device__ __forceinline__ void end_block(long long b) {
        coefs[b * 64 + lane] = (short)mine;
        mine = 0;
    }
};

__global__ __launch_bounds__(kWave) void k_jpeg_entropy(const unsigned char* __restrict__ streams,
                                                        const rk_jpeg_frame* __restrict__ frames,
                                                        const rk_jpeg_huff* __restrict__ htabs, unsigned char* __restrict__ ws,
                                                        int* __restrict__ status) {
    __shared__ rk_jpeg_huff tabs[6];
    __shared__ unsigned char win[kJpegWindow];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (status[i] != RK_JPEG_OK) return;                // the record is invalid: nothing of it is read
    const rk_jpeg_frame f = frames[i];
    rkjpeg::Geometry g;
    rkjpeg::geometry(f, g);
    constexpr int kWords = sizeof(rk_jpeg_huff) / 4;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                       // unrolled: f.dc[c] with a run-time c would put the record in scratch
        if (c >= g.ncomp) break;
        const unsigned* d = reinterpret_cast<const unsigned*>(htabs + f.dc[c]);
        const unsigned* a = reinterpret_cast<const unsigned*>(htabs + f.ac[c]);
        for (int k = lane; k < kWords; k += kWave) {
            reinterpret_cast<unsigned*>(&tabs[c])[k] = d[k];
            reinterpret_cast<unsigned*>(&tabs[3 + c])[k] = a[k];
        }
    }
    __syncthreads();
    WindowSrc src{streams + f.stream_off, win, -(long long)kJpegWindow - 1, f.stream_len, lane};
    int zigzag = 0;
    for (int k = 0; k < 64; ++k) zigzag = rkjpeg::natural_of(k) == lane ? k : zigzag;
    LaneSink sink{reinterpret_cast<short*>(ws + reinterpret_cast<const long long*>(ws)[i]), lane, zigzag, 0};
    const int rc = rkjpeg::decode_scan(f, g, src, tabs, sink);
    if (lane == 0) status[i] = rc;
}

__global__ __launch_bounds__(kBlock) void k_jpeg_idct(const rk_jpeg_frame* __restrict__ frames,
                                                      const unsigned short* __restrict__ qtabs, unsigned char* __restrict__ ws,
                                                      const int* __restrict__ status) {
    const int i = blockIdx.x;
    if (status[i] != RK_JPEG_OK) return;
    const rk_jpeg_frame f = frames[i];
    rkjpeg::Geometry g;
    rkjpeg::geometry(f, g);
    unsigned char* base = ws + reinterpret_cast<const long long*>(ws)[i];
    for (long long b = (long long)blockIdx.y * kBlock + threadIdx.x; b < g.nblocks; b += (long long)kBlock * gridDim.y) {
        int comp, stride;
        long long off;
        rkjpeg::block_place(g, b, &comp, &off, &stride);
        alignas(16) short coef[64];
        const uint4* src = reinterpret_cast<const uint4*>(base + b * 128);      // the region and b * 128 are 16-byte aligned
#pragma unroll
        for (int k = 0; k < 8; ++k) reinterpret_cast<uint4*>(coef)[k] = src[k];
        // selects, not f.quant[comp] / g.plane_off[comp]: a run-time index would put the structs in scratch memory
        const int qi = comp == 0 ? f.quant[0] : (comp == 1 ? f.quant[1] : f.quant[2]);
        const long long plane = comp == 0 ? g.plane_off[0] : (comp == 1 ? g.plane_off[1] : g.plane_off[2]);
        rkjpeg::idct_islow(coef, qtabs + (long long)qi * 64, base + plane + off, stride);
    }
}

__global__ __launch_bounds__(kBlock) void k_jpeg_colour(const rk_jpeg_frame* __restrict__ frames,
                                                        const unsigned char* __restrict__ ws, const int* __restrict__ status,
                                                        unsigned char* __restrict__ rgb, long long rgb_bytes) {
    const int i = blockIdx.x;
    const rk_jpeg_frame f = frames[i];
    if (!rkjpeg::rgb_range_ok(f, rgb_bytes)) return;    // nowhere to write
    const int npix = f.width * f.height;                // at most 2^28
    unsigned char* out = rgb + f.rgb_off;
    const int first = blockIdx.y * kBlock + threadIdx.x, step = kBlock * gridDim.y;
    if (status[i] != RK_JPEG_OK) {
        for (int p = first; p < npix; p += step) out[3LL * p] = out[3LL * p + 1] = out[3LL * p + 2] = 0;
        return;
    }
    rkjpeg::Geometry g;
    rkjpeg::geometry(f, g);
    const unsigned char* base = ws + reinterpret_cast<const long long*>(ws)[i];
    for (int p = first; p < npix; p += step) {
        const int y = p / f.width, x = p - y * f.width;
        rkjpeg::pixel_rgb(base, g, x, y, out + 3LL * p);
    }
}

__global__ __launch_bounds__(kBlock) void k_jpeg_count(int* __restrict__ status, int n) {
    __shared__ int part[kBlock];
    int bad = 0;
    for (int i = threadIdx.x; i < n; i += kBlock) bad += status[i] != RK_JPEG_OK;
    part[threadIdx.x] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int k = 0; k < kBlock; ++k) total += part[k];
        status[n] = total;
    }
}

}  // namespace
}  // namespace rk

extern "C" {

size_t rk_jpeg_workspace_bytes(const rk_jpeg_frame* frames_host, int n) {
    if (!frames_host || n < 1) return 0;
    long long total = rkjpeg::offset_table_bytes(n);
    for (int i = 0; i < n; ++i) total += rkjpeg::frame_workspace_bytes(frames_host[i]);
    return (size_t)total;
}

int rk_jpeg_decode_u8(const unsigned char* streams, long long stream_bytes, const rk_jpeg_frame* frames,
                      const unsigned short* qtabs, const rk_jpeg_huff* htabs, int nq, int nh, int n, unsigned char* rgb,
                      long long rgb_bytes, void* workspace, size_t workspace_bytes, int* status, rk_stream_t stream) {
    using namespace rk;
    if (!streams || !frames || !qtabs || !htabs || !rgb || !status) return RK_ERR_NULL_POINTER;
    if (n < 1 || n > 65535 || nq < 1 || nq > 65535 || nh < 1 || nh > 65535 || stream_bytes < 0 || rgb_bytes < 0)
        return RK_ERR_BAD_DIMS;
    if (((uintptr_t)frames & 7) || ((uintptr_t)htabs & 3) || ((uintptr_t)qtabs & 1) || ((uintptr_t)status & 3)) return RK_ERR_BAD_DIMS;
    if (!workspace || ((uintptr_t)workspace & 15) || (long long)workspace_bytes < rkjpeg::offset_table_bytes(n))
        return RK_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    hipLaunchKernelGGL(k_jpeg_plan, dim3(1), dim3(kBlock), 0, s, frames, n, stream_bytes, rgb_bytes, nq, nh,
                       reinterpret_cast<long long*>(ws), (long long)workspace_bytes, status);
    hipLaunchKernelGGL(k_jpeg_entropy, dim3(n), dim3(kWave), 0, s, streams, frames, htabs, ws, status);
    hipLaunchKernelGGL(k_jpeg_idct, dim3(n, kIdctSlices), dim3(kBlock), 0, s, frames, qtabs, ws, status);
    hipLaunchKernelGGL(k_jpeg_colour, dim3(n, kColourSlices), dim3(kBlock), 0, s, frames, ws, status, rgb, rgb_bytes);
    hipLaunchKernelGGL(k_jpeg_count, dim3(1), dim3(kBlock), 0, s, status, n);
    return launch_status();
}

}  // extern "C"
