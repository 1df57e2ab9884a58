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
//
// A resident set (rk_jpeg_build_index, rk_jpeg_decode_indexed_u8) replaces the one chain per frame by one per segment:
//
//   k_jpeg_index        one wave per frame, once: the same walk with no coefficient stored, the reader's position and the
//                       DC predictors written every E MCUs
//   k_jpeg_gather       the picked records, with their places in the RGB arena, into the head of the workspace, so that
//                       plan, IDCT, colour and count run on them unchanged
//   k_jpeg_entropy_seg  one wave (and one workgroup) per segment: resumes at its entry, must end at the next one
//   k_jpeg_seg_status   a frame's code = that of its lowest failing segment
//
// rk_jpeg_build_index_chunked builds the same index from many short walks instead of one frame-long chain per frame
// (k_jpeg_chunk_plan, k_jpeg_index_chunked, k_jpeg_index_chain; see below).
#include <initializer_list>

#include "rk_common.hpp"
#include "rk_jpeg_core.hpp"

namespace rk {
namespace {

constexpr int kJpegWindow = 2048;       // bytes of a frame's stream staged in LDS at a time
constexpr int kSegWindow = 1024;        // the same for one segment of a frame: tables + window stay under 160 KB / 16 per CU
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
template <int kWindow>
struct WindowSrcT {
    const unsigned char* g;         // the segment in global memory
    unsigned char* win;
    long long base, len;
    int lane;
    __device__ __forceinline__ int byte(long long p) {
        if (p < base || p >= base + kWindow) {
            __syncthreads();        // one wave per workgroup: orders the LDS traffic, cannot wait on anyone
            base = p;
            for (int k = lane; k < kWindow; k += kWave) win[k] = (base + k < len) ? g[base + k] : (unsigned char)0;
            __syncthreads();
        }
        return win[(int)(p - base)];
    }
};
typedef WindowSrcT<kJpegWindow> WindowSrc;

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
// The lane's sink onto frame i's coefficient region of the workspace.
__device__ __forceinline__ LaneSink lane_sink(unsigned char* __restrict__ ws, int i, int lane) {
    int zigzag = 0;
    for (int k = 0; k < 64; ++k) zigzag = rkjpeg::natural_of(k) == lane ? k : zigzag;
    return LaneSink{reinterpret_cast<short*>(ws + reinterpret_cast<const long long*>(ws)[i]), lane, zigzag, 0};
}

// The frame's six tables into LDS, DC of component c at [c], AC at [3 + c], by the `lanes` lanes of the workgroup (the
// caller syncs).
__device__ __forceinline__ void load_tables(const rk_jpeg_frame& f, int ncomp, const rk_jpeg_huff* __restrict__ htabs,
                                            rk_jpeg_huff* tabs, int lane, int lanes) {
    constexpr int kWords = sizeof(rk_jpeg_huff) / 4;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                       // unrolled: f.dc[c] with a run-time c would put the record in scratch
        if (c >= ncomp) break;
        const unsigned* d = reinterpret_cast<const unsigned*>(htabs + f.dc[c]);
        const unsigned* a = reinterpret_cast<const unsigned*>(htabs + f.ac[c]);
        for (int k = lane; k < kWords; k += lanes) {
            reinterpret_cast<unsigned*>(&tabs[c])[k] = d[k];
            reinterpret_cast<unsigned*>(&tabs[3 + c])[k] = a[k];
        }
    }
}

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
    // load_tables' text in place: through the call this kernel's table load comes out in another order than it had
    constexpr int kWords = sizeof(rk_jpeg_huff) / 4;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
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
    LaneSink sink = lane_sink(ws, i, lane);
    const int rc = rkjpeg::decode_scan(f, g, src, tabs, sink);
    if (lane == 0) status[i] = rc;
}

// ---------------------------------------------------------------------------------------------- the scan index
// One wave per resident frame: the record and its row of the index checked from their own fields, then the one
// sequential walk the frame ever gets, which stores no coefficient and writes the entry of every E-th MCU.
__device__ __forceinline__ void index_frame(const unsigned char* __restrict__ streams, long long stream_bytes,
                                            const rk_jpeg_frame* __restrict__ frames, const rk_jpeg_huff* __restrict__ htabs,
                                            int nq, int nh, const int* __restrict__ seg_mcus,
                                            const long long* __restrict__ entry_off, rk_jpeg_entry* __restrict__ entries,
                                            long long n_entries, int* __restrict__ status) {
    __shared__ rk_jpeg_huff tabs[6];
    __shared__ unsigned char win[kJpegWindow];
    const int i = blockIdx.x, lane = threadIdx.x;
    const rk_jpeg_frame f = frames[i];
    int rc = rkjpeg::check_resident(f, stream_bytes, nq, nh);
    rkjpeg::Geometry g;
    const int E = seg_mcus[i];
    const long long first = entry_off[i], last = entry_off[i + 1];
    if (rc == RK_JPEG_OK) {
        rkjpeg::geometry(f, g);
        if (!rkjpeg::index_row_ok(g, E, first, last, n_entries)) rc = RK_JPEG_BAD_INDEX;
    }
    if (rc != RK_JPEG_OK) {                             // uniform: nothing of the frame is read
        if (lane == 0) status[i] = rc;
        return;
    }
    load_tables(f, g.ncomp, htabs, tabs, lane, kWave);
    __syncthreads();
    WindowSrc src{streams + f.stream_off, win, -(long long)kJpegWindow - 1, f.stream_len, lane};
    rc = rkjpeg::record_index(f, g, src, tabs, E, entries + first, lane == 0);
    if (lane == 0) status[i] = rc;
}

__global__ __launch_bounds__(kWave) void k_jpeg_index(const unsigned char* __restrict__ streams, long long stream_bytes,
                                                      const rk_jpeg_frame* __restrict__ frames,
                                                      const rk_jpeg_huff* __restrict__ htabs, int nq, int nh,
                                                      const int* __restrict__ seg_mcus, const long long* __restrict__ entry_off,
                                                      rk_jpeg_entry* __restrict__ entries, long long n_entries,
                                                      int* __restrict__ status) {
    index_frame(streams, stream_bytes, frames, htabs, nq, nh, seg_mcus, entry_off, entries, n_entries, status);
}

// ---------------------------------------------------------------------------------------------- the chunked index build
// rk_jpeg_build_index_chunked (the scheme: rk_jpeg_core.hpp).  Four launches:
//
//   k_jpeg_chunk_plan     one workgroup: the frames' regions of the workspace (32 bytes per chunk) behind an offset table
//   k_jpeg_index_chunked  one workgroup of 1024 lanes per frame; lane t walks chunks t, t + 1024, ...  The frame's tables sit
//                         in LDS; every chunk's p_in, p_out and sums sit in the frame's region of the workspace, which
//                         only this workgroup touches, always with a barrier between a store and another lane's load.
//                         The rounds are separated by barriers in uniform control flow (a lane with nothing to walk
//                         still reaches them); inside a walk the lanes diverge, each on a chain of its own that is one
//                         chunk long.  Then the sums in front of every chunk, the final pass that writes the entries, and
//                         route[i]: the rounds it took, or 0 where the frame is left to the next launch.
//                         The stream is NOT staged in LDS: a walk reads its chunk as a few aligned 8-byte words, which
//                         costs little beside the walk itself, while 40 KB of LDS per frame would leave a CU one
//                         workgroup, every SIMD a few waves and nothing to hide the walks' latency with when a whole
//                         set is built (profiles/jpeg_chunked_time.txt).
//   k_jpeg_index_chain    the sequential walk of k_jpeg_index for the frames with route 0, and only for them
//   k_jpeg_count
using rkjpeg::kChunkBlock;

// The frame's stream read as aligned 8-byte words of which the lane keeps the last: a walk asks for consecutive bytes
// (and for the one behind an FF), so seven of eight bytes cost no memory access.  A word that is not wholly inside
// [streams, streams + stream_bytes) -- the arena's first or last -- is put together from the bytes that are.  No barrier
// inside: the lanes diverge.
struct WordSrc {
    const unsigned char* mem;           // the frame's segment
    uintptr_t lo, hi;                   // the arena: [streams, streams + stream_bytes)
    uintptr_t at;                       // the address of the word held in `cur`, 0: none
    unsigned long long cur;
    __device__ __forceinline__ int byte(long long p) {
        const uintptr_t addr = (uintptr_t)(mem + p), w = addr & ~(uintptr_t)7;
        if (w != at) {
            at = w;
            if (w >= lo && w + 8 <= hi) {
                cur = *reinterpret_cast<const unsigned long long*>(w);
            } else {
                cur = 0;
                for (int k = 0; k < 8; ++k)
                    if (w + k >= lo && w + k < hi) cur |= (unsigned long long)*reinterpret_cast<const unsigned char*>(w + k) << (8 * k);
            }
        }
        return (int)(cur >> (((int)addr & 7) * 8)) & 0xFF;
    }
};

__global__ __launch_bounds__(kBlock) void k_jpeg_chunk_plan(const rk_jpeg_frame* __restrict__ frames, int n, int S,
                                                            long long* __restrict__ offsets) {
    __shared__ long long part[kBlock];
    const int t = threadIdx.x, per = (n + kBlock - 1) / kBlock;
    const int lo = min(n, t * per), hi = min(n, lo + per);
    long long sum = 0;
    for (int i = lo; i < hi; ++i) sum += rkjpeg::chunk_count(frames[i], S);
    part[t] = sum;
    __syncthreads();
    long long at = 0;
    for (int k = 0; k < t; ++k) at += part[k];
    for (int i = lo; i < hi; ++i) {
        offsets[i] = rkjpeg::chunked_workspace_bytes(at, n);
        at += rkjpeg::chunk_count(frames[i], S);
    }
    if (t == kBlock - 1) offsets[n] = rkjpeg::chunked_workspace_bytes(at, n);
}

// The phases of rk_jpeg_core.hpp with a barrier behind each; every lane of the workgroup calls it, and the control flow
// around the barriers is uniform (the words of `sh` that steer it are the same for every lane).
// -> the rounds after which the walk had converged, 0 where the frame is left to the sequential walk.
template <class Src>
__device__ __forceinline__ int chunked_frame(const rk_jpeg_frame& f, const rkjpeg::Geometry& g, Src& src, const rk_jpeg_huff* tabs,
                                             rkjpeg::ChunkShared& sh, rkjpeg::ChunkState* __restrict__ st, int nch, int S,
                                             int max_rounds, int E, rk_jpeg_entry* __restrict__ row) {
    const int t = threadIdx.x;
    rkjpeg::chunk_init(t, kChunkBlock, sh, st, nch, S);
    __syncthreads();
    int rounds = 0;
    for (int r = 1; r <= max_rounds && !rounds; ++r) {
        rkjpeg::chunk_walk_dirty(t, kChunkBlock, f, g, src, tabs, st, nch, S);
        __syncthreads();                // the workgroup's own stores to global memory are visible to it behind a barrier
        rkjpeg::chunk_advance(t, kChunkBlock, sh, st, nch, S, r);
        __syncthreads();
        if (rkjpeg::chunk_converged(sh, r)) rounds = r;
    }
    if (rounds == 0) return 0;
    rkjpeg::chunk_run_sums(t, kChunkBlock, sh, st, nch);
    __syncthreads();
    const int dead = rkjpeg::chunk_sums_in_front(t, kChunkBlock, sh, st, nch);     // lane-local, the same in every lane
    __syncthreads();
    rkjpeg::chunk_final_pass(t, kChunkBlock, f, g, src, tabs, sh, st, nch, S, E, row, dead);
    __syncthreads();
    return rkjpeg::chunk_route(sh, rounds);
}

// 8 waves per SIMD asked for: at most 64 VGPRs, so that two workgroups of 16 waves share a CU when a whole set is built.
__global__ __launch_bounds__(kChunkBlock, 8) void k_jpeg_index_chunked(
    const unsigned char* __restrict__ streams, long long stream_bytes, const rk_jpeg_frame* __restrict__ frames,
    const rk_jpeg_huff* __restrict__ htabs, int nq, int nh, const int* __restrict__ seg_mcus,
    const long long* __restrict__ entry_off, rk_jpeg_entry* __restrict__ entries, long long n_entries, int S, int max_rounds,
    unsigned char* __restrict__ ws, long long ws_bytes, int* __restrict__ status, int* __restrict__ route) {
    __shared__ rk_jpeg_huff tabs[6];
    __shared__ rkjpeg::ChunkShared sh;
    const int i = blockIdx.x, t = threadIdx.x;
    const rk_jpeg_frame f = frames[i];
    rkjpeg::Geometry g;
    const int E = seg_mcus[i];
    const long long first = entry_off[i], last = entry_off[i + 1];
    const long long ws_lo = reinterpret_cast<const long long*>(ws)[i], ws_hi = reinterpret_cast<const long long*>(ws)[i + 1];
    const int nch = rkjpeg::chunk_count(f, S);
    // what is not plainly a frame for this kernel is the sequential walk's, with the code it gives (uniform: one record)
    bool mine = max_rounds > 0 && nch > 0 && rkjpeg::check_resident(f, stream_bytes, nq, nh) == RK_JPEG_OK;
    if (mine) {
        rkjpeg::geometry(f, g);
        mine = rkjpeg::index_row_ok(g, E, first, last, n_entries) && ws_hi - ws_lo == 32LL * nch && ws_hi <= ws_bytes;
    }
    if (!mine) {
        if (t == 0) route[i] = 0;
        return;
    }
    load_tables(f, g.ncomp, htabs, tabs, t, kChunkBlock);
    __syncthreads();
    WordSrc src{streams + f.stream_off, (uintptr_t)streams, (uintptr_t)(streams + stream_bytes), 0, 0ull};
    const int rounds = chunked_frame(f, g, src, tabs, sh, reinterpret_cast<rkjpeg::ChunkState*>(ws + ws_lo), nch, S,
                                     max_rounds, E, entries + first);
    if (t == 0) {
        route[i] = rounds;
        if (rounds) status[i] = RK_JPEG_OK;
    }
}

__global__ __launch_bounds__(kWave) void k_jpeg_index_chain(const unsigned char* __restrict__ streams, long long stream_bytes,
                                                            const rk_jpeg_frame* __restrict__ frames,
                                                            const rk_jpeg_huff* __restrict__ htabs, int nq, int nh,
                                                            const int* __restrict__ seg_mcus,
                                                            const long long* __restrict__ entry_off,
                                                            rk_jpeg_entry* __restrict__ entries, long long n_entries,
                                                            int* __restrict__ status, const int* __restrict__ route) {
    if (route[blockIdx.x] != 0) return;                 // uniform: the chunked walk has written the frame's entries and code
    index_frame(streams, stream_bytes, frames, htabs, nq, nh, seg_mcus, entry_off, entries, n_entries, status);
}

// The m picked records, each with its own place in the RGB arena, into the head of the workspace: from here on the
// plan / IDCT / colour / count kernels run on them as on any frame table.  A pick outside the set gives a zero record,
// which k_jpeg_plan refuses and k_jpeg_colour has no range for.
__global__ __launch_bounds__(kBlock) void k_jpeg_gather(const rk_jpeg_frame* __restrict__ frames, int n,
                                                        const int* __restrict__ pick, const long long* __restrict__ rgb_off,
                                                        int m, rk_jpeg_frame* __restrict__ out) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const int p = pick[j];
    rk_jpeg_frame f = {};
    if (p >= 0 && p < n) {
        f = frames[p];
        f.rgb_off = rgb_off[j];
    }
    out[j] = f;
}

// Grid (m, max_segments), one wave per segment, ONE WAVE PER WORKGROUP: WindowSrc::byte holds barriers inside
// data-dependent control flow, which is safe only while no second wave exists to wait for.  Segment s of picked frame
// j resumes at its entry, decodes its MCUs into the frame's coefficient region and checks that it ends at the next
// entry; its code goes to segs[j * max_segments + s].  Blocks beyond the frame's segment count leave at once; a frame
// the plan or the index build refused, or whose index row does not fit, is not read (k_jpeg_seg_status gives it its code).
__global__ __launch_bounds__(kWave) void k_jpeg_entropy_seg(const unsigned char* __restrict__ streams,
                                                            const rk_jpeg_frame* __restrict__ gathered,
                                                            const rk_jpeg_huff* __restrict__ htabs,
                                                            const rk_jpeg_entry* __restrict__ entries, long long n_entries,
                                                            const long long* __restrict__ entry_off,
                                                            const int* __restrict__ seg_mcus, const int* __restrict__ build_status,
                                                            const int* __restrict__ pick, unsigned char* __restrict__ ws,
                                                            const int* __restrict__ status, int* __restrict__ segs) {
    __shared__ rk_jpeg_huff tabs[6];
    __shared__ unsigned char win[kSegWindow];
    const int j = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
    if (status[j] != RK_JPEG_OK) return;                // the record is invalid (a pick outside the set included)
    const int p = pick[j];
    if (build_status[p] != RK_JPEG_OK) return;
    const rk_jpeg_frame f = gathered[j];
    rkjpeg::Geometry g;
    rkjpeg::geometry(f, g);
    const int E = seg_mcus[p];
    const long long first = entry_off[p], last = entry_off[p + 1];
    if (!rkjpeg::index_row_ok(g, E, first, last, n_entries) || last - first > gridDim.y || s >= last - first) return;
    load_tables(f, g.ncomp, htabs, tabs, lane, kWave);
    __syncthreads();
    WindowSrcT<kSegWindow> src{streams + f.stream_off, win, -(long long)kSegWindow - 1, f.stream_len, lane};
    LaneSink sink = lane_sink(ws, j, lane);
    const long long nmcu = (long long)g.mcux * g.mcuy, m_begin = (long long)s * E;
    const long long m_end = m_begin + E < nmcu ? m_begin + E : nmcu;
    const rk_jpeg_entry entry = entries[first + s];
    const rk_jpeg_entry next = entries[first + (s + 1 < last - first ? s + 1 : s)];     // the last segment does not look at it
    const int rc = rkjpeg::decode_span(f, g, src, tabs, sink, entry, m_begin, m_end, &next);
    if (lane == 0) segs[(long long)j * gridDim.y + s] = rc;
}

// status[j] of a picked frame the plan accepted: the build's code where the build refused the frame, RK_JPEG_BAD_INDEX
// where its index row does not fit, else the code of its lowest failing segment -- a plain pass, the same code on every run.
__global__ __launch_bounds__(kBlock) void k_jpeg_seg_status(const rk_jpeg_frame* __restrict__ gathered, long long n_entries,
                                                            const long long* __restrict__ entry_off,
                                                            const int* __restrict__ seg_mcus, const int* __restrict__ build_status,
                                                            const int* __restrict__ pick, const int* __restrict__ segs, int m,
                                                            int max_segments, int* __restrict__ status) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m || status[j] != RK_JPEG_OK) return;
    const int p = pick[j];
    int rc = build_status[p];
    if (rc == RK_JPEG_OK) {
        rkjpeg::Geometry g;
        rkjpeg::geometry(gathered[j], g);
        const long long first = entry_off[p], last = entry_off[p + 1];
        if (!rkjpeg::index_row_ok(g, seg_mcus[p], first, last, n_entries) || last - first > max_segments) {
            rc = RK_JPEG_BAD_INDEX;
        } else {
            for (long long s = 0; s < last - first && rc == RK_JPEG_OK; ++s) rc = segs[(long long)j * max_segments + s];
        }
    }
    status[j] = rc;
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

// ---------------------------------------------------------------------------------------------- packed coefficients
// rk_jpeg_coef_sizes / rk_jpeg_coef_pack / rk_jpeg_decode_coef_u8 (the format and its checks: rk_jpeg_core.hpp).
//
//   building, after the entropy stage of a slab (k_jpeg_plan + k_jpeg_entropy, or + k_jpeg_entropy_seg + k_jpeg_seg_status):
//   k_coef_blocks        one workgroup: the exclusive sum of the frames' block counts; a frame past block_cap is refused
//   k_coef_block_sizes   a lane per block: the header of its 64 coefficients -> the bytes of its record
//   k_coef_frame_scan    a workgroup per frame: those bytes -> each record's offset in the frame's region, the region's length
//   k_coef_region_scan   one workgroup: the lengths -> the regions' offsets
//   k_coef_pack          a lane per block: the table entry and the record
//
//   per batch
//   k_jpeg_gather, k_coef_plan (records and regions checked, the planes laid out), k_coef_idct, k_coef_status,
//   k_jpeg_colour, k_jpeg_count
//
// k_coef_idct is a lane per block, as k_jpeg_idct: the lane reads its two table entries, its header and then only the
// values the header names -- reads of its own length per lane.  Lanes next to each other hold blocks next to each other,
// whose records lie back to back, so a wave's reads fall into a few consecutive cache lines (a record is 10 .. 136
// bytes, some 20 .. 40 for video frames) and are served from L2 after the first touch; the three dependent reads
// (offset, header, values) are the whole chain, where the Huffman stage has one per symbol.  Staging a workgroup's
// records in LDS first would make the global reads whole lines, but the bytes are few (the packed set is read at a
// small fraction of what HBM gives) and a lane's LDS reads would be as scattered as its global ones.  The expansion is
// unrolled over the 63 positions with constant indices, so the block stays in registers and goes into idct_islow as
// k_jpeg_idct's does.
//
// The entry points with a trailing record_format (rk_jpeg_coef_sizes_as, rk_jpeg_coef_pack_as, rk_jpeg_decode_coef_as_u8)
// are the drivers; the ones without are calls of them with RK_JPEG_COEF_WIDE.  The format is a template policy of
// k_coef_block_sizes, k_coef_pack and k_coef_idct (WideRecords, DenseRecords below) and a number to k_coef_frame_scan and
// k_coef_plan, which need the table's size and the region's bounds; every other kernel does not know it.  With
// DenseRecords the lane of k_coef_idct takes its record's span from the table (a base per 64 blocks and a 16-bit distance
// per block), holds the mask in one 64-bit register and takes the nibbles from a 32-bit window that is refilled every
// eighth nibble from an address that the count of nibbles taken gives -- the mask alone decides it -- so that only an
// escaped value's load waits for loaded data; every read is checked against the span first and the record must fill
// it exactly (rkjpeg::dense_expand_block).  The same unrolled loop, the same registers: 0 bytes of scratch.
struct RegionSrc {          // a region of the blob, 2-byte aligned
    const unsigned char* p;
    __device__ __forceinline__ unsigned u16(long long at) const { return *reinterpret_cast<const unsigned short*>(p + at); }
    __device__ __forceinline__ int s8(long long at) const { return *reinterpret_cast<const signed char*>(p + at); }
};
struct RegionDst {
    unsigned char* p;
    __device__ __forceinline__ void put16(long long at, unsigned v) { *reinterpret_cast<unsigned short*>(p + at) = (unsigned short)v; }
    __device__ __forceinline__ void put8(long long at, int v) { p[at] = (unsigned char)v; }
};

// The record format as a policy of k_coef_block_sizes, k_coef_pack and k_coef_idct: what a block's record takes, how it
// and its table entry are written, and how a lane gets its block back, checked.  Everything else is shared, and where a
// shared kernel needs the table's size or a region's bounds it takes the format's number.  k_coef_idct asks in two steps,
// find (the table; for the wide format also the header) and expand, with block_place between them as it always stood.
struct WideRecords {
    static constexpr int kFormat = RK_JPEG_COEF_WIDE;
    typedef unsigned long long Shape;
    static __device__ __forceinline__ Shape shape_of(const short* coef) { return rkjpeg::coef_header_of(coef); }
    static __device__ __forceinline__ int bytes_of(Shape header) { return rkjpeg::coef_record_bytes(header); }
    // offs: the frame's row of block_off
    static __device__ __forceinline__ bool put_entry(RegionDst& dst, const rkjpeg::Geometry&, long long b, long long at, const unsigned*) {
        dst.put16(4 * b, (unsigned)at & 0xFFFFu);
        dst.put16(4 * b + 2, (unsigned)(at >> 16) & 0xFFFFu);
        return true;
    }
    static __device__ __forceinline__ void pack(const short* coef, Shape header, RegionDst& dst, long long at) {
        rkjpeg::coef_pack_block(coef, header, dst, at);
    }
    struct Where {          // of a block that find() accepted
        long long at;
        unsigned long long header;
    };
    // the table and the header: everything the wide format checks
    static __device__ __forceinline__ bool find(RegionSrc& src, long long len, const rkjpeg::Geometry& g, long long b, Where* w) {
        return rkjpeg::coef_block_ok(src, len, g, b, &w->at, &w->header);
    }
    static __device__ __forceinline__ bool expand(RegionSrc& src, const Where& w, short* coef) {
        rkjpeg::coef_expand_block(src, w.at, w.header, coef);
        return true;
    }
};

struct DenseRecords {
    static constexpr int kFormat = RK_JPEG_COEF_DENSE;
    typedef rkjpeg::DenseShape Shape;
    static __device__ __forceinline__ Shape shape_of(const short* coef) { return rkjpeg::dense_shape_of(coef); }
    static __device__ __forceinline__ int bytes_of(const Shape& s) { return rkjpeg::dense_record_bytes(s); }
    // base[g] = the start of the group's first record, from the same row of block_off; rel[b] = the distance from it
    static __device__ __forceinline__ bool put_entry(RegionDst& dst, const rkjpeg::Geometry& g, long long b, long long at,
                                                     const unsigned* offs) {
        const long long base = offs[b & ~(long long)(rkjpeg::kDenseGroup - 1)];
        if (at < base || at - base > 0xFFFF) return false;
        if ((b & (rkjpeg::kDenseGroup - 1)) == 0) {
            dst.put16(4 * (b / rkjpeg::kDenseGroup), (unsigned)base & 0xFFFFu);
            dst.put16(4 * (b / rkjpeg::kDenseGroup) + 2, (unsigned)(base >> 16) & 0xFFFFu);
        }
        dst.put16(4 * rkjpeg::dense_groups(g) + 2 * b, (unsigned)(at - base));
        return true;
    }
    static __device__ __forceinline__ void pack(const short* coef, const Shape& s, RegionDst& dst, long long at) {
        rkjpeg::dense_pack_block(coef, s, dst, at);
    }
    struct Where {
        long long at;
        int span;
    };
    // the table alone gives the span; the record is checked against it as it is expanded
    static __device__ __forceinline__ bool find(RegionSrc& src, long long len, const rkjpeg::Geometry& g, long long b, Where* w) {
        return rkjpeg::dense_block_span(src, len, g, b, &w->at, &w->span);
    }
    static __device__ __forceinline__ bool expand(RegionSrc& src, const Where& w, short* coef) {
        return rkjpeg::dense_expand_block(src, w.at, w.span, coef);
    }
};

__device__ __forceinline__ long long frame_blocks(const rk_jpeg_frame& f) {
    rkjpeg::Geometry g;
    return rkjpeg::geometry(f, g) ? g.nblocks : 0;
}

__global__ __launch_bounds__(kBlock) void k_coef_blocks(const rk_jpeg_frame* __restrict__ frames, int n, long long block_cap,
                                                        long long* __restrict__ first_block, int* __restrict__ status) {
    __shared__ long long part[kBlock];
    const int t = threadIdx.x, per = (n + kBlock - 1) / kBlock;
    const int lo = min(n, t * per), hi = min(n, lo + per);
    long long sum = 0;
    for (int i = lo; i < hi; ++i) sum += frame_blocks(frames[i]);
    part[t] = sum;
    __syncthreads();
    long long at = 0;
    for (int k = 0; k < t; ++k) at += part[k];
    for (int i = lo; i < hi; ++i) {
        first_block[i] = at;
        at += frame_blocks(frames[i]);
        if (at > block_cap && status[i] == RK_JPEG_OK) status[i] = RK_JPEG_BAD_RECORD;
    }
    if (t == kBlock - 1) first_block[n] = at;
}

// The block's 64 coefficients out of the frame's coefficient region, as k_jpeg_idct reads them.
__device__ __forceinline__ void load_block(const unsigned char* __restrict__ base, long long b, short* coef) {
    const uint4* src = reinterpret_cast<const uint4*>(base + b * 128);
#pragma unroll
    for (int k = 0; k < 8; ++k) reinterpret_cast<uint4*>(coef)[k] = src[k];
}

template <class Records>
__global__ __launch_bounds__(kBlock) void k_coef_block_sizes(const rk_jpeg_frame* __restrict__ frames,
                                                             const unsigned char* __restrict__ ws, const int* __restrict__ status,
                                                             const long long* __restrict__ first_block,
                                                             unsigned* __restrict__ block_off) {
    const int i = blockIdx.x;
    if (status[i] != RK_JPEG_OK) return;
    rkjpeg::Geometry g;
    rkjpeg::geometry(frames[i], g);
    const unsigned char* base = ws + reinterpret_cast<const long long*>(ws)[i];
    unsigned* out = block_off + first_block[i];
    for (long long b = (long long)blockIdx.y * kBlock + threadIdx.x; b < g.nblocks; b += (long long)kBlock * gridDim.y) {
        alignas(16) short coef[64];
        load_block(base, b, coef);
        out[b] = (unsigned)Records::bytes_of(Records::shape_of(coef));
    }
}

// In place: the records' bytes of frame i become their offsets in the region (behind the table); region_off[i] = the
// region's length, 0 for a frame with a code.  At most 12.6 M blocks of 136 bytes: below 2^32.
__global__ __launch_bounds__(kBlock) void k_coef_frame_scan(const rk_jpeg_frame* __restrict__ frames, const int* __restrict__ status,
                                                            const long long* __restrict__ first_block,
                                                            unsigned* __restrict__ block_off, long long* __restrict__ region_off,
                                                            int format) {
    __shared__ long long part[kBlock];
    const int i = blockIdx.x, t = threadIdx.x;
    if (status[i] != RK_JPEG_OK) {                      // uniform
        if (t == 0) region_off[i] = 0;
        return;
    }
    rkjpeg::Geometry g;
    rkjpeg::geometry(frames[i], g);
    unsigned* mine = block_off + first_block[i];
    const long long per = (g.nblocks + kBlock - 1) / kBlock;
    const long long lo = min(g.nblocks, t * per), hi = min(g.nblocks, lo + per);
    long long sum = 0;
    for (long long b = lo; b < hi; ++b) sum += mine[b];
    part[t] = sum;
    __syncthreads();
    long long at = rkjpeg::coef_table_bytes_as(format, g);
    for (int k = 0; k < t; ++k) at += part[k];
    for (long long b = lo; b < hi; ++b) {
        const unsigned bytes = mine[b];
        mine[b] = (unsigned)at;
        at += bytes;
    }
    if (t == kBlock - 1) region_off[i] = at;
}

// In place: region_off[0 .. n) from lengths to offsets, region_off[n] = the total.
__global__ __launch_bounds__(kBlock) void k_coef_region_scan(long long* __restrict__ region_off, int n) {
    __shared__ long long part[kBlock];
    const int t = threadIdx.x, per = (n + kBlock - 1) / kBlock;
    const int lo = min(n, t * per), hi = min(n, lo + per);
    long long sum = 0;
    for (int i = lo; i < hi; ++i) sum += region_off[i];
    part[t] = sum;
    __syncthreads();                                    // every length is read before any offset is written
    long long at = 0;
    for (int k = 0; k < t; ++k) at += part[k];
    for (int i = lo; i < hi; ++i) {
        const long long len = region_off[i];
        region_off[i] = at;
        at += len;
    }
    if (t == kBlock - 1) region_off[n] = at;
}

template <class Records>
__global__ __launch_bounds__(kBlock) void k_coef_pack(const rk_jpeg_frame* __restrict__ frames, const unsigned char* __restrict__ ws,
                                                      const int* __restrict__ status, const unsigned* __restrict__ block_off,
                                                      long long block_cap, const long long* __restrict__ first_block,
                                                      const long long* __restrict__ region_off, unsigned char* __restrict__ blob,
                                                      long long blob_bytes) {
    const int i = blockIdx.x;
    if (status[i] != RK_JPEG_OK) return;
    rkjpeg::Geometry g;
    rkjpeg::geometry(frames[i], g);
    const long long lo = region_off[i], hi = region_off[i + 1], fb = first_block[i];
    if (!rkjpeg::coef_region_ok_as(Records::kFormat, lo, hi, blob_bytes, g) || fb < 0 || fb > block_cap - g.nblocks) return;
    const unsigned char* base = ws + reinterpret_cast<const long long*>(ws)[i];
    RegionDst dst{blob + lo};
    for (long long b = (long long)blockIdx.y * kBlock + threadIdx.x; b < g.nblocks; b += (long long)kBlock * gridDim.y) {
        alignas(16) short coef[64];
        load_block(base, b, coef);
        const typename Records::Shape shape = Records::shape_of(coef);
        const long long at = block_off[fb + b];
        if (at < rkjpeg::coef_table_bytes_as(Records::kFormat, g) || (at & 1) || at > hi - lo - Records::bytes_of(shape)) continue;
        if (!Records::put_entry(dst, g, b, at, block_off + fb)) continue;
        Records::pack(coef, shape, dst, at);
    }
}

// k_jpeg_plan for a batch of packed frames: the planes' regions of the workspace behind the offset table, every record
// and its region of the blob checked from their own fields, flag[j] cleared.  offsets[j] is the planes' place MINUS
// the frame's coefficient bytes, so that the plane offsets of rkjpeg::Geometry (which count from a region that starts
// with the coefficients) land in the planes: k_jpeg_colour runs on this workspace as it is.
__global__ __launch_bounds__(kBlock) void k_coef_plan(const rk_jpeg_frame* __restrict__ gathered, int m, long long rgb_bytes,
                                                      int nq, const int* __restrict__ pick, const int* __restrict__ build_status,
                                                      const long long* __restrict__ region_off, long long blob_bytes,
                                                      long long* __restrict__ offsets, long long workspace_bytes,
                                                      int* __restrict__ flag, int* __restrict__ status, int format) {
    __shared__ long long part[kBlock];
    const int t = threadIdx.x, per = (m + kBlock - 1) / kBlock;
    const int lo = min(m, t * per), hi = min(m, lo + per);
    long long sum = 0;
    for (int j = lo; j < hi; ++j) sum += rkjpeg::frame_plane_bytes(gathered[j]);
    part[t] = sum;
    __syncthreads();
    long long at = rkjpeg::offset_table_bytes(m);
    for (int k = 0; k < t; ++k) at += part[k];
    for (int j = lo; j < hi; ++j) {
        const rk_jpeg_frame f = gathered[j];
        rkjpeg::Geometry g;
        const bool sized = rkjpeg::geometry(f, g);
        offsets[j] = at - (sized ? g.coef_bytes : 0);
        at += sized ? rkjpeg::plane_bytes(g) : 0;
        int rc = rkjpeg::check_coef_record(f, rgb_bytes, nq, at, workspace_bytes);
        if (rc == RK_JPEG_OK) {                         // a pick outside the set is a zero record and was refused above
            const int p = pick[j];
            rc = build_status[p];
            if (rc == RK_JPEG_OK && !rkjpeg::coef_region_ok_as(format, region_off[p], region_off[p + 1], blob_bytes, g)) rc = RK_JPEG_BAD_INDEX;
        }
        flag[j] = 0;
        status[j] = rc;
    }
    if (t == kBlock - 1) offsets[m] = at;
}

template <class Records>
__global__ __launch_bounds__(kBlock) void k_coef_idct(const rk_jpeg_frame* __restrict__ gathered,
                                                      const unsigned short* __restrict__ qtabs,
                                                      const unsigned char* __restrict__ blob, const long long* __restrict__ region_off,
                                                      const int* __restrict__ pick, unsigned char* __restrict__ ws,
                                                      const int* __restrict__ status, int* __restrict__ flag) {
    const int j = blockIdx.x;
    if (status[j] != RK_JPEG_OK) return;
    const rk_jpeg_frame f = gathered[j];
    rkjpeg::Geometry g;
    rkjpeg::geometry(f, g);
    const int p = pick[j];
    const long long lo = region_off[p], len = region_off[p + 1] - lo;       // k_coef_plan has checked them
    RegionSrc src{blob + lo};
    unsigned char* base = ws + reinterpret_cast<const long long*>(ws)[j];
    for (long long b = (long long)blockIdx.y * kBlock + threadIdx.x; b < g.nblocks; b += (long long)kBlock * gridDim.y) {
        typename Records::Where where;
        if (!Records::find(src, len, g, b, &where)) {
            flag[j] = 1;                                // the same word from every lane that refuses; k_coef_status reads it
            continue;
        }
        int comp, stride;
        long long off;
        rkjpeg::block_place(g, b, &comp, &off, &stride);
        alignas(16) short coef[64];
        if (!Records::expand(src, where, coef)) {       // the dense record did not fill its span (the wide one cannot fail here)
            flag[j] = 1;
            continue;
        }
        const int qi = comp == 0 ? f.quant[0] : (comp == 1 ? f.quant[1] : f.quant[2]);
        const long long plane = comp == 0 ? g.plane_off[0] : (comp == 1 ? g.plane_off[1] : g.plane_off[2]);
        rkjpeg::idct_islow(coef, qtabs + (long long)qi * 64, base + plane + off, stride);
    }
}

__global__ __launch_bounds__(kBlock) void k_coef_status(const int* __restrict__ flag, int m, int* __restrict__ status) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j < m && status[j] == RK_JPEG_OK && flag[j]) status[j] = RK_JPEG_BAD_INDEX;
}

// pick[j] = j: the slab's records are the entropy stage's "picked" frames, each once, in order.
__global__ __launch_bounds__(kBlock) void k_coef_iota(int* __restrict__ pick, int n) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j < n) pick[j] = j;
}

// What the entry points ask of their arguments, in their order: pointers, then counts, sizes and alignment, then the workspace.
bool any_null(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (!p) return true;
    return false;
}
bool counts_ok(std::initializer_list<int> counts) {         // grid dimensions and 16-bit table indices: 1 .. 65535
    for (int v : counts)
        if (v < 1 || v > 65535) return false;
    return true;
}
bool sizes_ok(std::initializer_list<long long> sizes) {     // byte and entry counts
    for (long long v : sizes)
        if (v < 0) return false;
    return true;
}
bool aligned(uintptr_t to, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if ((uintptr_t)p & (to - 1)) return false;
    return true;
}
bool workspace_ok(const void* workspace, size_t bytes, long long least) {
    return workspace && aligned(16, {workspace}) && (long long)bytes >= least;
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
    if (any_null({streams, frames, qtabs, htabs, rgb, status})) return RK_ERR_NULL_POINTER;
    if (!counts_ok({n, nq, nh}) || !sizes_ok({stream_bytes, rgb_bytes}) || !aligned(8, {frames}) || !aligned(4, {htabs, status}) ||
        !aligned(2, {qtabs}))
        return RK_ERR_BAD_DIMS;
    if (!workspace_ok(workspace, workspace_bytes, rkjpeg::offset_table_bytes(n))) return RK_ERR_WORKSPACE;
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

int rk_jpeg_build_index(const unsigned char* streams, long long stream_bytes, const rk_jpeg_frame* frames,
                        const rk_jpeg_huff* htabs, int nq, int nh, int n, const int* seg_mcus, const long long* entry_off,
                        rk_jpeg_entry* entries, long long n_entries, int* status, rk_stream_t stream) {
    using namespace rk;
    if (any_null({streams, frames, htabs, seg_mcus, entry_off, entries, status})) return RK_ERR_NULL_POINTER;
    if (!counts_ok({n, nq, nh}) || !sizes_ok({stream_bytes, n_entries}) || !aligned(8, {frames, entry_off, entries}) ||
        !aligned(4, {htabs, status, seg_mcus}))
        return RK_ERR_BAD_DIMS;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_jpeg_index, dim3(n), dim3(kWave), 0, s, streams, stream_bytes, frames, htabs, nq, nh, seg_mcus,
                       entry_off, entries, n_entries, status);
    hipLaunchKernelGGL(k_jpeg_count, dim3(1), dim3(kBlock), 0, s, status, n);
    return launch_status();
}

size_t rk_jpeg_chunked_workspace_bytes(const rk_jpeg_frame* frames_host, int n, int chunk_bytes) {
    if (!frames_host || n < 1 || !rkjpeg::chunk_bytes_ok(chunk_bytes)) return 0;
    long long chunks = 0;
    for (int i = 0; i < n; ++i) chunks += rkjpeg::chunk_count(frames_host[i], chunk_bytes);
    return (size_t)rkjpeg::chunked_workspace_bytes(chunks, n);
}

int rk_jpeg_build_index_chunked(const unsigned char* streams, long long stream_bytes, const rk_jpeg_frame* frames,
                                const rk_jpeg_huff* htabs, int nq, int nh, int n, const int* seg_mcus,
                                const long long* entry_off, rk_jpeg_entry* entries, long long n_entries, int chunk_bytes,
                                int max_rounds, void* workspace, size_t workspace_bytes, int* status, int* route,
                                rk_stream_t stream) {
    using namespace rk;
    if (any_null({streams, frames, htabs, seg_mcus, entry_off, entries, status, route})) return RK_ERR_NULL_POINTER;
    if (!counts_ok({n, nq, nh}) || !sizes_ok({stream_bytes, n_entries}) || !aligned(8, {frames, entry_off, entries}) ||
        !aligned(4, {htabs, status, seg_mcus, route}) || !rkjpeg::chunk_bytes_ok(chunk_bytes) || max_rounds < 0 || max_rounds > 64)
        return RK_ERR_BAD_DIMS;
    if (!workspace_ok(workspace, workspace_bytes, rkjpeg::offset_table_bytes(n))) return RK_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    hipLaunchKernelGGL(k_jpeg_chunk_plan, dim3(1), dim3(kBlock), 0, s, frames, n, chunk_bytes, reinterpret_cast<long long*>(ws));
    hipLaunchKernelGGL(k_jpeg_index_chunked, dim3(n), dim3(kChunkBlock), 0, s, streams, stream_bytes, frames, htabs, nq, nh, seg_mcus,
                       entry_off, entries, n_entries, chunk_bytes, max_rounds, ws, (long long)workspace_bytes, status, route);
    hipLaunchKernelGGL(k_jpeg_index_chain, dim3(n), dim3(kWave), 0, s, streams, stream_bytes, frames, htabs, nq, nh, seg_mcus,
                       entry_off, entries, n_entries, status, route);
    hipLaunchKernelGGL(k_jpeg_count, dim3(1), dim3(kBlock), 0, s, status, n);
    return launch_status();
}

size_t rk_jpeg_indexed_workspace_bytes(const rk_jpeg_frame* frames_host, int n, const int* pick_host, int m, int max_segments) {
    if (!frames_host || !pick_host || n < 1 || m < 1 || max_segments < 1) return 0;
    long long total = rkjpeg::indexed_head_bytes(m, max_segments) + rkjpeg::offset_table_bytes(m);
    for (int j = 0; j < m; ++j)
        if (pick_host[j] >= 0 && pick_host[j] < n) total += rkjpeg::frame_workspace_bytes(frames_host[pick_host[j]]);
    return (size_t)total;
}

int rk_jpeg_decode_indexed_u8(const unsigned char* streams, long long stream_bytes, const rk_jpeg_frame* frames,
                              const unsigned short* qtabs, const rk_jpeg_huff* htabs, int nq, int nh, int n,
                              const rk_jpeg_entry* entries, long long n_entries, const long long* entry_off,
                              const int* seg_mcus, const int* build_status, const int* pick, const long long* rgb_off, int m,
                              int max_segments, unsigned char* rgb, long long rgb_bytes, void* workspace,
                              size_t workspace_bytes, int* status, rk_stream_t stream) {
    using namespace rk;
    if (any_null({streams, frames, qtabs, htabs, entries, entry_off, seg_mcus, build_status, pick, rgb_off, rgb, status}))
        return RK_ERR_NULL_POINTER;
    if (n < 1 || !counts_ok({nq, nh, m, max_segments}) || !sizes_ok({stream_bytes, rgb_bytes, n_entries}) ||
        !aligned(8, {frames, entries, entry_off, rgb_off}) || !aligned(4, {htabs, status, seg_mcus, build_status, pick}) ||
        !aligned(2, {qtabs}))
        return RK_ERR_BAD_DIMS;
    const long long head = rkjpeg::indexed_head_bytes(m, max_segments);
    if (!workspace_ok(workspace, workspace_bytes, head + rkjpeg::offset_table_bytes(m))) return RK_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    unsigned char* base = static_cast<unsigned char*>(workspace);
    rk_jpeg_frame* gathered = reinterpret_cast<rk_jpeg_frame*>(base);
    int* segs = reinterpret_cast<int*>(base + rkjpeg::gathered_bytes(m));
    unsigned char* ws = base + head;                    // the plain decode's workspace: offset table, frame regions
    const long long ws_bytes = (long long)workspace_bytes - head;
    const int groups = (m + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_jpeg_gather, dim3(groups), dim3(kBlock), 0, s, frames, n, pick, rgb_off, m, gathered);
    hipLaunchKernelGGL(k_jpeg_plan, dim3(1), dim3(kBlock), 0, s, gathered, m, stream_bytes, rgb_bytes, nq, nh,
                       reinterpret_cast<long long*>(ws), ws_bytes, status);
    hipLaunchKernelGGL(k_jpeg_entropy_seg, dim3(m, max_segments), dim3(kWave), 0, s, streams, gathered, htabs, entries, n_entries,
                       entry_off, seg_mcus, build_status, pick, ws, status, segs);
    hipLaunchKernelGGL(k_jpeg_seg_status, dim3(groups), dim3(kBlock), 0, s, gathered, n_entries, entry_off, seg_mcus, build_status,
                       pick, segs, m, max_segments, status);
    hipLaunchKernelGGL(k_jpeg_idct, dim3(m, kIdctSlices), dim3(kBlock), 0, s, gathered, qtabs, ws, status);
    hipLaunchKernelGGL(k_jpeg_colour, dim3(m, kColourSlices), dim3(kBlock), 0, s, gathered, ws, status, rgb, rgb_bytes);
    hipLaunchKernelGGL(k_jpeg_count, dim3(1), dim3(kBlock), 0, s, status, m);
    return launch_status();
}

int rk_jpeg_coef_sizes_as(const unsigned char* streams, long long stream_bytes, const rk_jpeg_frame* frames,
                          const rk_jpeg_huff* htabs, int nq, int nh, int n, const rk_jpeg_entry* entries, long long n_entries,
                          const long long* entry_off, const int* seg_mcus, const int* build_status, int max_segments,
                          void* workspace, size_t workspace_bytes, int* status, unsigned* block_off, long long block_cap,
                          long long* first_block, long long* region_off, rk_stream_t stream, int record_format) {
    using namespace rk;
    if (any_null({streams, frames, htabs, status, block_off, first_block, region_off})) return RK_ERR_NULL_POINTER;
    if (entries && any_null({entry_off, seg_mcus, build_status})) return RK_ERR_NULL_POINTER;
    if (!rkjpeg::coef_format_ok(record_format) || !counts_ok({n, nq, nh, max_segments}) || !sizes_ok({stream_bytes, n_entries, block_cap}) ||
        !aligned(8, {frames, entries, entry_off, first_block, region_off}) ||
        !aligned(4, {htabs, status, seg_mcus, build_status, block_off}))
        return RK_ERR_BAD_DIMS;
    const long long head = rkjpeg::indexed_head_bytes(n, max_segments);
    if (!workspace_ok(workspace, workspace_bytes, head + rkjpeg::offset_table_bytes(n))) return RK_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    unsigned char* base = static_cast<unsigned char*>(workspace);
    int* pick = reinterpret_cast<int*>(base);           // in the place of the gathered records, which are `frames` themselves
    int* segs = reinterpret_cast<int*>(base + rkjpeg::gathered_bytes(n));
    unsigned char* ws = base + head;
    const long long ws_bytes = (long long)workspace_bytes - head;
    const int groups = (n + kBlock - 1) / kBlock;
    // a resident record has no place in an RGB arena and needs none here: any range is inside this one
    hipLaunchKernelGGL(k_jpeg_plan, dim3(1), dim3(kBlock), 0, s, frames, n, stream_bytes, 1LL << 62, nq, nh,
                       reinterpret_cast<long long*>(ws), ws_bytes, status);
    if (entries) {
        hipLaunchKernelGGL(k_coef_iota, dim3(groups), dim3(kBlock), 0, s, pick, n);
        hipLaunchKernelGGL(k_jpeg_entropy_seg, dim3(n, max_segments), dim3(kWave), 0, s, streams, frames, htabs, entries, n_entries,
                           entry_off, seg_mcus, build_status, pick, ws, status, segs);
        hipLaunchKernelGGL(k_jpeg_seg_status, dim3(groups), dim3(kBlock), 0, s, frames, n_entries, entry_off, seg_mcus,
                           build_status, pick, segs, n, max_segments, status);
    } else {
        hipLaunchKernelGGL(k_jpeg_entropy, dim3(n), dim3(kWave), 0, s, streams, frames, htabs, ws, status);
    }
    hipLaunchKernelGGL(k_coef_blocks, dim3(1), dim3(kBlock), 0, s, frames, n, block_cap, first_block, status);
    const auto sizes = record_format == RK_JPEG_COEF_DENSE ? k_coef_block_sizes<DenseRecords> : k_coef_block_sizes<WideRecords>;
    hipLaunchKernelGGL(sizes, dim3(n, kIdctSlices), dim3(kBlock), 0, s, frames, ws, status, first_block, block_off);
    hipLaunchKernelGGL(k_coef_frame_scan, dim3(n), dim3(kBlock), 0, s, frames, status, first_block, block_off, region_off,
                       record_format);
    hipLaunchKernelGGL(k_coef_region_scan, dim3(1), dim3(kBlock), 0, s, region_off, n);
    hipLaunchKernelGGL(k_jpeg_count, dim3(1), dim3(kBlock), 0, s, status, n);
    return launch_status();
}

int rk_jpeg_coef_sizes(const unsigned char* streams, long long stream_bytes, const rk_jpeg_frame* frames,
                       const rk_jpeg_huff* htabs, int nq, int nh, int n, const rk_jpeg_entry* entries, long long n_entries,
                       const long long* entry_off, const int* seg_mcus, const int* build_status, int max_segments,
                       void* workspace, size_t workspace_bytes, int* status, unsigned* block_off, long long block_cap,
                       long long* first_block, long long* region_off, rk_stream_t stream) {
    return rk_jpeg_coef_sizes_as(streams, stream_bytes, frames, htabs, nq, nh, n, entries, n_entries, entry_off, seg_mcus,
                                 build_status, max_segments, workspace, workspace_bytes, status, block_off, block_cap,
                                 first_block, region_off, stream, RK_JPEG_COEF_WIDE);
}

int rk_jpeg_coef_pack_as(const rk_jpeg_frame* frames, int n, int max_segments, const void* workspace, size_t workspace_bytes,
                         const int* status, const unsigned* block_off, long long block_cap, const long long* first_block,
                         const long long* region_off, unsigned char* blob, long long blob_bytes, rk_stream_t stream,
                         int record_format) {
    using namespace rk;
    if (any_null({frames, status, block_off, first_block, region_off, blob})) return RK_ERR_NULL_POINTER;
    if (!rkjpeg::coef_format_ok(record_format) || !counts_ok({n, max_segments}) || !sizes_ok({block_cap, blob_bytes}) ||
        !aligned(8, {frames, first_block, region_off}) || !aligned(4, {status, block_off}) || !aligned(2, {blob}))
        return RK_ERR_BAD_DIMS;
    const long long head = rkjpeg::indexed_head_bytes(n, max_segments);
    if (!workspace_ok(workspace, workspace_bytes, head + rkjpeg::offset_table_bytes(n))) return RK_ERR_WORKSPACE;
    const unsigned char* ws = static_cast<const unsigned char*>(workspace) + head;
    const auto pack = record_format == RK_JPEG_COEF_DENSE ? k_coef_pack<DenseRecords> : k_coef_pack<WideRecords>;
    hipLaunchKernelGGL(pack, dim3(n, kIdctSlices), dim3(kBlock), 0, (hipStream_t)stream, frames, ws, status, block_off, block_cap,
                       first_block, region_off, blob, blob_bytes);
    return launch_status();
}

int rk_jpeg_coef_pack(const rk_jpeg_frame* frames, int n, int max_segments, const void* workspace, size_t workspace_bytes,
                      const int* status, const unsigned* block_off, long long block_cap, const long long* first_block,
                      const long long* region_off, unsigned char* blob, long long blob_bytes, rk_stream_t stream) {
    return rk_jpeg_coef_pack_as(frames, n, max_segments, workspace, workspace_bytes, status, block_off, block_cap, first_block,
                                region_off, blob, blob_bytes, stream, RK_JPEG_COEF_WIDE);
}

int rk_jpeg_coef_region_bounds(int record_format, long long nblocks, long long* min_bytes, long long* max_bytes) {
    if (!min_bytes || !max_bytes) return RK_ERR_NULL_POINTER;
    if (!rkjpeg::coef_format_ok(record_format) || nblocks < 1) return RK_ERR_BAD_DIMS;
    rkjpeg::Geometry g = {};
    g.nblocks = nblocks;
    const bool dense = record_format == RK_JPEG_COEF_DENSE;
    const long long table = rkjpeg::coef_table_bytes_as(record_format, g);
    *min_bytes = table + nblocks * (dense ? rkjpeg::kDenseRecordMin : rkjpeg::kCoefRecordMin);
    *max_bytes = table + nblocks * (dense ? rkjpeg::kDenseRecordMax : rkjpeg::kCoefRecordMax);
    return RK_OK;
}

size_t rk_jpeg_coef_workspace_bytes(const rk_jpeg_frame* frames_host, int n, const int* pick_host, int m) {
    if (!frames_host || !pick_host || n < 1 || m < 1) return 0;
    long long total = rkjpeg::coef_head_bytes(m) + rkjpeg::offset_table_bytes(m);
    for (int j = 0; j < m; ++j)
        if (pick_host[j] >= 0 && pick_host[j] < n) total += rkjpeg::frame_plane_bytes(frames_host[pick_host[j]]);
    return (size_t)total;
}

int rk_jpeg_decode_coef_as_u8(const unsigned char* blob, long long blob_bytes, const rk_jpeg_frame* frames,
                              const unsigned short* qtabs, int nq, int n, const long long* region_off, const int* build_status,
                              const int* pick, const long long* rgb_off, int m, unsigned char* rgb, long long rgb_bytes,
                              void* workspace, size_t workspace_bytes, int* status, rk_stream_t stream, int record_format) {
    using namespace rk;
    if (any_null({blob, frames, qtabs, region_off, build_status, pick, rgb_off, rgb, status})) return RK_ERR_NULL_POINTER;
    if (!rkjpeg::coef_format_ok(record_format) || n < 1 || !counts_ok({nq, m}) || !sizes_ok({blob_bytes, rgb_bytes}) || !aligned(8, {frames, region_off, rgb_off}) ||
        !aligned(4, {status, build_status, pick}) || !aligned(2, {qtabs, blob}))
        return RK_ERR_BAD_DIMS;
    const long long head = rkjpeg::coef_head_bytes(m);
    if (!workspace_ok(workspace, workspace_bytes, head + rkjpeg::offset_table_bytes(m))) return RK_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    unsigned char* base = static_cast<unsigned char*>(workspace);
    rk_jpeg_frame* gathered = reinterpret_cast<rk_jpeg_frame*>(base);
    int* flag = reinterpret_cast<int*>(base + rkjpeg::gathered_bytes(m));
    unsigned char* ws = base + head;                    // an offset table, then planes only
    const int groups = (m + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_jpeg_gather, dim3(groups), dim3(kBlock), 0, s, frames, n, pick, rgb_off, m, gathered);
    hipLaunchKernelGGL(k_coef_plan, dim3(1), dim3(kBlock), 0, s, gathered, m, rgb_bytes, nq, pick, build_status, region_off,
                       blob_bytes, reinterpret_cast<long long*>(ws), (long long)workspace_bytes - head, flag, status, record_format);
    const auto idct = record_format == RK_JPEG_COEF_DENSE ? k_coef_idct<DenseRecords> : k_coef_idct<WideRecords>;
    hipLaunchKernelGGL(idct, dim3(m, kIdctSlices), dim3(kBlock), 0, s, gathered, qtabs, blob, region_off, pick, ws, status, flag);
    hipLaunchKernelGGL(k_coef_status, dim3(groups), dim3(kBlock), 0, s, flag, m, status);
    hipLaunchKernelGGL(k_jpeg_colour, dim3(m, kColourSlices), dim3(kBlock), 0, s, gathered, ws, status, rgb, rgb_bytes);
    hipLaunchKernelGGL(k_jpeg_count, dim3(1), dim3(kBlock), 0, s, status, m);
    return launch_status();
}

int rk_jpeg_decode_coef_u8(const unsigned char* blob, long long blob_bytes, const rk_jpeg_frame* frames,
                           const unsigned short* qtabs, int nq, int n, const long long* region_off, const int* build_status,
                           const int* pick, const long long* rgb_off, int m, unsigned char* rgb, long long rgb_bytes,
                           void* workspace, size_t workspace_bytes, int* status, rk_stream_t stream) {
    return rk_jpeg_decode_coef_as_u8(blob, blob_bytes, frames, qtabs, nq, n, region_off, build_status, pick, rgb_off, m, rgb,
                                     rgb_bytes, workspace, workspace_bytes, status, stream, RK_JPEG_COEF_WIDE);
}

}  // extern "C"
