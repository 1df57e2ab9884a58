// rk_jpeg_core.hpp -- the baseline JPEG decode core of rk_jpeg.hip as plain host/device C++: record check and
// geometry, bit reader, Huffman step, one scan's entropy decode -- whole, or a span of MCUs resumed at a recorded entry,
// the walk that records those entries, and the same entries from many short walks in lock-step rounds -- jidctint's ISLOW
// IDCT, the packed form of a frame's coefficients with its checks, fancy upsampling and YCbCr -> RGB.  The kernels only
// distribute this code over lanes; tests/jpeg_core_main.cpp, tests/jpeg_index_main.cpp, tests/jpeg_chunked_main.cpp,
// tests/jpeg_coef_main.cpp and tests/jpeg_dense_main.cpp compile the same text for the CPU under AddressSanitizer /
// UBSan, which is the bounds proof for the kernels' logic.  That holds for everything in this file, the chunked build's
// per-frame driver included: its phases are here, and what rk_jpeg.hip adds to them is barriers.  It does not hold for
// what only rk_jpeg.hip has: the stream sources, the lane sink, the plan kernels' sums and the launch geometry.
//
// Every function is bounded by counts from the record and reads the stream through a source object that the caller
// bounds; arithmetic that a hostile stream could overflow is done in unsigned (two's complement wrap, as the hardware).
#pragma once
#include <stdint.h>

#include "rubiks_hip.h"

#if defined(__HIPCC__)
#define RKJ_HD __host__ __device__ __forceinline__
#else
#define RKJ_HD inline
#endif

namespace rkjpeg {

// zigzag position -> natural (row-major) position
RKJ_HD int natural_of(int k) {
    static constexpr unsigned char t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k & 63];
}

// ------------------------------------------------------------------------------------------------ geometry
struct Geometry {
    int ncomp;              // 1 or 3
    int hs, vs;             // luma blocks per MCU, horizontally and vertically (1 or 2)
    int mcux, mcuy;         // MCUs per row / column
    int bpm;                // blocks per MCU
    int cw, ch;             // the REAL chroma size: ceil(W / hs), ceil(H / vs) (what the upsampler may look at)
    int yw, yh;             // luma plane size (whole MCUs)
    int pcw, pch;           // chroma plane size (whole MCUs)
    long long nblocks;      // blocks of the frame
    long long coef_bytes;   // nblocks * 64 shorts
    long long plane_off[3]; // byte offsets of the planes behind the coefficients
    long long bytes;        // coefficients + planes, rounded up to 16
};

// Sizes from the record's own fields; false when a field is outside the supported class.
RKJ_HD bool geometry(const rk_jpeg_frame& f, Geometry& g) {
    if (f.width < 1 || f.width > RK_JPEG_MAX_SIDE || f.height < 1 || f.height > RK_JPEG_MAX_SIDE) return false;
    if (f.components != 1 && f.components != 3) return false;
    if (f.components == 3 && (f.sampling < 0 || f.sampling > 2)) return false;
    g.ncomp = f.components;
    g.hs = (f.components == 3 && f.sampling >= 1) ? 2 : 1;
    g.vs = (f.components == 3 && f.sampling == 2) ? 2 : 1;
    g.mcux = (f.width + 8 * g.hs - 1) / (8 * g.hs);
    g.mcuy = (f.height + 8 * g.vs - 1) / (8 * g.vs);
    g.bpm = g.ncomp == 1 ? 1 : g.hs * g.vs + 2;
    g.cw = (f.width + g.hs - 1) / g.hs;
    g.ch = (f.height + g.vs - 1) / g.vs;
    g.yw = g.mcux * 8 * g.hs;
    g.yh = g.mcuy * 8 * g.vs;
    g.pcw = g.mcux * 8;
    g.pch = g.mcuy * 8;
    g.nblocks = (long long)g.mcux * g.mcuy * g.bpm;
    g.coef_bytes = g.nblocks * 128;
    g.plane_off[0] = g.coef_bytes;
    g.plane_off[1] = g.plane_off[0] + (long long)g.yw * g.yh;
    g.plane_off[2] = g.plane_off[1] + (long long)g.pcw * g.pch;
    const long long end = g.ncomp == 1 ? g.plane_off[1] : g.plane_off[2] + (long long)g.pcw * g.pch;
    g.bytes = (end + 15) & ~15LL;
    return true;
}

// Workspace bytes of one record: 0 when its sizes are not valid (such a frame is never decoded).
RKJ_HD long long frame_workspace_bytes(const rk_jpeg_frame& f) {
    Geometry g;
    return geometry(f, g) ? g.bytes : 0;
}

// Bytes of the offset table that heads the workspace: n + 1 int64, rounded up to 16.
RKJ_HD long long offset_table_bytes(int n) { return (((long long)n + 1) * 8 + 15) & ~15LL; }

// May the frame's H * W * 3 bytes be written?  (asked even of a record that is otherwise invalid: it is zeroed then)
RKJ_HD bool rgb_range_ok(const rk_jpeg_frame& f, long long rgb_bytes) {
    if (f.width < 1 || f.width > RK_JPEG_MAX_SIDE || f.height < 1 || f.height > RK_JPEG_MAX_SIDE) return false;
    const long long need = (long long)f.width * f.height * 3;
    return f.rgb_off >= 0 && f.rgb_off <= rgb_bytes && need <= rgb_bytes - f.rgb_off;
}

// A resident record (rk_jpeg_build_index) alone: RK_JPEG_OK or RK_JPEG_BAD_RECORD.  Its sizes, its segment and its
// tables; not the output range and the workspace, which a resident frame gets only when it is picked.
RKJ_HD int check_resident(const rk_jpeg_frame& f, long long stream_bytes, int nq, int nh) {
    Geometry g;
    if (!geometry(f, g)) return RK_JPEG_BAD_RECORD;
    if (f.stream_off < 0 || f.stream_len < 0 || f.stream_off > stream_bytes || f.stream_len > stream_bytes - f.stream_off)
        return RK_JPEG_BAD_RECORD;
    if (f.restart_interval < 0 || f.restart_interval > 65535) return RK_JPEG_BAD_RECORD;
    for (int c = 0; c < g.ncomp; ++c)
        if (f.quant[c] >= nq || f.dc[c] >= nh || f.ac[c] >= nh) return RK_JPEG_BAD_RECORD;
    return RK_JPEG_OK;
}

// A record that is decoded where it stands: check_resident's checks, the output range, and ws_end, the end of the frame's
// region of the workspace.  Spelt out, not composed of check_resident: every composition tried gave k_jpeg_plan other
// instructions than it had, and that kernel is in every decode launch (profiles/jpeg_refactor.txt).
RKJ_HD int check_record(const rk_jpeg_frame& f, long long stream_bytes, long long rgb_bytes, int nq, int nh,
                        long long ws_end, long long workspace_bytes) {
    Geometry g;
    if (!geometry(f, g)) return RK_JPEG_BAD_RECORD;
    if (!rgb_range_ok(f, rgb_bytes)) return RK_JPEG_BAD_RECORD;
    if (f.stream_off < 0 || f.stream_len < 0 || f.stream_off > stream_bytes || f.stream_len > stream_bytes - f.stream_off)
        return RK_JPEG_BAD_RECORD;
    if (f.restart_interval < 0 || f.restart_interval > 65535) return RK_JPEG_BAD_RECORD;
    for (int c = 0; c < g.ncomp; ++c)
        if (f.quant[c] >= nq || f.dc[c] >= nh || f.ac[c] >= nh) return RK_JPEG_BAD_RECORD;
    if (ws_end > workspace_bytes) return RK_JPEG_BAD_RECORD;
    return RK_JPEG_OK;
}

// Bytes in front of the plain workspace in an indexed decode: the m gathered records, then the per-segment codes.
RKJ_HD long long gathered_bytes(int m) { return (long long)m * 64; }
RKJ_HD long long indexed_head_bytes(int m, int max_segments) {
    return gathered_bytes(m) + ((((long long)m * max_segments) * 4 + 15) & ~15LL);
}

// ------------------------------------------------------------------------------------------------ bits
// Src: `int byte(long long pos)` for 0 <= pos < len, the byte at that position of the frame's segment.
// The reader never asks for a position outside [0, len).  Bits past the end or past a marker read as zero and are
// counted (`fake`): a decoder that used one has run off the data.
// kTrack: keep what bit_pos() needs; the whole-frame decode never asks and does without.
template <class Src, bool kTrack = true>
struct BitReader {
    Src& src;
    long long pos, len;
    unsigned acc;           // the next bits, most significant first
    int bits;               // valid bits in acc
    int fake;               // how many of them are zeros that stand for missing data
    unsigned wide;          // a 4-bit shift register, newest in bit 0: was the data byte read k bytes ago an FF 00 pair?
    bool stopped;           // a marker or the end was reached: nothing more is read

    RKJ_HD BitReader(Src& s, long long n) : src(s), pos(0), len(n), acc(0), bits(0), fake(0), wide(0), stopped(false) {}

    // Start afresh at raw bit position p (0 <= p <= 8 * len; see bit_pos).  A position inside the 00 of an FF 00 pair, or
    // any other a walk never stood at, is read as what the bytes from there on spell: bounded like everything else.
    RKJ_HD void seek(long long p) {
        pos = p >> 3;
        acc = 0;
        bits = fake = 0;
        wide = 0;
        stopped = false;
        fill();
        drop((int)(p & 7));
    }
    // 8 * (offset of the raw byte that holds the next unread bit) + (bit in that byte, 0 = most significant); FF 00 is two
    // raw bytes and its bits live in the FF.  With no real bit left: the byte the reader would read next (the marker's FF
    // or len once stopped), bit 0.  The reader holds at most four data bytes, whose raw widths `wide` remembers.
    RKJ_HD long long bit_pos() const {
        const int real = bits - fake;
        if (real <= 0) return pos * 8;
        const int nb = (real + 7) >> 3;                                     // 1..4 data bytes held, the first in part
        const int raw = nb + __builtin_popcount(wide & ((1u << nb) - 1u));
        return (pos - raw) * 8 + (nb * 8 - real);
    }

    RKJ_HD bool at_stop() {
        if (pos >= len) return true;
        if (src.byte(pos) != 0xFF) return false;
        return pos + 1 >= len || src.byte(pos + 1) != 0x00;
    }
    RKJ_HD void fill() {    // at least 25 bits afterwards; at most 4 rounds
        while (bits <= 24) {
            unsigned b = 0;
            if (!stopped) {
                if (pos >= len) {
                    stopped = true;
                } else {
                    b = (unsigned)src.byte(pos) & 0xFFu;
                    if (b != 0xFF) {
                        pos += 1;
                        if (kTrack) wide <<= 1;
                    } else if (pos + 1 < len && src.byte(pos + 1) == 0x00) {
                        pos += 2;                       // FF 00 is the data byte FF
                        if (kTrack) wide = (wide << 1) | 1u;
                    } else {
                        stopped = true;                 // a marker (or a lone FF at the end): not consumed
                        b = 0;
                    }
                }
            }
            if (stopped) fake += 8;
            acc |= b << (24 - bits);
            bits += 8;
        }
    }
    RKJ_HD unsigned peek(int n) const { return acc >> (32 - n); }       // 1 <= n <= 25, after fill()
    RKJ_HD void drop(int n) { acc <<= n; bits -= n; }
    RKJ_HD bool overrun() const { return bits < fake; }                   // a fake bit was consumed

    // The end of an entropy-coded interval: less than a byte of real bits left, all ones, and a marker or the end next.
    RKJ_HD int end_interval() {
        if (overrun()) return RK_JPEG_TRUNCATED;
        const int real = bits - fake;
        if (real >= 8) return RK_JPEG_TRAILING;
        if (real > 0 && peek(real) != (1u << real) - 1u) return RK_JPEG_TRAILING;
        if (!stopped && !at_stop()) return RK_JPEG_TRAILING;
        return RK_JPEG_OK;
    }
    // Between two intervals: the marker must be RSTn with n == expected; the reader starts afresh behind it.
    RKJ_HD int restart(int expected) {
        const int rc = end_interval();
        if (rc != RK_JPEG_OK) return rc;
        if (pos + 1 >= len || src.byte(pos) != 0xFF || src.byte(pos + 1) != 0xD0 + (expected & 7)) return RK_JPEG_BAD_RESTART;
        pos += 2;
        acc = 0;
        bits = fake = 0;
        stopped = false;
        return RK_JPEG_OK;
    }
    RKJ_HD int finish() {
        const int rc = end_interval();
        if (rc != RK_JPEG_OK) return rc;
        return pos >= len ? RK_JPEG_OK : RK_JPEG_TRAILING;              // a marker inside the segment: data left over
    }
};

// One Huffman symbol, or -1 when the bits are no code.  Every index is masked: the table is untrusted device data.
template <class Src, bool kTrack>
RKJ_HD int huff_symbol(BitReader<Src, kTrack>& br, const rk_jpeg_huff& h) {
    br.fill();
    const unsigned e = h.look[br.peek(9) & 511];
    const int l = (int)(e >> 8);
    if (l >= 1 && l <= 9) {
        br.drop(l);
        return (int)(e & 255);
    }
    for (int n = 10; n <= 16; ++n) {
        const int code = (int)br.peek(n);
        if (code <= h.maxcode[n]) {
            br.drop(n);
            return h.huffval[(unsigned)(code + h.valoff[n]) & 255];
        }
    }
    return -1;
}

// s bits as a JPEG signed magnitude (1 <= s <= 15)
template <class Src, bool kTrack>
RKJ_HD int receive_extend(BitReader<Src, kTrack>& br, int s) {
    br.fill();
    const int v = (int)br.peek(s);
    br.drop(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// ------------------------------------------------------------------------------------------------ one scan
// Sink: put(zigzag_position, value) for the non-zero coefficients of the current block (the sink maps the position to
// natural order: natural_of, or its inverse once per lane -- a table lookup per coefficient here would be a global
// memory round trip on the device), end_block(block_index) after each; the blocks come in scan order (MCU by MCU; in an MCU the luma blocks row by row, then Cb, then Cr).
// tabs: the frame's six tables, DC of component c at [c], AC at [3 + c].
// Returns a RK_JPEG_* code; on an error the blocks from the failing one on have not been written.
//
// The walk can be entered at any MCU m whose ENTRY is known: the reader's bit_pos() and the three DC predictors at the
// top of the loop's iteration m, before that iteration's restart handling (rk_jpeg_entry, include/rubiks_hip.h).  The
// restart state needs no storing: with R = restart_interval > 0, the iterations R, 2R, ... <= m - 1 have each passed a
// marker, j = (m - 1) / R of them, so the next marker is RST(j & 7), and the countdown was set to R at iteration j * R (or
// at the start) and has run m - j * R times since.
struct NoRecorder {
    static constexpr bool enabled = false;
    RKJ_HD void at(long long, long long, int, int, int) {}
};

struct NullSink {
    RKJ_HD void put(int, int) {}
    RKJ_HD void end_block(long long) {}
};

// One block of component c, the only entropy block loop there is: the DC symbol and the predictor's update, the AC
// symbols into sink.put, the overrun check (sink.end_block is the caller's); a refusal RETURNS its code from the function
// that holds the block.  p0..p2 are the three predictors as scalars (a lane-private array indexed by c lives in scratch
// memory); the DC difference is added in unsigned, so that a caller that lets the sums run (range false: they are sums of
// differences, not predictors yet) wraps; range: the sum is the predictor and must stay inside +-2047, where the unsigned
// sum is the signed one.
// A macro, not a function, with its locals in the caller's scope (one use per scope): as a force-inlined function the
// same text came out of the compiler with its blocks laid out otherwise, and the chain kernels, which are this loop
// and little else, ran 5 % longer (profiles/jpeg_refactor.txt).  Expanded so, they are the instructions they were; its own
// scope (do { } while (0)) changes them again, so it has none.
#define RKJ_DECODE_BLOCK(range, br, tabs, c, p0, p1, p2, sink)                                          \
    int s_ = huff_symbol((br), (tabs)[c]);                                                              \
    if (s_ < 0) return RK_JPEG_BAD_CODE;                                                                \
    if (s_ > 11) return RK_JPEG_BAD_VALUE;                                                              \
    int dcv_ = (c) == 0 ? (p0) : ((c) == 1 ? (p1) : (p2));                                              \
    if (s_) dcv_ = (int)((unsigned)dcv_ + (unsigned)receive_extend((br), s_));                          \
    if ((range) && (dcv_ < -2047 || dcv_ > 2047)) return RK_JPEG_BAD_VALUE;                             \
    (p0) = (c) == 0 ? dcv_ : (p0);                                                                      \
    (p1) = (c) == 1 ? dcv_ : (p1);                                                                      \
    (p2) = (c) == 2 ? dcv_ : (p2);                                                                      \
    if (dcv_) (sink).put(0, dcv_);                                                                      \
    int k_ = 1;                                                                                         \
    for (int guard_ = 0; guard_ < 63 && k_ < 64; ++guard_) { /* at most 63 symbols a block */           \
        const int rs_ = huff_symbol((br), (tabs)[3 + (c)]);                                             \
        if (rs_ < 0) return RK_JPEG_BAD_CODE;                                                           \
        const int r_ = rs_ >> 4;                                                                        \
        s_ = rs_ & 15;                                                                                  \
        if (s_ == 0) {                                                                                  \
            if (r_ != 15) break; /* EOB */                                                              \
            k_ += 16;            /* ZRL: a coefficient of this block must follow */                     \
            if (k_ > 63) return RK_JPEG_BAD_RUN;                                                        \
            continue;                                                                                   \
        }                                                                                               \
        k_ += r_;                                                                                       \
        if (k_ > 63) return RK_JPEG_BAD_RUN;                                                            \
        if (s_ > 10) return RK_JPEG_BAD_VALUE;                                                          \
        (sink).put(k_, receive_extend((br), s_));                                                       \
        ++k_;                                                                                           \
    }                                                                                                   \
    if ((br).overrun()) return RK_JPEG_TRUNCATED;

RKJ_HD bool entry_equals(const rk_jpeg_entry& e, long long bit_pos, int p0, int p1, int p2) {
    return e.bit_pos == bit_pos && e.pred[0] == p0 && e.pred[1] == p1 && e.pred[2] == p2;
}

// MCUs [m_begin, m_end) of the scan, resumed at `entry`; block indices handed to the sink stay frame-global.  A span that
// ends before the last MCU must leave the reader exactly at *next (position and predictors), the last one at the end of
// the stream (BitReader::finish): spans that each return RK_JPEG_OK therefore tile the stream.  The entries are
// untrusted: RK_JPEG_BAD_INDEX, before any read, for a range outside the frame, a bit_pos outside [0, 8 * stream_len], a
// predictor outside +-2047 or an entry of MCU 0 that is not zero; RK_JPEG_BAD_INDEX after the span's last MCU where
// the reader does not stand at *next.  rec.at(m, bit_pos, pred0, pred1, pred2) sees every entry of the span when
// Rec::enabled.  kWhole: the caller only ever walks [0, nmcu) from the zero entry (anything else is RK_JPEG_BAD_INDEX), so
// no position is asked for unless a recorder does, and the reader keeps none: the plain decode's loop as it always was.
template <bool kWhole, class Src, class Sink, class Rec>
RKJ_HD int walk_span(const rk_jpeg_frame& f, const Geometry& g, Src& src, const rk_jpeg_huff* tabs, Sink& sink, Rec& rec,
                     const rk_jpeg_entry& entry, long long m_begin, long long m_end, const rk_jpeg_entry* next) {
    const int nluma = g.ncomp == 1 ? 1 : g.hs * g.vs;
    const long long nmcu = (long long)g.mcux * g.mcuy;
    if (m_begin < 0 || m_begin >= m_end || m_end > nmcu || (m_end < nmcu && !next)) return RK_JPEG_BAD_INDEX;
    if (kWhole && (m_begin != 0 || m_end != nmcu)) return RK_JPEG_BAD_INDEX;
    if (entry.bit_pos < 0 || entry.bit_pos > f.stream_len * 8) return RK_JPEG_BAD_INDEX;
    int pred0 = entry.pred[0], pred1 = entry.pred[1], pred2 = entry.pred[2];    // scalars, not an array: a lane-private array indexed by c lives in scratch memory
    if (pred0 < -2047 || pred0 > 2047 || pred1 < -2047 || pred1 > 2047 || pred2 < -2047 || pred2 > 2047) return RK_JPEG_BAD_INDEX;
    if (m_begin == 0 && (entry.bit_pos | pred0 | pred1 | pred2) != 0) return RK_JPEG_BAD_INDEX;
    BitReader<Src, !kWhole || Rec::enabled> br(src, f.stream_len);
    int next_rst = 0, until_rst = f.restart_interval;
    if (!kWhole && m_begin > 0) {
        br.seek(entry.bit_pos);
        if (f.restart_interval > 0) {
            const long long j = (m_begin - 1) / f.restart_interval;
            next_rst = (int)(j & 7);
            until_rst = (int)(f.restart_interval - (m_begin - j * f.restart_interval));
        }
    }
    long long block = m_begin * g.bpm;
    for (long long m = m_begin; m < m_end; ++m) {
        if (Rec::enabled) rec.at(m, br.bit_pos(), pred0, pred1, pred2);
        if (f.restart_interval > 0) {
            if (until_rst == 0) {
                const int rc = br.restart(next_rst);
                if (rc != RK_JPEG_OK) return rc;
                next_rst = (next_rst + 1) & 7;
                until_rst = f.restart_interval;
                pred0 = pred1 = pred2 = 0;
            }
            --until_rst;
        }
        for (int j = 0; j < g.bpm; ++j, ++block) {
            const int c = j < nluma ? 0 : j - nluma + 1;
            RKJ_DECODE_BLOCK(true, br, tabs, c, pred0, pred1, pred2, sink)
            sink.end_block(block);
        }
    }
    if (kWhole || m_end == nmcu) return br.finish();
    return entry_equals(*next, br.bit_pos(), pred0, pred1, pred2) ? RK_JPEG_OK : RK_JPEG_BAD_INDEX;
}

// The whole frame: the span [0, nmcu) from the zero entry.
template <class Src, class Sink>
RKJ_HD int decode_scan(const rk_jpeg_frame& f, const Geometry& g, Src& src, const rk_jpeg_huff* tabs, Sink& sink) {
    rk_jpeg_entry zero = {0, {0, 0, 0}, 0};
    NoRecorder none;
    return walk_span<true>(f, g, src, tabs, sink, none, zero, 0, (long long)g.mcux * g.mcuy, nullptr);
}

template <class Src, class Sink>
RKJ_HD int decode_span(const rk_jpeg_frame& f, const Geometry& g, Src& src, const rk_jpeg_huff* tabs, Sink& sink,
                       const rk_jpeg_entry& entry, long long m_begin, long long m_end, const rk_jpeg_entry* next) {
    NoRecorder none;
    return walk_span<false>(f, g, src, tabs, sink, none, entry, m_begin, m_end, next);
}

// ------------------------------------------------------------------------------------------------ the scan index
// Segments of a frame walked in pieces of E MCUs: how many, and is the frame's row of the index table usable?
RKJ_HD long long segment_count(const Geometry& g, int E) { return ((long long)g.mcux * g.mcuy + E - 1) / E; }
RKJ_HD bool index_row_ok(const Geometry& g, int E, long long first, long long last, long long n_entries) {
    if (E < 1 || first < 0 || last < first || last > n_entries) return false;
    return last - first == segment_count(g, E);
}

RKJ_HD void write_entry(rk_jpeg_entry* e, long long bit_pos, int p0, int p1, int p2) {
    e->bit_pos = bit_pos;
    e->pred[0] = (short)p0;
    e->pred[1] = (short)p1;
    e->pred[2] = (short)p2;
    e->reserved = 0;
}

// Writes the entry of every E-th MCU; `writer` says whether this caller stores (one lane of a wave that walks together).
struct EntryRecorder {
    static constexpr bool enabled = true;
    rk_jpeg_entry* out;
    int E, left;            // left: MCUs until the next entry
    bool writer;
    RKJ_HD void at(long long, long long bit_pos, int p0, int p1, int p2) {
        if (left == 0) {
            if (writer) write_entry(out, bit_pos, p0, p1, p2);
            ++out;
            left = E;
        }
        --left;
    }
};

// The one sequential walk a resident frame gets: no coefficient is stored, out[s] becomes the entry of MCU s * E for
// every segment s (the caller has checked index_row_ok).  Returns the code decode_scan returns for the frame.
template <class Src>
RKJ_HD int record_index(const rk_jpeg_frame& f, const Geometry& g, Src& src, const rk_jpeg_huff* tabs, int E,
                        rk_jpeg_entry* out, bool writer) {
    rk_jpeg_entry zero = {0, {0, 0, 0}, 0};
    NullSink sink;
    EntryRecorder rec{out, E, 0, writer};
    return walk_span<true>(f, g, src, tabs, sink, rec, zero, 0, (long long)g.mcux * g.mcuy, nullptr);
}

// ------------------------------------------------------------------------------------------------ the chunked index build
// The same index without the frame-long chain (rk_jpeg_build_index_chunked).  A frame without restart markers is cut into
// chunks of S raw bytes; chunk c covers the bit positions [8 c S, 8 (c + 1) S).  A WALK of chunk c takes a position p_in
// to be the start of an MCU and decodes whole MCUs until the first MCU boundary at or past the chunk's end, p_out; its
// state is that one position, because a walk stops at MCU boundaries only.  Rounds in lock-step: in round 1 every chunk
// starts at its own first bit, in round r + 1 at p_out of the chunk before it from round r (its own first bit again
// where that walk was refused: a refusal must not travel down the frame).  Chunk 0 always starts at bit 0, the true
// start, so by induction chunks 0 .. r - 1 hold the sequential walk's positions after round r: a fixed point IS the
// sequential walk, and Huffman streams fall into step so quickly that it is reached in a few rounds, not in nchunks.
// The MCU counts and DC sums of the walks, summed over the chunks in front, then give every chunk its first MCU
// number and predictors, and a final pass walks each chunk once more and writes the entries.
constexpr int kMaxChunks = 4096;        // the largest chunk count of a frame that takes the chunked route

RKJ_HD bool chunk_bytes_ok(int S) { return S == 16 || S == 32 || S == 64 || S == 128 || S == 256 || S == 512; }

// Chunks of the frame at S bytes each; 0 where the frame takes the sequential chain whatever its contents: restart
// markers, an empty segment, more than kMaxChunks chunks.  From two fields alone, so that the host can size the workspace.
RKJ_HD int chunk_count(const rk_jpeg_frame& f, int S) {
    if (f.restart_interval != 0 || f.stream_len < 1 || f.stream_len > (long long)S * kMaxChunks) return 0;
    return (int)((f.stream_len + S - 1) / S);
}
// Workspace of the chunked build: an offset table like the decoder's, then 32 bytes per chunk (its positions and sums).
RKJ_HD long long chunked_workspace_bytes(long long total_chunks, int n) { return offset_table_bytes(n) + total_chunks * 32; }

struct ChunkSums {          // of one walk: MCUs completed, DC differences added up per component (wrapping; see index_chunk)
    int mcus, dc0, dc1, dc2;
};

// One MCU with nothing stored: walk_span's loop body.  p0..p2 are running sums of the DC differences; kRange: they are
// the true predictors and must stay inside +-2047.
template <bool kRange, class Src>
RKJ_HD int skip_mcu(BitReader<Src, true>& br, const Geometry& g, int nluma, const rk_jpeg_huff* tabs, int& p0, int& p1, int& p2) {
    NullSink none;
    for (int j = 0; j < g.bpm; ++j) {
        const int c = j < nluma ? 0 : j - nluma + 1;
        RKJ_DECODE_BLOCK(kRange, br, tabs, c, p0, p1, p2, none)
    }
    return RK_JPEG_OK;
}

// A speculative walk of one chunk from p_in (0 <= p_in <= 8 * stream_len) -> p_out, or -1 where the walk is DEAD: any
// refusal, or a bit used past the end or past a marker.  p_in at or past end_bit passes through: p_out = p_in, no MCU.
// Every MCU moves the position on by at least two bits or is refused: at most ceil(bits / 2) MCUs start inside the chunk,
// and one more look at the position ends the loop.
template <class Src>
RKJ_HD long long walk_chunk(const rk_jpeg_frame& f, const Geometry& g, Src& src, const rk_jpeg_huff* tabs, long long p_in,
                            long long end_bit, ChunkSums& sums) {
    sums.mcus = sums.dc0 = sums.dc1 = sums.dc2 = 0;
    if (p_in >= end_bit) return p_in;
    const int nluma = g.ncomp == 1 ? 1 : g.hs * g.vs;
    BitReader<Src, true> br(src, f.stream_len);
    br.seek(p_in);
    for (long long guard = (end_bit - p_in + 1) / 2 + 1; guard > 0; --guard) {
        const long long pos = br.bit_pos();
        if (pos >= end_bit) return pos;
        if (skip_mcu<false>(br, g, nluma, tabs, sums.dc0, sums.dc1, sums.dc2) != RK_JPEG_OK) return -1;
        ++sums.mcus;
    }
    return -1;
}

// Where chunk c starts in the next round, given the chunk before it ended at prev_out in this one.
RKJ_HD long long chunk_next_in(int c, int S, long long prev_out) {
    return c == 0 ? 0 : (prev_out >= 0 ? prev_out : 8LL * c * S);
}

// The final pass over one chunk of a converged frame: p_in is its true start, `before` what the chunks in front of it
// add up to -- its first MCU number and, DC differences being what predictors are sums of, its predictors.  (The sums
// wrap; where every chunk in front kept its predictors inside +-2047, which each checks here, the wrapped sum is the
// true one.)  Writes out[m / E] for every MCU m with m % E == 0 that starts in the chunk (out: the frame's row of the
// index; m < nmcu, so the row holds it).  The chunk in which MCU nmcu - 1 ends applies BitReader::finish() there and
// reports it in *finished; a chunk that starts at or past MCU nmcu has nothing to do.  Any other chunk must end exactly
// at expect_out, the next chunk's start.  end_bit of the last chunk: past 8 * stream_len, which no position reaches.
// Returns RK_JPEG_OK or the refusal; the frame has taken the chunked route only if no chunk refused and one finished.
template <class Src>
RKJ_HD int index_chunk(const rk_jpeg_frame& f, const Geometry& g, Src& src, const rk_jpeg_huff* tabs, long long p_in,
                       long long end_bit, long long expect_out, const ChunkSums& before, int E, rk_jpeg_entry* out,
                       bool* finished) {
    const long long nmcu = (long long)g.mcux * g.mcuy;
    long long m = before.mcus;
    if (m < 0) return RK_JPEG_BAD_INDEX;
    if (m >= nmcu) return RK_JPEG_OK;
    if (p_in >= end_bit) return p_in == expect_out ? RK_JPEG_OK : RK_JPEG_BAD_INDEX;
    int p0 = before.dc0, p1 = before.dc1, p2 = before.dc2;
    if (p0 < -2047 || p0 > 2047 || p1 < -2047 || p1 > 2047 || p2 < -2047 || p2 > 2047) return RK_JPEG_BAD_VALUE;
    if (p_in < 0 || p_in > f.stream_len * 8 || E < 1) return RK_JPEG_BAD_INDEX;
    const int nluma = g.ncomp == 1 ? 1 : g.hs * g.vs;
    BitReader<Src, true> br(src, f.stream_len);
    br.seek(p_in);
    long long until = (E - m % E) % E;                      // MCUs until the next entry
    rk_jpeg_entry* at = out + (m + E - 1) / E;
    for (long long guard = (end_bit - p_in + 1) / 2 + 1; guard > 0; --guard) {
        const long long pos = br.bit_pos();
        if (pos >= end_bit) return pos == expect_out ? RK_JPEG_OK : RK_JPEG_BAD_INDEX;
        if (until == 0) {
            write_entry(at++, pos, p0, p1, p2);
            until = E;
        }
        --until;
        const int rc = skip_mcu<true>(br, g, nluma, tabs, p0, p1, p2);
        if (rc != RK_JPEG_OK) return rc;
        if (++m == nmcu) {
            const int end = br.finish();
            *finished = end == RK_JPEG_OK;
            return end;
        }
    }
    return RK_JPEG_BAD_INDEX;
}

// The chunked build of one frame by `lanes` lanes (at most kChunkBlock), lane t taking chunks t, t + lanes, ...: the
// PHASES below, each called by every lane with a barrier after it and none inside.  k_jpeg_index_chunked is that sequence
// with __syncthreads() for the barriers, tests/jpeg_chunked_main.cpp runs each phase for t = 0 .. lanes - 1 in turn; no
// phase reads what another lane writes in the same phase, so both compute the same.
//
//   chunk_init
//   for r = 1 .. max_rounds:  chunk_walk_dirty;  chunk_advance(r);  leave with rounds = r where chunk_converged(r)
//   (never converged: the frame is the sequential walk's)
//   chunk_run_sums;  dead = chunk_sums_in_front;  chunk_final_pass(dead);  chunk_route(rounds)
constexpr int kChunkBlock = 1024;

struct ChunkState {         // 32 bytes of the workspace per chunk
    ChunkSums sums;         // of the chunk's last walk; after chunk_sums_in_front: of all chunks in front of it
    int pin, pout;          // bit positions (at most 8 * 512 * kMaxChunks); pout -1: the walk is dead
    int dirty, reserved;    // p_in changed: the chunk is walked in the next round
};
static_assert(sizeof(ChunkState) == 32, "ChunkState is 32 bytes");

struct ChunkShared {        // of one frame, shared by its lanes
    int part[kChunkBlock][4], part_dead[kChunkBlock];
    int changed[2], refused, finished;
};

RKJ_HD int chunk_min(int a, int b) { return a < b ? a : b; }

RKJ_HD void chunk_init(int t, int lanes, ChunkShared& sh, ChunkState* __restrict__ st, int nch, int S) {
    for (int c = t; c < nch; c += lanes) {
        st[c].pin = 8 * c * S;
        st[c].dirty = 1;
    }
    if (t == 0) sh.changed[0] = sh.changed[1] = sh.refused = sh.finished = 0;
}

template <class Src>
RKJ_HD void chunk_walk_dirty(int t, int lanes, const rk_jpeg_frame& f, const Geometry& g, Src& src, const rk_jpeg_huff* tabs,
                             ChunkState* __restrict__ st, int nch, int S) {
    for (int c = t; c < nch; c += lanes) {
        if (!st[c].dirty) continue;
        st[c].dirty = 0;
        ChunkSums own;
        st[c].pout = (int)walk_chunk(f, g, src, tabs, st[c].pin, 8LL * (c + 1) * S, own);
        st[c].sums = own;
    }
}

// Jacobi: every p_in comes from the round just walked.  This round's flag is changed[r & 1]; the other one, which every
// lane read before it came through the barrier in front of this phase, is cleared for the next round.
RKJ_HD void chunk_advance(int t, int lanes, ChunkShared& sh, ChunkState* __restrict__ st, int nch, int S, int r) {
    if (t == 0) sh.changed[(r + 1) & 1] = 0;
    for (int c = t; c < nch; c += lanes) {
        const int want = (int)chunk_next_in(c, S, c ? st[c - 1].pout : 0);
        if (want != st[c].pin) {
            st[c].pin = want;
            st[c].dirty = 1;
            sh.changed[r & 1] = 1;
        }
    }
}
RKJ_HD bool chunk_converged(const ChunkShared& sh, int r) { return !sh.changed[r & 1]; }    // the same word for every lane

// The sums in front of every chunk, in two levels: each lane a run of `per` consecutive chunks, then the lanes' totals.
RKJ_HD void chunk_run(int t, int lanes, int nch, int& per, int& lo, int& hi) {
    per = (nch + lanes - 1) / lanes;
    lo = chunk_min(nch, t * per);
    hi = chunk_min(nch, lo + per);
}

RKJ_HD void chunk_run_sums(int t, int lanes, ChunkShared& sh, const ChunkState* __restrict__ st, int nch) {
    int per, lo, hi;
    chunk_run(t, lanes, nch, per, lo, hi);
    unsigned a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    int dead = nch;
    for (int c = hi - 1; c >= lo; --c) {
        const ChunkSums own = st[c].sums;
        a0 += (unsigned)own.mcus;
        a1 += (unsigned)own.dc0;
        a2 += (unsigned)own.dc1;
        a3 += (unsigned)own.dc2;
        if (st[c].pout < 0) dead = c;
    }
    sh.part[t][0] = (int)a0;
    sh.part[t][1] = (int)a1;
    sh.part[t][2] = (int)a2;
    sh.part[t][3] = (int)a3;
    sh.part_dead[t] = dead;
}

// st[c].sums becomes what the chunks in front of c add up to.  -> the first dead walk (nch: none): the sums in front
// of the chunks up to it are true.
RKJ_HD int chunk_sums_in_front(int t, int lanes, const ChunkShared& sh, ChunkState* __restrict__ st, int nch) {
    int per, lo, hi;
    chunk_run(t, lanes, nch, per, lo, hi);
    unsigned a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    int dead = nch;
    const int used = chunk_min(lanes, (nch + per - 1) / per);      // the lanes whose runs are not empty
    for (int k = 0; k < used; ++k) {
        if (k < t) {
            a0 += (unsigned)sh.part[k][0];
            a1 += (unsigned)sh.part[k][1];
            a2 += (unsigned)sh.part[k][2];
            a3 += (unsigned)sh.part[k][3];
        }
        dead = chunk_min(dead, sh.part_dead[k]);
    }
    for (int c = lo; c < hi; ++c) {
        const ChunkSums own = st[c].sums;
        st[c].sums = ChunkSums{(int)a0, (int)a1, (int)a2, (int)a3};
        a0 += (unsigned)own.mcus;
        a1 += (unsigned)own.dc0;
        a2 += (unsigned)own.dc1;
        a3 += (unsigned)own.dc2;
    }
    return dead;
}

template <class Src>
RKJ_HD void chunk_final_pass(int t, int lanes, const rk_jpeg_frame& f, const Geometry& g, Src& src, const rk_jpeg_huff* tabs,
                             ChunkShared& sh, const ChunkState* __restrict__ st, int nch, int S, int E,
                             rk_jpeg_entry* __restrict__ row, int dead) {
    for (int c = t; c < nch && c <= dead; c += lanes) {
        const bool last = c + 1 == nch;
        const ChunkSums before = st[c].sums;
        bool done = false;
        const int rc = index_chunk(f, g, src, tabs, st[c].pin, last ? f.stream_len * 8 + 1 : 8LL * (c + 1) * S,
                                   last ? -1LL : (long long)st[c].pout, before, E, row, &done);
        if (rc != RK_JPEG_OK) sh.refused = 1;
        if (done) sh.finished = 1;
    }
}
// -> the rounds after which the walk had converged, 0 where the frame is left to the sequential walk.
RKJ_HD int chunk_route(const ChunkShared& sh, int rounds) { return sh.finished && !sh.refused ? rounds : 0; }

// ------------------------------------------------------------------------------------------------ IDCT
// libjpeg's jidctint.c (jpeg_idct_islow), 8-bit samples: CONST_BITS 13, PASS1_BITS 2, dequantisation by multiplication,
// the all-zero-AC column shortcut, the masked range limit.  out: 8 rows of 8 samples, `stride` bytes apart.
RKJ_HD unsigned idct_descale(unsigned x, int n) { return (unsigned)((int)(x + (1u << (n - 1))) >> n); }
RKJ_HD unsigned char idct_limit(unsigned x) {
    // range_limit[(x & 1023) + 128]: the 10-bit field read as signed, plus 128, clamped to a sample
    const int s = (int)((x & 1023u) ^ 512u) - 512 + 128;
    return (unsigned char)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

RKJ_HD void idct_islow(const short* coef, const unsigned short* q, unsigned char* out, long long stride) {
    typedef unsigned U;
    constexpr U F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299,
                F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
    U ws[64];
#define RKJ_IDCT_BODY(I0, I1, I2, I3, I4, I5, I6, I7)                                                  \
    U z2 = I2, z3 = I6;                                                                                \
    U z1 = (z2 + z3) * F0_541;                                                                         \
    U tmp2 = z1 - z3 * F1_847;                                                                         \
    U tmp3 = z1 + z2 * F0_765;                                                                         \
    z2 = I0;                                                                                           \
    z3 = I4;                                                                                           \
    U tmp0 = (z2 + z3) << 13;                                                                          \
    U tmp1 = (z2 - z3) << 13;                                                                          \
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;        \
    tmp0 = I7;                                                                                         \
    tmp1 = I5;                                                                                         \
    tmp2 = I3;                                                                                         \
    tmp3 = I1;                                                                                         \
    z1 = tmp0 + tmp3;                                                                                  \
    z2 = tmp1 + tmp2;                                                                                  \
    z3 = tmp0 + tmp2;                                                                                  \
    U z4 = tmp1 + tmp3;                                                                                \
    const U z5 = (z3 + z4) * F1_175;                                                                   \
    tmp0 *= F0_298;                                                                                    \
    tmp1 *= F2_053;                                                                                    \
    tmp2 *= F3_072;                                                                                    \
    tmp3 *= F1_501;                                                                                    \
    z1 *= 0u - F0_899;                                                                                 \
    z2 *= 0u - F2_562;                                                                                 \
    z3 *= 0u - F1_961;                                                                                 \
    z4 *= 0u - F0_390;                                                                                 \
    z3 += z5;                                                                                          \
    z4 += z5;                                                                                          \
    tmp0 += z1 + z3;                                                                                   \
    tmp1 += z2 + z4;                                                                                   \
    tmp2 += z2 + z3;                                                                                   \
    tmp3 += z1 + z4;
#define RKJ_DQ(r) ((U)(int)coef[(r) * 8 + c] * (U)q[(r) * 8 + c])
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if ((coef[8 + c] | coef[16 + c] | coef[24 + c] | coef[32 + c] | coef[40 + c] | coef[48 + c] | coef[56 + c]) == 0) {
            const U dcval = RKJ_DQ(0) << 2;
#pragma unroll
            for (int r = 0; r < 8; ++r) ws[r * 8 + c] = dcval;
            continue;
        }
        RKJ_IDCT_BODY(RKJ_DQ(0), RKJ_DQ(1), RKJ_DQ(2), RKJ_DQ(3), RKJ_DQ(4), RKJ_DQ(5), RKJ_DQ(6), RKJ_DQ(7))
        ws[0 * 8 + c] = idct_descale(tmp10 + tmp3, 11);
        ws[7 * 8 + c] = idct_descale(tmp10 - tmp3, 11);
        ws[1 * 8 + c] = idct_descale(tmp11 + tmp2, 11);
        ws[6 * 8 + c] = idct_descale(tmp11 - tmp2, 11);
        ws[2 * 8 + c] = idct_descale(tmp12 + tmp1, 11);
        ws[5 * 8 + c] = idct_descale(tmp12 - tmp1, 11);
        ws[3 * 8 + c] = idct_descale(tmp13 + tmp0, 11);
        ws[4 * 8 + c] = idct_descale(tmp13 - tmp0, 11);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const U* w = ws + r * 8;
        unsigned char* o = out + r * stride;
        RKJ_IDCT_BODY(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7])
        o[0] = idct_limit(idct_descale(tmp10 + tmp3, 18));
        o[7] = idct_limit(idct_descale(tmp10 - tmp3, 18));
        o[1] = idct_limit(idct_descale(tmp11 + tmp2, 18));
        o[6] = idct_limit(idct_descale(tmp11 - tmp2, 18));
        o[2] = idct_limit(idct_descale(tmp12 + tmp1, 18));
        o[5] = idct_limit(idct_descale(tmp12 - tmp1, 18));
        o[3] = idct_limit(idct_descale(tmp13 + tmp0, 18));
        o[4] = idct_limit(idct_descale(tmp13 - tmp0, 18));
    }
#undef RKJ_DQ
#undef RKJ_IDCT_BODY
}

// Where block `b` (scan order) of the frame goes: component and the byte offset of its top-left sample in that
// component's plane; *stride = the plane's row pitch.
RKJ_HD void block_place(const Geometry& g, long long b, int* comp, long long* offset, int* stride) {
    const long long m = b / g.bpm;
    const int j = (int)(b % g.bpm);
    const int my = (int)(m / g.mcux), mx = (int)(m % g.mcux);
    const int nluma = g.ncomp == 1 ? 1 : g.hs * g.vs;
    if (j < nluma) {
        const int by = my * g.vs + j / g.hs, bx = mx * g.hs + j % g.hs;
        *comp = 0;
        *stride = g.yw;
        *offset = (long long)by * 8 * g.yw + bx * 8;
    } else {
        *comp = j - nluma + 1;
        *stride = g.pcw;
        *offset = (long long)my * 8 * g.pcw + mx * 8;
    }
}

// ------------------------------------------------------------------------------------------------ packed coefficients
// What the entropy stage leaves -- short[64] per block, natural order, not dequantised -- kept without its zeros
// (rk_jpeg_coef_sizes / rk_jpeg_coef_pack / rk_jpeg_decode_coef_u8).  One frame's REGION, every part on a 2-byte boundary:
//
//   uint32 off[nblocks]    byte offset of block b's record from the region's start (blocks in block_place's order, MCU
//                          padding blocks included); read and written as two 16-bit halves, low half first
//   records, back to back, in block order: off[0] = 4 * nblocks, off[b + 1] = off[b] + bytes(b), the last one ends the region
//
//   record   uint64 header (four 16-bit words, lowest first): bit 0 = the AC values are 16-bit, bit k (1..63) = the AC
//                   coefficient at zigzag position k is not zero
//            int16  DC
//            the non-zero AC values in zigzag order, int8 each where all of them fit, else int16 each (little endian),
//            then one zero byte where that leaves an odd count:  10 + n * w rounded up to even, 10 .. 136 bytes
//
// The offsets make any block addressable on its own; the records still tile the region, which is what a reader checks:
// every access is bounded from the frame's geometry (the table), the region's length (the 10 bytes of header and DC) and
// the header (the values), and a block whose record does not end where the next one starts -- or the region, for the
// last -- is refused, so no changed offset, header or length decodes as something else.  Geometry allows an 8x8 block
// every one of the 63 AC positions, so the only header refused on its own is the one no packer writes: 16-bit values
// with no value.
// Src: `unsigned u16(long long at)` (at even) and `int s8(long long at)`, positions in bytes from the region's start.
// Dst: `void put16(long long at, unsigned v)` (at even) and `void put8(long long at, int v)`.
constexpr int kCoefRecordMin = 10, kCoefRecordMax = 136;

RKJ_HD long long coef_table_bytes(const Geometry& g) { return g.nblocks * 4; }
// The planes alone of a frame's workspace region (Geometry::bytes without the 128 bytes per block), a multiple of 16.
RKJ_HD long long plane_bytes(const Geometry& g) { return g.bytes - g.coef_bytes; }
RKJ_HD long long frame_plane_bytes(const rk_jpeg_frame& f) {
    Geometry g;
    return geometry(f, g) ? plane_bytes(g) : 0;
}

RKJ_HD int coef_ac_count(unsigned long long header) { return __builtin_popcountll(header >> 1); }
RKJ_HD int coef_record_bytes(unsigned long long header) {
    const int n = coef_ac_count(header), w = (header & 1) ? 2 : 1;
    return kCoefRecordMin + ((n * w + 1) & ~1);
}
RKJ_HD bool coef_header_ok(unsigned long long header) { return (header & 1) == 0 || (header >> 1) != 0; }

// The header of a block's 64 coefficients (natural order).
RKJ_HD unsigned long long coef_header_of(const short* coef) {
    unsigned long long mask = 0;
    bool wide = false;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = coef[natural_of(k)];
        if (v != 0) mask |= 1ull << k;
        wide = wide || v < -128 || v > 127;
    }
    return mask | (wide ? 1ull : 0ull);
}

// Writes the block's record at `at`; coef_record_bytes(header) bytes, every one of them.
template <class Dst>
RKJ_HD void coef_pack_block(const short* coef, unsigned long long header, Dst& dst, long long at) {
#pragma unroll
    for (int h = 0; h < 4; ++h) dst.put16(at + 2 * h, (unsigned)(header >> (16 * h)) & 0xFFFFu);
    dst.put16(at + 8, (unsigned)coef[0] & 0xFFFFu);
    const bool wide = (header & 1) != 0;
    long long p = at + kCoefRecordMin;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        if (!((header >> k) & 1)) continue;
        const int v = coef[natural_of(k)];
        if (wide) {
            dst.put16(p, (unsigned)v & 0xFFFFu);
            p += 2;
        } else {
            dst.put8(p, v);
            p += 1;
        }
    }
    if ((p - at) & 1) dst.put8(p, 0);
}

template <class Src>
RKJ_HD unsigned long long coef_read_header(Src& src, long long at) {
    unsigned long long header = 0;
#pragma unroll
    for (int h = 0; h < 4; ++h) header |= (unsigned long long)(src.u16(at + 2 * h) & 0xFFFFu) << (16 * h);
    return header;
}

// The record at `at` back into 64 coefficients (natural order); reads coef_record_bytes(header) bytes at most.  The
// loop is unrolled with every index a constant, so that on the device coef[] stays in registers.
template <class Src>
RKJ_HD void coef_expand_block(Src& src, long long at, unsigned long long header, short* coef) {
    coef[0] = (short)src.u16(at + 8);
    const bool wide = (header & 1) != 0;
    long long p = at + kCoefRecordMin;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        short v = 0;
        if ((header >> k) & 1) {
            if (wide) {
                v = (short)src.u16(p);
                p += 2;
            } else {
                v = (short)src.s8(p);
                p += 1;
            }
        }
        coef[natural_of(k)] = v;
    }
}

// May bytes [lo, hi) of a blob of blob_bytes be frame g's region?  Inside the blob, on a 2-byte boundary, and long enough
// for the table and the smallest record of every block (so the table can be read); at most what the blocks can take.
RKJ_HD bool coef_region_ok(long long lo, long long hi, long long blob_bytes, const Geometry& g) {
    if (lo < 0 || hi < lo || hi > blob_bytes || (lo & 1)) return false;
    const long long len = hi - lo;
    return len >= g.nblocks * (4 + kCoefRecordMin) && len <= g.nblocks * (4 + kCoefRecordMax);
}

RKJ_HD long long coef_offset_of(unsigned lo16, unsigned hi16) { return (long long)((lo16 & 0xFFFFu) | ((hi16 & 0xFFFFu) << 16)); }

// Block b of a region that passed coef_region_ok: its offset from the table, inside the region with room for header and
// DC before the header is read; then the header, and the record must end exactly where block b + 1 starts (the region,
// for the last block).  true: *at and *header are the block's, and every byte of the record lies inside the region.
template <class Src>
RKJ_HD bool coef_block_ok(Src& src, long long region_len, const Geometry& g, long long b, long long* at,
                          unsigned long long* header) {
    const long long off = coef_offset_of(src.u16(4 * b), src.u16(4 * b + 2));
    const long long end = b + 1 < g.nblocks ? coef_offset_of(src.u16(4 * b + 4), src.u16(4 * b + 6)) : region_len;
    if ((off & 1) || off < coef_table_bytes(g) || off > region_len - kCoefRecordMin) return false;
    if (b == 0 && off != coef_table_bytes(g)) return false;
    const unsigned long long h = coef_read_header(src, off);
    if (!coef_header_ok(h) || off + coef_record_bytes(h) != end || end > region_len) return false;
    *at = off;
    *header = h;
    return true;
}

// ------------------------------------------------------------------------------------------------ dense records
// The second record format of the same packed set (RK_JPEG_COEF_DENSE; the one above is RK_JPEG_COEF_WIDE and stays as it
// is).  Video frames have, per block, one to three large low-frequency values and some 25 small ones, so the value class
// is chosen per COEFFICIENT: a 4-bit nibble each, and a byte or a word only for the few that do not fit one.  One
// frame's region, little endian, every record on a 2-byte boundary, no padding between regions:
//
//   uint32 base[G]         G = ceil(nblocks / 64); read and written as two 16-bit halves, low half first
//   uint16 rel[nblocks]    block b's record starts base[b / 64] + rel[b] bytes from the region's start (blocks in
//                          block_place's order, MCU padding blocks included).  The packer writes base[g] = the start of
//                          record 64 g, so rel[64 g] = 0 and rel <= 63 * 130.
//   records, back to back, in block order: the first at 4 G + 2 nblocks, the last one ends the region
//
//   ordinary record
//     uint8  tag            bits 0-5 `last`: the zigzag position of the last non-zero AC (0: no AC); bits 6-7 the class
//     int16  DC             (at an odd offset: read and written as bytes)
//     ceil(last / 8) mask bytes: bit j of the mask = the AC at zigzag position j + 1 is not zero
//     ceil(n / 2) bytes of nibbles, one per non-zero AC in zigzag order, low nibble first: the value in 4-bit two's
//                           complement where it lies in -7 .. 7, 0x8 = escaped (a nibble of 0 names no value)
//     the e escaped values in order: int8 each in class 0, int16 each in class 1 (used when one of them leaves int8)
//     one zero byte where that leaves an odd count:  roundup2(3 + ceil(last / 8) + ceil(n / 2) + e w), 4 .. 130 bytes
//   raw record (class 2), for a block whose ordinary record would exceed 130 bytes
//     tag 0x80, a zero byte, int16[64] in natural order: 130 bytes
//
// A reader takes a record's SPAN -- [its start, the next record's start), the region's end for the last -- from the
// table alone (dense_block_span), checks every read of the record against that span before it makes it, and refuses a
// record whose own length, from its tag, mask, nibbles and class, is not exactly the span (dense_expand_block).  The
// loops are bounded by the 63 positions and the block count.
// Src and Dst as above.
constexpr int kDenseRecordMin = 4, kDenseRecordMax = 130, kDenseGroup = 64;

RKJ_HD long long dense_groups(const Geometry& g) { return (g.nblocks + kDenseGroup - 1) / kDenseGroup; }
RKJ_HD long long dense_table_bytes(const Geometry& g) { return 4 * dense_groups(g) + 2 * g.nblocks; }

struct DenseShape {         // of a block's 64 coefficients: what its record's length follows from
    int last, n, e;         // the last non-zero AC's zigzag position, the non-zero ACs, those outside -7 .. 7
    bool wide, raw;         // an escaped value leaves int8; the ordinary record would exceed kDenseRecordMax
};

RKJ_HD int dense_ordinary_bytes(int last, int n, int e, bool wide) {
    return (3 + ((last + 7) >> 3) + ((n + 1) >> 1) + e * (wide ? 2 : 1) + 1) & ~1;
}

RKJ_HD DenseShape dense_shape_of(const short* coef) {
    DenseShape s = {0, 0, 0, false, false};
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = coef[natural_of(k)];
        if (v != 0) {
            s.last = k;
            ++s.n;
        }
        if (v < -7 || v > 7) ++s.e;
        s.wide = s.wide || v < -128 || v > 127;
    }
    s.raw = dense_ordinary_bytes(s.last, s.n, s.e, s.wide) > kDenseRecordMax;
    return s;
}
RKJ_HD int dense_record_bytes(const DenseShape& s) {
    return s.raw ? kDenseRecordMax : dense_ordinary_bytes(s.last, s.n, s.e, s.wide);
}

// Writes the block's record at `at` (even); dense_record_bytes(s) bytes, every one of them.
template <class Dst>
RKJ_HD void dense_pack_block(const short* coef, const DenseShape& s, Dst& dst, long long at) {
    if (s.raw) {
        dst.put16(at, 0x0080u);
#pragma unroll
        for (int k = 0; k < 64; ++k) dst.put16(at + 2 + 2 * k, (unsigned)coef[k] & 0xFFFFu);
        return;
    }
    dst.put8(at, s.last | (s.wide ? 0x40 : 0));
    dst.put8(at + 1, coef[0] & 0xFF);
    dst.put8(at + 2, (coef[0] >> 8) & 0xFF);
    const int mb = (s.last + 7) >> 3;
    long long np = at + 3 + mb, ep = np + ((s.n + 1) >> 1);
    unsigned mbyte = 0, nbyte = 0;
    int c = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = coef[natural_of(k)];
        if (v != 0) {
            mbyte |= 1u << ((k - 1) & 7);
            const bool small = v >= -7 && v <= 7;
            nbyte |= (small ? (unsigned)v & 15u : 8u) << (4 * (c & 1));
            if (c & 1) {
                dst.put8(np++, (int)nbyte);
                nbyte = 0;
            }
            ++c;
            if (!small) {
                dst.put8(ep++, v & 0xFF);
                if (s.wide) dst.put8(ep++, (v >> 8) & 0xFF);
            }
        }
        if ((k & 7) == 0 || k == 63) {                  // positions 8 i + 1 .. 8 i + 8 are mask byte i
            if (((k - 1) >> 3) < mb) dst.put8(at + 3 + ((k - 1) >> 3), (int)mbyte);
            mbyte = 0;
        }
    }
    if (c & 1) dst.put8(np, (int)nbyte);
    if ((ep - at) & 1) dst.put8(ep, 0);
}

// May bytes [lo, hi) of a blob of blob_bytes be frame g's dense region?  Inside the blob, both ends on a 2-byte boundary,
// and between the table plus the smallest and the table plus the largest record of every block.
RKJ_HD bool dense_region_ok(long long lo, long long hi, long long blob_bytes, const Geometry& g) {
    if (lo < 0 || hi < lo || hi > blob_bytes || (lo & 1) || (hi & 1)) return false;
    const long long len = hi - lo, table = dense_table_bytes(g);
    return len >= table + g.nblocks * kDenseRecordMin && len <= table + g.nblocks * kDenseRecordMax;
}

RKJ_HD long long dense_start_of(unsigned base_lo, unsigned base_hi, unsigned rel) { return coef_offset_of(base_lo, base_hi) + (long long)(rel & 0xFFFFu); }

// Block b of a region that passed dense_region_ok, from the table alone: its record's start -- behind the table, even,
// with room for the smallest record; exactly behind the table for block 0 -- and its span up to the next record's start
// (the region's end for the last block), 4 .. 130 bytes inside the region.  true: [*at, *at + *span) is the record's.
template <class Src>
RKJ_HD bool dense_block_span(Src& src, long long region_len, const Geometry& g, long long b, long long* at, int* span) {
    const long long rel0 = 4 * dense_groups(g), table = dense_table_bytes(g);
    const long long gb = b / kDenseGroup, gn = (b + 1) / kDenseGroup;
    const long long off = dense_start_of(src.u16(4 * gb), src.u16(4 * gb + 2), src.u16(rel0 + 2 * b));
    const long long end = b + 1 < g.nblocks ? dense_start_of(src.u16(4 * gn), src.u16(4 * gn + 2), src.u16(rel0 + 2 * b + 2)) : region_len;
    if ((off & 1) || off < table || off > region_len - kDenseRecordMin) return false;
    if (b == 0 && off != table) return false;
    if (end > region_len || end - off < kDenseRecordMin || end - off > kDenseRecordMax) return false;
    *at = off;
    *span = (int)(end - off);
    return true;
}

// The record in [at, at + span) -- dense_block_span's: at even, span even -- back into 64 coefficients (natural order),
// checked as it is read: false for class 3, a raw record with last != 0 or another span than 130, a mask whose bit
// `last` is clear or that has a bit above it, a nibble of 0 for a coefficient the mask names, a read that would leave
// the span, and a record whose own length is not the span; coef is then not to be used.  No read is made before it is
// known to lie in the span.  The mask sits in one 64-bit word; the nibbles come out of a 32-bit window that is refilled
// every eighth nibble from an address that follows from the count of nibbles taken, which the mask gives, so no load
// but an escaped value's waits for loaded data; the loop is unrolled with every index a constant, so that on the
// device coef[] stays in registers.
template <class Src>
RKJ_HD bool dense_expand_block(Src& src, long long at, int span, short* coef) {
    const unsigned w0 = src.u16(at), w1 = src.u16(at + 2);              // span >= 4
    const int last = (int)(w0 & 63u), cls = (int)((w0 >> 6) & 3u);
    if (cls == 2) {
        if (last != 0 || span != kDenseRecordMax) return false;
        coef[0] = (short)w1;
#pragma unroll
        for (int k = 1; k < 64; ++k) coef[k] = (short)src.u16(at + 2 + 2 * k);
        return true;
    }
    const int mb = (last + 7) >> 3, w = cls == 1 ? 2 : 1;
    if (cls == 3 || 3 + mb > span) return false;
    coef[0] = (short)((w0 >> 8) | ((w1 & 0xFFu) << 8));
    unsigned long long m = w1 >> 8;                                     // byte 3 of the record is mask byte 0
#pragma unroll
    for (int i = 0; i < 4; ++i)                                         // bytes 4 + 2 i, 5 + 2 i: mask bytes 1 + 2 i, 2 + 2 i
        if (4 + 2 * i < 3 + mb) m |= (unsigned long long)(src.u16(at + 4 + 2 * i) & 0xFFFFu) << (8 + 16 * i);
    if (mb < 8) m &= (1ull << (8 * mb)) - 1ull;
    if (last > 0 && (m >> (last - 1)) != 1ull) return false;
    const int n = __builtin_popcountll(m);
    const int nib_at = 3 + mb;
    int ep = nib_at + ((n + 1) >> 1);                                   // the escaped values' place
    if (ep > span) return false;
    const unsigned long long mask = m << 1;                             // bit k: zigzag position k
    const int a0 = nib_at & ~1;
    int c = (nib_at & 1) ? 2 : 0;                                       // nibbles from a0 on
    unsigned win = 0;
    if (a0 < span) win = src.u16(at + a0) & 0xFFFFu;
    if (a0 + 2 < span) win |= (src.u16(at + a0 + 2) & 0xFFFFu) << 16;
    bool bad = false;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        int v = 0;
        if ((mask >> k) & 1) {
            const unsigned nib = (win >> (4 * (c & 7))) & 15u;
            ++c;
            if ((c & 7) == 0) {
                const int r = a0 + (c >> 1);
                win = r < span ? src.u16(at + r) & 0xFFFFu : 0u;
                if (r + 2 < span) win |= (src.u16(at + r + 2) & 0xFFFFu) << 16;
            }
            v = (int)(nib ^ 8u) - 8;
            bad = bad || nib == 0;
            if (nib == 8) {
                v = 0;
                if (ep + w <= span) {
                    v = w == 2 ? (int)(short)((src.s8(at + ep) & 0xFF) | ((src.s8(at + ep + 1) & 0xFF) << 8)) : src.s8(at + ep);
                } else {
                    bad = true;
                }
                ep += w;
            }
        }
        coef[natural_of(k)] = (short)v;
    }
    return !bad && ((ep + 1) & ~1) == span;
}

// The two formats by number, for what both share: the scans, the plan and the host's bounds.
RKJ_HD bool coef_format_ok(int format) { return format == RK_JPEG_COEF_WIDE || format == RK_JPEG_COEF_DENSE; }
RKJ_HD long long coef_table_bytes_as(int format, const Geometry& g) {
    return format == RK_JPEG_COEF_DENSE ? dense_table_bytes(g) : coef_table_bytes(g);
}
RKJ_HD bool coef_region_ok_as(int format, long long lo, long long hi, long long blob_bytes, const Geometry& g) {
    return format == RK_JPEG_COEF_DENSE ? dense_region_ok(lo, hi, blob_bytes, g) : coef_region_ok(lo, hi, blob_bytes, g);
}

// A record that is decoded from a packed region: its sizes, its output range, its quantisation tables and ws_end, the
// end of its planes in the workspace.  RK_JPEG_OK or RK_JPEG_BAD_RECORD.
RKJ_HD int check_coef_record(const rk_jpeg_frame& f, long long rgb_bytes, int nq, long long ws_end, long long workspace_bytes) {
    Geometry g;
    if (!geometry(f, g)) return RK_JPEG_BAD_RECORD;
    if (!rgb_range_ok(f, rgb_bytes)) return RK_JPEG_BAD_RECORD;
    for (int c = 0; c < g.ncomp; ++c)
        if (f.quant[c] >= nq) return RK_JPEG_BAD_RECORD;
    if (ws_end > workspace_bytes) return RK_JPEG_BAD_RECORD;
    return RK_JPEG_OK;
}

// Bytes in front of the planes in rk_jpeg_decode_coef_u8's workspace: the m gathered records, a flag per picked frame,
// then the offset table.
RKJ_HD long long coef_head_bytes(int m) { return gathered_bytes(m) + (((long long)m * 4 + 15) & ~15LL); }

// ------------------------------------------------------------------------------------------------ upsampling and colour
// One chroma sample at output pixel (x, y) as libjpeg's jdsample.c gives it.  plane: the component's plane, pitch pcw;
// only columns < cw and rows < ch are looked at (the real samples; what partial MCUs decode beyond them is padding).
//   4:4:4                     the sample itself
//   cw <= 2                   box replication (libjpeg takes the plain upsamplers for such narrow components)
//   4:2:2  h2v1_fancy         even x: (3 s[i] + s[i-1] + 1) >> 2, odd x: (3 s[i] + s[i+1] + 2) >> 2
//   4:2:0  h2v2_fancy         column sums 3 near + far row, then even x: (3 t + l + 8) >> 4, odd x: (3 t + r + 7) >> 4
// with an edge column standing in for its missing neighbour, row -1 = row 0 and row ch = row ch - 1.
RKJ_HD int chroma_at(const unsigned char* plane, const Geometry& g, int x, int y) {
    if (g.hs == 1) return plane[(long long)y * g.pcw + x];
    const int i = x >> 1;
    if (g.cw <= 2) return plane[(long long)(g.vs == 2 ? y >> 1 : y) * g.pcw + i];
    const int nb = (x & 1) ? (i + 1 < g.cw ? i + 1 : i) : (i > 0 ? i - 1 : i);
    if (g.vs == 1) {
        const unsigned char* row = plane + (long long)y * g.pcw;
        return (3 * row[i] + row[nb] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int r = y >> 1;
    const int far = (y & 1) ? (r + 1 < g.ch ? r + 1 : r) : (r > 0 ? r - 1 : r);
    const unsigned char* near_row = plane + (long long)r * g.pcw;
    const unsigned char* far_row = plane + (long long)far * g.pcw;
    const int t = 3 * near_row[i] + far_row[i];
    const int n = 3 * near_row[nb] + far_row[nb];
    return (3 * t + n + ((x & 1) ? 7 : 8)) >> 4;
}

RKJ_HD unsigned char clamp_u8(int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// jdcolor.c's tables as arithmetic: SCALEBITS 16, FIX(x) = (int)(x * 65536 + 0.5), arithmetic right shifts.
RKJ_HD void ycc_to_rgb(int y, int cb, int cr, unsigned char* rgb) {
    const int u = cb - 128, v = cr - 128;
    rgb[0] = clamp_u8(y + ((91881 * v + 32768) >> 16));
    rgb[1] = clamp_u8(y + ((-22554 * u - 46802 * v + 32768) >> 16));
    rgb[2] = clamp_u8(y + ((116130 * u + 32768) >> 16));
}

// The RGB of output pixel (x, y) from the frame's planes (`base`: the frame's workspace region).
RKJ_HD void pixel_rgb(const unsigned char* base, const Geometry& g, int x, int y, unsigned char* rgb) {
    const int luma = base[g.plane_off[0] + (long long)y * g.yw + x];
    if (g.ncomp == 1) {
        rgb[0] = rgb[1] = rgb[2] = (unsigned char)luma;
        return;
    }
    ycc_to_rgb(luma, chroma_at(base + g.plane_off[1], g, x, y), chroma_at(base + g.plane_off[2], g, x, y), rgb);
}

#undef RKJ_DECODE_BLOCK

}  // namespace rkjpeg
