// Host run of the chunked index build of the device JPEG decode (rubiksnet_amd/csrc/rk_jpeg_core.hpp): what
// rk_jpeg_build_index_chunked does per frame, with the lanes of its workgroup simulated in order and the rounds in
// lock-step, beside the sequential walk (record_index) on the same frames, on exactly-sized heap buffers.
// tests/test_jpeg_chunked.py builds this with -fsanitize=address,undefined: the bounds proof for the kernel's logic, and
// the oracle for its route array.
//
//   jpeg_chunked_main IN OUT
//   IN : int32 n, nq, nh, nsettings; int64 stream_bytes, n_entries, 0, 0; frames [n * 64]; htabs [nh * 1424];
//        streams [stream_bytes]; int32 seg_mcus [n]; int64 entry_off [n + 1]; int32 settings [nsettings][2]: chunk_bytes,
//        max_rounds
//   OUT: int32 chain [n] (the sequential walk's code); its entries [n_entries * 16]; then per setting: int32 status [n],
//        route [n] (0: the sequential walk gave the frame's result, else the rounds after which the chunked walk had
//        converged), passed [n] (chunks of the fixed point that only passed a position through), chunks [n] (the frame's
//        chunk count, 0 where it cannot take the chunked route), entries [n_entries * 16]
// Entries no walk wrote keep the byte 0x5A.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "rk_jpeg_core.hpp"

namespace {

constexpr int kLanes = 1024;

struct PtrSrc {
    const unsigned char* p;
    int byte(long long pos) { return p[pos]; }
};

template <class T>
std::unique_ptr<T[]> read_exact(FILE* fh, size_t count) {       // exactly `count` elements: ASan sees the true end
    std::unique_ptr<T[]> buf(new T[count ? count : 1]);
    if (count && fread(buf.get(), sizeof(T), count, fh) != count) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return buf;
}

struct Frame {
    rk_jpeg_frame f;
    rkjpeg::Geometry g;
    rk_jpeg_huff tabs[6];
    std::unique_ptr<unsigned char[]> stream;    // a copy of exactly stream_len bytes
    int E;
};

// The chunked route of one frame, as the kernel's workgroup takes it -> rounds (> 0: `row` holds the frame's entries and
// its code is 0) or 0 (the frame is the sequential walk's).
int chunked(const Frame& fr, int S, int max_rounds, rk_jpeg_entry* row, int* passed) {
    const int nch = rkjpeg::chunk_count(fr.f, S);
    *passed = 0;
    if (nch < 1 || max_rounds < 1) return 0;
    std::vector<long long> pin((size_t)nch), pout((size_t)nch);
    std::vector<unsigned char> dirty((size_t)nch, 1);
    std::vector<rkjpeg::ChunkSums> sums((size_t)nch);
    PtrSrc src{fr.stream.get()};
    for (int c = 0; c < nch; ++c) pin[c] = 8LL * c * S;
    int rounds = 0;
    for (int r = 1; r <= max_rounds && !rounds; ++r) {
        for (int t = 0; t < kLanes; ++t)
            for (int c = t; c < nch; c += kLanes)
                if (dirty[c]) {
                    dirty[c] = 0;
                    pout[c] = rkjpeg::walk_chunk(fr.f, fr.g, src, fr.tabs, pin[c], 8LL * (c + 1) * S, sums[c]);
                }
        bool changed = false;                   // every lane reads this round's results only: the order does not matter
        for (int t = 0; t < kLanes; ++t)
            for (int c = t; c < nch; c += kLanes) {
                const long long want = rkjpeg::chunk_next_in(c, S, c ? pout[c - 1] : 0);
                if (want != pin[c]) {
                    pin[c] = want;
                    dirty[c] = 1;
                    changed = true;
                }
            }
        if (!changed) rounds = r;
    }
    if (!rounds) return 0;
    int dead = nch;                             // the first dead walk: the sums in front of the chunks up to it are true
    for (int c = nch - 1; c >= 0; --c)
        if (pout[c] < 0) dead = c;
    rkjpeg::ChunkSums run = {0, 0, 0, 0};
    for (int c = 0; c < nch; ++c) {
        const rkjpeg::ChunkSums own = sums[c];
        sums[c] = run;
        run.mcus = (int)((unsigned)run.mcus + (unsigned)own.mcus);
        run.dc0 = (int)((unsigned)run.dc0 + (unsigned)own.dc0);
        run.dc1 = (int)((unsigned)run.dc1 + (unsigned)own.dc1);
        run.dc2 = (int)((unsigned)run.dc2 + (unsigned)own.dc2);
    }
    bool refused = false, finished = false;
    for (int t = 0; t < kLanes; ++t)
        for (int c = t; c < nch; c += kLanes) {
            if (c > dead) continue;
            const bool last = c + 1 == nch;
            const long long end_bit = last ? fr.f.stream_len * 8 + 1 : 8LL * (c + 1) * S;
            if (pin[c] >= end_bit) ++*passed;
            bool done = false;
            if (rkjpeg::index_chunk(fr.f, fr.g, src, fr.tabs, pin[c], end_bit, last ? -1 : pout[c], sums[c], fr.E, row,
                                    &done) != RK_JPEG_OK)
                refused = true;
            finished = finished || done;
        }
    return finished && !refused ? rounds : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    int head[4];
    long long sizes[4];
    if (fread(head, sizeof head, 1, fh) != 1 || fread(sizes, sizeof sizes, 1, fh) != 1) return 2;
    const int n = head[0], nq = head[1], nh = head[2], nset = head[3];
    const long long stream_bytes = sizes[0], n_entries = sizes[1];
    if (n < 1 || nq < 1 || nh < 1 || nset < 0 || stream_bytes < 0 || n_entries < 0) return 2;
    auto frames = read_exact<rk_jpeg_frame>(fh, (size_t)n);
    auto htabs = read_exact<rk_jpeg_huff>(fh, (size_t)nh);
    auto streams = read_exact<unsigned char>(fh, (size_t)stream_bytes);
    auto seg_mcus = read_exact<int>(fh, (size_t)n);
    auto entry_off = read_exact<long long>(fh, (size_t)n + 1);
    auto settings = read_exact<int>(fh, (size_t)nset * 2);
    fclose(fh);

    std::vector<Frame> frs((size_t)n);
    std::vector<int> record((size_t)n), chain((size_t)n);
    std::vector<rk_jpeg_entry> seq((size_t)n_entries);
    memset(seq.data(), 0x5A, sizeof(rk_jpeg_entry) * seq.size());
    for (int i = 0; i < n; ++i) {
        Frame& fr = frs[i];
        fr.f = frames[i];
        fr.E = seg_mcus[i];
        record[i] = chain[i] = rkjpeg::check_resident(fr.f, stream_bytes, nq, nh);
        if (record[i] != RK_JPEG_OK) continue;
        rkjpeg::geometry(fr.f, fr.g);
        if (!rkjpeg::index_row_ok(fr.g, fr.E, entry_off[i], entry_off[i + 1], n_entries)) {
            record[i] = chain[i] = RK_JPEG_BAD_INDEX;
            continue;
        }
        for (int c = 0; c < 3; ++c) {
            fr.tabs[c] = htabs[fr.f.dc[c < fr.g.ncomp ? c : 0]];
            fr.tabs[3 + c] = htabs[fr.f.ac[c < fr.g.ncomp ? c : 0]];
        }
        fr.stream.reset(new unsigned char[fr.f.stream_len ? fr.f.stream_len : 1]);
        memcpy(fr.stream.get(), streams.get() + fr.f.stream_off, (size_t)fr.f.stream_len);
        PtrSrc src{fr.stream.get()};
        chain[i] = rkjpeg::record_index(fr.f, fr.g, src, fr.tabs, fr.E, seq.data() + entry_off[i], true);
    }

    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    fwrite(chain.data(), sizeof(int), chain.size(), fh);
    fwrite(seq.data(), sizeof(rk_jpeg_entry), seq.size(), fh);
    for (int k = 0; k < nset; ++k) {
        const int S = settings[2 * k], max_rounds = settings[2 * k + 1];
        if (!rkjpeg::chunk_bytes_ok(S) || max_rounds < 0 || max_rounds > 64) return 2;
        std::vector<int> status((size_t)n), route((size_t)n, 0), passed((size_t)n, 0), chunks((size_t)n, 0);
        std::vector<rk_jpeg_entry> entries((size_t)n_entries);
        memset(entries.data(), 0x5A, sizeof(rk_jpeg_entry) * entries.size());
        for (int i = 0; i < n; ++i) {
            const Frame& fr = frs[i];
            status[i] = record[i];
            if (record[i] != RK_JPEG_OK) continue;
            chunks[i] = rkjpeg::chunk_count(fr.f, S);
            route[i] = chunked(fr, S, max_rounds, entries.data() + entry_off[i], &passed[i]);
            if (route[i]) {
                status[i] = RK_JPEG_OK;
            } else {                            // the sequential walk, over whatever a refused final pass left behind
                PtrSrc src{fr.stream.get()};
                status[i] = rkjpeg::record_index(fr.f, fr.g, src, fr.tabs, fr.E, entries.data() + entry_off[i], true);
            }
        }
        fwrite(status.data(), sizeof(int), status.size(), fh);
        fwrite(route.data(), sizeof(int), route.size(), fh);
        fwrite(passed.data(), sizeof(int), passed.size(), fh);
        fwrite(chunks.data(), sizeof(int), chunks.size(), fh);
        fwrite(entries.data(), sizeof(rk_jpeg_entry), entries.size(), fh);
    }
    fclose(fh);
    return 0;
}
