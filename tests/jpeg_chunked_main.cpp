// Host run of the chunked index build of the device JPEG decode (rubiksnet_amd/csrc/rk_jpeg_core.hpp): what
// rk_jpeg_build_index_chunked does per frame -- the kernel's own phases, its lanes taken in order between the barriers --
// beside the sequential walk (record_index) on the same frames, on exactly-sized heap buffers.
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
#include "jpeg_host.hpp"

namespace {

constexpr int kLanes = rkjpeg::kChunkBlock;

struct Frame {
    rk_jpeg_frame f;
    rkjpeg::Geometry g;
    rk_jpeg_huff tabs[6];
    std::unique_ptr<unsigned char[]> stream;    // a copy of exactly stream_len bytes
    int E;
};

template <class Phase>
void every_lane(Phase phase) {
    for (int t = 0; t < kLanes; ++t) phase(t);
}

// The chunked route of one frame: the phases the kernel's workgroup runs (rk_jpeg_core.hpp), each for every lane in turn
// where the kernel has a barrier, on exactly nch chunk states -> rounds (> 0: `row` holds the frame's entries and its
// code is 0) or 0 (the frame is the sequential walk's).
int chunked(const Frame& fr, int S, int max_rounds, rk_jpeg_entry* row, int* passed) {
    using namespace rkjpeg;
    const int nch = chunk_count(fr.f, S);
    *passed = 0;
    if (nch < 1 || max_rounds < 1) return 0;
    std::unique_ptr<ChunkState[]> st(new ChunkState[nch]);
    std::unique_ptr<ChunkShared> sh(new ChunkShared);
    std::vector<int> dead((size_t)kLanes);      // a lane-local of the kernel that lives across a barrier
    PtrSrc src{fr.stream.get()};
    every_lane([&](int t) { chunk_init(t, kLanes, *sh, st.get(), nch, S); });
    int rounds = 0;
    for (int r = 1; r <= max_rounds && !rounds; ++r) {
        every_lane([&](int t) { chunk_walk_dirty(t, kLanes, fr.f, fr.g, src, fr.tabs, st.get(), nch, S); });
        every_lane([&](int t) { chunk_advance(t, kLanes, *sh, st.get(), nch, S, r); });
        if (chunk_converged(*sh, r)) rounds = r;
    }
    if (!rounds) return 0;
    every_lane([&](int t) { chunk_run_sums(t, kLanes, *sh, st.get(), nch); });
    every_lane([&](int t) { dead[t] = chunk_sums_in_front(t, kLanes, *sh, st.get(), nch); });
    every_lane([&](int t) {
        chunk_final_pass(t, kLanes, fr.f, fr.g, src, fr.tabs, *sh, st.get(), nch, S, fr.E, row, dead[t]);
    });
    for (int c = 0; c < nch && c <= dead[0]; ++c)
        *passed += st[c].pin >= (c + 1 == nch ? fr.f.stream_len * 8 + 1 : 8LL * (c + 1) * S);
    return chunk_route(*sh, rounds);
}

}  // namespace

int main(int argc, char** argv) {
    int head[4];
    long long sizes[4];
    FILE* fh = open_in(argc, argv, head, sizes);
    if (!fh) return 2;
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
        copy_tables(fr.f, fr.g.ncomp, htabs.get(), fr.tabs);
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
