// Host run of the scan index of the device JPEG decode (rubiksnet_amd/csrc/rk_jpeg_core.hpp): what rk_jpeg_build_index and
// rk_jpeg_decode_indexed_u8 do per frame and per segment, on exactly-sized heap buffers.  tests/test_jpeg_index.py builds
// this with -fsanitize=address,undefined and runs it over the goldens at several segment lengths, the corrupted corpus and
// a list of tampered entries: the bounds proof for the kernels' logic.
//
//   jpeg_index_main IN OUT
//   IN : int32 n, nq, nh, ntamper; int64 stream_bytes, rgb_bytes, n_entries, 0; frames [n * 64]; htabs [nh * 1424];
//        qtabs [nq * 128]; streams [stream_bytes]; int32 seg_mcus [n]; int64 entry_off [n + 1];
//        int32 tampers [ntamper][4]: frame, kind, entry a, entry b
//   OUT: int32 whole [n] (decode_scan's code), built [n] (the recording walk's code), tiled [n] (1: every segment, decoded
//        alone in reverse order into a fresh buffer, gave code 0, exactly the whole walk's coefficients for its blocks and
//        touched no other block); entries [n_entries * 16]; int32 tampered [ntamper][2]: the frame's code (that of its
//        lowest failing segment), 1 where the RGB still equals the untampered decode; rgb [rgb_bytes] from the segments'
//        coefficients (a failed frame is zeroed; bytes no frame owns keep 0xA5)
// Tamper kinds: 0 bit_pos + 1, 1 bit_pos - 1, 2 bit_pos = 8 * stream_len + 1, 3 bit_pos = -1, 4 pred[0] + 1,
// 5 pred[0] = 4000, 6 entries a and b swapped.
#include "jpeg_host.hpp"

namespace {

constexpr short kUntouched = 0x7F7F;

struct Frame {
    rk_jpeg_frame f;
    rkjpeg::Geometry g;
    rk_jpeg_huff tabs[6];
    const unsigned char* stream;
    int E;
    long long nseg, nmcu;
};

// Segment s alone into a fresh, exactly-sized coefficient buffer -> its code.
int segment(const Frame& fr, const rk_jpeg_entry* entries, long long s, std::vector<short>& out) {
    out.assign((size_t)fr.g.nblocks * 64, kUntouched);
    PtrSrc src{fr.stream};
    BlockSink sink{out.data(), {0}};
    const long long m_begin = s * fr.E, m_end = m_begin + fr.E < fr.nmcu ? m_begin + fr.E : fr.nmcu;
    return rkjpeg::decode_span(fr.f, fr.g, src, fr.tabs, sink, entries[s], m_begin, m_end, s + 1 < fr.nseg ? &entries[s + 1] : nullptr);
}

// Every segment in reverse order; the frame's code is that of its lowest failing segment.  coefs: the segments' blocks
// put together.  *tiled (optional): did every segment write exactly its own blocks, equal to `whole`'s?
int by_segments(const Frame& fr, const rk_jpeg_entry* entries, std::vector<short>& coefs, const short* whole, bool* tiled) {
    coefs.assign((size_t)fr.g.nblocks * 64, 0);
    std::vector<short> one;
    int code = RK_JPEG_OK;
    if (tiled) *tiled = true;
    for (long long s = fr.nseg - 1; s >= 0; --s) {
        const int rc = segment(fr, entries, s, one);
        if (rc != RK_JPEG_OK) code = rc;
        const long long lo = s * fr.E * fr.g.bpm * 64, hi = (s + 1 == fr.nseg ? fr.nmcu : (s + 1) * fr.E) * fr.g.bpm * 64;
        for (long long k = 0; k < (long long)one.size(); ++k) {
            const bool mine = k >= lo && k < hi;
            if (mine) coefs[k] = one[k];
            if (tiled && rc == RK_JPEG_OK && (mine ? one[k] != whole[k] : one[k] != kUntouched)) *tiled = false;
            if (tiled && rc != RK_JPEG_OK) *tiled = false;
        }
    }
    return code;
}

void to_rgb(const Frame& fr, const std::vector<short>& coefs, const unsigned short* qtabs, unsigned char* out) {
    std::vector<unsigned char> region((size_t)fr.g.bytes, 0);
    memcpy(region.data(), coefs.data(), (size_t)fr.g.coef_bytes);
    region_to_rgb(fr.f, fr.g, qtabs, region.data(), out);
}

}  // namespace

int main(int argc, char** argv) {
    int head[4];
    long long sizes[4];
    FILE* fh = open_in(argc, argv, head, sizes);
    if (!fh) return 2;
    const int n = head[0], nq = head[1], nh = head[2], ntamper = head[3];
    const long long stream_bytes = sizes[0], rgb_bytes = sizes[1], n_entries = sizes[2];
    if (n < 1 || nq < 1 || nh < 1 || ntamper < 0 || stream_bytes < 0 || rgb_bytes < 0 || n_entries < 0) return 2;
    auto frames = read_exact<rk_jpeg_frame>(fh, (size_t)n);
    auto htabs = read_exact<rk_jpeg_huff>(fh, (size_t)nh);
    auto qtabs = read_exact<unsigned short>(fh, (size_t)nq * 64);
    auto streams = read_exact<unsigned char>(fh, (size_t)stream_bytes);
    auto seg_mcus = read_exact<int>(fh, (size_t)n);
    auto entry_off = read_exact<long long>(fh, (size_t)n + 1);
    auto tampers = read_exact<int>(fh, (size_t)ntamper * 4);
    fclose(fh);

    std::vector<int> whole((size_t)n, 0), built((size_t)n, 0), tiled((size_t)n, 0), tampered((size_t)ntamper * 2, 0);
    std::unique_ptr<rk_jpeg_entry[]> entries(new rk_jpeg_entry[n_entries ? n_entries : 1]);
    memset(entries.get(), 0x5A, sizeof(rk_jpeg_entry) * (size_t)n_entries);
    std::unique_ptr<unsigned char[]> rgb(new unsigned char[rgb_bytes ? rgb_bytes : 1]);
    memset(rgb.get(), 0xA5, (size_t)rgb_bytes);

    std::vector<Frame> frs((size_t)n);
    for (int i = 0; i < n; ++i) {
        Frame& fr = frs[i];
        fr.f = frames[i];
        fr.E = seg_mcus[i];
        whole[i] = built[i] = rkjpeg::check_record(fr.f, stream_bytes, rgb_bytes, nq, nh, 0, 0);
        if (whole[i] != RK_JPEG_OK) continue;
        rkjpeg::geometry(fr.f, fr.g);
        fr.nmcu = (long long)fr.g.mcux * fr.g.mcuy;
        if (!rkjpeg::index_row_ok(fr.g, fr.E, entry_off[i], entry_off[i + 1], n_entries)) return 2;
        fr.nseg = entry_off[i + 1] - entry_off[i];
        copy_tables(fr.f, fr.g.ncomp, htabs.get(), fr.tabs);
        fr.stream = streams.get() + fr.f.stream_off;
        rk_jpeg_entry* mine = entries.get() + entry_off[i];

        std::vector<short> all((size_t)fr.g.nblocks * 64, kUntouched), coefs;
        {
            PtrSrc src{fr.stream};
            BlockSink sink{all.data(), {0}};
            whole[i] = rkjpeg::decode_scan(fr.f, fr.g, src, fr.tabs, sink);
        }
        {
            PtrSrc src{fr.stream};
            built[i] = rkjpeg::record_index(fr.f, fr.g, src, fr.tabs, fr.E, mine, true);
        }
        unsigned char* out = rgb.get() + fr.f.rgb_off;
        const size_t out_bytes = 3 * (size_t)fr.f.width * fr.f.height;
        if (whole[i] != RK_JPEG_OK || built[i] != RK_JPEG_OK) {
            memset(out, 0, out_bytes);
            continue;
        }
        bool ok;
        const int code = by_segments(fr, mine, coefs, all.data(), &ok);
        tiled[i] = ok && code == RK_JPEG_OK;
        if (code == RK_JPEG_OK) to_rgb(fr, coefs, qtabs.get(), out); else memset(out, 0, out_bytes);
    }

    for (int t = 0; t < ntamper; ++t) {
        const int i = tampers[4 * t], kind = tampers[4 * t + 1], a = tampers[4 * t + 2], b = tampers[4 * t + 3];
        if (i < 0 || i >= n || whole[i] != RK_JPEG_OK || built[i] != RK_JPEG_OK) return 2;
        const Frame& fr = frs[i];
        if (a < 0 || a >= fr.nseg || b < 0 || b >= fr.nseg) return 2;
        std::vector<rk_jpeg_entry> mine(entries.get() + entry_off[i], entries.get() + entry_off[i + 1]);
        switch (kind) {
            case 0: mine[a].bit_pos += 1; break;
            case 1: mine[a].bit_pos -= 1; break;
            case 2: mine[a].bit_pos = fr.f.stream_len * 8 + 1; break;
            case 3: mine[a].bit_pos = -1; break;
            case 4: mine[a].pred[0] = (short)(mine[a].pred[0] + 1); break;
            case 5: mine[a].pred[0] = 4000; break;
            case 6: { const rk_jpeg_entry e = mine[a]; mine[a] = mine[b]; mine[b] = e; break; }
            default: return 2;
        }
        std::vector<short> coefs;
        const int code = by_segments(fr, mine.data(), coefs, nullptr, nullptr);
        tampered[2 * t] = code;
        if (code == RK_JPEG_OK) {
            const size_t out_bytes = 3 * (size_t)fr.f.width * fr.f.height;
            std::vector<unsigned char> again(out_bytes);
            to_rgb(fr, coefs, qtabs.get(), again.data());
            tampered[2 * t + 1] = memcmp(again.data(), rgb.get() + fr.f.rgb_off, out_bytes) == 0;
        }
    }

    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    fwrite(whole.data(), sizeof(int), whole.size(), fh);
    fwrite(built.data(), sizeof(int), built.size(), fh);
    fwrite(tiled.data(), sizeof(int), tiled.size(), fh);
    fwrite(entries.get(), sizeof(rk_jpeg_entry), (size_t)n_entries, fh);
    fwrite(tampered.data(), sizeof(int), tampered.size(), fh);
    fwrite(rgb.get(), 1, (size_t)rgb_bytes, fh);
    fclose(fh);
    return 0;
}
