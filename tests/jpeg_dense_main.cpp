// Host run of the DENSE record format of the packed coefficients (rubiksnet_amd/csrc/rk_jpeg_core.hpp): what
// rk_jpeg_coef_sizes_as, rk_jpeg_coef_pack_as and rk_jpeg_decode_coef_as_u8 do per frame and per block with
// RK_JPEG_COEF_DENSE, on exactly-sized heap buffers.  tests/test_jpeg_dense.py builds this with
// -fsanitize=address,undefined and runs it over the set of tests/_jpeg_dense_cases.py and a table of tampered regions: the
// bounds proof for the kernels' logic.
//
//   jpeg_dense_main IN OUT
//   IN : int32 n, nq, nh, ntamper; int64 stream_bytes, rgb_bytes, 0, 0; frames [n * 64]; htabs [nh * 1424];
//        qtabs [nq * 128]; streams [stream_bytes]; int32 tampers [ntamper][3]: frame, kind, block
//   OUT: int32 code [n] (decode_scan's code); int32 exact [n] (1: every block expanded from its record equals the walked
//        block); int32 kinds [n][5]: blocks with no AC, with nibbles only, with int8 escapes, with int16 escapes, raw;
//        int64 first_block [n + 1]; int64 region_off [n + 1] (a refused frame: length 0); int16 coefs
//        [first_block[n] * 64] as walked (refused frames: zeros); blob [region_off[n]]; rgb [rgb_bytes] decoded from the
//        blob (a refused frame is zeroed; bytes no frame owns keep 0xA5); then per tamper: int32 code, int32 same (1: code
//        0 and the RGB equals the untampered decode), int64 lo, hi, bytes and the `bytes` bytes of the tampered copy of
//        the frame's region -- [lo, hi) is the region claimed in a blob of `bytes` bytes
// Tamper kinds (block: the block whose table entry or record is changed; for 2 - 4 the group is the block's):
//   0 rel + 2, 1 rel - 2, 2 base + 2, 3 base - 2, 4 base past the region, 5 the region's offset past the blob, 6 the region
//   cut by 2 bytes, 7 last + 1, 8 last - 1, 9 the lowest clear mask bit below last set, 10 the class bit flipped (0 <-> 1),
//   11 class 3, 12 the first value nibble turned into 0x8, 13 the first escape nibble turned into the value 1, 14 the tag
//   replaced by the raw tag.  Kinds 7 - 14 return 2 where the block's record is not an ordinary one that has what they change.
#include "jpeg_host.hpp"

namespace {

struct BytesSrc {           // a region held in a buffer of exactly its bytes
    const unsigned char* p;
    unsigned u16(long long at) const {
        unsigned short v;
        memcpy(&v, p + at, 2);
        return v;
    }
    int s8(long long at) const { return (signed char)p[at]; }
};
struct BytesDst {
    unsigned char* p;
    void put16(long long at, unsigned v) {
        const unsigned short w = (unsigned short)v;
        memcpy(p + at, &w, 2);
    }
    void put8(long long at, int v) { p[at] = (unsigned char)v; }
};

struct Frame {
    rk_jpeg_frame f;
    rkjpeg::Geometry g;
    std::vector<short> coefs;
};

// One block out of a region held in exactly its bytes: the table, then the record against its span.
bool load_block(BytesSrc& src, long long len, const rkjpeg::Geometry& g, long long b, short* coef) {
    long long at;
    int span;
    return rkjpeg::dense_block_span(src, len, g, b, &at, &span) && rkjpeg::dense_expand_block(src, at, span, coef);
}

// rk_jpeg_decode_coef_as_u8 for one frame: region [lo, hi) of a blob of blob_bytes.  The region is copied into a buffer of
// exactly hi - lo bytes first, so that a read past either end is a sanitizer report, not a neighbour's byte.
int decode_packed(const Frame& fr, const unsigned char* blob, long long blob_bytes, long long lo, long long hi,
                  const unsigned short* qtabs, unsigned char* out) {
    const size_t out_bytes = 3 * (size_t)fr.f.width * fr.f.height;
    memset(out, 0, out_bytes);
    if (!rkjpeg::dense_region_ok(lo, hi, blob_bytes, fr.g)) return RK_JPEG_BAD_INDEX;
    const long long len = hi - lo;
    std::unique_ptr<unsigned char[]> region(new unsigned char[(size_t)len]);
    memcpy(region.get(), blob + lo, (size_t)len);
    BytesSrc src{region.get()};
    std::vector<unsigned char> ws((size_t)fr.g.bytes, 0);
    bool bad = false;
    for (long long b = 0; b < fr.g.nblocks; ++b) {
        short coef[64];
        if (!load_block(src, len, fr.g, b, coef)) {
            bad = true;
            continue;
        }
        int comp, stride;
        long long off;
        rkjpeg::block_place(fr.g, b, &comp, &off, &stride);
        rkjpeg::idct_islow(coef, qtabs + (long long)fr.f.quant[comp] * 64, ws.data() + fr.g.plane_off[comp] + off, stride);
    }
    if (bad) return RK_JPEG_BAD_INDEX;
    const int npix = fr.f.width * fr.f.height;
    for (int p = 0; p < npix; ++p) rkjpeg::pixel_rgb(ws.data(), fr.g, p % fr.f.width, p / fr.f.width, out + 3LL * p);
    return RK_JPEG_OK;
}

long long get_base(const unsigned char* region, long long grp) {
    BytesSrc src{region};
    return rkjpeg::coef_offset_of(src.u16(4 * grp), src.u16(4 * grp + 2));
}
void put_base(unsigned char* region, long long grp, long long v) {
    BytesDst dst{region};
    dst.put16(4 * grp, (unsigned)v & 0xFFFFu);
    dst.put16(4 * grp + 2, (unsigned)(v >> 16) & 0xFFFFu);
}

}  // namespace

int main(int argc, char** argv) {
    int head[4];
    long long sizes[4];
    FILE* fh = open_in(argc, argv, head, sizes);
    if (!fh) return 2;
    const int n = head[0], nq = head[1], nh = head[2], ntamper = head[3];
    const long long stream_bytes = sizes[0], rgb_bytes = sizes[1];
    if (n < 1 || nq < 1 || nh < 1 || ntamper < 0 || stream_bytes < 0 || rgb_bytes < 0) return 2;
    auto frames = read_exact<rk_jpeg_frame>(fh, (size_t)n);
    auto htabs = read_exact<rk_jpeg_huff>(fh, (size_t)nh);
    auto qtabs = read_exact<unsigned short>(fh, (size_t)nq * 64);
    auto streams = read_exact<unsigned char>(fh, (size_t)stream_bytes);
    auto tampers = read_exact<int>(fh, (size_t)ntamper * 3);
    fclose(fh);

    std::vector<int> code((size_t)n, 0), exact((size_t)n, 0), kinds((size_t)n * 5, 0);
    std::vector<long long> first_block((size_t)n + 1, 0), region_off((size_t)n + 1, 0);
    std::vector<Frame> frs((size_t)n);
    std::vector<unsigned char> blob;
    std::unique_ptr<unsigned char[]> rgb(new unsigned char[rgb_bytes ? rgb_bytes : 1]);
    memset(rgb.get(), 0xA5, (size_t)rgb_bytes);

    // the walk, once per frame; then the sizes, the table and the records (rk_jpeg_coef_sizes_as / rk_jpeg_coef_pack_as)
    for (int i = 0; i < n; ++i) {
        Frame& fr = frs[i];
        fr.f = frames[i];
        code[i] = rkjpeg::check_record(fr.f, stream_bytes, rgb_bytes, nq, nh, 0, 0);
        first_block[i + 1] = first_block[i];
        region_off[i + 1] = region_off[i];
        if (code[i] != RK_JPEG_OK) continue;
        rkjpeg::geometry(fr.f, fr.g);
        first_block[i + 1] += fr.g.nblocks;
        fr.coefs.assign((size_t)fr.g.nblocks * 64, 0);
        rk_jpeg_huff tabs[6];
        copy_tables(fr.f, fr.g.ncomp, htabs.get(), tabs);
        {
            PtrSrc src{streams.get() + fr.f.stream_off};
            BlockSink sink{fr.coefs.data(), {0}};
            code[i] = rkjpeg::decode_scan(fr.f, fr.g, src, tabs, sink);
        }
        if (code[i] != RK_JPEG_OK) {
            fr.coefs.assign(fr.coefs.size(), 0);
            continue;
        }
        long long len = rkjpeg::dense_table_bytes(fr.g);
        std::vector<long long> at((size_t)fr.g.nblocks);
        for (long long b = 0; b < fr.g.nblocks; ++b) {
            const rkjpeg::DenseShape s = rkjpeg::dense_shape_of(fr.coefs.data() + b * 64);
            at[(size_t)b] = len;
            len += rkjpeg::dense_record_bytes(s);
            ++kinds[5 * i + (s.raw ? 4 : s.n == 0 ? 0 : s.e == 0 ? 1 : s.wide ? 3 : 2)];
        }
        std::unique_ptr<unsigned char[]> region(new unsigned char[(size_t)len]);      // exactly the measured bytes
        memset(region.get(), 0xEE, (size_t)len);
        BytesDst dst{region.get()};
        const long long rel0 = 4 * rkjpeg::dense_groups(fr.g);
        for (long long b = 0; b < fr.g.nblocks; ++b) {
            const long long base = at[(size_t)(b - b % rkjpeg::kDenseGroup)];
            if (b % rkjpeg::kDenseGroup == 0) put_base(region.get(), b / rkjpeg::kDenseGroup, base);
            dst.put16(rel0 + 2 * b, (unsigned)(at[(size_t)b] - base));
            rkjpeg::dense_pack_block(fr.coefs.data() + b * 64, rkjpeg::dense_shape_of(fr.coefs.data() + b * 64), dst, at[(size_t)b]);
        }
        blob.insert(blob.end(), region.get(), region.get() + len);
        region_off[i + 1] += len;
    }

    // every block back out of the blob; the RGB from the packed form
    for (int i = 0; i < n; ++i) {
        const Frame& fr = frs[i];
        if (!rkjpeg::rgb_range_ok(fr.f, rgb_bytes)) continue;
        unsigned char* out = rgb.get() + fr.f.rgb_off;
        if (code[i] != RK_JPEG_OK) {
            memset(out, 0, 3 * (size_t)fr.f.width * fr.f.height);
            continue;
        }
        const long long lo = region_off[i], len = region_off[i + 1] - lo;
        std::unique_ptr<unsigned char[]> region(new unsigned char[(size_t)len]);
        memcpy(region.get(), blob.data() + lo, (size_t)len);
        BytesSrc src{region.get()};
        bool same = rkjpeg::dense_region_ok(lo, lo + len, (long long)blob.size(), fr.g);
        for (long long b = 0; same && b < fr.g.nblocks; ++b) {
            short coef[64];
            same = load_block(src, len, fr.g, b, coef) && memcmp(coef, fr.coefs.data() + b * 64, sizeof coef) == 0;
        }
        exact[i] = same;
        if (decode_packed(fr, blob.data(), (long long)blob.size(), lo, lo + len, qtabs.get(), out) != RK_JPEG_OK) return 3;
    }

    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    fwrite(code.data(), sizeof(int), code.size(), fh);
    fwrite(exact.data(), sizeof(int), exact.size(), fh);
    fwrite(kinds.data(), sizeof(int), kinds.size(), fh);
    fwrite(first_block.data(), sizeof(long long), first_block.size(), fh);
    fwrite(region_off.data(), sizeof(long long), region_off.size(), fh);
    for (int i = 0; i < n; ++i) fwrite(frs[i].coefs.data(), sizeof(short), frs[i].coefs.size(), fh);
    fwrite(blob.data(), 1, blob.size(), fh);
    fwrite(rgb.get(), 1, (size_t)rgb_bytes, fh);

    for (int t = 0; t < ntamper; ++t) {
        const int i = tampers[3 * t], kind = tampers[3 * t + 1], b = tampers[3 * t + 2];
        if (i < 0 || i >= n || code[i] != RK_JPEG_OK) return 2;
        const Frame& fr = frs[i];
        if (b < 0 || b >= fr.g.nblocks) return 2;
        const long long len = region_off[i + 1] - region_off[i];
        long long bytes = len, lo = 0, hi = len;
        std::vector<unsigned char> copy(blob.begin() + region_off[i], blob.begin() + region_off[i + 1]);
        BytesSrc src{copy.data()};
        BytesDst dst{copy.data()};
        const long long grp = b / rkjpeg::kDenseGroup, rel_at = 4 * rkjpeg::dense_groups(fr.g) + 2LL * b;
        const long long base = get_base(copy.data(), grp), rel = src.u16(rel_at), at = base + rel;
        const int tag = copy[(size_t)at], last = tag & 63, cls = tag >> 6, mb = (last + 7) >> 3;
        unsigned long long mask = 0;                    // bit j: zigzag position j + 1
        if (cls < 2)
            for (int j = 0; j < mb; ++j) mask |= (unsigned long long)copy[(size_t)(at + 3 + j)] << (8 * j);
        const int count = __builtin_popcountll(mask);
        const long long nib_at = at + 3 + mb;
        auto nibble = [&](int c) { return (copy[(size_t)(nib_at + c / 2)] >> (4 * (c & 1))) & 15; };
        auto set_nibble = [&](int c, int v) {
            unsigned char& byte = copy[(size_t)(nib_at + c / 2)];
            byte = (unsigned char)((byte & ~(15 << (4 * (c & 1)))) | (v << (4 * (c & 1))));
        };
        if (kind >= 7 && cls >= 2) return 2;
        switch (kind) {
            case 0: dst.put16(rel_at, (unsigned)(rel + 2)); break;
            case 1: dst.put16(rel_at, (unsigned)(rel - 2) & 0xFFFFu); break;
            case 2: put_base(copy.data(), grp, base + 2); break;
            case 3: put_base(copy.data(), grp, base - 2); break;
            case 4: put_base(copy.data(), grp, len + 8); break;
            case 5: lo = len + 2; hi = 2 * len + 2; break;
            case 6: bytes = hi = len - 2; break;
            case 7:
                if (last < 1 || last >= 63) return 2;
                copy[(size_t)at] = (unsigned char)((cls << 6) | (last + 1));
                break;
            case 8:
                if (last < 2) return 2;
                copy[(size_t)at] = (unsigned char)((cls << 6) | (last - 1));
                break;
            case 9: {
                int j = 0;
                while (j < last - 1 && ((mask >> j) & 1)) ++j;
                if (j >= last - 1) return 2;
                copy[(size_t)(at + 3 + j / 8)] |= (unsigned char)(1 << (j & 7));
                break;
            }
            case 10: copy[(size_t)at] = (unsigned char)(tag ^ 0x40); break;
            case 11: copy[(size_t)at] = (unsigned char)(tag | 0xC0); break;
            case 12:
            case 13: {
                int c = 0;
                while (c < count && (nibble(c) == 8) != (kind == 13)) ++c;
                if (c >= count) return 2;
                set_nibble(c, kind == 12 ? 8 : 1);
                break;
            }
            case 14: copy[(size_t)at] = 0x80; break;
            default: return 2;
        }
        std::unique_ptr<unsigned char[]> tampered(new unsigned char[(size_t)bytes]);       // exactly the claimed blob
        memcpy(tampered.get(), copy.data(), (size_t)bytes);
        const size_t out_bytes = 3 * (size_t)fr.f.width * fr.f.height;
        std::vector<unsigned char> again(out_bytes);
        const int rc = decode_packed(fr, tampered.get(), bytes, lo, hi, qtabs.get(), again.data());
        const int same = rc == RK_JPEG_OK && memcmp(again.data(), rgb.get() + fr.f.rgb_off, out_bytes) == 0;
        const long long where[3] = {lo, hi, bytes};
        fwrite(&rc, sizeof(int), 1, fh);
        fwrite(&same, sizeof(int), 1, fh);
        fwrite(where, sizeof(long long), 3, fh);
        fwrite(tampered.get(), 1, (size_t)bytes, fh);
    }
    fclose(fh);
    return 0;
}
