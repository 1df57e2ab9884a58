// Host run of the device JPEG decode core (rubiksnet_amd/csrc/rk_jpeg_core.hpp): the stages of rk_jpeg_decode_u8 in the
// kernels' order, one frame after another, on exactly-sized heap buffers.  tests/test_jpeg.py builds this with
// -fsanitize=address,undefined and runs it over the goldens and the corrupted corpus: the bounds proof for the kernels'
// logic.
//
//   jpeg_core_main IN OUT
//   IN : int32 n, nq, nh, 0; int64 stream_bytes, rgb_bytes, workspace_bytes, 0; frames [n * 64]; htabs [nh * 1424];
//        qtabs [nq * 128]; streams [stream_bytes]
//   OUT: int32 status [n + 1]; rgb [rgb_bytes] (bytes no frame owns keep 0xA5)
#include "jpeg_host.hpp"

int main(int argc, char** argv) {
    int head[4];
    long long sizes[4];
    FILE* fh = open_in(argc, argv, head, sizes);
    if (!fh) return 2;
    const int n = head[0], nq = head[1], nh = head[2];
    const long long stream_bytes = sizes[0], rgb_bytes = sizes[1], workspace_bytes = sizes[2];
    if (n < 1 || nq < 1 || nh < 1 || stream_bytes < 0 || rgb_bytes < 0 || workspace_bytes < rkjpeg::offset_table_bytes(n)) return 2;
    auto frames = read_exact<rk_jpeg_frame>(fh, (size_t)n);
    auto htabs = read_exact<rk_jpeg_huff>(fh, (size_t)nh);
    auto qtabs = read_exact<unsigned short>(fh, (size_t)nq * 64);
    auto streams = read_exact<unsigned char>(fh, (size_t)stream_bytes);
    fclose(fh);

    std::vector<int> status((size_t)n + 1, 0);
    std::unique_ptr<unsigned char[]> rgb(new unsigned char[rgb_bytes ? rgb_bytes : 1]);
    memset(rgb.get(), 0xA5, (size_t)rgb_bytes);
    std::unique_ptr<unsigned char[]> ws(new unsigned char[workspace_bytes]);
    memset(ws.get(), 0x5A, (size_t)workspace_bytes);
    long long* offsets = reinterpret_cast<long long*>(ws.get());

    // k_jpeg_plan
    long long at = rkjpeg::offset_table_bytes(n);
    for (int i = 0; i < n; ++i) {
        offsets[i] = at;
        at += rkjpeg::frame_workspace_bytes(frames[i]);
        status[i] = rkjpeg::check_record(frames[i], stream_bytes, rgb_bytes, nq, nh, at, workspace_bytes);
    }
    offsets[n] = at;
    for (int i = 0; i < n; ++i) {
        const rk_jpeg_frame& f = frames[i];
        rkjpeg::Geometry g;
        unsigned char* base = ws.get() + offsets[i];
        if (status[i] == RK_JPEG_OK) {      // k_jpeg_entropy
            rkjpeg::geometry(f, g);
            rk_jpeg_huff tabs[6];
            copy_tables(f, g.ncomp, htabs.get(), tabs);
            PtrSrc src{streams.get() + f.stream_off};
            BlockSink sink{reinterpret_cast<short*>(base), {0}};
            status[i] = rkjpeg::decode_scan(f, g, src, tabs, sink);
        }
        if (rkjpeg::rgb_range_ok(f, rgb_bytes)) {       // k_jpeg_idct, k_jpeg_colour; a failed frame is zeroed
            unsigned char* out = rgb.get() + f.rgb_off;
            if (status[i] == RK_JPEG_OK)
                region_to_rgb(f, g, qtabs.get(), base, out);
            else
                memset(out, 0, 3 * (size_t)f.width * f.height);
        }
        status[n] += status[i] != RK_JPEG_OK;          // k_jpeg_count
    }
    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    fwrite(status.data(), sizeof(int), status.size(), fh);
    fwrite(rgb.get(), 1, (size_t)rgb_bytes, fh);
    fclose(fh);
    return 0;
}
