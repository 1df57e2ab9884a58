// What the host programs of the device JPEG decode share (jpeg_core_main.cpp, jpeg_index_main.cpp, jpeg_chunked_main.cpp):
// the byte source and the block sink that stand in for the kernels', exactly-sized reads, the head of an IN file, a
// frame's six tables, and a frame's coefficients taken to RGB.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "rk_jpeg_core.hpp"

struct PtrSrc {
    const unsigned char* p;
    int byte(long long pos) { return p[pos]; }
};

struct BlockSink {
    short* coefs;
    short block[64];
    void put(int k, int v) { block[rkjpeg::natural_of(k)] = (short)v; }
    void end_block(long long b) {
        memcpy(coefs + b * 64, block, sizeof block);
        memset(block, 0, sizeof block);
    }
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

// `prog IN OUT`: IN opened and its head read (int32 head [4], int64 sizes [4]), or nullptr.
inline FILE* open_in(int argc, char** argv, int* head, long long* sizes) {
    FILE* fh = argc == 3 ? fopen(argv[1], "rb") : nullptr;
    if (fh && (fread(head, 4 * sizeof(int), 1, fh) != 1 || fread(sizes, 4 * sizeof(long long), 1, fh) != 1)) {
        fclose(fh);
        fh = nullptr;
    }
    return fh;
}

// The frame's six tables as the kernels stage them: DC of component c at [c], AC at [3 + c].
inline void copy_tables(const rk_jpeg_frame& f, int ncomp, const rk_jpeg_huff* htabs, rk_jpeg_huff* tabs) {
    for (int c = 0; c < 3; ++c) {
        tabs[c] = htabs[f.dc[c < ncomp ? c : 0]];
        tabs[3 + c] = htabs[f.ac[c < ncomp ? c : 0]];
    }
}

// k_jpeg_idct and k_jpeg_colour for one frame: `base` is its region of the workspace with the coefficients in place.
inline void region_to_rgb(const rk_jpeg_frame& f, const rkjpeg::Geometry& g, const unsigned short* qtabs, unsigned char* base,
                          unsigned char* out) {
    for (long long b = 0; b < g.nblocks; ++b) {
        int comp, stride;
        long long off;
        rkjpeg::block_place(g, b, &comp, &off, &stride);
        rkjpeg::idct_islow(reinterpret_cast<const short*>(base) + b * 64, qtabs + (long long)f.quant[comp] * 64,
                           base + g.plane_off[comp] + off, stride);
    }
    const int npix = f.width * f.height;
    for (int p = 0; p < npix; ++p) rkjpeg::pixel_rgb(base, g, p % f.width, p / f.width, out + 3LL * p);
}
