"""The index arithmetic of the per-CU fp32 1x1 GEMM (rk_pw3.hip: k_pw3_gemm, pw3::gemm) restated in numpy and checked
without a device, for every column-range geometry the planner (rk_pw.hip: pw3::plan, through rk_debug_pw_gemm_plan) can hand it:

  * every global address formed -- the A and X LDS-DMA sources with their clamps over all stages, the unconditional loads
    of R / bx (yo[cb] + mo, rows past M clamped to row 0), bpack, ka / kb, the Y stores and the statistics / bred records --
    lies inside its tensor, and every LDS byte read lies inside the stage it is read from;
  * what a lane reads from LDS for an output it stores is the A element (row, k) and the X element (frame, k, pixel) of that
    output: the DMA layout, the clamped copies and the fragment offsets agree;
  * every column of [0, F P) x every row < M is stored by exactly one lane, nothing else is stored, and a 16-byte store is
    4 columns of one frame at a 16-byte aligned address;
  * tile 2 blockIdx + cs counts exactly its columns (n = wcols, first column = the pivot lane's), per row the n sum to F P,
    every tile index is < 2 nwg, and 2 nwg is what the plan and rk_pw_gemm_tiles promise.

Swept: the two RubiksNet-Large layers the kernel serves (288 -> 288 on 14 x 14, 144 -> 288 on 28 x 28; rubiksnet/backbone.py
:139-171) at every frame count up to 1024 the planner takes, both operand layouts, at 256 CUs; and the geometry classes
tests/test_pw3_gpu.py runs on the device (which imports the search and the classes from here)."""
import ctypes
import os

import numpy as np
import pytest

from rubiksnet_amd import _native

# k_pw3_gemm<RB, NRG, CB, ...> as pw3::launch instantiates it, and pw3::gemm's Dims
RB, NRG, CB = 3, 6, 7
NW = 2 * NRG                                   # waves
KNS, KKC = 4, 16                               # ring stages, reduction indices per stage
MR = 16 * RB * NRG                             # rows of the A stage
ABYTES = MR * KKC * 4
NPA = ABYTES // 1024
NPW = 4                                        # DMA pieces per wave and stage, at most
SPLIT = 112
MAX_LDS = 160 * 1024
CUS = 256


def plan(F, K, M, P, a_is_mk=1, epi=0, res=0, pro=0, modes=(1, 1, 1), cus=CUS):
    """(rc, gen, cw, nwg, tiles) of one aligned call"""
    out = (ctypes.c_int * 5)()
    rc = _native.lib().rk_debug_pw_gemm_plan(F, K, M, P, a_is_mk, 1, epi, res, pro, 0, *modes, cus, out)
    return rc, out[0], out[1], out[2], out[4]


def search(P, K, M, want, cus=CUS, modes=(1, 1, 1), f_max=4096):
    """the first F, counting up, that the planner gives to rk_pw3.hip with want(F, cw, nwg, last); last = columns of the last
    workgroup"""
    for F in range(1, f_max + 1):
        rc, gen, cw, nwg, _ = plan(F, K, M, P, modes=modes, cus=cus)
        if rc == 0 and gen == 3:
            last = F * P - (nwg - 1) * cw
            if want(F, cw, nwg, last):
                return F, cw, nwg, last
    return None


# name -> (P, K, M, property of (F, cw, nwg, last) given the CU count); K = M = 288 on 14 x 14 planes unless stated
def classes(cus=CUS):
    def r1(prop, P):                                                  # ... within one launch round
        return lambda F, cw, nwg, last: F * P <= 224 * cus and prop(F, cw, nwg, last)
    straddle = lambda P: r1(lambda F, cw, nwg, last: cw % P != 0 and 113 <= last <= cw - 1, P)
    sliver = lambda P: r1(lambda F, cw, nwg, last: last <= 16, P)
    widest = lambda P: r1(lambda F, cw, nwg, last: cw == 224 and last == cw, P)
    # some range touches 3 frames or more: one that starts on a frame's last 4 pixels does, if any does
    spans3 = lambda P: r1(lambda F, cw, nwg, last: P % 16 != 0 and cw - 4 > P
                          and any((wg * cw) % P + cw > 2 * P for wg in range(nwg - 1)), P)
    out = {
        "control": (196, 288, 288, r1(lambda F, cw, nwg, last: cw == 196, 196)),
        "straddle": (196, 288, 288, straddle(196)),
        "empty-half": (196, 288, 288, r1(lambda F, cw, nwg, last: last <= 112, 196)),
        "sliver": (196, 288, 288, sliver(196)),
        "sliver-28x28": (784, 144, 288, sliver(784)),
        "widest": (196, 288, 288, widest(196)),
        "widest-28x28": (784, 144, 288, widest(784)),
        "short-planes-100": (100, 288, 288, spans3(100)),
        "short-planes-36": (36, 288, 288, spans3(36)),
        "two-rounds": (196, 288, 288, lambda F, cw, nwg, last: nwg > cus and cw % 196 != 0),
    }
    for M in (272, 260):
        out["rows-%d" % M] = (196, 288, M, straddle(196))
    for K in (16, 32, 48, 64, 1024):
        out["depth-%d" % K] = (196, K, 288, straddle(196))
    return out


class Model:
    """k_pw3_gemm's indices for one launch.  Arrays carry a workgroup axis first, over the workgroups `wgs`: all of them
    (full), or the first workgroup of every (c0 mod P, ncols) and the last two of the launch -- a workgroup's (frame, pixel)
    pattern and its column masks depend on these two alone, and every address grows with the column, so the last
    workgroups form the largest."""

    def __init__(self, F, K, M, P, cw, nwg, a_is_mk, full=True):
        self.F, self.K, self.M, self.P, self.cw, self.nwg, self.a_is_mk = F, K, M, P, cw, nwg, a_is_mk
        self.split = SPLIT
        self.ntot = F * P
        self.G = (cw // 4) | 1
        self.xrow = 16 * self.G
        self.XBYTES = KKC * self.xrow
        self.NPX = (self.XBYTES + 1023) // 1024
        self.stage_bytes = ABYTES + self.NPX * 1024
        self.ns = K // KKC
        wg = np.arange(nwg, dtype=np.int64)
        if not full:
            ph = (wg * cw) % P
            ph[-1] = -1                                                # the last workgroup: a class of its own
            wg = np.union1d(np.unique(ph, return_index=True)[1], [max(nwg - 2, 0), nwg - 1])
        self.wgs = wg
        self.c0 = wg * cw                                              # blockIdx.x * d.Cw
        self.cend = np.minimum(self.c0 + cw, self.ntot)
        self.ncols = self.cend - self.c0

    # ---- launch ----
    def check_launch(self):
        assert self.P % 4 == 0 and self.K % KKC == 0 and self.M % 4 == 0 and 0 < self.M <= MR and self.ns >= 1
        assert self.cw % 4 == 0 and 4 * self.G >= self.cw and self.split % 16 == 0
        assert NPA + self.NPX <= NPW * NW                              # every piece has a wave: pi = wave + NW t, t < NPW
        # the ranges [wg cw, min((wg + 1) cw, ntot)) tile [0, ntot) and none is empty
        assert (self.nwg - 1) * self.cw + 4 <= self.ntot <= self.nwg * self.cw and self.ntot % 4 == 0
        assert KNS * self.stage_bytes + 2 * self.K * 4 <= MAX_LDS      # with the prologue's ka / kb behind the ring
        assert (self.ns - 1) * KKC + 4 * 3 + 4 <= self.K               # ... read 16 bytes at stage 16 st + 4 kq of ka[K], kb[K]

    # ---- A: DMA sources of stage 0 per 16-byte unit, floats to advance per stage, the LDS image ----
    def a_dma(self):
        K, M = self.K, self.M
        pi, lane = np.divmod(np.arange(NPA * 64), 64)
        q = pi * 64 + lane
        if self.a_is_mk:
            row = np.minimum(q >> 2, M - 1)
            src, step = row * K + 4 * (q & 3), KKC
        else:
            k = q // (MR // 4)
            m4 = 4 * (q - k * (MR // 4))
            m4 = np.where(m4 + 4 <= M, m4, M - 4)
            src, step = k * M + m4, KKC * M
        dst = pi * 1024 + lane * 16
        return src, step, dst

    def check_a(self):
        K, M = self.K, self.M
        src, step, dst = self.a_dma()
        assert src.min() >= 0 and src.max() + (self.ns - 1) * step + 4 <= M * K
        assert (src % 4 == 0).all()                                    # 16-byte loads of an aligned A
        assert sorted(dst) == list(range(0, ABYTES, 16))
        img = np.full(ABYTES // 4, -1, dtype=np.int64)                 # LDS float -> global float of stage 0
        for e in range(4):
            img[dst // 4 + e] = src + e
        rg, rb, j, kq, s = np.meshgrid(np.arange(NRG), np.arange(RB), np.arange(16), np.arange(4), np.arange(4), indexing="ij")
        mrow0 = 16 * RB * rg
        if self.a_is_mk:                                               # one 16-byte read: element s of it
            byte = (mrow0 + j) * 64 + kq * 16 + rb * (16 * 64) + 4 * s
            assert (((mrow0 + j) * 64 + kq * 16 + rb * 1024) % 16 == 0).all()
        else:
            byte = (4 * kq) * (MR * 4) + (mrow0 + j) * 4 + s * (MR * 4) + rb * 64
        assert byte.min() >= 0 and byte.max() + 4 <= ABYTES
        row, k = mrow0 + 16 * rb + j, 4 * kq + s                       # MFMA 16x16x4: lane (j, kq) feeds A[row j][k kq] of step s
        want = row * K + k if self.a_is_mk else k * M + row
        ok = row < M
        assert (img[byte // 4][ok] == want[ok]).all()
        assert (img[byte // 4] >= 0).all()                             # rows past M: a copy, never uninitialised LDS

    # ---- X ----
    def check_x_layout(self):
        """unit q of the X stage (LDS byte 16 q) holds group g of row k; a lane reads row 4 kq + s at its columns"""
        G = self.G
        q = np.arange(self.NPX * 64)
        k = q // G
        g = q - k * G
        inside = k < KKC
        assert (16 * q[inside] == k[inside] * self.xrow + 16 * g[inside]).all() and inside.sum() == KKC * G
        assert (g < G).all()                                           # units past the stage: row 15 again, a group of the row
        j, kq, s = np.meshgrid(np.arange(16), np.arange(4), np.arange(4), indexing="ij")
        for cs in (0, 1):
            col_lo = 0 if cs == 0 else self.split
            x_off = (4 * kq) * self.xrow + (col_lo + 4 * j) * 4 + s * self.xrow
            x_off2 = (4 * kq) * self.xrow + (col_lo + 64 + (CB - 4) * j) * 4 + s * self.xrow
            assert (x_off % 16 == 0).all() and x_off.min() >= 0
            assert x_off.max() + 16 <= self.NPX * 1024 and x_off2.max() + (CB - 4) * 4 <= self.NPX * 1024   # DMA-written, any lane
            # a valid column, col_lo + rel < ncols <= cw <= 4 G (check_launch), lies in the lane's row: byte = row xrow + 4 column

    def check_x(self):
        F, K, P, G = self.F, self.K, self.P, self.G
        c0, cend = self.c0[:, None], self.cend[:, None]
        c = c0 + 4 * np.arange(G, dtype=np.int64)[None, :]
        c = np.where(c + 4 <= cend, c, cend - 4)                       # groups past the range: a copy
        f = c // P
        p = c - f * P
        base = f * K * P + p                                           # row k of the stage: + k P, stage st: + 16 st P
        assert base.min() >= 0 and base.max() + (KKC - 1) * P + (self.ns - 1) * KKC * P + 4 <= F * K * P
        assert (p + 4 <= P).all() and (base % 4 == 0).all()            # 4 pixels of one (frame, k) row, 16-byte aligned
        x = np.arange(self.cw, dtype=np.int64)[None, :]                # column of the range; LDS row k holds it at 4 x
        col = c0 + x
        fx = col // P
        want = fx * K * P + (col - fx * P)
        got = base[:, x[0] // 4] + x % 4
        on = x < self.ncols[:, None]
        assert (got[on] == want[on]).all()

    # ---- output ----
    def wcols(self, cs):
        w = np.full(len(self.c0), self.split, dtype=np.int64) if cs == 0 else self.ncols - self.split
        return np.clip(w, 0, self.ncols)

    def rows(self):
        rg, rb, kq, r = np.meshgrid(np.arange(NRG), np.arange(RB), np.arange(4), np.arange(4), indexing="ij")
        return (16 * RB * rg + 16 * rb + 4 * kq + r).ravel()

    def check_rows(self):
        M = self.M
        m = self.rows()
        assert sorted(m[m < M]) == list(range(M))                      # every row < M has exactly one (wave row group, rb, kq, r)
        mc = np.where(m < M, m, 0)
        assert mc.min() >= 0 and mc.max() < M                          # bpack[mc], mo = mc P

    def check_output(self, tiles):
        F, M, P, ntot, nwg, cw = self.F, self.M, self.P, self.ntot, self.nwg, self.cw
        J = 2 * nwg
        assert tiles == J
        mo_max = (M - 1) * P
        size = F * M * P
        nsel = len(self.c0)
        j, cb = np.meshgrid(np.arange(16), np.arange(CB), indexing="ij")
        rel = np.where(cb < 4, 4 * j + cb, 64 + (CB - 4) * j + (cb - 4))[None]
        wg_i = np.arange(nsel)[:, None, None]
        stored, counted = [], []       # (workgroup, column of its range) of the Y stores / of the epilogue sums, flattened
        nsum = np.zeros(nsel, dtype=np.int64)
        for cs in (0, 1):
            col_lo = 0 if cs == 0 else self.split
            wc = self.wcols(cs)
            con = rel < wc[:, None, None]
            c = self.c0[:, None, None] + col_lo + np.where(con, rel, 0)
            cc = np.where(c < ntot, c, 0)
            f = cc // P
            p = cc - f * P
            yo = f * M * P + p
            # unconditional loads of R / bx at yo + mo: 16 bytes for cb 0, 4 for cb >= 4 (cb 1..3 form no address)
            assert yo.min() >= 0 and (yo[:, :, 0] % 4 == 0).all() and (p[:, :, 0] + 4 <= P).all()
            assert yo[:, :, 0].max() + mo_max + 4 <= size and yo[:, :, 4:].max() + mo_max + 1 <= size
            # stores: o[0..3] as 16 bytes when con[0], o[cb >= 4] as 4 bytes when con[cb]
            assert (c[con] < ntot).all()
            assert (con[:, :, 0] == con[:, :, 1]).all() and (con[:, :, 0] == con[:, :, 2]).all() and (con[:, :, 0] == con[:, :, 3]).all()
            c4 = c[:, :, 0][con[:, :, 0]]
            f4 = c4 // P
            assert ((c4 - f4 * P) + 4 <= P).all() and ((f4 * M * P + (c4 - f4 * P)) % 4 == 0).all() and (M * P) % 4 == 0
            x = c - self.c0[:, None, None]                             # column inside the range
            assert x.min() >= 0 and x[con].max(initial=0) < cw + 4
            flat = wg_i * (cw + 8) + x
            stored += [flat[:, :, 0][con[:, :, 0]] + e for e in range(4)] + [flat[:, :, 4:][con[:, :, 4:]]]
            counted.append(flat[con])
            # the tile of (workgroup, cs): n = wcols columns from c0 + col_lo on, the pivot lane (j = 0, cb = 0) on the first
            assert (con.sum(axis=(1, 2)) == wc).all()
            first = self.c0 + col_lo
            has = wc > 0
            lo = np.where(con, c, ntot + 8).min(axis=(1, 2))
            hi = np.where(con, c, -1).max(axis=(1, 2))
            assert (lo[has] == first[has]).all() and (hi[has] == (first + wc - 1)[has]).all()
            assert (c[:, 0, 0][has] == first[has]).all()
            tile = 2 * self.wgs + cs
            assert tile.max() < J and (M - 1) * J + tile.max() < M * J
            nsum += wc
        # every column of the workgroup's range [c0, c0 + ncols) once, nothing else; the ranges tile [0, ntot) (check_launch)
        want = (np.arange(cw + 8)[None, :] < self.ncols[:, None]).astype(np.int64)
        for cols in (stored, counted):
            assert (np.bincount(np.concatenate(cols), minlength=want.size).reshape(want.shape) == want).all()
        assert (nsum == self.ncols).all()                              # per row, the n of a workgroup's two tiles; sum: ntot

    def check(self, tiles):
        self.check_launch()
        self.check_a()
        self.check_x_layout()
        self.check_x()
        self.check_rows()
        self.check_output(tiles)


def check_geometry(F, K, M, P, cus=CUS, full=True):
    """both operand layouts of one planned shape, with the epilogue that promises tiles"""
    for a_is_mk, epi, pro in ((1, 1, 1), (0, 2, 0)):
        rc, gen, cw, nwg, tiles = plan(F, K, M, P, a_is_mk=a_is_mk, epi=epi, res=1, pro=pro, cus=cus)
        assert (rc, gen) == (0, 3), (F, K, M, P, a_is_mk)
        m = Model(F, K, M, P, cw, nwg, a_is_mk, full=full)
        if a_is_mk:
            m.check(tiles)
        else:                                                          # X, rows and the output do not depend on A's layout
            assert tiles == 2 * nwg
            m.check_launch()
            m.check_a()
    return cw, nwg


LAYERS = [(288, 288, 196), (144, 288, 784)]


@pytest.mark.parametrize("K,M,P", LAYERS)
def test_every_planned_frame_count_of_the_large_layers(K, M, P):
    seen = set()
    n = 0
    for F in range(1, 1025):
        rc, gen, cw, nwg, _ = plan(F, K, M, P)
        if rc == 0 and gen == 3:
            check_geometry(F, K, M, P, full=False)
            seen.add(cw)
            n += 1
    assert seen == set(range(196, 225, 4)) and n >= 60, (sorted(seen), n)   # every range width the planner can choose
    print("%d frame counts, widths %s" % (n, sorted(seen)))


@pytest.mark.parametrize("name", sorted(classes()))
def test_geometry_class(name):
    P, K, M, want = classes()[name]
    found = search(P, K, M, want)
    assert found, name
    F, cw, nwg, last = found
    assert check_geometry(F, K, M, P) == (cw, nwg)
    print("%s: F %d cw %d nwg %d last %d" % (name, F, cw, nwg, last))


def test_tiles_of_264_frames_and_the_promise():
    """2 nwg records per row: the plan's `tiles` and rk_pw_gemm_tiles agree (264 frames of 288 -> 288 on 14 x 14: 508), on
    this process's switches and the CU count the library sees."""
    rc, gen, cw, nwg, tiles = plan(264, 288, 288, 196, epi=1)
    assert (rc, gen, cw, nwg, tiles) == (0, 3, 204, 254, 508)
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else CUS
    modes = tuple(int(os.environ.get(k, "1") or 0) for k in ("RK_PW2", "RK_PW3", "RK_PW4"))
    L = _native.lib()
    for K, M, P in LAYERS:
        for F in range(1, 1025):
            for a_is_mk, epi in ((1, 1), (0, 2)):
                rc, gen, cw, nwg, tiles = plan(F, K, M, P, a_is_mk=a_is_mk, epi=epi, modes=modes, cus=cus)
                if rc == 0:
                    assert tiles == L.rk_pw_gemm_tiles(ctypes.c_void_p(4096), F, K, M, P, a_is_mk), (F, K, M, P, a_is_mk)
                    assert gen != 3 or tiles == 2 * nwg
