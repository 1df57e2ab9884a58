"""Resident frames as packed DCT coefficients, without a GPU: a host run of the device code (csrc/rk_jpeg_core.hpp through
tests/jpeg_coef_main.cpp, built with AddressSanitizer and UBSan and run as a child process) over the index cases, every
supported fixture, the corrupted corpus, two Pillow-written frames and a table of tampered regions; the format's
arithmetic restated in numpy; and the host side -- the workspace size, the entry points' argument checks,
DeviceFrameCache's argument errors."""
import os

import numpy as np
import pytest
import torch

import _jpeg_cases as jc
import _jpeg_coef_cases as cc
from rubiksnet_amd import dataset, jpeg


@pytest.fixture(scope="module")
def host():
    pytest.importorskip("PIL")
    run = cc.host_run()
    if run is None:
        pytest.skip("no host C++ compiler")
    return run


# ------------------------------------------------------------------------------------------------- host run of the device code
def test_the_set_holds_every_case_and_every_kind_of_block(host):
    assert set(cc.GOOD) >= set(jc.SUPPORTED) | set(cc.ic.CASES) | {cc.NOISE, cc.FLAT} and cc.NAMES[len(cc.GOOD):] == list(jc.CORRUPT)
    n = len(cc.GOOD)
    assert host["code"][:n].tolist() == [0] * n and (host["code"][n:] != 0).all()
    wide, narrow, none = host["kinds"][:n].sum(axis=0).tolist()
    print("blocks with 16-bit ACs, with 8-bit ACs, without ACs:", wide, narrow, none)
    assert wide >= 1 and narrow >= 1 and none >= 1
    assert host["kinds"][cc.NAMES.index(cc.NOISE), 0] >= 1                       # the noise frame brings the wide blocks
    assert host["kinds"][cc.NAMES.index(cc.FLAT)].tolist() == [0, 0, 6]          # one 4:2:0 MCU, no AC anywhere
    assert (host["kinds"].sum(axis=1)[:n] == np.diff(host["first_block"])[:n]).all() and not host["kinds"][n:].any()


def test_every_block_comes_back_out_of_its_record(host):
    n = len(cc.GOOD)
    assert host["exact"][:n].tolist() == [1] * n


def test_the_packed_rgb_equals_the_fixtures_and_pillow(host):
    for i, name in enumerate(cc.GOOD):
        want = cc.want_rgb(name)
        off = int(host["rgb_off"][i])
        got = host["rgb"][off:off + want.size].reshape(want.shape)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        pil = jc.pillow_rgb_where_defined(cc.jpg(name))
        if pil is not None:
            assert np.array_equal(got, pil), name
    for i in range(len(cc.GOOD), len(cc.NAMES)):            # a refused frame: no region, a zero frame
        assert host["region_off"][i + 1] == host["region_off"][i]
        off = int(host["rgb_off"][i])
        assert not host["rgb"][off:off + 17 * 23 * 3].any()


def test_the_sizes_are_the_formats_arithmetic(host):
    """From the walked coefficients, in numpy: n non-zero ACs, w = 2 where one of them leaves int8, 10 + n w rounded up to
    even per record; the table holds their running sum behind its own 4 bytes per block; the records hold the values."""
    zz = jpeg._ZIGZAG
    blob, fb, ro = host["blob"], host["first_block"], host["region_off"]
    for i, name in enumerate(cc.GOOD):
        coefs = host["coefs"][fb[i]:fb[i + 1]][:, zz]      # zigzag order
        nb = len(coefs)
        ac = coefs[:, 1:]
        count = (ac != 0).sum(axis=1)
        width = np.where(((ac < -128) | (ac > 127)).any(axis=1), 2, 1)
        size = 10 + ((count * width + 1) & ~1)
        assert size.min() >= jpeg.COEF_RECORD_MIN and size.max() <= jpeg.COEF_RECORD_MAX
        region = blob[ro[i]:ro[i + 1]]
        table = region[:4 * nb].view("<u4").astype(np.int64)
        want = 4 * nb + np.concatenate([[0], np.cumsum(size)[:-1]])
        assert np.array_equal(table, want), name
        assert len(region) == 4 * nb + int(size.sum()), name
        for b in (0, nb // 2, nb - 1):                      # a few records, field by field
            r = region[table[b]:table[b] + size[b]]
            header = int(r[:8].view("<u8")[0])
            assert header & 1 == (width[b] == 2) and [k for k in range(1, 64) if header >> k & 1] == (np.flatnonzero(ac[b]) + 1).tolist()
            assert int(r[8:10].view("<i2")[0]) == int(coefs[b, 0])
            vals = r[10:10 + count[b] * width[b]].view("<i2" if width[b] == 2 else "i1")
            assert vals.tolist() == ac[b][ac[b] != 0].tolist(), (name, b)
    print("packed bytes per block: %.1f" % (len(blob) / fb[len(cc.GOOD)]))


def test_no_tampered_region_decodes_silently_wrong(host):
    rows = cc.tampers()
    assert {k for _, k, _ in rows} == set(range(len(cc.KINDS))) and len(rows) == len(host["tampered"])
    print({(cc.NAMES[i], cc.KINDS[k], b): jpeg.STATUS_NAMES[code] for (i, k, b), (code, _, _, _, _) in zip(rows, host["tampered"])})
    for (i, k, b), (code, same, lo, hi, blob) in zip(rows, host["tampered"]):
        assert code != 0 or same == 1, (cc.NAMES[i], cc.KINDS[k], b)
        assert code == 8, (cc.NAMES[i], cc.KINDS[k], b)     # the records tile the region: every one of these is noticed


# ------------------------------------------------------------------------------------------------- sizes, arguments
def _lib():
    from rubiksnet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("the HIP library is not built")
    return _native.lib()


def test_coef_workspace_bytes_equal_the_library():
    L = _lib()
    _, res = cc.resident()
    (frames, _, _, _), (n, _, _) = jpeg.sections(res.blob, res.layout)
    rec = np.frombuffer(frames.numpy().tobytes(), dtype=jpeg.FRAME_DTYPE).copy()
    rec["width"][1] = 0                                     # an invalid record takes no planes
    for pick in ([7, 2, 2, 9], [0], [1, 1], [n - 1, -1, n, 4], list(range(n))):
        arr = np.asarray(pick, dtype=np.int32)
        want = L.rk_jpeg_coef_workspace_bytes(rec.ctypes.data, n, arr.ctypes.data, len(pick))
        assert want == jpeg.coef_workspace_bytes_for(rec, pick) > 0, pick
        blocks = int(jpeg._geometry_blocks(rec)[3][[p for p in pick if 0 <= p < n]].sum())
        assert want % 16 == 0 and want == jpeg.indexed_workspace_bytes_for(rec, pick, 1) - 128 * blocks     # planes only
    one = np.zeros(1, dtype=np.int32)
    assert L.rk_jpeg_coef_workspace_bytes(None, n, one.ctypes.data, 1) == 0
    assert L.rk_jpeg_coef_workspace_bytes(rec.ctypes.data, n, None, 1) == 0
    assert L.rk_jpeg_coef_workspace_bytes(rec.ctypes.data, n, one.ctypes.data, 0) == 0
    assert L.rk_jpeg_coef_workspace_bytes(rec.ctypes.data, 0, one.ctypes.data, 1) == 0
    assert jpeg.coef_workspace_bytes_for(rec, []) == 0
    # 64 bytes of samples per block, 16-byte rounded: 17x23 4:2:0 is 2x2 MCUs of 6 blocks
    assert jpeg.frame_plane_bytes(rec[0:1]).tolist() == [24 * 64] and jpeg.frame_plane_bytes(rec[1:2]).tolist() == [0]


def test_the_entry_points_validate_before_anything_is_launched():
    import ctypes
    L, one, odd = _lib(), ctypes.c_void_p(64), ctypes.c_void_p(65)      # non-NULL dummies, never dereferenced on these paths
    big = 1 << 20

    def sizes(streams=one, n=1, nq=1, nh=1, entries=None, entry_off=None, most=1, ws=one, ws_bytes=big, status=one,
              block_off=one, cap=10, first_block=one, region_off=one, stream_bytes=10):
        return L.rk_jpeg_coef_sizes(streams, stream_bytes, one, one, nq, nh, n, entries, 4, entry_off, one, one, most, ws, ws_bytes,
                                    status, block_off, cap, first_block, region_off, None)
    assert sizes(streams=None) == -1 and sizes(status=None) == -1 and sizes(block_off=None) == -1 and sizes(region_off=None) == -1
    assert sizes(entries=one, entry_off=None) == -1         # an index without its tables
    assert sizes(n=0) == -2 and sizes(n=65536) == -2 and sizes(nq=0) == -2 and sizes(nh=65536) == -2 and sizes(most=0) == -2
    assert sizes(cap=-1) == -2 and sizes(stream_bytes=-1) == -2
    assert sizes(first_block=ctypes.c_void_p(68)) == -2 and sizes(block_off=ctypes.c_void_p(66)) == -2 and sizes(status=odd) == -2
    assert sizes(ws=None) == -4 and sizes(ws=ctypes.c_void_p(72)) == -4
    assert sizes(n=2, most=3, ws_bytes=2 * 64 + 32 + 32 - 1) == -4     # the head of 2 frames x 3 segments + their offset table

    def pack(n=1, most=1, ws=one, ws_bytes=big, status=one, blob=one, blob_bytes=100, cap=10, region_off=one):
        return L.rk_jpeg_coef_pack(one, n, most, ws, ws_bytes, status, one, cap, one, region_off, blob, blob_bytes, None)
    assert pack(blob=None) == -1 and pack(status=None) == -1 and pack(region_off=None) == -1
    assert pack(n=0) == -2 and pack(n=65536) == -2 and pack(most=0) == -2 and pack(blob_bytes=-1) == -2 and pack(cap=-1) == -2
    assert pack(blob=odd) == -2 and pack(region_off=ctypes.c_void_p(68)) == -2
    assert pack(ws=None) == -4 and pack(ws=ctypes.c_void_p(72)) == -4 and pack(ws_bytes=64 + 16 + 16 - 1) == -4

    def dec(blob=one, n=3, nq=1, m=1, ws=one, ws_bytes=big, pick=one, region_off=one, status=one, qtabs=one, blob_bytes=100,
            rgb_bytes=100, build_status=one):
        return L.rk_jpeg_decode_coef_u8(blob, blob_bytes, one, qtabs, nq, n, region_off, build_status, pick, one, m, one, rgb_bytes,
                                        ws, ws_bytes, status, None)
    assert dec(blob=None) == -1 and dec(pick=None) == -1 and dec(region_off=None) == -1 and dec(build_status=None) == -1
    assert dec(n=0) == -2 and dec(nq=0) == -2 and dec(nq=65536) == -2 and dec(m=0) == -2 and dec(m=65536) == -2
    assert dec(blob_bytes=-1) == -2 and dec(rgb_bytes=-1) == -2
    assert dec(blob=odd) == -2 and dec(qtabs=odd) == -2 and dec(region_off=ctypes.c_void_p(68)) == -2 and dec(pick=ctypes.c_void_p(66)) == -2
    assert dec(ws=None) == -4 and dec(ws=ctypes.c_void_p(72)) == -4
    assert dec(m=2, ws_bytes=2 * 64 + 16 + 32 - 1) == -4    # records + flags + offset table of 2 frames


def test_build_coef_refuses_what_it_cannot_do():
    _, res = cc.resident()
    with pytest.raises(RuntimeError, match="runs on a GPU"):
        jpeg.build_coef(res, "cpu")
    for kw, match in ((dict(method="rows"), "method must be"), (dict(slab_frames=0), "slab_frames must be"),
                      (dict(method="chunked", chunk_bytes=100), "chunk_bytes must be")):
        with pytest.raises(ValueError, match=match):        # the argument checks come before the device is touched
            jpeg.build_coef(res, "cuda:0", **kw)


def test_the_cache_refuses_sources_that_hold_no_files(tmp_path):
    videos = [(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), 0)]
    with pytest.raises(ValueError, match="resident must be 'rgb' or 'jpeg' or 'coef'"):
        dataset.DeviceFrameCache(videos, 1, "val", num_segments=2, resident="nonsense")
    with pytest.raises(ValueError, match="resident='coef'.*decode='device'.*in-memory"):
        dataset.DeviceFrameCache(videos, 1, "val", num_segments=2, resident="coef")
    mem = dataset.InMemoryVideos([v for v, _ in videos], [0], num_segments=2, random_shift=False)
    with pytest.raises(ValueError, match="resident='coef'.*decode='device'.*in-memory"):
        dataset.DeviceFrameCache(mem, 1, "val", resident="coef")
    os.makedirs(tmp_path / "a")
    for k in range(1, 5):
        with open(tmp_path / "a" / ("img_%05d.jpg" % k), "wb") as fh:
            fh.write(jc.jpg("p17x23_420"))
    with open(tmp_path / "list.txt", "w") as fh:
        fh.write("a 4 3\n")
    host = dataset.RubiksDataset(str(tmp_path), str(tmp_path / "list.txt"), num_segments=2, random_shift=False,
                                 only_even_indices=False, decode="host")
    with pytest.raises(ValueError, match="resident='coef'.*decode='device'.*decode='host' dataset"):
        dataset.DeviceFrameCache(host, 1, "val", resident="coef")
    with pytest.raises(ValueError, match="index_build='chunked'.*resident='jpeg' or 'coef'"):
        dataset.DeviceFrameCache(videos, 1, "val", num_segments=2, index_build="chunked")
