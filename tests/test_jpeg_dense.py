"""The dense record format of the packed DCT coefficients, without a GPU: a host run of the device code
(csrc/rk_jpeg_core.hpp through tests/jpeg_dense_main.cpp, built with AddressSanitizer and UBSan and run as a child process)
over the set of tests/_jpeg_dense_cases.py and a table of tampered regions; a packer written in numpy from the format's
description (tests/_jpeg_dense_ref.py) against the host program's blob byte for byte; the sizes against the wide
format's; and the host side -- the entry points' argument checks, build_coef's and DeviceFrameCache's argument errors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _jpeg_cases as jc
import _jpeg_dense_cases as dc
import _jpeg_dense_ref as ref
from rubiksnet_amd import dataset, jpeg


@pytest.fixture(scope="module")
def host():
    pytest.importorskip("PIL")
    run = dc.host_run()
    if run is None:
        pytest.skip("no host C++ compiler")
    return run


def _coefs(run, i):
    return run["coefs"][run["first_block"][i]:run["first_block"][i + 1]]


def _region(run, i):
    return run["blob"][run["region_off"][i]:run["region_off"][i + 1]]


# ------------------------------------------------------------------------------------------------- host run of the device code
def test_the_set_holds_every_case_and_every_kind_of_block(host):
    assert dc.GOOD[:len(dc.cc.GOOD)] == list(dc.cc.GOOD) and dc.NAMES[len(dc.GOOD):] == list(jc.CORRUPT)
    n = len(dc.GOOD)
    assert host["code"][:n].tolist() == [0] * n and (host["code"][n:] != 0).all()
    kinds = host["kinds"]
    print(dict(zip(dc.BLOCK_KINDS, kinds[:n].sum(axis=0).tolist())))
    assert (kinds[:n].sum(axis=0) >= 1).all()
    assert (kinds.sum(axis=1)[:n] == np.diff(host["first_block"])[:n]).all() and not kinds[n:].any()
    row = dict(zip(dc.NAMES, kinds.tolist()))
    assert row[dc.STEP][3] == 2 and row[dc.STEP][4] == 0                # two blocks with int16 escapes, none raw
    assert sum(row[dc.WAVE]) == 180 and row[dc.WAVE][2] == 179 and row[dc.WAVE][1] == 1
    assert row[dc.cc.NOISE][4] == 4 and row["noise_q10_420"][1] >= 1 and row[dc.cc.FLAT] == [6, 0, 0, 0, 0]


def test_every_block_comes_back_out_of_its_record(host):
    n = len(dc.GOOD)
    assert host["exact"][:n].tolist() == [1] * n


def test_the_packed_rgb_equals_the_fixtures_and_pillow(host):
    for i, name in enumerate(dc.GOOD):
        want = dc.want_rgb(name)
        off = int(host["rgb_off"][i])
        got = host["rgb"][off:off + want.size].reshape(want.shape)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        pil = jc.pillow_rgb_where_defined(dc.jpg(name))
        if pil is not None:
            assert np.array_equal(got, pil), name
    for i in range(len(dc.GOOD), len(dc.NAMES)):            # a refused frame: no region, a zero frame
        assert host["region_off"][i + 1] == host["region_off"][i]
        off = int(host["rgb_off"][i])
        assert not host["rgb"][off:off + 17 * 23 * 3].any()


def test_the_blob_is_the_numpy_packers_byte_for_byte(host):
    """tests/_jpeg_dense_ref.py shares no code with the device's packer: it is the format's description in numpy."""
    total = 0
    for i, name in enumerate(dc.GOOD):
        want, got = ref.region(_coefs(host, i)), _region(host, i)
        assert len(got) == len(want) and np.array_equal(got, want), (name, len(got), len(want))
        nb = len(_coefs(host, i))
        least, most = jpeg.coef_region_bounds("dense", nb)
        assert least <= len(got) <= most and len(got) % 2 == 0
        total += len(got)
    print("dense bytes per block: %.1f" % (total / host["first_block"][len(dc.GOOD)]))


def test_no_good_frames_dense_region_is_longer_than_its_wide_one(host):
    ratios = {}
    for i, name in enumerate(dc.GOOD):
        dense, wide = len(_region(host, i)), ref.wide_bytes(_coefs(host, i))
        ratios[name] = round(dense / wide, 3)
        assert dense <= wide, (name, dense, wide)
    print(ratios)


def test_a_benchmark_frame_packs_to_seven_tenths_of_its_wide_size():
    pytest.importorskip("PIL")
    run = dc.bench_run()
    if run is None:
        pytest.skip("no host C++ compiler")
    assert run["code"].tolist() == [0] and run["exact"].tolist() == [1]
    dense, wide = len(run["blob"]), ref.wide_bytes(run["coefs"])
    print("256 x 340 4:2:0 q90: dense %d, wide %d, %.3f; %.1f bytes a block" % (dense, wide, dense / wide, dense / len(run["coefs"])))
    assert np.array_equal(run["blob"], ref.region(run["coefs"]))
    assert dense <= 0.70 * wide


def test_no_tampered_region_decodes_silently(host):
    rows = host["tampers"].tolist()
    assert {k for _, k, _ in rows} == set(range(len(dc.KINDS))) and len(rows) == len(host["tampered"])
    for name in dc.TAMPERED:                                # every kind on every one of the three frames
        assert {k for i, k, _ in rows if dc.NAMES[i] == name} == set(range(len(dc.KINDS))), name
    wave = dc.NAMES.index(dc.WAVE)
    assert any(i == wave and k in (0, 1) and b >= 64 for i, k, b in rows)       # a rel in the second group
    assert any(i == wave and k in (2, 3) and b >= 64 for i, k, b in rows)       # a base that is not the first
    print({(dc.NAMES[i], dc.KINDS[k], b): jpeg.STATUS_NAMES[code] for (i, k, b), (code, _, _, _, _) in zip(rows, host["tampered"])})
    for (i, k, b), (code, same, lo, hi, blob) in zip(rows, host["tampered"]):
        assert code != 0 or same == 1, (dc.NAMES[i], dc.KINDS[k], b)
        assert code == 8, (dc.NAMES[i], dc.KINDS[k], b)


# ------------------------------------------------------------------------------------------------- sizes, arguments
def _lib():
    from rubiksnet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("the HIP library is not built")
    return _native.lib()


def test_the_region_bounds_equal_the_library():
    L = _lib()
    least, most = ctypes.c_longlong(), ctypes.c_longlong()
    for record, fmt in jpeg.COEF_RECORDS.items():
        for nb in (1, 6, 63, 64, 65, 180, 2112):
            assert L.rk_jpeg_coef_region_bounds(fmt, nb, ctypes.byref(least), ctypes.byref(most)) == 0
            assert (least.value, most.value) == jpeg.coef_region_bounds(record, nb), (record, nb)
    assert jpeg.coef_region_bounds("dense", 65) == (8 + 130 + 65 * 4, 8 + 130 + 65 * 130)
    assert jpeg.coef_region_bounds("wide", 3) == (3 * 14, 3 * 140)
    assert (jpeg.COEF_DENSE_RECORD_MIN, jpeg.COEF_DENSE_RECORD_MAX, jpeg.COEF_DENSE_GROUP) == (4, 130, 64)
    assert L.rk_jpeg_coef_region_bounds(2, 6, ctypes.byref(least), ctypes.byref(most)) == -2
    assert L.rk_jpeg_coef_region_bounds(-1, 6, ctypes.byref(least), ctypes.byref(most)) == -2
    assert L.rk_jpeg_coef_region_bounds(1, 0, ctypes.byref(least), ctypes.byref(most)) == -2
    assert L.rk_jpeg_coef_region_bounds(1, 6, None, ctypes.byref(most)) == -1
    with pytest.raises(ValueError, match="record must be"):
        jpeg.coef_region_bounds("narrow", 6)


@pytest.mark.parametrize("fmt", [0, 1])
def test_the_entry_points_validate_before_anything_is_launched(fmt):
    L, one, odd = _lib(), ctypes.c_void_p(64), ctypes.c_void_p(65)      # non-NULL dummies, never dereferenced on these paths
    big = 1 << 20

    def sizes(streams=one, n=1, nq=1, nh=1, entries=None, entry_off=None, most=1, ws=one, ws_bytes=big, status=one,
              block_off=one, cap=10, first_block=one, region_off=one, stream_bytes=10, fmt=fmt):
        return L.rk_jpeg_coef_sizes_as(streams, stream_bytes, one, one, nq, nh, n, entries, 4, entry_off, one, one, most, ws, ws_bytes,
                                       status, block_off, cap, first_block, region_off, None, fmt)
    assert sizes(streams=None) == -1 and sizes(status=None) == -1 and sizes(block_off=None) == -1 and sizes(region_off=None) == -1
    assert sizes(entries=one, entry_off=None) == -1         # an index without its tables
    assert sizes(n=0) == -2 and sizes(n=65536) == -2 and sizes(nq=0) == -2 and sizes(nh=65536) == -2 and sizes(most=0) == -2
    assert sizes(cap=-1) == -2 and sizes(stream_bytes=-1) == -2
    assert sizes(first_block=ctypes.c_void_p(68)) == -2 and sizes(block_off=ctypes.c_void_p(66)) == -2 and sizes(status=odd) == -2
    assert sizes(fmt=2) == -2 and sizes(fmt=-1) == -2
    assert sizes(ws=None) == -4 and sizes(ws=ctypes.c_void_p(72)) == -4
    assert sizes(n=2, most=3, ws_bytes=2 * 64 + 32 + 32 - 1) == -4     # the head of 2 frames x 3 segments + their offset table

    def pack(n=1, most=1, ws=one, ws_bytes=big, status=one, blob=one, blob_bytes=100, cap=10, region_off=one, fmt=fmt):
        return L.rk_jpeg_coef_pack_as(one, n, most, ws, ws_bytes, status, one, cap, one, region_off, blob, blob_bytes, None, fmt)
    assert pack(blob=None) == -1 and pack(status=None) == -1 and pack(region_off=None) == -1
    assert pack(n=0) == -2 and pack(n=65536) == -2 and pack(most=0) == -2 and pack(blob_bytes=-1) == -2 and pack(cap=-1) == -2
    assert pack(blob=odd) == -2 and pack(region_off=ctypes.c_void_p(68)) == -2
    assert pack(fmt=2) == -2 and pack(fmt=-1) == -2
    assert pack(ws=None) == -4 and pack(ws=ctypes.c_void_p(72)) == -4 and pack(ws_bytes=64 + 16 + 16 - 1) == -4

    def dec(blob=one, n=3, nq=1, m=1, ws=one, ws_bytes=big, pick=one, region_off=one, status=one, qtabs=one, blob_bytes=100,
            rgb_bytes=100, build_status=one, fmt=fmt):
        return L.rk_jpeg_decode_coef_as_u8(blob, blob_bytes, one, qtabs, nq, n, region_off, build_status, pick, one, m, one,
                                           rgb_bytes, ws, ws_bytes, status, None, fmt)
    assert dec(blob=None) == -1 and dec(pick=None) == -1 and dec(region_off=None) == -1 and dec(build_status=None) == -1
    assert dec(n=0) == -2 and dec(nq=0) == -2 and dec(nq=65536) == -2 and dec(m=0) == -2 and dec(m=65536) == -2
    assert dec(blob_bytes=-1) == -2 and dec(rgb_bytes=-1) == -2
    assert dec(blob=odd) == -2 and dec(qtabs=odd) == -2 and dec(region_off=ctypes.c_void_p(68)) == -2 and dec(pick=ctypes.c_void_p(66)) == -2
    assert dec(fmt=2) == -2 and dec(fmt=-1) == -2
    assert dec(ws=None) == -4 and dec(ws=ctypes.c_void_p(72)) == -4
    assert dec(m=2, ws_bytes=2 * 64 + 16 + 32 - 1) == -4    # records + flags + offset table of 2 frames


def test_build_coef_refuses_a_record_format_it_does_not_know():
    pytest.importorskip("PIL")
    _, res = dc.resident()
    with pytest.raises(RuntimeError, match="runs on a GPU"):
        jpeg.build_coef(res, "cpu", record="dense")
    for record in ("narrow", 1, None):
        with pytest.raises(ValueError, match="record must be 'wide' or 'dense'"):      # before the device is touched
            jpeg.build_coef(res, "cuda:0", record=record)
    assert jpeg.DeviceCoef(*range(10)).record == "wide" and jpeg.DeviceCoef(*range(10), "dense").record == "dense"


def test_the_cache_refuses_a_coef_record_that_does_not_fit():
    videos = [(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), 0)]
    for resident in ("rgb", "jpeg"):
        with pytest.raises(ValueError, match="coef_record='dense'.*resident='coef'.*resident='%s'" % resident):
            dataset.DeviceFrameCache(videos, 1, "val", num_segments=2, resident=resident, coef_record="dense")
    for resident in ("rgb", "coef"):
        with pytest.raises(ValueError, match="coef_record must be 'wide' or 'dense'"):
            dataset.DeviceFrameCache(videos, 1, "val", num_segments=2, resident=resident, coef_record="narrow")
    with pytest.raises(ValueError, match="resident must be 'rgb' or 'jpeg' or 'coef'"):     # no new resident value
        dataset.DeviceFrameCache(videos, 1, "val", num_segments=2, resident="dense")
    with pytest.raises(ValueError, match="resident='coef'.*decode='device'.*in-memory"):    # the source is still checked
        dataset.DeviceFrameCache(videos, 1, "val", num_segments=2, resident="coef", coef_record="dense")
