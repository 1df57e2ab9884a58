"""The chunked build of the JPEG scan index, without a GPU: a host run of the device code (csrc/rk_jpeg_core.hpp through
tests/jpeg_chunked_main.cpp, built with AddressSanitizer and UBSan and run as a child process, the lanes simulated in order
and the rounds in lock-step) beside the sequential walk on the same frames, at six settings; and the host side -- the
workspace size, row_tables, the entry point's argument checks, the keyword errors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _jpeg_cases as jc
import _jpeg_chunked_cases as cc
import _jpeg_index_cases as ic
from rubiksnet_amd import dataset, jpeg


@pytest.fixture(scope="module")
def host():
    run = cc.host_run()
    if run is None:
        pytest.skip("no host C++ compiler")
    return run


@pytest.fixture(scope="module")
def rec():
    return cc.records(cc.resident()[1])


# ------------------------------------------------------------------------------------------------- host run of the device code
def test_the_set_holds_what_the_scheme_must_meet(rec):
    names, res = cc.resident()
    base, _ = ic.resident()
    assert names[:len(base)] == list(base) and names[len(base):len(base) + len(cc.EXTRA)] == cc.EXTRA
    assert {int(r) for r in rec["restart_interval"]} == {0, 1, 2}
    length = dict(zip(names, rec["stream_len"].tolist()))
    assert all(length[x] <= 256 for x in cc.SHORT) and all(length["clip%d" % k] > 16 * 200 for k in range(8))
    if cc.big_picture() is not None:
        assert names[-1] == cc.BIG and 1024 < cc.chunk_counts(rec, 16)[-1] <= jpeg.MAX_CHUNKS     # more chunks than lanes


@pytest.mark.parametrize("setting", cc.SETTINGS)
def test_status_and_entries_are_the_sequential_walks(host, rec, setting):
    names, res = cc.resident()
    eo = res.entry_off.numpy()
    run = host[setting]
    assert run["status"].tolist() == host["chain"].tolist()
    assert np.array_equal(run["chunks"], cc.chunk_counts(rec, setting[0]))
    for i, name in enumerate(names):
        if host["chain"][i] == 0:
            a, b = run["entries"][eo[i]:eo[i + 1]], host["chain_entries"][eo[i]:eo[i + 1]]
            assert a.tobytes() == b.tobytes(), (setting, name, int(run["route"][i]))
    assert (host["chain"] == 0).sum() >= len(ic.GOOD) + len(cc.EXTRA) and (host["chain"] != 0).sum() == len(jc.CORRUPT)


def test_the_equality_is_not_won_by_falling_back(host, rec):
    names, _ = cc.resident()
    routes = {s: host[s]["route"] for s in cc.SETTINGS}
    cc.check_routes(routes, rec, names, host["chain"])
    print({s: {names[i]: int(routes[s][i]) for i in range(len(ic.GOOD) + len(jc.CORRUPT), len(names))} for s in cc.SETTINGS})
    # the dense noise frames do converge where a chunk is long enough to hold whole blocks, and the big one does at 64 bytes
    for name in cc.NOISE:
        assert routes[(256, 64)][names.index(name)] > 1
    if cc.big_picture() is not None:
        assert routes[(64, 16)][-1] > 1 and routes[(256, 64)][-1] > 1 and routes[(16, 64)][-1] > 1


def test_a_chunk_boundary_inside_a_stuffed_ff(host, rec):
    """From the bytes: good frames without restart markers in which a chunk starts at the 00 of an FF 00 pair, at a chunk
    size among the settings; the chunked walk won such a frame (route > 0) with the sequential walk's entries."""
    names, res = cc.resident()
    (_, _, _, streams), _ = jpeg.sections(res.blob, res.layout)
    streams = streams.numpy()
    found = []
    for setting in ((16, 64), (64, 16), (256, 64)):
        S = setting[0]
        for i in cc.good_plain(host, rec):
            seg = streams[int(rec["stream_off"][i]):int(rec["stream_off"][i]) + int(rec["stream_len"][i])]
            at = np.flatnonzero((seg[:-1] == 0xFF) & (seg[1:] == 0x00)) + 1
            if (at % S == 0).any() and host[setting]["route"][i] > 0:
                found.append((setting, names[i]))
    print(found)
    assert found


def test_some_chunks_only_pass_a_position_through(host):
    """Counted in the final pass, so at fixed points only: noise_q100_444 at 16 bytes has blocks longer than a chunk but reaches
    none within 64 rounds; the frames that do at 16 bytes hold pass-through chunks too (an MCU of a 4:2:0 clip frame often
    spans two chunks), and at 256 bytes nothing here is longer than a chunk."""
    names, _ = cc.resident()
    run = host[(16, 64)]
    won = [(names[i], int(run["passed"][i])) for i in range(len(names)) if run["route"][i] > 0 and run["passed"][i] > 0]
    print(won)
    assert len(won) >= 8 and any(name.startswith("clip") for name, _ in won)
    assert not host[(256, 64)]["passed"].any()


# ------------------------------------------------------------------------------------------------- sizes, tables, arguments
def test_chunked_workspace_bytes_equal_the_library(rec):
    from rubiksnet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("the HIP library is not built")
    L = _native.lib()
    frames = rec.copy()
    frames["stream_len"][3] = 0                             # no chunk
    frames["stream_len"][4] = 512 * 4096 + 1                # too many at every chunk size
    for S in jpeg.CHUNK_BYTES:
        for part in (frames, frames[:1], frames[5:9]):
            want = L.rk_jpeg_chunked_workspace_bytes(part.ctypes.data, len(part), S)
            assert want == jpeg.chunked_workspace_bytes_for(part, S) > 0 and want % 16 == 0, S
    assert jpeg.chunked_workspace_bytes_for(frames[4:5], 512) == 16 == jpeg.chunked_workspace_bytes_for(frames[3:4], 16)  # the table alone
    assert L.rk_jpeg_chunked_workspace_bytes(None, 3, 256) == 0 == L.rk_jpeg_chunked_workspace_bytes(frames.ctypes.data, 0, 256)
    assert L.rk_jpeg_chunked_workspace_bytes(frames.ctypes.data, 3, 48) == 0 == jpeg.chunked_workspace_bytes_for(frames, 48)


def test_the_entry_point_validates_before_anything_is_launched():
    from rubiksnet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("the HIP library is not built")
    L, one = _native.lib(), ctypes.c_void_p(64)              # a non-NULL dummy, never dereferenced on these paths
    def build(n=1, entries=one, n_entries=4, S=256, rounds=24, ws=one, ws_bytes=1 << 20, route=one):
        return L.rk_jpeg_build_index_chunked(one, 10, one, one, 1, 1, n, one, one, entries, n_entries, S, rounds, ws, ws_bytes, one,
                                             route, None)
    assert build(entries=None) == -1 and build(route=None) == -1
    assert build(n=0) == -2 and build(n=65536) == -2 and build(n_entries=-1) == -2
    assert [build(S=s) for s in (0, 8, 48, 100, 1024, -256)] == [-2] * 6
    assert build(rounds=-1) == -2 and build(rounds=65) == -2 and build(route=ctypes.c_void_p(66)) == -2
    assert build(ws=None) == -4 and build(ws=ctypes.c_void_p(72)) == -4 and build(n=3, ws_bytes=31) == -4


def test_row_tables_index_a_batch_by_mcu_row():
    names = ["p17x23_420", "p33x17_422", "p17x23_gray", "rst2_40x24_444", "clip0"]
    packed = jpeg.pack_jpeg_clips([([jc.jpg(x)], 0) for x in names])
    (frames, _, _, _), (n, _, _) = jpeg.sections(packed.blob, packed.layout)
    rec = np.frombuffer(frames.numpy().tobytes(), dtype=jpeg.FRAME_DTYPE).copy()
    rec["width"][2] = 0                                     # a record the build refuses: one segment of one MCU
    rows = jpeg.row_tables(rec, 64)
    raw = rows.tables.numpy()
    take = lambda k, dtype, count: np.frombuffer(raw[rows.offsets[k]:].tobytes(), dtype=dtype, count=count)
    mcus = [ic.mcus(x) for x in names]
    mcus[2] = (1, 1)
    assert take(0, np.int32, n).tolist() == [mx for mx, _ in mcus] and rows.max_segments == max(my for _, my in mcus)
    assert take(1, np.int64, n + 1).tolist() == np.concatenate([[0], np.cumsum([my for _, my in mcus])]).tolist()
    assert take(2, np.int32, n).tolist() == list(range(n)) and take(3, np.int64, n).tolist() == rec["rgb_off"].tolist()
    assert rows.n == n and rows.n_entries == sum(my for _, my in mcus) and all(o % 16 == 0 for o in rows.offsets)
    assert rows.build_bytes == jpeg.chunked_workspace_bytes_for(rec, 64)
    assert rows.decode_bytes == jpeg.indexed_workspace_bytes_for(rec, list(range(n)), rows.max_segments)


def test_the_keywords_are_checked(tmp_path):
    _, res = ic.resident()
    with pytest.raises(ValueError, match="method must be 'chain' or 'chunked'"):
        jpeg.build_index(res, "cuda:0", method="rows")
    with pytest.raises(ValueError, match="chunk_bytes must be one of"):
        jpeg.build_index(res, "cuda:0", method="chunked", chunk_bytes=100)
    with pytest.raises(ValueError, match=r"max_rounds must be in \[0, 64\]"):
        jpeg.build_index(res, "cuda:0", method="chunked", max_rounds=65)
    packed = jpeg.pack_jpeg_clips([([jc.jpg("p17x23_420")], 0)])
    with pytest.raises(ValueError, match="entropy must be 'chain' or 'rows'"):
        jpeg.decode_jpeg_frames(packed, "cuda:0", entropy="chunked")
    with pytest.raises(ValueError, match="chunk_bytes must be one of"):
        jpeg.decode_jpeg_frames(packed, "cuda:0", entropy="rows", chunk_bytes=8)
    videos = [(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), 0)]
    mem = dataset.InMemoryVideos([v for v, _ in videos], [0], num_segments=2, random_shift=False)
    with pytest.raises(ValueError, match="entropy must be 'chain' or 'rows'"):
        dataset.FrameLoader(mem, 1, "val", entropy="row")
    with pytest.raises(ValueError, match="entropy='rows'.*decode='device'"):
        dataset.FrameLoader(mem, 1, "val", entropy="rows")
    with pytest.raises(ValueError, match="index_build must be 'chain' or 'chunked'"):
        dataset.DeviceFrameCache(videos, 1, "val", num_segments=2, index_build="rows")
    with pytest.raises(ValueError, match="index_build='chunked'.*resident='jpeg'"):
        dataset.DeviceFrameCache(videos, 1, "val", num_segments=2, index_build="chunked")
    assert jpeg.DeviceIndex._fields[-1] == "route" and jpeg.DeviceIndex(*range(13)).route is None
