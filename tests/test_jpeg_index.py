"""The scan index of the device JPEG decode, without a GPU: a host run of the device code (csrc/rk_jpeg_core.hpp through
tests/jpeg_index_main.cpp, built with AddressSanitizer and UBSan and run as a child process) over every index case at
every segment length, the corrupted corpus and a list of tampered entries; and the host side -- pack_resident,
pick_tables, the workspace size, DeviceFrameCache's argument errors."""
import os

import numpy as np
import pytest
import torch

import _jpeg_cases as jc
import _jpeg_index_cases as ic
from rubiksnet_amd import dataset, jpeg


@pytest.fixture(scope="module")
def host():
    run = ic.host_run()
    if run is None:
        pytest.skip("no host C++ compiler")
    return run


# ------------------------------------------------------------------------------------------------- host run of the device code
def test_the_cases_are_what_the_index_needs():
    assert [ic.mcus(n) for n in ("p17x23_420", "p33x17_422", "rst2_40x24_444")] == [(2, 2), (3, 3), (5, 3)]
    assert ic.segment_lengths("rst2_40x24_444") == [1, 5, 15, 18] and len(ic.GOOD) == 4 * len(ic.CASES)
    assert {jpeg.parse_jpeg(jc.jpg(n)).restart_interval for n in ic.CASES} == {0, 1, 2}


def test_recorded_index_starts_at_zero_and_never_goes_back(host):
    _, res = ic.resident()
    eo = res.entry_off.numpy()
    for i, (name, E) in enumerate(ic.GOOD):
        assert host["whole"][i] == host["built"][i] == 0, (name, E)
        e = host["entries"][eo[i]:eo[i + 1]]
        mx, my = ic.mcus(name)
        assert len(e) == (mx * my + E - 1) // E == int(res.segments[i])
        assert int(e["bit_pos"][0]) == 0 and not e["pred"][0].any() and not e["reserved"].any(), (name, E)
        assert (np.diff(e["bit_pos"]) >= 0).all() and (np.abs(e["pred"]) <= 2047).all(), (name, E)
        head = jpeg.parse_jpeg(jc.jpg(name))
        assert int(e["bit_pos"][-1]) <= 8 * (head.scan[1] - head.scan[0])
        if len(e) > 1:
            assert int(e["bit_pos"][1]) > 0
    # the same frame at E = 1 and at E = mcux: the coarser index is every mcux-th entry of the finer one
    for name in ic.CASES:
        mx, _ = ic.mcus(name)
        i, j = ic.frame_of(name, 1), ic.frame_of(name, mx)
        fine, coarse = host["entries"][eo[i]:eo[i + 1]], host["entries"][eo[j]:eo[j + 1]]
        assert np.array_equal(fine[::mx], coarse), name


def test_restart_entries_sit_on_the_marker(host):
    """R = 1: every entry but the first is taken with a restart due.  Where the MCU ended on a byte boundary the reader has
    used everything up to the marker and bit_pos is the marker's FF, bit 0; otherwise it stands in the last data byte, in
    front of pad bits that are ones, and the marker follows that byte."""
    _, res = ic.resident()
    eo = res.entry_off.numpy()
    i = ic.frame_of("rst1_64x48_420", 1)
    data = jc.jpg("rst1_64x48_420")
    a, _ = jpeg.parse_jpeg(data).scan
    pos = host["entries"][eo[i]:eo[i + 1]]["bit_pos"]
    assert len(pos) == 12
    aligned = 0
    for m, p in enumerate(pos[1:].tolist(), 1):
        at, bit = a + p // 8, p % 8
        if bit:
            pad = (1 << (8 - bit)) - 1
            assert data[at] & pad == pad, m
            at += 2 if data[at] == 0xFF else 1              # a data byte FF is FF 00
        aligned += bit == 0
        assert data[at] == 0xFF and data[at + 1] == 0xD0 + ((m - 1) & 7), m
    print("entries on a byte boundary:", aligned)


def test_every_segment_alone_in_reverse_order_tiles_the_frame(host):
    """tiled: each segment decoded alone into a fresh buffer gave code 0, the whole walk's coefficients for its own blocks
    and touched no other; the RGB put together from the segments equals the golden."""
    for i, (name, E) in enumerate(ic.GOOD):
        assert host["tiled"][i] == 1, (name, E)
        want = jc.rgb(name)
        off = int(host["rgb_off"][i])
        got = host["rgb"][off:off + want.size].reshape(want.shape)
        assert np.array_equal(got, want), (name, E, int((got != want).sum()))


def test_the_build_gives_the_corrupted_corpus_the_whole_walks_codes(host):
    first = len(ic.GOOD)
    assert host["names"][first:] == list(jc.CORRUPT)
    for k, name in enumerate(jc.CORRUPT, first):
        assert host["built"][k] == host["whole"][k] != 0, (name, host["built"][k], host["whole"][k])
        off = int(host["rgb_off"][k])
        assert not host["rgb"][off:off + 17 * 23 * 3].any()
    assert len(set(host["whole"][first:].tolist())) >= 3        # several kinds of failure are among them


def test_no_tampered_entry_decodes_silently_wrong(host):
    rows = ic.tampers()
    assert {k for _, k, _, _ in rows} == set(range(len(ic.KINDS))) and len(rows) == len(host["tampered"])
    print({(ic.GOOD[i][0], ic.KINDS[k], a, b): jpeg.STATUS_NAMES[code]
           for (i, k, a, b), (code, _) in zip(rows, host["tampered"].tolist())})
    for (i, k, a, b), (code, same) in zip(rows, host["tampered"].tolist()):
        assert code != 0 or same == 1, (ic.GOOD[i], ic.KINDS[k], a, b)
        assert 0 <= code < len(jpeg.STATUS_NAMES)
    # the spans tile the stream: an entry that was changed is noticed by the span that ends there, or starts there
    assert all(code == 8 for code, _ in host["tampered"].tolist())


# ------------------------------------------------------------------------------------------------- pack_resident
def test_pack_resident_lays_out_the_set_and_shares_tables():
    pytest.importorskip("PIL")
    a, b, g = jc.jpg("p17x23_420"), jc.jpg("p17x23_444"), jc.jpg("p17x23_gray")
    prog = jc.jpg("unsupported_progressive")                # 16x16, decoded on the host
    flat = jc.jpg("flat_420")                               # 16x16
    res = jpeg.pack_resident([([a, b, a], 4), ([flat, prog, flat], 9), ([g, g], 1)])
    (frames, htabs, qtabs, streams), (n, nh, nq) = jpeg.sections(res.blob, res.layout)
    assert (n, len(res.fallback)) == (7, 1) and res.labels.tolist() == [4, 9, 1]
    assert res.videos.tolist() == [[0, 3, 23, 17], [3, 3, 16, 16], [6, 2, 23, 17]]
    assert res.slots.tolist() == [0, 1, 2, 3, -1, 4, 5, 6]
    assert np.array_equal(res.fallback[0].numpy(), jpeg._host_rgb(prog))
    rec = np.frombuffer(frames.numpy().tobytes(), dtype=jpeg.FRAME_DTYPE)
    heads = [jpeg.parse_jpeg(x) for x in (a, b, a, flat, flat, g, g)]
    lens = [h.scan[1] - h.scan[0] for h in heads]
    assert rec["stream_len"].tolist() == lens and rec["stream_off"].tolist() == np.cumsum([0] + lens[:-1]).tolist()
    assert not rec["rgb_off"].any()                         # a resident frame gets its place when it is picked
    for r, h, data in zip(rec, heads, (a, b, a, flat, flat, g, g)):
        s = int(r["stream_off"])
        assert streams[s:s + int(r["stream_len"])].numpy().tobytes() == data[h.scan[0]:h.scan[1]]
    # Pillow's default tables at one quality: 2 quantisation and 4 Huffman tables in all, a repeated file adds none
    assert (nq, nh) == (2, 4) and rec["quant"][0].tolist() == rec["quant"][1].tolist() == rec["quant"][2].tolist()
    # one segment per MCU row by default: 17x23 4:2:0 is 2x2 MCUs, 4:4:4 and gray 3x3, 16x16 4:2:0 one MCU
    assert res.seg_mcus.tolist() == [2, 3, 2, 1, 1, 3, 3] and res.segments.tolist() == [2, 3, 2, 1, 1, 3, 3]
    assert res.entry_off.tolist() == [0, 2, 5, 7, 8, 9, 12, 15]
    one = jpeg.pack_resident([([a, b], 0)], seg_mcus=4)
    assert one.seg_mcus.tolist() == [4, 4] and one.segments.tolist() == [1, 3] and one.entry_off.tolist() == [0, 1, 4]
    each = jpeg.pack_resident([([a, b], 0)], seg_mcus=[1, 100])
    assert each.segments.tolist() == [4, 1]
    with pytest.raises(ValueError, match="differ in size"):
        jpeg.pack_resident([([a, flat], 0)])
    with pytest.raises(ValueError, match="at least 1"):
        jpeg.pack_resident([([a], 0)], seg_mcus=0)


# ------------------------------------------------------------------------------------------------- pick_tables
def _brute_pick(res, ids, numbers):
    """pick_tables restated: walk the asked-for frames one by one and look every earlier one up again."""
    pick, rgb_off, rows, idx, fallback, at = [], [], [], [], [], 0
    for v, nums in zip(ids, numbers):
        first, count, h, w = res.videos[v].tolist()
        seen = []
        for p in nums:
            if p not in seen:
                seen.append(p)
        for k, p in enumerate(seen):
            slot = int(res.slots[first + p])
            if slot < 0:
                fallback.append((-1 - slot, at + k * h * w * 3))
            else:
                pick.append(slot)
                rgb_off.append(at + k * h * w * 3)
        idx.append([seen.index(p) for p in nums])
        rows.append([at, h, w, len(seen)])
        at += len(seen) * h * w * 3
    return pick, rgb_off, rows, idx, fallback, at


def _check_pick(res, ids, numbers):
    t = jpeg.pick_tables(res, ids, numbers)
    pick, rgb_off, rows, idx, fallback, total = _brute_pick(res, ids, numbers)
    assert t.pick.dtype == torch.int32 and t.rgb_off.dtype == torch.int64 and t.clips.dtype == torch.int64
    assert t.pick.tolist() == pick and t.rgb_off.tolist() == rgb_off and t.clips.tolist() == rows
    assert [x.tolist() for x in t.frame_idx] == idx and t.fallback == fallback and t.rgb_bytes == total
    assert t.max_segments == max([1] + [int(res.segments[p]) for p in pick])
    return t


def test_pick_tables_decodes_a_repeated_frame_once():
    pytest.importorskip("PIL")
    a, b, flat, prog = jc.jpg("p17x23_420"), jc.jpg("p17x23_444"), jc.jpg("flat_420"), jc.jpg("unsupported_progressive")
    res = jpeg.pack_resident([([a, b, a], 0), ([flat, prog, flat, flat], 1), ([b] * 5, 2)])
    # a short video read at frames 0, 0, 1, 2, 2, 2 holds three frames in the arena
    t = _check_pick(res, [0], [[0, 0, 1, 2, 2, 2]])
    assert t.pick.tolist() == [0, 1, 2] and t.frame_idx[0].tolist() == [0, 0, 1, 2, 2, 2] and t.clips.tolist() == [[0, 23, 17, 3]]
    # first use decides the order; the host-decoded frame takes a place and no pick; a video may come twice
    t = _check_pick(res, [1, 2, 0, 1], [[3, 1, 3, 0], [4, 4, 4], [2, 0], [1]])
    assert t.pick.tolist() == [5, 3, 10, 2, 0] and t.fallback == [(0, 768), (0, t.clips[3, 0].item())]
    assert t.max_segments == 3
    with pytest.raises(ValueError, match="frame 3 of a video of 3"):
        jpeg.pick_tables(res, [0], [[3]])


def test_pick_tables_on_a_twice_sample_draw():
    """Eleven frames, test split with twice_sample: 2 x 4 frame numbers, some of them equal."""
    b = jc.jpg("p17x23_444")
    res = jpeg.pack_resident([([b] * 11, 0), ([b] * 3, 1)])
    for nf, v in ((11, 0), (3, 1)):
        p = dataset.segment_indices(nf, 4, "test", twice_sample=True)
        assert len(p) == 8
        nums = (np.clip(p, 1, nf) - 1).tolist()
        t = _check_pick(res, [v], [nums])
        assert len(set(nums)) == t.pick.numel() <= 8
    assert t.pick.numel() < 8                               # three frames cannot fill eight places without repeats


# ------------------------------------------------------------------------------------------------- sizes, arguments
def test_indexed_workspace_bytes_equal_the_library():
    from rubiksnet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("the HIP library is not built")
    _, res = ic.resident()
    (frames, _, _, _), (n, _, _) = jpeg.sections(res.blob, res.layout)
    rec = np.frombuffer(frames.numpy().tobytes(), dtype=jpeg.FRAME_DTYPE).copy()
    rec["width"][1] = 0                                     # an invalid record takes no frame region
    L = _native.lib()
    for pick, most in (([7, 2, 2, 9], 5), ([0], 1), ([1, 1], 3), ([n - 1, -1, n, 4], 65535), (list(range(n)), 16)):
        arr = np.asarray(pick, dtype=np.int32)
        want = L.rk_jpeg_indexed_workspace_bytes(rec.ctypes.data, n, arr.ctypes.data, len(pick), most)
        assert want == jpeg.indexed_workspace_bytes_for(rec, pick, most) > 0, (pick, most)
        assert want % 16 == 0 and want >= len(pick) * (64 + 4 * most)
    one = np.zeros(1, dtype=np.int32)
    assert L.rk_jpeg_indexed_workspace_bytes(None, n, one.ctypes.data, 1, 1) == 0
    assert L.rk_jpeg_indexed_workspace_bytes(rec.ctypes.data, n, one.ctypes.data, 0, 1) == 0
    assert L.rk_jpeg_indexed_workspace_bytes(rec.ctypes.data, n, one.ctypes.data, 1, 0) == 0
    assert jpeg.indexed_workspace_bytes_for(rec, [], 4) == 0 and jpeg.indexed_workspace_bytes_for(rec, [1], 0) == 0


def test_the_entry_points_validate_before_anything_is_launched():
    from rubiksnet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("the HIP library is not built")
    import ctypes
    L, one = _native.lib(), ctypes.c_void_p(64)              # a non-NULL dummy, never dereferenced on these paths
    build = lambda n=1, entries=one, n_entries=4: L.rk_jpeg_build_index(one, 10, one, one, 1, 1, n, one, one, entries, n_entries,
                                                                        one, None)
    assert build(entries=None) == -1 and build(n=0) == -2 and build(n=65536) == -2 and build(n_entries=-1) == -2
    dec = lambda m=1, most=1, ws=one, ws_bytes=1 << 20, pick=one: L.rk_jpeg_decode_indexed_u8(
        one, 10, one, one, one, 1, 1, 3, one, 4, one, one, one, pick, one, m, most, one, 100, ws, ws_bytes, one, None)
    assert dec(pick=None) == -1 and dec(m=0) == -2 and dec(m=65536) == -2 and dec(most=0) == -2 and dec(most=65536) == -2
    assert dec(ws=None) == -4 and dec(ws=ctypes.c_void_p(72)) == -4
    assert dec(m=2, most=3, ws_bytes=2 * 64 + 32 + 32 - 1) == -4      # records + segment table + offset table of 2 frames
    assert jpeg.STATUS_NAMES[8] == "bad index" and len(jpeg.STATUS_NAMES) == 9


def test_the_cache_refuses_sources_that_hold_no_files(tmp_path):
    pytest.importorskip("PIL")
    videos = [(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), 0)]
    with pytest.raises(ValueError, match="resident must be 'rgb' or 'jpeg'"):
        dataset.DeviceFrameCache(videos, 1, "val", num_segments=2, resident="bytes")
    with pytest.raises(ValueError, match="decode='device'.*in-memory"):
        dataset.DeviceFrameCache(videos, 1, "val", num_segments=2, resident="jpeg")
    mem = dataset.InMemoryVideos([v for v, _ in videos], [0], num_segments=2, random_shift=False)
    with pytest.raises(ValueError, match="decode='device'.*in-memory"):
        dataset.DeviceFrameCache(mem, 1, "val", resident="jpeg")
    os.makedirs(tmp_path / "a")
    for k in range(1, 5):
        with open(tmp_path / "a" / ("img_%05d.jpg" % k), "wb") as fh:
            fh.write(jc.jpg("p17x23_420"))
    with open(tmp_path / "list.txt", "w") as fh:
        fh.write("a 4 3\n")
    make = lambda decode: dataset.RubiksDataset(str(tmp_path), str(tmp_path / "list.txt"), num_segments=2, random_shift=False,
                                                only_even_indices=False, decode=decode)
    with pytest.raises(ValueError, match="decode='device'.*decode='host' dataset"):
        dataset.DeviceFrameCache(make("host"), 1, "val", resident="jpeg")
    frames, label = make("device").whole_bytes(0)
    assert label == 3 and frames == [jc.jpg("p17x23_420")] * 4
