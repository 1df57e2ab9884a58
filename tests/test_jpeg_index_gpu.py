"""Resident JPEG frames decoded by scan index on the device (rk_jpeg_build_index, rk_jpeg_decode_indexed_u8) and
DeviceFrameCache(resident="jpeg") on them: every index case at every segment length bit-equal to its committed Pillow
decode inside guard bands, scattered picks, the corrupted corpus, tampered entries (after the host program has passed on the
same list), the cache against resident="rgb", the budget, graph capture.  Tiny images throughout."""
import io
import os

import numpy as np
import pytest
import torch

import _jpeg_cases as jc
import _jpeg_index_cases as ic
from rubiksnet_amd import dataset, jpeg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 4096, 0xC3


@pytest.fixture(scope="module", autouse=True)
def _hand_the_sentinel_blocks_back():
    """This module fills its arenas and guard bands with a sentinel byte.  When it is done those blocks go back to the
    driver instead of staying in torch's cache, where a later test's `torch.empty` would get them as they are."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def built():
    """The shared resident set (ic.resident(): the index cases at every E, then the corrupted corpus) on the device,
    its index built once.  -> (names, ResidentJpeg, DeviceIndex, host copy of the records, build status on the host)."""
    names, res = ic.resident()
    index = jpeg.build_index(res, DEV)
    torch.cuda.synchronize()
    (frames, _, _, _), _ = jpeg.sections(res.blob, res.layout)
    rec = np.frombuffer(frames.numpy().tobytes(), dtype=jpeg.FRAME_DTYPE)
    return names, res, index, rec, index.status.cpu().numpy()


def _decode_guarded(index, rec, res, pick, rgb_off, rgb_bytes, most=None, fill=SENTINEL):
    """One indexed launch: the RGB arena and a workspace of exactly the bytes asked for inside 4 KB guard bands of a
    sentinel byte.  -> (rgb, status) on the host after checking every guard."""
    m = len(pick)
    most = max(int(res.segments[p]) for p in pick if 0 <= p < index.n) if most is None else most
    ws_bytes = jpeg.indexed_workspace_bytes_for(rec, pick, most)
    arena = torch.full((rgb_bytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    arena[GUARD:GUARD + rgb_bytes] = fill
    ws = torch.full((ws_bytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    status = torch.full((m + 1 + 2,), -77, dtype=torch.int32, device=DEV)
    jpeg.launch_decode_indexed(index, torch.tensor(pick, dtype=torch.int32, device=DEV),
                               torch.tensor(rgb_off, dtype=torch.int64, device=DEV), most, arena[GUARD:GUARD + rgb_bytes],
                               ws[GUARD:GUARD + ws_bytes], status[:m + 1])
    torch.cuda.synchronize()
    arena, ws, status = arena.cpu().numpy(), ws.cpu().numpy(), status.cpu().numpy()
    for name, t, k in (("rgb", arena, rgb_bytes), ("workspace", ws, ws_bytes)):
        assert (t[:GUARD] == SENTINEL).all() and (t[GUARD + k:] == SENTINEL).all(), name + " guard touched"
    assert status[m + 1:].tolist() == [-77, -77]
    return arena[GUARD:GUARD + rgb_bytes], status[:m + 1]


def _bytes_of(rec, p):
    return int(rec["width"][p]) * int(rec["height"][p]) * 3


# ------------------------------------------------------------------------------------------------- goldens
def test_the_build_accepts_every_case_and_writes_the_host_cores_entries(built):
    names, res, index, rec, status = built
    n = len(ic.GOOD)
    assert status[:n].tolist() == [0] * n and status[-1] == len(jc.CORRUPT)
    host = ic.host_run()
    if host is not None:                                    # the same entries as the host run of the same code
        got = np.frombuffer(index.entries.cpu().numpy().tobytes(), dtype=jpeg.ENTRY_DTYPE)
        last = int(res.entry_off[n])
        assert np.array_equal(got[:last], host["entries"][:last])


@pytest.mark.parametrize("name", ic.CASES)
def test_every_case_at_every_segment_length_is_bit_equal_inside_guards(built, name):
    _, res, index, rec, _ = built
    for E in ic.segment_lengths(name):
        p = ic.frame_of(name, E)
        assert int(res.seg_mcus[p]) == E
        out, status = _decode_guarded(index, rec, res, [p], [0], _bytes_of(rec, p))
        want = jc.rgb(name)
        assert status.tolist() == [0, 0], (name, E, status.tolist())
        got = out.reshape(want.shape)
        assert np.array_equal(got, want), (name, E, int((got != want).sum()))


def test_all_cases_in_one_launch(built):
    _, res, index, rec, _ = built
    pick = list(range(len(ic.GOOD)))
    off, total = ic.rgb_table(res)
    out, status = _decode_guarded(index, rec, res, pick, off[:len(pick)].tolist(), int(off[len(pick)]))
    assert status.tolist() == [0] * (len(pick) + 1)
    for p, (name, E) in enumerate(ic.GOOD):
        want = jc.rgb(name)
        assert np.array_equal(out[off[p]:off[p] + want.size].reshape(want.shape), want), (name, E)


# ------------------------------------------------------------------------------------------------- picks
def test_scattered_picks_equal_the_single_frames_and_leave_the_gaps_alone():
    """Ten resident frames; [7, 2, 2, 9] to scattered offsets, frame 2 to two of them."""
    ten = ["b8_444", "b1_444", "p17x23_420", "p33x17_422", "p17x23_444", "p17x23_gray", "rst1_48x48_420", "rst2_40x24_444",
           "flat_420", "rst1_64x48_420"]
    res = jpeg.pack_resident([([jc.jpg(x)], 0) for x in ten])
    index = jpeg.build_index(res, DEV)
    assert index.status.tolist() == [0] * 11
    (frames, _, _, _), _ = jpeg.sections(res.blob, res.layout)
    rec = np.frombuffer(frames.numpy().tobytes(), dtype=jpeg.FRAME_DTYPE)
    pick = [7, 2, 2, 9]
    sizes = [_bytes_of(rec, p) for p in pick]
    offs = [12000, 11, 16000, 1500]
    spans = sorted(zip(offs, sizes))
    assert all(a + k <= b for (a, k), (b, _) in zip(spans, spans[1:]))
    total = 17500
    out, status = _decode_guarded(index, rec, res, pick, offs, total, fill=0x5E)
    assert status.tolist() == [0, 0, 0, 0, 0]
    mask = np.ones(total, dtype=bool)
    for p, off, k in zip(pick, offs, sizes):
        single, st = _decode_guarded(index, rec, res, [p], [0], k)
        assert st.tolist() == [0, 0] and np.array_equal(out[off:off + k], single)
        want = jc.rgb(ten[p])
        assert np.array_equal(single.reshape(want.shape), want)
        mask[off:off + k] = False
    assert (out[mask] == 0x5E).all()


# ------------------------------------------------------------------------------------------------- the corrupted corpus
def test_the_build_status_of_the_corrupted_corpus_is_the_plain_decoders(built):
    names, res, index, rec, status = built
    first = len(ic.GOOD)
    packed = jpeg.pack_jpeg_clips([([jc.jpg(x)], 0) for x in jc.CORRUPT])
    _, _, plain = jpeg.decode_jpeg_frames(packed, DEV)
    plain = plain.cpu().numpy()
    assert names[first:] == list(jc.CORRUPT) and plain[-1] == len(jc.CORRUPT)
    assert status[first:first + len(jc.CORRUPT)].tolist() == plain[:-1].tolist()
    assert (plain[:-1] != 0).all()


def test_a_corrupt_frame_between_two_good_ones_is_a_zero_frame_with_its_code(built):
    names, res, index, rec, status = built
    good = ic.frame_of("p17x23_420", 2)
    k = 17 * 23 * 3
    for bad in (len(ic.GOOD) + jc.CORRUPT.index("corrupt_cut50"), len(ic.GOOD) + jc.CORRUPT.index("corrupt_rst_swapped"),
                len(ic.GOOD) + len(jc.BROKEN)):
        out, st = _decode_guarded(index, rec, res, [good, bad, good], [0, k, 2 * k], 3 * k)
        assert st.tolist() == [0, int(status[bad]), 0, 1] and status[bad] != 0
        frames = out.reshape(3, 23, 17, 3)
        assert np.array_equal(frames[0], jc.rgb("p17x23_420")) and np.array_equal(frames[2], jc.rgb("p17x23_420"))
        assert not frames[1].any()


def test_picks_and_records_that_do_not_fit(built):
    """A pick outside the set, an output range past the arena, max_segments smaller than the frame's count: a code each,
    zeros where the range is valid, nothing written where it is not, the good neighbour untouched by any of it."""
    _, res, index, rec, _ = built
    good = ic.frame_of("p17x23_420", 1)                     # four segments
    k = 17 * 23 * 3
    out, st = _decode_guarded(index, rec, res, [good, index.n, -1, good, good], [0, k, k, 3 * k + 1, 2 * k], 4 * k, most=4)
    assert st.tolist() == [0, 1, 1, 1, 0, 3]
    frames = out.reshape(4, 23, 17, 3)
    assert np.array_equal(frames[0], jc.rgb("p17x23_420")) and np.array_equal(frames[2], jc.rgb("p17x23_420"))
    assert (frames[1] == SENTINEL).all() and (frames[3] == SENTINEL).all()
    out, st = _decode_guarded(index, rec, res, [good, ic.frame_of("p17x23_420", 4)], [0, k], 2 * k, most=3)
    assert st.tolist() == [8, 0, 1] and not out[:k].any()
    assert np.array_equal(out[k:].reshape(23, 17, 3), jc.rgb("p17x23_420"))


# ------------------------------------------------------------------------------------------------- tampered entries
@pytest.fixture(scope="module")
def host_codes():
    """The host program's verdict on ic.tampers(); the device test below runs only after it passed on the same list."""
    host = ic.host_run()
    if host is None:
        pytest.skip("no host C++ compiler")
    for (i, k, a, b), (code, same) in zip(ic.tampers(), host["tampered"].tolist()):
        assert code != 0 or same == 1, (ic.GOOD[i], ic.KINDS[k], a, b)
    return host["tampered"][:, 0].tolist()


def test_tampered_entries_get_the_host_cores_codes_and_a_zero_frame(built, host_codes):
    """Bounded refusal: an entry that was changed makes a segment fail its checks (before its first read, or where it
    ends); nothing here reads or writes outside the arenas.  All tampered copies are decoded in ONE launch, each from its
    own copy of the frame's entries appended to the table, an untouched frame in front and behind."""
    names, res, index, rec, _ = built
    rows = ic.tampers()
    entries = np.frombuffer(index.entries.cpu().numpy().tobytes(), dtype=jpeg.ENTRY_DTYPE).copy()
    eo = res.entry_off.numpy()
    # resident records n, n + 1, ...: copies of the tampered frames' records, each with entries of its own
    extra_rec, extra_entries, extra_off = [], [], [int(eo[-1])]
    for i, kind, a, b in rows:
        e = entries[eo[i]:eo[i + 1]].copy()
        if kind == 0:
            e["bit_pos"][a] += 1
        elif kind == 1:
            e["bit_pos"][a] -= 1
        elif kind == 2:
            e["bit_pos"][a] = 8 * int(rec["stream_len"][i]) + 1
        elif kind == 3:
            e["bit_pos"][a] = -1
        elif kind == 4:
            e["pred"][a][0] += 1
        elif kind == 5:
            e["pred"][a][0] = 4000
        else:
            e[[a, b]] = e[[b, a]]
        extra_rec.append(rec[i])
        extra_entries.append(e)
        extra_off.append(extra_off[-1] + len(e))
    n = index.n
    all_rec = np.concatenate([rec, np.stack(extra_rec)])
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to(DEV)
    tampered = index._replace(
        frames=dev(all_rec), n=n + len(rows),
        seg_mcus=torch.cat([index.seg_mcus, index.seg_mcus[[i for i, _, _, _ in rows]]]),
        entry_off=torch.cat([index.entry_off, torch.tensor(extra_off[1:], dtype=torch.int64, device=DEV)]),
        entries=dev(np.concatenate([entries] + extra_entries)), n_entries=extra_off[-1],
        status=torch.cat([index.status[:n], torch.zeros(len(rows) + 1, dtype=torch.int32, device=DEV)]))
    good = ic.frame_of("p33x17_422", 3)
    pick = [good] + list(range(n, n + len(rows))) + [good]
    sizes = [_bytes_of(all_rec, p) for p in pick]
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    res2 = res._replace(segments=torch.cat([res.segments, res.segments[[i for i, _, _, _ in rows]]]))
    out, st = _decode_guarded(tampered, all_rec, res2, pick, offs[:-1], offs[-1])
    assert st[0] == st[len(pick) - 1] == 0
    for p in (0, len(pick) - 1):
        assert np.array_equal(out[offs[p]:offs[p + 1]].reshape(17, 33, 3), jc.rgb("p33x17_422"))
    assert st[1:-2].tolist() == host_codes
    assert st[-1] == sum(c != 0 for c in host_codes) == len(rows)
    assert not out[offs[1]:offs[-2]].any()


# ------------------------------------------------------------------------------------------------- the cache
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """Six Pillow-written videos of 6-10 frames, four at 48x64 and two at 40x56 (smooth pictures: small files), and list
    files; one frame is progressive, so the host decodes it."""
    pytest.importorskip("PIL")
    from PIL import Image
    root = tmp_path_factory.mktemp("jpeg_cache")
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:48, 0:64]
    lines = []
    for v, (count, (h, w)) in enumerate(zip((6, 7, 8, 9, 10, 6), [(48, 64)] * 4 + [(40, 56)] * 2)):
        os.makedirs(root / ("v%d" % v))
        for k in range(count):
            a, b, c = rng.uniform(0.5, 3.0, 3)
            pic = np.stack([127 + 120 * np.sin(xx / (4 * a) + k) * np.cos(yy / (5 * b)), 2 * xx + 3 * yy + 9 * k,
                            127 + 100 * np.cos((xx + yy) / (6 * c) - k)], axis=-1)[:h, :w]
            pic = np.clip(pic + rng.normal(0, 2, pic.shape), 0, 255).astype(np.uint8)
            buf = io.BytesIO()
            Image.fromarray(pic).save(buf, "JPEG", quality=85, progressive=(v, k) == (2, 3))
            with open(root / ("v%d" % v) / ("img_%05d.jpg" % (k + 1)), "wb") as fh:
                fh.write(buf.getvalue())
        lines.append("v%d %d %d\n" % (v, count, v % 4))
    with open(root / "list.txt", "w") as fh:
        fh.writelines(lines)
    return str(root)


def _dataset(folder, split, decode, **kw):
    return dataset.RubiksDataset(folder, os.path.join(folder, "list.txt"), num_segments=4, random_shift=split == "train",
                                 test_mode=split == "test", twice_sample=split == "test", only_even_indices=False,
                                 decode=decode, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("split", ["train", "val", "test"])
def test_the_jpeg_cache_equals_the_rgb_cache(folder, split, dtype):
    """Two epochs, equal seeds: clips and labels of resident="jpeg" are bit-equal to resident="rgb"."""
    def run(resident):
        ds = _dataset(folder, split, "device" if resident == "jpeg" else "host")
        cache = dataset.DeviceFrameCache(ds, 4, split, device=DEV, dtype=dtype, size=32, seed=5, resident=resident)
        got = [(clips.clone(), labels.clone()) for _ in range(2) for clips, labels in cache]
        torch.cuda.synchronize()
        return got, cache

    rgb, _ = run("rgb")
    jpg, cache = run("jpeg")
    assert len(rgb) == len(jpg) == 4
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    for (rc, rl), (jc_, jl) in zip(rgb, jpg):
        assert rc.shape == jc_.shape == (rl.numel() * (2 if split == "test" else 1), 4, 3, 32, 32) and jc_.dtype == dtype
        assert torch.equal(rc.view(bits), jc_.view(bits)) and torch.equal(rl, jl)
    assert cache.fallback_frames == 1 and cache.decode_errors() == 0


def test_a_budget_between_the_two_footprints(folder):
    decoded = sum(n * h * w * 3 for n, (h, w) in zip((6, 7, 8, 9, 10, 6), [(48, 64)] * 4 + [(40, 56)] * 2))
    probe = dataset.DeviceFrameCache(_dataset(folder, "val", "device"), 1, "val", device=DEV, size=32, resident="jpeg")
    for _ in probe:
        pass
    need = probe.resident_bytes
    assert need < decoded * 3 // 4, (need, decoded)
    budget = (need + decoded) // 2
    with pytest.raises(RuntimeError, match="over the budget"):
        dataset.DeviceFrameCache(_dataset(folder, "val", "host"), 1, "val", device=DEV, size=32, budget_bytes=budget)
    cache = dataset.DeviceFrameCache(_dataset(folder, "val", "device"), 1, "val", device=DEV, size=32, budget_bytes=budget,
                                     resident="jpeg")
    assert sum(labels.numel() for _, labels in cache) == 6 and cache.resident_bytes <= budget
    with pytest.raises(RuntimeError, match="over the budget"):
        dataset.DeviceFrameCache(_dataset(folder, "val", "device"), 1, "val", device=DEV, size=32, resident="jpeg",
                                 budget_bytes=probe._fixed_bytes - 1)
    tight = dataset.DeviceFrameCache(_dataset(folder, "val", "device"), 1, "val", device=DEV, size=32, resident="jpeg",
                                     budget_bytes=probe._fixed_bytes + 100)
    with pytest.raises(RuntimeError, match="over the budget"):
        next(iter(tight))


# ------------------------------------------------------------------------------------------------- capture
def test_the_indexed_decode_is_capturable_as_one_chain(built):
    _, res, index, rec, _ = built
    pick = [ic.frame_of("p17x23_420", 2), ic.frame_of("rst1_64x48_420", 4), ic.frame_of("p17x23_gray", 1)]
    sizes = [_bytes_of(rec, p) for p in pick]
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    eager, eager_status = _decode_guarded(index, rec, res, pick, offs[:-1], offs[-1])
    most = max(int(res.segments[p]) for p in pick)
    pick_d = torch.tensor(pick, dtype=torch.int32, device=DEV)
    off_d = torch.tensor(offs[:-1], dtype=torch.int64, device=DEV)
    rgb = torch.full((offs[-1],), 9, dtype=torch.uint8, device=DEV)
    ws = torch.empty(jpeg.indexed_workspace_bytes_for(rec, pick, most), dtype=torch.uint8, device=DEV)
    status = torch.full((len(pick) + 1,), -1, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):          # seven launches on one stream: a linear chain, no branches
            jpeg.launch_decode_indexed(index, pick_d, off_d, most, rgb, ws, status)
    torch.cuda.current_stream(DEV).wait_stream(side)
    rgb.fill_(9)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(rgb.cpu().numpy(), eager) and status.cpu().numpy().tolist() == eager_status.tolist() == [0, 0, 0, 0]
