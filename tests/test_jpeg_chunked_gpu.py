"""The chunked build of the JPEG scan index on the device (rk_jpeg_build_index_chunked) and what is built on it: status and
entries equal to rk_jpeg_build_index's inside guard bands at six settings, the route array equal to the host program's
element for element, decode_jpeg_frames / FrameLoader with entropy="rows" and DeviceFrameCache(index_build="chunked")
bit-equal to the sequential paths, graph capture.  Small images throughout."""
import io
import os

import numpy as np
import pytest
import torch

import _jpeg_cases as jc
import _jpeg_chunked_cases as cc
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
def chain():
    """cc.resident() on the device with the sequential build: the reference, computed once.
    -> (names, ResidentJpeg, DeviceIndex, records, status, entries) -- the last three on the host."""
    names, res = cc.resident()
    index = jpeg.build_index(res, DEV, method="chain")
    torch.cuda.synchronize()
    assert index.route is None
    entries = np.frombuffer(index.entries.cpu().numpy().tobytes(), dtype=jpeg.ENTRY_DTYPE)
    return names, res, index, cc.records(res), index.status.cpu().numpy(), entries


def _guarded(nbytes):
    t = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    return t, t[GUARD:GUARD + nbytes]


def _guards_ok(t, nbytes):
    t = t.cpu().numpy()
    return bool((t[:GUARD] == SENTINEL).all() and (t[GUARD + nbytes:] == SENTINEL).all())


def _build_guarded(index, rec, chunk_bytes, max_rounds):
    """One chunked build over the set `index` holds: entries, workspace, status and route each inside 4 KB guard bands of a
    sentinel.  -> (status [n + 1], route [n], entries) on the host after checking every guard."""
    n = index.n
    ws_bytes = jpeg.chunked_workspace_bytes_for(rec, chunk_bytes)
    whole_e, entries = _guarded(index.n_entries * 16)
    whole_w, ws = _guarded(ws_bytes)
    whole_s, status = _guarded(4 * (n + 1))
    whole_r, route = _guarded(4 * n)
    jpeg.launch_build_index_chunked(index.streams, index.frames, index.htabs, index.nq, index.nh, n, index.seg_mcus, index.entry_off,
                                    entries, index.n_entries, chunk_bytes, max_rounds, ws, status.view(torch.int32),
                                    route.view(torch.int32))
    torch.cuda.synchronize()
    for name, t, k in (("entries", whole_e, index.n_entries * 16), ("workspace", whole_w, ws_bytes), ("status", whole_s, 4 * (n + 1)),
                       ("route", whole_r, 4 * n)):
        assert _guards_ok(t, k), name + " guard touched"
    return (status.view(torch.int32).cpu().numpy(), route.view(torch.int32).cpu().numpy(),
            np.frombuffer(entries.cpu().numpy().tobytes(), dtype=jpeg.ENTRY_DTYPE))


@pytest.fixture(scope="module")
def builds(chain):
    _, _, index, rec, _, _ = chain
    return {setting: _build_guarded(index, rec, *setting) for setting in cc.SETTINGS}


# ------------------------------------------------------------------------------------------------- the build
@pytest.mark.parametrize("setting", cc.SETTINGS)
def test_status_and_entries_equal_the_sequential_build_inside_guards(chain, builds, setting):
    names, res, index, rec, want_status, want_entries = chain
    status, route, entries = builds[setting]
    assert status.tolist() == want_status.tolist() and status[-1] == len(jc.CORRUPT)
    eo = res.entry_off.numpy()
    for i, name in enumerate(names):
        if want_status[i] == 0:
            assert entries[eo[i]:eo[i + 1]].tobytes() == want_entries[eo[i]:eo[i + 1]].tobytes(), (setting, name, int(route[i]))


def test_the_route_is_the_host_programs_and_is_not_won_by_falling_back(chain, builds):
    names, _, _, rec, want_status, _ = chain
    routes = {s: builds[s][1] for s in cc.SETTINGS}
    cc.check_routes(routes, rec, names, want_status[:-1])
    host = cc.host_run()
    if host is None:
        pytest.skip("no host C++ compiler")
    for setting in cc.SETTINGS:                             # the algorithm is deterministic: element for element
        assert routes[setting].tolist() == host[setting]["route"].tolist(), setting
        assert builds[setting][0][:-1].tolist() == host[setting]["status"].tolist()


def test_a_workspace_too_short_for_a_frame_sends_it_down_the_chain(chain):
    """The launcher checks the offset table alone; a frame whose region does not fit takes the sequential walk."""
    names, res, index, rec, want_status, want_entries = chain
    n = index.n
    full = jpeg.chunked_workspace_bytes_for(rec, 64)
    tail = cc.chunk_counts(rec, 64)[n - 3:]
    assert (tail > 0).all()
    short = full - 32 * int(tail.sum())                     # the whole offset table, the regions of all frames but three
    assert short < full
    whole_w, ws = _guarded(short)
    entries = torch.zeros(index.n_entries * 2, dtype=torch.int64, device=DEV).view(torch.uint8)
    status = torch.full((n + 1,), -5, dtype=torch.int32, device=DEV)
    route = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    jpeg.launch_build_index_chunked(index.streams, index.frames, index.htabs, index.nq, index.nh, n, index.seg_mcus, index.entry_off,
                                    entries, index.n_entries, 64, 16, ws, status, route)
    torch.cuda.synchronize()
    assert _guards_ok(whole_w, short)
    assert status.tolist() == want_status.tolist() and route[n - 3:].tolist() == [0, 0, 0] and (route[:n - 3] > 0).sum() > 20
    got = np.frombuffer(entries.cpu().numpy().tobytes(), dtype=jpeg.ENTRY_DTYPE)
    eo = res.entry_off.numpy()
    assert got[eo[n - 3]:].tobytes() == want_entries[eo[n - 3]:].tobytes()


def test_bad_arguments_return_codes_without_a_launch(chain):
    import ctypes

    from rubiksnet_amd import _native
    L, one = _native.lib(), ctypes.c_void_p(64)
    def build(n=1, entries=one, S=256, rounds=24, ws=one, ws_bytes=1 << 20, route=one):
        return L.rk_jpeg_build_index_chunked(one, 10, one, one, 1, 1, n, one, one, entries, 4, S, rounds, ws, ws_bytes, one, route,
                                             None)
    assert build(entries=None) == -1 and build(route=None) == -1 and build(n=0) == -2 and build(n=65536) == -2
    assert build(S=48) == -2 and build(S=1024) == -2 and build(rounds=-1) == -2 and build(rounds=65) == -2
    assert build(ws=None) == -4 and build(ws=ctypes.c_void_p(72)) == -4 and build(n=3, ws_bytes=31) == -4
    torch.cuda.synchronize()
    _, _, index, _, _, _ = chain
    with pytest.raises(ValueError, match="route must be a contiguous"):
        jpeg.launch_build_index_chunked(index.streams, index.frames, index.htabs, index.nq, index.nh, index.n, index.seg_mcus,
                                        index.entry_off, index.entries, index.n_entries, 256, 24,
                                        torch.empty(64, dtype=torch.uint8, device=DEV), index.status,
                                        torch.zeros(index.n, dtype=torch.int64, device=DEV))


def test_build_index_chunked_then_the_indexed_decode_gives_the_committed_rgb():
    _, res = ic.resident()
    index = jpeg.build_index(res, DEV, method="chunked")
    (frames, _, _, _), _ = jpeg.sections(res.blob, res.layout)
    rec = np.frombuffer(frames.numpy().tobytes(), dtype=jpeg.FRAME_DTYPE)
    n = len(ic.GOOD)
    assert index.status[:n].tolist() == [0] * n and int(index.status[-1]) == len(jc.CORRUPT)
    route = index.route.tolist()
    assert all((route[i] > 0) == (int(rec["restart_interval"][i]) == 0) for i in range(n)) and not any(route[n:])
    pick = list(range(n))
    off, _ = ic.rgb_table(res)
    rgb_bytes = int(off[n])
    most = max(int(res.segments[p]) for p in pick)
    ws_bytes = jpeg.indexed_workspace_bytes_for(rec, pick, most)
    whole_rgb, arena = _guarded(rgb_bytes)
    whole_ws, ws = _guarded(ws_bytes)
    status = torch.full((n + 3,), -77, dtype=torch.int32, device=DEV)
    jpeg.launch_decode_indexed(index, torch.tensor(pick, dtype=torch.int32, device=DEV),
                               torch.tensor(off[:n], dtype=torch.int64, device=DEV), most, arena, ws, status[:n + 1])
    torch.cuda.synchronize()
    assert _guards_ok(whole_rgb, rgb_bytes) and _guards_ok(whole_ws, ws_bytes)
    assert status.tolist() == [0] * (n + 1) + [-77, -77]
    out = arena.cpu().numpy()
    for p, (name, E) in enumerate(ic.GOOD):
        want = jc.rgb(name)
        assert np.array_equal(out[off[p]:off[p] + want.size].reshape(want.shape), want), (name, E)


# ------------------------------------------------------------------------------------------------- a streamed batch by rows
def test_decode_jpeg_frames_by_rows_equals_the_chain():
    """Clips, a grayscale frame, frames with restart markers, a corrupt frame (a zero frame with the same code) and a
    progressive frame that the host decodes."""
    pytest.importorskip("PIL")
    samples = [([jc.jpg("clip0"), jc.jpg("clip1"), jc.jpg("clip2")], 1), ([jc.jpg("p17x23_gray")], 2),
               ([jc.jpg("p17x23_420"), jc.jpg("corrupt_cut50"), jc.jpg("corrupt_flip02")], 3),
               ([jc.jpg("flat_420"), jc.jpg("unsupported_progressive")], 4), ([jc.jpg("rst1_64x48_420")], 5),
               ([jc.jpg("noise_q100_444")], 6)]
    packed = jpeg.pack_jpeg_clips(samples)
    assert len(packed.fallback) == 1
    want_rgb, want_clips, want_status = jpeg.decode_jpeg_frames(packed, DEV, entropy="chain")
    for chunk_bytes, max_rounds in ((256, 24), (16, 8), (64, 0)):
        out = torch.full((packed.rgb_bytes + 64,), 0x5E, dtype=torch.uint8, device=DEV)
        rgb, clips, status = jpeg.decode_jpeg_frames(packed, DEV, out=out, entropy="rows", chunk_bytes=chunk_bytes,
                                                     max_rounds=max_rounds)
        torch.cuda.synchronize()
        assert torch.equal(rgb, want_rgb) and torch.equal(clips, want_clips) and (out[packed.rgb_bytes:] == 0x5E).all()
        assert status.tolist() == want_status.tolist()
    assert want_status.tolist()[:3] == [0, 0, 0] and want_status[-1] == 2 and want_status[5] != 0 != want_status[6]
    with pytest.raises(ValueError, match="workspace holds 16 bytes"):
        jpeg.decode_jpeg_frames(packed, DEV, workspace=torch.empty(16, dtype=torch.uint8, device=DEV), entropy="rows")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """tests/test_jpeg_index_gpu.py's folder: six Pillow-written videos of 6-10 frames, four at 48x64 and two at 40x56
    (smooth pictures: small files), and a list file; one frame is progressive, so the host decodes it."""
    pytest.importorskip("PIL")
    from PIL import Image
    root = tmp_path_factory.mktemp("jpeg_rows")
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


def _dataset(folder, split, decode):
    return dataset.RubiksDataset(folder, os.path.join(folder, "list.txt"), num_segments=4, random_shift=split == "train",
                                 test_mode=split == "test", twice_sample=split == "test", only_even_indices=False, decode=decode)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_loader_by_rows_equals_the_chain(folder, dtype):
    """Two epochs, equal seeds: clips and labels of entropy="rows" are bit-equal to entropy="chain"."""
    def run(entropy, **kw):
        loader = dataset.FrameLoader(_dataset(folder, "train", "device"), 4, "train", device=DEV, dtype=dtype, size=32, seed=5,
                                     decode="device", entropy=entropy, **kw)
        torch.manual_seed(11)                               # the dataset draws from torch's global generator
        got = [(clips.clone(), labels.clone()) for _ in range(2) for clips, labels in loader]
        torch.cuda.synchronize()
        return got, loader

    want, plain = run("chain")
    got, loader = run("rows")
    assert len(want) == len(got) == 4
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    for (wc, wl), (gc, gl) in zip(want, got):
        assert gc.shape == wc.shape == (wl.numel(), 4, 3, 32, 32) and gc.dtype == dtype
        assert torch.equal(wc.view(bits), gc.view(bits)) and torch.equal(wl, gl)
    assert loader.decode_errors() == plain.decode_errors() == 0 and loader.fallback_frames == plain.fallback_frames
    assert loader.chain_frames() == 0 and plain.chain_frames() == 0
    none, forced = run("rows", max_rounds=0)                # every frame down the chain: the same clips, and counted
    assert all(torch.equal(a.view(bits), b.view(bits)) for (a, _), (b, _) in zip(want, none))
    assert forced.chain_frames() == 2 * 6 * 4 - forced.fallback_frames


def test_the_cache_with_the_chunked_build_equals_the_chain(folder):
    def run(index_build):
        cache = dataset.DeviceFrameCache(_dataset(folder, "val", "device"), 4, "val", device=DEV, size=32, seed=5, resident="jpeg",
                                         index_build=index_build)
        got = [(clips.clone(), labels.clone()) for _ in range(2) for clips, labels in cache]
        torch.cuda.synchronize()
        return got, cache

    want, plain = run("chain")
    got, cache = run("chunked")
    assert len(want) == len(got) == 4 and plain.index.route is None
    for (wc, wl), (gc, gl) in zip(want, got):
        assert torch.equal(wc.view(torch.int32), gc.view(torch.int32)) and torch.equal(wl, gl)
    assert torch.equal(cache.index.status, plain.index.status) and torch.equal(cache.index.entries, plain.index.entries)
    assert (cache.index.route > 0).all() and cache.decode_errors() == 0 and cache.fallback_frames == 1


# ------------------------------------------------------------------------------------------------- capture
def test_build_and_decode_are_capturable_as_one_chain():
    names = ["clip3", "p17x23_gray", "rst2_40x24_444", "corrupt_cut25", "p33x17_422"]
    packed = jpeg.pack_jpeg_clips([([jc.jpg(x)], 0) for x in names])
    eager, _, eager_status = jpeg.decode_jpeg_frames(packed, DEV, entropy="rows", chunk_bytes=64, max_rounds=16)
    torch.cuda.synchronize()
    (frames, htabs, qtabs, streams), (n, nh, nq) = jpeg.sections(packed.blob.to(DEV), packed.layout)
    (host_frames, _, _, _), _ = jpeg.sections(packed.blob, packed.layout)
    rows = jpeg.row_tables(np.frombuffer(host_frames.numpy().tobytes(), dtype=jpeg.FRAME_DTYPE), 64)
    tables = rows.tables.to(DEV)
    entries = torch.zeros(rows.n_entries * 2, dtype=torch.int64, device=DEV).view(torch.uint8)
    build_ws = torch.empty(rows.build_bytes, dtype=torch.uint8, device=DEV)
    decode_ws = torch.empty(rows.decode_bytes, dtype=torch.uint8, device=DEV)
    build_status = torch.full((n + 1,), -1, dtype=torch.int32, device=DEV)
    route = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    status = torch.full((n + 1,), -1, dtype=torch.int32, device=DEV)
    rgb = torch.full((packed.rgb_bytes,), 9, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):          # eleven launches on one stream: a linear chain, no branches
            jpeg.launch_decode_rows(streams, frames, qtabs, htabs, nq, nh, rows, tables, entries, build_ws, build_status, route, rgb,
                                    decode_ws, status, 64, 16)
    torch.cuda.current_stream(DEV).wait_stream(side)
    rgb.fill_(9)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(rgb, eager) and status.tolist() == eager_status.tolist()
    assert eager_status.tolist()[:3] == [0, 0, 0] and eager_status[3] != 0 and eager_status[-1] == 1
    assert route.tolist()[2:4] == [0, 0] and route[0] > 0 and route[1] > 0 and route[4] > 0
