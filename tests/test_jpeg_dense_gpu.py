"""The dense record format of the packed DCT coefficients on the device (rk_jpeg_coef_sizes_as, rk_jpeg_coef_pack_as,
rk_jpeg_decode_coef_as_u8 with RK_JPEG_COEF_DENSE) and DeviceFrameCache(resident="coef", coef_record="dense") on it: the
device's blob against the host program's byte for byte for both entropy stages, decodes inside guard bands against the
fixtures, the host program's own tampered regions, graph capture, and the cache against resident="rgb" and the wide
records.  Tiny images throughout: the largest frame is 96 x 80."""
import os

import numpy as np
import pytest
import torch

import _jpeg_cases as jc
import _jpeg_dense_cases as dc
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
def host():
    pytest.importorskip("PIL")
    run = dc.host_run()
    if run is None:
        pytest.skip("no host C++ compiler")
    return run


@pytest.fixture(scope="module")
def built():
    """The shared set transcoded once per entropy stage, in slabs of 7 frames (several slabs, the last one short).
    -> (names, ResidentJpeg, {method: DeviceCoef}, host copy of the records)."""
    pytest.importorskip("PIL")
    names, res = dc.resident()
    coefs = {method: jpeg.build_coef(res, DEV, method=method, slab_frames=7, record="dense") for method in ("chain", "chunked")}
    torch.cuda.synchronize()
    rec = jpeg.records(res.blob, res.layout).copy()
    return names, res, coefs, rec


def _decode_guarded(coef, rec, pick, rgb_off, rgb_bytes, fill=SENTINEL):
    """One launch: the RGB arena and a workspace of exactly the bytes asked for inside 4 KB guard bands of a sentinel
    byte.  -> (rgb, status) on the host after checking every guard."""
    m = len(pick)
    ws_bytes = jpeg.coef_workspace_bytes_for(rec, pick)
    arena = torch.full((rgb_bytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    arena[GUARD:GUARD + rgb_bytes] = fill
    ws = torch.full((ws_bytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    status = torch.full((m + 1 + 2,), -77, dtype=torch.int32, device=DEV)
    jpeg.launch_decode_coef(coef, torch.tensor(pick, dtype=torch.int32, device=DEV),
                            torch.tensor(rgb_off, dtype=torch.int64, device=DEV), arena[GUARD:GUARD + rgb_bytes],
                            ws[GUARD:GUARD + ws_bytes], status[:m + 1])
    torch.cuda.synchronize()
    arena, ws, status = arena.cpu().numpy(), ws.cpu().numpy(), status.cpu().numpy()
    for name, t, k in (("rgb", arena, rgb_bytes), ("workspace", ws, ws_bytes)):
        assert (t[:GUARD] == SENTINEL).all() and (t[GUARD + k:] == SENTINEL).all(), name + " guard touched"
    assert status[m + 1:].tolist() == [-77, -77]
    return arena[GUARD:GUARD + rgb_bytes], status[:m + 1]


def _bytes_of(rec, p):
    return int(rec["width"][p]) * int(rec["height"][p]) * 3


# ------------------------------------------------------------------------------------------------- the build
@pytest.mark.parametrize("method", ["chain", "chunked"])
def test_the_devices_dense_blob_is_the_host_programs(built, host, method):
    names, res, coefs, rec = built
    coef = coefs[method]
    n = len(dc.GOOD)
    status = coef.status.cpu().numpy()
    assert coef.record == "dense"
    assert status[:len(names)].tolist() == host["code"].tolist() and status[-1] == len(jc.CORRUPT)
    assert status[:n].tolist() == [0] * n
    assert coef.region_off.cpu().numpy().tolist() == host["region_off"].tolist()
    assert coef.packed_bytes == len(host["blob"]) <= coef.blob.numel()
    got = coef.blob.cpu().numpy()[:coef.packed_bytes]
    assert np.array_equal(got, host["blob"]), int(np.flatnonzero(got != host["blob"])[0])


# ------------------------------------------------------------------------------------------------- decodes
def test_all_cases_in_one_launch_equal_the_fixtures(built):
    names, res, coefs, rec = built
    pick = list(range(len(dc.GOOD)))
    off, _ = dc.cc.rgb_table(res)
    total = int(off[len(pick)])
    for method in ("chain", "chunked"):
        out, status = _decode_guarded(coefs[method], rec, pick, off[:len(pick)].tolist(), total)
        assert status.tolist() == [0] * (len(pick) + 1), (method, status.tolist())
        for p, name in enumerate(dc.GOOD):
            want = dc.want_rgb(name)
            got = out[off[p]:off[p] + want.size].reshape(want.shape)
            assert np.array_equal(got, want), (name, method, int((got != want).sum()))


def test_duplicate_and_out_of_range_picks_and_a_frame_with_a_build_code(built):
    """Scattered output places with gaps, a frame twice, a pick outside the set, an output range past the arena, a frame
    the build refused: a code each, zeros where the range is valid, nothing written where it is not, the gaps and the
    good neighbours untouched."""
    names, res, coefs, rec = built
    coef = coefs["chunked"]
    wave, small, step = names.index(dc.WAVE), names.index("p17x23_420"), names.index(dc.STEP)
    refused = len(dc.GOOD)                                  # the first frame of the corrupted corpus, 17 x 23
    build_code = int(coef.status[refused].item())
    assert build_code != 0
    kw, ks, kt = _bytes_of(rec, wave), _bytes_of(rec, small), _bytes_of(rec, step)
    assert ks == _bytes_of(rec, refused)
    #        wave         small   small (again)  outside  outside  past the arena  refused        step
    pick = [wave, small, small, coef.n, -1, small, refused, step]
    offs = [11, 25000, 27000, 29000, 29000, 40000 - ks + 1, 31000, 33000]
    total = 40000
    assert 11 + kw <= 25000 and 33000 + kt <= 40000 - ks
    out, st = _decode_guarded(coef, rec, pick, offs, total, fill=0x5E)
    assert st.tolist() == [0, 0, 0, 1, 1, 1, build_code, 0, 4]
    mask = np.ones(total, dtype=bool)
    for j, (p, k) in enumerate(((wave, kw), (small, ks), (small, ks), (None, 0), (None, 0), (None, 0), (refused, ks), (step, kt))):
        got = out[offs[j]:offs[j] + k]
        mask[offs[j]:offs[j] + k] = False
        if p == refused:
            assert not got.any()
        elif p is not None:
            want = dc.want_rgb(names[p])
            assert np.array_equal(got.reshape(want.shape), want), names[p]
    assert (out[mask] == 0x5E).all()


# ------------------------------------------------------------------------------------------------- tampered regions
def test_the_host_programs_tampered_regions_get_code_8_and_a_zero_frame(built, host):
    """Bounded refusal: every tampered copy -- the host program's own bytes, which it refused under the sanitizers -- is
    appended to the blob as the region of a record of its own, and all are decoded in ONE launch, an untouched frame in
    front and behind."""
    names, res, coefs, rec = built
    coef = coefs["chain"]
    rows = host["tampers"].tolist()
    assert len(rows) == len(host["tampered"]) and all(code == 8 for code, _, _, _, _ in host["tampered"])
    n = coef.n
    parts, region_off, at = [coef.blob.cpu().numpy()[:coef.packed_bytes]], coef.region_off.cpu().numpy()[:n].tolist(), coef.packed_bytes
    total = at + sum(len(blob) for _, _, _, _, blob in host["tampered"])
    extra_rec = []
    for (i, kind, b), (_, _, lo, hi, blob) in zip(rows, host["tampered"]):
        # records n + 2 t and n + 2 t + 1: the first one's region is [lo, hi) of its copy (past the whole blob where the
        # host program put it past its own), the second is never picked and only ends the first
        past = hi > len(blob)
        region_off += [(total if past else at) + lo, (total if past else at) + hi]
        extra_rec += [rec[i], rec[i]]
        parts.append(blob)
        at += len(blob)
        assert at % 2 == 0
    region_off.append(at)
    all_rec = np.concatenate([rec, np.stack(extra_rec)])
    tampered = coef._replace(
        blob=torch.from_numpy(np.concatenate(parts)).to(DEV), packed_bytes=at, n=len(all_rec),
        frames=torch.from_numpy(all_rec.view(np.uint8).reshape(-1).copy()).to(DEV),
        region_off=torch.tensor(region_off, dtype=torch.int64, device=DEV),
        status=torch.cat([coef.status[:n], torch.zeros(2 * len(rows) + 1, dtype=torch.int32, device=DEV)]))
    assert tampered.record == "dense"
    good = names.index("p33x17_422")
    pick = [good] + [n + 2 * t for t in range(len(rows))] + [good]
    sizes = [_bytes_of(all_rec, p) for p in pick]
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    out, st = _decode_guarded(tampered, all_rec, pick, offs[:-1], offs[-1])
    assert st[0] == st[len(pick) - 1] == 0
    for p in (0, len(pick) - 1):
        assert np.array_equal(out[offs[p]:offs[p + 1]].reshape(17, 33, 3), jc.rgb("p33x17_422"))
    assert st[1:-2].tolist() == [8] * len(rows), [(dc.NAMES[i], dc.KINDS[k], b) for (i, k, b), c in zip(rows, st[1:-2]) if c != 8]
    assert st[-1] == len(rows)
    assert not out[offs[1]:offs[-2]].any()


# ------------------------------------------------------------------------------------------------- capture
def test_the_dense_decode_is_capturable_as_one_chain(built):
    names, res, coefs, rec = built
    coef = coefs["chain"]
    pick = [names.index(x) for x in ("p17x23_420", dc.WAVE, "p17x23_gray", dc.STEP)]
    sizes = [_bytes_of(rec, p) for p in pick]
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    eager, eager_status = _decode_guarded(coef, rec, pick, offs[:-1], offs[-1])
    pick_d = torch.tensor(pick, dtype=torch.int32, device=DEV)
    off_d = torch.tensor(offs[:-1], dtype=torch.int64, device=DEV)
    rgb = torch.full((offs[-1],), 9, dtype=torch.uint8, device=DEV)
    ws = torch.empty(jpeg.coef_workspace_bytes_for(rec, pick), dtype=torch.uint8, device=DEV)
    status = torch.full((len(pick) + 1,), -1, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):          # six launches on one stream: a linear chain, no branches
            jpeg.launch_decode_coef(coef, pick_d, off_d, rgb, ws, status)
    torch.cuda.current_stream(DEV).wait_stream(side)
    rgb.fill_(9)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(rgb.cpu().numpy(), eager) and status.cpu().numpy().tolist() == eager_status.tolist() == [0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------- the cache
CACHED = ("rst1_48x48_420", "rst1_64x48_420", "wave96x80", "rst2_40x24_444")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """Four videos of 5 frames, each the same fixture frame five times (a video's frames share a size), and a list file."""
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("jpeg_dense_cache")
    lines = []
    for v, name in enumerate(CACHED):
        os.makedirs(root / ("v%d" % v))
        for k in range(5):
            with open(root / ("v%d" % v) / ("img_%05d.jpg" % (k + 1)), "wb") as fh:
                fh.write(dc.jpg(name))
        lines.append("v%d 5 %d\n" % (v, v))
    with open(root / "list.txt", "w") as fh:
        fh.writelines(lines)
    return str(root)


def _dataset(folder, split, decode):
    return dataset.RubiksDataset(folder, os.path.join(folder, "list.txt"), num_segments=3, random_shift=split == "train",
                                 test_mode=split == "test", twice_sample=split == "test", only_even_indices=False, decode=decode)


@pytest.mark.parametrize("split", ["train", "val"])
def test_the_dense_cache_equals_the_rgb_and_the_wide_cache_and_is_smaller(folder, split):
    """Two epochs, equal seeds: clips and labels of coef_record="dense" are bit-equal to resident="rgb" and to the wide
    records; the dense set takes fewer bytes."""
    def run(resident, **kw):
        ds = _dataset(folder, split, "host" if resident == "rgb" else "device")
        cache = dataset.DeviceFrameCache(ds, 2, split, device=DEV, size=16, seed=5, resident=resident, **kw)
        got = [(clips.clone(), labels.clone()) for _ in range(2) for clips, labels in cache]
        torch.cuda.synchronize()
        return got, cache

    rgb, _ = run("rgb")
    wide, wide_cache = run("coef", slab_frames=6)
    dense, cache = run("coef", slab_frames=6, coef_record="dense", index_build="chunked" if split == "val" else "chain")
    assert len(rgb) == len(wide) == len(dense) == 4
    for (rc, rl), (wc, wl), (dc_, dl) in zip(rgb, wide, dense):
        assert dc_.shape == rc.shape == (rl.numel(), 3, 3, 16, 16)
        assert torch.equal(rc.view(torch.int32), dc_.view(torch.int32)) and torch.equal(wc.view(torch.int32), dc_.view(torch.int32))
        assert torch.equal(rl, dl) and torch.equal(wl, dl)
    assert cache.coef.record == "dense" and wide_cache.coef.record == "wide" and cache.coef_record == "dense"
    assert cache.fallback_frames == 0 and cache.decode_errors() == 0
    print("resident bytes: dense %d (packed %d), wide %d (packed %d)" % (cache.resident_bytes, cache.coef.packed_bytes,
                                                                         wide_cache.resident_bytes, wide_cache.coef.packed_bytes))
    assert cache.coef.packed_bytes < wide_cache.coef.packed_bytes and cache.resident_bytes < wide_cache.resident_bytes
