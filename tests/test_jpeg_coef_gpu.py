"""Resident frames as packed DCT coefficients on the device (rk_jpeg_coef_sizes, rk_jpeg_coef_pack,
rk_jpeg_decode_coef_u8) and DeviceFrameCache(resident="coef") on them: the device's blob against the host program's byte for
byte, every case bit-equal to Pillow inside guard bands, scattered picks, the corrupted corpus, tampered regions (after the
host program has passed on the same table), the cache against resident="rgb" and "jpeg", the budget, graph capture.  Tiny
images throughout."""
import io
import os

import numpy as np
import pytest
import torch

import _jpeg_cases as jc
import _jpeg_coef_cases as cc
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
    run = cc.host_run()
    if run is None:
        pytest.skip("no host C++ compiler")
    return run


@pytest.fixture(scope="module")
def built():
    """The shared set transcoded once per method, in slabs of 7 frames (several slabs, the last one short).
    -> (names, ResidentJpeg, {method: DeviceCoef}, host copy of the records)."""
    pytest.importorskip("PIL")
    names, res = cc.resident()
    coefs = {method: jpeg.build_coef(res, DEV, method=method, slab_frames=7) for method in ("chain", "chunked")}
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
def test_the_devices_blob_and_offsets_are_the_host_programs(built, host, method):
    names, res, coefs, rec = built
    coef = coefs[method]
    n = len(cc.GOOD)
    status = coef.status.cpu().numpy()
    assert status[:len(names)].tolist() == host["code"].tolist() and status[-1] == len(jc.CORRUPT)
    assert status[:n].tolist() == [0] * n
    assert coef.region_off.cpu().numpy().tolist() == host["region_off"].tolist()
    assert coef.packed_bytes == len(host["blob"]) <= coef.blob.numel()      # the blob was sized from the first slab: with some to spare
    assert np.array_equal(coef.blob.cpu().numpy()[:coef.packed_bytes], host["blob"])
    assert coef.file_bytes == int(rec["stream_len"].sum()) and coef.build_bytes > 0


def test_the_slab_size_does_not_change_the_blob(built):
    names, res, coefs, rec = built
    whole = jpeg.build_coef(res, DEV, slab_frames=256)      # one slab: the blob is exactly its bytes
    k = whole.packed_bytes
    assert k == coefs["chain"].packed_bytes and whole.blob.numel() == (k + 15) // 16 * 16
    assert torch.equal(whole.blob[:k], coefs["chain"].blob[:k]) and torch.equal(whole.region_off, coefs["chain"].region_off)
    assert torch.equal(whole.status, coefs["chain"].status)
    # slabs of one frame: the larger frames further on outgrow what the first, small one let expect, and the blob grows
    ones = jpeg.build_coef(res, DEV, slab_frames=1)
    assert torch.equal(ones.blob[:k], whole.blob[:k]) and torch.equal(ones.region_off, whole.region_off)


def test_a_build_over_its_budget_stops_before_the_next_allocation(built):
    names, res, coefs, rec = built
    asked = []

    def admit(held):
        asked.append(held)
        if len(asked) == 4:
            raise RuntimeError("enough")

    with pytest.raises(RuntimeError, match="enough"):
        jpeg.build_coef(res, DEV, slab_frames=7, admit=admit)
    assert len(asked) == 4 and min(asked) > 0               # the tables; slab 0 and its part; slab 1 -- and no further


# ------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("name", cc.GOOD)
def test_every_case_is_bit_equal_to_pillow_inside_guards(built, name):
    names, res, coefs, rec = built
    p = names.index(name)
    want = cc.want_rgb(name)
    for method in ("chain", "chunked"):
        out, status = _decode_guarded(coefs[method], rec, [p], [0], _bytes_of(rec, p))
        assert status.tolist() == [0, 0], (name, method, status.tolist())
        got = out.reshape(want.shape)
        assert np.array_equal(got, want), (name, method, int((got != want).sum()))


def test_all_cases_in_one_launch(built):
    names, res, coefs, rec = built
    pick = list(range(len(cc.GOOD)))
    off, _ = cc.rgb_table(res)
    total = int(off[len(pick)])
    out, status = _decode_guarded(coefs["chain"], rec, pick, off[:len(pick)].tolist(), total)
    assert status.tolist() == [0] * (len(pick) + 1)
    for p, name in enumerate(cc.GOOD):
        want = cc.want_rgb(name)
        assert np.array_equal(out[off[p]:off[p] + want.size].reshape(want.shape), want), name


# ------------------------------------------------------------------------------------------------- picks
def test_scattered_picks_equal_the_single_frames_and_leave_the_gaps_alone(built):
    names, res, coefs, rec = built
    coef = coefs["chunked"]
    pick = [names.index(x) for x in ("rst2_40x24_444", "p17x23_420", "p17x23_420", cc.NOISE)]
    sizes = [_bytes_of(rec, p) for p in pick]
    offs = [12000, 11, 16000, 1500]
    spans = sorted(zip(offs, sizes))
    assert all(a + k <= b for (a, k), (b, _) in zip(spans, spans[1:]))
    total = 17500
    out, status = _decode_guarded(coef, rec, pick, offs, total, fill=0x5E)
    assert status.tolist() == [0, 0, 0, 0, 0]
    mask = np.ones(total, dtype=bool)
    for p, off, k in zip(pick, offs, sizes):
        single, st = _decode_guarded(coef, rec, [p], [0], k)
        assert st.tolist() == [0, 0] and np.array_equal(out[off:off + k], single)
        want = cc.want_rgb(names[p])
        assert np.array_equal(single.reshape(want.shape), want)
        mask[off:off + k] = False
    assert (out[mask] == 0x5E).all()


# ------------------------------------------------------------------------------------------------- the corrupted corpus
def test_the_corrupted_corpus_gives_zero_frames_with_the_plain_decoders_codes(built):
    names, res, coefs, rec = built
    first = len(cc.GOOD)
    packed = jpeg.pack_jpeg_clips([([jc.jpg(x)], 0) for x in jc.CORRUPT])
    _, _, plain = jpeg.decode_jpeg_frames(packed, DEV)
    plain = plain.cpu().numpy()
    assert names[first:] == list(jc.CORRUPT) and plain[-1] == len(jc.CORRUPT) and (plain[:-1] != 0).all()
    good = names.index("p17x23_420")
    k = 17 * 23 * 3
    for method in ("chain", "chunked"):
        assert coefs[method].status.cpu().numpy()[first:first + len(jc.CORRUPT)].tolist() == plain[:-1].tolist()
        pick, offs = [good], [0]
        for j in range(len(jc.CORRUPT)):                    # good, bad, good, bad, ..., good
            pick += [first + j, good]
            offs += [offs[-1] + k, offs[-1] + 2 * k]
        out, st = _decode_guarded(coefs[method], rec, pick, offs, offs[-1] + k)
        assert st[:-1].tolist() == [0] + [c for code in plain[:-1].tolist() for c in (code, 0)] and st[-1] == len(jc.CORRUPT)
        frames = out.reshape(len(pick), 23, 17, 3)
        assert all(np.array_equal(f, jc.rgb("p17x23_420")) for f in frames[0::2]) and not frames[1::2].any()


def test_picks_and_records_that_do_not_fit(built):
    """A pick outside the set, an output range past the arena: a code each, zeros where the range is valid, nothing
    written where it is not, the good neighbour untouched by any of it."""
    names, res, coefs, rec = built
    coef = coefs["chain"]
    good = names.index("p17x23_420")
    k = 17 * 23 * 3
    out, st = _decode_guarded(coef, rec, [good, coef.n, -1, good, good], [0, k, k, 3 * k + 1, 2 * k], 4 * k)
    assert st.tolist() == [0, 1, 1, 1, 0, 3]
    frames = out.reshape(4, 23, 17, 3)
    assert np.array_equal(frames[0], jc.rgb("p17x23_420")) and np.array_equal(frames[2], jc.rgb("p17x23_420"))
    assert (frames[1] == SENTINEL).all() and (frames[3] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------- tampered regions
@pytest.fixture(scope="module")
def host_codes(host):
    """The host program's verdict on cc.tampers(); the device test below runs only after it passed, under the sanitizers, on
    the same table."""
    for (i, k, b), (code, same, _, _, _) in zip(cc.tampers(), host["tampered"]):
        assert code != 0 or same == 1, (cc.NAMES[i], cc.KINDS[k], b)
    return [code for code, _, _, _, _ in host["tampered"]]


def test_tampered_regions_get_the_host_programs_codes_and_a_zero_frame(built, host, host_codes):
    """Bounded refusal: a region that was changed fails a check that reads nothing outside it.  Every tampered copy -- the
    host program's own bytes -- is appended to the blob as the region of a record of its own, and all are decoded in ONE
    launch, an untouched frame in front and behind."""
    names, res, coefs, rec = built
    coef = coefs["chain"]
    rows = cc.tampers()
    n = coef.n
    parts, region_off, at = [coef.blob.cpu().numpy()[:coef.packed_bytes]], coef.region_off.cpu().numpy()[:n].tolist(), coef.packed_bytes
    total = at + sum(len(blob) + (len(blob) & 1) for _, _, _, _, blob in host["tampered"])
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
    good = names.index("p33x17_422")
    pick = [good] + [n + 2 * t for t in range(len(rows))] + [good]
    sizes = [_bytes_of(all_rec, p) for p in pick]
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    out, st = _decode_guarded(tampered, all_rec, pick, offs[:-1], offs[-1])
    assert st[0] == st[len(pick) - 1] == 0
    for p in (0, len(pick) - 1):
        assert np.array_equal(out[offs[p]:offs[p + 1]].reshape(17, 33, 3), jc.rgb("p33x17_422"))
    assert st[1:-2].tolist() == host_codes
    assert st[-1] == sum(c != 0 for c in host_codes) == len(rows)
    assert not out[offs[1]:offs[-2]].any()


# ------------------------------------------------------------------------------------------------- the cache
SIZES = ((48, 64), (40, 56), (33, 47))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """Three Pillow-written videos of 6 frames at 48x64, 40x56 and 33x47 (smooth pictures: small files), and a list file;
    one frame is progressive, so the host decodes it."""
    pytest.importorskip("PIL")
    from PIL import Image
    root = tmp_path_factory.mktemp("jpeg_coef_cache")
    rng = np.random.default_rng(23)
    yy, xx = np.mgrid[0:48, 0:64]
    lines = []
    for v, (h, w) in enumerate(SIZES):
        os.makedirs(root / ("v%d" % v))
        for k in range(6):
            a, b, c = rng.uniform(0.5, 3.0, 3)
            pic = np.stack([127 + 120 * np.sin(xx / (4 * a) + k) * np.cos(yy / (5 * b)), 2 * xx + 3 * yy + 9 * k,
                            127 + 100 * np.cos((xx + yy) / (6 * c) - k)], axis=-1)[:h, :w]
            pic = np.clip(pic + rng.normal(0, 2, pic.shape), 0, 255).astype(np.uint8)
            buf = io.BytesIO()
            Image.fromarray(pic).save(buf, "JPEG", quality=85, progressive=(v, k) == (1, 3))
            with open(root / ("v%d" % v) / ("img_%05d.jpg" % (k + 1)), "wb") as fh:
                fh.write(buf.getvalue())
        lines.append("v%d 6 %d\n" % (v, v))
    with open(root / "list.txt", "w") as fh:
        fh.writelines(lines)
    return str(root)


def _dataset(folder, split, decode, **kw):
    return dataset.RubiksDataset(folder, os.path.join(folder, "list.txt"), num_segments=4, random_shift=split == "train",
                                 test_mode=split == "test", twice_sample=split == "test", only_even_indices=False,
                                 decode=decode, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("split", ["train", "val", "test"])
def test_the_coef_cache_equals_the_rgb_and_the_jpeg_cache(folder, split, dtype):
    """Two epochs, equal seeds: clips and labels of resident="coef" are bit-equal to resident="rgb" and "jpeg"."""
    def run(resident, **kw):
        ds = _dataset(folder, split, "host" if resident == "rgb" else "device")
        cache = dataset.DeviceFrameCache(ds, 2, split, device=DEV, dtype=dtype, size=32, seed=5, resident=resident, **kw)
        got = [(clips.clone(), labels.clone()) for _ in range(2) for clips, labels in cache]
        torch.cuda.synchronize()
        return got, cache

    rgb, _ = run("rgb")
    jpg, _ = run("jpeg")
    coef, cache = run("coef", slab_frames=5, index_build="chunked" if split == "val" else "chain")
    assert len(rgb) == len(jpg) == len(coef) == 4
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    for (rc, rl), (jc_, jl), (cc_, cl) in zip(rgb, jpg, coef):
        assert rc.shape == cc_.shape == (rl.numel() * (2 if split == "test" else 1), 4, 3, 32, 32) and cc_.dtype == dtype
        assert torch.equal(rc.view(bits), cc_.view(bits)) and torch.equal(jc_.view(bits), cc_.view(bits))
        assert torch.equal(rl, cl) and torch.equal(jl, cl)
    assert cache.fallback_frames == 1 and cache.decode_errors() == 0


def test_a_budget_between_the_coef_and_the_rgb_footprint(folder):
    decoded = sum(6 * h * w * 3 for h, w in SIZES)
    probe = dataset.DeviceFrameCache(_dataset(folder, "val", "device"), 1, "val", device=DEV, size=32, resident="coef", slab_frames=4)
    for _ in probe:
        pass
    need = max(probe.resident_bytes, probe.build_peak_bytes)     # with the batch buffers; with a slab's buffers
    print("decoded %d, coef resident %d (packed %d, files %d), the build's peak %d" % (
        decoded, probe.resident_bytes, probe.coef.packed_bytes, probe.coef.file_bytes, probe.build_peak_bytes))
    assert need < decoded
    budget = (need + decoded) // 2
    with pytest.raises(RuntimeError, match="over the budget"):
        dataset.DeviceFrameCache(_dataset(folder, "val", "host"), 1, "val", device=DEV, size=32, budget_bytes=budget)
    cache = dataset.DeviceFrameCache(_dataset(folder, "val", "device"), 1, "val", device=DEV, size=32, budget_bytes=budget,
                                     resident="coef", slab_frames=4)
    assert sum(labels.numel() for _, labels in cache) == 3 and cache.resident_bytes <= budget
    for short in (probe.build_peak_bytes - 1, probe.coef.packed_bytes):     # the last allocation of the build; the first slab
        with pytest.raises(RuntimeError, match="over the budget"):
            dataset.DeviceFrameCache(_dataset(folder, "val", "device"), 1, "val", device=DEV, size=32, resident="coef",
                                     slab_frames=4, budget_bytes=short)
    tight = dataset.DeviceFrameCache(_dataset(folder, "val", "device"), 1, "val", device=DEV, size=32, resident="coef",
                                     slab_frames=4, budget_bytes=max(probe.build_peak_bytes, probe._fixed_bytes + 100))
    if probe.build_peak_bytes <= probe._fixed_bytes + 100:
        with pytest.raises(RuntimeError, match="over the budget"):      # built, but no room for a batch's buffers
            next(iter(tight))


# ------------------------------------------------------------------------------------------------- capture
def test_the_coef_decode_is_capturable_as_one_chain(built):
    names, res, coefs, rec = built
    coef = coefs["chain"]
    pick = [names.index(x) for x in ("p17x23_420", "rst1_64x48_420", "p17x23_gray")]
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
    assert np.array_equal(rgb.cpu().numpy(), eager) and status.cpu().numpy().tolist() == eager_status.tolist() == [0, 0, 0, 0]
