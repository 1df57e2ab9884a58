"""The device JPEG decode (rk_jpeg_decode_u8, rubiksnet_amd/jpeg.py) and FrameLoader(decode="device") on it: bit-equal
to the committed Pillow decodes inside guard bands, one mixed launch, the corrupted corpus (one launch, shared by the
tests that look at it), records that do not fit, the loader against the host-decoding loader, graph capture.  Tiny
images; the only larger ones are the eight 240x320 frames the loader test needs."""
import hashlib
import io
import os

import numpy as np
import pytest
import torch

import _jpeg_cases as jc
from rubiksnet_amd import dataset, jpeg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_GOOD = jc.SUPPORTED + jc.CLIP
GUARD, SENTINEL = 4096, 0xC3


def _launch_guarded(packed):
    """One launch of a packed batch: the RGB arena inside 4 KB guard bands of a sentinel byte, the stream arena at an
    odd byte offset, a workspace of exactly the bytes asked for (inside guards too).  Returns (rgb, status) on the host
    after checking every guard."""
    (frames, htabs, qtabs, streams), (n, nh, nq) = jpeg.sections(packed.blob, packed.layout)
    odd = torch.zeros(streams.numel() + 3, dtype=torch.uint8, device=DEV)
    odd[1:1 + streams.numel()].copy_(streams)
    stream_dev = odd[1:1 + streams.numel()]
    assert stream_dev.data_ptr() % 2 == 1
    arena = torch.full((packed.rgb_bytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    ws_bytes = (int(packed.workspace_bytes) + 15) & ~15
    ws = torch.full((ws_bytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    status = torch.full((n + 1 + 2,), -77, dtype=torch.int32, device=DEV)
    jpeg.launch_decode(stream_dev, frames.to(DEV), qtabs.to(DEV), htabs.to(DEV), n, arena[GUARD:GUARD + packed.rgb_bytes],
                       ws[GUARD:GUARD + ws_bytes], status[:n + 1], nq, nh)
    torch.cuda.synchronize()
    arena, ws, status = arena.cpu().numpy(), ws.cpu().numpy(), status.cpu().numpy()
    for name, t, m in (("rgb", arena, packed.rgb_bytes), ("workspace", ws, ws_bytes)):
        assert (t[:GUARD] == SENTINEL).all() and (t[GUARD + m:] == SENTINEL).all(), name + " guard touched"
    assert status[n + 1:].tolist() == [-77, -77]
    return arena[GUARD:GUARD + packed.rgb_bytes], status[:n + 1]


def _frames_of(packed, out):
    return [out[off:off + h * w * 3].reshape(h, w, 3) for off, h, w, _ in packed.clips.tolist()]


def _check_good(name, got):
    if name in jc.SUPPORTED:
        want = jc.rgb(name)
        assert got.shape == want.shape and np.array_equal(got, want), (name, int((got != want).sum()))
    else:
        assert hashlib.sha256(got.tobytes()).digest() == jc.clip_digest(jc.CLIP.index(name)), name


@pytest.mark.parametrize("name", ALL_GOOD)
def test_every_golden_decodes_bit_equal_inside_guards(name):
    packed = jpeg.pack_jpeg_clips([([jc.jpg(name)], 0)])
    assert len(packed.fallback) == 0 and int(packed.layout[0]) == 1      # decoded by the device, not by Pillow in disguise
    out, status = _launch_guarded(packed)
    assert status.tolist() == [0, 0]
    _check_good(name, _frames_of(packed, out)[0])


def test_a_mixed_batch_equals_the_single_frames():
    """Every golden in one launch: all samplings and sizes, shared and distinct tables."""
    packed = jpeg.pack_jpeg_clips([([jc.jpg(n)], 0) for n in ALL_GOOD])
    assert len(packed.fallback) == 0 and int(packed.layout[2]) > 3 and int(packed.layout[1]) >= 8
    out, status = _launch_guarded(packed)
    assert status.tolist() == [0] * (len(ALL_GOOD) + 1)
    for name, got in zip(ALL_GOOD, _frames_of(packed, out)):
        _check_good(name, got)


def test_decode_jpeg_frames_feeds_the_ragged_entry_and_places_host_decoded_frames():
    pytest.importorskip("PIL")
    from PIL import Image
    prog = jc.jpg("unsupported_progressive")
    packed = jpeg.pack_jpeg_clips([([jc.jpg("flat_420"), prog], 3), ([jc.jpg("p33x17_422")], 1)])
    rgb, clips, status = jpeg.decode_jpeg_frames(packed, DEV)
    assert status.tolist() == [0, 0, 0] and len(packed.fallback) == 1 and clips.tolist() == [[0, 16, 16, 2], [1536, 17, 33, 1]]
    frames = _frames_of(packed, rgb.cpu().numpy())
    assert np.array_equal(frames[0][:16], jc.rgb("flat_420")) and np.array_equal(frames[1], jc.rgb("p33x17_422"))
    with Image.open(io.BytesIO(prog)) as im:
        assert np.array_equal(rgb[768:1536].cpu().numpy().reshape(16, 16, 3), np.asarray(im.convert("RGB")))


# ------------------------------------------------------------------------------------------------- the corrupted corpus
@pytest.fixture(scope="module")
def corrupted():
    """ONE launch of the whole corrupted corpus and of the flips that stay valid, a good frame on either side of each; guards, the good
    neighbours and the count are checked here.  -> {name: (code, frame)} of the bad ones.  (tests/test_jpeg.py runs the
    same files through the same decode core on the host under AddressSanitizer.)"""
    good = jc.jpg("p17x23_420")
    names = ["good"] + [x for c in jc.CORRUPT + jc.ALTERED for x in (c, "good")]
    packed = jpeg.pack_jpeg_clips([([good if x == "good" else jc.jpg(x)], 0) for x in names])
    assert len(packed.fallback) == 0
    out, status = _launch_guarded(packed)
    rows = {}
    for x, code, got in zip(names, status.tolist(), _frames_of(packed, out)):
        if x == "good":
            assert code == 0 and np.array_equal(got, jc.rgb("p17x23_420"))
        else:
            rows[x] = (code, got)
    assert status[-1] == sum(code != 0 for code, _ in rows.values())
    print({x: jpeg.STATUS_NAMES[code] for x, (code, _) in rows.items()})
    return rows


def test_broken_files_give_zero_frames_and_a_status(corrupted):
    for x in jc.BROKEN:
        code, got = corrupted[x]
        assert code != 0 and not got.any(), (x, code)


def test_every_flipped_byte_is_refused(corrupted):
    """The 16 seeded single-byte flips whose stream T.81 does not allow: a zero frame and a non-zero status for each."""
    assert len(jc.FLIPS) == 16
    for x in jc.FLIPS:
        code, got = corrupted[x]
        assert code != 0 and not got.any(), (x, code)


def test_a_flipped_byte_is_never_decoded_silently_wrong(corrupted):
    """The flips that leave a valid baseline stream: accepted, and equal to what libjpeg makes of the same bytes wherever
    libjpeg is one reference (_jpeg_cases.pillow_rgb_where_defined)."""
    pytest.importorskip("PIL")
    compared = 0
    for x in jc.ALTERED:
        code, got = corrupted[x]
        assert code == 0 and got.any(), (x, code)
        want = jc.pillow_rgb_where_defined(jc.jpg(x))          # None: libjpeg's own paths differ on this file
        if want is not None:
            assert np.array_equal(got, want), x
            compared += 1
    assert compared >= 30, compared


def test_records_that_do_not_fit_give_zeros_and_a_status():
    base = jpeg.pack_jpeg_clips([([jc.jpg("p17x23_420")], 0) for _ in range(7)])
    (frames, _, _, streams), _ = jpeg.sections(base.blob, base.layout)
    rec = np.frombuffer(frames.numpy(), dtype=jpeg.FRAME_DTYPE)        # a view: the edits land in the blob
    rec["stream_len"][1] = streams.numel() - int(rec["stream_off"][1]) + 1      # offset + length > stream_bytes
    rec["rgb_off"][2] = base.rgb_bytes - 17 * 23 * 3 + 1                       # output past rgb_bytes
    rec["width"][3] = 0
    rec["width"][4] = 16385
    rec["ac"][5][2] = 4                                                        # a table that is not there
    out, status = _launch_guarded(base)
    assert status.tolist() == [0, 1, 1, 1, 1, 1, 0, 5]
    got = out.reshape(7, 23, 17, 3)
    assert np.array_equal(got[0], jc.rgb("p17x23_420")) and np.array_equal(got[6], jc.rgb("p17x23_420"))
    assert not got[1].any() and not got[5].any()            # their rgb range is valid: zeroed
    assert (got[2:5] == SENTINEL).all()                     # no valid range of their own: nothing written


# ------------------------------------------------------------------------------------------------- the loader
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """Three videos of different sizes (the 240x320 clip among them) and a list file; one frame is progressive."""
    pytest.importorskip("PIL")
    from PIL import Image
    root = tmp_path_factory.mktemp("jpeg_frames")
    rng = np.random.default_rng(3)

    def video(name, frames):
        os.makedirs(root / name)
        for i, data in enumerate(frames):
            with open(root / name / ("img_%05d.jpg" % (i + 1)), "wb") as fh:
                fh.write(data)

    def encoded(h, w, count, **kw):
        out = []
        for _ in range(count):
            buf = io.BytesIO()
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(buf, "JPEG", **kw)
            out.append(buf.getvalue())
        return out

    video("a", [jc.jpg(c) for c in jc.CLIP])
    video("b", encoded(40, 56, 6, quality=80, subsampling=1))
    mixed = encoded(33, 47, 7, quality=70, subsampling=0)
    mixed[2] = encoded(33, 47, 1, quality=70, progressive=True)[0]          # frame 3: the host decodes it
    video("c", mixed)
    with open(root / "list.txt", "w") as fh:
        fh.write("a 8 0\nb 6 1\nc 7 2\n")
    return str(root)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("split", ["train", "val"])
def test_frame_loader_device_decode_equals_host_decode(folder, split, dtype):
    """Same files, same seed: FrameLoader(decode="device") and the host-decoding FrameLoader yield the same bits."""
    def run(decode):
        ds = dataset.RubiksDataset(folder, os.path.join(folder, "list.txt"), num_segments=4, random_shift=split == "train",
                                   only_even_indices=False, generator=torch.Generator().manual_seed(11), decode=decode)
        loader = dataset.FrameLoader(ds, 2, split, device=DEV, dtype=dtype, size=32, num_workers=0, seed=5, shuffle=False,
                                     decode=decode)
        got = [(clips.clone(), labels.clone()) for clips, labels in loader]
        torch.cuda.synchronize()
        return got, loader

    host, _ = run("host")
    dev, loader = run("device")
    assert len(host) == len(dev) == 2
    for (hc, hl), (dc, dl) in zip(host, dev):
        assert hc.shape == dc.shape and hc.dtype == dc.dtype == dtype
        assert torch.equal(hc.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                           dc.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
        assert torch.equal(hl, dl)
    # video c is read at frames 1..4 ("train": 7 // 4 = 1 frame per segment) or 1, 3, 5, 7 ("val"): frame 3, the
    # progressive one, is among them either way
    assert loader.fallback_frames == 1 and loader.decode_errors() == 0


def test_the_decode_launch_is_capturable():
    packed = jpeg.pack_jpeg_clips([([jc.jpg(n)], 0) for n in ("p17x23_420", "rst1_64x48_420", "p17x23_gray")])
    (frames, htabs, qtabs, streams), (n, nh, nq) = jpeg.sections(packed.blob.to(DEV), packed.layout)
    eager, _, eager_status = jpeg.decode_jpeg_frames(packed, DEV)
    rgb = torch.full((packed.rgb_bytes,), 9, dtype=torch.uint8, device=DEV)
    ws = torch.empty(packed.workspace_bytes, dtype=torch.uint8, device=DEV)
    status = torch.full((n + 1,), -1, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            jpeg.launch_decode(streams, frames, qtabs, htabs, n, rgb, ws, status, nq, nh)
    torch.cuda.current_stream(DEV).wait_stream(side)
    rgb.fill_(9)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(rgb, eager) and torch.equal(status, eager_status) and status.tolist() == [0, 0, 0, 0]
