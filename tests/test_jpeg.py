"""The host side of the device JPEG decode (rubiksnet_amd/jpeg.py) and a host run of the device code
(csrc/rk_jpeg_core.hpp through tests/jpeg_core_main.cpp, built with AddressSanitizer and UBSan and run as a child
process): parse_jpeg against Pillow, pack_jpeg_clips' layout, the goldens against this Pillow, and the decode core
bit-equal on every golden and failing cleanly on every corrupted file.  No GPU."""
import hashlib
import io
import os
import subprocess

import numpy as np
import pytest
import torch

import _jpeg_cases as jc
from rubiksnet_amd import jpeg

ALL_GOOD = jc.SUPPORTED + jc.CLIP


def _pil(data):
    from PIL import Image
    return Image.open(io.BytesIO(data))


# ------------------------------------------------------------------------------------------------- parse_jpeg
def test_the_fixture_covers_what_the_issue_lists():
    for name in ("b8_444", "b1_444", "p17x23_420", "p33x17_422", "p17x23_444", "p17x23_gray", "rst1_48x48_420",
                 "rst2_40x24_444", "noise_q100_444", "noise_q10_420", "gradient_q75_420", "flat_420"):
        assert name in jc.SUPPORTED
    assert jc.UNSUPPORTED == ["unsupported_440", "unsupported_cmyk", "unsupported_progressive"]
    assert len(jc.FLIPS) == 16 and len(set(jc.jpg(c) for c in jc.FLIPS + jc.ALTERED)) == len(jc.FLIPS) + len(jc.ALTERED)
    assert {"corrupt_cut25", "corrupt_cut50", "corrupt_cut75", "corrupt_eoi", "corrupt_rst_swapped"} <= set(jc.CORRUPT)
    assert os.path.getsize(os.path.join(jc.GOLDEN, "jpeg_cases.npz")) <= 200 * 1024


@pytest.mark.parametrize("name", ALL_GOOD)
def test_parse_agrees_with_pillow(name):
    pytest.importorskip("PIL")
    data = jc.jpg(name)
    head = jpeg.parse_jpeg(data)
    assert head is not None
    with _pil(data) as im:
        assert (head.width, head.height) == im.size
        assert head.components == len(im.getbands())
        layers = im.layer                                   # [(id, h, v, quant table)]
        if head.components == 3:
            assert (layers[0][1], layers[0][2]) == {0: (1, 1), 1: (2, 1), 2: (2, 2)}[head.sampling]
        assert len({q.tobytes() for q in head.quant}) == len({tuple(v) for v in im.quantization.values()})
        for c, layer in enumerate(layers):                  # natural order (a Pillow before 8.3: zigzag, as read)
            theirs = np.asarray(im.quantization[layer[3]], dtype=np.uint16)
            assert np.array_equal(head.quant[c], theirs) or np.array_equal(head.quant[c][jpeg._ZIGZAG], theirs)
    a, b = head.scan
    assert data[b:b + 2] == b"\xff\xd9" and data[a - 3:a] == b"\x00\x3f\x00"
    assert len(head.dc) == len(head.ac) == head.components
    if name.startswith("rst"):
        assert head.restart_interval == int(name[3])
        assert data.count(b"\xff\xd0", a, b) >= 1
    if name == "rst1_64x48_420":
        assert data.count(b"\xff\xd0", a, b) == 2          # 11 markers: RST0 comes round again
    if name == "noise_q100_444":
        assert all(int(q.max()) == 1 for q in head.quant)


@pytest.mark.parametrize("name", jc.UNSUPPORTED)
def test_parse_refuses_what_the_device_does_not_decode(name):
    assert jpeg.parse_jpeg(jc.jpg(name)) is None


def test_parse_never_raises_on_garbage_or_prefixes():
    rng = np.random.default_rng(5)
    for k in range(200):
        blob = rng.integers(0, 256, int(rng.integers(0, 400)), dtype=np.uint8).tobytes()
        if k % 2:
            blob = b"\xff\xd8" + blob                       # past the first check
        if k % 4 == 3:
            blob = jc.jpg("p17x23_420")[:int(rng.integers(2, 300))] + blob
        head = jpeg.parse_jpeg(blob)
        assert head is None or isinstance(head, jpeg.JpegHeader)
    whole = jc.jpg("p17x23_420")
    start = jpeg.parse_jpeg(whole).scan[0]
    for cut in range(len(whole) + 1):
        head = jpeg.parse_jpeg(whole[:cut])
        assert (head is not None) == (cut >= start), cut    # the headers complete: a (possibly cut) scan to decode
        if head is not None:
            assert head.scan[0] == start and head.scan[1] <= cut


@pytest.mark.parametrize("name", jc.CORRUPT)
def test_the_corrupted_files_reach_the_device(name):
    """Their headers are intact, so parse_jpeg hands them on: it is the decoder that has to refuse them."""
    head = jpeg.parse_jpeg(jc.jpg(name))
    assert head is not None and (head.width, head.height, head.sampling) == (17, 23, 2)


def test_the_goldens_are_what_this_pillow_decodes():
    pytest.importorskip("PIL")
    for name in jc.SUPPORTED:
        with _pil(jc.jpg(name)) as im:
            assert np.array_equal(np.asarray(im.convert("RGB")), jc.rgb(name)), name
    for k, name in enumerate(jc.CLIP):
        with _pil(jc.jpg(name)) as im:
            assert im.size == (320, 240)
            assert hashlib.sha256(np.asarray(im.convert("RGB")).tobytes()).digest() == jc.clip_digest(k)


# ------------------------------------------------------------------------------------------------- pack_jpeg_clips
def test_huffman_record_decodes_its_own_codes():
    counts, values = jpeg.parse_jpeg(jc.jpg("noise_q100_std_444")).ac[0]
    rec = jpeg.huffman_record(counts, values)
    code, p = 0, 0
    for l in range(1, 17):
        for _ in range(int(counts[l - 1])):
            if l <= 9:
                lo = code << (9 - l)
                assert set(rec["look"][lo:lo + (1 << (9 - l))].tolist()) == {(l << 8) | values[p]}
            assert code <= rec["maxcode"][l] and rec["huffval"][code + rec["valoff"][l]] == values[p]
            code, p = code + 1, p + 1
        code <<= 1
    assert p == len(values) and max(counts[9:]) > 0         # the standard table has codes beyond the 9-bit lookup
    assert int((rec["look"] == 0).sum()) > 0


def test_pack_lays_out_offsets_tables_and_clips():
    a, b, g = jc.jpg("p17x23_420"), jc.jpg("p17x23_444"), jc.jpg("p17x23_gray")
    wide = jc.jpg("p33x17_422")
    packed = jpeg.pack_jpeg_clips([([a, b, a], 4), ([wide], 9), ([g, g], 1)])
    (frames, htabs, qtabs, streams), (n, nh, nq) = jpeg.sections(packed.blob, packed.layout)
    assert (n, len(packed.fallback)) == (6, 0)
    assert all(int(o) % 16 == 0 for o in packed.layout[3:7])
    rec = np.frombuffer(frames.numpy().tobytes(), dtype=jpeg.FRAME_DTYPE)
    heads = [jpeg.parse_jpeg(x) for x in (a, b, a, wide, g, g)]
    lens = [h.scan[1] - h.scan[0] for h in heads]
    assert rec["stream_len"].tolist() == lens and rec["stream_off"].tolist() == np.cumsum([0] + lens[:-1]).tolist()
    assert streams.numel() == sum(lens)
    for r, h, data in zip(rec, heads, (a, b, a, wide, g, g)):
        s = int(r["stream_off"])
        assert streams[s:s + int(r["stream_len"])].numpy().tobytes() == data[h.scan[0]:h.scan[1]]
        assert (r["width"], r["height"], r["components"], r["sampling"]) == (h.width, h.height, h.components, h.sampling)
    sizes = [17 * 23 * 3] * 3 + [33 * 17 * 3] + [17 * 23 * 3] * 2
    assert rec["rgb_off"].tolist() == np.cumsum([0] + sizes[:-1]).tolist() and packed.rgb_bytes == sum(sizes)
    assert packed.clips.tolist() == [[0, 23, 17, 3], [3 * sizes[0], 17, 33, 1], [3 * sizes[0] + sizes[3], 23, 17, 2]]
    assert packed.labels.tolist() == [4, 9, 1]
    # Pillow's default tables at one quality: every file shares them (2 quantisation, 4 Huffman tables in all), and a
    # repeated file adds none
    assert (nq, nh) == (2, 4)
    assert rec["quant"][0].tolist() == rec["quant"][2].tolist() == rec["quant"][1].tolist()
    assert rec["quant"][4][0] == rec["quant"][0][0]
    other = jpeg.pack_jpeg_clips([([a, a], 0), ([jc.jpg("noise_q100_444")], 0)])
    assert int(other.layout[2]) == 3 and int(other.layout[1]) > 4      # one all-ones quantisation table, optimised Huffman tables
    assert packed.workspace_bytes == jpeg.workspace_bytes_for(rec) > 0


def test_pack_sends_a_refused_file_as_rgb_and_counts_it():
    pytest.importorskip("PIL")
    prog = jc.jpg("unsupported_progressive")
    good = jc.jpg("flat_420")
    packed = jpeg.pack_jpeg_clips([([good, prog], 2)])
    assert int(packed.layout[0]) == 1 and len(packed.fallback) == 1
    off, frame = packed.fallback[0]
    with _pil(prog) as im:
        assert off == 16 * 16 * 3 and np.array_equal(frame.numpy(), np.asarray(im.convert("RGB")))
    assert packed.clips.tolist() == [[0, 16, 16, 2]] and packed.rgb_bytes == 2 * 16 * 16 * 3
    with pytest.raises(ValueError, match="differ in size"):
        jpeg.pack_jpeg_clips([([good, jc.jpg("b8_444")], 0)])


def test_workspace_bytes_equal_the_library(tmp_path):
    from rubiksnet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("the HIP library is not built")
    packed = jpeg.pack_jpeg_clips([([jc.jpg(n)], 0) for n in jc.SUPPORTED])
    (frames, _, _, _), (n, _, _) = jpeg.sections(packed.blob, packed.layout)
    rec = np.frombuffer(frames.numpy().tobytes(), dtype=jpeg.FRAME_DTYPE).copy()
    rec["width"][1] = 0                                     # an invalid record takes no workspace
    want = _native.lib().rk_jpeg_workspace_bytes(rec.ctypes.data, n)
    assert want == jpeg.workspace_bytes_for(rec) and _native.lib().rk_jpeg_workspace_bytes(None, 3) == 0


# ------------------------------------------------------------------------------------------------- host run of the device code
@pytest.fixture(scope="module")
def core_main(tmp_path_factory):
    """tests/jpeg_core_main.cpp + csrc/rk_jpeg_core.hpp, host compiler, AddressSanitizer + UBSan; a stand-alone program."""
    exe = jc.build_program("jpeg_core_main", tmp_path_factory.mktemp("jpeg_core"))
    if exe is None:
        pytest.skip("no host C++ compiler")
    return exe


def _run_core(exe, packed, tmp_path, tag):
    """One packed batch through the host program -> (status int32 [n + 1], rgb uint8 [rgb_bytes])."""
    (frames, htabs, qtabs, streams), (n, nh, nq) = jpeg.sections(packed.blob, packed.layout)
    src, dst = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".out"))
    with open(src, "wb") as fh:
        fh.write(np.array([n, nq, nh, 0], dtype=np.int32).tobytes())
        fh.write(np.array([streams.numel(), packed.rgb_bytes, packed.workspace_bytes, 0], dtype=np.int64).tobytes())
        for t in (frames, htabs, qtabs, streams):
            fh.write(t.numpy().tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, src, dst], env=env, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "Sanitizer" not in done.stderr and "runtime error" not in done.stderr, done.stderr[-3000:]
    raw = open(dst, "rb").read()
    return np.frombuffer(raw[:4 * (n + 1)], dtype=np.int32), np.frombuffer(raw[4 * (n + 1):], dtype=np.uint8)


def test_core_decodes_every_golden_bit_equal(core_main, tmp_path):
    packed = jpeg.pack_jpeg_clips([([jc.jpg(n)], 0) for n in ALL_GOOD])
    assert not packed.fallback
    status, out = _run_core(core_main, packed, tmp_path, "good")
    assert status.tolist() == [0] * (len(ALL_GOOD) + 1)
    for name, (off, h, w, _) in zip(ALL_GOOD, packed.clips.tolist()):
        got = out[off:off + h * w * 3].reshape(h, w, 3)
        if name in jc.SUPPORTED:
            want = jc.rgb(name)
            assert got.shape == want.shape and np.array_equal(got, want), \
                (name, np.argwhere(got != want)[:5].tolist(), int((got != want).sum()))
        else:
            assert hashlib.sha256(got.tobytes()).digest() == jc.clip_digest(jc.CLIP.index(name)), name


def _run_between_good_frames(core_main, tmp_path, bad, tag):
    """A good frame on either side of each bad one, one run -> [(name, code, frame)] of the bad ones; the good
    neighbours and the count are checked here."""
    good = jc.jpg("p17x23_420")
    names = ["good"] + [x for c in bad for x in (c, "good")]
    packed = jpeg.pack_jpeg_clips([([good if x == "good" else jc.jpg(x)], 0) for x in names])
    status, out = _run_core(core_main, packed, tmp_path, tag)
    rows = []
    for x, code, (off, h, w, _) in zip(names, status.tolist(), packed.clips.tolist()):
        got = out[off:off + h * w * 3].reshape(h, w, 3)
        if x == "good":
            assert code == 0 and np.array_equal(got, jc.rgb("p17x23_420"))
        else:
            rows.append((x, code, got))
    assert status[-1] == sum(code != 0 for _, code, _ in rows)
    print({x: jpeg.STATUS_NAMES[code] for x, code, _ in rows})
    return rows


def test_core_refuses_every_broken_file_cleanly(core_main, tmp_path):
    """Cut at 25 / 50 / 75 %, a stray EOI, RST markers swapped: zero frames, non-zero codes, no sanitizer report."""
    for x, code, got in _run_between_good_frames(core_main, tmp_path, jc.BROKEN, "broken"):
        assert code != 0 and not got.any(), (x, code)


def test_core_refuses_every_flipped_byte(core_main, tmp_path):
    """The 16 seeded single-byte flips whose stream T.81 does not allow (tests/golden/gen_jpeg_golden.py judges that with
    its own restatement of the standard's decoding procedure): every one ends with a non-zero status and a zero frame."""
    assert len(jc.FLIPS) == 16
    for x, code, got in _run_between_good_frames(core_main, tmp_path, jc.FLIPS, "flips"):
        assert code != 0 and not got.any(), (x, code)


def test_core_never_decodes_a_flipped_byte_silently_wrong(core_main, tmp_path):
    """The flips drawn on the way that leave a VALID baseline stream (a Huffman stream re-synchronises, so an inverted
    byte often just spells other coefficients; nothing a status could report): accepted, and decoded to exactly what
    libjpeg makes of the same bytes -- a picture that differs from the unflipped one -- wherever libjpeg is one reference
    (_jpeg_cases.pillow_rgb_where_defined)."""
    pytest.importorskip("PIL")
    compared = 0
    for x, code, got in _run_between_good_frames(core_main, tmp_path, jc.ALTERED, "altered"):
        assert code == 0 and got.any(), (x, code)
        want = jc.pillow_rgb_where_defined(jc.jpg(x))          # None: libjpeg's own paths differ on this file
        if want is not None:
            assert np.array_equal(got, want) and not np.array_equal(want, jc.rgb("p17x23_420")), x
            compared += 1
    assert compared >= 30, compared


def test_core_rejects_records_that_do_not_fit(core_main, tmp_path):
    base = jpeg.pack_jpeg_clips([([jc.jpg("p17x23_420")], 0) for _ in range(7)])
    (frames, _, _, streams), _ = jpeg.sections(base.blob, base.layout)
    rec = np.frombuffer(frames.numpy(), dtype=jpeg.FRAME_DTYPE)        # a view: the edits land in the blob
    rec["stream_len"][1] = streams.numel() - int(rec["stream_off"][1]) + 1
    rec["rgb_off"][2] = base.rgb_bytes - 17 * 23 * 3 + 1
    rec["width"][3] = 0
    rec["width"][4] = 16385
    rec["quant"][5][1] = 2
    status, out = _run_core(core_main, base, tmp_path, "records")
    assert status.tolist() == [0, 1, 1, 1, 1, 1, 0, 5]
    frames_out = out.reshape(7, 23, 17, 3)
    assert np.array_equal(frames_out[0], jc.rgb("p17x23_420")) and np.array_equal(frames_out[6], jc.rgb("p17x23_420"))
    assert not frames_out[1].any() and not frames_out[5].any()          # a valid rgb range: zeroed
    assert (frames_out[2:5] == 0xA5).all()                              # no valid range of their own: untouched
