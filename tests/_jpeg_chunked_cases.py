"""What tests/test_jpeg_chunked.py and tests/test_jpeg_chunked_gpu.py share: the resident set of the chunked index build
(the index cases at every segment length and the corrupted corpus, then the clip frames, the dense noise frames, frames
shorter than one chunk and one large Pillow-written picture), the settings, and ONE run per process of the host program
tests/jpeg_chunked_main.cpp (csrc/rk_jpeg_core.hpp under AddressSanitizer + UBSan, a stand-alone child process)."""
import functools
import io
import os
import subprocess
import tempfile

import numpy as np

import _jpeg_cases as jc
import _jpeg_index_cases as ic
from rubiksnet_amd import jpeg

SETTINGS = [(16, 64), (64, 16), (256, 64), (16, 8), (256, 0), (256, 1)]         # chunk_bytes, max_rounds
NOISE = ["noise_q100_444", "noise_q100_std_444"]
SHORT = ["flat_420", "b8_444", "n4x3_420"]                                      # shorter than one 256-byte chunk
EXTRA = jc.CLIP + NOISE + SHORT
BIG = "big_640x480"


@functools.lru_cache(maxsize=None)
def big_picture():
    """A smooth 640x480 picture with mild noise, written by Pillow at quality 90, 4:2:0: at 16 bytes a chunk it has more
    chunks than a workgroup has lanes.  None without Pillow."""
    try:
        from PIL import Image
    except ImportError:
        return None
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:480, 0:640]
    pic = np.stack([127 + 100 * np.sin(xx / 37.0) * np.cos(yy / 29.0), 0.3 * xx + 0.2 * yy, 127 + 90 * np.cos((xx + yy) / 53.0)],
                   axis=-1)
    pic = np.clip(pic + rng.normal(0, 3, pic.shape), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(pic).save(buf, "JPEG", quality=90)
    return buf.getvalue()


def data_of(name):
    return big_picture() if name == BIG else jc.jpg(name)


@functools.lru_cache(maxsize=None)
def resident():
    """ic.resident()'s frames, then EXTRA and (with Pillow) BIG at one segment per MCU row: one video per frame.
    -> (names, ResidentJpeg)."""
    base, res = ic.resident()
    extra = EXTRA + ([BIG] if big_picture() is not None else [])
    names = list(base) + extra
    heads = [jpeg.parse_jpeg(data_of(x)) for x in extra]
    seg = res.seg_mcus.tolist() + [jpeg._mcus(h.width, h.height, h.components, h.sampling)[0] for h in heads]
    out = jpeg.pack_resident([([data_of(x)], 0) for x in names], seg_mcus=seg)
    assert not out.fallback and int(out.layout[0]) == len(names)
    return names, out


def records(res):
    rec = jpeg.records(res.blob, res.layout).copy()
    rec.flags.writeable = False                 # the set is cached: nobody edits it through this
    return rec


def chunk_counts(rec, chunk_bytes):
    """rkjpeg::chunk_count per record: 0 where the frame cannot take the chunked route."""
    length = rec["stream_len"].astype(np.int64)
    ok = (rec["restart_interval"] == 0) & (length >= 1) & (length <= chunk_bytes * 4096)
    return np.where(ok, (length + chunk_bytes - 1) // chunk_bytes, 0)


@functools.lru_cache(maxsize=None)
def host_run():
    """One run of the host program over resident() at every setting.  None without a compiler; otherwise a dict: names,
    chain int32 [n] and chain_entries (the sequential walk), and per setting (chunk_bytes, max_rounds) a dict of status,
    route, passed, chunks int32 [n] and entries.  The program must end with status 0 and no sanitizer report."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = jc.build_program("jpeg_chunked_main", tmp)
        if exe is None:
            return None
        names, res = resident()
        (frames, htabs, _, streams), (n, nh, nq) = jpeg.sections(res.blob, res.layout)
        n_entries = int(res.entry_off[-1])
        src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(src, "wb") as fh:
            fh.write(np.array([n, nq, nh, len(SETTINGS)], dtype=np.int32).tobytes())
            fh.write(np.array([streams.numel(), n_entries, 0, 0], dtype=np.int64).tobytes())
            for t in (frames, htabs, streams):
                fh.write(t.numpy().tobytes())
            fh.write(res.seg_mcus.numpy().astype(np.int32).tobytes())
            fh.write(res.entry_off.numpy().astype(np.int64).tobytes())
            fh.write(np.asarray(SETTINGS, dtype=np.int32).tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        done = subprocess.run([exe, src, dst], env=env, capture_output=True, text=True, timeout=300)
        assert done.returncode == 0 and "Sanitizer" not in done.stderr and "runtime error" not in done.stderr, \
            (done.returncode, done.stderr[-3000:])
        raw = open(dst, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        size = np.dtype(dtype).itemsize * count
        arr = np.frombuffer(raw[at:at + size], dtype=dtype)
        at += size
        return arr

    out = {"names": names, "chain": take(np.int32, n), "chain_entries": take(jpeg.ENTRY_DTYPE, n_entries)}
    for setting in SETTINGS:
        out[setting] = {"status": take(np.int32, n), "route": take(np.int32, n), "passed": take(np.int32, n),
                        "chunks": take(np.int32, n), "entries": take(jpeg.ENTRY_DTYPE, n_entries)}
    assert at == len(raw)
    return out


def good_plain(host, rec):
    """Frames the sequential walk accepts that have no restart interval: those the chunked walk may be asked to win."""
    return [i for i in range(len(rec)) if host["chain"][i] == 0 and int(rec["restart_interval"][i]) == 0]


def check_routes(host_or_routes, rec, names, chain):
    """The conditions that keep the equality from being won by falling back.  host_or_routes: {setting: route int32 [n]}."""
    good = [i for i in range(len(rec)) if chain[i] == 0 and int(rec["restart_interval"][i]) == 0]
    assert len(good) >= 20
    for setting in ((256, 64), (16, 64)):
        chunks = chunk_counts(rec, setting[0])
        small = [i for i in good if 1 <= chunks[i] <= 64]
        assert len(small) >= 10, setting
        for i in small:
            assert 0 < host_or_routes[setting][i] <= chunks[i], (setting, names[i], int(host_or_routes[setting][i]))
    for i in good:
        if names[i].startswith("clip"):
            assert host_or_routes[(64, 16)][i] > 0, names[i]
    assert host_or_routes[(16, 8)][names.index("noise_q100_444")] == 0
    assert not host_or_routes[(256, 0)].any()
    for setting in SETTINGS:
        for i in range(len(rec)):
            if chain[i] != 0 or int(rec["restart_interval"][i]) != 0:
                assert host_or_routes[setting][i] == 0, (setting, names[i])
            assert 0 <= host_or_routes[setting][i] <= setting[1], (setting, names[i])
