"""What tests/test_jpeg_index.py and tests/test_jpeg_index_gpu.py share: the resident set built from the committed JPEG
fixtures (every index case at every segment length, then the corrupted corpus), the list of tampered entries, and ONE run
per process of the host program tests/jpeg_index_main.cpp (csrc/rk_jpeg_core.hpp under AddressSanitizer + UBSan, a
stand-alone child process) over all of it."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import _jpeg_cases as jc
from rubiksnet_amd import jpeg

# 2x2 MCUs; 3x3; 4:4:4; grayscale; R = 1; RSTn wrapping past 7; 5x3 MCUs with R = 2 (row entries on and between restarts)
CASES = ["p17x23_420", "p33x17_422", "p17x23_444", "p17x23_gray", "rst1_48x48_420", "rst1_64x48_420", "rst2_40x24_444"]
KINDS = ("bit + 1", "bit - 1", "bit_pos = 8 len + 1", "bit_pos = -1", "pred + 1", "pred = 4000", "swapped")


def mcus(name):
    h = jpeg.parse_jpeg(jc.jpg(name))
    return jpeg._mcus(h.width, h.height, h.components, h.sampling)


def segment_lengths(name):
    """E in {1, mcux, nmcu, nmcu + 3}."""
    mx, my = mcus(name)
    return [1, mx, mx * my, mx * my + 3]


GOOD = [(name, E) for name in CASES for E in segment_lengths(name)]


@functools.lru_cache(maxsize=None)
def resident():
    """GOOD, then the corrupted corpus at one segment per MCU row: one video per frame."""
    names = [n for n, _ in GOOD] + list(jc.CORRUPT)
    seg = [E for _, E in GOOD] + [mcus(n)[0] for n in jc.CORRUPT]
    res = jpeg.pack_resident([([jc.jpg(n)], 0) for n in names], seg_mcus=seg)
    assert not res.fallback and int(res.layout[0]) == len(names)
    return names, res


def frame_of(name, E):
    return GOOD.index((name, E))


def tampers():
    """[(frame, kind, entry a, entry b)]: every kind on a middle entry, and some on the first and the last, of a frame
    with a restart interval (entries on and between restarts) and of one without."""
    rows = []
    for name, E in (("rst2_40x24_444", 5), ("p17x23_420", 1), ("rst1_64x48_420", 4)):
        i = frame_of(name, E)
        mx, my = mcus(name)
        last = (mx * my + E - 1) // E - 1
        assert last >= 2
        rows += [(i, kind, 1, 1) for kind in range(6)]
        rows += [(i, kind, 0, 0) for kind in (0, 2, 3, 4)] + [(i, kind, last, last) for kind in (0, 1, 5)]
        rows += [(i, 6, 1, 2), (i, 6, 0, last)]
    return rows


def rgb_table(res):
    """Back-to-back places for every record -> (int64 rgb_off [n], rgb_bytes)."""
    rec = jpeg.records(res.blob, res.layout).copy()
    sizes = rec["width"].astype(np.int64) * rec["height"] * 3
    return np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64), int(sizes.sum())


@functools.lru_cache(maxsize=None)
def host_run():
    """One run of the host program over resident() and tampers().  None without a compiler; otherwise a dict: names,
    whole / built / tiled int32 [n], entries (ENTRY_DTYPE [n_entries]), tampered int32 [t, 2], rgb uint8 [rgb_bytes],
    rgb_off int64 [n], stderr.  The program must end with status 0 and no sanitizer report."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = jc.build_program("jpeg_index_main", tmp)
        if exe is None:
            return None
        names, res = resident()
        (frames, htabs, qtabs, streams), (n, nh, nq) = jpeg.sections(res.blob, res.layout)
        rec = jpeg.records(res.blob, res.layout).copy()
        rgb_off, rgb_bytes = rgb_table(res)
        rec["rgb_off"] = rgb_off
        tam = np.asarray(tampers(), dtype=np.int32).reshape(-1, 4)
        n_entries = int(res.entry_off[-1])
        src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(src, "wb") as fh:
            fh.write(np.array([n, nq, nh, len(tam)], dtype=np.int32).tobytes())
            fh.write(np.array([streams.numel(), rgb_bytes, n_entries, 0], dtype=np.int64).tobytes())
            fh.write(rec.tobytes())
            for t in (htabs, qtabs, streams):
                fh.write(t.numpy().tobytes())
            fh.write(res.seg_mcus.numpy().astype(np.int32).tobytes())
            fh.write(res.entry_off.numpy().astype(np.int64).tobytes())
            fh.write(tam.tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        done = subprocess.run([exe, src, dst], env=env, capture_output=True, text=True, timeout=120)
        assert done.returncode == 0 and "Sanitizer" not in done.stderr and "runtime error" not in done.stderr, \
            (done.returncode, done.stderr[-3000:])
        raw = open(dst, "rb").read()
    out, at = {"names": names, "rgb_off": rgb_off, "tampers": tam}, 0
    for key, dtype, count in (("whole", np.int32, n), ("built", np.int32, n), ("tiled", np.int32, n),
                              ("entries", jpeg.ENTRY_DTYPE, n_entries), ("tampered", np.int32, 2 * len(tam)),
                              ("rgb", np.uint8, rgb_bytes)):
        size = np.dtype(dtype).itemsize * count
        out[key] = np.frombuffer(raw[at:at + size], dtype=dtype)
        at += size
    assert at == len(raw)
    out["tampered"] = out["tampered"].reshape(-1, 2)
    return out
