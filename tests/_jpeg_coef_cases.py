"""What tests/test_jpeg_coef.py and tests/test_jpeg_coef_gpu.py share: the resident set of the packed-coefficient tests
(every index case, every supported fixture, the corrupted corpus, and two frames written with Pillow here: uniform noise
at quality 100 for 16-bit and crowded blocks, a flat 8x8 frame for blocks with no AC), the table of tampered regions, and
ONE run per process of the host program tests/jpeg_coef_main.cpp (csrc/rk_jpeg_core.hpp under AddressSanitizer + UBSan, a
stand-alone child process) over all of it."""
import functools
import io
import os
import subprocess
import tempfile

import numpy as np

import _jpeg_cases as jc
import _jpeg_index_cases as ic
from rubiksnet_amd import jpeg

NOISE, FLAT = "noise16_q100", "flat8"
GOOD = list(ic.CASES) + [n for n in jc.SUPPORTED if n not in ic.CASES] + [NOISE, FLAT]
NAMES = GOOD + list(jc.CORRUPT)
KINDS = ("off + 2", "off - 2", "off past the region", "region past the blob", "every mask bit set", "wide bit of the last block",
         "region cut by 2")


@functools.lru_cache(maxsize=None)
def written():
    """The two frames Pillow writes here -> {name: file bytes}."""
    from PIL import Image
    rng = np.random.default_rng(7)
    out = {}
    # the same uniform noise in all three channels: independent channels average out in the luma, and its ACs stay in int8
    for name, pic, quality in ((NOISE, np.repeat(rng.integers(0, 256, (16, 16, 1), dtype=np.uint8), 3, axis=2), 100),
                               (FLAT, np.full((8, 8, 3), 90, dtype=np.uint8), 90)):
        buf = io.BytesIO()
        Image.fromarray(pic).save(buf, "JPEG", quality=quality)
        out[name] = buf.getvalue()
    return out


def jpg(name):
    return written()[name] if name in (NOISE, FLAT) else jc.jpg(name)


@functools.lru_cache(maxsize=None)
def want_rgb(name):
    """The committed Pillow decode of a fixture; Pillow's decode, now, of a frame written here."""
    if name in (NOISE, FLAT):
        from PIL import Image
        with Image.open(io.BytesIO(jpg(name))) as im:
            return np.asarray(im.convert("RGB"))
    return jc.rgb(name)


@functools.lru_cache(maxsize=None)
def resident():
    """NAMES as a resident set, one video per frame -> (names, ResidentJpeg)."""
    res = jpeg.pack_resident([([jpg(n)], 0) for n in NAMES])
    assert not res.fallback and int(res.layout[0]) == len(NAMES)
    return list(NAMES), res


def rgb_table(res):
    return ic.rgb_table(res)


def tampers():
    """[(frame, kind, block)]: every kind on a 4:2:0 frame without and a 4:4:4 frame with restart markers -- offsets of the
    first, a middle and the last block, the mask of a middle block (the smooth fixtures leave room for more bits)."""
    rows = []
    for name in ("p17x23_420", "rst2_40x24_444"):
        i = NAMES.index(name)
        head = jpeg.parse_jpeg(jpg(name))
        rec = np.array([(0, 0, 0, head.width, head.height, head.components, head.sampling, 0, 0, 0, 0, 0)], dtype=jpeg.FRAME_DTYPE)
        last = int(jpeg._geometry_blocks(rec)[3][0]) - 1
        assert last >= 4
        rows += [(i, 0, b) for b in (0, 2, last)] + [(i, 1, b) for b in (0, 2, last)] + [(i, 2, b) for b in (0, 2, last)]
        rows += [(i, 3, 0), (i, 4, 2), (i, 4, last), (i, 5, last), (i, 6, 0)]
    return rows


@functools.lru_cache(maxsize=None)
def host_run():
    """One run of the host program over resident() and tampers().  None without a compiler; otherwise a dict: names, code /
    exact int32 [n], kinds int32 [n, 3], first_block / region_off int64 [n + 1], coefs int16 [blocks, 64], blob uint8, rgb
    uint8 [rgb_bytes], rgb_off int64 [n], tampered: [(code, same, lo, hi, bytes of the tampered blob)].  The program must
    end with status 0 and no sanitizer report.  Asserts that the set holds every kind of block."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = jc.build_program("jpeg_coef_main", tmp)
        if exe is None:
            return None
        names, res = resident()
        (frames, htabs, qtabs, streams), (n, nh, nq) = jpeg.sections(res.blob, res.layout)
        rec = jpeg.records(res.blob, res.layout).copy()
        rgb_off, rgb_bytes = rgb_table(res)
        rec["rgb_off"] = rgb_off
        tam = np.asarray(tampers(), dtype=np.int32).reshape(-1, 3)
        src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(src, "wb") as fh:
            fh.write(np.array([n, nq, nh, len(tam)], dtype=np.int32).tobytes())
            fh.write(np.array([streams.numel(), rgb_bytes, 0, 0], dtype=np.int64).tobytes())
            fh.write(rec.tobytes())
            for t in (htabs, qtabs, streams):
                fh.write(t.numpy().tobytes())
            fh.write(tam.tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        done = subprocess.run([exe, src, dst], env=env, capture_output=True, text=True, timeout=120)
        assert done.returncode == 0 and "Sanitizer" not in done.stderr and "runtime error" not in done.stderr, \
            (done.returncode, done.stderr[-3000:])
        raw = open(dst, "rb").read()
    out, at = {"names": names, "rgb_off": rgb_off, "tampers": tam}, 0

    def take(dtype, count):
        nonlocal at
        size = np.dtype(dtype).itemsize * count
        arr = np.frombuffer(raw[at:at + size], dtype=dtype)
        assert arr.size == count
        at += size
        return arr

    out["code"], out["exact"], out["kinds"] = take(np.int32, n), take(np.int32, n), take(np.int32, 3 * n).reshape(n, 3)
    out["first_block"], out["region_off"] = take(np.int64, n + 1), take(np.int64, n + 1)
    out["coefs"] = take(np.int16, int(out["first_block"][n]) * 64).reshape(-1, 64)
    out["blob"], out["rgb"] = take(np.uint8, int(out["region_off"][n])), take(np.uint8, rgb_bytes)
    out["tampered"] = []
    for _ in range(len(tam)):
        code, same = take(np.int32, 2).tolist()
        lo, hi, size = take(np.int64, 3).tolist()
        out["tampered"].append((code, same, lo, hi, take(np.uint8, size)))
    assert at == len(raw)
    wide, narrow, none = out["kinds"][:len(GOOD)].sum(axis=0).tolist()
    assert wide >= 1 and narrow >= 1 and none >= 1, (wide, narrow, none)
    return out
