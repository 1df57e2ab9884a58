"""What tests/test_jpeg_dense.py and tests/test_jpeg_dense_gpu.py share: the resident set of the dense-record tests (the
good frames of tests/_jpeg_coef_cases.py, two more frames written with Pillow here -- a hard edge at quality 100 for
16-bit escapes that are not raw, a 96x80 picture of 180 blocks in three table groups -- and the corrupted corpus), the table
of tampered regions, and the runs of the host program tests/jpeg_dense_main.cpp (csrc/rk_jpeg_core.hpp under
AddressSanitizer + UBSan, a stand-alone child process), which is built once per process."""
import atexit
import functools
import io
import os
import shutil
import subprocess
import tempfile

import numpy as np

import _jpeg_cases as jc
import _jpeg_coef_cases as cc
import _jpeg_dense_ref as ref
from rubiksnet_amd import jpeg

STEP, WAVE = "step16", "wave96x80"
GOOD = list(cc.GOOD) + [STEP, WAVE]
NAMES = GOOD + list(jc.CORRUPT)
TAMPERED = ("p17x23_420", "rst2_40x24_444", WAVE)        # 4:2:0; 4:4:4 with restart markers; three table groups
KINDS = ("rel + 2", "rel - 2", "base + 2", "base - 2", "base past the region", "region past the blob", "region cut by 2",
         "last raised", "last lowered", "a mask bit added below last", "class flipped 0 <-> 1", "class 3",
         "a nibble turned into 0x8", "an escape nibble turned into a value", "a raw tag on an ordinary record")
BLOCK_KINDS = ("no AC", "nibbles only", "int8 escapes", "int16 escapes", "raw")


@functools.lru_cache(maxsize=None)
def written():
    """The two frames Pillow writes here -> {name: file bytes}."""
    from PIL import Image
    step = np.full((16, 16, 3), 255, dtype=np.uint8)
    step[:, :5] = 0
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:80, 0:96]
    img = np.stack([128 + 100 * np.sin(xx / 7.0) * np.cos(yy / 5.0), 128 + 90 * np.cos((xx - yy) / 9.0), 40 + 2 * xx], -1) \
        + rng.uniform(-20, 20, (80, 96, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    out = {}
    for name, pic, kw in ((STEP, step, dict(quality=100, subsampling=0)), (WAVE, img, dict(quality=90, subsampling=2))):
        buf = io.BytesIO()
        Image.fromarray(pic).save(buf, "JPEG", **kw)
        out[name] = buf.getvalue()
    return out


def jpg(name):
    return written()[name] if name in (STEP, WAVE) else cc.jpg(name)


@functools.lru_cache(maxsize=None)
def want_rgb(name):
    """The committed Pillow decode of a fixture; Pillow's decode, now, of a frame written here."""
    if name in (STEP, WAVE):
        from PIL import Image
        with Image.open(io.BytesIO(jpg(name))) as im:
            return np.asarray(im.convert("RGB"))
    return cc.want_rgb(name)


@functools.lru_cache(maxsize=None)
def resident():
    """NAMES as a resident set, one video per frame -> (names, ResidentJpeg)."""
    res = jpeg.pack_resident([([jpg(n)], 0) for n in NAMES])
    assert not res.fallback and int(res.layout[0]) == len(NAMES)
    return list(NAMES), res


@functools.lru_cache(maxsize=None)
def bench_frame():
    """One frame of the benchmark generator's formula (tools/jpeg_decode_time.py: seed 0, 256 x 340, quality 90, 4:2:0)
    -> file bytes."""
    from PIL import Image
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:256, 0:340].astype(np.float64)
    a, b, c = rng.uniform(0.02, 0.2, 3)
    img = np.stack([128 + 90 * np.sin(a * x) * np.cos(b * y), 128 + 80 * np.cos(c * (x - y)), 60 + 0.5 * x + 0.2 * y],
                   axis=-1) + rng.uniform(-25, 25, (256, 340, 3))
    buf = io.BytesIO()
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=90, subsampling=2)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def program():
    """The host program, built once per process -> its path, None without a compiler."""
    tmp = tempfile.mkdtemp(prefix="jpeg_dense_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    return jc.build_program("jpeg_dense_main", tmp)


def run_program(res, tam):
    """One run over a ResidentJpeg and a tamper table [(frame, kind, block)] -> dict: code / exact int32 [n], kinds int32
    [n, 5], first_block / region_off int64 [n + 1], coefs int16 [blocks, 64], blob uint8, rgb uint8 [rgb_bytes], rgb_off
    int64 [n], tampered: [(code, same, lo, hi, bytes of the tampered blob)].  The program must end with status 0 and no
    sanitizer report."""
    exe = program()
    (frames, htabs, qtabs, streams), (n, nh, nq) = jpeg.sections(res.blob, res.layout)
    rec = jpeg.records(res.blob, res.layout).copy()
    rgb_off, rgb_bytes = cc.rgb_table(res)
    rec["rgb_off"] = rgb_off
    tam = np.asarray(tam, dtype=np.int32).reshape(-1, 3)
    with tempfile.TemporaryDirectory() as tmp:
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
    out, at = {"rgb_off": rgb_off, "tampers": tam}, 0

    def take(dtype, count):
        nonlocal at
        size = np.dtype(dtype).itemsize * count
        arr = np.frombuffer(raw[at:at + size], dtype=dtype)
        assert arr.size == count
        at += size
        return arr

    out["code"], out["exact"], out["kinds"] = take(np.int32, n), take(np.int32, n), take(np.int32, 5 * n).reshape(n, 5)
    out["first_block"], out["region_off"] = take(np.int64, n + 1), take(np.int64, n + 1)
    out["coefs"] = take(np.int16, int(out["first_block"][n]) * 64).reshape(-1, 64)
    out["blob"], out["rgb"] = take(np.uint8, int(out["region_off"][n])), take(np.uint8, rgb_bytes)
    out["tampered"] = []
    for _ in range(len(tam)):
        code, same = take(np.int32, 2).tolist()
        lo, hi, size = take(np.int64, 3).tolist()
        out["tampered"].append((code, same, lo, hi, take(np.uint8, size)))
    assert at == len(raw)
    return out


def _first(ok, what, name):
    hits = np.flatnonzero(ok)
    assert hits.size, "%s: no block for %r" % (name, what)
    return int(hits[0])


def tampers_for(plain):
    """[(frame, kind, block)] from a run without tampers: every kind on each frame of TAMPERED.  The table kinds take the
    first, a middle and the last block, and a block of every further group.  The record kinds take the first block where the
    format is bound to notice -- where the change alters the record's length by what its padding cannot absorb, or breaks
    a rule outright:
      last raised           last + 1 stays in the same mask byte, where its bit is clear
      last lowered          last - 1 stays in the same mask byte, which then has a bit above it
      a mask bit added      an odd n: the added nibble is the zero in the last nibble byte's high half; or an even n with no
                            padding byte to take the byte the nibbles grow by
      the class flipped     two escapes or more: the length changes by two bytes at least
      a nibble -> 0x8       class 1, or class 0 with no padding byte
      an escape -> a value  class 1, or class 0 with a padding byte (the length drops to an even count below the span)
      a raw tag             any ordinary record that is not 130 bytes long"""
    rows = []
    for name in TAMPERED:
        i = NAMES.index(name)
        coefs = plain["coefs"][plain["first_block"][i]:plain["first_block"][i + 1]]
        s = ref.shapes(coefs)
        nb = len(coefs)
        assert nb >= 5
        for kind in (0, 1):
            rows += [(i, kind, b) for b in (0, 2, nb - 1)] + [(i, kind, b) for b in range(70, nb, 64)]
        for kind in (2, 3, 4):
            rows += [(i, kind, b) for b in range(0, nb, 64)]
        rows += [(i, 5, 0), (i, 6, 0)]
        plainly = s["raw"] == 0
        last, n, e, wide, padded = s["last"], s["n"], s["e"], s["wide"] == 1, s["plain"] % 2 == 1
        rows += [(i, 7, _first(plainly & (last >= 1) & (last < 63) & (last % 8 != 0), KINDS[7], name)),
                 (i, 8, _first(plainly & (last >= 2) & (last % 8 != 1), KINDS[8], name)),
                 (i, 9, _first(plainly & (n < last) & ((n % 2 == 1) | ~padded), KINDS[9], name)),
                 (i, 10, _first(plainly & (e >= 2), KINDS[10], name)),
                 (i, 11, _first(plainly, KINDS[11], name)),
                 (i, 12, _first(plainly & (n > e) & (wide | ~padded), KINDS[12], name)),
                 (i, 13, _first(plainly & (e >= 1) & (wide | padded), KINDS[13], name)),
                 (i, 14, _first(plainly & (s["size"] != ref.RECORD_MAX), KINDS[14], name))]
    return rows


@functools.lru_cache(maxsize=None)
def host_run():
    """The host program over resident(): once without tampers, for the coefficients the tamper table is chosen from, then
    with it.  None without a compiler; otherwise run_program's dict of the second run, with names.  Asserts that the set
    holds every kind of block."""
    if program() is None:
        return None
    names, res = resident()
    plain = run_program(res, [])
    out = run_program(res, tampers_for(plain))
    assert np.array_equal(out["blob"], plain["blob"]) and np.array_equal(out["coefs"], plain["coefs"])
    out["names"] = names
    have = out["kinds"][:len(GOOD)].sum(axis=0).tolist()
    assert min(have) >= 1, dict(zip(BLOCK_KINDS, have))
    return out


@functools.lru_cache(maxsize=None)
def bench_run():
    """The host program over bench_frame() alone -> run_program's dict, None without a compiler."""
    if program() is None:
        return None
    res = jpeg.pack_resident([([bench_frame()], 0)])
    assert not res.fallback
    return run_program(res, [])
