"""What the JPEG tests share: the committed JPEG fixtures (tests/golden/jpeg_cases.npz, written by
tests/golden/gen_jpeg_golden.py) read once, and the build of the host programs tests/jpeg_*_main.cpp."""
import functools
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def build_program(name, directory):
    """tests/<name>.cpp + tests/jpeg_host.hpp + csrc/rk_jpeg_core.hpp with the host compiler, AddressSanitizer + UBSan: a
    stand-alone program -> its path, None without a compiler."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        return None
    exe = os.path.join(str(directory), name)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rubiksnet_amd", "csrc"),
           os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe]
    # the sanitizer runtimes inside the program (g++ links them as shared libraries unless told otherwise): the program
    # then runs as it is, whatever else the process environment loads
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    return exe


@functools.lru_cache(maxsize=None)
def _npz():
    with np.load(os.path.join(GOLDEN, "jpeg_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def _names(prefix="", suffix=".jpg"):
    return sorted(k[:-len(suffix)] for k in _npz() if k.endswith(suffix) and k.startswith(prefix))


def jpg(name):
    """The file of a case.  The flipped files are stored as positions: byte `at` of the entropy-coded segment of the
    17x23 4:2:0 case inverted -- "corrupt_flipNN" where that leaves a stream T.81 does not allow, "altered_flipNN" where
    the stream is still a valid one that spells another picture (tests/golden/gen_jpeg_golden.py classifies them)."""
    for prefix, key in (("corrupt_flip", "flip_invalid_at"), ("altered_flip", "flip_valid_at")):
        if name.startswith(prefix):
            data = bytearray(_npz()["p17x23_420.jpg"].tobytes())
            data[int(_npz()["flip_scan_start"][0]) + int(_npz()[key][int(name[len(prefix):])])] ^= 0xFF
            return bytes(data)
    return _npz()[name + ".jpg"].tobytes()


def rgb(name):
    return _npz()[name + ".rgb"]


SUPPORTED = sorted(k[:-4] for k in _npz() if k.endswith(".rgb"))
CLIP = ["clip%d" % k for k in range(8)]
UNSUPPORTED = _names("unsupported_")
BROKEN = _names("corrupt_")                             # cut at 25 / 50 / 75 %, a stray EOI, RST markers swapped
FLIPS = ["corrupt_flip%02d" % k for k in range(len(_npz()["flip_invalid_at"]))]     # one byte inverted: invalid streams
ALTERED = ["altered_flip%02d" % k for k in range(len(_npz()["flip_valid_at"]))]     # one byte inverted: still valid streams
CORRUPT = BROKEN + FLIPS


def pillow_rgb_where_defined(data):
    """`convert("RGB")` of a file as Pillow decodes it, or None where a sample of its YCbCr planes touches 0 or 255.
    Such a picture went through libjpeg's range limit, and there libjpeg is not one reference: jidctint.c masks the
    descaled value into its table (a far-out value wraps) while libjpeg-turbo's SIMD passes saturate at 16 bits, so what
    Pillow gives depends on the build and the CPU.  Inside the limit every path computes the same integers.  Only files
    that no encoder wrote (the altered flips) get there."""
    import io

    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        if im.mode != "L":
            im.draft("YCbCr", im.size)
        planes = np.asarray(im)
    if planes.min() == 0 or planes.max() == 255:
        return None
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def clip_digest(k):
    return _npz()["clip%d.sha256" % k].tobytes()
