"""The dense record format of the packed coefficients, written down once more in numpy from its description
(include/rubiks_hip.h) and from nothing else: no code is shared with csrc/rk_jpeg_core.hpp, which tests/test_jpeg_dense.py
holds against this byte for byte."""
import numpy as np

from rubiksnet_amd import jpeg

RECORD_MAX, GROUP = 130, 64


def shapes(coefs):
    """coefs int16 [nb, 64], natural order -> dict of int arrays [nb]: last, n, e, wide (0 / 1), raw (0 / 1), plain (the
    ordinary record's bytes before the padding byte), size (the record's bytes)."""
    ac = np.asarray(coefs, dtype=np.int64)[:, jpeg._ZIGZAG][:, 1:]
    nz = ac != 0
    last = np.where(nz.any(axis=1), 63 - np.argmax(nz[:, ::-1], axis=1), 0)
    n = nz.sum(axis=1)
    esc = np.abs(ac) > 7
    e = esc.sum(axis=1)
    wide = ((ac < -128) | (ac > 127)).any(axis=1).astype(np.int64)
    plain = 3 + (last + 7) // 8 + (n + 1) // 2 + e * (1 + wide)
    size = (plain + 1) // 2 * 2
    raw = (size > RECORD_MAX).astype(np.int64)
    return dict(last=last, n=n, e=e, wide=wide, raw=raw, plain=plain, size=np.where(raw == 1, RECORD_MAX, size))


def record(block):
    """One block's record as bytes: block int16 [64], natural order."""
    block = np.asarray(block, dtype=np.int16)
    s = {k: int(v[0]) for k, v in shapes(block[None]).items()}
    if s["raw"]:
        return bytes([0x80, 0]) + block.astype("<i2").tobytes()
    zz = block[jpeg._ZIGZAG].astype(np.int64)
    out = bytearray([s["last"] | (s["wide"] << 6)]) + np.int16(zz[0]).astype("<i2").tobytes()
    mask = sum(1 << (k - 1) for k in range(1, 64) if zz[k] != 0)
    out += mask.to_bytes(8, "little")[:(s["last"] + 7) // 8]
    values = [int(v) for v in zz[1:] if v != 0]
    nibbles = [(v & 15) if -7 <= v <= 7 else 8 for v in values] + [0]
    out += bytes(nibbles[2 * i] | (nibbles[2 * i + 1] << 4) for i in range((len(values) + 1) // 2))
    for v in values:
        if not -7 <= v <= 7:
            out += np.int16(v).astype("<i2").tobytes() if s["wide"] else np.int8(v).tobytes()
    if len(out) & 1:
        out += b"\0"
    assert len(out) == s["size"]
    return bytes(out)


def region(coefs):
    """One frame's region as a uint8 array: coefs int16 [nb, 64], natural order, blocks in scan order."""
    coefs = np.asarray(coefs, dtype=np.int16)
    nb = len(coefs)
    groups = (nb + GROUP - 1) // GROUP
    records = [record(c) for c in coefs]
    start = 4 * groups + 2 * nb + np.concatenate([[0], np.cumsum([len(r) for r in records])[:-1]]).astype(np.int64)
    base = start[::GROUP]
    rel = start - np.repeat(base, GROUP)[:nb]
    assert rel.max() < 1 << 16
    return np.frombuffer(base.astype("<u4").tobytes() + rel.astype("<u2").tobytes() + b"".join(records), dtype=np.uint8)


def wide_bytes(coefs):
    """The same blocks' region in the wide format: 4 bytes of table and 10 + n w rounded up to even per block."""
    ac = np.asarray(coefs, dtype=np.int64)[:, jpeg._ZIGZAG][:, 1:]
    count = (ac != 0).sum(axis=1)
    width = np.where(((ac < -128) | (ac > 127)).any(axis=1), 2, 1)
    return int((4 + 10 + ((count * width + 1) & ~1)).sum())
