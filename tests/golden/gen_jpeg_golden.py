"""Writes tests/golden/jpeg_cases.npz: JPEG files made with Pillow's own encoder from synthetic images, and what
`Image.open(f).convert("RGB")` gives for them.  Nothing here depends on the decoder under test.

    python tests/golden/gen_jpeg_golden.py

Keys: "<case>.jpg" (the file, uint8) and "<case>.rgb" (uint8 [H, W, 3]) for the supported cases; "clip<k>.jpg" and
"clip<k>.sha256" (the digest of the RGB bytes: eight 240x320 frames decoded would not fit the size budget) for the
8-frame clip; "unsupported_<kind>.jpg" for files parse_jpeg must refuse; "corrupt_<kind>.jpg" for the corrupted corpus,
all made from the 17x23 4:2:0 case and all expected to decode to a zero frame with a non-zero status.  The single-byte
flips of that corpus are stored as positions in the entropy-coded segment ("flip_scan_start", "flip_invalid_at"), next
to the flips that leave a valid stream ("flip_valid_at"); tests/_jpeg_cases.py builds the files.
"""
import hashlib
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def encode(rgb, mode="RGB", **kw):
    buf = io.BytesIO()
    Image.fromarray(rgb, mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def decode(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def scan_range(data):
    """(start, end) of the entropy-coded segment of a file Pillow wrote: behind the SOS header, up to the EOI."""
    sos = data.index(b"\xff\xda")
    assert data[-2:] == b"\xff\xd9"
    return sos + 2 + ((data[sos + 2] << 8) | data[sos + 3]), len(data) - 2


def scan_is_valid(data):
    """Is the one scan of a baseline file Pillow wrote (no restart interval) a stream ITU-T T.81 allows?  The decoding
    procedure of F.2.2 on bit strings, as slow and plain as it gets, with the rules a stream must keep:
      - no marker inside the entropy-coded segment (B.1.1.5: only RSTn may, and only with a restart interval);
      - every code is one of its table's (F.2.2.3); DC categories 0..11, AC categories 1..10 (tables F.1, F.2), the DC
        value within the 12 bits a DIFF of two can span;
      - a run never leads past coefficient 63, and ZRL is followed by a coefficient of the same block (F.1.2.2.3 emits
        it only in front of one);
      - the scan's MCUs use the data up: less than a byte is left, and those pad bits are ones (F.1.2.3)."""
    pos, huff, comps = 2, {}, None
    while True:
        assert data[pos] == 0xFF
        m, n = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + n]
        if m == 0xC4:
            p = 0
            while p < len(seg):
                counts, table, code = seg[p + 1:p + 17], {}, 0
                vals = seg[p + 17:p + 17 + sum(counts)]
                k = 0
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        table[(length, code)] = vals[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                huff[seg[p]] = table
                p += 17 + len(vals)
        elif m == 0xC0:
            h, w = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15) for i in range(seg[5])]
        elif m == 0xDD:
            raise AssertionError("written for files without a restart interval")
        elif m == 0xDA:
            sel = {seg[1 + 2 * i]: (seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(seg[0])}
            pos += 2 + n
            break
        pos += 2 + n
    bits = []
    while True:                                           # the segment ends at the EOI Pillow wrote
        byte = data[pos]
        if byte == 0xFF:
            if data[pos + 1] == 0x00:
                pos += 1
            elif data[pos + 1] == 0xD9 and pos + 2 == len(data):
                break
            else:
                return False                              # a marker inside the segment
        bits.append(format(byte, "08b"))
        pos += 1
    bits = "".join(bits)
    at = 0

    def symbol(table):
        nonlocal at
        for length in range(1, 17):
            if at + length > len(bits):
                return None
            sym = table.get((length, int(bits[at:at + length], 2)))
            if sym is not None:
                at += length
                return sym
        return None

    def magnitude(size):
        nonlocal at
        if at + size > len(bits):
            return None
        v = int(bits[at:at + size], 2)
        at += size
        return v if v >= 1 << (size - 1) else v - (1 << size) + 1

    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mcus = -(-w // (8 * hmax)) * -(-h // (8 * vmax))
    pred = {c[0]: 0 for c in comps}
    for _ in range(mcus):
        for cid, hs, vs in comps:
            for _ in range(hs * vs if len(comps) > 1 else 1):
                s = symbol(huff[sel[cid][0]])
                if s is None or s > 11:
                    return False
                if s:
                    diff = magnitude(s)
                    if diff is None:
                        return False
                    pred[cid] += diff
                if abs(pred[cid]) > 2047:
                    return False
                k = 1
                while k < 64:
                    rs = symbol(huff[0x10 | sel[cid][1]])
                    if rs is None:
                        return False
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        if k > 63:
                            return False
                        continue
                    k += r
                    if k > 63 or s > 10 or magnitude(s) is None:
                        return False
                    k += 1
    return len(bits) - at < 8 and set(bits[at:]) <= {"1"}


def smooth(h, w, seed, noise=0):
    """A colourful low-frequency picture, plus uniform noise of the given amplitude."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((h, w, 3))
    for c in range(3):
        a, b, p, q = rng.uniform(0.02, 0.25, 4)
        out[..., c] = 128 + 70 * np.sin(a * x + p * 20) + 50 * np.cos(b * y + q * 20) + 0.3 * (x - y) * (c - 1)
    if noise:
        out += rng.uniform(-noise, noise, out.shape)
    return np.clip(out, 0, 255).astype(np.uint8)


def main():
    rng = np.random.default_rng(20240611)
    cases, out = {}, {}
    cases["b8_444"] = encode(smooth(8, 8, 1, 30), quality=75, subsampling=0)
    cases["b1_444"] = encode(np.array([[[200, 30, 90]]], dtype=np.uint8), quality=75, subsampling=0)
    base = smooth(23, 17, 2, 40)                       # 17 wide, 23 high: partial MCUs on both edges, odd chroma sizes
    cases["p17x23_420"] = encode(base, quality=75, subsampling=2)
    cases["p33x17_422"] = encode(smooth(17, 33, 3, 40), quality=75, subsampling=1)
    cases["p17x23_444"] = encode(base, quality=75, subsampling=0)
    cases["p17x23_gray"] = encode(base[..., 1].copy(), mode="L", quality=75)
    cases["n4x3_420"] = encode(smooth(3, 4, 4, 60), quality=90, subsampling=2)      # chroma 2 wide: box replication
    cases["n3x5_422"] = encode(smooth(5, 3, 5, 60), quality=90, subsampling=1)
    cases["n6x6_420"] = encode(smooth(6, 6, 6, 60), quality=90, subsampling=2)      # chroma 3 wide: the narrowest fancy case
    cases["rst1_48x48_420"] = encode(smooth(48, 48, 7, 30), quality=75, subsampling=2, restart_marker_blocks=1)
    cases["rst1_64x48_420"] = encode(smooth(48, 64, 8, 30), quality=75, subsampling=2, restart_marker_blocks=1)  # RST wraps past 7
    cases["rst2_40x24_444"] = encode(smooth(24, 40, 9, 30), quality=75, subsampling=0, restart_marker_blocks=2)
    loud = rng.integers(0, 256, (32, 32, 3)).astype(np.int64)
    loud[:, 8:16] //= 8                                 # dark and bright block columns: large DC differences
    loud[:, 16:24] = 255 - loud[:, 16:24] // 8
    cases["noise_q100_444"] = encode(loud.astype(np.uint8), quality=100, subsampling=0, optimize=True)
    cases["noise_q100_std_444"] = encode(loud.astype(np.uint8), quality=100, subsampling=0)     # the standard tables: 16-bit codes
    cases["noise_q10_420"] = encode(smooth(32, 32, 10, 90), quality=10, subsampling=2)
    cases["gradient_q75_420"] = encode(smooth(24, 32, 11), quality=75, subsampling=2)
    cases["flat_420"] = encode(np.full((16, 16, 3), (90, 140, 200), dtype=np.uint8), quality=75, subsampling=2)
    for name, data in cases.items():
        out[name + ".jpg"] = np.frombuffer(data, dtype=np.uint8)
        out[name + ".rgb"] = decode(data)

    for k in range(8):                                  # one clip of 8 frames, 240 high and 320 wide
        y, x = np.mgrid[0:240, 0:320].astype(np.float64)
        frame = np.stack([128 + 100 * np.sin((x + 9 * k) / 23) * np.cos(y / 31), 128 + 90 * np.cos((x - y + 5 * k) / 40),
                          40 + 0.6 * x + 0.1 * k * y / 8], axis=-1)
        frame[60 + 4 * k:120 + 4 * k, 100 + 6 * k:180 + 6 * k] = (250, 20 * k, 10)      # a moving hard-edged box
        data = encode(np.clip(frame, 0, 255).astype(np.uint8), quality=60, subsampling=2)
        out["clip%d.jpg" % k] = np.frombuffer(data, dtype=np.uint8)
        out["clip%d.sha256" % k] = np.frombuffer(hashlib.sha256(decode(data).tobytes()).digest(), dtype=np.uint8)

    small = smooth(16, 16, 12, 20)
    out["unsupported_progressive.jpg"] = np.frombuffer(encode(small, quality=75, progressive=True), dtype=np.uint8)
    cmyk = np.concatenate([small, small[..., :1]], axis=-1)
    out["unsupported_cmyk.jpg"] = np.frombuffer(encode(cmyk, mode="CMYK", quality=75), dtype=np.uint8)
    v440 = bytearray(encode(small, quality=75, subsampling=1))
    sof = v440.index(b"\xff\xc0")
    assert v440[sof + 11] == 0x21
    v440[sof + 11] = 0x12                               # the luma factors 2x1 -> 1x2: a 4:4:0 header (Pillow writes none)
    out["unsupported_440.jpg"] = np.frombuffer(bytes(v440), dtype=np.uint8)

    good = cases["p17x23_420"]
    a, b = scan_range(good)
    for pct in (25, 50, 75):                            # cut inside the entropy-coded segment
        out["corrupt_cut%d.jpg" % pct] = np.frombuffer(good[:a + (b - a) * pct // 100], dtype=np.uint8)
    # Single-byte flips (one byte of the segment inverted), drawn in one seeded order.  A Huffman stream re-synchronises
    # within a few symbols, so many a flipped file is still a VALID baseline stream that spells other coefficients: no
    # decoder can tell it from an intended file (libjpeg decodes it without a warning), and it is no corrupted input in
    # any sense a status could report.  Every drawn position is therefore classified by scan_is_valid below -- T.81's
    # decoding procedure restated here, independent of the decoder under test -- and kept: the first 16 whose stream
    # T.81 does not allow are the corrupted corpus ("corrupt_flipNN", must be refused), the valid ones drawn on the way
    # are "altered_flipNN" (must decode to exactly what libjpeg makes of the same bytes).  Stored as positions.
    order = np.random.default_rng(7).permutation(b - a)
    invalid, valid = [], []
    for at in (int(v) for v in order):
        bad = bytearray(good)
        bad[a + at] ^= 0xFF
        (valid if scan_is_valid(bytes(bad)) else invalid).append(at)
        if len(invalid) == 16:
            break
    assert len(invalid) == 16 and scan_is_valid(good)
    out["flip_scan_start"] = np.array([a], dtype=np.int64)
    out["flip_invalid_at"] = np.array(invalid, dtype=np.int64)
    out["flip_valid_at"] = np.array(valid, dtype=np.int64)
    bad = bytearray(good)
    bad[(a + b) // 2:(a + b) // 2 + 2] = b"\xff\xd9"    # a stray EOI
    out["corrupt_eoi.jpg"] = np.frombuffer(bytes(bad), dtype=np.uint8)
    bad = bytearray(encode(base, quality=75, subsampling=2, restart_marker_blocks=1))
    start = scan_range(bytes(bad))[0]
    first, second = bad.index(b"\xff\xd0", start), bad.index(b"\xff\xd1", start)
    bad[first + 1], bad[second + 1] = 0xD1, 0xD0        # RST0 and RST1 change places
    out["corrupt_rst_swapped.jpg"] = np.frombuffer(bytes(bad), dtype=np.uint8)

    path = os.path.join(HERE, "jpeg_cases.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
