"""Baseline JPEG frames decoded on the device (rk_jpeg_decode_u8, csrc/rk_jpeg.hip), bit-exact to what Pillow's
`Image.open(f).convert("RGB")` gives with libjpeg(-turbo)'s defaults.

A DataLoader worker only reads the files and walks their headers; the file bytes travel instead of decoded frames
(about an eighth of the bytes), and the GPU does the Huffman decode, the IDCT, the upsampling and the colour conversion.

  parse_jpeg          marker walk over one file: a JpegHeader for SOF0 / 8-bit / one interleaved scan / grayscale or YCbCr
                      at 4:4:4, 4:2:2, 4:2:0; None for anything else; never raises
  pack_jpeg_clips     the collate function, twin of dataset.pack_clips: entropy-coded segments back to back, a record per
                      frame, de-duplicated quantisation / Huffman tables, and the `clips` table pack_clips would have made
                      of the decoded frames.  A frame parse_jpeg rejects is decoded here with Pillow and travels as RGB.
  launch_decode       the launch on device tensors
  decode_jpeg_frames  upload + launch for one packed batch

A set that stays on the device keeps its files' bytes there and is decoded by scan index (rk_jpeg_build_index,
rk_jpeg_decode_indexed_u8; dataset.DeviceFrameCache(resident="jpeg")):

  pack_resident          a whole set as one blob + the index tables (one segment per MCU row by default)
  build_index            upload + the one sequential walk every frame gets (method="chain"), or the same index from
                         many short walks in lock-step rounds (method="chunked": rk_jpeg_build_index_chunked)
  pick_tables            per batch, on the host: which resident frames go where in the batch's RGB arena
  launch_decode_indexed  the launch on device tensors

A streamed batch can take the row-parallel decoder too (decode_jpeg_frames(entropy="rows"), FrameLoader(entropy="rows")):
row_tables makes the index tables of the batch's own records on the host, one segment per MCU row, the chunked build
finds the entries on the device and rk_jpeg_decode_indexed_u8 decodes every record to its own place.

A resident set can also be kept as what the Huffman stage leaves (dataset.DeviceFrameCache(resident="coef")):

  build_coef             the set transcoded once, slab by slab, into packed DCT coefficients (rk_jpeg_coef_sizes,
                         rk_jpeg_coef_pack): per block an offset, a 64-bit mask, the DC and the non-zero AC values
  launch_decode_coef     the per-batch launch (rk_jpeg_decode_coef_u8): no Huffman stage, the same IDCT on the same
                         coefficients; pick_tables as above
  build_coef(record="dense") packs the second record format (a nibble per small AC value; include/rubiks_hip.h); the
                         DeviceCoef remembers it and launch_decode_coef dispatches on it

There is no CPU path: a missing library is an error (tests compare with Pillow).
"""
import collections
import io

import numpy as np
import torch

__all__ = ["JpegHeader", "parse_jpeg", "pack_jpeg_clips", "PackedJpeg", "decode_jpeg_frames", "launch_decode",
           "workspace_bytes_for", "huffman_record", "FRAME_DTYPE", "HUFF_DTYPE", "STATUS_NAMES", "MAX_SIDE", "ENTRY_DTYPE",
           "ResidentJpeg", "pack_resident", "DeviceIndex", "build_index", "PickTables", "pick_tables",
           "frame_workspace_bytes", "indexed_workspace_bytes_for", "launch_decode_indexed", "chunked_workspace_bytes_for",
           "launch_build_index_chunked", "RowTables", "row_tables", "launch_decode_rows", "CHUNK_BYTES", "MAX_ROUNDS",
           "MAX_CHUNKS", "DeviceCoef", "build_coef", "frame_plane_bytes", "coef_workspace_bytes_for", "launch_decode_coef",
           "coef_region_bounds", "COEF_RECORDS"]

MAX_SIDE = 16384
STATUS_NAMES = ("ok", "bad record", "bad code", "run past 63", "truncated", "bad restart", "trailing data", "bad value",
                "bad index")

# include/rubiks_hip.h: rk_jpeg_frame (64 bytes) and rk_jpeg_huff (1424 bytes)
FRAME_DTYPE = np.dtype({"names": ["stream_off", "stream_len", "rgb_off", "width", "height", "components", "sampling",
                                  "restart_interval", "quant", "dc", "ac", "reserved"],
                        "formats": ["<i8", "<i8", "<i8", "<i4", "<i4", "<i4", "<i4", "<i4", ("<u2", 3), ("<u2", 3), ("<u2", 3),
                                    "<u2"],
                        "offsets": [0, 8, 16, 24, 28, 32, 36, 40, 44, 50, 56, 62], "itemsize": 64})
HUFF_DTYPE = np.dtype([("look", "<u2", 512), ("maxcode", "<i4", 18), ("valoff", "<i4", 18), ("huffval", "u1", 256)])
assert FRAME_DTYPE.itemsize == 64 and HUFF_DTYPE.itemsize == 1424

_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                    21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                    60, 61, 54, 47, 55, 62, 63])
_SAMPLING = {0x11: 0, 0x21: 1, 0x22: 2}            # luma H/V factors -> sampling class (chroma 1x1)


class JpegHeader:
    """What the device needs of one file.  width, height; components 1 or 3; sampling 0 (4:4:4), 1 (4:2:2), 2 (4:2:0);
    restart_interval; per component: quant (uint16 [64], natural order), dc / ac ((counts uint8 [16], values bytes));
    scan: the (start, end) byte range of the entropy-coded segment in the file."""
    __slots__ = ("width", "height", "components", "sampling", "restart_interval", "quant", "dc", "ac", "scan")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


def _scan_end(arr, start):
    """The entropy-coded segment runs to the first FF that is followed by anything but 00 (a stuffed FF) or D0..D7
    (RSTn) -- or to the end of the data, where a file was cut."""
    body = arr[start:]
    ff = np.flatnonzero(body[:-1] == 0xFF)
    if ff.size:
        nxt = body[ff + 1]
        stop = ff[(nxt != 0) & ((nxt < 0xD0) | (nxt > 0xD7))]
        if stop.size:
            return start + int(stop[0])
    return arr.size


def _parse(data):
    arr = np.frombuffer(data, dtype=np.uint8)
    size = arr.size
    if size < 4 or arr[0] != 0xFF or arr[1] != 0xD8:
        return None
    qt, dc, ac = {}, {}, {}
    frame, restart, jfif, pos = None, 0, False, 2
    while True:
        if pos + 4 > size or arr[pos] != 0xFF:
            return None
        m = int(arr[pos + 1])
        if m == 0xFF:                                   # a fill byte in front of a marker
            pos += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:              # stand-alone markers carry no length
            pos += 2
            continue
        if m in (0xD8, 0xD9):
            return None
        n = (int(arr[pos + 2]) << 8) | int(arr[pos + 3])
        seg, end = pos + 4, pos + 2 + n
        if n < 2 or end > size:
            return None
        if m == 0xDB:                                   # DQT
            p = seg
            while p < end:
                if p + 65 > end or arr[p] >> 4:         # 16-bit tables belong to 12-bit files
                    return None
                tab = np.zeros(64, dtype=np.uint16)
                tab[_ZIGZAG] = arr[p + 1:p + 65]
                qt[int(arr[p]) & 15] = tab
                p += 65
        elif m == 0xC4:                                 # DHT
            p = seg
            while p < end:
                if p + 17 > end:
                    return None
                tc, th = int(arr[p]) >> 4, int(arr[p]) & 15
                counts = arr[p + 1:p + 17]
                nval = int(counts.sum())
                if tc > 1 or th > 3 or nval > 256 or p + 17 + nval > end:
                    return None
                (ac if tc else dc)[th] = (counts.copy(), arr[p + 17:p + 17 + nval].tobytes())
                p += 17 + nval
        elif m == 0xC0:                                 # SOF0
            if frame is not None or n < 8:
                return None
            prec, h, w, nf = int(arr[seg]), (int(arr[seg + 1]) << 8) | int(arr[seg + 2]), \
                (int(arr[seg + 3]) << 8) | int(arr[seg + 4]), int(arr[seg + 5])
            if prec != 8 or nf not in (1, 3) or n != 8 + 3 * nf or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
                return None
            frame = (w, h, [(int(arr[seg + 6 + 3 * i]), int(arr[seg + 7 + 3 * i]), int(arr[seg + 8 + 3 * i])) for i in range(nf)])
        elif 0xC1 <= m <= 0xCF:                         # every other SOFn, arithmetic conditioning, JPG
            return None
        elif m == 0xDD:                                 # DRI
            if n != 4:
                return None
            restart = (int(arr[seg]) << 8) | int(arr[seg + 1])
        elif m == 0xE0:
            jfif = jfif or arr[seg:seg + 5].tobytes() == b"JFIF\0"
        elif m == 0xEE:
            if arr[seg:seg + 5].tobytes() == b"Adobe":  # Adobe's transform flag: RGB, CMYK or YCCK data
                return None
        elif m == 0xDC:                                 # DNL
            return None
        elif m == 0xDA:                                 # SOS
            if frame is None:
                return None
            w, h, comps = frame
            ns = int(arr[seg])
            if ns != len(comps) or n != 6 + 2 * ns:
                return None
            sel = [(int(arr[seg + 1 + 2 * i]), int(arr[seg + 2 + 2 * i])) for i in range(ns)]
            if [c for c, _ in sel] != [c for c, _, _ in comps]:
                return None
            if (int(arr[seg + 1 + 2 * ns]), int(arr[seg + 2 + 2 * ns]), int(arr[seg + 3 + 2 * ns])) != (0, 63, 0):
                return None
            if ns == 1:
                if comps[0][1] != 0x11:
                    return None
                sampling = 0
            else:
                if comps[1][1] != 0x11 or comps[2][1] != 0x11 or comps[0][1] not in _SAMPLING:
                    return None
                if not jfif and [c for c, _, _ in comps] != [1, 2, 3]:      # libjpeg would guess the colour space
                    return None
                sampling = _SAMPLING[comps[0][1]]
            try:
                quant = [qt[tq] for _, _, tq in comps]
                dcs = [dc[t >> 4] for _, t in sel]
                acs = [ac[t & 15] for _, t in sel]
            except KeyError:
                return None
            for counts, _ in dcs + acs:
                if not _counts_fit(counts):
                    return None
            return JpegHeader(width=w, height=h, components=ns, sampling=sampling, restart_interval=restart, quant=quant,
                              dc=dcs, ac=acs, scan=(end, _scan_end(arr, end)))
        pos = end


def _counts_fit(counts):
    """Do the code counts per length describe a prefix code (no length holds more codes than are left)?"""
    code = 0
    for l in range(16):
        code += int(counts[l])
        if code > (1 << (l + 1)):
            return False
        code <<= 1
    return True


def parse_jpeg(data):
    """A JpegHeader for a file the device decodes, None for anything else (progressive, arithmetic, 12-bit, CMYK / Adobe,
    other samplings, several scans' worth of components, garbage).  Never raises."""
    try:
        return _parse(data)
    except Exception:
        return None


# ------------------------------------------------------------------------------------------------- tables
def huffman_record(counts, values):
    """The rk_jpeg_huff record (HUFF_DTYPE scalar array) of a DHT table: counts uint8 [16], values bytes."""
    rec = np.zeros((), dtype=HUFF_DTYPE)
    look, maxcode, valoff, huffval = rec["look"], rec["maxcode"], rec["valoff"], rec["huffval"]
    vals = np.frombuffer(values, dtype=np.uint8)
    huffval[:vals.size] = vals
    maxcode[:] = -1
    code, p = 0, 0
    for l in range(1, 17):
        cnt = int(counts[l - 1])
        if cnt:
            valoff[l] = p - code
            if l <= 9:
                for k in range(cnt):
                    lo = (code + k) << (9 - l)
                    look[lo:lo + (1 << (9 - l))] = (l << 8) | int(vals[p + k])
            code += cnt
            p += cnt
            maxcode[l] = code - 1
        code <<= 1
    maxcode[17] = 0x7fffffff
    return rec


def _align16(v):
    return (v + 15) & ~15


def _geometry_blocks(frames):
    """rkjpeg::geometry of a FRAME_DTYPE array, in numpy -> (ok, mcux, mcuy, blocks), each per record: are its sizes
    valid, its MCUs per row and per column (1 where they are not), its 8x8 blocks (0 where they are not)."""
    f = np.asarray(frames).reshape(-1)
    w, h, nc, s = (f[k].astype(np.int64) for k in ("width", "height", "components", "sampling"))
    ok = (w >= 1) & (w <= MAX_SIDE) & (h >= 1) & (h <= MAX_SIDE) & ((nc == 1) | ((nc == 3) & (s >= 0) & (s <= 2)))
    hs, vs = np.where((nc == 3) & (s >= 1), 2, 1), np.where((nc == 3) & (s == 2), 2, 1)
    mcux = np.where(ok, (w + 8 * hs - 1) // (8 * hs), 1)
    mcuy = np.where(ok, (h + 8 * vs - 1) // (8 * vs), 1)
    return ok, mcux, mcuy, np.where(ok, mcux * mcuy * np.where(nc == 1, 1, hs * vs + 2), 0)


def _geometry(frames):
    """-> (ok, mcux, mcuy, bytes) per record: _geometry_blocks with, for the blocks, the bytes of the record's region of
    the workspace (0 where its sizes are not valid: 128 of coefficients and 64 of samples per block, rounded up to 16)."""
    ok, mcux, mcuy, blocks = _geometry_blocks(frames)
    return ok, mcux, mcuy, _align16(blocks * 192)


def _mcus(width, height, components, sampling):
    """(MCUs per row, MCUs per column) of one frame's sizes, by _geometry."""
    rec = np.array([(0, 0, 0, width, height, components, sampling, 0, 0, 0, 0, 0)], dtype=FRAME_DTYPE)
    return tuple(int(v[0]) for v in _geometry(rec)[1:3])


def frame_workspace_bytes(frames):
    """int64 per record of a FRAME_DTYPE array: the bytes of its region of the workspace (0 for sizes that are not valid),
    what workspace_bytes_for sums (a resident set asks once and indexes the answer per batch)."""
    return _geometry(frames)[3]


def workspace_bytes_for(frames):
    """rk_jpeg_workspace_bytes of a FRAME_DTYPE array, in numpy (a DataLoader worker does not load the HIP library)."""
    per_frame = frame_workspace_bytes(frames)
    return _align16((per_frame.size + 1) * 8) + int(per_frame.sum())


def sections(blob, layout):
    """(frames, htabs, qtabs, streams) views of a PackedJpeg blob (host or device) and (n, nh, nq)."""
    n, nh, nq, o_frames, o_huff, o_quant, o_stream, stream_bytes = (int(v) for v in layout.tolist())
    return (blob[o_frames:o_frames + n * 64], blob[o_huff:o_huff + nh * HUFF_DTYPE.itemsize],
            blob[o_quant:o_quant + nq * 128], blob[o_stream:o_stream + stream_bytes]), (n, nh, nq)


def records(blob, layout):
    """The frame records of a host blob as a FRAME_DTYPE array: a view, an edit lands in the blob."""
    return np.frombuffer(sections(blob, layout)[0][0].numpy(), dtype=FRAME_DTYPE)


def _check_tensors(specs, say=str):
    """specs: (name, tensor, dtype); say: how the message names a dtype."""
    for name, t, dt in specs:
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor on the GPU" % (name, say(dt)))


# ------------------------------------------------------------------------------------------------- collate
PackedJpeg = collections.namedtuple("PackedJpeg", [
    "blob",             # uint8: frame records | Huffman records | quantisation tables | streams, each section 16-byte aligned
    "layout",           # int64 [8]: n, nh, nq, offsets of the four sections in blob, stream_bytes
    "clips",            # int64 [B, 4]: what pack_clips gives for the decoded frames (offset in the RGB arena, H, W, K)
    "labels",           # int64 [B]
    "rgb_bytes",        # bytes of the RGB arena
    "workspace_bytes",  # rk_jpeg_workspace_bytes of the frame table
    "fallback",         # [(offset in the RGB arena, uint8 [H, W, 3])]: frames decoded on the host
])


def _host_rgb(item):
    from PIL import Image
    with Image.open(io.BytesIO(item)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def pack_jpeg_clips(samples):
    """The collate function of the device-decode path.  samples: [(frames, label)], `frames` a list whose items are the
    bytes of a JPEG file, or uint8 [H, W, 3] (a frame the dataset already decoded on the host); all frames of a sample
    have one size, sizes and frame counts differ freely between samples.  Returns a PackedJpeg.  A file parse_jpeg
    rejects is decoded here with Pillow and travels as RGB (`fallback`); its place in the RGB arena is reserved like
    any other frame's."""
    records, segments, fallback, rows, labels = [], [], [], [], []
    qindex, hindex, qtabs, htabs = {}, {}, [], []

    def table(index, store, key, build):
        i = index.get(key)
        if i is None:
            i = index[key] = len(store)
            store.append(build())
        return i

    rgb_off = stream_off = 0
    for frames, label in samples:
        if len(frames) < 1:
            raise ValueError("a sample without frames")
        size, first = None, rgb_off
        for item in frames:
            head = parse_jpeg(item) if isinstance(item, (bytes, bytearray, memoryview)) else None
            if head is None:
                rgb = _host_rgb(item) if isinstance(item, (bytes, bytearray, memoryview)) else np.asarray(item)
                if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
                    raise ValueError("a frame must be JPEG bytes or uint8 [H, W, 3], got %s %s" % (rgb.dtype, rgb.shape))
                hw = (rgb.shape[0], rgb.shape[1])
                fallback.append((rgb_off, torch.from_numpy(np.array(rgb, dtype=np.uint8, order="C"))))
            else:
                hw = (head.height, head.width)
                a, b = head.scan
                rec = np.zeros((), dtype=FRAME_DTYPE)
                rec["stream_off"], rec["stream_len"], rec["rgb_off"] = stream_off, b - a, rgb_off
                rec["width"], rec["height"], rec["components"] = head.width, head.height, head.components
                rec["sampling"], rec["restart_interval"] = head.sampling, head.restart_interval
                for c in range(head.components):
                    q = head.quant[c]
                    rec["quant"][c] = table(qindex, qtabs, q.tobytes(), lambda: q)
                    for name, (counts, values) in (("dc", head.dc[c]), ("ac", head.ac[c])):
                        rec[name][c] = table(hindex, htabs, counts.tobytes() + values,
                                             lambda: huffman_record(counts, values))
                records.append(rec)
                segments.append(np.frombuffer(item, dtype=np.uint8)[a:b])
                stream_off += b - a
            if size is None:
                size = hw
            elif hw != size:
                raise ValueError("the frames of one sample differ in size: %r and %r" % (size, hw))
            rgb_off += hw[0] * hw[1] * 3
        rows.append((first, size[0], size[1], len(frames)))
        labels.append(int(label))
    n, nh, nq = len(records), len(htabs), len(qtabs)
    if nh > 65535 or nq > 65535:
        raise ValueError("more than 65535 distinct tables in one batch")
    frames_arr = np.stack(records) if n else np.zeros(0, dtype=FRAME_DTYPE)
    o_frames = 0
    o_huff = _align16(o_frames + n * FRAME_DTYPE.itemsize)
    o_quant = _align16(o_huff + nh * HUFF_DTYPE.itemsize)
    o_stream = _align16(o_quant + nq * 128)
    blob = np.zeros(o_stream + stream_off, dtype=np.uint8)
    blob[o_frames:o_frames + n * 64] = frames_arr.view(np.uint8).reshape(-1)
    if nh:
        blob[o_huff:o_huff + nh * HUFF_DTYPE.itemsize] = np.stack(htabs).view(np.uint8).reshape(-1)
    if nq:
        blob[o_quant:o_quant + nq * 128] = np.stack(qtabs).astype("<u2").view(np.uint8).reshape(-1)
    at = o_stream
    for seg in segments:
        blob[at:at + seg.size] = seg
        at += seg.size
    layout = torch.tensor([n, nh, nq, o_frames, o_huff, o_quant, o_stream, stream_off], dtype=torch.int64)
    return PackedJpeg(torch.from_numpy(blob), layout, torch.tensor(rows, dtype=torch.int64).reshape(-1, 4),
                      torch.tensor(labels, dtype=torch.int64), rgb_off, workspace_bytes_for(frames_arr), fallback)


# ------------------------------------------------------------------------------------------------- launch
def launch_decode(streams, frames, qtabs, htabs, n, rgb, workspace, status, nq=None, nh=None):
    """rk_jpeg_decode_u8 on the current stream.  Device tensors: streams uint8 [stream_bytes] (any alignment), frames
    uint8 [n * 64] (rk_jpeg_frame records), qtabs uint8 [nq * 128], htabs uint8 [nh * 1424], rgb uint8 [rgb_bytes],
    workspace uint8 (16-byte aligned), status int32 [n + 1].  Nothing is allocated and the host does not wait."""
    from . import _native
    _check_tensors(((name, t, torch.uint8) for name, t in (("streams", streams), ("frames", frames), ("qtabs", qtabs),
                                                           ("htabs", htabs), ("rgb", rgb), ("workspace", workspace))),
                   say=lambda dt: "uint8")
    if status.dtype != torch.int32 or not status.is_cuda or status.numel() < n + 1 or not status.is_contiguous():
        raise ValueError("status must be int32 [n + 1] on the GPU")
    if frames.numel() < n * FRAME_DTYPE.itemsize:
        raise ValueError("%d bytes of frame records for n = %d" % (frames.numel(), n))
    nq = qtabs.numel() // 128 if nq is None else nq
    nh = htabs.numel() // HUFF_DTYPE.itemsize if nh is None else nh
    if qtabs.numel() < nq * 128 or htabs.numel() < nh * HUFF_DTYPE.itemsize:
        raise ValueError("the table arenas are shorter than nq / nh say")
    _native.launch("rk_jpeg_decode_u8", rgb.device, streams.data_ptr(), streams.numel(), frames.data_ptr(), qtabs.data_ptr(),
                   htabs.data_ptr(), nq, nh, n, rgb.data_ptr(), rgb.numel(), workspace.data_ptr(), workspace.numel(),
                   status.data_ptr())


# ------------------------------------------------------------------------------------------------- resident sets
ENTRY_DTYPE = np.dtype([("bit_pos", "<i8"), ("pred", "<i2", 3), ("reserved", "<i2")])      # rk_jpeg_entry
assert ENTRY_DTYPE.itemsize == 16
MAX_LAUNCH = 65535                                          # frames per build call, picks per decode call

ResidentJpeg = collections.namedtuple("ResidentJpeg", [
    "blob",             # uint8: the records of every device-decoded frame, tables, streams -- PackedJpeg's blob and layout
    "layout",
    "seg_mcus",         # int32 [n]: E of each record (default: its MCUs per row)
    "entry_off",        # int64 [n + 1]: exclusive sum of the records' segment counts ceil(nmcu / E)
    "segments",         # int64 [n]: those counts
    "videos",           # int64 [V, 4]: first slot, frame count, H, W; frame k of video v is slot videos[v, 0] + k
    "slots",            # int64 [slots]: the slot's record, or -1 - f for the f-th host-decoded frame
    "fallback",         # [uint8 [H, W, 3]]: the frames parse_jpeg refused, decoded here with Pillow
    "labels",           # int64 [V]
])


def pack_resident(videos, seg_mcus=None):
    """A set of videos for rk_jpeg_build_index / rk_jpeg_decode_indexed_u8.  videos: [(frames, label)] as pack_jpeg_clips
    takes them (a frame: the bytes of its file, or uint8 [H, W, 3]); all frames of a video share one size (ValueError
    otherwise).  seg_mcus: MCUs per segment -- None: one MCU row; an int: that for every frame; or one per device-decoded
    frame.  Returns a ResidentJpeg: pack_jpeg_clips' blob (records, de-duplicated tables, streams; rgb_off is 0, a
    resident frame gets its place when it is picked) and the index tables.  Files parse_jpeg refuses are decoded here,
    once, and stay RGB."""
    packed = pack_jpeg_clips(videos)
    rec = records(packed.blob, packed.layout)
    n = rec.size
    host = {int(off): i for i, (off, _) in enumerate(packed.fallback)}
    rows, slots, r = [], [], 0
    for off, h, w, k in packed.clips.tolist():
        rows.append((len(slots), k, h, w))
        for j in range(k):
            at = off + j * h * w * 3
            if at in host:
                slots.append(-1 - host[at])
            else:
                slots.append(r)
                r += 1
    assert r == n
    rec["rgb_off"][:] = 0
    _, mcux, mcuy, _ = _geometry(rec)
    E = mcux.copy() if seg_mcus is None else np.broadcast_to(np.asarray(seg_mcus, dtype=np.int64), (n,)).copy()
    if n and (E.min() < 1 or E.max() >= 1 << 31):
        raise ValueError("seg_mcus must be at least 1")
    segments = (mcux * mcuy + E - 1) // E
    entry_off = np.concatenate([[0], np.cumsum(segments)]).astype(np.int64)
    return ResidentJpeg(packed.blob, packed.layout, torch.from_numpy(E.astype(np.int32)), torch.from_numpy(entry_off),
                        torch.from_numpy(segments.astype(np.int64)), torch.tensor(rows, dtype=torch.int64).reshape(-1, 4),
                        torch.tensor(slots, dtype=torch.int64), [frame for _, frame in packed.fallback], packed.labels)


DeviceIndex = collections.namedtuple("DeviceIndex", [
    "blob", "frames", "htabs", "qtabs", "streams", "n", "nh", "nq",      # the resident blob on the device and its sections
    "seg_mcus", "entry_off", "entries", "n_entries",                     # int32 [n], int64 [n + 1], uint8 [n_entries * 16]
    "status",                                                            # int32 [n + 1]: the build's codes, [n] their count
    "route",                                                             # method="chunked": int32 [n], 0 where the sequential
], defaults=(None,))                                                     # walk gave the frame's result, else the rounds; or None

CHUNK_BYTES = (16, 32, 64, 128, 256, 512)                   # what rk_jpeg_build_index_chunked takes
MAX_ROUNDS = 64
MAX_CHUNKS = 4096                                           # a frame with more chunks takes the sequential walk


def _check_chunking(chunk_bytes, max_rounds):
    if chunk_bytes not in CHUNK_BYTES:
        raise ValueError("chunk_bytes must be one of %r, got %r" % (CHUNK_BYTES, chunk_bytes))
    if not 0 <= int(max_rounds) <= MAX_ROUNDS:
        raise ValueError("max_rounds must be in [0, %d], got %r" % (MAX_ROUNDS, max_rounds))


def chunked_workspace_bytes_for(frames, chunk_bytes):
    """rk_jpeg_chunked_workspace_bytes of a FRAME_DTYPE array, in numpy: an offset table, then 32 bytes per chunk of every
    frame that can take the chunked route (no restart interval, 1 .. MAX_CHUNKS chunks)."""
    f = np.asarray(frames).reshape(-1)
    if f.size < 1 or chunk_bytes not in CHUNK_BYTES:
        return 0
    length = f["stream_len"].astype(np.int64)
    ok = (f["restart_interval"] == 0) & (length >= 1) & (length <= chunk_bytes * MAX_CHUNKS)
    chunks = np.where(ok, (length + chunk_bytes - 1) // chunk_bytes, 0)
    return (((f.size + 1) * 8 + 15) & ~15) + int(chunks.sum()) * 32


def launch_build_index_chunked(streams, frames, htabs, nq, nh, n, seg_mcus, entry_off, entries, n_entries, chunk_bytes, max_rounds,
                               workspace, status, route):
    """rk_jpeg_build_index_chunked on the current stream.  Device tensors: streams, frames, htabs, entries (16-byte entries,
    8-byte aligned), workspace (16-byte aligned) uint8; seg_mcus int32 [n], entry_off int64 [n + 1], status int32 [n + 1],
    route int32 [n].  Nothing is allocated and the host does not wait."""
    from . import _native
    _check_tensors((("streams", streams, torch.uint8), ("frames", frames, torch.uint8), ("htabs", htabs, torch.uint8),
                    ("entries", entries, torch.uint8), ("workspace", workspace, torch.uint8), ("seg_mcus", seg_mcus, torch.int32),
                    ("entry_off", entry_off, torch.int64), ("status", status, torch.int32), ("route", route, torch.int32)))
    _check_chunking(chunk_bytes, max_rounds)
    if frames.numel() < n * 64 or seg_mcus.numel() < n or entry_off.numel() < n + 1 or status.numel() < n + 1 or route.numel() < n:
        raise ValueError("frames, seg_mcus, entry_off, status or route is shorter than n = %d asks for" % n)
    if entries.numel() < n_entries * ENTRY_DTYPE.itemsize or htabs.numel() < nh * HUFF_DTYPE.itemsize:
        raise ValueError("the entries or the table arena are shorter than n_entries / nh say")
    _native.launch("rk_jpeg_build_index_chunked", streams.device, streams.data_ptr(), streams.numel(), frames.data_ptr(),
                   htabs.data_ptr(), nq, nh, n, seg_mcus.data_ptr(), entry_off.data_ptr(), entries.data_ptr(), n_entries,
                   int(chunk_bytes), int(max_rounds), workspace.data_ptr(), workspace.numel(), status.data_ptr(), route.data_ptr())


def build_index(resident, device="cuda:0", method="chain", chunk_bytes=256, max_rounds=32):
    """Upload a ResidentJpeg and build its scan index (in chunks of 65535 frames, current stream).  method="chain": the one
    sequential walk per frame of rk_jpeg_build_index.  method="chunked": rk_jpeg_build_index_chunked -- walks of chunk_bytes
    each in lock-step rounds, at most max_rounds of them, the sequential walk for the frames that do not take that route;
    the same entries and codes, and `route` says which frames went which way.  Returns a DeviceIndex; nothing waits for
    the device."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("build_index runs on a GPU (no CPU path)")
    if method not in ("chain", "chunked"):
        raise ValueError("method must be 'chain' or 'chunked', got %r" % (method,))
    if method == "chunked":
        _check_chunking(chunk_bytes, max_rounds)
    from . import _native
    blob = resident.blob.to(device)
    (frames, htabs, qtabs, streams), (n, nh, nq) = sections(blob, resident.layout)
    n_entries = int(resident.entry_off[-1])
    seg_mcus, entry_off = resident.seg_mcus.to(device), resident.entry_off.to(device)
    entries = torch.zeros(max(n_entries, 1) * ENTRY_DTYPE.itemsize // 8, dtype=torch.int64, device=device).view(torch.uint8)
    status = torch.zeros(n + 1, dtype=torch.int32, device=device)
    route = torch.zeros(n, dtype=torch.int32, device=device) if method == "chunked" else None
    if method == "chunked":
        rec = records(resident.blob, resident.layout)
    for lo in range(0, n, MAX_LAUNCH):
        k = min(MAX_LAUNCH, n - lo)
        part = torch.zeros(k + 1, dtype=torch.int32, device=device)
        if method == "chunked":
            ws = torch.empty(chunked_workspace_bytes_for(rec[lo:lo + k], chunk_bytes), dtype=torch.uint8, device=device)
            launch_build_index_chunked(streams, frames[lo * 64:], htabs, nq, nh, k, seg_mcus[lo:], entry_off[lo:], entries, n_entries,
                                       chunk_bytes, max_rounds, ws, part, route[lo:])
        else:
            _native.launch("rk_jpeg_build_index", device, streams.data_ptr(), streams.numel(),
                           frames[lo * 64:].data_ptr(), htabs.data_ptr(), nq, nh, k, seg_mcus[lo:].data_ptr(),
                           entry_off[lo:].data_ptr(), entries.data_ptr(), n_entries, part.data_ptr())
        status[lo:lo + k].copy_(part[:k])
        status[n] += part[k]
    return DeviceIndex(blob, frames, htabs, qtabs, streams, n, nh, nq, seg_mcus, entry_off, entries, n_entries, status, route)


PickTables = collections.namedtuple("PickTables", [
    "pick",             # int32 [m]: the records to decode, each once
    "rgb_off",          # int64 [m]: where each goes in the batch's RGB arena
    "clips",            # int64 [B, 4]: the arena's rows for augment.ragged_u8_to_clips (offset, H, W, distinct frames)
    "frame_idx",        # per video: int64 array, the given frame numbers remapped into that video's frames of the arena
    "fallback",         # [(index in resident.fallback, offset in the arena)]
    "rgb_bytes",
    "max_segments",     # the largest segment count among the picked records (at least 1)
])


def pick_tables(resident, video_ids, frame_numbers_per_video):
    """The tables of one batch, on the host.  video_ids: the batch's videos; frame_numbers_per_video: for each, the 0-based
    frames its clips read.  A frame repeated inside a video's sample (short videos) is decoded once: the arena holds every
    video's distinct frames in order of first use, back to back, and frame_idx says where each asked-for frame went."""
    pick, rgb_off, rows, remapped, fallback, at, most = [], [], [], [], [], 0, 1
    videos, slots, segments = resident.videos.numpy(), resident.slots.numpy(), resident.segments.numpy()   # views, no copies
    for v, numbers in zip(video_ids, frame_numbers_per_video):
        first, count, h, w = (int(x) for x in videos[int(v)])
        place, local = {}, []
        for p in (int(x) for x in numbers):
            if not 0 <= p < count:
                raise ValueError("frame %d of a video of %d frames" % (p, count))
            if p not in place:
                place[p] = len(place)
                slot = int(slots[first + p])
                off = at + place[p] * h * w * 3
                if slot < 0:
                    fallback.append((-1 - slot, off))
                else:
                    pick.append(slot)
                    rgb_off.append(off)
                    most = max(most, int(segments[slot]))
            local.append(place[p])
        rows.append((at, h, w, len(place)))
        remapped.append(np.asarray(local, dtype=np.int64))
        at += len(place) * h * w * 3
    return PickTables(torch.tensor(pick, dtype=torch.int32), torch.tensor(rgb_off, dtype=torch.int64),
                      torch.tensor(rows, dtype=torch.int64).reshape(-1, 4), remapped, fallback, at, most)


def _head_bytes(m, max_segments):
    return m * 64 + ((m * max_segments * 4 + 15) & ~15)


def indexed_workspace_bytes_for(frames, pick, max_segments, per_frame=None):
    """rk_jpeg_indexed_workspace_bytes of a FRAME_DTYPE array and a pick list, in numpy.  per_frame: frame_workspace_bytes
    of `frames`, where the caller keeps it."""
    frames, pick = np.asarray(frames).reshape(-1), np.asarray(pick, dtype=np.int64).reshape(-1)
    if frames.size < 1 or pick.size < 1 or max_segments < 1:
        return 0
    per_frame = frame_workspace_bytes(frames) if per_frame is None else per_frame
    inside = pick[(pick >= 0) & (pick < frames.size)]
    return _head_bytes(pick.size, int(max_segments)) + (((pick.size + 1) * 8 + 15) & ~15) + int(per_frame[inside].sum())


def launch_decode_indexed(index, pick, rgb_off, max_segments, rgb, workspace, status):
    """rk_jpeg_decode_indexed_u8 on the current stream.  index: a DeviceIndex; pick int32 [m], rgb_off int64 [m], rgb uint8
    [rgb_bytes], workspace uint8 (16-byte aligned), status int32 [m + 1]: device tensors.  Nothing is allocated and the
    host does not wait."""
    from . import _native
    m = pick.numel()
    _check_tensors((("pick", pick, torch.int32), ("rgb_off", rgb_off, torch.int64), ("rgb", rgb, torch.uint8),
                    ("workspace", workspace, torch.uint8), ("status", status, torch.int32)))
    if rgb_off.numel() != m or status.numel() < m + 1:
        raise ValueError("pick [%d], rgb_off [%d], status [%d]: want m, m, m + 1" % (m, rgb_off.numel(), status.numel()))
    _native.launch("rk_jpeg_decode_indexed_u8", rgb.device, index.streams.data_ptr(), index.streams.numel(),
                   index.frames.data_ptr(), index.qtabs.data_ptr(), index.htabs.data_ptr(), index.nq, index.nh, index.n,
                   index.entries.data_ptr(), index.n_entries, index.entry_off.data_ptr(), index.seg_mcus.data_ptr(),
                   index.status.data_ptr(), pick.data_ptr(), rgb_off.data_ptr(), m, int(max_segments), rgb.data_ptr(),
                   rgb.numel(), workspace.data_ptr(), workspace.numel(), status.data_ptr())


# ------------------------------------------------------------------------------------------------- packed coefficients
DeviceCoef = collections.namedtuple("DeviceCoef", [
    "blob",             # uint8 on the device: every frame's region (offset table, block records), back to back in its first
                        # packed_bytes bytes; what the estimate left over follows
    "region_off",       # int64 [n + 1] on the device: frame i's region is blob[region_off[i]:region_off[i + 1]]
    "frames", "qtabs",  # uint8 on the device: the n records and the quantisation tables
    "n", "nq",
    "status",           # int32 [n + 1] on the device: the entropy stage's code per frame, [n] their count
    "packed_bytes",     # bytes of all regions
    "file_bytes",       # bytes of the same frames' entropy-coded segments, what resident="jpeg" would keep of them
    "build_bytes",      # the most the build held on the device beside the blob and the tables (one slab's buffers)
    "record",           # "wide" or "dense": the record format of the blob (RK_JPEG_COEF_WIDE / RK_JPEG_COEF_DENSE)
], defaults=("wide",))

COEF_RECORD_MIN, COEF_RECORD_MAX = 10, 136
COEF_DENSE_RECORD_MIN, COEF_DENSE_RECORD_MAX, COEF_DENSE_GROUP = 4, 130, 64
COEF_RECORDS = {"wide": 0, "dense": 1}


def coef_region_bounds(record, nblocks):
    """(least, most) bytes of one frame's region of nblocks blocks in record format `record`, the table included
    (rk_jpeg_coef_region_bounds, in Python)."""
    if record not in COEF_RECORDS:
        raise ValueError("record must be 'wide' or 'dense', got %r" % (record,))
    nblocks = int(nblocks)
    if record == "dense":
        table = 4 * ((nblocks + COEF_DENSE_GROUP - 1) // COEF_DENSE_GROUP) + 2 * nblocks
        return table + nblocks * COEF_DENSE_RECORD_MIN, table + nblocks * COEF_DENSE_RECORD_MAX
    return nblocks * (4 + COEF_RECORD_MIN), nblocks * (4 + COEF_RECORD_MAX)


def frame_plane_bytes(frames):
    """int64 per record of a FRAME_DTYPE array: the bytes of its component planes in rk_jpeg_decode_coef_u8's workspace
    (64 per block, rounded up to 16; 0 for sizes that are not valid)."""
    blocks = _geometry_blocks(frames)[3]
    return _align16(blocks * 192) - blocks * 128


def coef_workspace_bytes_for(frames, pick, per_frame=None):
    """rk_jpeg_coef_workspace_bytes of a FRAME_DTYPE array and a pick list, in numpy: the gathered records, a flag per
    picked frame, the offset table, the picked frames' planes.  per_frame: frame_plane_bytes of `frames`, where the
    caller keeps it."""
    frames, pick = np.asarray(frames).reshape(-1), np.asarray(pick, dtype=np.int64).reshape(-1)
    if frames.size < 1 or pick.size < 1:
        return 0
    per_frame = frame_plane_bytes(frames) if per_frame is None else per_frame
    inside = pick[(pick >= 0) & (pick < frames.size)]
    return pick.size * 64 + _align16(pick.size * 4) + _align16((pick.size + 1) * 8) + int(per_frame[inside].sum())


def _as_bytes(arr, device):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to(device)


def build_coef(resident, device="cuda:0", method="chain", slab_frames=256, chunk_bytes=256, max_rounds=32, admit=None,
               record="wide"):
    """A ResidentJpeg transcoded on the device into packed DCT coefficients (rk_jpeg_coef_sizes, rk_jpeg_coef_pack): every
    frame's Huffman code is undone once, here.  The set goes through in slabs of slab_frames frames: a slab's file bytes
    and records are uploaded, its entropy stage runs -- method="chain": one chain per frame; method="chunked": the scan
    index of the slab from rk_jpeg_build_index_chunked (chunk_bytes, max_rounds), then one chain per segment -- its blocks
    are measured, the host reads the slab's total, and the records are written behind those of the slabs before it;
    then the slab's buffers are dropped, so the file bytes, the index entries and the 128-byte-per-block workspace never
    exist for more than one slab.  The blob is allocated once the first slab is measured, at that slab's bytes per frame
    for the whole set plus 3 % (and again, larger, should a later slab not fit).  admit(bytes): called before every
    allocation with the bytes the build is about to hold on the device (the blob included); it may raise.
    record="dense" packs the denser records (rk_jpeg_coef_sizes_as / rk_jpeg_coef_pack_as with RK_JPEG_COEF_DENSE: a
    nibble per small AC value, a byte or a word only for the few large ones, a table of half the size); the build is
    otherwise the same and the DeviceCoef remembers its format.  Returns a DeviceCoef.  The host waits once per slab."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("build_coef runs on a GPU (no CPU path)")
    if method not in ("chain", "chunked"):
        raise ValueError("method must be 'chain' or 'chunked', got %r" % (method,))
    if not 1 <= int(slab_frames) <= MAX_LAUNCH:
        raise ValueError("slab_frames must be in [1, %d], got %r" % (MAX_LAUNCH, slab_frames))
    if method == "chunked":
        _check_chunking(chunk_bytes, max_rounds)
    if record not in COEF_RECORDS:
        raise ValueError("record must be 'wide' or 'dense', got %r" % (record,))
    from . import _native
    admit = admit or (lambda held: None)
    (frames_h, htabs_h, qtabs_h, streams_h), (n, nh, nq) = sections(resident.blob, resident.layout)
    rec = records(resident.blob, resident.layout).copy()
    blocks = _geometry_blocks(rec)[3]
    fixed = frames_h.numel() + qtabs_h.numel() + (n + 1) * 12
    admit(fixed + htabs_h.numel())
    frames, qtabs, htabs = frames_h.to(device), qtabs_h.to(device), htabs_h.to(device)
    region_off = torch.zeros(n + 1, dtype=torch.int64, device=device)
    status = torch.zeros(n + 1, dtype=torch.int32, device=device)
    blob, room, done, most_held = None, 0, 0, 0
    for lo in range(0, n, int(slab_frames)):
        hi = min(n, lo + int(slab_frames))
        k = hi - lo
        slab = rec[lo:hi].copy()
        first = int(slab["stream_off"].min())
        last = int((slab["stream_off"] + slab["stream_len"]).max())
        slab["stream_off"] -= first
        most = int(resident.segments[lo:hi].max()) if method == "chunked" else 1
        ws_bytes = indexed_workspace_bytes_for(slab, np.arange(k), most)
        cap = max(int(blocks[lo:hi].sum()), 1)
        held = (last - first) + k * 64 + ws_bytes + cap * 4 + (k + 1) * 20
        if method == "chunked":
            eo = (resident.entry_off[lo:hi + 1] - resident.entry_off[lo]).contiguous()
            n_entries = int(eo[-1])
            build_ws_bytes = chunked_workspace_bytes_for(slab, chunk_bytes)
            held += max(n_entries, 1) * 16 + build_ws_bytes + k * 16 + 12
        admit(fixed + htabs_h.numel() + room + held)
        most_held = max(most_held, held)
        streams = streams_h[first:last].to(device) if last > first else torch.zeros(1, dtype=torch.uint8, device=device)
        slab_d = _as_bytes(slab, device)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        block_off = torch.empty(cap, dtype=torch.int32, device=device)
        first_block = torch.empty(k + 1, dtype=torch.int64, device=device)
        rel = torch.empty(k + 1, dtype=torch.int64, device=device)
        part_status = torch.zeros(k + 1, dtype=torch.int32, device=device)
        index = (None, 0, None, None, None)
        if method == "chunked":
            seg_mcus, entry_off = resident.seg_mcus[lo:hi].contiguous().to(device), eo.to(device)
            entries = torch.zeros(max(n_entries, 1) * 2, dtype=torch.int64, device=device).view(torch.uint8)
            build_status = torch.zeros(k + 1, dtype=torch.int32, device=device)
            route = torch.zeros(k, dtype=torch.int32, device=device)
            launch_build_index_chunked(streams, slab_d, htabs, nq, nh, k, seg_mcus, entry_off, entries, n_entries, chunk_bytes,
                                       max_rounds, torch.empty(build_ws_bytes, dtype=torch.uint8, device=device), build_status,
                                       route)
            index = (entries.data_ptr(), n_entries, entry_off.data_ptr(), seg_mcus.data_ptr(), build_status.data_ptr())
        _native.launch("rk_jpeg_coef_sizes_as", device, streams.data_ptr(), streams.numel(), slab_d.data_ptr(), htabs.data_ptr(), nq,
                       nh, k, *index, most, ws.data_ptr(), ws.numel(), part_status.data_ptr(), block_off.data_ptr(), cap,
                       first_block.data_ptr(), rel.data_ptr(), after=(COEF_RECORDS[record],))
        total = int(rel[k].item())                      # the host waits here, once per slab
        if blob is None or done + total > room:
            # the blob is one allocation that the slabs fill in turn: its size is the first slab's bytes a frame carried over
            # to the whole set, with 3 % to spare (the last slab knows the size); where a later slab still does not fit,
            # a larger one takes over what is packed so far -- only then do two blobs exist at once
            want = max(_align16(int((done + total) * (1.0 if hi == n else 1.03 * n / hi))), 16)
            admit(fixed + htabs_h.numel() + room + held + want)
            grown = torch.empty(want, dtype=torch.uint8, device=device)
            if done:
                grown[:done].copy_(blob[:done])
            blob, room = grown, want
            del grown
        rel += done
        _native.launch("rk_jpeg_coef_pack_as", device, slab_d.data_ptr(), k, most, ws.data_ptr(), ws.numel(), part_status.data_ptr(),
                       block_off.data_ptr(), cap, first_block.data_ptr(), rel.data_ptr(), blob.data_ptr(), room,
                       after=(COEF_RECORDS[record],))
        region_off[lo:hi + 1].copy_(rel)
        status[lo:hi].copy_(part_status[:k])
        status[n] += part_status[k]
        done += total
        torch.cuda.current_stream(device).synchronize()   # the slab's buffers go back before the next slab asks for its own
        del streams, slab_d, ws, block_off, first_block, rel, part_status, index
    del htabs
    if blob is None:                                    # no frame at all: sixteen bytes that no region lies in
        blob = torch.zeros(16, dtype=torch.uint8, device=device)
    return DeviceCoef(blob, region_off, frames, qtabs, n, nq, status, done, int(rec["stream_len"].sum()), most_held, record)


def launch_decode_coef(coef, pick, rgb_off, rgb, workspace, status):
    """rk_jpeg_decode_coef_as_u8, in the DeviceCoef's record format, on the current stream.  coef: a DeviceCoef; pick
    int32 [m], rgb_off int64 [m], rgb uint8 [rgb_bytes], workspace uint8 (16-byte aligned, coef_workspace_bytes_for), status int32 [m + 1]: device tensors.  Nothing
    is allocated and the host does not wait."""
    from . import _native
    m = pick.numel()
    _check_tensors((("pick", pick, torch.int32), ("rgb_off", rgb_off, torch.int64), ("rgb", rgb, torch.uint8),
                    ("workspace", workspace, torch.uint8), ("status", status, torch.int32)))
    if rgb_off.numel() != m or status.numel() < m + 1:
        raise ValueError("pick [%d], rgb_off [%d], status [%d]: want m, m, m + 1" % (m, rgb_off.numel(), status.numel()))
    _native.launch("rk_jpeg_decode_coef_as_u8", rgb.device, coef.blob.data_ptr(), coef.packed_bytes, coef.frames.data_ptr(),
                   coef.qtabs.data_ptr(), coef.nq, coef.n, coef.region_off.data_ptr(), coef.status.data_ptr(), pick.data_ptr(),
                   rgb_off.data_ptr(), m, rgb.data_ptr(), rgb.numel(), workspace.data_ptr(), workspace.numel(),
                   status.data_ptr(), after=(COEF_RECORDS[coef.record],))


# ------------------------------------------------------------------------------------------------- a streamed batch by rows
RowTables = collections.namedtuple("RowTables", [
    "tables",           # uint8: seg_mcus int32 [n] | entry_off int64 [n + 1] | pick int32 [n] | rgb_off int64 [n], 16-byte aligned
    "offsets",          # the four sections' byte offsets in `tables`
    "n", "n_entries", "max_segments",
    "build_bytes",      # rk_jpeg_chunked_workspace_bytes of the records
    "decode_bytes",     # rk_jpeg_indexed_workspace_bytes of the records, each picked once
])


def row_tables(frames, chunk_bytes=256):
    """The index tables of a batch's own records, on the host (a FRAME_DTYPE array; n >= 1): one segment per MCU row --
    seg_mcus is the MCUs per row and entry_off its rows' exclusive sum -- every record picked once, in order, to its own
    rgb_off; and the two workspace sizes, in numpy (a DataLoader worker does not load the HIP library).  A record whose
    sizes are not valid gets one segment of one MCU; the build refuses it from its fields."""
    f = np.asarray(frames).reshape(-1)
    n = f.size
    _, mcux, mcuy, per_frame = _geometry(f)
    entry_off = np.concatenate([[0], np.cumsum(mcuy)]).astype(np.int64)
    parts = (mcux.astype(np.int32), entry_off, np.arange(n, dtype=np.int32), f["rgb_off"].astype(np.int64))
    offsets, at = [], 0
    for part in parts:
        offsets.append(at)
        at = _align16(at + part.nbytes)
    tables = np.zeros(at, dtype=np.uint8)
    for off, part in zip(offsets, parts):
        tables[off:off + part.nbytes] = part.view(np.uint8)
    most = int(mcuy.max())
    return RowTables(torch.from_numpy(tables), tuple(offsets), n, int(entry_off[-1]), most,
                     chunked_workspace_bytes_for(f, chunk_bytes), indexed_workspace_bytes_for(f, parts[2], most, per_frame))


def launch_decode_rows(streams, frames, qtabs, htabs, nq, nh, rows, tables, entries, build_ws, build_status, route, rgb,
                       decode_ws, status, chunk_bytes=256, max_rounds=32):
    """A batch decoded by MCU row on the current stream: rk_jpeg_build_index_chunked over the batch's own records, then
    rk_jpeg_decode_indexed_u8 of every record to its own place.  rows: row_tables of the records; tables: rows.tables on
    the device (16-byte aligned); entries uint8 [rows.n_entries * 16] (8-byte aligned), build_ws / decode_ws uint8
    (rows.build_bytes / rows.decode_bytes, 16-byte aligned), build_status int32 [n + 1], route int32 [n], status int32
    [n + 1]: device tensors.  Eleven launches, one linear chain; nothing is allocated and the host does not wait."""
    n = rows.n
    o_seg, o_off, o_pick, o_rgb = rows.offsets
    seg_mcus = tables[o_seg:o_seg + 4 * n].view(torch.int32)
    entry_off = tables[o_off:o_off + 8 * (n + 1)].view(torch.int64)
    pick = tables[o_pick:o_pick + 4 * n].view(torch.int32)
    rgb_off = tables[o_rgb:o_rgb + 8 * n].view(torch.int64)
    launch_build_index_chunked(streams, frames, htabs, nq, nh, n, seg_mcus, entry_off, entries, rows.n_entries, chunk_bytes,
                               max_rounds, build_ws, build_status, route)
    index = DeviceIndex(None, frames, htabs, qtabs, streams, n, nh, nq, seg_mcus, entry_off, entries, rows.n_entries,
                        build_status, route)
    launch_decode_indexed(index, pick, rgb_off, rows.max_segments, rgb, decode_ws, status)


def decode_jpeg_frames(packed, device="cuda:0", out=None, workspace=None, entropy="chain", chunk_bytes=256, max_rounds=32):
    """Decode one packed batch on `device` (current stream).  Returns (rgb arena uint8 [rgb_bytes], clips, status int32
    [n + 1]): the arena and `clips` are what augment.ragged_u8_to_clips takes.  out / workspace: device uint8 tensors to
    use (at least rgb_bytes / workspace_bytes long).  Frames that travelled as RGB are copied into the arena; status
    covers the device-decoded frames in order, status[n] counts those that failed (zero frames).
    entropy="chain": rk_jpeg_decode_u8, one Huffman chain per frame.  entropy="rows": one chain per MCU row -- the scan
    index of the batch's own records is built on the device by rk_jpeg_build_index_chunked (chunk_bytes, max_rounds) and
    rk_jpeg_decode_indexed_u8 decodes by it; the same arena and the same codes.  workspace must then hold the
    decoder's row_tables(...).decode_bytes; the build's buffers are allocated here."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("decode_jpeg_frames decodes on a GPU (no CPU path)")
    if entropy not in ("chain", "rows"):
        raise ValueError("entropy must be 'chain' or 'rows', got %r" % (entropy,))
    if entropy == "rows":
        _check_chunking(chunk_bytes, max_rounds)
    (frames, htabs, qtabs, streams), (n, nh, nq) = sections(packed.blob.to(device), packed.layout)
    rgb = torch.empty(packed.rgb_bytes, dtype=torch.uint8, device=device) if out is None else out[:packed.rgb_bytes]
    if rgb.numel() < packed.rgb_bytes:
        raise ValueError("out holds %d bytes, the batch decodes to %d" % (rgb.numel(), packed.rgb_bytes))
    status = torch.zeros(n + 1, dtype=torch.int32, device=device)
    if n and entropy == "rows":
        rows = row_tables(records(packed.blob, packed.layout), chunk_bytes)
        if workspace is None:
            workspace = torch.empty(rows.decode_bytes, dtype=torch.uint8, device=device)
        elif workspace.numel() < rows.decode_bytes:
            raise ValueError("workspace holds %d bytes, the decode by rows needs %d" % (workspace.numel(), rows.decode_bytes))
        entries = torch.empty(max(rows.n_entries, 1) * 2, dtype=torch.int64, device=device).view(torch.uint8)
        launch_decode_rows(streams, frames, qtabs, htabs, nq, nh, rows, rows.tables.to(device), entries,
                           torch.empty(rows.build_bytes, dtype=torch.uint8, device=device),
                           torch.zeros(n + 1, dtype=torch.int32, device=device), torch.zeros(n, dtype=torch.int32, device=device),
                           rgb, workspace, status, chunk_bytes, max_rounds)
    elif n:
        if workspace is None:
            workspace = torch.empty(packed.workspace_bytes, dtype=torch.uint8, device=device)
        launch_decode(streams, frames, qtabs, htabs, n, rgb, workspace, status, nq, nh)
    for off, frame in packed.fallback:
        rgb[off:off + frame.numel()].copy_(frame.reshape(-1))
    return rgb, packed.clips, status
