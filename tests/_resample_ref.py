"""Host restatement of the device crop / resize / flip / normalise definition (include/rubiks_hip.h,
rk_clip_resample_u8_*), in numpy: the reference the CPU and GPU tests of rubiksnet_amd.augment compare with.

The resampler is Pillow's 8-bit BILINEAR one restated from its definition: per axis, fp64 triangle-filter
coefficients of support max(in / out, 1) normalised by their left-to-right sum, integer weights
(int)(w * 2^22 + 0.5), out = clip8((2^21 + sum in * k) >> 22); horizontal pass first, to uint8, then vertical; a pass
whose lengths are equal is the identity.  tests/test_augment.py checks it byte for byte against PIL itself."""
import numpy as np

PRECISION_BITS = 22


def axis_coeffs(n, m):
    """[(xmin, int weights)] for each of the m output samples of an axis of n input samples."""
    scale = float(n) / float(m)
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    out = []
    for i in range(m):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)          # int() truncates towards zero, as the C cast does
        xmax = min(int(center + support + 0.5), n)
        w = []
        ww = 0.0
        for j in range(xmax - xmin):
            a = abs((j + xmin - center + 0.5) * ss)
            v = 1.0 - a if a < 1.0 else 0.0
            w.append(v)
            ww += v
        k = [int((v / ww if ww != 0.0 else v) * float(1 << PRECISION_BITS) + 0.5) for v in w]
        out.append((xmin, np.asarray(k, dtype=np.int64)))
    return out


def resample_axis0(img, m):
    """img uint8 [n, ...] -> uint8 [m, ...] along axis 0."""
    n = img.shape[0]
    if n == m:
        return img.copy()
    res = np.empty((m,) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int64)
    for i, (xmin, k) in enumerate(axis_coeffs(n, m)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, src[xmin:xmin + len(k)], axes=(0, 0))
        res[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return res


def resize_u8(img, rw, rh):
    """img uint8 [h, w, C] -> [rh, rw, C] as PIL's Image.resize((rw, rh), BILINEAR) does."""
    hor = resample_axis0(np.ascontiguousarray(img.transpose(1, 0, 2)), rw).transpose(1, 0, 2)     # horizontal first
    return resample_axis0(np.ascontiguousarray(hor), rh)


def frame_u8(frame, box, out_hw):
    """One source frame [Hs, Ws, 3] and one box -> the uint8 window [Sh, Sw, 3] (steps 1-4 of the definition)."""
    x0, y0, cw, ch, rw, rh, ox, oy, flip = (int(v) for v in box)
    sh, sw = out_hw
    win = resize_u8(frame[y0:y0 + ch, x0:x0 + cw], rw, rh)[oy:oy + sh, ox:ox + sw]
    assert win.shape[:2] == (sh, sw), (win.shape, box, out_hw)
    return win[:, ::-1] if flip else win


def normalise(u8_chw, mean, std):
    """((v / 255) - mean[c]) / std[c], every operation rounded in fp32.  u8_chw [..., 3, H, W]."""
    m = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    v = u8_chw.astype(np.float32) / np.float32(255.0)
    return ((v - m) / s).astype(np.float32)


def clips_u8(frames, boxes, out_hw, views=1):
    """frames uint8 [B, T, Hs, Ws, 3], boxes [B * V, 9] -> uint8 [B * V, T, 3, Sh, Sw]."""
    B, T = frames.shape[:2]
    boxes = np.asarray(boxes).reshape(B * views, 9)
    out = np.empty((B * views, T, 3) + tuple(out_hw), dtype=np.uint8)
    for oc in range(B * views):
        for t in range(T):
            out[oc, t] = frame_u8(frames[oc // views, t], boxes[oc], out_hw).transpose(2, 0, 1)
    return out


def clips_f32(frames, boxes, out_hw, views=1, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    return normalise(clips_u8(frames, boxes, out_hw, views), mean, std)
