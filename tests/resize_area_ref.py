"""The project's statement of cv2.resize(..., interpolation=cv2.INTER_AREA) for a shrinking 8-bit image, following OpenCV's published
scalar code (resize.cpp: computeResizeAreaTab + ResizeArea_Invoker).  cv2 is absent here, so like the fillPoly / warpAffine / HSV
restatements this is unpinned against cv2; it is the reference dy_aug_resize_area_u8 is held to, byte for byte.

Per axis (source length S, destination length D, scale = S / D in float64), for d = 0 .. D - 1:
    f1 = d * scale, f2 = f1 + scale, cell = min(scale, S - f1)
    s1 = ceil(f1), s2 = min(floor(f2), S - 1), s1 = min(s1, s2)
    entries, in this order:  (s1 - 1, (s1 - f1) / cell)                    if s1 - f1 > 1e-3
                             (s, 1 / cell)                                  for s in [s1, s2)
                             (s2, min(min(f2 - s2, 1.0), cell) / cell)      if f2 - s2 > 1e-3
each weight computed in float64 and rounded once to float32.
Accumulation, all float32, in table order, multiply and add rounded separately:
    buf[sy][dx] = sum_x src[sy][sx] * ax      (buf starts at 0, x entries ascending)
    sum[dy][dx] = sum_y buf[sy][dx] * by      (y entries ascending)
Store: uint8(clamp(rint(sum), 0, 255)), rint = round half to even.

Exact integer ratios take the same table (every weight 1 / scale).  Known spot where real cv2 may differ by 1: its vectorised 2 x 2 path
computes (a + b + c + d + 2) >> 2, which rounds .5 ties up instead of to even."""
import math

import numpy as np

F32 = np.float32


def axis_table(S, D):
    """[(source index, float32 weight), ...] per destination index"""
    scale = S / D
    out = []
    for d in range(D):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, S - f1)
        s1 = math.ceil(f1)
        s2 = min(math.floor(f2), S - 1)
        s1 = min(s1, s2)
        e = []
        if s1 - f1 > 1e-3:
            e.append((s1 - 1, F32((s1 - f1) / cell)))
        for s in range(s1, s2):
            e.append((s, F32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            e.append((s2, F32(min(min(f2 - s2, 1.0), cell) / cell)))
        out.append(e)
    return out


def area_sums(src, dh, dw):
    """the float32 sums [dh, dw, C] before rounding"""
    src = np.asarray(src)
    sh, sw = src.shape[:2]
    if dh > sh or dw > sw:
        raise ValueError("INTER_AREA here is the shrinking rule: dh <= sh and dw <= sw")
    xt, yt = axis_table(sw, dw), axis_table(sh, dh)
    srcf = src.astype(F32)
    buf = np.zeros((sh, dw) + src.shape[2:], dtype=F32)
    for dx, entries in enumerate(xt):                        # a column of buf at a time: the same per-pixel order for every row
        for sx, a in entries:
            buf[:, dx] = buf[:, dx] + srcf[:, sx] * a
    out = np.zeros((dh, dw) + src.shape[2:], dtype=F32)
    for dy, entries in enumerate(yt):
        for sy, b in entries:
            out[dy] = out[dy] + buf[sy] * b
    return out


def resize_area_u8(src, dh, dw):
    return np.clip(np.rint(area_sums(src, dh, dw)), 0, 255).astype(np.uint8)


def load_image_shape(h0, w0, imgsz):
    """(h, w) BaseDataset.load_image resizes to (base.py:153-156)"""
    r = imgsz / max(h0, w0)
    return min(math.ceil(h0 * r), imgsz), min(math.ceil(w0 * r), imgsz)


def exact_box(src, dh, dw):
    """float64 box integration of the piecewise-constant image over each destination cell (independent of the tables above)"""
    src = np.asarray(src, dtype=np.float64)
    sh, sw = src.shape[:2]

    def overlap(S, D):
        edges = np.arange(D + 1, dtype=np.float64) * (S / D)
        lo = np.maximum(edges[:-1, None], np.arange(S)[None, :])
        hi = np.minimum(edges[1:, None], np.arange(S)[None, :] + 1.0)
        return np.clip(hi - lo, 0, None) / (S / D)           # [D, S], rows sum to 1
    wy, wx = overlap(sh, dh), overlap(sw, dw)
    rows = np.tensordot(wy, src, axes=(1, 0))                 # [dh, sw, C]
    return np.einsum("dx,yxc->ydc", wx, rows)
