"""Plain-numpy statement of the polygon-mask rule of csrc/polymask.hip ("Polygon masks").  TEST INFRASTRUCTURE.

The reference rasterises with cv2.fillPoly and shrinks with cv2.resize (ultralytics/data/utils.py:137-155); cv2 is not available, so the
rule is the project's own restatement:
  * full-resolution pixel (x, y) is set iff the integer point lies in the CLOSED polygon: inside by the even-odd rule, or on one of its
    edges (closing edge included).  Written here PER PIXEL with integer cross products -- a crossing count and a collinearity test --
    not as the kernel's scanline toggles;
  * the mask at ratio r is oracle.augment.cv_resize_linear_u8 of that plane;
  * polygons2masks_overlap (utils.py:173-190): area = set mask pixels, order by area descending with ties by original index (numpy's
    default argsort gives no rule for them), pixel = 1 + largest rank covering it.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.augment import cv_resize_linear_u8  # noqa: E402


def fill_closed(poly, h, w):
    """uint8 [h, w]: 1 where the integer point (x, y) is inside (even-odd) or on the boundary of the closed polygon `poly` [P, 2] ints"""
    p = np.asarray(poly).astype(np.int64).reshape(-1, 2)
    Y, X = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    odd = np.zeros((h, w), dtype=bool)
    on = np.zeros((h, w), dtype=bool)
    for k in range(len(p)):
        (x0, y0), (x1, y1) = p[k], p[(k + 1) % len(p)]
        cross = (x1 - x0) * (Y - y0) - (y1 - y0) * (X - x0)          # 0 on the edge's line
        on |= (cross == 0) & (X >= min(x0, x1)) & (X <= max(x0, x1)) & (Y >= min(y0, y1)) & (Y <= max(y0, y1))
        if y0 != y1:
            straddle = (y0 > Y) != (y1 > Y)
            # the ray to +x from (X, Y) meets the edge strictly right of the point: X < x0 + (Y - y0) (x1 - x0) / (y1 - y0)
            right = (cross > 0) if y1 > y0 else (cross < 0)
            odd ^= straddle & right
    return (odd | on).astype(np.uint8)


def polygon2mask(poly, h, w, ratio):
    """polygon2mask (utils.py:137-155) under the stated pixel rule: uint8 [h // ratio, w // ratio] 0/1"""
    if ratio != 1 and (ratio <= 0 or ratio % 2):
        raise ValueError("mask_ratio must be 1 or even")
    plane = fill_closed(poly, h, w)
    if ratio == 1:
        return plane
    return cv_resize_linear_u8(plane[..., None], (w // ratio, h // ratio))[..., 0]


def polygons2masks(polys, h, w, ratio):
    """polygons2masks (utils.py:158-170): uint8 [n, mh, mw]"""
    if len(polys) == 0:
        return np.zeros((0, h // ratio, w // ratio), np.uint8)
    return np.stack([polygon2mask(p, h, w, ratio) for p in polys])


def stable_order(areas):
    """area descending, ties by original index"""
    return np.argsort(-np.asarray(areas, dtype=np.int64), kind="stable")


def polygons2masks_overlap(polys, h, w, ratio):
    """polygons2masks_overlap (utils.py:173-190) with the stable order: (uint8 [mh, mw] index map, sorted_idx int64 [n], areas)"""
    if len(polys) > 255:
        raise NotImplementedError("more than 255 instances in one image")
    ms = polygons2masks(polys, h, w, ratio)
    areas = ms.reshape(len(ms), -1).sum(1).astype(np.int64)
    index = stable_order(areas)
    out = np.zeros((h // ratio, w // ratio), dtype=np.uint8)
    for rank, j in enumerate(index):                                 # later (smaller) instances overwrite: the largest rank wins
        out[ms[j] != 0] = rank + 1
    return out, index, areas


def batch_reference(polys, offsets, rows, h, w, ratio, overlap=True):
    """what DeviceAugmenter.polygon_masks returns for a packed batch: overlap -> (masks [B, mh, mw], rows permuted, perm int32
    [n_total]); else -> planes [n_total, mh, mw]"""
    polys, rows = np.asarray(polys), np.asarray(rows, dtype=np.float32).reshape(-1, 6)
    B = len(offsets) - 1
    if not overlap:
        return polygons2masks(polys, h, w, ratio)
    masks = np.zeros((B, h // ratio, w // ratio), np.uint8)
    rows_out, perm = rows.copy(), np.zeros(len(rows), np.int32)
    for b in range(B):
        o, e = int(offsets[b]), int(offsets[b + 1])
        if e > o:
            masks[b], idx, _ = polygons2masks_overlap(polys[o:e], h, w, ratio)
            perm[o:e] = idx
            rows_out[o:e] = rows[o:e][idx]
    return masks, rows_out, perm
