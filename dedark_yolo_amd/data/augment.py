"""Training / validation transforms of the reference's data pipeline with the PIXEL work on the device.

Reference (host, per sample, cv2 + numpy in dataloader workers): ultralytics/data/base.py:142-169 load_image (resize so that the long
side is imgsz), ultralytics/data/augment.py `v8_transforms` :753-783 = Mosaic :118-216 -> CopyPaste(p=0) -> RandomPerspective :292-478 ->
MixUp :272-288 -> Albumentations (package absent: bookkeeping only) -> RandomHSV :480-499 -> RandomFlip x2 :502-537, then Format :697-751 and
YOLODataset.collate_fn (dataset.py:172-188).  Validation: LetterBox(scaleup=False) :540-603 + Format.

Here the split is:
  * `plan_train_sample` draws the random numbers in the reference's CALL ORDER from the same generators (`random`, `numpy.random`), so a
    run seeded like the reference picks the same mosaic partners, centre, affine matrix, HSV gains and flips (pinned by
    tests/golden/g13_augment.npz);
  * `train_labels` / `val_labels` move the boxes through the same float32 steps as the reference's Instances bookkeeping (a few dozen
    numbers per image: host numpy, like the reference);
  * the pixels never exist on the host in augmented form: `DeviceAugmenter` keeps the decoded uint8 images in HBM (or uploads them) and
    ONE kernel per batch (dy_aug_mosaic_warp; dy_aug_mosaic_warp_mix when hyp.mixup > 0: the partner's warped image is blended in before
    the HSV gains) samples mosaic canvas -> affine warp (cv2.warpAffine's fixed-point bilinear) -> HSV
    gains (cv2's 8-bit BGR<->HSV + the three lookup tables) -> flips -> CHW RGB uint8, i.e. batch['img'] of the reference's batch dict.
    The 2s x 2s mosaic canvas is never materialised: every bilinear tap is resolved through the four placement rectangles.
There is no CPU pixel path: without the library the augmenter raises.
"""
import math
import random as _random
from types import SimpleNamespace

import numpy as np
import torch

F32 = np.float32


def AugmentHyp(**kw):
    """the reference's augmentation hyper-parameters (cfg/default.yaml:101-113)"""
    d = dict(mosaic=1.0, copy_paste=0.0, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0, mixup=0.0, hsv_h=0.015,
             hsv_s=0.7, hsv_v=0.4, flipud=0.0, fliplr=0.5)
    d.update(kw)
    return SimpleNamespace(**d)


def _check_hyp(hyp):
    if hyp.copy_paste or hyp.perspective:
        raise NotImplementedError("copy_paste / perspective are 0 in the reference's configuration and are not implemented")


def _plan_geometry(index, shapes, buffer, s, hyp, rnd):
    """The draws of the reference's `pre_transform` = [Mosaic, CopyPaste(p=0), RandomPerspective] for dataset image `index`: mosaic coin,
    three partners, centre (or the LetterBox geometry), eight affine draws.  The primary of a sample and the partner of a MixUp both go
    through it (BaseMixTransform.__call__ :97-101 applies MixUp's pre_transform to the partner)."""
    p = SimpleNamespace(index=int(index), imgsz=s)
    p.mosaic = not (rnd.uniform(0, 1) > hyp.mosaic)
    if p.mosaic:
        p.sources = [int(index)] + [int(i) for i in rnd.choices(list(buffer), k=3)]
        border = (-s // 2, -s // 2)
        p.yc, p.xc = (int(rnd.uniform(-x, 2 * s + x)) for x in border)
        p.border = border
        p.canvas_hw = (2 * s, 2 * s)
        p.rects = mosaic4_rects(s, p.yc, p.xc, [shapes[i] for i in p.sources])
    else:                                                     # RandomPerspective's pre_transform: LetterBox((s, s)) (:767)
        p.sources = [int(index)]
        p.border = (0, 0)
        h, w = shapes[index]
        geo = letterbox_geometry((h, w), (s, s), scaleup=True)
        if (w, h) != geo.new_unpad:
            raise NotImplementedError("letterbox with resize inside the training chain: images must be at their load_image size")
        p.canvas_hw = (s, s)
        p.letterbox = geo
        p.rects = [(geo.left, geo.top, geo.left + w, geo.top + h, 0, 0, w, h)]
    draws = [rnd.uniform(-hyp.perspective, hyp.perspective), rnd.uniform(-hyp.perspective, hyp.perspective),
             rnd.uniform(-hyp.degrees, hyp.degrees), rnd.uniform(1 - hyp.scale, 1 + hyp.scale),
             rnd.uniform(-hyp.shear, hyp.shear), rnd.uniform(-hyp.shear, hyp.shear),
             rnd.uniform(0.5 - hyp.translate, 0.5 + hyp.translate), rnd.uniform(0.5 - hyp.translate, 0.5 + hyp.translate)]
    p.M, p.scale, p.size = affine_matrix(draws, p.canvas_hw, p.border)
    return p


def plan_train_sample(index, shapes, buffer, imgsz, hyp, rnd=_random, nprnd=np.random):
    """Random draws of ONE training sample, in the call order of the reference's transform chain:
      Mosaic.__call__ (augment.py:86-104): uniform(0, 1) against p; 3 partners with random.choices(buffer, k=3) (:145-150);
        centre yc, xc = int(uniform(-x, 2 s + x)) for x in border = (-s // 2, -s // 2) (:161);
      RandomPerspective.affine_transform (:317-339): 2 perspective, rotation, scale, 2 shear, 2 translation draws;
      MixUp.__call__ (:86-107, 272-288): uniform(0, 1) against hyp.mixup (always one draw); only when taken: the partner image
        random.randint(0, len(dataset) - 1), the partner's own Mosaic / RandomPerspective draws as above (it may fall onto the
        letterbox path when mosaic < 1), then r = numpy.random.beta(32, 32);
      RandomHSV (:490): numpy.random.uniform(-1, 1, 3) when any gain is non-zero;
      RandomFlip vertical (:527): random.random(); RandomFlip horizontal (:530): random.random().
    `shapes[i]` = (h, w) of dataset image i at its load_image size: the non-mosaic (letterbox) path -- the primary's or a MixUp
    partner's when hyp.mosaic < 1, every sample after close_mosaic -- needs images at that size and raises NotImplementedError otherwise.
    Returns a SimpleNamespace plan; `plan.mix` is the partner's plan (sources, rects, canvas_hw, M, scale, size, border / letterbox)
    and `plan.mix_r` the blend ratio (Python float) when MixUp was taken, else plan.mix is None."""
    _check_hyp(hyp)
    s = int(imgsz)
    p = _plan_geometry(index, shapes, buffer, s, hyp, rnd)
    p.mix, p.mix_r = None, None
    taken = not (rnd.uniform(0, 1) > hyp.mixup)               # MixUp's own coin (drawn whatever p is)
    if taken and hyp.mixup > 0:                               # (p = 0: never, also not on a draw of exactly 0.0 -- the un-mixed kernel renders)
        p.mix = _plan_geometry(rnd.randint(0, len(shapes) - 1), shapes, buffer, s, hyp, rnd)
        p.mix_r = float(nprnd.beta(32.0, 32.0))
    p.hsv_gains = None
    if hyp.hsv_h or hyp.hsv_s or hyp.hsv_v:
        p.hsv_gains = nprnd.uniform(-1, 1, 3) * [hyp.hsv_h, hyp.hsv_s, hyp.hsv_v] + 1
        p.luts = hsv_luts(p.hsv_gains)
    p.flipud = rnd.random() < hyp.flipud
    p.fliplr = rnd.random() < hyp.fliplr
    return p


def mosaic4_rects(s, yc, xc, shapes):
    """placement of the four images around the centre (Mosaic._mosaic4, augment.py:166-186): canvas rectangle (x1a, y1a, x2a, y2a) and
    source rectangle (x1b, y1b, x2b, y2b) per image"""
    rects = []
    for i, (h, w) in enumerate(shapes):
        if i == 0:                                            # top left
            a = (max(xc - w, 0), max(yc - h, 0), xc, yc)
            b = (w - (a[2] - a[0]), h - (a[3] - a[1]), w, h)
        elif i == 1:                                          # top right
            a = (xc, max(yc - h, 0), min(xc + w, s * 2), yc)
            b = (0, h - (a[3] - a[1]), min(w, a[2] - a[0]), h)
        elif i == 2:                                          # bottom left
            a = (max(xc - w, 0), yc, xc, min(s * 2, yc + h))
            b = (w - (a[2] - a[0]), 0, w, min(a[3] - a[1], h))
        else:                                                 # bottom right
            a = (xc, yc, min(xc + w, s * 2), min(s * 2, yc + h))
            b = (0, 0, min(w, a[2] - a[0]), min(a[3] - a[1], h))
        rects.append(a + b)
    return rects


def rotation_matrix_2d(angle, scale):
    """cv2.getRotationMatrix2D(angle, (0, 0), scale) (OpenCV's documented closed form)"""
    a = scale * math.cos(angle * math.pi / 180)
    b = scale * math.sin(angle * math.pi / 180)
    return np.array([[a, b, 0.0], [-b, a, 0.0]], dtype=np.float64)


def affine_matrix(draws, canvas_hw, border):
    """T S R P C of RandomPerspective.affine_transform (augment.py:310-345), float32 like the reference.  Returns (M 3x3, scale, (w, h))."""
    size = canvas_hw[1] + border[1] * 2, canvas_hw[0] + border[0] * 2
    C = np.eye(3, dtype=F32)
    C[0, 2] = -canvas_hw[1] / 2
    C[1, 2] = -canvas_hw[0] / 2
    P = np.eye(3, dtype=F32)
    P[2, 0], P[2, 1] = draws[0], draws[1]
    R = np.eye(3, dtype=F32)
    R[:2] = rotation_matrix_2d(draws[2], draws[3])
    S = np.eye(3, dtype=F32)
    S[0, 1] = math.tan(draws[4] * math.pi / 180)
    S[1, 0] = math.tan(draws[5] * math.pi / 180)
    T = np.eye(3, dtype=F32)
    T[0, 2] = draws[6] * size[0]
    T[1, 2] = draws[7] * size[1]
    return T @ S @ R @ P @ C, draws[3], size


def hsv_luts(r):
    """RandomHSV's tables (augment.py:493-497)"""
    x = np.arange(0, 256, dtype=r.dtype)
    return (((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8), np.clip(x * r[2], 0, 255).astype(np.uint8))


def letterbox_geometry(shape, new_shape, scaleup=True):
    """LetterBox's arithmetic (augment.py:566-590, center=True)"""
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scaleup:
        r = min(r, 1.0)
    new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
    dw, dh = (new_shape[1] - new_unpad[0]) / 2, (new_shape[0] - new_unpad[1]) / 2
    return SimpleNamespace(r=r, new_unpad=new_unpad, dw=dw, dh=dh, top=int(round(dh - 0.1)), bottom=int(round(dh + 0.1)),
                           left=int(round(dw - 0.1)), right=int(round(dw + 0.1)))


# ---------------------------------------------------------------------------------------------------------------- labels (host, float32)
def _xywh2xyxy(x):
    y = np.empty_like(x)
    dw, dh = x[..., 2] / 2, x[..., 3] / 2
    y[..., 0], y[..., 1], y[..., 2], y[..., 3] = x[..., 0] - dw, x[..., 1] - dh, x[..., 0] + dw, x[..., 1] + dh
    return y


def _xyxy2xywh(x):
    y = np.copy(x)
    y[..., 0] = (x[..., 0] + x[..., 2]) / 2
    y[..., 1] = (x[..., 1] + x[..., 3]) / 2
    y[..., 2] = x[..., 2] - x[..., 0]
    y[..., 3] = x[..., 3] - x[..., 1]
    return y


def _mul(b, sx, sy):
    """Bboxes.mul (utils/instance.py:103-115): column by column, in place, python scalars"""
    b[:, 0] *= sx
    b[:, 1] *= sy
    b[:, 2] *= sx
    b[:, 3] *= sy


def _apply_affine(bboxes, M):
    n = len(bboxes)
    if n == 0:
        return bboxes
    xy = np.ones((n * 4, 3), dtype=bboxes.dtype)
    xy[:, :2] = bboxes[:, [0, 1, 2, 3, 0, 3, 2, 1]].reshape(n * 4, 2)
    xy = (xy @ M.T)[:, :2].reshape(n, 8)
    x, y = xy[:, [0, 2, 4, 6]], xy[:, [1, 3, 5, 7]]
    return np.concatenate((x.min(1), y.min(1), x.max(1), y.max(1)), dtype=bboxes.dtype).reshape(4, n).T


def _candidates(box1, box2, wh_thr=2, ar_thr=100, area_thr=0.1, eps=1e-16):
    w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
    w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
    ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
    return (w2 > wh_thr) & (h2 > wh_thr) & (w2 * h2 / (w1 * h1 + eps) > area_thr) & (ar < ar_thr)


N_RESAMPLE = 1000                                             # points per polygon (resample_segments' default n)


def resample_segments(segments, n=N_RESAMPLE):
    """resample_segments (utils/ops.py:533-550) of a list of [k_i, 2] polygons: the closing point is appended and both coordinates are
    interpolated (np.interp, float64) at n equidistant parameters, result float32 [len, n, 2].  Instances.__init__ does this to the
    raw polygons of a label (utils/instance.py:200-204)."""
    out = np.zeros((len(segments), n, 2), dtype=F32)
    for i, sg in enumerate(segments):
        sg = np.asarray(sg).reshape(-1, 2)
        sg = np.concatenate((sg, sg[0:1, :]), axis=0)
        x, xp = np.linspace(0, len(sg) - 1, n), np.arange(len(sg))
        out[i] = np.concatenate([np.interp(x, xp, sg[:, k]) for k in range(2)], dtype=F32).reshape(2, -1).T
    return out


_RS_T = np.linspace(0, N_RESAMPLE, N_RESAMPLE) - np.arange(N_RESAMPLE)      # parameter i lies in interval [i, i + 1) of the closed polygon
assert _RS_T[0] == 0 and np.all((_RS_T[:-1] >= 0) & (_RS_T[:-1] < 1)) and _RS_T[-1] == 1


def _reresample(seg):
    """What every further Instances(...) construction does to segments that are ALREADY [n, 1000, 2] (a reference quirk:
    Instances.__init__ resamples whatever it is handed, utils/instance.py:200-204, and Instances.concatenate / __getitem__ and
    RandomPerspective all construct new Instances): the 1001-point closed polygon resampled to 1000 points again.  np.interp's
    arithmetic `slope * (x - xp[j]) + fp[j]` in float64 for all polygons at once (same operations, so the same bits); parameter i of
    linspace(0, 1000, 1000) falls into interval j == i, the last one is the end point itself."""
    if len(seg) == 0:
        return seg
    fp = np.concatenate((seg, seg[:, 0:1]), axis=1, dtype=np.float64)                         # [n, 1001, 2]
    out = (fp[:, 1:] - fp[:, :-1]) * _RS_T[None, :, None] + fp[:, :-1]
    out[:, -1] = fp[:, -1]                                                                    # x == xp[-1]: np.interp returns fp[-1]
    return out.astype(F32)


def _segments2boxes(sg, width, height):
    """segment2box (utils/ops.py:75-92) of every polygon of sg [n, P, 2] at once, with its quirk: `any(x)` is false when no inside
    point has a non-zero x -> zeros.  (min / max of float32 are exact, so masking with +-inf gives the reference's values.)"""
    x, y = sg[..., 0], sg[..., 1]
    inside = (x >= 0) & (y >= 0) & (x <= width) & (y <= height)
    inf = sg.dtype.type(np.inf)
    out = np.stack((np.where(inside, x, inf).min(1), np.where(inside, y, inf).min(1), np.where(inside, x, -inf).max(1),
                    np.where(inside, y, -inf).max(1)), 1)
    out[~(inside & (x != 0)).any(1)] = 0
    return out


def keypoints_with_visibility(keypoints):
    """[n, K, 2 or 3] float32; for ndim == 2 the visibility column the label reader appends (data/utils.py:124-128): 0 where a
    coordinate is negative, else 1"""
    kp = np.array(keypoints, dtype=F32)
    if kp.ndim != 3 or kp.shape[2] not in (2, 3):
        raise ValueError("keypoints must be [n, K, 2 or 3]")
    if kp.shape[2] == 2:
        vis = np.ones(kp.shape[:2], dtype=F32)
        vis = np.where(kp[..., 0] < 0, 0.0, vis)
        vis = np.where(kp[..., 1] < 0, 0.0, vis)
        kp = np.concatenate([kp, vis[..., None]], axis=-1).astype(F32)
    return kp


def check_flip_idx(hyp, flip_idx, n_kpt):
    """the rule of v8_transforms (augment.py:780-787) for a pose dataset: no flip_idx and fliplr > 0 -> fliplr = 0 with a warning (a COPY
    of hyp is returned, the caller's object is left alone); a flip_idx of the wrong length raises ValueError"""
    import copy
    import warnings
    flip_idx = [] if flip_idx is None else [int(i) for i in flip_idx]
    if len(flip_idx) == 0 and hyp.fliplr > 0.0:
        hyp = copy.copy(hyp)
        hyp.fliplr = 0.0
        warnings.warn("no 'flip_idx' given for a pose dataset: setting augmentation fliplr=0.0")
    elif flip_idx and len(flip_idx) != n_kpt:
        raise ValueError(f"flip_idx={flip_idx} length must be equal to kpt_shape[0]={n_kpt}")
    return hyp, (flip_idx or None)


def _stage_labels(plan, labels, shapes, segments, keypoints):
    """train_labels up to and including box_candidates for ONE side of a sample (the primary, or the partner of a MixUp: a plan's
    geometry part): (cls [m, 1], pixel xyxy boxes [m, 4], segments [m, 1000, 2] or None, keypoints [m, K, 3] or None) as
    RandomPerspective.__call__ leaves them (:464-468)"""
    seg_on, kp_on = segments is not None, keypoints is not None
    cls, boxes, segs, kps = [], [], [], []
    for src, rect in zip(plan.sources, plan.rects):
        h, w = shapes[src]
        b = _xywh2xyxy(np.array(labels[src]["bboxes"], dtype=F32, copy=True).reshape(-1, 4))
        _mul(b, w, h)
        if plan.mosaic:
            padw, padh = rect[0] - rect[4], rect[1] - rect[5]           # Mosaic._update_labels: integer paste offset (augment.py:189-192)
        else:
            padw, padh = plan.letterbox.dw, plan.letterbox.dh          # LetterBox._update_labels: the UNROUNDED half padding (:593-603)
        b[:, 0] += padw
        b[:, 1] += padh
        b[:, 2] += padw
        b[:, 3] += padh
        boxes.append(b)
        cls.append(np.array(labels[src]["cls"], dtype=F32).reshape(-1, 1))
        for on, store, dst in ((seg_on, segments, segs), (kp_on, keypoints, kps)):
            if on:
                e = np.array(store[src], dtype=F32, copy=True)
                e[..., :2] *= np.array([w, h], dtype=F32)             # per element the reference's `[..., 0] *= w`, `[..., 1] *= h`
                e[..., :2] += np.array([padw, padh], dtype=F32)
                dst.append(e)
    b, c = np.concatenate(boxes, 0), np.concatenate(cls, 0)
    sg = np.concatenate(segs, 0) if seg_on else None
    kp = np.concatenate(kps, 0) if kp_on else None
    if plan.mosaic:
        ch, cw = plan.canvas_hw
        if seg_on:
            sg = _reresample(sg)                                      # Instances.concatenate constructs a new Instances
        b[:, [0, 2]] = b[:, [0, 2]].clip(0, cw)
        b[:, [1, 3]] = b[:, [1, 3]].clip(0, ch)
        for e in (sg, kp):
            if e is not None:
                np.clip(e[..., :2], 0, np.array([cw, ch], dtype=F32), out=e[..., :2])
        good = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) > 0
        b, c = b[good], c[good]
        sg, kp = (sg[good] if seg_on else None), (kp[good] if kp_on else None)
    nb = _apply_affine(b, plan.M)
    w, h = plan.size
    if seg_on and len(sg):                                        # apply_segments: the boxes come from the polygons
        n = len(sg)
        xy = np.ones((n * sg.shape[1], 3), dtype=sg.dtype)
        xy[:, :2] = sg.reshape(-1, 2)
        xy = xy @ plan.M.T
        xy = xy[:, :2] / xy[:, 2:3]
        sg = xy.reshape(n, -1, 2)
        nb = _segments2boxes(sg, w, h)
        sg = _reresample(sg)                                          # Instances(bboxes, segments, keypoints)
    if kp_on and len(kp):                                         # apply_keypoints
        n, nk = kp.shape[:2]
        xy = np.ones((n * nk, 3), dtype=kp.dtype)
        vis = kp[..., 2].reshape(n * nk, 1).copy()
        xy[:, :2] = kp[..., :2].reshape(n * nk, 2)
        xy = xy @ plan.M.T
        xy = xy[:, :2] / xy[:, 2:3]
        vis[(xy[:, 0] < 0) | (xy[:, 1] < 0) | (xy[:, 0] > w) | (xy[:, 1] > h)] = 0
        kp = np.concatenate([xy, vis], axis=-1).reshape(n, nk, 3)
    nb[:, [0, 2]] = nb[:, [0, 2]].clip(0, w)
    nb[:, [1, 3]] = nb[:, [1, 3]].clip(0, h)
    for e in (sg, kp):
        if e is not None:
            np.clip(e[..., :2], 0, np.array([w, h], dtype=F32), out=e[..., :2])
    _mul(b, plan.scale, plan.scale)
    keep = _candidates(b.T, nb.T, area_thr=0.01 if (seg_on and len(sg)) else 0.10)
    nb, c = nb[keep], c[keep]
    if seg_on:
        sg = _reresample(sg[keep])                                    # new_instances[i]
    if kp_on:
        kp = kp[keep]
    return c, nb, sg, kp


def train_labels(plan, labels, shapes, segments=None, keypoints=None, flip_idx=None):
    """The boxes of one planned sample through the reference's bookkeeping: per source xywhn -> xyxy pixels + mosaic offset
    (Mosaic._update_labels :262-268), concatenation, clip to the canvas and zero-area removal (_cat_labels :270-288), affine + clip
    + box_candidates against the scaled originals (RandomPerspective.__call__ :432-468), xywh-normalised (Albumentations' bookkeeping
    :681-692), flips on normalised centres (RandomFlip :521-534), Format's denormalise / normalise round trip (:719-733).
    labels[i] = dict(cls [n,1] float32, bboxes [n,4] normalised xywh float32).  Returns (cls [m,1], bboxes [m,4]) float32.

    `segments[i]` (float32 [n_i, 1000, 2], normalised, resample_segments of image i's polygons) or `keypoints[i]` (float32 [n_i, K, 3],
    normalised x, y + visibility) move through the same steps (Instances.denormalize / add_padding / clip :229-329,
    RandomPerspective.apply_segments / apply_keypoints :375-421, Instances.flipud / fliplr, `flip_idx` on a horizontal flip :533-534) and a
    third value is returned: the int32 [m, 1000, 2] pixel polygons exactly as polygon2mask hands them to cv2.fillPoly
    (data/utils.py:146-147, astype(np.int32) of Format's denormalised segments), or the normalised keypoints [m, K, 3] of
    Format(return_keypoint=True).  Rows are in LABEL order; the area order of Format._format_segments is applied on the device.
    Reference quirks reproduced (the g20 fixtures decide):
      * every Instances construction resamples non-empty segments again (_reresample): Instances.concatenate in Mosaic._cat_labels,
        RandomPerspective's new_instances and its new_instances[i] -- three times on the mosaic path, twice on the letterbox path;
      * with segments the boxes become segment2box of the transformed polygons (zeros when no inside point has a non-zero x) and
        box_candidates uses area_thr 0.01 instead of 0.10 (:464-466);
      * keypoints outside [0, w] x [0, h] after the affine map get visibility 0 and are then clipped like the rest (:419-420, :459);
      * a MixUp (plan.mix set) concatenates the partner's rows after the primary's at this point -- pixel xyxy boxes already filtered by
        box_candidates on each side, Instances.concatenate (:286): one more re-resampling of the segments; normalisation, flips
        (flip_idx on all rows) and Format then see the merged set, so the polygons reach polygon2mask in primary-then-partner order
        and the area ranking is over the merged set;
      * Albumentations' normalisation divides segments / keypoints by w, h while the boxes are multiplied by 1 / w, 1 / h."""
    seg_on, kp_on = segments is not None, keypoints is not None
    if seg_on and kp_on:
        raise ValueError("Can not use both segments and keypoints.")
    c, nb, sg, kp = _stage_labels(plan, labels, shapes, segments, keypoints)
    if getattr(plan, "mix", None) is not None:                # MixUp._mix_transform (:286-287)
        c2, nb2, sg2, kp2 = _stage_labels(plan.mix, labels, shapes, segments, keypoints)
        c, nb = np.concatenate((c, c2), 0), np.concatenate((nb, nb2), 0)
        if seg_on:
            sg = _reresample(np.concatenate((sg, sg2), 0))         # Instances.concatenate constructs a new Instances
        if kp_on:
            kp = np.concatenate((kp, kp2), 0)
    w, h = plan.size
    if len(c):                                                # Albumentations.__call__ touches the boxes only when there are any
        nb = _xyxy2xywh(nb)
        _mul(nb, 1 / w, 1 / h)
        for e in (sg, kp):
            if e is not None:
                e[..., :2] /= np.array([w, h], dtype=F32)
        normalized = True
    else:
        normalized = False
    # RandomFlip: convert_bbox('xywh') first (a real conversion when Albumentations skipped the empty set)
    if not normalized:
        nb = _xyxy2xywh(nb)
    fh, fw = (1, 1) if normalized else (h, w)
    if plan.flipud:
        nb[:, 1] = fh - nb[:, 1]
        for e in (sg, kp):
            if e is not None:
                e[..., 1] = fh - e[..., 1]
    if plan.fliplr:
        nb[:, 0] = fw - nb[:, 0]
        for e in (sg, kp):
            if e is not None:
                e[..., 0] = fw - e[..., 0]
        if kp_on and flip_idx is not None:
            kp = np.ascontiguousarray(kp[:, flip_idx, :])
    if normalized:                                            # Format: denormalize(w, h) ...
        _mul(nb, w, h)
        for e in (sg, kp):
            if e is not None:
                e[..., :2] *= np.array([w, h], dtype=F32)
    polys = sg.astype(np.int32) if seg_on else None           # ... polygon2mask's truncation of the pixel polygons ...
    _mul(nb, 1 / w, 1 / h)                                    # ... then normalize(w, h)
    if kp_on and normalized:
        kp[..., 0] /= w
        kp[..., 1] /= h
    if seg_on:
        return c, nb, polys
    if kp_on:
        return c, nb, kp
    return c, nb


def val_labels(bboxes, shape, imgsz, segments=None, keypoints=None, rect_shape=None):
    """LetterBox(scaleup=False)._update_labels + Format for the validation set (augment.py:593-603, 719-733).  Returns (bboxes
    normalised xywh float32, ratio_pad ((r, r), (dw, dh)), geometry).  With `segments` (list of [k, 2] normalised polygons, or the
    resampled [n, 1000, 2] array) or `keypoints` ([n, K, 2 or 3] normalised) a fourth value follows: the int32 [n, 1000, 2] polygons
    polygon2mask hands to cv2.fillPoly (in label order), or the normalised keypoints [n, K, 3]: Instances.denormalize(w, h),
    scale(r, r), add_padding(dw, dh), then Format's normalize(imgsz, imgsz).  `rect_shape` (H, W): the batch shape of a rect
    validation set (LetterBox pops it in place of its own new_shape, augment.py:563; Format normalises by the letter-boxed image's
    own width and height)."""
    if segments is not None and keypoints is not None:
        raise ValueError("Can not use both segments and keypoints.")
    h, w = shape
    H, W = (imgsz, imgsz) if rect_shape is None else (int(rect_shape[0]), int(rect_shape[1]))
    geo = letterbox_geometry((h, w), (H, W), scaleup=False)
    b = _xywh2xyxy(np.array(bboxes, dtype=F32, copy=True).reshape(-1, 4))
    _mul(b, w, h)
    _mul(b, geo.r, geo.r)
    b[:, 0] += geo.dw
    b[:, 1] += geo.dh
    b[:, 2] += geo.dw
    b[:, 3] += geo.dh
    b = _xyxy2xywh(b)
    _mul(b, 1 / W, 1 / H)
    out = (b, ((geo.r, geo.r), (geo.dw, geo.dh)), geo)
    if segments is None and keypoints is None:
        return out
    if segments is not None:
        e = segments if (isinstance(segments, np.ndarray) and segments.ndim == 3) else resample_segments(segments)
        e = np.array(e, dtype=F32, copy=True)
    else:
        e = keypoints_with_visibility(keypoints)
    e[..., 0] *= w
    e[..., 1] *= h
    e[..., 0] *= geo.r
    e[..., 1] *= geo.r
    e[..., 0] += geo.dw
    e[..., 1] += geo.dh
    if segments is not None:
        return out + (e.astype(np.int32),)
    e[..., 0] /= W
    e[..., 1] /= H
    return out + (e,)


def collate(samples):
    """YOLODataset.collate_fn (dataset.py:172-188) for (cls, bboxes) pairs: concatenation + batch_idx"""
    cls = np.concatenate([c for c, _ in samples], 0) if samples else np.zeros((0, 1), F32)
    bb = np.concatenate([b for _, b in samples], 0) if samples else np.zeros((0, 4), F32)
    bi = np.concatenate([np.full(len(c), i, dtype=F32) for i, (c, _) in enumerate(samples)]) if samples else np.zeros(0, F32)
    return torch.from_numpy(bi), torch.from_numpy(cls), torch.from_numpy(bb)


# ---------------------------------------------------------------------------------------------------------------- device side
class DeviceAugmenter:
    """Owns the decoded dataset images (uint8 HWC BGR at their load_image size, device-resident) and produces the reference's batch dict
    {img uint8 [B,3,s,s] RGB, cls, bboxes, batch_idx, n_max} for lists of sample plans.  `images`: list of uint8 HWC numpy arrays or
    device tensors; `labels`: list of dict(cls, bboxes normalised xywh).

    task="segment": every label dict also carries `segments` (list of [k, 2] normalised polygons; resampled once here) and the batch
    gains `masks` (uint8, device: [B, s / mask_ratio, s / mask_ratio] overlap index maps, or [N, ...] 0/1 planes with
    overlap_mask=False) with cls / bboxes / batch_idx in the matching (area) order, on the device.  task="pose": `keypoints`
    ([n, K, 2 or 3] normalised) -> batch `keypoints` [N, K, 3]."""

    def __init__(self, images, labels, imgsz, hyp=None, device="cuda", task="detect", flip_idx=None, mask_ratio=4, overlap_mask=True):
        from .. import ops
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceAugmenter: the pixel pipeline only exists on the device")
        self.imgsz = int(imgsz)
        self.hyp = hyp or AugmentHyp()
        self.images = []
        for im in images:
            if torch.is_tensor(im):
                ops.require_gpu(im)
            self.images.append(im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im)).to(self.device))
        for im in self.images:
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or not im.is_contiguous():
                raise ValueError("DeviceAugmenter: images must be contiguous uint8 HWC with 3 channels")
        self.shapes = [(int(im.shape[0]), int(im.shape[1])) for im in self.images]
        self.labels = labels
        self.buffer = list(range(len(self.images)))
        self.extras = TaskLabels(labels, task, self.hyp, flip_idx, mask_ratio, overlap_mask, self.imgsz)
        self.hyp, self.task = self.extras.hyp, self.extras.task

    def plan(self, index, rnd=_random, nprnd=np.random):
        return plan_train_sample(index, self.shapes, self.buffer, self.imgsz, self.hyp, rnd, nprnd)

    def render(self, plans, staging=None):
        """pixels of a list of plans: uint8 [B, 3, s, s] RGB on the device (one launch on the current stream).  `staging`: optional
        pinned uint8 host tensor (>= B * descriptor_bytes(mix)) the descriptors are written into and copied from asynchronously;
        without it the copy comes from pageable memory and blocks the host.  With hyp.mixup > 0 the launch is dy_aug_mosaic_warp_mix
        over dy_aug_mix_sample descriptors (mixed and un-mixed samples alike); with mixup == 0 nothing changes."""
        from .._C import call
        from ..ops import ptr, stream
        B, s = len(plans), self.imgsz
        mix = self.hyp.mixup > 0
        nbytes = B * descriptor_bytes(mix)
        host = staging[:nbytes] if staging is not None else torch.empty(nbytes, dtype=torch.uint8)
        if mix and nbytes:
            host.zero_()                                      # padding and the unread half of un-mixed descriptors: defined bytes
        fill_descriptors(plans, self.images, host.data_ptr(), mix)
        dev = host.to(self.device, non_blocking=staging is not None)
        out = torch.empty((B, 3, s, s), dtype=torch.uint8, device=self.device)
        call("dy_aug_mosaic_warp_mix" if mix else "dy_aug_mosaic_warp", ptr(dev), B, s, s, ptr(out), stream())
        self._keep = dev                                      # descriptor array stays alive until the next call
        return out

    def batch(self, indices, rnd=_random, nprnd=np.random):
        plans = [self.plan(i, rnd, nprnd) for i in indices]
        img = self.render(plans)
        lab = [self.extras.train_labels(p, self.shapes) for p in plans]
        n_max = max([len(l[0]) for l in lab] + [0])
        meta = dict(n_max=n_max, im_file=[f"{i}" for i in indices], ori_shape=[self.shapes[i] for i in indices],
                    resized_shape=[(self.imgsz, self.imgsz)] * len(indices))
        if self.task == "segment":                            # labels on the device, in the order the masks index them
            rows, polys, offsets = pack_rows(lab), pack_polygons(lab), instance_offsets(lab)
            dev = lambda a: torch.from_numpy(a).to(self.device)
            out = polygon_masks(dev(polys), dev(offsets), dev(rows), len(lab), self.imgsz, self.imgsz, self.extras.mask_ratio, self.extras.overlap_mask)
            rows_d = out[1] if self.extras.overlap_mask else dev(rows)
            return dict(img=img, batch_idx=rows_d[:, 0], cls=rows_d[:, 1:2], bboxes=rows_d[:, 2:6], masks=out[0],
                        sorted_idx=out[2] if self.extras.overlap_mask else None, **meta)
        bi, cls, bb = collate([l[:2] for l in lab])
        batch = dict(img=img, batch_idx=bi, cls=cls, bboxes=bb, **meta)
        if self.task == "pose":
            batch["keypoints"] = torch.from_numpy(np.concatenate([l[2] for l in lab], 0))
        return batch


class TaskLabels:
    """the per-task side of the label bookkeeping shared by DeviceAugmenter and DeviceAugmentLoader: polygons resampled once
    (Instances.__init__), keypoints with their visibility column, the flip_idx rule of v8_transforms"""

    def __init__(self, labels, task, hyp, flip_idx, mask_ratio, overlap_mask, imgsz):
        if task not in ("detect", "segment", "pose"):
            raise ValueError(f"task must be 'detect', 'segment' or 'pose', got {task!r}")
        self.labels, self.task, self.hyp, self.flip_idx = labels, task, hyp, None
        self.mask_ratio, self.overlap_mask = int(mask_ratio), bool(overlap_mask)
        self.segments = self.keypoints = None
        for lab in labels:
            if lab.get("segments") is not None and lab.get("keypoints") is not None:
                raise ValueError("Can not use both segments and keypoints.")         # dataset.py:27
        if task == "segment":
            if self.mask_ratio != 1 and (self.mask_ratio <= 0 or self.mask_ratio % 2):
                raise ValueError("mask_ratio must be 1 or even")
            if imgsz % self.mask_ratio:
                raise ValueError("imgsz must be a multiple of mask_ratio")
            self.segments = []
            for lab in labels:
                sg = lab.get("segments")
                if sg is None or len(sg) != len(np.asarray(lab["cls"]).reshape(-1)):
                    raise ValueError("task='segment': every label needs one polygon per instance in 'segments'")
                self.segments.append(resample_segments(sg))
        elif task == "pose":
            if any(lab.get("keypoints") is None for lab in labels):
                raise ValueError("task='pose': every label needs 'keypoints' [n, K, 2 or 3]")
            self.keypoints = [keypoints_with_visibility(lab["keypoints"]) for lab in labels]
            ks = {k.shape[1] for k in self.keypoints}
            if len(ks) > 1:
                raise ValueError(f"task='pose': labels disagree on the number of keypoints: {sorted(ks)}")
            self.hyp, self.flip_idx = check_flip_idx(hyp, flip_idx, ks.pop() if ks else 0)

    def train_labels(self, plan, shapes):
        out = train_labels(plan, self.labels, shapes, self.segments, self.keypoints, self.flip_idx)
        if self.task == "segment" and len(out[0]) > 255:
            raise NotImplementedError("more than 255 instances in one image (the overlap mask is uint8)")
        return out


def instance_offsets(lab):
    """int32 [B + 1]: first label row of every image"""
    return np.concatenate(([0], np.cumsum([len(l[0]) for l in lab]))).astype(np.int32)


def pack_rows(lab, out=None):
    """f32 [N, 6] rows (batch_idx, cls, x, y, w, h) of a list of per-image (cls, bboxes, ...)"""
    n = sum(len(l[0]) for l in lab)
    rows = np.empty((n, 6), dtype=F32) if out is None else out[:n]
    o = 0
    for i, l in enumerate(lab):
        m = len(l[0])
        rows[o:o + m, 0], rows[o:o + m, 1], rows[o:o + m, 2:6] = i, l[0].reshape(-1), l[1]
        o += m
    return rows


def pack_polygons(lab, out=None):
    """int16 [N, 1000, 2]: the int32 polygons of train_labels / val_labels (already inside [0, s]) as the rasteriser reads them"""
    n = sum(len(l[0]) for l in lab)
    polys = np.empty((n, N_RESAMPLE, 2), dtype=np.int16) if out is None else out[:n]
    o = 0
    for l in lab:
        m = len(l[0])
        if m:
            if int(l[2].min()) < -32768 or int(l[2].max()) > 32767:
                raise ValueError("polygon vertex outside the int16 range")
            polys[o:o + m] = l[2]
        o += m
    return polys


def polygon_masks(polys, offsets, rows, B, h, w, mask_ratio=4, overlap=True):
    """Ground-truth masks of a batch on the device (csrc/polymask.hip) = polygon2mask / polygons2masks / polygons2masks_overlap
    (data/utils.py:137-190) + the re-ordering of Format._format_segments (augment.py:757-760), on the current stream, no host sync.
    polys int16 [N, P, 2], offsets int32 [B + 1], rows f32 [N, 6] (device tensors).  overlap: (masks uint8 [B, h / r, w / r], rows in
    area order [N, 6], sorted_idx int32 [N] = index within its image of the instance at each rank); else (planes uint8 [N, h / r, w / r]
    in label order, None, None)."""
    from .._C import call
    from ..ops import ptr, stream
    r = int(mask_ratio)
    if r != 1 and (r <= 0 or r % 2):
        raise ValueError("mask_ratio must be 1 or even")
    if h % r or w % r:
        raise ValueError("the image size must be a multiple of mask_ratio")
    if polys.dtype != torch.int16 or polys.dim() != 3 or polys.shape[2] != 2 or not polys.is_cuda:
        raise ValueError("polygon_masks: polys must be a device int16 tensor [N, P, 2]")
    N, P = int(polys.shape[0]), int(polys.shape[1])
    if offsets.dtype != torch.int32 or offsets.numel() != B + 1 or rows.dtype != torch.float32 or tuple(rows.shape) != (N, 6):
        raise ValueError("polygon_masks: offsets must be int32 [B + 1] and rows f32 [N, 6]")
    polys, offsets, rows = polys.contiguous(), offsets.contiguous(), rows.contiguous()
    dev, mh, mw = polys.device, h // r, w // r
    planes = torch.empty((N, mh, mw), dtype=torch.uint8, device=dev)
    area = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    call("dy_polymask_raster", ptr(polys), N, max(P, 1), h, w, r, ptr(planes), ptr(area), stream())
    if not overlap:
        return planes, None, None
    masks = torch.empty((B, mh, mw), dtype=torch.uint8, device=dev)
    rows_out, perm = torch.empty_like(rows), torch.empty(N, dtype=torch.int32, device=dev)
    call("dy_polymask_compose", ptr(planes), ptr(area), ptr(offsets), B, N, mh, mw, ptr(rows), ptr(rows_out), ptr(perm), ptr(masks), stream())
    return masks, rows_out, perm


def descriptor_bytes(mix=False):
    """sizeof(dy_aug_sample), or of dy_aug_mix_sample (the descriptor of dy_aug_mosaic_warp_mix)"""
    import ctypes as C
    from .._C import AugMixSample, AugSample
    return C.sizeof(AugMixSample if mix else AugSample)


def _fill_geometry(a, p, images):
    """the fields of a dy_aug_sample both sides of a MixUp need: sources, placement rectangles, canvas, inverse matrix"""
    a.n_src = len(p.sources)
    for j, (src, r) in enumerate(zip(p.sources, p.rects)):
        im = images[src]
        a.src[j], a.sh[j], a.sw[j], a.pitch[j] = im.data_ptr(), im.shape[0], im.shape[1], im.stride(0)
        rj = a.rect[j]
        rj[0], rj[1], rj[2], rj[3], rj[4], rj[5] = int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), int(r[5])
    a.canvas_h, a.canvas_w = p.canvas_hw
    minv = invert_affine(p.M[:2]).reshape(-1)
    m = a.minv
    m[0], m[1], m[2], m[3], m[4], m[5] = (float(v) for v in minv)


def fill_descriptors(plans, images, address, mix=False):
    """dy_aug_sample[len(plans)] (mix: dy_aug_mix_sample[len(plans)]) at `address` (host memory owned by the caller) for plans over
    `images` (device tensors by dataset index).  Without `mix` a plan that carries a MixUp partner is an error."""
    import ctypes as C
    from .._C import AugMixSample, AugSample
    arr = ((AugMixSample if mix else AugSample) * len(plans)).from_address(address)
    for k, p in enumerate(plans):
        partner = getattr(p, "mix", None)
        if mix:
            d = arr[k]
            a = d.a
            d.mix = int(partner is not None)
            if partner is not None:
                _fill_geometry(d.b, partner, images)
                d.r, d.r1 = p.mix_r, 1.0 - p.mix_r           # 1 - r in float64 on the host, as Python computes it
        elif partner is not None:
            raise ValueError("fill_descriptors: a plan with a MixUp partner needs the mix descriptor")
        else:
            a = arr[k]
        _fill_geometry(a, p, images)
        a.hsv = int(p.hsv_gains is not None)
        if a.hsv:
            for c_ in range(3):
                C.memmove(a.lut[c_], p.luts[c_].ctypes.data, 256)
        a.flipud, a.fliplr = int(p.flipud), int(p.fliplr)


def invert_affine(M):
    """the inversion cv::warpAffine applies to its 2x3 matrix (double)"""
    m = np.array(M, dtype=np.float64).reshape(2, 3).copy()
    D = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[1, 1] * D, m[0, 0] * D
    m[0, 0] = A11
    m[0, 1] *= -D
    m[1, 0] *= -D
    m[1, 1] = A22
    b1 = -m[0, 0] * m[0, 2] - m[0, 1] * m[1, 2]
    b2 = -m[1, 0] * m[0, 2] - m[1, 1] * m[1, 2]
    m[0, 2], m[1, 2] = b1, b2
    return m


def load_resize(image, imgsz, augment=True):
    """BaseDataset.load_image's resize (base.py:152-157) of a decoded uint8 HWC device image: long side -> imgsz, with the reference's
    `interp = cv2.INTER_LINEAR if (self.augment or r > 1) else cv2.INTER_AREA`: training (augment=True) and every enlargement are
    linear (dy_aug_resize_u8), a validation image that shrinks goes through dy_aug_resize_area_u8.  Returns the image itself when the
    ratio is 1."""
    from .._C import call
    from ..ops import ptr, stream
    h0, w0 = int(image.shape[0]), int(image.shape[1])
    r = imgsz / max(h0, w0)
    if r == 1:
        return image
    w, h = min(math.ceil(w0 * r), imgsz), min(math.ceil(h0 * r), imgsz)
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=image.device)
    kernel = "dy_aug_resize_u8" if (augment or r > 1) else "dy_aug_resize_area_u8"
    call(kernel, ptr(image), h0, w0, image.stride(0), ptr(out), h, w, out.stride(0), stream())
    return out


def _hw(shape):
    """an int means a square (h, w)"""
    return (int(shape), int(shape)) if isinstance(shape, (int, np.integer)) else (int(shape[0]), int(shape[1]))


def letterbox_batch(images, imgsz, scaleup=False):
    """Validation transform: LetterBox(new_shape, scaleup) + Format's CHW RGB for a list of decoded uint8 HWC device images
    -> uint8 [B, 3, H, W] (resize + constant border 114 + channel flip in one launch per image).  `imgsz`: an int (square) or the
    (H, W) of a rect batch (the `rect_shape` LetterBox pops, augment.py:563)."""
    from .._C import call
    from ..ops import ptr, stream
    dev = images[0].device
    H, W = _hw(imgsz)
    out = torch.empty((len(images), 3, H, W), dtype=torch.uint8, device=dev)
    geos = []
    for k, im in enumerate(images):
        h, w = int(im.shape[0]), int(im.shape[1])
        g = letterbox_geometry((h, w), (H, W), scaleup)
        geos.append(g)
        call("dy_aug_letterbox", ptr(im), h, w, im.stride(0), g.new_unpad[1], g.new_unpad[0], g.top, g.left, H, W, ptr(out[k]), stream())
    return out, geos


def letterbox_auto(image, imgsz, stride=32):
    """The predictor's pre_transform for ONE decoded uint8 HWC BGR device image (engine/predictor.py:134-147: LetterBox(imgsz,
    auto=True, stride), augment.py:566-590): scale the long side to imgsz (scaleup, linear), pad each axis only up to the next
    multiple of `stride` (np.mod(dw, stride)), centred, border 114 -> uint8 [3, H, W] RGB and the geometry (r, new_unpad, dw, dh,
    top, left, out_hw)."""
    from .._C import call
    from ..ops import ptr, stream
    h, w = int(image.shape[0]), int(image.shape[1])
    S = _hw(imgsz)
    r = min(S[0] / h, S[1] / w)
    nw, nh = int(round(w * r)), int(round(h * r))
    dw, dh = (S[1] - nw) % stride, (S[0] - nh) % stride
    H, W = nh + dh, nw + dw
    dw, dh = dw / 2, dh / 2
    top, left = int(round(dh - 0.1)), int(round(dw - 0.1))
    out = torch.empty((3, H, W), dtype=torch.uint8, device=image.device)
    call("dy_aug_letterbox", ptr(image), h, w, image.stride(0), nh, nw, top, left, H, W, ptr(out), stream())
    return out, SimpleNamespace(r=r, new_unpad=(nw, nh), dw=dw, dh=dh, top=top, left=left, out_hw=(H, W))


def dark_channel_prior(img):
    """Deterministic device version of the trainer's DarkChannel / AtmLight / DarkIcA (models/yolo/detect/train.py:42-68) on the darkened
    float image batch [B, 3, H, W] in [0, 1]: returns (dedark_A [B, 3], IcA [B, 1, H, W]) as preprocess_batch stores them (:95-96).
    Semantics where the reference leaves them open (ties of its unstable argsort, the uninitialised rows of DarkIcA's buffer) are the
    ones oracle/augment.py documents: ties by pixel index, rows >= 3 by the per-channel formula."""
    from .._C import call
    from ..ops import ptr, stream
    if img.dtype != torch.float32 or not img.is_cuda or img.dim() != 4 or img.shape[1] != 3:
        raise RuntimeError("dark_channel_prior expects the f32 device image batch [B, 3, H, W]")
    img = img.contiguous()
    B, _, H, W = img.shape
    A = torch.empty((B, 3), dtype=torch.float32, device=img.device)
    ica = torch.empty((B, 1, H, W), dtype=torch.float32, device=img.device)
    call("dy_dark_channel_prior", ptr(img), B, H, W, ptr(A), ptr(ica), stream())
    return A, ica


# ---------------------------------------------------------------------------------------------------------------- classify
# Pinned to the reference: center_crop_rect (CenterCrop, data/augment.py:879-891) and, through it, the val / predict / augment=False
# transform classify_transforms = CenterCrop(size) + ToTensor() (:799-806, 894-907).  NOT pinned: the training augmentation.  The
# reference's chain is classify_albumentations (:814-855: RandomResizedCrop, flips, ColorJitter) and needs a package that is absent, so
# plan_cls_sample is this project's own rule over the parameters the reference hands to that chain.
CLS_RATIO = (3.0 / 4.0, 4.0 / 3.0)                            # aspect-ratio interval of the random resized crop
CLS_ATTEMPTS = 10


def ClassifyHyp(**kw):
    """the augmentation parameters of the classify training set: the cfg keys the reference passes to classify_albumentations
    (scale -> (1 - scale, 1), fliplr, flipud, hsv_h / hsv_s / hsv_v) with cfg/default.yaml's values"""
    d = dict(scale=0.5, fliplr=0.5, flipud=0.0, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4)
    d.update(kw)
    return SimpleNamespace(**d)


def center_crop_rect(h, w):
    """the window of the reference's CenterCrop (data/augment.py:887-891) in an h x w image as (x0, y0, cw, ch): m = min(h, w),
    top = (h - m) // 2, left = (w - m) // 2; the window is then resized to (size, size) with cv2.INTER_LINEAR"""
    m = min(int(h), int(w))
    return (int(w) - m) // 2, (int(h) - m) // 2, m, m


def plan_cls_sample(shape, hyp, rnd=_random, nprnd=np.random):
    """Random draws of ONE classify training sample.  This augmentation is the PROJECT'S OWN: the reference's training chain
    (classify_albumentations) cannot run or be pinned here, so only its parameters are kept -- scale=(1 - hyp.scale, 1), hflip =
    hyp.fliplr, vflip = hyp.flipud, and hsv_h / hsv_s / hsv_v, which it turns into ColorJitter(v, v, s, h) and which drive the detect
    pipeline's RandomHSV tables (hsv_luts) here instead.  `shape` = (H, W) of the decoded image.  Draws, in this order, only from the
    generators passed in:
      1. random resized crop (skipped, with no draw, when hyp.scale == 0: the full image).  Up to 10 attempts, each two draws:
         s = rnd.uniform(1 - hyp.scale, 1), r = exp(rnd.uniform(log 3/4, log 4/3)); w = round(sqrt(H W s r)), h = round(sqrt(H W s / r))
         (Python's round); accepted when 0 < w <= W and 0 < h <= H, then y0 = rnd.randint(0, H - h), x0 = rnd.randint(0, W - w) and no
         further attempt.  All ten refused: the central crop with the image's ratio W / H clamped to [3/4, 4/3] -- below 3/4:
         w = W, h = round(W / (3/4)); above 4/3: h = H, w = round(H * 4/3); else the full image -- at y0 = (H - h) // 2, x0 = (W - w) // 2;
      2. fliplr = rnd.random() < hyp.fliplr;  3. flipud = rnd.random() < hyp.flipud (both always drawn);
      4. when any of hsv_h / hsv_s / hsv_v is non-zero: nprnd.uniform(-1, 1, 3) * [hsv_h, hsv_s, hsv_v] + 1 -> hsv_luts.
    Returns a SimpleNamespace(rect=(x0, y0, cw, ch), fliplr, flipud, hsv_gains (None without gains), luts)."""
    H, W = int(shape[0]), int(shape[1])
    rect = None
    if hyp.scale == 0:
        rect = (0, 0, W, H)
    else:
        area, lo, hi = H * W, math.log(CLS_RATIO[0]), math.log(CLS_RATIO[1])
        for _ in range(CLS_ATTEMPTS):
            s = rnd.uniform(1 - hyp.scale, 1)
            r = math.exp(rnd.uniform(lo, hi))
            w, h = int(round(math.sqrt(area * s * r))), int(round(math.sqrt(area * s / r)))
            if 0 < w <= W and 0 < h <= H:
                y0 = rnd.randint(0, H - h)
                rect = (rnd.randint(0, W - w), y0, w, h)
                break
        if rect is None:
            ratio = W / H
            if ratio < CLS_RATIO[0]:
                w, h = W, int(round(W / CLS_RATIO[0]))
            elif ratio > CLS_RATIO[1]:
                w, h = int(round(H * CLS_RATIO[1])), H
            else:
                w, h = W, H
            rect = ((W - w) // 2, (H - h) // 2, w, h)
    p = SimpleNamespace(rect=rect, hsv_gains=None, luts=None)
    p.fliplr = rnd.random() < hyp.fliplr
    p.flipud = rnd.random() < hyp.flipud
    if hyp.hsv_h or hyp.hsv_s or hyp.hsv_v:
        p.hsv_gains = nprnd.uniform(-1, 1, 3) * [hyp.hsv_h, hyp.hsv_s, hyp.hsv_v] + 1
        p.luts = hsv_luts(p.hsv_gains)
    return p


def center_plan(shape):
    """the plan of the centre-crop transform: no flips, no colour gains"""
    return SimpleNamespace(rect=center_crop_rect(*shape), fliplr=False, flipud=False, hsv_gains=None, luts=None)


def cls_descriptors(n, buffer=None):
    """numpy record view of n dy_cls_sample over `buffer` (a uint8 host tensor, e.g. a pinned staging slot) or over fresh memory"""
    import ctypes as C
    from .._C import ClsSample
    dt = np.dtype(dict(names=["src", "pitch", "sh", "sw", "x0", "y0", "cw", "ch", "fliplr", "flipud", "hsv", "reserved", "lut"],
                       formats=["<u8", "<i8"] + ["<i4"] * 10 + [("u1", (3, 256))],
                       offsets=[getattr(ClsSample, f).offset for f, _ in ClsSample._fields_], itemsize=C.sizeof(ClsSample)))
    if buffer is None:
        return np.zeros(n, dtype=dt)
    return buffer.numpy()[:n * dt.itemsize].view(dt)


def fill_cls_descriptors(desc, images, plans):
    """writes one dy_cls_sample per (image, plan): `images[k]` the uint8 HWC BGR device tensor plan k reads (any row pitch)"""
    for k, (im, p) in enumerate(zip(images, plans)):
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.stride(2) != 1 or im.stride(1) != 3 or not im.is_cuda:
            raise ValueError("classify render: images must be device uint8 HWC tensors with 3 packed channels")
        x0, y0, cw, ch = p.rect
        if not (cw > 0 and ch > 0 and x0 >= 0 and y0 >= 0 and x0 + cw <= im.shape[1] and y0 + ch <= im.shape[0]):
            raise ValueError(f"classify render: crop {p.rect} is empty or not inside its {im.shape[0]} x {im.shape[1]} image")
        d = desc[k]
        d["src"], d["pitch"], d["sh"], d["sw"] = im.data_ptr(), im.stride(0), im.shape[0], im.shape[1]
        d["x0"], d["y0"], d["cw"], d["ch"] = x0, y0, cw, ch
        d["fliplr"], d["flipud"], d["hsv"], d["reserved"] = int(p.fliplr), int(p.flipud), int(p.hsv_gains is not None), 0
        if p.hsv_gains is not None:
            d["lut"][0], d["lut"][1], d["lut"][2] = p.luts


def cls_render(images, plans, imgsz, staging=None):
    """uint8 [B, 3, S, S] planar RGB of B (image, plan) pairs: ONE dy_cls_render launch on the current stream.  `staging`: optional
    pinned uint8 host tensor the descriptors are written into and copied from without blocking; without it they come from pageable
    memory.  B == 0 gives an empty batch."""
    from .._C import ClsSample, call
    from ..ops import ptr, stream
    import ctypes as C
    B, S = len(plans), int(imgsz)
    if len(images) != B:
        raise ValueError("classify render: one image per plan")
    dev = images[0].device if B else torch.device("cuda")
    out = torch.empty((B, 3, S, S), dtype=torch.uint8, device=dev)
    if B == 0:
        return out
    nbytes = B * C.sizeof(ClsSample)
    host = staging[:nbytes] if staging is not None else torch.empty(nbytes, dtype=torch.uint8)
    fill_cls_descriptors(cls_descriptors(B, host), images, plans)
    desc = host.to(dev, non_blocking=staging is not None)
    call("dy_cls_render", ptr(desc), B, S, ptr(out), stream())
    return out


def center_crop_batch(images, imgsz):
    """the reference's classify_transforms up to its / 255 (CenterCrop(imgsz) + ToTensor's HWC BGR -> CHW RGB) for a list of decoded
    uint8 HWC BGR device images: uint8 [B, 3, imgsz, imgsz]"""
    return cls_render(images, [center_plan(im.shape[:2]) for im in images], imgsz)
