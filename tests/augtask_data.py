"""Seeded synthetic segment / pose datasets shared by tests/golden/make_augtask_golden.py (which runs the reference on them) and the
tests (which run the product on the same inputs).  TEST INFRASTRUCTURE."""
import numpy as np

COCO_FLIP_IDX = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
K5_FLIP_IDX = [1, 0, 2, 4, 3]


def synth_task_dataset(seed, n, imgsz, kind, fixed_long_side=False, empty=(), K=17, ndim=3):
    """n decoded BGR images (48..96 px a side for imgsz 64; with fixed_long_side the long side is imgsz, as load_image leaves it) with
    3..6 instances each: kind 'segment' -> `segments` (5..12-vertex star-shaped polygons, normalised) and their bounding boxes;
    kind 'pose' -> boxes and `keypoints` [k, K, ndim] inside them (a few negative = unlabelled for ndim 2).  Images listed in `empty`
    have no instances."""
    g = np.random.default_rng(seed)
    lo, hi = (3 * imgsz) // 4, (3 * imgsz) // 2
    ims, labels = [], []
    for i in range(n):
        if fixed_long_side:
            h, w = (imgsz, int(g.integers(lo, imgsz + 1))) if i % 2 else (int(g.integers(lo, imgsz + 1)), imgsz)
        else:
            h, w = int(g.integers(lo, hi + 1)), int(g.integers(lo, hi + 1))
        ims.append(g.integers(0, 256, (h, w, 3), dtype=np.uint8))
        k = 0 if i in empty else int(g.integers(3, 7))
        cls = g.integers(0, 20, (k, 1)).astype(np.float32)
        cxy = g.uniform(0.25, 0.75, (k, 2))
        lab = dict(cls=cls)
        if kind == "segment":
            segs, boxes = [], []
            for j in range(k):
                nv = int(g.integers(5, 13))
                ang = np.sort(g.uniform(0, 2 * np.pi, nv))
                rad = g.uniform(0.08, 0.30, nv)
                p = np.clip(cxy[j] + np.stack((rad * np.cos(ang), rad * np.sin(ang)), 1), 0.0, 1.0).astype(np.float32)
                segs.append(p)
                boxes.append([(p[:, 0].min() + p[:, 0].max()) / 2, (p[:, 1].min() + p[:, 1].max()) / 2, p[:, 0].max() - p[:, 0].min(),
                              p[:, 1].max() - p[:, 1].min()])
            lab["segments"] = segs
            lab["bboxes"] = np.array(boxes, dtype=np.float32).reshape(-1, 4)
        else:
            wh = g.uniform(0.15, 0.45, (k, 2))
            lab["bboxes"] = np.concatenate((cxy, wh), 1).astype(np.float32)
            kp = cxy[:, None, :] + g.uniform(-0.5, 0.5, (k, K, 2)) * wh[:, None, :]
            if ndim == 3:
                kp = np.concatenate((kp, g.integers(0, 3, (k, K, 1)).astype(np.float64)), -1)
            else:
                kp = np.where(g.uniform(0, 1, (k, K, 1)) < 0.15, -1.0, kp)           # unlabelled points: negative coordinates
            lab["keypoints"] = kp.astype(np.float32)
        labels.append(lab)
    return ims, labels


CASES = {
    # tag: (kind, dataset keywords, number of images, picks, hyper-parameter overrides, mask_ratio, overlap_mask, flip_idx)
    "s0": ("segment", dict(), 6, [0, 3, 5, 1], dict(degrees=10.0, shear=2.0, flipud=0.5, fliplr=0.5), 4, True, None),
    "s1": ("segment", dict(fixed_long_side=True, empty=(2,)), 5, [0, 1, 2, 3, 4], dict(mosaic=0.0, degrees=5.0, flipud=0.5), 1, True, None),
    "s2": ("segment", dict(), 5, [4, 2, 0], dict(translate=0.2, scale=0.3), 2, False, None),
    "p0": ("pose", dict(K=17, ndim=3), 6, [0, 2, 5, 3], dict(degrees=10.0, flipud=0.5, fliplr=0.5), 4, True, COCO_FLIP_IDX),
    "p1": ("pose", dict(K=5, ndim=2, fixed_long_side=True, empty=(1,)), 5, [0, 1, 2, 3], dict(mosaic=0.0, fliplr=1.0), 4, True, K5_FLIP_IDX),
}
IMGSZ = 64
