#!/usr/bin/env python3
"""tests/golden/g20_augseg.npz, g20_augpose.npz: the reference's OWN training transforms (ultralytics/data/augment.py `v8_transforms` +
`Format(return_mask / return_keypoint)`) on the seeded synthetic segment / pose datasets of tests/augtask_data.py, the way
make_augment_golden.py made g13 (whose cv2 / easydict / torchvision stand-ins are reused by importing it).

Two more cv2 stand-ins are needed for polygon2mask (data/utils.py:137-155): cv2.fillPoly RECORDS the int32 polygon it is handed and fills
by the project's stated pixel rule (tests/polymask_ref.fill_closed), cv2.resize of a 2-D mask is oracle.augment.cv_resize_linear_u8.
So everything the reference computes itself is pinned -- the polygons / keypoints through mosaic, affine, clip, filter, flips and
Format (with every re-resampling of Instances.__init__), segment2box, the area order and the composition of polygons2masks_overlap --
and the pixel rule stays the project's own.

The reference orders instances with numpy's default argsort of -areas (unstable for ties; uint64 areas, so an EMPTY mask would also sort
first).  The generator therefore re-seeds the dataset until the mask areas within every image are pairwise distinct and non-zero: the
reference's order is then unambiguous and equals the product's rule (area descending, ties by index), and no sample is left out.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_augtask_golden.py
"""
import os
import random
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_augment_golden as base  # noqa: E402  (installs the import stand-ins, puts the reference on sys.path)
import numpy as np  # noqa: E402
import cv2  # noqa: E402  (the stand-in module)

import polymask_ref as pr  # noqa: E402
from augtask_data import CASES, IMGSZ, synth_task_dataset  # noqa: E402
from oracle import augment as oa  # noqa: E402
from ultralytics.data import augment as ua  # noqa: E402
from ultralytics.data.augment import Format, v8_transforms  # noqa: E402
from ultralytics.utils.instance import Instances  # noqa: E402

REC = dict(polys=[], sorted_idx=[], flips=[])


def fill_poly(mask, polygons, color=1):
    assert polygons.dtype == np.int32 and polygons.shape[0] == 1
    REC["polys"].append(polygons[0].copy())
    mask[pr.fill_closed(polygons[0], mask.shape[0], mask.shape[1]) != 0] = color


_base_resize = cv2.resize


def resize(img, dsize, interpolation=None, **kw):
    if img.ndim == 2:
        if tuple(dsize) == img.shape[::-1]:
            return img.copy()
        return oa.cv_resize_linear_u8(img[..., None], dsize)[..., 0]
    return _base_resize(img, dsize, interpolation=interpolation, **kw)


cv2.fillPoly = fill_poly
cv2.resize = resize
_overlap = ua.polygons2masks_overlap


def overlap_recording(imgsz, segments, downsample_ratio=1):
    masks, index = _overlap(imgsz, segments, downsample_ratio=downsample_ratio)
    REC["sorted_idx"].append(np.array(index))
    return masks, index


ua.polygons2masks_overlap = overlap_recording
for _name in ("flipud", "fliplr"):
    def _wrap(fn, name):
        def f(self, x):
            REC["flips"].append(name)
            return fn(self, x)
        return f
    setattr(Instances, _name, _wrap(getattr(Instances, _name), _name))


class FakeDataset:
    """what Mosaic / MixUp / v8_transforms need from YOLODataset: buffer, __len__, get_image_and_label (update_labels_info builds the
    Instances from the raw polygons / keypoints, dataset.py:157-169), data, use_keypoints"""

    def __init__(self, ims, labels, kind, flip_idx, K):
        self.ims, self.labels = ims, labels
        self.buffer = list(range(len(ims)))
        self.use_keypoints = kind == "pose"
        self.data = dict(flip_idx=flip_idx or [], kpt_shape=[K, 3])

    def __len__(self):
        return len(self.ims)

    def get_image_and_label(self, i):
        im, lab = self.ims[i].copy(), self.labels[i]
        out = dict(im_file=f"img{i}.jpg", cls=lab["cls"].copy(), img=im, ori_shape=im.shape[:2], resized_shape=im.shape[:2], ratio_pad=(1.0, 1.0))
        segs = [s.copy() for s in lab.get("segments", [])]
        kp = None
        if self.use_keypoints:                                        # the label reader's visibility column (data/utils.py:124-128)
            kp = lab["keypoints"].copy()
            if kp.shape[-1] == 2:
                m = np.ones(kp.shape[:2], dtype=np.float32)
                m = np.where(kp[..., 0] < 0, 0.0, m)
                m = np.where(kp[..., 1] < 0, 0.0, m)
                kp = np.concatenate([kp, m[..., None]], axis=-1)
        out["instances"] = Instances(lab["bboxes"].copy(), segs, kp, bbox_format="xywh", normalized=True)
        return out


def run_case(tag, seed):
    kind, dkw, n_img, picks, over, ratio, overlap, flip_idx = CASES[tag]
    hyp = SimpleNamespace(**dict(base.HYP, **over))
    ims, labels = synth_task_dataset(seed, n_img, IMGSZ, kind, **dkw)
    ds = FakeDataset(ims, labels, kind, flip_idx, dkw.get("K", 17))
    tf = v8_transforms(ds, IMGSZ, hyp)
    tf.append(Format(bbox_format="xywh", normalize=True, return_mask=kind == "segment", return_keypoint=kind == "pose", batch_idx=True,
                     mask_ratio=ratio, mask_overlap=overlap))
    out = dict(data_seed=seed, hyp=np.array([hyp.degrees, hyp.translate, hyp.scale, hyp.shear, hyp.perspective, hyp.hsv_h, hyp.hsv_s, hyp.hsv_v,
                                            hyp.flipud, hyp.fliplr, hyp.mosaic]))
    random.seed(seed + 1)
    np.random.seed(seed + 2)
    flips = set()
    for k, idx in enumerate(picks):
        for v in list(base.REC.values()) + list(REC.values()):
            v.clear()
        s = tf(ds.get_image_and_label(idx))
        out[f"n{k}_M"] = base.REC["warp"][0]["M"]
        out[f"n{k}_flips"] = np.array([int("flipud" in REC["flips"]), int("fliplr" in REC["flips"])])
        flips |= set(REC["flips"])
        nl = len(s["batch_idx"])
        out[f"n{k}_cls"] = s["cls"].numpy().reshape(-1, 1).astype(np.float32)
        out[f"n{k}_bboxes"] = s["bboxes"].numpy().reshape(-1, 4).astype(np.float32)
        if kind == "pose":
            out[f"n{k}_keypoints"] = s["keypoints"].numpy()
        else:
            assert len(REC["polys"]) == nl
            polys = np.stack(REC["polys"]) if nl else np.zeros((0, 1000, 2), np.int32)
            assert polys.min(initial=0) >= 0 and polys.max(initial=0) <= IMGSZ
            out[f"n{k}_polys"] = polys.astype(np.int16)
            m = s["masks"].numpy()
            out[f"n{k}_masks"] = m.astype(np.uint8)
            if nl:
                planes = pr.polygons2masks(polys, IMGSZ, IMGSZ, ratio)
                areas = planes.reshape(nl, -1).sum(1)
                if len(set(areas.tolist())) != nl or areas.min() == 0:
                    return None                                            # ambiguous order under the reference's argsort: re-seed
                if overlap:
                    idx_ref = REC["sorted_idx"][0]
                    assert np.array_equal(idx_ref, pr.stable_order(areas))
                    out[f"n{k}_sorted_idx"] = idx_ref.astype(np.int32)
                    want, _, _ = pr.polygons2masks_overlap(polys, IMGSZ, IMGSZ, ratio)
                    assert np.array_equal(m[0], want)                      # the reference's composition == the stated rule
                else:
                    assert np.array_equal(m, planes)
            elif overlap:
                out[f"n{k}_sorted_idx"] = np.zeros(0, np.int32)
    out["flips_seen"] = np.array([int("flipud" in flips), int("fliplr" in flips)])
    out["rng_after"] = np.array([random.random(), np.random.uniform()])      # both generators consumed exactly as far as the reference
    return out


def main():
    files = dict(g20_augseg={}, g20_augpose={})
    for tag in CASES:
        seed = 2000 + 10 * list(CASES).index(tag)
        while True:
            res = run_case(tag, seed)
            if res is not None:
                break
            seed += 1000
        n_inst = [len(res[f"n{k}_cls"]) for k in range(len(CASES[tag][3]))]
        print(tag, "data seed", seed, "instances per sample", n_inst, "flips seen", res["flips_seen"])
        if tag in ("s1", "p1"):
            assert 0 in n_inst, "the case must contain an image that ends with no instances"
        for k, v in res.items():
            files["g20_augseg" if CASES[tag][0] == "segment" else "g20_augpose"][f"{tag}_{k}"] = v
    for name, out in files.items():
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB,", len(out), "arrays")


if __name__ == "__main__":
    main()
