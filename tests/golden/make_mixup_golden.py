#!/usr/bin/env python3
"""tests/golden/g24_mixup.npz, g24_mixseg.npz, g24_mixpose.npz: the reference's OWN training transforms with MixUp switched on
(ultralytics/data/augment.py `v8_transforms`: MixUp :272-288 over pre_transform = [Mosaic, CopyPaste(p=0), RandomPerspective], then
`Format`) on the seeded datasets of tests/mixup_ref.py, the way make_augment_golden.py / make_augtask_golden.py made g13 / g20 (whose
cv2 / easydict / torchvision stand-ins, fillPoly / mask-resize stand-ins and fake dataset are reused by importing them).

One stand-in differs: cv2.warpAffine RECORDS its arguments and returns the project's own restated warp (oracle.augment.
cv_warp_affine_linear_u8) of the canvas it was handed instead of the placeholder pattern.  So the reference's own
`(img1 * r + img2 * (1 - r)).astype(np.uint8)` runs on real pixels and its result is recorded: cvtColor / LUT stay identity stand-ins, the
final `img` is flips + Format of the blend.  Pinned: the draw order of both generators (partner index, the partner's own mosaic coin /
partners / centre / affine draws, r from numpy before RandomHSV's gains), both canvases and matrices, the blend, and the merged labels
(boxes, the polygons handed to fillPoly in primary-then-partner order, the area order over the merged set, keypoints with flip_idx).

The dataset is re-seeded until the mask areas within every merged image are pairwise distinct and non-zero (the reference's argsort is
unstable for ties) and until the half-mixed cases (d1, s1, p1: mixup 0.5, mosaic 0.5) contain: a mixed sample whose primary ends without
instances next to a partner with some, the reverse, an un-mixed sample, a partner on the letterbox path and one on the mosaic path and
both flips; d1 also a mixed sample with no instance on either side.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mixup_golden.py
"""
import os
import random
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_augtask_golden as task  # noqa: E402  (installs every stand-in, puts the reference on sys.path)
import numpy as np  # noqa: E402
import cv2  # noqa: E402  (the stand-in module)

import polymask_ref as pr  # noqa: E402
from mixup_ref import FILES, MIX_CASES, mix_dataset  # noqa: E402
from oracle import augment as oa  # noqa: E402
from ultralytics.data import augment as ua  # noqa: E402
from ultralytics.data.augment import Format, v8_transforms  # noqa: E402

base = task.base
REC = dict(warp=[], partner=[], r=[], counts=[])


def warp_affine(img, M, dsize=None, borderValue=None, **kw):
    assert tuple(borderValue) == (114, 114, 114)
    REC["warp"].append(dict(img=img.copy(), M=np.array(M).copy(), dsize=tuple(dsize)))
    return oa.cv_warp_affine_linear_u8(img, M, dsize)


cv2.warpAffine = warp_affine
_get_indexes, _mix_transform, _beta = ua.MixUp.get_indexes, ua.MixUp._mix_transform, np.random.beta


def get_indexes(self):
    i = _get_indexes(self)
    REC["partner"].append(int(i))
    return i


def mix_transform(self, labels):
    REC["counts"].append((len(labels["instances"]), len(labels["mix_labels"][0]["instances"])))
    assert labels["img"].dtype == np.uint8 and labels["mix_labels"][0]["img"].dtype == np.uint8
    return _mix_transform(self, labels)


def beta(a, b):
    r = _beta(a, b)
    REC["r"].append(float(r))
    return r


ua.MixUp.get_indexes, ua.MixUp._mix_transform, np.random.beta = get_indexes, mix_transform, beta


def run_case(tag, seed):
    kind, imgsz, n_img, _, picks, over, ratio, flip_idx = MIX_CASES[tag]
    hyp = SimpleNamespace(**dict(base.HYP, **over))
    ims, labels = mix_dataset(seed, tag)
    ds = task.FakeDataset(ims, labels, kind, flip_idx, 17)
    tf = v8_transforms(ds, imgsz, hyp)
    tf.append(Format(bbox_format="xywh", normalize=True, return_mask=kind == "segment", return_keypoint=kind == "pose", batch_idx=True,
                     mask_ratio=ratio, mask_overlap=True))
    out = dict(data_seed=seed, hyp=np.array([hyp.degrees, hyp.translate, hyp.scale, hyp.shear, hyp.perspective, hyp.hsv_h, hyp.hsv_s, hyp.hsv_v,
                                            hyp.flipud, hyp.fliplr, hyp.mosaic, hyp.mixup]))
    random.seed(seed + 1)
    np.random.seed(seed + 2)
    seen = set()
    for k, idx in enumerate(picks):
        for v in list(base.REC.values()) + list(task.REC.values()) + list(REC.values()):
            v.clear()
        s = tf(ds.get_image_and_label(idx))
        mixed = len(REC["partner"]) == 1
        assert len(REC["warp"]) == 1 + mixed and len(REC["r"]) == mixed and len(base.REC["lut"]) == 3
        w = REC["warp"][0]
        assert w["dsize"] == (imgsz, imgsz)
        out[f"n{k}_canvas"], out[f"n{k}_M"] = w["img"], w["M"]
        out[f"n{k}_partner"] = np.array(REC["partner"][0] if mixed else -1)
        out[f"n{k}_lut"] = np.stack(base.REC["lut"])
        out[f"n{k}_flips"] = np.array([int("flipud" in task.REC["flips"]), int("fliplr" in task.REC["flips"])])
        seen |= set(task.REC["flips"])
        if mixed:
            w2 = REC["warp"][1]
            out[f"n{k}_canvas2"], out[f"n{k}_M2"], out[f"n{k}_r"] = w2["img"], w2["M"], np.array(REC["r"][0])
            out[f"n{k}_counts"] = np.array(REC["counts"][0])
            n1, n2 = REC["counts"][0]
            seen |= {"mixed", "letterbox partner" if w2["img"].shape[0] == imgsz else "mosaic partner"}
            seen |= {("primary empty" if n2 else "both empty") if n1 == 0 else ("partner empty" if n2 == 0 else "both")}
        else:
            seen.add("un-mixed")
        seen.add("letterbox primary" if w["img"].shape[0] == imgsz else "mosaic primary")
        nl = len(s["batch_idx"])
        assert not mixed or nl == sum(REC["counts"][0])
        out[f"n{k}_cls"] = s["cls"].numpy().reshape(-1, 1).astype(np.float32)
        out[f"n{k}_bboxes"] = s["bboxes"].numpy().reshape(-1, 4).astype(np.float32)
        out[f"n{k}_img"] = s["img"].numpy()                      # flips + Format (CHW, RGB) of the reference's blend
        if kind == "pose":
            out[f"n{k}_keypoints"] = s["keypoints"].numpy()
        elif kind == "segment":
            assert len(task.REC["polys"]) == nl
            polys = np.stack(task.REC["polys"]) if nl else np.zeros((0, 1000, 2), np.int32)
            assert polys.min(initial=0) >= 0 and polys.max(initial=0) <= imgsz
            out[f"n{k}_polys"] = polys.astype(np.int16)
            m = s["masks"].numpy()
            out[f"n{k}_masks"] = m.astype(np.uint8)
            out[f"n{k}_sorted_idx"] = np.zeros(0, np.int32)
            if nl:
                areas = pr.polygons2masks(polys, imgsz, imgsz, ratio).reshape(nl, -1).sum(1)
                if len(set(areas.tolist())) != nl or areas.min() == 0:
                    return None, seen                                      # ambiguous order under the reference's argsort: re-seed
                idx_ref = task.REC["sorted_idx"][0]
                assert np.array_equal(idx_ref, pr.stable_order(areas))
                out[f"n{k}_sorted_idx"] = idx_ref.astype(np.int32)
                want, _, _ = pr.polygons2masks_overlap(polys, imgsz, imgsz, ratio)
                assert np.array_equal(m[0], want)                          # the reference's composition == the stated rule
    out["rng_after"] = np.array([random.random(), np.random.uniform()])      # both generators consumed exactly as far as the reference
    return out, seen


NEED = {"mixed", "un-mixed", "primary empty", "partner empty", "both", "letterbox partner", "mosaic partner", "letterbox primary",
        "mosaic primary", "flipud", "fliplr"}


def main():
    files = {name: {} for name in FILES.values()}
    for n, tag in enumerate(MIX_CASES):
        seed = 2400 + 10 * n
        while True:
            res, seen = run_case(tag, seed)
            half = MIX_CASES[tag][5]["mixup"] < 1.0
            need = (NEED | ({"both empty"} if tag == "d1" else set())) if half else {"flipud"}
            print(tag, seed, res is not None, sorted(need - seen), flush=True)
            if res is not None and need <= seen:
                break
            seed += 1000
        print(tag, "data seed", seed, "instances per sample", [len(res[f"n{k}_cls"]) for k in range(len(MIX_CASES[tag][4]))], sorted(seen))
        for k, v in res.items():
            files[FILES[MIX_CASES[tag][0]]][f"{tag}_{k}"] = v
    for name, out in files.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB,", len(out), "arrays")


if __name__ == "__main__":
    main()
