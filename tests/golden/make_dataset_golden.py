#!/usr/bin/env python3
"""tests/golden/g26_dataset.npz: the reference's OWN label reader on the tree tests/dataset_fixture.py writes -- verify_image_label
through YOLODataset.get_labels (cache_labels), BaseDataset.get_img_files / update_labels / set_rectangle -- with the import
stand-ins of make_augment_golden.py (cv2 / easydict / torchvision are absent; none of the functions run here touches a pixel).
Results only: per set the kept files (relative to the tree), shapes, cls, bboxes, segments, keypoints, the counts
(missing, found, empty, corrupt); update_labels(single_cls) and update_labels(classes=[1, 2]) on det_train; the rect order, batch index
and batch shapes of det_val for every dataset_fixture.RECT_CASES.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dataset_golden.py
"""
import copy
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_augment_golden as base  # noqa: E402,F401  (installs the import stand-ins, puts the reference on sys.path)
import numpy as np  # noqa: E402

import dataset_fixture as fx  # noqa: E402
from ultralytics.data.dataset import YOLODataset  # noqa: E402


def ref_dataset(path, task, kpt, nc):
    """a YOLODataset up to get_labels, built field by field (its __init__ goes on to the cv2 transforms)"""
    ds = YOLODataset.__new__(YOLODataset)
    ds.use_segments, ds.use_keypoints = task == "segment", task == "pose"
    ds.data = dict(names={i: str(i) for i in range(nc)})
    if kpt:
        ds.data["kpt_shape"] = list(kpt)
    ds.img_path, ds.prefix, ds.fraction, ds.single_cls = path, "", 1.0, False
    ds.im_files = ds.get_img_files(path)
    ds.labels = ds.get_labels()
    return ds


def main():
    out = {}
    with tempfile.TemporaryDirectory() as root:
        fx.write_dataset(root)
        rel = lambda f: os.path.relpath(f, root).replace(os.sep, "/")
        for name in fx.SETS:
            path, task, kpt = fx.set_path(root, name)
            ds = ref_dataset(path, task, kpt, fx.set_nc(name))
            cache = np.load(str(next(p for p in _caches(root))), allow_pickle=True).item()
            nf, nm, ne, ncor, _ = cache["results"]
            for p in list(_caches(root)):
                os.remove(p)
            out[f"{name}_counts"] = np.array([nm, nf, ne, ncor], dtype=np.int64)
            out[f"{name}_files"] = np.array([rel(l["im_file"]) for l in ds.labels])
            out[f"{name}_all_files"] = np.array([rel(f) for f in ds.get_img_files(path)])
            out[f"{name}_shapes"] = np.array([l["shape"] for l in ds.labels], dtype=np.int64)
            for i, l in enumerate(ds.labels):
                assert l["normalized"] is True and l["bbox_format"] == "xywh"
                out[f"{name}_{i}_cls"], out[f"{name}_{i}_bboxes"] = l["cls"], l["bboxes"]
                out[f"{name}_{i}_nseg"] = np.int64(len(l["segments"]))
                for j, s in enumerate(l["segments"]):
                    out[f"{name}_{i}_seg{j}"] = s
                if l["keypoints"] is not None:
                    out[f"{name}_{i}_keypoints"] = l["keypoints"]
            if name == "det_train":
                for tag, single, classes in (("single", True, None), ("classes", False, [1, 2])):
                    d2 = copy.copy(ds)
                    d2.labels, d2.single_cls = copy.deepcopy(ds.labels), single
                    d2.update_labels(include_class=classes)
                    for i, l in enumerate(d2.labels):
                        out[f"{name}_{tag}_{i}_cls"], out[f"{name}_{tag}_{i}_bboxes"] = l["cls"], l["bboxes"]
            if name == "det_val":
                for k, (imgsz, batch, stride, pad) in enumerate(fx.RECT_CASES):
                    d2 = copy.copy(ds)
                    d2.labels, d2.im_files = copy.deepcopy(ds.labels), list(ds.im_files)
                    d2.ni, d2.batch_size, d2.imgsz, d2.stride, d2.pad = len(d2.labels), batch, imgsz, stride, pad
                    before = list(d2.im_files)
                    d2.set_rectangle()
                    out[f"rect{k}_order"] = np.array([before.index(f) for f in d2.im_files], dtype=np.int64)
                    out[f"rect{k}_batch"] = np.asarray(d2.batch, dtype=np.int64)
                    out[f"rect{k}_batch_shapes"] = np.asarray(d2.batch_shapes, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "g26_dataset.npz"), **out)
    print("wrote g26_dataset.npz:", len(out), "arrays")


def _caches(root):
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".cache"):
                yield os.path.join(d, f)


if __name__ == "__main__":
    main()
