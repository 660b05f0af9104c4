#!/usr/bin/env python3
"""tests/golden/g34_clsdata.npz: the reference's OWN classify data code on the tree tests/clsdata_fixture.py writes, with the import
stand-ins of make_augment_golden.py (cv2 / torchvision are absent):
  * check_cls_dataset (ultralytics/data/utils.py:269-315) of the fixture roots that have a train/ folder, for split '', 'val' and
    'test': train / val / test relative to the root ('' for None), nc, names;
  * CenterCrop(S) (data/augment.py:879-891) on six image shapes: cv2.resize is a recorder here, so what is pinned is what the
    reference computes itself -- the window it slices (top, left, height, width, read off the view it hands to cv2.resize) and the
    dsize it asks for; the pixel arithmetic of cv2.resize stays unpinned (oracle/augment.py restates it);
  * ToTensor (:894-907) on one small array: the CHW RGB float tensor.
Results only.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_clsdata_golden.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_augment_golden as base  # noqa: E402,F401  (installs the import stand-ins, puts the reference on sys.path)
import numpy as np  # noqa: E402

import clsdata_fixture as fx  # noqa: E402
from ultralytics.data.augment import CenterCrop, ToTensor  # noqa: E402
from ultralytics.data.utils import check_cls_dataset  # noqa: E402


def crop_calls(shapes, size):
    """[top, left, h, w, dsize_w, dsize_h] of the one cv2.resize call CenterCrop(size) issues per image shape"""
    import cv2
    rows = []
    for h, w in shapes:
        im = np.zeros((h, w, 3), dtype=np.uint8)
        seen = []

        def resize(view, dsize, interpolation=None, **kw):
            off = view.__array_interface__["data"][0] - im.__array_interface__["data"][0]
            assert view.strides == im.strides and view.base is not None
            seen.append([off // im.strides[0], (off % im.strides[0]) // im.strides[1], view.shape[0], view.shape[1], dsize[0], dsize[1]])
            return np.zeros((dsize[1], dsize[0], 3), dtype=np.uint8)
        cv2.resize = resize
        out = CenterCrop(size)(im)
        assert len(seen) == 1 and out.shape == (size, size, 3)
        rows.append(seen[0])
    return np.array(rows, dtype=np.int64)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as root:
        roots = fx.write_clsdata(root)
        dicts = {}
        for name in ("main", "only_test", "mismatch", "empty_class"):
            for split in ("", "val", "test"):
                d = check_cls_dataset(roots[name], split=split)
                rel = lambda p: "" if p is None else os.path.relpath(str(p), os.path.realpath(roots[name])).replace(os.sep, "/")
                dicts[f"{name}:{split}"] = dict(train=rel(d["train"]), val=rel(d["val"]), test=rel(d["test"]), nc=int(d["nc"]),
                                                names={str(k): v for k, v in d["names"].items()})
    out["check_cls_dataset"] = np.array(json.dumps(dicts, sort_keys=True))
    out["crop_shapes"] = np.array(fx.CROP_SHAPES, dtype=np.int64)
    out["crop_size"] = np.int64(fx.CROP_SIZE)
    out["crop_calls"] = crop_calls(fx.CROP_SHAPES, fx.CROP_SIZE)
    g = np.random.default_rng(34)
    im = g.integers(0, 256, (3, 4, 3), dtype=np.uint8)
    out["totensor_in"], out["totensor_out"] = im, ToTensor()(im).numpy()
    path = os.path.join(HERE, "g34_clsdata.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")
    print(json.dumps(dicts, indent=1)[:600])
    print(out["crop_calls"])


if __name__ == "__main__":
    main()
