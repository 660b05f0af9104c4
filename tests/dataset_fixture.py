"""A deterministic tiny dataset tree for the dataset-layer tests (tests/test_dataset_cpu.py, tests/test_gpu_dataset.py) and for
tests/golden/make_dataset_golden.py, which runs the reference's own label reader over the same tree.  Images are lossless PNGs of
seeded random pixels (every decoder yields the same bytes) plus one EXIF-rotated JPEG.

  det/   images/train: a normal pair, a missing label file, an empty one, duplicate rows, a coordinate > 1 (corrupt), a negative value
         (corrupt), a class id == nc (passes: the reference tests `<=`), one above it (corrupt), a 9 x 40 image (corrupt), an EXIF
         orientation-6 JPEG, and a pair in a nested directory; train.txt lists three of them with './' paths;
         images/val: 9 images of aspect ratio below 1 (4), equal to 1 (2) and above 1 (3), most of them larger than 64 px
  seg/   polygon labels;  pose2/ and pose3/: keypoint labels for kpt_shape [5, 2] and [5, 3]
"""
import os

import numpy as np

NC = 3
NAMES = ["cat", "dog", "bird"]
SETS = dict(det_train=("det", "images/train", "detect", None), det_list=("det", "train.txt", "detect", None),
            det_val=("det", "images/val", "detect", None), seg=("seg", "images/train", "segment", None),
            pose2=("pose2", "images/train", "pose", (5, 2)), pose3=("pose3", "images/train", "pose", (5, 3)))
VAL_SHAPES = [(50, 100), (60, 90), (35, 80), (45, 70), (64, 64), (80, 80), (100, 50), (90, 60), (72, 40)]       # (h, w)
RECT_CASES = [(64, 4, 32, 0.5), (96, 2, 32, 0.0)]             # (imgsz, batch, stride, pad)


def _png(path, g, h, w):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(path)


def _txt(path, rows):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        for r in rows:
            f.write(" ".join([str(int(r[0]))] + [f"{v:.6f}" for v in r[1:]]) + "\n")


def _boxes(g, n, cls_hi=NC):
    xy, wh = g.uniform(0.3, 0.7, (n, 2)), g.uniform(0.1, 0.5, (n, 2))
    return [[int(g.integers(0, cls_hi))] + list(xy[i]) + list(wh[i]) for i in range(n)]


def write_dataset(root):
    """writes the tree under `root` and returns {name: yaml path}"""
    from PIL import Image
    root = str(root)
    g = np.random.default_rng(2026)
    im = lambda *p: os.path.join(root, "det", "images", *p)
    lb = lambda *p: os.path.join(root, "det", "labels", *p)
    _png(im("train", "a_normal.png"), g, 32, 48)
    _txt(lb("train", "a_normal.txt"), [[1, 0.5, 0.5, 0.4, 0.3], [0, 0.25, 0.3, 0.2, 0.2]])
    _png(im("train", "b_missing.png"), g, 40, 40)
    _png(im("train", "c_empty.png"), g, 36, 20)
    _txt(lb("train", "c_empty.txt"), [])
    _png(im("train", "d_dup.png"), g, 30, 44)
    _txt(lb("train", "d_dup.txt"), [[2, 0.6, 0.6, 0.2, 0.2], [0, 0.4, 0.4, 0.3, 0.1], [2, 0.6, 0.6, 0.2, 0.2], [1, 0.2, 0.7, 0.1, 0.2]])
    _png(im("train", "e_gt1.png"), g, 32, 32)
    _txt(lb("train", "e_gt1.txt"), [[0, 0.5, 1.2, 0.2, 0.2]])
    _png(im("train", "f_neg.png"), g, 32, 32)
    _txt(lb("train", "f_neg.txt"), [[0, 0.5, -0.1, 0.2, 0.2]])
    _png(im("train", "g_clsnc.png"), g, 32, 40)
    _txt(lb("train", "g_clsnc.txt"), [[NC, 0.5, 0.5, 0.2, 0.2]])
    _png(im("train", "h_clsbig.png"), g, 32, 40)
    _txt(lb("train", "h_clsbig.txt"), [[NC + 1, 0.5, 0.5, 0.2, 0.2]])
    _png(im("train", "i_small.png"), g, 9, 40)
    _txt(lb("train", "i_small.txt"), [[0, 0.5, 0.5, 0.2, 0.2]])
    exif = Image.Exif()
    exif[0x0112] = 6                                           # stored 24 x 40 (h x w), displayed 40 x 24
    os.makedirs(im("train"), exist_ok=True)
    Image.fromarray(g.integers(0, 256, (24, 40, 3), dtype=np.uint8), "RGB").save(im("train", "j_exif.jpg"), quality=95, exif=exif)
    _txt(lb("train", "j_exif.txt"), [[1, 0.5, 0.4, 0.3, 0.5]])
    _png(im("train", "nested", "k_nested.png"), g, 28, 52)
    _txt(lb("train", "nested", "k_nested.txt"), [[2, 0.45, 0.55, 0.5, 0.4]])
    with open(os.path.join(root, "det", "train.txt"), "w") as f:
        f.write("./images/train/a_normal.png\n./images/train/nested/k_nested.png\n./images/train/d_dup.png\n")
    for k, (h, w) in enumerate(VAL_SHAPES):
        _png(im("val", f"v{k}.png"), g, h, w)
        _txt(lb("val", f"v{k}.txt"), _boxes(g, 1 + k % 3))
    # polygons: 3, 5 and 4 points
    sp = lambda *p: os.path.join(root, "seg", *p)
    _png(sp("images", "train", "s0.png"), g, 48, 64)
    _txt(sp("labels", "train", "s0.txt"), [[0, 0.1, 0.1, 0.6, 0.2, 0.4, 0.8], [2, 0.5, 0.5, 0.9, 0.5, 0.95, 0.7, 0.7, 0.9, 0.5, 0.8]])
    _png(sp("images", "train", "s1.png"), g, 64, 40)
    _txt(sp("labels", "train", "s1.txt"), [[1, 0.2, 0.3, 0.8, 0.3, 0.8, 0.7, 0.2, 0.7]])
    _png(sp("images", "train", "s2.png"), g, 40, 64)
    _txt(sp("labels", "train", "s2.txt"), [[1, 0.3, 0.2, 0.7, 0.25, 0.6, 0.9, 0.35, 0.8], [0, 0.05, 0.5, 0.5, 0.55, 0.3, 0.95]])
    for name, ndim in (("pose2", 2), ("pose3", 3)):
        pp = lambda *p: os.path.join(root, name, *p)
        for k, (h, w) in enumerate([(48, 64), (64, 36), (40, 64)]):
            _png(pp("images", "train", f"p{k}.png"), g, h, w)
            rows = []
            for b in _boxes(g, 1 + k % 2, cls_hi=1):
                kp = g.uniform(0.1, 0.9, (5, 2))
                if ndim == 3:
                    kp = np.concatenate((kp, g.integers(0, 3, (5, 1)).astype(float)), 1)
                elif k == 1:
                    kp[2, 0] = -0.5                            # ndim == 2: a negative coordinate gets visibility 0
                rows.append(b + list(kp.reshape(-1)))
            _txt(pp("labels", "train", f"p{k}.txt"), rows)
    yamls = {}
    docs = dict(
        det="path: det\ntrain: images/train\nval: images/val\nnames: [cat, dog, bird]\n",
        det_list="path: det\ntrain: [train.txt, images/train/nested]\nval: [images/val]\nnames:\n  0: cat\n  1: dog\n  2: bird\n",
        det_nc="path: det\ntrain: images/train\nval: images/val\nnc: 3\n",
        seg="path: seg\ntrain: images/train\nval: images/train\nnames: [cat, dog, bird]\n",
        pose2="path: pose2\ntrain: images/train\nval: images/train\nnames: [person]\nkpt_shape: [5, 2]\nflip_idx: [0, 2, 1, 4, 3]\n",
        pose3="path: pose3\ntrain: images/train\nval: images/train\nnames: [person]\nkpt_shape: [5, 3]\nflip_idx: [0, 2, 1, 4, 3]\n",
        det_trainval="path: det\ntrain: images/val\nval: images/val\nnames: [cat, dog, bird]\n",
        bad_split="path: det\ntrain: images/train\nval: images/nowhere\nnames: [cat, dog, bird]\n",
        bad_nc="path: det\ntrain: images/train\nval: images/val\nnc: 4\nnames: [cat, dog, bird]\n")
    for k, text in docs.items():
        yamls[k] = os.path.join(root, f"{k}.yaml")
        with open(yamls[k], "w") as f:
            f.write(text)
    return yamls


def set_path(root, name):
    sub, rel, task, kpt = SETS[name]
    return os.path.join(str(root), sub, *rel.split("/")), task, kpt


def set_nc(name):
    return 1 if name.startswith("pose") else NC
