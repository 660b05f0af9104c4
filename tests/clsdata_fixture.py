"""A deterministic tiny classification dataset tree for tests/test_clsdata_cpu.py, tests/test_gpu_clsdata.py and
tests/golden/make_clsdata_golden.py (which runs the reference's check_cls_dataset and CenterCrop over it).  Lossless PNGs of seeded
random pixels (every decoder yields the same bytes) plus one EXIF-rotated JPEG.

  main/        train/{ant,bee,cat}: ant holds a nested sub-folder, a .txt file (ignored) and an upper-case .PNG; bee holds the
               orientation-6 JPEG; val/ with the same three classes
  only_test/   train/ and test/, no val/ (split='val' falls back to test/)
  mismatch/    val/ lacks `cat` and has `dog` instead
  empty_class/ train/cat holds no image file
  no_train/    a val/ folder only
"""
import os

import numpy as np

CLASSES = ["ant", "bee", "cat"]
ROOTS = ["main", "only_test", "mismatch", "empty_class", "no_train"]
# (relative path below main/train, (h, w)) in image_folder order: classes sorted, inside a class directories and names sorted
# (upper-case letters sort before lower-case ones; a directory's own files come before those of its sub-directories)
TRAIN = [("ant/B_upper.PNG", (40, 64)), ("ant/a0.png", (37, 53)), ("ant/a1.png", (64, 64)), ("ant/sub/a2.png", (70, 45)),
         ("ant/sub/deep/a3.png", (33, 80)), ("bee/b0.png", (50, 100)), ("bee/b1.png", (100, 50)), ("bee/b2_exif.jpg", (40, 24)),
         ("cat/c0.png", (48, 48)), ("cat/c1.png", (61, 47)), ("cat/c2.png", (35, 90)), ("cat/c3.png", (72, 72))]
TRAIN_CLS = [0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2]
CROP_SHAPES = [(37, 53), (64, 64), (5, 200), (200, 5), (1, 1), (300, 301)]          # the shapes the golden pins CenterCrop on
CROP_SIZE = 32
VAL = list(zip(["ant/v0.png", "ant/v1.png", "bee/v2.png", "bee/v3.png", "cat/v4.png", "cat/v5.png"], CROP_SHAPES))      # one per pinned shape
VAL_CLS = [0, 0, 1, 1, 2, 2]


def _png(path, g, h, w):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(path, format="PNG")


def _split(root, split, items, g):
    from PIL import Image
    for rel, (h, w) in items:
        path = os.path.join(root, split, *rel.split("/"))
        if rel.endswith(".jpg"):                               # stored w x h = 40 x 24, displayed 24 x 40 after the EXIF transpose
            exif = Image.Exif()
            exif[0x0112] = 6
            os.makedirs(os.path.dirname(path), exist_ok=True)
            Image.fromarray(g.integers(0, 256, (w, h, 3), dtype=np.uint8), "RGB").save(path, quality=95, exif=exif)
        else:
            _png(path, g, h, w)


def write_clsdata(root):
    """writes the five roots under `root` and returns {name: path}"""
    root = str(root)
    g = np.random.default_rng(2031)
    main = os.path.join(root, "main")
    _split(main, "train", TRAIN, g)
    _split(main, "val", VAL, g)
    with open(os.path.join(main, "train", "ant", "notes.txt"), "w") as f:
        f.write("not an image\n")
    with open(os.path.join(main, "train", "readme.txt"), "w") as f:          # a file next to the class folders: not a class
        f.write("classes: ant bee cat\n")
    ot = os.path.join(root, "only_test")
    _split(ot, "train", [("ant/a.png", (34, 40)), ("bee/b.png", (40, 34)), ("cat/c.png", (36, 36))], g)
    _split(ot, "test", [("ant/t0.png", (44, 40)), ("bee/t1.png", (40, 58)), ("cat/t2.png", (36, 36)), ("cat/t3.png", (50, 41))], g)
    mm = os.path.join(root, "mismatch")
    _split(mm, "train", [("ant/a.png", (34, 40)), ("bee/b.png", (40, 34)), ("cat/c.png", (36, 36))], g)
    _split(mm, "val", [("ant/a.png", (34, 40)), ("bee/b.png", (40, 34)), ("dog/d.png", (36, 36))], g)
    ec = os.path.join(root, "empty_class")
    _split(ec, "train", [("ant/a.png", (34, 40)), ("bee/b.png", (40, 34))], g)
    os.makedirs(os.path.join(ec, "train", "cat"))
    with open(os.path.join(ec, "train", "cat", "list.txt"), "w") as f:
        f.write("nothing here\n")
    _split(os.path.join(root, "no_train"), "val", [("ant/a.png", (34, 40))], g)
    return {name: os.path.join(root, name) for name in ROOTS}
