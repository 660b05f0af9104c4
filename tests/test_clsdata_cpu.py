"""CPU tests of the classify data layer: check_cls_dataset and center_crop_rect against the reference's own results
(tests/golden/g34_clsdata.npz, written by tests/golden/make_clsdata_golden.py), image_folder / load_cls_split on the fixture tree of
tests/clsdata_fixture.py, every error case, and plan_cls_sample -- the project's own training augmentation -- against a second, plainly
written statement of its rule."""
import json
import math
import os
import random

import numpy as np
import pytest

import clsdata_fixture as fx
from dedark_yolo_amd.data import augment as A
from dedark_yolo_amd.data import dataset as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g34():
    return np.load(os.path.join(ROOT, "tests", "golden", "g34_clsdata.npz"))


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    return fx.write_clsdata(tmp_path_factory.mktemp("clsdata"))


def _rel(p, root):
    return "" if p is None else os.path.relpath(str(p), os.path.realpath(root)).replace(os.sep, "/")


def test_check_cls_dataset_equals_the_reference(g34, roots):
    want = json.loads(str(g34["check_cls_dataset"]))
    assert len(want) == 12
    for key, w in want.items():
        name, split = key.split(":")
        d = ds.check_cls_dataset(roots[name], split)
        assert set(d) == {"train", "val", "test", "nc", "names"}
        got = dict(train=_rel(d["train"], roots[name]), val=_rel(d["val"], roots[name]), test=_rel(d["test"], roots[name]), nc=d["nc"],
                   names={str(k): v for k, v in d["names"].items()})
        assert got == w, key
    d = ds.check_cls_dataset(roots["only_test"], "val")
    assert d["val"] == d["test"] and d["val"].name == "test"                   # val falls back to test ...
    d = ds.check_cls_dataset(roots["main"], "test")
    assert d["test"] == d["val"] and d["test"].name == "val"                   # ... and test to val


def test_check_cls_dataset_errors_name_the_path(roots, tmp_path):
    missing = str(tmp_path / "nowhere")
    with pytest.raises(FileNotFoundError, match="nowhere"):
        ds.check_cls_dataset(missing)
    with pytest.raises(FileNotFoundError, match="no_train"):
        ds.check_cls_dataset(roots["no_train"])
    a_file = tmp_path / "file.txt"
    a_file.write_text("x")
    with pytest.raises(FileNotFoundError, match="file.txt"):
        ds.check_cls_dataset(str(a_file))


def test_center_crop_rect_equals_the_reference(g34):
    calls = g34["crop_calls"]
    assert [tuple(s) for s in g34["crop_shapes"]] == fx.CROP_SHAPES and int(g34["crop_size"]) == fx.CROP_SIZE
    for (h, w), (top, left, ch, cw, dw, dh) in zip(fx.CROP_SHAPES, calls):
        assert A.center_crop_rect(h, w) == (left, top, cw, ch), (h, w)
        assert (dw, dh) == (fx.CROP_SIZE, fx.CROP_SIZE)
        p = A.center_plan((h, w))
        assert p.rect == (left, top, cw, ch) and not p.fliplr and not p.flipud and p.hsv_gains is None
    # ToTensor (data/augment.py:902-907) is HWC BGR -> CHW RGB, / 255: format_img of the oracle, then the trainer's / 255
    from oracle import augment as oa
    assert np.array_equal(oa.format_img(g34["totensor_in"]).astype(np.float32) / np.float32(255.0), g34["totensor_out"])


def test_image_folder_order_classes_ids_and_suffix_filter(roots):
    train = os.path.join(roots["main"], "train")
    files, cls, classes = ds.image_folder(train)
    assert classes == fx.CLASSES
    assert [os.path.relpath(f, train).replace(os.sep, "/") for f in files] == [rel for rel, _ in fx.TRAIN]
    assert cls.dtype == np.int64 and cls.tolist() == fx.TRAIN_CLS
    assert not any(f.endswith(".txt") for f in files) and any(f.endswith(".PNG") for f in files)
    files, cls, classes = ds.image_folder(os.path.join(roots["main"], "val"))
    assert [os.path.relpath(f, os.path.join(roots["main"], "val")).replace(os.sep, "/") for f in files] == [rel for rel, _ in fx.VAL]
    assert cls.tolist() == fx.VAL_CLS
    for ext in ds.CLS_IMG_EXTENSIONS:
        assert ext == ext.lower() and ext.startswith(".")
    assert set(ds.CLS_IMG_EXTENSIONS) == {".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp"}


def test_image_folder_follows_links_and_decodes_the_shapes(roots, tmp_path):
    linked = tmp_path / "linked"
    linked.mkdir()
    for c in fx.CLASSES:
        os.symlink(os.path.join(roots["main"], "train", c), linked / c)
    files, cls, classes = ds.image_folder(str(linked))
    assert len(files) == len(fx.TRAIN) and cls.tolist() == fx.TRAIN_CLS and classes == fx.CLASSES
    for f, (_, shape) in zip(files, fx.TRAIN):
        assert ds.decode(f).shape == shape + (3,), f                           # the JPEG after its EXIF transpose: 40 x 24


def test_image_folder_errors(roots, tmp_path):
    with pytest.raises(FileNotFoundError, match="cat"):
        ds.image_folder(os.path.join(roots["empty_class"], "train"))
    empty = tmp_path / "no_classes"
    empty.mkdir()
    (empty / "stray.png").write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="no_classes"):
        ds.image_folder(str(empty))
    with pytest.raises(FileNotFoundError, match="nowhere"):
        ds.image_folder(str(tmp_path / "nowhere"))


def test_fraction_applies_to_the_training_split_only(roots):
    from types import SimpleNamespace
    data = ds.check_cls_dataset(roots["main"])
    full, cls_full = ds.load_cls_split(data, "train", SimpleNamespace(fraction=1.0))
    assert len(full) == 12
    for fr in (0.5, 0.3, 0.04):
        files, cls = ds.load_cls_split(data, "train", SimpleNamespace(fraction=fr))
        n = round(12 * fr)
        assert files == full[:n] and cls.tolist() == cls_full[:n].tolist(), fr
    files, cls = ds.load_cls_split(data, "val", SimpleNamespace(fraction=0.5))
    assert len(files) == len(fx.VAL) and cls.tolist() == fx.VAL_CLS
    assert len(ds.load_cls_split(data, "train")[0]) == 12                       # no args: everything


def test_split_with_other_class_folders_raises(roots):
    data = ds.check_cls_dataset(roots["mismatch"])
    assert len(ds.load_cls_split(data, "train")[0]) == 3
    with pytest.raises(ValueError, match="dog"):
        ds.load_cls_split(data, "val")
    with pytest.raises(ValueError, match="dog"):
        ds.load_cls_split(data, "test")                                        # test falls back to val
    data = ds.check_cls_dataset(roots["only_test"], "val")
    assert len(ds.load_cls_split(data, "val")[0]) == 4


def test_the_label_file_entries_keep_refusing_classify():
    with pytest.raises(NotImplementedError):
        ds.read_labels(["x.png"], "classify", 3)
    with pytest.raises(NotImplementedError):
        ds.task_labels([], "classify")
    with pytest.raises(ValueError):
        A.TaskLabels([], "classify", A.AugmentHyp(), None, 4, True, 64)


# ---- plan_cls_sample ------------------------------------------------------------------------------------------------------------------
def _plain_plan(H, W, hyp, rnd, nprnd):
    """the rule of plan_cls_sample's docstring, written out a second time"""
    box = None
    if hyp.scale != 0:
        for _ in range(10):
            s = rnd.uniform(1 - hyp.scale, 1)
            r = math.exp(rnd.uniform(math.log(3 / 4), math.log(4 / 3)))
            w = int(round(math.sqrt(H * W * s * r)))
            h = int(round(math.sqrt(H * W * s / r)))
            if 0 < w <= W and 0 < h <= H:
                top = rnd.randint(0, H - h)
                left = rnd.randint(0, W - w)
                box = (left, top, w, h)
                break
        if box is None:
            if W / H < 3 / 4:
                w, h = W, int(round(W / (3 / 4)))
            elif W / H > 4 / 3:
                w, h = int(round(H * (4 / 3))), H
            else:
                w, h = W, H
            box = ((W - w) // 2, (H - h) // 2, w, h)
    else:
        box = (0, 0, W, H)
    lr = rnd.random() < hyp.fliplr
    ud = rnd.random() < hyp.flipud
    gains = None
    if hyp.hsv_h or hyp.hsv_s or hyp.hsv_v:
        gains = nprnd.uniform(-1, 1, 3) * [hyp.hsv_h, hyp.hsv_s, hyp.hsv_v] + 1
    return box, lr, ud, gains


def _inside(rect, H, W):
    x0, y0, cw, ch = rect
    return cw > 0 and ch > 0 and x0 >= 0 and y0 >= 0 and x0 + cw <= W and y0 + ch <= H


SHAPES = [(37, 53), (64, 64), (300, 301), (480, 640), (500, 256), (5, 200), (200, 5), (1, 1), (2, 3), (10, 14)]


def test_plans_equal_the_plain_statement_on_200_seeded_draws():
    from oracle import augment as oa
    hyps = [A.ClassifyHyp(), A.ClassifyHyp(scale=0.92, flipud=0.5), A.ClassifyHyp(scale=0.0, hsv_h=0.0, hsv_s=0.0, hsv_v=0.0),
            A.ClassifyHyp(scale=0.2, fliplr=0.0, hsv_s=0.0, hsv_v=0.0)]
    ra, rb = random.Random(11), random.Random(11)
    na, nb = np.random.RandomState(12), np.random.RandomState(12)
    accepted = fallback = 0
    for k in range(200):
        (H, W), hyp = SHAPES[k % len(SHAPES)], hyps[k % len(hyps)]
        p = A.plan_cls_sample((H, W), hyp, ra, na)
        box, lr, ud, gains = _plain_plan(H, W, hyp, rb, nb)
        assert p.rect == box and p.fliplr == lr and p.flipud == ud, (k, H, W)
        assert _inside(p.rect, H, W), (k, p.rect)
        if gains is None:
            assert p.hsv_gains is None and p.luts is None
        else:
            assert np.array_equal(p.hsv_gains, gains)
            for got, want in zip(p.luts, oa.hsv_luts(gains)):                  # RandomHSV's tables as the detect pipeline makes them
                assert got.dtype == np.uint8 and np.array_equal(got, want)
        if (H, W) in ((5, 200), (200, 5)) and hyp.scale:
            fallback += 1
        elif hyp.scale:
            accepted += 1
    assert ra.random() == rb.random() and na.uniform() == nb.uniform()         # both generators consumed equally far
    assert accepted > 50 and fallback > 10


def test_same_seed_same_plans_and_other_seed_other_plans():
    def run(seed):
        r, n = random.Random(seed), np.random.RandomState(seed + 1)
        return [A.plan_cls_sample(s, A.ClassifyHyp(), r, n) for s in SHAPES * 3]
    a, b, c = run(5), run(5), run(6)
    assert all(x.rect == y.rect and x.fliplr == y.fliplr and x.flipud == y.flipud and np.array_equal(x.hsv_gains, y.hsv_gains)
               for x, y in zip(a, b))
    assert any(x.rect != y.rect for x, y in zip(a, c))


def test_scale_zero_gives_the_full_image_and_draws_no_crop():
    r = random.Random(3)
    twin = random.Random(3)
    for H, W in SHAPES:
        p = A.plan_cls_sample((H, W), A.ClassifyHyp(scale=0.0, hsv_h=0.0, hsv_s=0.0, hsv_v=0.0), r, None)       # no numpy draw either
        assert p.rect == (0, 0, W, H)
        twin.random(), twin.random()                                           # the two flip coins are all that is drawn
    assert r.random() == twin.random()


def test_degenerate_shapes_fall_back_and_stay_inside():
    """(5, 200) and (200, 5): every attempt wants both sides near sqrt(area) = 32, above the short side, so all ten are refused and the
    central crop with the ratio clamped to 4/3 (3/4) is taken -- 7 x 5 (5 x 7) in the middle, after exactly twenty crop draws.  (1, 1):
    sqrt(s r) and sqrt(s / r) lie in [0.61, 1.16] for the default scale, both sides round to 1 and the FIRST attempt is accepted;
    the fallback of a 1 x 1 image would be the same single pixel."""
    hyp = A.ClassifyHyp(hsv_h=0.0, hsv_s=0.0, hsv_v=0.0)
    r, twin = random.Random(9), random.Random(9)
    for _ in range(20):
        assert A.plan_cls_sample((5, 200), hyp, r, None).rect == (96, 0, 7, 5)
        assert A.plan_cls_sample((200, 5), hyp, r, None).rect == (0, 96, 5, 7)
        for _ in range(2 * (10 * 2 + 2)):                                      # per sample: ten attempts of two draws, two flip coins
            twin.random()
    assert r.random() == twin.random()
    for _ in range(50):
        assert A.plan_cls_sample((1, 1), hyp, r, None).rect == (0, 0, 1, 1)


def test_flip_frequencies_at_p_zero_and_one():
    r, n = random.Random(1), np.random.RandomState(2)
    never = [A.plan_cls_sample((40, 50), A.ClassifyHyp(fliplr=0.0, flipud=0.0), r, n) for _ in range(300)]
    always = [A.plan_cls_sample((40, 50), A.ClassifyHyp(fliplr=1.0, flipud=1.0), r, n) for _ in range(300)]
    assert not any(p.fliplr or p.flipud for p in never) and all(p.fliplr and p.flipud for p in always)
    half = [A.plan_cls_sample((40, 50), A.ClassifyHyp(), r, n) for _ in range(400)]
    assert 120 < sum(p.fliplr for p in half) < 280 and not any(p.flipud for p in half)


def test_descriptor_records_match_the_c_struct():
    import ctypes as C
    from dedark_yolo_amd._C import ClsSample
    d = A.cls_descriptors(3)
    assert d.dtype.itemsize == C.sizeof(ClsSample) == 824
    for name, _ in ClsSample._fields_:
        assert d.dtype.fields[name][1] == getattr(ClsSample, name).offset, name
    host = np.zeros(2 * 824, dtype=np.uint8)
    import torch
    view = A.cls_descriptors(2, torch.from_numpy(host))
    view[1]["x0"], view[1]["lut"][2][255] = 7, 9
    c = ClsSample.from_buffer(host, 824)
    assert c.x0 == 7 and c.lut[2][255] == 9
