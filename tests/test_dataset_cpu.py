"""CPU tests of the dataset layer (dedark_yolo_amd/data/dataset.py): the label reader, class filters and rect order against
tests/golden/g26_dataset.npz -- the reference's own verify_image_label / get_labels / update_labels / set_rectangle on the tree
tests/dataset_fixture.py writes (tests/golden/make_dataset_golden.py) -- the data yaml checks, and tests/resize_area_ref.py (the
project's statement of cv2.INTER_AREA, the reference of dy_aug_resize_area_u8) against float64 box integration."""
import os

import numpy as np
import pytest

import dataset_fixture as fx
import resize_area_ref as rar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g26():
    return np.load(os.path.join(ROOT, "tests", "golden", "g26_dataset.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("dataset")
    return str(root), fx.write_dataset(root)


def _rel(root, f):
    return os.path.relpath(f, root).replace(os.sep, "/")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _read(root, name):
    from dedark_yolo_amd.data import dataset as ds
    path, task, kpt = fx.set_path(root, name)
    files = ds.get_img_files(path)
    return files, ds.read_labels(files, task, fx.set_nc(name), kpt)


@pytest.mark.parametrize("name", list(fx.SETS))
def test_labels_match_the_reference_reader(g26, tree, name):
    root, _ = tree
    files, (labels, counts) = _read(root, name)
    assert [_rel(root, f) for f in files] == list(g26[f"{name}_all_files"])
    assert tuple(counts) == tuple(int(v) for v in g26[f"{name}_counts"])           # (missing, found, empty, corrupt)
    assert [_rel(root, lab["im_file"]) for lab in labels] == list(g26[f"{name}_files"])
    for i, lab in enumerate(labels):
        assert tuple(lab["shape"]) == tuple(int(v) for v in g26[f"{name}_shapes"][i])
        assert _same(lab["cls"], g26[f"{name}_{i}_cls"]) and _same(lab["bboxes"], g26[f"{name}_{i}_bboxes"]), (name, i)
        assert lab["normalized"] is True and lab["bbox_format"] == "xywh"
        assert len(lab["segments"]) == int(g26[f"{name}_{i}_nseg"])
        for j, s in enumerate(lab["segments"]):
            assert _same(s, g26[f"{name}_{i}_seg{j}"])
        key = f"{name}_{i}_keypoints"
        assert (lab["keypoints"] is None) == (key not in g26.files)
        if lab["keypoints"] is not None:
            assert _same(lab["keypoints"], g26[key])


def test_the_fixture_cases_are_what_they_claim(tree):
    root, _ = tree
    _, (labels, counts) = _read(root, "det_train")
    kept = {os.path.basename(lab["im_file"]): lab for lab in labels}
    assert counts == (1, 9, 1, 4)
    assert not {"e_gt1.png", "f_neg.png", "h_clsbig.png", "i_small.png"} & set(kept)
    assert float(kept["g_clsnc.png"]["cls"][0, 0]) == fx.NC                       # class id == nc passes (the reference's `<=`)
    assert len(kept["b_missing.png"]["cls"]) == 0 and len(kept["c_empty.png"]["cls"]) == 0
    assert len(kept["d_dup.png"]["cls"]) == 3                                      # 4 rows, one duplicate
    assert kept["j_exif.jpg"]["shape"] == (40, 24)                                 # stored 24 x 40, EXIF orientation 6
    assert "k_nested.png" in kept
    from dedark_yolo_amd.data.dataset import decode
    assert decode(kept["j_exif.jpg"]["im_file"]).shape == (40, 24, 3)
    im = decode(kept["a_normal.png"]["im_file"])
    from PIL import Image
    assert im.dtype == np.uint8 and np.array_equal(im[:, :, ::-1], np.asarray(Image.open(kept["a_normal.png"]["im_file"])))   # BGR
    _, (pose2, _) = _read(root, "pose2")
    assert pose2[1]["keypoints"].shape[1:] == (5, 3) and float(pose2[1]["keypoints"][0, 2, 2]) == 0.0


def test_update_labels_single_cls_and_classes(g26, tree):
    import copy
    from dedark_yolo_amd.data.dataset import update_labels
    root, _ = tree
    _, (labels, _) = _read(root, "det_train")
    for tag, single, classes in (("single", True, None), ("classes", False, [1, 2])):
        got = update_labels(copy.deepcopy(labels), single_cls=single, classes=classes)
        for i, lab in enumerate(got):
            assert _same(lab["cls"], g26[f"det_train_{tag}_{i}_cls"]) and _same(lab["bboxes"], g26[f"det_train_{tag}_{i}_bboxes"])
    _, (seg, _) = _read(root, "seg")
    got = update_labels(copy.deepcopy(seg), classes=[1])
    assert [len(lab["segments"]) for lab in got] == [int((lab["cls"] == 1).sum()) for lab in seg]


def test_set_rectangle_matches_the_reference(g26, tree):
    from dedark_yolo_amd.data.dataset import set_rectangle
    root, _ = tree
    _, (labels, _) = _read(root, "det_val")
    for k, (imgsz, batch, stride, pad) in enumerate(fx.RECT_CASES):
        order, bi, shapes = set_rectangle([lab["shape"] for lab in labels], batch, imgsz, stride, pad)
        assert np.array_equal(order, g26[f"rect{k}_order"]) and np.array_equal(bi, g26[f"rect{k}_batch"])
        assert np.array_equal(shapes, g26[f"rect{k}_batch_shapes"])
    assert len({tuple(s) for s in g26["rect0_batch_shapes"]}) == 3                 # wide, square and tall batches


def test_check_det_dataset(tree):
    from dedark_yolo_amd.data.dataset import check_det_dataset, get_img_files
    root, yamls = tree
    names = {0: "cat", 1: "dog", 2: "bird"}
    d = check_det_dataset(yamls["det"])                                           # relative `path`, names as a list
    assert d["nc"] == 3 and d["names"] == names and str(d["path"]) == os.path.join(root, "det")
    assert d["train"] == os.path.join(root, "det", "images", "train") and d["val"] == os.path.join(root, "det", "images", "val")
    d = check_det_dataset(yamls["det_list"])                                      # list splits, names as a dict
    assert d["names"] == names and d["train"] == [os.path.join(root, "det", "train.txt"), os.path.join(root, "det", "images", "train", "nested")]
    assert [os.path.basename(f) for f in get_img_files(d["train"])] == ["a_normal.png", "d_dup.png", "k_nested.png", "k_nested.png"]
    d = check_det_dataset(yamls["det_nc"])                                        # names absent
    assert d["names"] == {0: "class_0", 1: "class_1", 2: "class_2"} and d["nc"] == 3
    d = check_det_dataset(yamls["pose2"])
    assert d["kpt_shape"] == [5, 2] and d["flip_idx"] == [0, 2, 1, 4, 3] and d["nc"] == 1
    with pytest.raises(FileNotFoundError, match="nowhere"):
        check_det_dataset(yamls["bad_split"])
    with pytest.raises(SyntaxError):
        check_det_dataset(yamls["bad_nc"])
    with pytest.raises(FileNotFoundError):
        check_det_dataset(os.path.join(root, "absent.yaml"))


def test_get_img_files_fraction_and_list_file(tree):
    from dedark_yolo_amd.data.dataset import get_img_files, img2label_paths
    root, _ = tree
    train = os.path.join(root, "det", "images", "train")
    files = get_img_files(train)
    assert len(files) == 11 and files == sorted(files)
    assert get_img_files(train, fraction=0.5) == files[:round(11 * 0.5)]
    listed = get_img_files(os.path.join(root, "det", "train.txt"))
    assert [_rel(root, f) for f in listed] == ["det/images/train/a_normal.png", "det/images/train/d_dup.png", "det/images/train/nested/k_nested.png"]
    assert _rel(root, img2label_paths(listed)[2]) == "det/labels/train/nested/k_nested.txt"
    with pytest.raises(FileNotFoundError):
        get_img_files(os.path.join(root, "det", "images", "none"))


def test_classify_is_refused_and_pools_are_capped():
    from dedark_yolo_amd.data import dataset as ds
    with pytest.raises(NotImplementedError):
        ds.read_labels(["x.png"], "classify", 3)
    with pytest.raises(NotImplementedError):
        ds.task_labels([], "classify")
    assert ds.pool_size(8) == 8 and ds.pool_size(1000) == 16 and ds.pool_size(0) == 1


# ---- the numpy statement of INTER_AREA -------------------------------------------------------------------------------------------
AREA_SHAPES = [((33, 47), rar.load_image_shape(33, 47, 32)), ((65, 64), rar.load_image_shape(65, 64, 64)),
               ((129, 128), rar.load_image_shape(129, 128, 64)), ((64, 128), (32, 64)), ((96, 192), rar.load_image_shape(96, 192, 64)),
               ((300, 11), rar.load_image_shape(300, 11, 64)), ((97, 131), rar.load_image_shape(97, 131, 64)), ((1000, 999), (640, 640))]


@pytest.mark.parametrize("src_hw,dst_hw", AREA_SHAPES)
def test_area_reference_against_exact_box_integration(src_hw, dst_hw):
    """|ref - exact| <= 0.5 (the one rounding) + 2 * 255 * 1e-3 (the two dropped slivers of at most 1e-3 source pixel, at full scale)
    + 1e-3 (float32 slack) = 1.011"""
    g = np.random.default_rng(src_hw[0] * 1000 + src_hw[1])
    src = g.integers(0, 256, src_hw + (3,), dtype=np.uint8)
    ref = rar.resize_area_u8(src, *dst_hw)
    exact = rar.exact_box(src, *dst_hw)
    assert ref.shape == exact.shape == dst_hw + (3,)
    err = float(np.abs(ref.astype(np.float64) - exact).max())
    assert err <= 0.5 + 2 * 255 * 1e-3 + 1e-3, err


@pytest.mark.parametrize("value", [0, 1, 128, 255])
def test_area_reference_keeps_constant_images_constant(value):
    for (sh, sw), (dh, dw) in AREA_SHAPES[:7] + [((45, 70), (20, 31)), ((100, 100), (99, 37)), ((640, 480), (427, 320))]:
        src = np.full((sh, sw, 3), value, dtype=np.uint8)
        assert (rar.resize_area_u8(src, dh, dw) == value).all(), ((sh, sw), (dh, dw))
        assert float(np.abs(rar.area_sums(src, dh, dw) - value).max()) <= 1e-4 * max(value, 1)


def test_area_reference_rounds_ties_to_even_at_exact_2_to_1():
    src = np.zeros((2, 4, 3), dtype=np.uint8)
    src[0, 0], src[0, 1] = 1, 1                                # mean 0.5 -> 0
    src[:, 2:] = 1
    src[0, 2] = 3                                              # mean 1.5 -> 2
    out = rar.resize_area_u8(src, 1, 2)
    assert out[0, 0, 0] == 0 and out[0, 1, 0] == 2


def test_train_without_loader_or_data_raises_value_error():
    from dedark_yolo_amd.engine.model import YOLO
    with pytest.raises(ValueError, match="data=.*loader="):
        YOLO("yolov8n.yaml").train()
