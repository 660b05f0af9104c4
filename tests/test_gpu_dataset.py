"""GPU tests of the dataset layer: dy_aug_resize_area_u8 byte for byte against tests/resize_area_ref.py (the project's statement of
cv2.INTER_AREA; unpinned against cv2), load_resize's interpolation choice (base.py:152-157), DeviceValLoader (rect batches) against the
g26 golden + the numpy composition area_ref -> oracle letterbox -> format_img, build_train_loader against a hand-built
DeviceAugmentLoader, and train(data=) / val(data=) / predict(paths) end to end on the fixture set of tests/dataset_fixture.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import resize_area_ref as rar  # noqa: E402

pytestmark = pytest.mark.gpu

# (source h, w) -> (dh, dw): as load_image yields them at imgsz, or given outright
AREA_CASES = {
    "33x47@32": ((33, 47), rar.load_image_shape(33, 47, 32)),            # non-integer ratio, unequal axes
    "65x64@64": ((65, 64), rar.load_image_shape(65, 64, 64)),            # ratio just above 1: every cell is two slivers
    "129x128@64": ((129, 128), rar.load_image_shape(129, 128, 64)),
    "64x128->32x64": ((64, 128), (32, 64)),                              # exact 2:1, .5 ties
    "96x192@64": ((96, 192), rar.load_image_shape(96, 192, 64)),         # 3:1
    "300x11@64": ((300, 11), rar.load_image_shape(300, 11, 64)),         # 3-column output
    "97x131@64": ((97, 131), rar.load_image_shape(97, 131, 64)),
    "1000x999->640x640": ((1000, 999), (640, 640)),                      # the min(ceil, imgsz) cap, the largest tables
}


def _image(name, shape):
    g = np.random.default_rng(sum(map(ord, name)))
    return g.integers(0, 256, shape + (3,), dtype=np.uint8)


def _area(src_t, dh, dw, dst=None):
    from dedark_yolo_amd._C import call
    from dedark_yolo_amd.ops import ptr, stream
    out = torch.empty((dh, dw, 3), dtype=torch.uint8, device="cuda") if dst is None else dst
    call("dy_aug_resize_area_u8", ptr(src_t), src_t.shape[0], src_t.shape[1], src_t.stride(0), ptr(out), dh, dw, out.stride(0), stream())
    return out


@pytest.mark.parametrize("name", list(AREA_CASES))
def test_area_kernel_vs_numpy_reference(name):
    (sh, sw), (dh, dw) = AREA_CASES[name]
    src = _image(name, (sh, sw))
    want = rar.resize_area_u8(src, dh, dw)
    if name == "64x128->32x64":                               # the fixture must hold .5 ties (the scalar rule rounds them to even)
        s = rar.area_sums(src, dh, dw)
        assert (np.abs(s - np.floor(s) - 0.5) == 0).any()
    got = _area(torch.from_numpy(src).cuda(), dh, dw).cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} of {want.size} bytes differ, max |d| {int(np.abs(got.astype(int) - want).max())}"


def test_area_kernel_pitched_views_and_guard_bytes():
    sh, sw, dh, dw = 45, 70, 20, 31
    src = _image("pitch", (sh, sw))
    want = rar.resize_area_u8(src, dh, dw)
    big = torch.full((sh, sw + 9, 3), 201, dtype=torch.uint8, device="cuda")
    big[:, :sw] = torch.from_numpy(src).cuda()
    canvas = torch.full((dh + 2, dw + 5, 3), 77, dtype=torch.uint8, device="cuda")
    _area(big[:, :sw], dh, dw, dst=canvas[1:dh + 1, 2:dw + 2])
    c = canvas.cpu().numpy()
    assert np.array_equal(c[1:dh + 1, 2:dw + 2], want)
    guard = np.ones(c.shape[:2], dtype=bool)
    guard[1:dh + 1, 2:dw + 2] = False
    assert (c[guard] == 77).all()


def test_area_kernel_refuses_bad_arguments():
    from dedark_yolo_amd._C import lib
    from dedark_yolo_amd.ops import ptr, stream
    src = torch.zeros((16, 16, 3), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((32, 32, 3), dtype=torch.uint8, device="cuda")
    f = lib().dy_aug_resize_area_u8
    assert f(ptr(src), 16, 16, 48, ptr(dst), 17, 16, 96, stream()) == 1          # dh > sh
    assert f(ptr(src), 16, 16, 48, ptr(dst), 16, 17, 96, stream()) == 1          # dw > sw
    assert f(None, 16, 16, 48, ptr(dst), 8, 8, 96, stream()) == 1                # null source
    assert f(ptr(src), 16, 16, 48, None, 8, 8, 96, stream()) == 1                # null destination
    assert f(ptr(src), 16, 16, 47, ptr(dst), 8, 8, 96, stream()) == 1            # source pitch below 3 * w
    assert f(ptr(src), 16, 16, 48, ptr(dst), 8, 8, 23, stream()) == 1            # destination pitch below 3 * w
    torch.cuda.synchronize()
    assert int(dst.sum()) == 0


def test_load_resize_picks_area_when_shrinking_and_linear_otherwise():
    from dedark_yolo_amd.data.augment import load_resize
    from oracle import augment as oa
    src = _image("load", (97, 131))
    t = torch.from_numpy(src).cuda()
    dh, dw = rar.load_image_shape(97, 131, 64)
    assert np.array_equal(load_resize(t, 64, augment=False).cpu().numpy(), rar.resize_area_u8(src, dh, dw))
    linear = oa.cv_resize_linear_u8(src, (dw, dh))
    assert np.array_equal(load_resize(t, 64, augment=True).cpu().numpy(), linear)
    assert torch.equal(load_resize(t, 64), load_resize(t, 64, augment=True))            # the default is today's call
    uh, uw = rar.load_image_shape(97, 131, 160)
    up = oa.cv_resize_linear_u8(src, (uw, uh))
    assert np.array_equal(load_resize(t, 160, augment=False).cpu().numpy(), up)          # r > 1 stays linear
    assert load_resize(t, 131, augment=False) is t


# ---- loaders and the public interface on the fixture set --------------------------------------------------------------------------
import dataset_fixture as fx  # noqa: E402


@pytest.fixture(scope="module")
def g26():
    return np.load(os.path.join(ROOT, "tests", "golden", "g26_dataset.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("dataset")
    return str(root), fx.write_dataset(root)


def _val_set(root):
    from dedark_yolo_amd.data import dataset as ds
    path, task, kpt = fx.set_path(root, "det_val")
    files = ds.get_img_files(path)
    labels, _ = ds.read_labels(files, task, fx.NC, kpt)
    return files, labels


def test_val_loader_rect_batches_against_golden_and_numpy(g26, tree):
    from dedark_yolo_amd.data import DeviceValLoader
    from dedark_yolo_amd.data.augment import val_labels
    from dedark_yolo_amd.data.dataset import decode
    from oracle import augment as oa
    root, _ = tree
    files, labels = _val_set(root)
    imgsz, bs, stride, pad = fx.RECT_CASES[0]
    loader = DeviceValLoader(files, labels, imgsz, bs, stride=stride, pad=pad, rect=True)
    order, bidx, shapes = g26["rect0_order"], g26["rect0_batch"], g26["rect0_batch_shapes"]
    assert loader.order == [int(i) for i in order] and len(loader) == 3
    first = list(loader)
    assert [len(b["im_file"]) for b in first] == [4, 4, 1]                         # the last, partial batch is there
    k = 0
    for bi, b in enumerate(first):
        H, W = (int(v) for v in shapes[bi])
        assert tuple(b["img"].shape) == (len(b["im_file"]), 3, H, W) and b["img"].dtype == torch.uint8
        got = b["img"].cpu().numpy()
        cls, boxes, idx = [], [], []
        for j, f in enumerate(b["im_file"]):
            i = int(order[k])
            assert f == files[i] and int(bidx[k]) == bi
            src = decode(f)
            h0, w0 = src.shape[:2]
            r = imgsz / max(h0, w0)
            rs = src
            if r != 1:
                dh, dw = rar.load_image_shape(h0, w0, imgsz)
                rs = rar.resize_area_u8(src, dh, dw) if r < 1 else oa.cv_resize_linear_u8(src, (dw, dh))
            want = oa.format_img(oa.letterbox(rs, (H, W), scaleup=False))
            assert np.array_equal(got[j], want), f"{f}: {int((got[j] != want).sum())} bytes differ"
            bb, (_, (dw_, dh_)), _ = val_labels(g26[f"det_val_{i}_bboxes"], rs.shape[:2], imgsz, rect_shape=(H, W))
            cls.append(g26[f"det_val_{i}_cls"]), boxes.append(bb), idx.append(np.full(len(bb), j, dtype=np.float32))
            assert b["ori_shape"][j] == (h0, w0) and b["resized_shape"][j] == rs.shape[:2]
            # the gain validation scales predictions back with is load_image's ratio (base.py:245-246); the pad is LetterBox's
            assert b["ratio_pad"][j] == ((rs.shape[0] / h0, rs.shape[1] / w0), (dw_, dh_))
            k += 1
        assert np.array_equal(b["cls"].numpy(), np.concatenate(cls)) and np.array_equal(b["bboxes"].numpy(), np.concatenate(boxes))
        assert np.array_equal(b["batch_idx"].numpy(), np.concatenate(idx))
    second = list(loader)                                                          # a second epoch: identical bytes
    for a, b in zip(first, second):
        assert torch.equal(a["img"], b["img"]) and torch.equal(a["bboxes"], b["bboxes"])


@pytest.mark.parametrize("name,yaml_key", [("det_val", "det_trainval"), ("seg", "seg"), ("pose2", "pose2")])
def test_train_loader_equals_hand_built_loader(tree, name, yaml_key):
    from dedark_yolo_amd.data import DeviceAugmentLoader, build_train_loader, check_det_dataset
    from dedark_yolo_amd.data import dataset as ds
    from dedark_yolo_amd.data.augment import load_resize
    from dedark_yolo_amd.data.loader import _augment_hyp
    from dedark_yolo_amd.engine.trainer import get_cfg
    root, yamls = tree
    path, task, kpt = fx.set_path(root, name)
    data = check_det_dataset(yamls[yaml_key])
    args = get_cfg(dict(imgsz=64, batch=2, seed=3, mixup=0.5))
    built = build_train_loader(args, data, task, "cuda")
    files = ds.get_img_files(path)
    labels, _ = ds.read_labels(files, task, data["nc"], kpt)
    images = [load_resize(torch.from_numpy(ds.decode(f)).cuda(), 64) for f in files]
    hand = DeviceAugmentLoader(images, ds.task_labels(labels, task), 64, 2, hyp=_augment_hyp(args), seed=3, task=task,
                               flip_idx=data.get("flip_idx"))
    assert built.resident and len(built) == len(hand) >= 1
    n = 0
    for _ in range(2):                                        # a 3-image set has one batch per epoch: the second one comes from the next
        for a, b in zip(built, hand):                         # epoch, after the shuffle and every draw of the first
            assert set(a) == set(b)
            for key in a:
                if torch.is_tensor(a[key]):
                    assert torch.equal(a[key], b[key]), key
                else:
                    assert a[key] == b[key], key
            n += 1
            if n == 2:
                break
        if n == 2:
            break
    assert n == 2


def _hand_geometry(shape, rect):
    """LetterBox(scaleup=False) of an image that is already at its load_image size inside a rect batch: r, dw, dh"""
    r = min(rect[0] / shape[0], rect[1] / shape[1], 1.0)
    nw, nh = int(round(shape[1] * r)), int(round(shape[0] * r))
    return r, (rect[1] - nw) / 2, (rect[0] - nh) / 2


def _to_rect(e, shape, rect):
    """normalised x, y -> pixels of the letter-boxed rect image, float32 step by step (Instances.denormalize / scale / add_padding)"""
    r, dw, dh = _hand_geometry(shape, rect)
    e = np.array(e, dtype=np.float32, copy=True)
    e[..., 0] *= shape[1]
    e[..., 1] *= shape[0]
    e[..., 0] *= r
    e[..., 1] *= r
    e[..., 0] += dw
    e[..., 1] += dh
    return e


def _fixture_val_loader(root, name, imgsz=64, bs=2):
    from dedark_yolo_amd.data import DeviceValLoader
    from dedark_yolo_amd.data import dataset as ds
    path, task, kpt = fx.set_path(root, name)
    files = ds.get_img_files(path)
    labels, _ = ds.read_labels(files, task, fx.set_nc(name), kpt)
    return DeviceValLoader(files, labels, imgsz, bs, stride=32, pad=0.5, rect=True, task=task), files, labels


def test_val_loader_segment_masks_at_rect_shapes(tree):
    """masks of a rect batch against the numpy polygon oracle (tests/polymask_ref.py), polygons placed by hand"""
    import polymask_ref as pr
    from dedark_yolo_amd.data.augment import resample_segments
    loader, files, labels = _fixture_val_loader(tree[0], "seg")
    by_file = dict(zip(files, labels))
    seen = 0
    for bi, b in enumerate(loader):
        H, W = (int(v) for v in loader.batch_shapes[bi])
        assert tuple(b["img"].shape[2:]) == (H, W) and tuple(b["masks"].shape) == (len(b["im_file"]), H // 4, W // 4)
        polys, rows, offsets = [], [], [0]
        for j, f in enumerate(b["im_file"]):
            lab, shape = by_file[f], b["resized_shape"][j]
            assert shape == tuple(lab["shape"])                # the fixture images are at their load_image size already
            px = _to_rect(resample_segments(lab["segments"]), shape, (H, W)).astype(np.int32)
            box = _to_rect(np.concatenate((lab["bboxes"][:, :2] - lab["bboxes"][:, 2:] / 2, lab["bboxes"][:, :2] + lab["bboxes"][:, 2:] / 2), 1)
                           .reshape(-1, 2, 2), shape, (H, W)).reshape(-1, 4)
            xywh = np.stack(((box[:, 0] + box[:, 2]) / 2 / W, (box[:, 1] + box[:, 3]) / 2 / H, (box[:, 2] - box[:, 0]) / W,
                             (box[:, 3] - box[:, 1]) / H), 1)
            polys.append(px)
            rows.append(np.concatenate((np.full((len(px), 1), j, np.float32), lab["cls"], xywh.astype(np.float32)), 1))
            offsets.append(offsets[-1] + len(px))
        masks, rows_sorted, _ = pr.batch_reference(np.concatenate(polys), offsets, np.concatenate(rows), H, W, 4, overlap=True)
        assert np.array_equal(b["masks"].cpu().numpy(), masks)
        assert np.array_equal(b["batch_idx"].cpu().numpy(), rows_sorted[:, 0]) and np.array_equal(b["cls"].cpu().numpy(), rows_sorted[:, 1:2])
        np.testing.assert_allclose(b["bboxes"].cpu().numpy(), rows_sorted[:, 2:6], rtol=0, atol=2e-7)      # one f32 ulp below 1
        seen += len(b["im_file"])
    assert seen == 3 and len({tuple(s) for s in loader.batch_shapes}) == 2


def test_val_loader_pose_keypoints_at_rect_shapes(tree):
    loader, files, labels = _fixture_val_loader(tree[0], "pose3")
    by_file = dict(zip(files, labels))
    seen = 0
    for bi, b in enumerate(loader):
        H, W = (int(v) for v in loader.batch_shapes[bi])
        want = []
        for j, f in enumerate(b["im_file"]):
            lab = by_file[f]
            e = _to_rect(lab["keypoints"], b["resized_shape"][j], (H, W))
            e[..., 0] /= W
            e[..., 1] /= H
            want.append(e)
        want = np.concatenate(want)
        assert b["keypoints"].dtype == torch.float32 and tuple(b["keypoints"].shape) == want.shape and want.shape[1:] == (5, 3)
        assert np.array_equal(b["keypoints"].numpy(), want)
        assert np.array_equal(b["keypoints"].numpy()[..., 2], np.concatenate([by_file[f]["keypoints"][..., 2] for f in b["im_file"]]))
        seen += len(b["im_file"])
    assert seen == 3


def test_train_val_predict_from_disk_end_to_end(tree):
    from dedark_yolo_amd.data import DeviceValLoader
    from dedark_yolo_amd.data.augment import letterbox_auto
    from dedark_yolo_amd.data.dataset import decode
    from dedark_yolo_amd.engine.model import YOLO
    root, yamls = tree
    torch.manual_seed(0)
    # yolov8nori.yaml: the plain YOLOv8 graph at scale n (the tiny model tests/test_gpu_tta.py uses).  yolov8n.yaml is this fork's ASFF
    # graph, whose ASFF level convolutions carry fixed widths: at scale n its training forward stops with "conv: weight expects 256 input
    # channels, got 64", with or without a dataset.
    m = YOLO("yolov8nori.yaml")
    kw = dict(imgsz=64, batch=4, dtype="fp32", lowlight_FLAG=False, dedark_FLAG=False, workers=2, conf=0.001)
    hist = m.train(data=yamls["det_trainval"], epochs=1, **kw)
    assert len(hist) == 1 and np.isfinite(hist[0]).all()
    assert m.model.yaml["nc"] == fx.NC and m.model.names == {0: "cat", 1: "dog", 2: "bird"}
    keys = {"metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)", "fitness"}
    assert keys <= set(m.trainer.metrics)
    got = m.val(data=yamls["det"], **kw)
    assert keys <= set(got)
    files, labels = _val_set(root)
    by_hand = list(DeviceValLoader(files, labels, 64, 4, stride=32, pad=0.5, rect=True))
    assert m.val(loader=by_hand, **kw) == got
    a, b = files[0], files[8]                                                       # 50 x 100 and 72 x 40
    res = m.predict([a, b], conf=0.001, imgsz=64)
    from oracle import augment as oa
    want_hw = {a: (32, 64), b: (64, 64)}
    for r, f in zip(res, (a, b)):
        src = decode(f)
        h, w = src.shape[:2]
        assert r.path == f and tuple(r.orig_shape) == (h, w)
        # the predictor's LetterBox(64, auto=True, stride=32) by hand, from the oracle's resize: scale the long side to 64 (scaleup,
        # linear), pad each axis to the next multiple of 32 only, centred, border 114, then Format's CHW RGB
        g = min(64 / h, 64 / w)
        nw, nh = int(round(w * g)), int(round(h * g))
        dw, dh = ((64 - nw) % 32) / 2, ((64 - nh) % 32) / 2
        top, bottom, left, right = int(round(dh - 0.1)), int(round(dh + 0.1)), int(round(dw - 0.1)), int(round(dw + 0.1))
        canvas = np.full((nh + top + bottom, nw + left + right, 3), 114, dtype=np.uint8)
        canvas[top:top + nh, left:left + nw] = oa.cv_resize_linear_u8(src, (nw, nh)) if (nw, nh) != (w, h) else src
        assert canvas.shape[:2] == want_hw[f]
        hand = torch.from_numpy(np.ascontiguousarray(oa.format_img(canvas))).cuda()
        assert torch.equal(letterbox_auto(torch.from_numpy(src).cuda(), 64, 32)[0], hand)
        want = m.predict(hand[None], conf=0.001, orig_shapes=[(h, w)])[0]
        assert len(want.boxes.data) > 0 and torch.equal(r.boxes.data, want.boxes.data)
    assert tuple(res[0].orig_shape) != tuple(res[1].orig_shape)
    with pytest.raises(ValueError, match="classes"):
        m.val(data=yamls["pose2"], **kw)                       # 1 class against the model's 3
