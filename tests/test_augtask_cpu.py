"""CPU tests of the segment / pose side of the device loader: the host bookkeeping of dedark_yolo_amd/data/augment.py against the
reference's own transforms (tests/golden/g20_augseg.npz, g20_augpose.npz, made by tests/golden/make_augtask_golden.py), the flip_idx
rule of v8_transforms, val_labels with polygons / keypoints, the untouched detect path (g13) and the properties of the numpy statement
of the polygon-mask rule (tests/polymask_ref.py) the kernel is held to on the GPU."""
import os
import random
import warnings

import numpy as np
import pytest

import polymask_ref as pr
from augtask_data import CASES, COCO_FLIP_IDX, IMGSZ, synth_task_dataset
from test_augment_cpu import _hyp, synth_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g20():
    z = {}
    for name in ("g20_augseg.npz", "g20_augpose.npz"):
        z.update(np.load(os.path.join(ROOT, "tests", "golden", name)))
    return z


def case_inputs(z, tag):
    kind, dkw, n_img, picks, _, ratio, overlap, flip_idx = CASES[tag]
    seed = int(z[f"{tag}_data_seed"])
    ims, labels = synth_task_dataset(seed, n_img, IMGSZ, kind, **dkw)
    return kind, seed, ims, labels, picks, _hyp(z[f"{tag}_hyp"]), ratio, overlap, flip_idx


@pytest.mark.parametrize("tag", list(CASES))
def test_bookkeeping_follows_the_reference(g20, tag):
    """integer polygons equal, labels and keypoints equal bit for bit, the affine matrix and flips of every sample, and both generators
    consumed exactly as far as the reference consumed them"""
    from dedark_yolo_amd.data import augment as A
    z = g20
    kind, seed, ims, labels, picks, hyp, ratio, overlap, flip_idx = case_inputs(z, tag)
    shapes = [im.shape[:2] for im in ims]
    ex = A.TaskLabels(labels, kind, hyp, flip_idx, ratio, overlap, IMGSZ)
    random.seed(seed + 1)
    np.random.seed(seed + 2)
    for k, idx in enumerate(picks):
        p = A.plan_train_sample(idx, shapes, list(range(len(ims))), IMGSZ, ex.hyp)
        assert np.array_equal(p.M[:2], z[f"{tag}_n{k}_M"]), (tag, k)
        assert [int(p.flipud), int(p.fliplr)] == list(z[f"{tag}_n{k}_flips"]) or len(z[f"{tag}_n{k}_cls"]) == 0
        c, b, e = ex.train_labels(p, shapes)
        assert c.dtype == b.dtype == np.float32 and c.shape == (len(b), 1)
        if kind == "segment":
            assert e.dtype == np.int32 and np.array_equal(e, z[f"{tag}_n{k}_polys"]), (tag, k)
            if overlap:                                   # the reference returns the rows in area order; the product permutes on the device
                order = z[f"{tag}_n{k}_sorted_idx"]
                c, b = c[order], b[order]
        else:
            assert e.dtype == np.float32 and np.array_equal(e, z[f"{tag}_n{k}_keypoints"]), (tag, k)
        assert np.array_equal(c, z[f"{tag}_n{k}_cls"]) and np.array_equal(b, z[f"{tag}_n{k}_bboxes"]), (tag, k)
    assert np.array_equal(np.array([random.random(), np.random.uniform()]), z[f"{tag}_rng_after"])


def test_fixture_covers_the_cases(g20):
    z = g20
    assert list(z["s0_flips_seen"]) == [1, 1] and list(z["p0_flips_seen"]) == [1, 1]                  # both flips, mosaic samples
    assert float(z["s1_hyp"][10]) == 0.0 and float(z["p1_hyp"][10]) == 0.0                            # the mosaic coin fails
    assert any(len(z[f"s1_n{k}_cls"]) == 0 for k in range(5)) and any(len(z[f"p1_n{k}_cls"]) == 0 for k in range(4))
    assert z["s2_n0_masks"].shape[0] == len(z["s2_n0_cls"]) and z["s0_n0_masks"].shape[0] == 1         # overlap_mask False / True
    for tag in ("s0", "s1", "s2"):                        # distinct, non-zero areas: the reference's unstable order is unambiguous
        ratio = CASES[tag][5]
        for k in range(len(CASES[tag][3])):
            polys = z[f"{tag}_n{k}_polys"]
            areas = [int(pr.polygon2mask(q, IMGSZ, IMGSZ, ratio).sum()) for q in polys]
            assert len(set(areas)) == len(areas) and 0 not in areas


def test_reresampling_is_np_interp():
    """_reresample (all polygons at once) == resample_segments (np.interp per coordinate) on already resampled polygons"""
    from dedark_yolo_amd.data import augment as A
    g = np.random.default_rng(3)
    seg = A.resample_segments([g.uniform(0, 1, (int(g.integers(3, 13)), 2)).astype(np.float32) for _ in range(7)])
    assert seg.shape == (7, 1000, 2) and seg.dtype == np.float32
    seg *= np.float32(613.7)
    assert np.array_equal(A._reresample(seg), A.resample_segments(list(seg)))
    assert A._reresample(seg[:0]).shape == (0, 1000, 2)


def test_flip_idx_rules():
    from dedark_yolo_amd.data import augment as A
    _, labels = synth_task_dataset(1, 3, IMGSZ, "pose")
    hyp = A.AugmentHyp(fliplr=0.5)
    with pytest.warns(UserWarning, match="fliplr"):
        ex = A.TaskLabels(labels, "pose", hyp, None, 4, True, IMGSZ)
    assert ex.hyp.fliplr == 0.0 and hyp.fliplr == 0.5 and ex.flip_idx is None          # the caller's hyp object is not modified
    with pytest.raises(ValueError, match="flip_idx"):
        A.TaskLabels(labels, "pose", hyp, [1, 0, 2], 4, True, IMGSZ)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ex = A.TaskLabels(labels, "pose", hyp, COCO_FLIP_IDX, 4, True, IMGSZ)
        assert ex.hyp.fliplr == 0.5 and ex.flip_idx == COCO_FLIP_IDX
        assert A.TaskLabels(labels, "pose", A.AugmentHyp(fliplr=0.0), None, 4, True, IMGSZ).hyp.fliplr == 0.0
        A.TaskLabels(labels, "detect", hyp, None, 4, True, IMGSZ)                      # not a pose set: no rule, no warning


def test_label_dict_rules():
    from dedark_yolo_amd.data import augment as A
    _, seg = synth_task_dataset(2, 2, IMGSZ, "segment")
    _, pose = synth_task_dataset(2, 2, IMGSZ, "pose")
    both = [dict(s, keypoints=p["keypoints"]) for s, p in zip(seg, pose)]
    with pytest.raises(ValueError, match="both segments and keypoints"):
        A.TaskLabels(both, "segment", A.AugmentHyp(), None, 4, True, IMGSZ)
    for bad in (3, 0, -2):
        with pytest.raises(ValueError, match="mask_ratio"):
            A.TaskLabels(seg, "segment", A.AugmentHyp(), None, bad, True, IMGSZ)
    with pytest.raises(ValueError, match="segments"):
        A.TaskLabels(pose, "segment", A.AugmentHyp(), None, 4, True, IMGSZ)
    with pytest.raises(ValueError, match="task"):
        A.TaskLabels(seg, "classify", A.AugmentHyp(), None, 4, True, IMGSZ)
    # ndim 2 keypoints get the label reader's visibility column
    kp = A.keypoints_with_visibility(np.array([[[0.5, 0.5], [-1.0, 0.2], [0.1, -0.3]]], np.float32))
    assert kp.shape == (1, 3, 3) and list(kp[0, :, 2]) == [1.0, 0.0, 0.0]
    # more than 255 instances in one image: the uint8 overlap map cannot hold them
    many = [dict(cls=np.zeros((300, 1), np.float32), bboxes=np.tile(np.array([[0.5, 0.5, 0.4, 0.4]], np.float32), (300, 1)),
                 segments=[np.array([[0.3, 0.3], [0.7, 0.3], [0.7, 0.7], [0.3, 0.7]], np.float32)] * 300)]
    ex = A.TaskLabels(many, "segment", A.AugmentHyp(mosaic=0.0, scale=0.0, translate=0.0), None, 4, True, IMGSZ)
    p = A.plan_train_sample(0, [(IMGSZ, IMGSZ)], [0], IMGSZ, ex.hyp, random.Random(1), np.random.RandomState(1))
    with pytest.raises(NotImplementedError, match="255"):
        ex.train_labels(p, [(IMGSZ, IMGSZ)])


def test_val_labels_with_segments_and_keypoints():
    from dedark_yolo_amd.data import augment as A
    g13 = np.load(os.path.join(ROOT, "tests", "golden", "g13_augment.npz"))
    _, seg = synth_task_dataset(5, 1, IMGSZ, "segment")
    _, pose = synth_task_dataset(5, 1, IMGSZ, "pose")
    for k, (h, w) in enumerate(g13["val_shapes"]):
        shape, bb = (int(h), int(w)), g13[f"val_v{k}_in_bboxes"]
        plain = A.val_labels(bb, shape, IMGSZ)
        assert len(plain) == 3 and np.array_equal(plain[0], g13[f"val_v{k}_bboxes"])               # unchanged without the new arguments
        geo = plain[2]
        b, rp, _, polys = A.val_labels(seg[0]["bboxes"], shape, IMGSZ, segments=seg[0]["segments"])
        assert np.array_equal(b, A.val_labels(seg[0]["bboxes"], shape, IMGSZ)[0]) and rp == plain[1]
        rs = A.resample_segments(seg[0]["segments"])
        want = rs.copy()                                  # Instances.denormalize(w, h), scale(r, r), add_padding(dw, dh); astype(int32)
        want[..., 0] *= w
        want[..., 1] *= h
        want[..., 0] *= geo.r
        want[..., 1] *= geo.r
        want[..., 0] += geo.dw
        want[..., 1] += geo.dh
        assert polys.dtype == np.int32 and polys.shape == rs.shape and np.array_equal(polys, want.astype(np.int32))
        assert polys.min() >= 0 and polys.max() <= IMGSZ
        assert np.array_equal(A.val_labels(seg[0]["bboxes"], shape, IMGSZ, segments=rs)[3], polys)   # already resampled input
        # the polygons' extent is the box the label carries (built from the same raw polygon): within 2 px = the truncation (< 1) plus
        # the vertex a resampled polygon can miss by one parameter step (< 64 px * 12 edges / 999 < 0.8 px)
        px = b.copy() * IMGSZ
        assert np.all(np.abs(polys[..., 0].min(1) - (px[:, 0] - px[:, 2] / 2)) <= 2) and np.all(np.abs(polys[..., 1].max(1) - (px[:, 1] + px[:, 3] / 2)) <= 2)
        kp = A.val_labels(pose[0]["bboxes"], shape, IMGSZ, keypoints=pose[0]["keypoints"])[3]
        src = pose[0]["keypoints"]
        assert kp.dtype == np.float32 and kp.shape == src.shape and np.array_equal(kp[..., 2], src[..., 2])
        np.testing.assert_allclose(kp[..., 0], (src[..., 0] * w * geo.r + geo.dw) / IMGSZ, rtol=0, atol=1e-6)
        np.testing.assert_allclose(kp[..., 1], (src[..., 1] * h * geo.r + geo.dh) / IMGSZ, rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        A.val_labels(bb, shape, IMGSZ, segments=seg[0]["segments"], keypoints=pose[0]["keypoints"])


@pytest.mark.parametrize("tag", ["t0", "t1", "t2"])
def test_detect_path_returns_what_it_did(tag):
    """train_labels without the new arguments on the g13 inputs: the reference's detect labels, and a two-value result"""
    from dedark_yolo_amd.data import augment as A
    z = np.load(os.path.join(ROOT, "tests", "golden", "g13_augment.npz"))
    imgsz, seed, picks = int(z[f"{tag}_imgsz"]), int(z[f"{tag}_data_seed"]), [int(i) for i in z[f"{tag}_picks"]]
    ims, labels = synth_dataset(seed, int(z[f"{tag}_n_img"]), imgsz)
    shapes = [im.shape[:2] for im in ims]
    random.seed(seed + 1)
    np.random.seed(seed + 2)
    ex = A.TaskLabels(labels, "detect", _hyp(z[f"{tag}_hyp"]), None, 4, True, imgsz)
    for k, idx in enumerate(picks):
        p = A.plan_train_sample(idx, shapes, list(range(len(ims))), imgsz, _hyp(z[f"{tag}_hyp"]))
        out = A.train_labels(p, labels, shapes)
        assert len(out) == 2 and np.array_equal(out[0], z[f"{tag}_s{k}_cls"]) and np.array_equal(out[1], z[f"{tag}_s{k}_bboxes"])
        via = ex.train_labels(p, shapes)
        assert len(via) == 2 and np.array_equal(via[0], out[0]) and np.array_equal(via[1], out[1])


# ------------------------------------------------------------------------------------------------ the numpy statement of the pixel rule
def test_ref_rectangle_is_the_closed_rectangle():
    m = pr.fill_closed([[3, 2], [10, 2], [10, 7], [3, 7]], 16, 16)
    want = np.zeros((16, 16), np.uint8)
    want[2:8, 3:11] = 1
    assert np.array_equal(m, want)
    assert np.array_equal(pr.fill_closed([[5, 5]] * 4, 16, 16), np.eye(1, 256, 5 * 16 + 5, dtype=np.uint8).reshape(16, 16))   # one pixel
    seg = pr.fill_closed([[2, 3], [9, 3]], 16, 16)                                    # a degenerate polygon is its boundary
    assert seg.sum() == 8 and seg[3, 2:10].all()


def test_ref_orientation_and_rotation_of_the_vertex_list_do_not_matter():
    g = np.random.default_rng(11)
    for _ in range(6):
        p = g.integers(0, 33, (int(g.integers(3, 9)), 2))                             # self-intersecting ones included
        a = pr.fill_closed(p, 32, 32)
        assert np.array_equal(a, pr.fill_closed(p[::-1], 32, 32)) and np.array_equal(a, pr.fill_closed(np.roll(p, 2, 0), 32, 32))
        assert np.array_equal(a, pr.fill_closed(np.repeat(p, 2, 0), 32, 32))          # repeated consecutive vertices


def test_ref_vertices_on_the_far_border_stay_in_bounds():
    s = 32
    m = pr.fill_closed([[s, 0], [s, s], [s, 10]], s, s)                               # collapsed onto x == s: outside the plane
    assert m.shape == (s, s) and m.sum() == 0
    m = pr.fill_closed([[0, 0], [s, 0], [s, s], [0, s]], s, s)
    assert m.shape == (s, s) and m.all()
    for r in (1, 2, 4):
        assert pr.polygon2mask([[0, 0], [s, 0], [s, s], [0, s]], s, s, r).shape == (s // r, s // r)


@pytest.mark.parametrize("r", [2, 4, 6, 8])
def test_ref_resize_is_two_of_four_taps(r):
    """cv2.resize(INTER_LINEAR) of a 0/1 plane by an even ratio == at least 2 of the 4 taps at rows / columns r i + r / 2 - 1, + 1: the
    form the kernel evaluates"""
    from oracle.augment import cv_resize_linear_u8
    g = np.random.default_rng(r)
    s = 8 * r
    plane = (g.uniform(0, 1, (s, s)) < 0.5).astype(np.uint8)
    t = np.arange(s // r) * r + r // 2 - 1
    taps = plane[t][:, t].astype(int) + plane[t][:, t + 1] + plane[t + 1][:, t] + plane[t + 1][:, t + 1]
    assert np.array_equal(cv_resize_linear_u8(plane[..., None], (s // r, s // r))[..., 0], (taps >= 2).astype(np.uint8))


def test_ref_overlap_order_and_composition():
    s = 32
    big, small = [[2, 2], [28, 2], [28, 28], [2, 28]], [[10, 10], [16, 10], [16, 16], [10, 16]]
    twin = [[20, 20], [26, 20], [26, 26], [20, 26]]                                   # same area as `small`
    m, idx, areas = pr.polygons2masks_overlap(np.array([small, big, twin]), s, s, 1)
    assert list(idx) == [1, 0, 2] and areas[0] == areas[2] == 49                      # ties by original index
    assert m[5, 5] == 1 and m[12, 12] == 2 and m[22, 22] == 3 and m[0, 0] == 0        # nested: the smaller one wins
    with pytest.raises(NotImplementedError):
        pr.polygons2masks_overlap(np.zeros((256, 3, 2), int), s, s, 1)
