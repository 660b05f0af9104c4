"""CPU tests of MixUp and close_mosaic in the device loader: planner draw order, geometry, blend and merged labels against the
reference's own transform objects (tests/golden/g24_mixup.npz, g24_mixseg.npz, g24_mixpose.npz, made by
tests/golden/make_mixup_golden.py), the untouched mixup = 0 path, and the close_mosaic switch of the loader and the trainer."""
import copy
import os
import random

import numpy as np
import pytest

import mixup_ref as mr
import polymask_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = list(mr.MIX_CASES)


@pytest.fixture(scope="module")
def g24():
    z = {}
    for name in mr.FILES.values():
        z.update(np.load(os.path.join(ROOT, "tests", "golden", name)))
    return z


def hyp_of(v):
    from dedark_yolo_amd.data.augment import AugmentHyp
    return AugmentHyp(degrees=float(v[0]), translate=float(v[1]), scale=float(v[2]), shear=float(v[3]), perspective=float(v[4]), hsv_h=float(v[5]),
                      hsv_s=float(v[6]), hsv_v=float(v[7]), flipud=float(v[8]), fliplr=float(v[9]), mosaic=float(v[10]), mixup=float(v[11]))


def case_inputs(z, tag):
    kind, imgsz, _, _, picks, _, ratio, flip_idx = mr.MIX_CASES[tag]
    seed = int(z[f"{tag}_data_seed"])
    ims, labels = mr.mix_dataset(seed, tag)
    return kind, imgsz, seed, ims, labels, picks, hyp_of(z[f"{tag}_hyp"]), ratio, flip_idx


def case_plans(z, tag):
    """the planner seeded like the generator: (plans, per-sample labels, generator state after the last draw)"""
    from dedark_yolo_amd.data import augment as A
    kind, imgsz, seed, ims, labels, picks, hyp, ratio, flip_idx = case_inputs(z, tag)
    shapes = [im.shape[:2] for im in ims]
    ex = A.TaskLabels(labels, kind, hyp, flip_idx, ratio, True, imgsz)
    rnd, nprnd = random.Random(seed + 1), np.random.RandomState(seed + 2)
    plans = [A.plan_train_sample(i, shapes, list(range(len(ims))), imgsz, ex.hyp, rnd, nprnd) for i in picks]
    return plans, [ex.train_labels(p, shapes) for p in plans], np.array([rnd.random(), nprnd.uniform()])


@pytest.mark.parametrize("tag", TAGS)
def test_plan_follows_the_reference(g24, tag):
    """partner index, r, both matrices, both canvases, the HSV tables, the flips and both generators consumed exactly as far"""
    z = g24
    ims = case_inputs(z, tag)[3]
    plans, _, rng_after = case_plans(z, tag)
    for k, p in enumerate(plans):
        assert np.array_equal(p.M[:2], z[f"{tag}_n{k}_M"]) and np.array_equal(mr.canvas(p, ims), z[f"{tag}_n{k}_canvas"]), (tag, k)
        assert np.array_equal(np.stack(p.luts), z[f"{tag}_n{k}_lut"]) and [int(p.flipud), int(p.fliplr)] == list(z[f"{tag}_n{k}_flips"]), (tag, k)
        partner = int(z[f"{tag}_n{k}_partner"])
        if partner < 0:
            assert p.mix is None and p.mix_r is None, (tag, k)
            continue
        assert p.mix.index == partner and type(p.mix_r) is float and p.mix_r == float(z[f"{tag}_n{k}_r"]), (tag, k)
        assert np.array_equal(p.mix.M[:2], z[f"{tag}_n{k}_M2"]) and p.mix.M.dtype == np.float32, (tag, k)
        assert np.array_equal(mr.canvas(p.mix, ims), z[f"{tag}_n{k}_canvas2"]) and tuple(p.mix.size) == tuple(p.size), (tag, k)
    assert np.array_equal(rng_after, z[f"{tag}_rng_after"])


@pytest.mark.parametrize("tag", TAGS)
def test_merged_labels_follow_the_reference(g24, tag):
    """cls / bboxes bit for bit; segment: the polygons handed to fillPoly (primary then partner) and the masks / area order over the merged
    set through tests/polymask_ref.py; pose: the keypoints (flip_idx on all rows)"""
    z = g24
    kind, imgsz, ratio = mr.MIX_CASES[tag][0], mr.MIX_CASES[tag][1], mr.MIX_CASES[tag][6]
    _, labs, _ = case_plans(z, tag)
    for k, out in enumerate(labs):
        c, b = out[:2]
        assert c.dtype == b.dtype == np.float32 and c.shape == (len(b), 1)
        if kind == "segment":
            polys = out[2]
            assert polys.dtype == np.int32 and np.array_equal(polys, z[f"{tag}_n{k}_polys"]), (tag, k)
            masks, order, _ = pr.polygons2masks_overlap(polys, imgsz, imgsz, ratio)
            assert np.array_equal(masks[None] if masks.ndim == 2 else masks, z[f"{tag}_n{k}_masks"]), (tag, k)
            assert np.array_equal(order, z[f"{tag}_n{k}_sorted_idx"]), (tag, k)
            c, b = c[order], b[order]                     # the reference returns the rows in area order; the product permutes on the device
        elif kind == "pose":
            assert out[2].dtype == np.float32 and np.array_equal(out[2], z[f"{tag}_n{k}_keypoints"]), (tag, k)
        assert np.array_equal(c, z[f"{tag}_n{k}_cls"]) and np.array_equal(b, z[f"{tag}_n{k}_bboxes"]), (tag, k)
        if int(z[f"{tag}_n{k}_partner"]) >= 0:
            assert len(c) == int(z[f"{tag}_n{k}_counts"].sum())


@pytest.mark.parametrize("tag", TAGS)
def test_host_render_equals_the_reference_blend(g24, tag):
    """oracle warp + the float64 blend + flips + Format == the image the reference's own MixUp line produced on the same warps"""
    z = g24
    ims = case_inputs(z, tag)[3]
    plans, _, _ = case_plans(z, tag)
    for k, p in enumerate(plans):
        assert np.array_equal(mr.render(p, ims, hsv=False), z[f"{tag}_n{k}_img"]), (tag, k)


def test_fixture_covers_the_cases(g24):
    z = g24
    for tag in ("d1", "s1", "p1"):
        n = len(mr.MIX_CASES[tag][4])
        mixed = [k for k in range(n) if int(z[f"{tag}_n{k}_partner"]) >= 0]
        counts = [tuple(z[f"{tag}_n{k}_counts"]) for k in mixed]
        assert 0 < len(mixed) < n
        assert any(a == 0 and b > 0 for a, b in counts) and any(a > 0 and b == 0 for a, b in counts) and any(a > 0 and b > 0 for a, b in counts)
        s = mr.MIX_CASES[tag][1]
        assert {z[f"{tag}_n{k}_canvas2"].shape[0] for k in mixed} == {s, 2 * s}          # partners on the letterbox and the mosaic path
        assert {z[f"{tag}_n{k}_canvas"].shape[0] for k in range(n)} == {s, 2 * s}
        assert {tuple(z[f"{tag}_n{k}_flips"]) for k in range(n)} >= {(0, 0)} and sum(z[f"{tag}_n{k}_flips"] for k in range(n)).min() > 0
    assert any(tuple(z[f"d1_n{k}_counts"]) == (0, 0) for k in range(len(mr.MIX_CASES["d1"][4])) if int(z[f"d1_n{k}_partner"]) >= 0)
    assert mr.MIX_CASES["d0"][1] == 96 and all(int(z[f"d0_n{k}_partner"]) >= 0 for k in range(len(mr.MIX_CASES["d0"][4])))
    for tag in ("s0", "s1"):                              # distinct, non-zero areas: the reference's unstable order is unambiguous
        for k in range(len(mr.MIX_CASES[tag][4])):
            areas = [int(pr.polygon2mask(q, 64, 64, mr.MIX_CASES[tag][6]).sum()) for q in z[f"{tag}_n{k}_polys"]]
            assert len(set(areas)) == len(areas) and 0 not in areas


def test_blend_is_float64_with_two_roundings():
    """the stated blend against exact rational arithmetic where the two differ from float32 / fused evaluation: p = 255, q = 1 at
    r = 0.5 is the exact tie 128.0; truncation, not rounding"""
    from fractions import Fraction
    g = np.random.RandomState(3)
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    for r in [0.5, 0.25] + list(g.beta(32.0, 32.0, 4)):
        got = mr.blend(a, b, r)
        r1 = 1.0 - float(r)
        for i, j in ((255, 1), (0, 255), (255, 255), (127, 128), (254, 3)):
            exact = Fraction(int(a[i, j])) * Fraction(float(r)) + Fraction(int(b[i, j])) * Fraction(r1)
            assert abs(int(got[i, j]) - int(exact)) <= 1          # float64 rounding of the sum can cross an integer only by an ulp
        assert got.dtype == np.uint8 and np.array_equal(got, (a * r + b * (1 - r)).astype(np.uint8))
    assert int(mr.blend(np.uint8([255]), np.uint8([255]), 0.3)[0]) in (254, 255)


# ------------------------------------------------------------------------------------------------ mixup = 0 changes nothing
def test_mixup_zero_plans_and_labels_are_the_old_ones():
    from dedark_yolo_amd.data import augment as A
    ims, labels = mr.mix_dataset(7, "s1")
    shapes = [im.shape[:2] for im in ims]
    base = dict(mosaic=0.5, flipud=0.5, degrees=5.0)
    with_key, without = A.AugmentHyp(mixup=0.0, **base), A.AugmentHyp(**base)          # given as 0 / not given (the default)
    outs = []
    for hyp in (with_key, without):
        ex = A.TaskLabels(labels, "segment", hyp, None, 4, True, 64)
        rnd, nprnd = random.Random(1), np.random.RandomState(2)
        plans = [A.plan_train_sample(i, shapes, list(range(len(ims))), 64, ex.hyp, rnd, nprnd) for i in range(len(ims))]
        assert all(p.mix is None and p.mix_r is None for p in plans)
        outs.append((plans, [ex.train_labels(p, shapes) for p in plans], rnd.random(), nprnd.uniform()))
    (pa, la, ra, na), (pb, lb, rb, nb) = outs
    assert ra == rb and na == nb
    for p, q, x, y in zip(pa, pb, la, lb):
        assert p.sources == q.sources and p.rects == q.rects and np.array_equal(p.M, q.M) and (p.flipud, p.fliplr) == (q.flipud, q.fliplr)
        assert all(np.array_equal(u, v) for u, v in zip(x, y))
    # the draws of an un-mixed sample are the pre-feature ones: mosaic coin, 3 partners, 2 centre, 8 affine, MixUp's coin, 2 flips
    rnd, ref = random.Random(5), random.Random(5)
    A.plan_train_sample(0, shapes, list(range(len(ims))), 64, A.AugmentHyp(hsv_h=0, hsv_s=0, hsv_v=0), rnd, np.random.RandomState(0))
    ref.uniform(0, 1)
    ref.choices(list(range(len(ims))), k=3)
    for _ in range(2 + 8 + 1 + 2):
        ref.random()
    assert rnd.random() == ref.random()


def test_descriptor_bytes_and_fill_without_mixup_are_unchanged():
    """descriptor_bytes() keeps its size; fill_descriptors over plain plans writes the same dy_aug_sample bytes into the plain array and
    into the `a` half of the mix array; a plan with a partner needs the mix array"""
    import ctypes as C

    from dedark_yolo_amd import _C
    from dedark_yolo_amd.data import augment as A
    assert A.descriptor_bytes() == C.sizeof(_C.AugSample) == 1032 and A.descriptor_bytes(mix=True) == C.sizeof(_C.AugMixSample) == 2088
    assert _C.AugMixSample.b.offset == 1032 and _C.AugMixSample.r.offset == 2064 and _C.AugMixSample.mix.offset == 2080

    class FakeImage:                                      # what fill_descriptors reads of a device tensor
        def __init__(self, im, k):
            self.shape, self.k = im.shape, k

        def data_ptr(self):
            return 4096 * (self.k + 1)

        def stride(self, d):
            return self.shape[1] * 3
    ims, _ = mr.mix_dataset(9, "d1")
    shapes = [im.shape[:2] for im in ims]
    fake = [FakeImage(im, k) for k, im in enumerate(ims)]
    rnd, nprnd = random.Random(1), np.random.RandomState(2)
    plans = [A.plan_train_sample(i, shapes, list(range(len(ims))), 64, A.AugmentHyp(mixup=0.5, mosaic=0.5), rnd, nprnd) for i in range(8)]
    plain = [p for p in plans if p.mix is None]
    assert 0 < len(plain) < len(plans)
    one, two = np.zeros(len(plain) * 1032, np.uint8), np.zeros(len(plans) * 2088, np.uint8)
    A.fill_descriptors(plain, fake, one.ctypes.data)
    A.fill_descriptors(plans, fake, two.ctypes.data, mix=True)
    two = two.reshape(len(plans), 2088)
    j = 0
    for k, p in enumerate(plans):
        d = _C.AugMixSample.from_buffer_copy(two[k].tobytes())
        assert d.mix == int(p.mix is not None)
        if p.mix is None:
            assert np.array_equal(two[k, :1032], one[j * 1032:(j + 1) * 1032]) and not two[k, 1032:].any()
            j += 1
        else:
            assert d.r == p.mix_r and d.r1 == 1.0 - p.mix_r and d.b.n_src == len(p.mix.sources) and d.b.canvas_h == p.mix.canvas_hw[0]
            assert list(d.b.minv) == [float(v) for v in A.invert_affine(p.mix.M[:2]).reshape(-1)]
    with pytest.raises(ValueError, match="mix"):
        A.fill_descriptors(plans, fake, np.zeros(len(plans) * 1032, np.uint8).ctypes.data)


def test_copy_paste_and_perspective_still_raise():
    from dedark_yolo_amd.data import augment as A
    for kw in (dict(copy_paste=0.1), dict(perspective=0.001)):
        with pytest.raises(NotImplementedError):
            A.plan_train_sample(0, [(64, 64)], [0], 64, A.AugmentHyp(**kw), random.Random(1), np.random.RandomState(1))
    A.plan_train_sample(0, [(64, 64)], [0], 64, A.AugmentHyp(mixup=0.3), random.Random(1), np.random.RandomState(1))


def test_more_than_255_merged_instances_raise():
    """150 instances per image pass alone; primary + partner = 300 do not fit the uint8 overlap map"""
    from dedark_yolo_amd.data import augment as A
    sq = np.array([[0.3, 0.3], [0.7, 0.3], [0.7, 0.7], [0.3, 0.7]], np.float32)
    many = [dict(cls=np.zeros((150, 1), np.float32), bboxes=np.tile(np.array([[0.5, 0.5, 0.4, 0.4]], np.float32), (150, 1)), segments=[sq] * 150)]
    shapes = [(64, 64)]
    for mixup, ok in ((0.0, True), (1.0, False)):
        ex = A.TaskLabels(many, "segment", A.AugmentHyp(mosaic=0.0, scale=0.0, translate=0.0, mixup=mixup), None, 4, True, 64)
        p = A.plan_train_sample(0, shapes, [0], 64, ex.hyp, random.Random(1), np.random.RandomState(1))
        if ok:
            assert len(ex.train_labels(p, shapes)[0]) == 150
        else:
            assert p.mix is not None
            with pytest.raises(NotImplementedError, match="255"):
                ex.train_labels(p, shapes)


# ------------------------------------------------------------------------------------------------ close_mosaic
class _Loader:
    """DeviceAugmentLoader without its device side: the hyper-parameter handling and the planner"""

    def __new__(cls, ims, labels, hyp):
        from dedark_yolo_amd.data.augment import TaskLabels
        from dedark_yolo_amd.data.loader import DeviceAugmentLoader
        ld = DeviceAugmentLoader.__new__(DeviceAugmentLoader)
        ld.imgsz, ld.bs, ld.hyp, ld.labels, ld.task = 64, 4, hyp, labels, "detect"
        ld.extras = TaskLabels(labels, "detect", hyp, None, 4, True, 64)
        ld.shapes = [im.shape[:2] for im in ims]
        ld.rnd, ld.nprnd, ld.aug, ld._close = random.Random(3), np.random.RandomState(4), None, False
        ld.shuffle, ld.drop_last = False, True
        ld._prepare = lambda idx: (dict(plans=ld._plans(idx)), None, ())          # no device: a batch is its plans
        return ld


def test_close_mosaic_switches_the_next_epoch(monkeypatch):
    import torch

    from dedark_yolo_amd.data.augment import AugmentHyp
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: type("S", (), dict(wait_event=lambda self, ev: None))())
    ims, labels = mr.mix_dataset(3, "d1")
    hyp = AugmentHyp(mixup=1.0)
    before = copy.copy(hyp)
    ld = _Loader(ims, labels, hyp)
    first = [p for b in ld for p in b["plans"]]
    assert len(first) == 8 and all(p.mosaic and p.mix is not None for p in first)
    it = iter(ld)
    next(it)
    ld.close_mosaic()                                     # in the middle of an epoch: this epoch keeps its hyper-parameters
    assert all(p.mosaic and p.mix is not None for b in it for p in b["plans"])
    closed = [p for b in ld for p in b["plans"]]
    assert len(closed) == 8 and not any(p.mosaic or p.mix is not None for p in closed)
    assert (ld.hyp.mosaic, ld.hyp.mixup, ld.hyp.copy_paste) == (0.0, 0.0, 0.0) and ld.hyp.fliplr == hyp.fliplr
    assert hyp == before and hyp.mixup == 1.0 and ld.hyp is not hyp          # the caller's object is left alone


@pytest.mark.parametrize("epochs,close,start,want", [(5, 2, 0, [3]), (5, 0, 0, []), (5, 2, 3, [3]), (5, 2, 4, [4]), (5, 2, 2, [3]), (3, 5, 0, [0])])
def test_trainer_calls_close_mosaic_at_the_right_epoch(epochs, close, start, want):
    """train()'s epoch loop with a stub loader and a stub step: the call lands at the top of epoch `epochs - close_mosaic`, or of the
    first epoch of a run resumed beyond it; never with the default 0"""
    import torch

    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    assert get_cfg().close_mosaic == 0

    class Stub:
        def __init__(self):
            self.epoch, self.calls = -1, []

        def __len__(self):
            return 2

        def __iter__(self):
            self.epoch += 1
            return iter([dict(k=0), dict(k=1)])

        def close_mosaic(self):
            self.calls.append(self.epoch + 1)             # the epoch whose batches come next

    tr = DetectionTrainer.__new__(DetectionTrainer)
    tr.args = get_cfg(dict(epochs=epochs, close_mosaic=close, warmup_epochs=0, val=False, save=False))
    tr.rank, tr.world_size, tr.last_opt_step, tr.accumulate = -1, 1, -1, 1
    tr._batches = lambda loader: loader
    tr.lr_factors = lambda ni, nw, epoch, epochs: ([0.01] * 3, 0.9)
    tr.train_step = lambda batch, lr, mom, step_optimizer=True: (0.0, torch.zeros(3))
    ld = Stub()
    ld.epoch = start - 1
    hist = tr.train(ld, start_epoch=start)
    assert len(hist) == epochs - start and ld.calls == want
    plain = type("NoSwitch", (), dict(__len__=lambda s: 1, __iter__=lambda s: iter([dict()])))()
    tr.train(plain)                                       # a loader without the method is left alone
