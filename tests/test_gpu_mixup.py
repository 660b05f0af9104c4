"""GPU tests of MixUp in the device input pipeline: dy_aug_mosaic_warp_mix byte for byte against the host statement of the chain
(tests/mixup_ref.py: oracle/augment.py's pieces plus the float64 blend, itself pinned to the reference's own MixUp line by
tests/test_mixup_cpu.py), un-mixed batches against dy_aug_mosaic_warp, the blend's rounding traps, loader batches of all three tasks
against the host bookkeeping, a training step per task, and close_mosaic."""
import random

import numpy as np
import pytest
import torch

import mixup_ref as mr
import polymask_ref as pr
from test_mixup_cpu import case_inputs, g24  # noqa: F401  (g24: the module-scoped fixture)

pytestmark = pytest.mark.gpu


def _plans(aug, indices, seed):
    rnd, nprnd = random.Random(seed), np.random.RandomState(seed + 1)
    return [aug.plan(i, rnd, nprnd) for i in indices]


@pytest.mark.parametrize("tag,hsv", [("d0", True), ("d1", True), ("d1", False), ("d0", False)])
def test_mix_kernel_vs_host_render(g24, tag, hsv):
    """batches of 6 plans from the golden's dataset and seeds at 96 x 96 (d0: every sample mixed; one and a half blocks wide) and
    64 x 64 (d1: mixed and un-mixed samples, letterbox-path primaries and partners in one launch), both flips, HSV on and off"""
    from dedark_yolo_amd.data import DeviceAugmenter
    _, imgsz, seed, ims, labels, picks, hyp, _, _ = case_inputs(g24, tag)
    if not hsv:
        hyp.hsv_h = hyp.hsv_s = hyp.hsv_v = 0.0
    aug = DeviceAugmenter(ims, labels, imgsz, hyp)
    plans = _plans(aug, (picks * 3)[:6], seed + 1)
    mixed = [p.mix is not None for p in plans]
    assert any(mixed) and (tag == "d0" or not all(mixed)) and any(p.flipud for p in plans) and any(p.fliplr for p in plans)
    assert tag == "d0" or (any(p.mix is not None and not p.mix.mosaic for p in plans) and any(not p.mosaic for p in plans))
    assert all((p.hsv_gains is not None) == hsv for p in plans)
    got = aug.render(plans)
    again = aug.render(plans)
    assert got.shape == (6, 3, imgsz, imgsz) and got.dtype == torch.uint8 and torch.equal(got, again)      # two renders: identical
    got = got.cpu().numpy()
    for k, p in enumerate(plans):
        want = mr.render(p, ims)
        assert np.array_equal(got[k], want), f"{tag} sample {k} (mixed {mixed[k]}): {int((got[k] != want).sum())} of {want.size} bytes differ"


@pytest.mark.parametrize("imgsz", [64, 96])
def test_unmixed_batch_equals_the_plain_entry_point(imgsz):
    """the same un-mixed plans through dy_aug_mosaic_warp (mixup = 0) and through dy_aug_mosaic_warp_mix (mixup > 0, no coin taken)"""
    from dedark_yolo_amd.data import AugmentHyp, DeviceAugmenter
    from test_augment_cpu import synth_dataset
    ims, labels = synth_dataset(31, 6, imgsz)
    kw = dict(mosaic=0.5, flipud=0.5, degrees=10.0)
    plain, mix = DeviceAugmenter(ims, labels, imgsz, AugmentHyp(**kw)), DeviceAugmenter(ims, labels, imgsz, AugmentHyp(mixup=1e-9, **kw))
    plans = _plans(plain, [0, 1, 2, 3, 4, 5], 8)
    assert [(p.mosaic, p.flipud, p.fliplr) for p in _plans(mix, [0, 1, 2, 3, 4, 5], 8)] == [(p.mosaic, p.flipud, p.fliplr) for p in plans]
    assert all(p.mix is None for p in plans) and any(p.mosaic for p in plans) and not all(p.mosaic for p in plans)
    a, b = plain.render(plans), mix.render(plans)
    assert torch.equal(a, b)
    assert np.array_equal(a[0].cpu().numpy(), mr.render(plans[0], ims))


def test_blend_rounding_traps():
    """constant images 0, 1, 127, 128, 254, 255 -- identity warps, so primary and partner pixels are those values: equal or
    complementary pairs -- at 20 ratios including 0.5 and draws of numpy.random.beta(32, 32): where float32 arithmetic or a fused
    multiply-add would show"""
    from dedark_yolo_amd.data import AugmentHyp, DeviceAugmenter
    vals = [0, 1, 127, 128, 254, 255]
    s = 64
    ims = [np.full((s, s, 3), v, np.uint8) for v in vals]
    labels = [dict(cls=np.zeros((0, 1), np.float32), bboxes=np.zeros((0, 4), np.float32)) for _ in vals]
    hyp = AugmentHyp(mosaic=0.0, mixup=1.0, scale=0.0, translate=0.0, hsv_h=0.0, hsv_s=0.0, hsv_v=0.0, fliplr=0.0)
    aug = DeviceAugmenter(ims, labels, s, hyp)
    ratios = [0.5, 0.25, 0.75, 1.0 / 3.0, 0.1, 0.9, 0.4999999999999999, 0.5000000000000001] + [float(v) for v in np.random.RandomState(32).beta(32.0, 32.0, 12)]
    rnd, nprnd = random.Random(2), np.random.RandomState(3)
    plans, pairs = [], set()
    for r in ratios:
        for i in range(len(vals)):
            p = aug.plan(i, rnd, nprnd)
            p.mix_r = r
            plans.append(p)
            pairs.add((vals[i], vals[p.mix.index]))
    assert {(0, 255), (255, 0)} & pairs and {(127, 128), (128, 127)} & pairs and any(a == b for a, b in pairs)
    got = aug.render(plans).cpu().numpy()
    for k, p in enumerate(plans):
        want = mr.render(p, ims)
        assert len(np.unique(want)) == 1 and np.array_equal(got[k], want), (p.index, p.mix.index, p.mix_r, int(got[k][0, 0, 0]), int(want[0, 0, 0]))


def _host_batch(ims, labels, imgsz, kind, hyp, flip_idx, ratio, picks, seed):
    """what the loader must yield for `picks`: the planner seeded like the loader's generators + the host bookkeeping"""
    from dedark_yolo_amd.data import augment as A
    shapes = [im.shape[:2] for im in ims]
    ex = A.TaskLabels(labels, kind, hyp, flip_idx, ratio, True, imgsz)
    rnd, nprnd = random.Random(seed), np.random.RandomState(seed + 1)
    plans = [A.plan_train_sample(i, shapes, list(range(len(ims))), imgsz, ex.hyp, rnd, nprnd) for i in picks]
    return plans, [ex.train_labels(p, shapes) for p in plans]


@pytest.mark.parametrize("tag", ["d1", "s1", "p1"])
def test_loader_with_mixup_matches_the_host_and_trains(g24, tag):
    """DeviceAugmentLoader(hyp=AugmentHyp(mixup=1.0)) at imgsz 64, batch 4: pixels == host render, label rows (segment: in the area order
    of the merged set, masks == polymask_ref; pose: keypoints) == host bookkeeping, resident and host-memory modes agree bit for bit,
    and one train_step of the task's n-scale model on such a batch gives a finite loss"""
    import dedark_yolo_amd as dy
    from dedark_yolo_amd.data import AugmentHyp, DeviceAugmentLoader
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    from dedark_yolo_amd.nn.tasks import DetectionModel, PoseModel, SegmentationModel
    from util import load_yaml
    kind, imgsz, seed, ims, labels, _, _, _, flip_idx = case_inputs(g24, tag)
    hyp, picks, ratio = AugmentHyp(mixup=1.0, flipud=0.5), [0, 1, 2, 3], 4
    mk = lambda resident: DeviceAugmentLoader(ims, labels, imgsz, 4, hyp=hyp, seed=11, task=kind, flip_idx=flip_idx, mask_ratio=ratio, resident=resident)
    ld, lh = mk(True), mk(False)
    (batch, ev, _), (bh, evh, _) = ld._prepare(picks), lh._prepare(picks)
    ev.synchronize()
    evh.synchronize()
    plans, lab = _host_batch(ims, labels, imgsz, kind, hyp, flip_idx, ratio, picks, 11)
    assert all(p.mix is not None for p in plans) and lh.uploaded_bytes > 0
    for key in batch:
        if torch.is_tensor(batch[key]):
            assert torch.equal(batch[key], bh[key]), key
    img = batch["img"].cpu().numpy()
    for k, p in enumerate(plans):
        assert np.array_equal(img[k], mr.render(p, ims)), k
    rows = [np.concatenate((np.full((len(l[0]), 1), k, np.float32), l[0], l[1]), 1) for k, l in enumerate(lab)]
    if kind == "segment":
        want_masks, order = [], []
        for l in lab:
            m, idx, _ = pr.polygons2masks_overlap(l[2], imgsz, imgsz, ratio)
            want_masks.append(m)
            order.append(np.asarray(idx, np.int64))
        rows = [r[o] for r, o in zip(rows, order)]
        assert np.array_equal(batch["masks"].cpu().numpy(), np.stack(want_masks))
        assert np.array_equal(batch["sorted_idx"].cpu().numpy(), np.concatenate(order).astype(np.int32))
    rows = np.concatenate(rows, 0)
    got = torch.cat((batch["batch_idx"][:, None], batch["cls"], batch["bboxes"]), 1).cpu().numpy()
    assert np.array_equal(got, rows) and batch["n_max"] == max(len(l[0]) for l in lab)
    if kind == "pose":
        assert np.array_equal(batch["keypoints"].cpu().numpy(), np.concatenate([l[2] for l in lab], 0))
    low = kind == "detect"                                # the detect model is the project's low-light one, front end included
    name, cls = dict(detect=("yolov8-lowlight.yaml", DetectionModel), segment=("yolov8-seg.yaml", SegmentationModel), pose=("yolov8-pose.yaml", PoseModel))[kind]
    cfgd = load_yaml(name)
    cfgd["scale"] = "n"
    try:
        torch.manual_seed(3)
        tr = DetectionTrainer(get_cfg(dict(model="n", dtype="fp32", optimizer="SGD", batch=4, lowlight_FLAG=low, dedark_FLAG=low, imgsz=imgsz,
                                           deterministic=False, overlap_mask=True, mask_ratio=ratio)))
        tr.setup(cls(dict(cfgd), nc=20))
        loss, items = tr.train_step(dict(next(iter(mk(True)))), [0.01] * 3, 0.9)
        assert bool(torch.isfinite(items).all()) and np.isfinite(float(loss))
    finally:
        dy.set_compute_dtype(torch.float32)


def test_close_mosaic_makes_the_next_epoch_unmixed():
    """epoch 1 is mixed mosaics through the mix entry point, epoch 2 after close_mosaic() un-mixed letterbox samples through the
    plain one: every image equals the host render of a plan made with mosaic = mixup = 0 from the same generator state"""
    from dedark_yolo_amd.data import AugmentHyp, DeviceAugmentLoader
    from dedark_yolo_amd.data import augment as A
    ims, labels = mr.mix_dataset(5, "d1")
    shapes = [im.shape[:2] for im in ims]
    hyp = AugmentHyp(mixup=1.0)
    ld = DeviceAugmentLoader(ims, labels, 64, 4, hyp=hyp, seed=4, shuffle=False)
    first = [b["img"].clone() for b in ld]
    ld.close_mosaic()
    rnd, nprnd = random.Random(), np.random.RandomState()
    rnd.setstate(ld.rnd.getstate())
    nprnd.set_state(ld.nprnd.get_state())
    second = [b["img"].clone() for b in ld]
    torch.cuda.synchronize()
    assert len(first) == len(second) == 2 and hyp.mixup == 1.0 and hyp.mosaic == 1.0 and ld.hyp.mixup == 0.0
    closed = AugmentHyp(mosaic=0.0, mixup=0.0)
    for k in range(8):
        p = A.plan_train_sample(k, shapes, list(range(8)), 64, closed, rnd, nprnd)
        assert not p.mosaic and p.mix is None
        assert np.array_equal(second[k // 4][k % 4].cpu().numpy(), mr.render(p, ims)), k
