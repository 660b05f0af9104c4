"""GPU tests of the segment / pose side of the device loader: the polygon rasteriser (csrc/polymask.hip: dy_polymask_raster,
dy_polymask_compose) byte for byte against tests/polymask_ref.py (the per-pixel numpy statement of the stated rule), loader batches of
task="segment" / "pose" against the reference's own batches (tests/golden/g20_*.npz), and a training step fed by the loader."""
import os

import numpy as np
import pytest
import torch

import polymask_ref as pr
from augtask_data import CASES, IMGSZ
from test_augtask_cpu import case_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = [0.33, 0.125, 1024]


def _pad(poly, P):
    """a polygon as exactly P vertices: the last one repeated (repeated consecutive vertices change nothing)"""
    p = np.asarray(poly, dtype=np.int64).reshape(-1, 2)
    assert len(p) <= P
    return np.concatenate((p, np.repeat(p[-1:], P - len(p), 0)), 0)


def _run(images, P, s, r, overlap=True):
    """images: per image a list of polygons.  Returns (device result, reference result, packed inputs)."""
    from dedark_yolo_amd.data import polygon_masks
    polys = np.array([_pad(q, P) for im in images for q in im], dtype=np.int16).reshape(-1, P, 2)
    offsets = np.concatenate(([0], np.cumsum([len(im) for im in images]))).astype(np.int32)
    n = len(polys)
    rows = np.zeros((n, 6), np.float32)
    rows[:, 0] = np.repeat(np.arange(len(images)), [len(im) for im in images])
    rows[:, 1:] = np.arange(n * 5, dtype=np.float32).reshape(n, 5) + 0.25           # every row distinct
    got = polygon_masks(torch.from_numpy(polys).cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(rows).cuda(), len(images), s, s, r,
                        overlap)
    torch.cuda.synchronize()
    want = pr.batch_reference(polys, offsets, rows, s, s, r, overlap)
    return got, want, (polys, offsets, rows)


def _same(got, want, overlap=True):
    if not overlap:
        assert got[1] is None and got[2] is None
        assert got[0].dtype == torch.uint8 and torch.equal(got[0].cpu(), torch.from_numpy(want))
        return
    for g, w, name in zip(got, want, ("masks", "rows", "perm")):
        w = torch.from_numpy(w)
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w), name


def _shapes(s, r):
    """the geometry list of the kernel tests, for an s x s plane at ratio r (tap rows: r i + r / 2 - 1 and the next)"""
    t = r * 3 + r // 2 - 1 if r > 1 else 5                                            # a tap row / column
    return [
        [[2, t], [s - 3, t], [s - 3, t + 1 + r], [2, t + 1 + r]],                     # horizontal edges ON tap rows
        [[t, 1], [t + 1, 1], [t + 1, s - 2], [t, s - 2]],                             # vertical edges on tap columns
        [[4, 4], [4, 4], [20, 4], [20, 4], [20, 4], [20, 18], [4, 18], [4, 18]],      # repeated consecutive vertices
        [[2, 2], [28, 2], [28, 26], [15, 8], [2, 26]],                                # concave
        [[16, 1], [25, 29], [2, 11], [30, 11], [7, 29]],                              # self-intersecting (pentagram)
        [[s, 0], [s, s], [s, s // 2]],                                                # collapsed onto the border x == s
        [[0, s], [s, s], [s // 2, s]],                                                # ... and onto y == s
        [[7, 9]],                                                                     # one pixel
        [[0, 0], [s, 0], [s, s], [0, s]],                                             # the whole plane, vertices at x == s, y == s
        [[1, 1], [s - 1, s - 2]],                                                     # a two-vertex polygon: a slanted segment
    ]


@pytest.mark.parametrize("s,r", [(64, 4), (32, 1), (32, 2)])
@pytest.mark.parametrize("P", [5, 64, 1000])
def test_rasteriser_vs_reference(s, r, P):
    """P = 5 (not a multiple of the wave), 64 (exactly one wave), 1000 (the real count; resampled random polygons join the list);
    an image without instances sits between two that have some"""
    g = np.random.default_rng(100 * P + s + r)
    shapes = [q for q in _shapes(s, r) if len(q) <= P]
    rand = [g.integers(0, s + 1, (int(g.integers(3, min(P, 12) + 1)), 2)) for _ in range(6)]
    if P == 1000:
        from dedark_yolo_amd.data import resample_segments
        rand += list((resample_segments([g.uniform(0, 1, (int(g.integers(5, 13)), 2)) for _ in range(4)]) * s).astype(np.int32))
    images = [shapes, [], rand]
    got, want, _ = _run(images, P, s, r)
    assert got[0].shape == (3, s // r, s // r) and int(got[0][1].max()) == 0          # the empty image is all zero
    _same(got, want)
    got, want, _ = _run(images, P, s, r, overlap=False)
    _same(got, want, overlap=False)


def test_empty_batch():
    from dedark_yolo_amd.data import polygon_masks
    z = lambda *sh, dt: torch.zeros(sh, dtype=dt, device="cuda")
    m, rows, perm = polygon_masks(z(0, 1000, 2, dt=torch.int16), z(4, dt=torch.int32), z(0, 6, dt=torch.float32), 3, 64, 64, 4, True)
    torch.cuda.synchronize()
    assert m.shape == (3, 16, 16) and int(m.max()) == 0 and rows.shape == (0, 6) and perm.shape == (0,)
    planes, _, _ = polygon_masks(z(0, 1000, 2, dt=torch.int16), z(4, dt=torch.int32), z(0, 6, dt=torch.float32), 3, 64, 64, 4, False)
    assert planes.shape == (0, 16, 16)


def test_seventy_instances_in_one_image():
    """more instances than a wave has lanes: the rank / permutation code walks all of them"""
    g = np.random.default_rng(70)
    many = []
    for _ in range(70):
        c, h = g.integers(8, 56, 2), g.integers(1, 8, 2)
        many.append([[c[0] - h[0], c[1] - h[1]], [c[0] + h[0], c[1] - h[1]], [c[0] + h[0], c[1] + h[1]], [c[0] - h[0], c[1] + h[1]]])
    got, want, _ = _run([many[:3], many], 5, 64, 4)
    _same(got, want)
    assert sorted(got[2][3:].cpu().tolist()) == list(range(70))


def test_nested_instances_and_the_tie_rule():
    s = 32
    big, small = [[2, 2], [28, 2], [28, 28], [2, 28]], [[10, 10], [16, 10], [16, 16], [10, 16]]
    twin = [[20, 20], [26, 20], [26, 26], [20, 26]]                                   # same area as `small`, later in the labels
    got, want, (_, _, rows) = _run([[small, big, twin]], 5, s, 1)
    _same(got, want)
    m = got[0][0].cpu()
    assert got[2].cpu().tolist() == [1, 0, 2]                                         # area descending, equal areas by original index
    assert int(m[5, 5]) == 1 and int(m[12, 12]) == 2 and int(m[22, 22]) == 3 and int(m[0, 0]) == 0      # the smaller instance wins
    assert torch.equal(got[1].cpu(), torch.from_numpy(rows[[1, 0, 2]]))               # the label rows follow the mask indices


def test_two_runs_give_identical_bytes():
    g = np.random.default_rng(5)
    images = [[g.integers(0, 65, (9, 2)) for _ in range(12)] for _ in range(4)]
    a, want, _ = _run(images, 64, 64, 4)
    b, _, _ = _run(images, 64, 64, 4)
    _same(a, want)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_bad_arguments_raise():
    from dedark_yolo_amd.data import polygon_masks
    p, o, r = torch.zeros((1, 5, 2), dtype=torch.int16, device="cuda"), torch.tensor([0, 1], dtype=torch.int32, device="cuda"), torch.zeros((1, 6), device="cuda")
    with pytest.raises(ValueError, match="mask_ratio"):
        polygon_masks(p, o, r, 1, 64, 64, 3)
    with pytest.raises(ValueError, match="multiple"):
        polygon_masks(p, o, r, 1, 66, 66, 4)
    with pytest.raises(RuntimeError, match="dy_polymask_raster"):
        polygon_masks(p, o, r, 1, 4096, 4096, 4)                                      # wider than the row bitmap


# ------------------------------------------------------------------------------------------------ the loader
@pytest.fixture(scope="module")
def g20():
    z = {}
    for name in ("g20_augseg.npz", "g20_augpose.npz"):
        z.update(np.load(os.path.join(ROOT, "tests", "golden", name)))
    return z


def _loader_batch(z, tag, task=None):
    """the golden's samples as ONE loader batch: the loader's own generators seeded like the generator's global ones"""
    from dedark_yolo_amd.data import DeviceAugmentLoader
    kind, seed, ims, labels, picks, hyp, ratio, overlap, flip_idx = case_inputs(z, tag)
    ld = DeviceAugmentLoader(ims, labels, IMGSZ, len(picks), hyp=hyp, seed=seed + 1, task=task or kind, flip_idx=flip_idx, mask_ratio=ratio,
                             overlap_mask=overlap)
    batch, ev, _ = ld._prepare(picks)
    ev.synchronize()
    return batch, ld


@pytest.mark.parametrize("tag", list(CASES))
def test_loader_batch_equals_the_reference_batch(g20, tag):
    z = g20
    kind, picks, overlap = CASES[tag][0], CASES[tag][3], CASES[tag][6]
    batch, _ = _loader_batch(z, tag)
    cat = lambda key, tail: np.concatenate([z[f"{tag}_n{k}_{key}"].reshape((-1,) + tail) for k in range(len(picks))], 0)
    counts = [len(z[f"{tag}_n{k}_cls"]) for k in range(len(picks))]
    assert np.array_equal(batch["batch_idx"].cpu().numpy(), np.repeat(np.arange(len(picks)), counts).astype(np.float32))
    assert np.array_equal(batch["cls"].cpu().numpy(), cat("cls", (1,))) and np.array_equal(batch["bboxes"].cpu().numpy(), cat("bboxes", (4,)))
    assert batch["n_max"] == max(counts) and batch["cls"].is_cuda
    if kind == "segment":
        m = batch["masks"]
        assert m.dtype == torch.uint8 and m.is_cuda and np.array_equal(m.cpu().numpy(), cat("masks", z[f"{tag}_n0_masks"].shape[1:]))
        if overlap:
            assert np.array_equal(batch["sorted_idx"].cpu().numpy(), cat("sorted_idx", ()))
            assert m.shape[0] == len(picks) and (0 not in counts or int(m[counts.index(0)].max()) == 0)
        else:
            assert m.shape[0] == sum(counts) and "sorted_idx" not in batch
    else:
        kp = batch["keypoints"]
        assert kp.dtype == torch.float32 and kp.is_cuda and np.array_equal(kp.cpu().numpy(), cat("keypoints", z[f"{tag}_n0_keypoints"].shape[1:]))
    det, _ = _loader_batch(z, tag, task="detect")                                      # the pixels do not depend on the task
    assert torch.equal(batch["img"], det["img"]) and "masks" not in det and "keypoints" not in det


@pytest.mark.parametrize("tag", ["s0", "s2", "p0"])
def test_train_step_from_loader_batches(g20, tag):
    """one train_step of a tiny segmentation / pose model on what the loader yields (iterated, so the stream hand-over is the real one)"""
    import dedark_yolo_amd as dy
    from dedark_yolo_amd.data import DeviceAugmentLoader
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    from dedark_yolo_amd.nn.tasks import PoseModel, SegmentationModel
    from util import load_yaml
    kind, seed, ims, labels, picks, hyp, ratio, overlap, flip_idx = case_inputs(g20, tag)
    cfgd = load_yaml("yolov8-seg.yaml" if kind == "segment" else "yolov8-pose.yaml")
    cfgd["scales"]["t"] = TINY
    cfgd["scale"] = "t"
    try:
        torch.manual_seed(3)
        tr = DetectionTrainer(get_cfg(dict(model="tiny", dtype="fp32", optimizer="SGD", batch=4, lowlight_FLAG=False, dedark_FLAG=False,
                                           imgsz=IMGSZ, deterministic=False, overlap_mask=overlap, mask_ratio=4)))
        tr.setup((SegmentationModel if kind == "segment" else PoseModel)(dict(cfgd), nc=20))
        ld = DeviceAugmentLoader(ims, labels, IMGSZ, 4, hyp=hyp, seed=1, task=kind, flip_idx=flip_idx, mask_ratio=4, overlap_mask=overlap)
        n = 0
        for batch in ld:
            loss, items = tr.train_step(dict(batch), [0.01] * 3, 0.9)
            assert items.numel() == (4 if kind == "segment" else 5) and bool(torch.isfinite(items).all()) and np.isfinite(float(loss))
            n += 1
        assert n == len(ims) // 4
    finally:
        dy.set_compute_dtype(torch.float32)
