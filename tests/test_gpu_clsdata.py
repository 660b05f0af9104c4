"""GPU tests of the classify data pipeline: dy_cls_render through the C-ABI, byte for byte against oracle/augment.py --
format_img(random_hsv(flip(cv_resize_linear_u8(crop, (S, S))))), the project's standing yardstick for the augment kernels (the numpy
restatement of the OpenCV routines, parity with cv2 unpinned; no tolerance) --, ClassifyValLoader / ClassifyTrainLoader on the fixture
tree of tests/clsdata_fixture.py with the crop windows of tests/golden/g34_clsdata.npz, and train(data=) / val(data=) / predict(path)
of a classify model end to end.  Every test runs under its own time limit (an alarm that fails the test instead of letting it wait)."""
import os
import random
import signal

import numpy as np
import pytest
import torch

import clsdata_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
LIMIT_S = 120
SENTINEL = 0xA5

SOURCES = [(37, 53), (64, 64), (5, 200), (200, 5), (1, 1), (300, 301)]                 # (h, w); the first one with a row pitch of 3 w + 7
SIZES = [32, 33, 64]
FLIPS = [(0, 0), (1, 0), (0, 1), (1, 1)]                                              # (fliplr, flipud)
GAINS = np.array([1.0112, 0.62, 1.31])                                                # RandomHSV gains of the "hsv on" cases


@pytest.fixture(autouse=True)
def _time_limit():
    def stop(signum, frame):
        raise TimeoutError(f"a classify data test ran longer than {LIMIT_S} s")
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(LIMIT_S)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def g34():
    return np.load(os.path.join(ROOT, "tests", "golden", "g34_clsdata.npz"))


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    return fx.write_clsdata(tmp_path_factory.mktemp("clsdata"))


def _crops(h, w):
    """(x0, y0, cw, ch): the full image, the last pixel, a one-pixel-wide column, a window ending exactly at the right and bottom
    edges, an interior window (as far as the image has an interior)"""
    return dict(full=(0, 0, w, h), last=(w - 1, h - 1, 1, 1), column=(w // 2, 0, 1, h), edge=(w // 3, h // 3, w - w // 3, h - h // 3),
                interior=(w // 4, h // 4, max(w // 2, 1), max(h // 2, 1)))


@pytest.fixture(scope="module")
def sources():
    """numpy images and their device copies: list of (numpy HWC, device HWC view); the first lives in rows of 3 w + 7 bytes"""
    g = np.random.default_rng(3401)
    out = []
    for k, (h, w) in enumerate(SOURCES):
        im = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        pitch = 3 * w + (7 if k == 0 else 0)
        flat = torch.full((h * pitch,), 201, dtype=torch.uint8, device="cuda")
        view = torch.as_strided(flat, (h, w, 3), (pitch, 3, 1))
        view.copy_(torch.from_numpy(im).cuda())
        assert view.stride(0) == pitch
        out.append((im, view))
    return out


_RESIZED = {}


def _want(k, im, rect, S, fliplr, flipud, hsv):
    """the yardstick; the resize of a (source, crop, S) is computed once and shared by its eight flip / colour cases"""
    from oracle import augment as oa
    x0, y0, cw, ch = rect
    key = (k, rect, S)
    if key not in _RESIZED:
        _RESIZED[key] = oa.cv_resize_linear_u8(im[y0:y0 + ch, x0:x0 + cw], (S, S))
    r = _RESIZED[key]
    if flipud:
        r = np.flipud(r)
    if fliplr:
        r = np.fliplr(r)
    if hsv:
        r = oa.random_hsv(np.ascontiguousarray(r), GAINS)
    return oa.format_img(r)


def _describe(cases, sources):
    """dy_cls_sample records of cases = [(source index, rect, fliplr, flipud, hsv)] as a device byte tensor"""
    from dedark_yolo_amd.data.augment import cls_descriptors
    from oracle import augment as oa
    d = cls_descriptors(len(cases))
    luts = oa.hsv_luts(GAINS)
    for rec, (k, rect, lr, ud, hsv) in zip(d, cases):
        view = sources[k][1]
        rec["src"], rec["pitch"], rec["sh"], rec["sw"] = view.data_ptr(), view.stride(0), view.shape[0], view.shape[1]
        rec["x0"], rec["y0"], rec["cw"], rec["ch"] = rect
        rec["fliplr"], rec["flipud"], rec["hsv"] = lr, ud, hsv
        if hsv:
            rec["lut"][0], rec["lut"][1], rec["lut"][2] = luts
        else:
            rec["lut"][...] = 77                                               # tables that must not be read
    return torch.from_numpy(d.view(np.uint8).copy()).cuda()


def _render(desc, B, S, front=64, back=64):
    """the launch into the middle of a sentinel buffer: (out [B, 3, S, S] as numpy, guards intact?)"""
    from dedark_yolo_amd._C import call
    from dedark_yolo_amd.ops import stream
    n = B * 3 * S * S
    buf = torch.full((front + n + back,), SENTINEL, dtype=torch.uint8, device="cuda")
    call("dy_cls_render", desc.data_ptr(), B, S, buf.data_ptr() + front, stream())
    host = buf.cpu().numpy()
    intact = bool((host[:front] == SENTINEL).all() and (host[front + n:] == SENTINEL).all())
    return host[front:front + n].reshape(B, 3, S, S), intact


@pytest.mark.parametrize("S", SIZES)
def test_render_every_source_crop_flip_and_colour_case_in_one_launch(sources, S):
    """6 sources x 5 crops x 4 flips x HSV on / off = 240 descriptors in ONE launch (blockIdx.z far above one wave's worth of samples,
    all six sources mixed); an unaligned output address sends S = 32 / 64 down the byte-store path as well"""
    cases = [(k, rect, lr, ud, hsv) for k, (h, w) in enumerate(SOURCES) for rect in _crops(h, w).values() for lr, ud in FLIPS
             for hsv in (0, 1)]
    assert len(cases) == 240
    desc = _describe(cases, sources)
    for front in (64, 61):                                                     # 4-byte aligned (one 32-bit store per plane when S % 4 == 0), and not
        got, intact = _render(desc, len(cases), S, front=front)
        assert intact, f"S={S} front={front}: bytes outside the output were written"
        for b, (k, rect, lr, ud, hsv) in enumerate(cases):
            want = _want(k, sources[k][0], rect, S, lr, ud, hsv)
            assert np.array_equal(got[b], want), (f"S={S} front={front} source {SOURCES[k]} crop {rect} fliplr={lr} flipud={ud} hsv={hsv}: "
                                                  f"{int((got[b] != want).sum())} of {want.size} bytes differ")


@pytest.mark.parametrize("S", SIZES)
def test_render_single_samples_and_a_batch_of_the_six_sources(sources, S):
    """B = 1 for every source (crop / flip / colour cases taken in turn), and B = 6 mixing all six sources"""
    names = list(_crops(8, 8))
    picks = []
    for k, (h, w) in enumerate(SOURCES):
        j = k + SIZES.index(S)
        picks.append((k, _crops(h, w)[names[j % 5]], *FLIPS[j % 4], j % 2))
    for case in picks:
        got, intact = _render(_describe([case], sources), 1, S, front=32, back=16)
        assert intact and np.array_equal(got[0], _want(case[0], sources[case[0]][0], case[1], S, *case[2:])), (S, case)
    got, intact = _render(_describe(picks, sources), 6, S)
    assert intact
    for b, case in enumerate(picks):
        assert np.array_equal(got[b], _want(case[0], sources[case[0]][0], case[1], S, *case[2:])), (S, case)


def test_pixels_outside_the_crop_never_reach_the_output(sources):
    """interior crops of the pitched 37 x 53 image and of 64 x 64: every pixel outside the window (and the row padding) is overwritten
    between two launches; the output bytes stay the same.  An enlarging resize (S = 64 from a 26 x 18 window) clamps at all four
    edges of the window."""
    for k in (0, 1):
        im, view = sources[k]
        h, w = im.shape[:2]
        rect = _crops(h, w)["interior"]
        x0, y0, cw, ch = rect
        assert x0 > 0 and y0 > 0 and x0 + cw < w and y0 + ch < h
        cases = [(k, rect, lr, ud, hsv) for lr, ud in FLIPS for hsv in (0, 1)]
        desc = _describe(cases, sources)
        for S in (33, 64):
            before, _ = _render(desc, len(cases), S)
            keep = view.clone()
            try:
                inside = view[y0:y0 + ch, x0:x0 + cw].clone()
                base = view._base if view._base is not None else view
                base.fill_(13)                                                  # the whole allocation, row padding included
                view.copy_(255 - keep)
                view[y0:y0 + ch, x0:x0 + cw] = inside
                after, _ = _render(desc, len(cases), S)
            finally:
                view.copy_(keep)
            assert np.array_equal(before, after), (SOURCES[k], S)
            assert np.array_equal(before[0], _want(k, im, rect, S, 0, 0, 0))


def test_render_refuses_bad_arguments_before_any_launch(sources):
    from dedark_yolo_amd._C import lib
    from dedark_yolo_amd.ops import stream
    f = lib().dy_cls_render
    S = 32
    out = torch.full((2 * 3 * S * S,), SENTINEL, dtype=torch.uint8, device="cuda")
    good = _describe([(1, (0, 0, 64, 64), 0, 0, 0)], sources)
    assert f(None, 1, S, out.data_ptr(), stream()) == 1                         # null descriptors with B > 0
    assert f(good.data_ptr(), 1, S, None, stream()) == 1                        # null output with B > 0
    assert f(good.data_ptr(), 1, 0, out.data_ptr(), stream()) == 1              # S <= 0
    assert f(good.data_ptr(), 1, -4, out.data_ptr(), stream()) == 1
    assert f(good.data_ptr(), -1, S, out.data_ptr(), stream()) == 1             # B < 0
    h, w = SOURCES[0]
    bad = [(0, 0, 0, 5), (0, 0, 5, 0), (0, 0, -3, 5),                           # empty
           (w - 4, 0, 5, 5), (0, h - 4, 5, 5), (-1, 0, 5, 5), (0, -1, 5, 5), (0, 0, w + 1, h), (2 ** 31 - 1, 0, 2, 2)]      # not inside
    for rect in bad:
        assert f(_describe([(0, rect, 0, 0, 0)], sources).data_ptr(), 1, S, out.data_ptr(), stream()) == 1, rect
        assert b"crop" in lib().dy_last_error()
    two = _describe([(1, (0, 0, 64, 64), 0, 0, 0), (0, (w - 4, 0, 5, 5), 0, 0, 0)], sources)
    assert f(two.data_ptr(), 2, S, out.data_ptr(), stream()) == 1               # one bad sample refuses the whole batch ...
    assert f(None, 0, S, None, stream()) == 0                                   # B == 0 succeeds and writes nothing
    assert f(good.data_ptr(), 0, S, out.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                        # ... and nothing was written by any of them
    assert f(good.data_ptr(), 1, S, out.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert bool((out[3 * S * S:] == SENTINEL).all()) and not bool((out[:3 * S * S] == SENTINEL).all())
    from dedark_yolo_amd.data.augment import center_plan, cls_render
    plan = center_plan((64, 64))
    plan.rect = (60, 0, 8, 8)
    with pytest.raises(ValueError, match="crop"):                               # the Python wrapper checks before it uploads
        cls_render([sources[1][1]], [plan], S)
    assert tuple(cls_render([], [], S).shape) == (0, 3, S, S)


# ---- loaders ---------------------------------------------------------------------------------------------------------------------------
def _centre_want(f, g34, S):
    """the val transform of file f by the yardstick, through the crop window the reference's CenterCrop takes for its shape"""
    from dedark_yolo_amd.data.dataset import decode
    from oracle import augment as oa
    im = decode(f)
    shapes = [tuple(s) for s in g34["crop_shapes"]]
    if im.shape[:2] in shapes:
        top, left, ch, cw = (int(v) for v in g34["crop_calls"][shapes.index(im.shape[:2])][:4])
    else:
        m = min(im.shape[:2])
        top, left, ch, cw = (im.shape[0] - m) // 2, (im.shape[1] - m) // 2, m, m
    return oa.format_img(oa.cv_resize_linear_u8(im[top:top + ch, left:left + cw], (S, S)))


def _split_files(roots, name, split):
    from dedark_yolo_amd.data import dataset as ds
    return ds.load_cls_split(ds.check_cls_dataset(roots[name]), split)


def test_val_loader_batches_equal_the_yardstick_on_the_golden_windows(g34, roots):
    from dedark_yolo_amd.data import ClassifyValLoader
    from dedark_yolo_amd.data.dataset import decode
    files, cls = _split_files(roots, "main", "val")
    assert [decode(f).shape[:2] for f in files] == [tuple(s) for s in g34["crop_shapes"]]      # every pinned window is used
    S = int(g34["crop_size"])
    loader = ClassifyValLoader(files, cls, S, 4, "cuda", workers=2)
    batches = list(loader)
    assert len(loader) == 2 and [len(b["im_file"]) for b in batches] == [4, 2]            # the last, smaller batch is there
    k = 0
    for b in batches:
        assert b["img"].dtype == torch.uint8 and b["img"].is_cuda and tuple(b["img"].shape) == (len(b["im_file"]), 3, S, S)
        assert b["cls"].dtype == torch.int64 and b["cls"].is_cuda and b["cls"].tolist() == fx.VAL_CLS[k:k + len(b["im_file"])]
        got = b["img"].cpu().numpy()
        for j, f in enumerate(b["im_file"]):
            assert f == files[k]
            want = _centre_want(f, g34, S)
            assert np.array_equal(got[j], want), f"{f}: {int((got[j] != want).sum())} bytes differ"
            k += 1
    for a, b in zip(batches, loader):                                                    # a second epoch: the same bytes
        assert torch.equal(a["img"], b["img"]) and torch.equal(a["cls"], b["cls"])


@pytest.fixture(scope="module")
def train_set(roots):
    from dedark_yolo_amd.data.dataset import decode
    files, cls = _split_files(roots, "main", "train")
    assert cls.tolist() == fx.TRAIN_CLS
    return files, cls, [decode(f) for f in files]


def _epoch(loader):
    out = [(b["img"].clone(), b["cls"].clone()) for b in loader]
    torch.cuda.synchronize()
    return out


def test_train_loader_seeds_modes_and_the_yardstick(train_set):
    from dedark_yolo_amd.data import ClassifyHyp, ClassifyTrainLoader, plan_cls_sample
    files, cls, ims = train_set
    S, bs, hyp = 32, 4, ClassifyHyp(flipud=0.5)
    mk = lambda **kw: ClassifyTrainLoader(ims, cls, S, bs, hyp=hyp, **kw)
    random.seed(123)
    before = random.getstate()
    a, b, c = _epoch(mk(seed=7)), _epoch(mk(seed=7)), _epoch(mk(seed=8))
    host = mk(seed=7, resident=False)
    d = _epoch(host)
    assert len(a) == len(b) == len(c) == len(d) == 3 and random.getstate() == before      # the caller's generator is left alone
    for (xa, ca), (xb, cb), (xd, cd) in zip(a, b, d):
        assert xa.dtype == torch.uint8 and tuple(xa.shape) == (bs, 3, S, S) and xa.is_cuda
        assert ca.dtype == torch.int64 and ca.is_cuda and tuple(ca.shape) == (bs,)
        assert torch.equal(xa, xb) and torch.equal(ca, cb), "one seed, two loaders"
        assert torch.equal(xa, xd) and torch.equal(ca, cd), "resident and pinned-host modes"
    assert host.uploaded_bytes == sum(im.size for im in ims) and not host.images[0].is_cuda and host.images[0].is_pinned()
    assert not all(torch.equal(x, y) for (x, _), (y, _) in zip(a, c)), "another seed gives other bytes"
    # the first epoch replayed: shuffle, then the plans sample by sample from the loader's two generators; pixels by the yardstick
    r, n = random.Random(7), np.random.RandomState(8)
    order = list(range(len(ims)))
    r.shuffle(order)
    for k, (img, ids) in enumerate(a):
        chunk = order[k * bs:(k + 1) * bs]
        assert ids.tolist() == [fx.TRAIN_CLS[i] for i in chunk]
        got = img.cpu().numpy()
        for j, i in enumerate(chunk):
            p = plan_cls_sample(ims[i].shape[:2], hyp, r, n)
            from oracle import augment as oa
            x0, y0, cw, ch = p.rect
            want = oa.cv_resize_linear_u8(ims[i][y0:y0 + ch, x0:x0 + cw], (S, S))
            want = np.flipud(want) if p.flipud else want
            want = np.fliplr(want) if p.fliplr else want
            want = oa.format_img(oa.random_hsv(np.ascontiguousarray(want), p.hsv_gains))
            assert np.array_equal(got[j], want), (k, j, p.rect, p.fliplr, p.flipud)
    second = _epoch(mk(seed=7))                                                          # (a fresh loader: epoch one again)
    assert all(torch.equal(x, y) for (x, _), (y, _) in zip(a, second))


def test_train_loader_without_augmentation_is_the_val_transform(g34, train_set):
    from dedark_yolo_amd.data import ClassifyTrainLoader
    files, cls, ims = train_set
    S = 32
    loader = ClassifyTrainLoader(ims, cls, S, 5, seed=3, shuffle=False, drop_last=False, augment=False)
    batches = _epoch(loader)
    assert len(loader) == 3 and [len(c) for _, c in batches] == [5, 5, 2]
    assert torch.cat([c for _, c in batches]).tolist() == fx.TRAIN_CLS                   # the folder ids, int64, on the device
    got = torch.cat([x for x, _ in batches]).cpu().numpy()
    for k, f in enumerate(files):
        assert np.array_equal(got[k], _centre_want(f, g34, S)), f
    assert len(ClassifyTrainLoader(ims, cls, S, 5, shuffle=False, augment=False)) == 2   # drop_last is the default


def test_built_loaders_equal_hand_built_ones(roots, train_set):
    from dedark_yolo_amd.data import (ClassifyTrainLoader, ClassifyValLoader, build_cls_train_loader, build_cls_val_loader,
                                      check_cls_dataset)
    from dedark_yolo_amd.data.loader import _classify_hyp
    from dedark_yolo_amd.engine.trainer import get_cfg
    files, cls, ims = train_set
    data = check_cls_dataset(roots["main"])
    args = get_cfg(dict(imgsz=32, batch=4, seed=5, workers=2, flipud=0.25))
    built = build_cls_train_loader(args, data, "cuda")
    hand = ClassifyTrainLoader(ims, cls, 32, 4, hyp=_classify_hyp(args), seed=5)
    assert built.resident and built.hyp.flipud == 0.25 and len(built) == len(hand) == 3
    for (xa, ca), (xb, cb) in zip(_epoch(built), _epoch(hand)):
        assert torch.equal(xa, xb) and torch.equal(ca, cb)
    shard = build_cls_train_loader(args, data, "cuda", rank=1, world_size=2)             # rank r takes the samples r::world_size
    assert shard.im_files == files[1::2] and shard.cls.tolist() == fx.TRAIN_CLS[1::2]
    half = build_cls_train_loader(get_cfg(dict(imgsz=32, batch=2, fraction=0.5, workers=2)), data, "cuda")
    assert half.im_files == files[:6]
    vfiles, vcls = _split_files(roots, "main", "val")
    bv, hv = build_cls_val_loader(args, data, "cuda", "val", batch=8), ClassifyValLoader(vfiles, vcls, 32, 8, "cuda")
    assert len(bv) == len(hv) == 1
    for x, y in zip(bv, hv):
        assert torch.equal(x["img"], y["img"]) and torch.equal(x["cls"], y["cls"]) and x["im_file"] == y["im_file"]


# ---- the public interface ---------------------------------------------------------------------------------------------------------------
TINY = [0.33, 0.125, 1024]                                                              # the scale tests/test_gpu_classify.py builds
KW = dict(imgsz=32, batch=4, dtype="fp32", workers=2)


def _tiny_yolo(nc=10):
    import dedark_yolo_amd as dy
    from util import load_yaml
    from dedark_yolo_amd.engine.model import YOLO
    from dedark_yolo_amd.nn.tasks import ClassificationModel
    dy.set_compute_dtype(torch.float32)
    cfg = load_yaml("cls/yolov8-cls.yaml")
    cfg["scales"]["t"] = TINY
    cfg["scale"] = "t"
    torch.manual_seed(4)
    y = YOLO("yolov8n-cls.yaml")
    y.model = ClassificationModel(cfg, nc=nc).cuda()
    return y


@pytest.fixture(scope="module")
def trained(roots, tmp_path_factory):
    """one epoch of train(data=<dir>) on the fixture tree, checkpoints into save_dir"""
    import dedark_yolo_amd as dy
    save = tmp_path_factory.mktemp("cls_run")
    y = _tiny_yolo()
    try:
        hist = y.train(data=roots["main"], epochs=1, save_dir=str(save), **KW)
    finally:
        dy.set_compute_dtype(torch.float32)
    return y, hist, str(save)


def test_train_from_a_dataset_directory(trained):
    y, hist, save = trained
    assert len(hist) == 1 and len(hist[0]) == 1 and np.isfinite(hist[0]).all()
    assert int(y.model.yaml["nc"]) == 3 and y.model.names == {0: "ant", 1: "bee", 2: "cat"}      # the head was rebuilt from nc = 10
    assert {"metrics/accuracy_top1", "metrics/accuracy_top5", "fitness"} <= set(y.trainer.metrics)
    assert 0.0 <= y.trainer.metrics["metrics/accuracy_top1"] <= y.trainer.metrics["metrics/accuracy_top5"] <= 1.0
    assert y.trainer.args.imgsz == 32 and os.path.isfile(os.path.join(save, "weights", "last.pt"))


def test_imgsz_defaults_to_224_for_a_classify_model_only_when_not_given():
    y = _tiny_yolo()
    assert y._cls_imgsz({})["imgsz"] == 224 and y._cls_imgsz(dict(imgsz=96))["imgsz"] == 96
    y.overrides["imgsz"] = 64
    assert "imgsz" not in y._cls_imgsz({})


def test_val_from_a_dataset_directory(trained, roots):
    from dedark_yolo_amd.data import ClassifyValLoader
    y = trained[0]
    got = y.val(data=roots["main"], **KW)
    assert set(got) == {"metrics/accuracy_top1", "metrics/accuracy_top5", "fitness"}
    files, cls = _split_files(roots, "main", "val")
    by_hand = list(ClassifyValLoader(files, cls, 32, 4, "cuda"))
    assert y.val(loader=by_hand, **KW) == got
    assert int(y.validator.confusion_matrix.sum()) == 6
    tfiles, tcls = _split_files(roots, "only_test", "test")
    got_t = y.val(data=roots["only_test"], split="val", **KW)                            # no val/ there: test/ is used
    assert int(y.validator.confusion_matrix.sum()) == len(tfiles) == 4
    assert y.val(loader=list(ClassifyValLoader(tfiles, tcls, 32, 4, "cuda")), **KW) == got_t
    with pytest.raises(ValueError, match="dog"):
        y.val(data=roots["mismatch"], **KW)
    ten = _tiny_yolo()
    with pytest.raises(ValueError, match="classes"):                                     # the ValueError the other tasks raise
        ten.val(data=roots["main"], **KW)


def test_predict_files_directories_and_arrays(trained, roots, g34):
    from dedark_yolo_amd.data.dataset import decode
    from dedark_yolo_amd.engine.results import Probs
    y = trained[0]
    files, _ = _split_files(roots, "main", "val")
    S = 32
    hand = torch.from_numpy(np.stack([_centre_want(f, g34, S) for f in files])).cuda()
    from dedark_yolo_amd.engine.trainer import get_cfg
    step = int(get_cfg(dict(y.overrides)).batch)                                         # the cfg's `batch`: the chunk predict() forwards
    assert 1 < step < len(files)
    want = [r for o in range(0, len(files), step) for r in y.predict(hand[o:o + step])]
    res = y.predict(os.path.join(roots["main"], "val"), imgsz=S)
    assert len(res) == len(files) == 6
    for r, f, w in zip(res, files, want):
        assert r.path == f and tuple(r.orig_shape) == decode(f).shape[:2] and isinstance(r.probs, Probs) and r.boxes is None
        assert torch.equal(r.probs.data, w.probs.data), f
        assert abs(float(r.probs.data.sum()) - 1.0) < 1e-5 and len(r.probs) == 3
    one = y.predict(files[5], imgsz=S)                                                   # the 300 x 301 file, alone
    assert len(one) == 1 and one[0].path == files[5] and torch.equal(one[0].probs.data, y.predict(hand[5:6])[0].probs.data)
    arr = y.predict([decode(files[0])], imgsz=S)
    assert arr[0].path is None and tuple(arr[0].orig_shape) == (37, 53)
    assert torch.equal(arr[0].probs.data, y.predict(hand[0:1])[0].probs.data)
    mixed = y(files[:2] + [decode(files[2])], imgsz=S)                                   # a list of files and arrays
    assert [r.path for r in mixed] == files[:2] + [None]
    assert all(torch.equal(r.probs.data, w.probs.data) for r, w in zip(mixed, want[:3]))


def test_train_refuses_a_mismatched_val_split_and_a_set_below_one_batch(roots):
    import dedark_yolo_amd as dy
    try:
        with pytest.raises(ValueError, match="dog"):
            _tiny_yolo().train(data=roots["mismatch"], epochs=1, imgsz=32, batch=2, dtype="fp32", workers=2)
        with pytest.raises(ValueError, match="fewer than one batch"):
            _tiny_yolo().train(data=roots["only_test"], epochs=1, **KW)                  # 3 training images, batch 4
        with pytest.raises(FileNotFoundError, match="no_train"):
            _tiny_yolo().train(data=roots["no_train"], epochs=1, **KW)
    finally:
        dy.set_compute_dtype(torch.float32)
