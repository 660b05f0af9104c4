"""GPU tests of test-time augmentation for detect (predict(augment=True), val(augment=True)): the two kernels per entry point
(dy_tta_scale_img against torch's flip / interpolate / pad on the CPU, dy_detect_decode_tta against dy_detect_decode followed by the
reference's de-scale / de-flip / slice), whole models against the reference's fixtures (tests/golden/make_tta_golden.py) and against
their own three-pass composition restated with torch operators, the engine (YOLO.predict, the validator), the NMS at the merged
anchor count of a 640 x 640 P2 model, and the single-scale fallback of the segment, pose and classify models."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import gold, load_yaml, rnd

pytestmark = pytest.mark.gpu

TINY = [0.33, 0.125, 1024]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SCALES, FLIPS = (1, 0.83, 0.67), (None, 3, None)          # the reference's passes (tasks.py:306-307)


@pytest.fixture(autouse=True)
def _fp32():
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(torch.float32)
    yield
    dy.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------ 1. dy_tta_scale_img
def _scale_img_torch(x, ratio, gs, flip):
    """scale_img(x.flip(flip), ratio, gs=gs) with torch operators (the contract: bilinear, align_corners=False, size = int(H * ratio),
    int(W * ratio); right / bottom padding with 0.447 to ceil(H * ratio / gs) * gs)."""
    import math
    if flip:
        x = x.flip(flip)
    if ratio == 1.0:
        return x
    H, W = x.shape[2:]
    hs, ws = int(H * ratio), int(W * ratio)
    y = F.interpolate(x, size=(hs, ws), mode="bilinear", align_corners=False)
    Hp, Wp = (math.ceil(v * ratio / gs) * gs for v in (H, W))
    return F.pad(y, [0, Wp - ws, 0, Hp - hs], value=0.447)


# (shape, ratio, flip, gs, padded size).  The last case is not a multiple of four wide: rows start off the 16-byte grid, so
# the kernel's scalar stores run
SCALE_CASES = [((2, 3, 96, 160), 0.83, 3, 32, (96, 160)), ((1, 3, 128, 192), 0.67, None, 64, (128, 192)),
               ((2, 3, 64, 96), 0.67, 2, 32, (64, 96)), ((1, 3, 128, 128), 0.67, None, 32, (96, 96)),
               ((2, 3, 64, 96), 1.0, 3, 32, (64, 96)), ((1, 2, 37, 53), 0.67, 3, 7, (28, 42))]


@pytest.mark.parametrize("shape,ratio,flip,gs,padded", SCALE_CASES,
                         ids=["r083_lr", "r067_gs64_kept", "r067_ud", "r067_85px", "r1_lr", "odd_gs7_lr"])
def test_tta_scale_img_vs_torch_cpu(shape, ratio, flip, gs, padded):
    """dy_tta_scale_img against F.pad(F.interpolate(x.flip(...))) evaluated by torch on the CPU.  Pad region exactly float32(0.447);
    ratio 1.0 bit-equal to the flipped image; interior within 2 * max(H, W) * 2^-23: one ulp of the source coordinate (at most
    max(H, W)) times a pixel contrast of at most 1 (x in [0, 1]), doubled.  A wrong tap or an off-by-one flip is about 0.3 off."""
    from dedark_yolo_amd import ops
    x = rnd(701 + shape[2] + shape[3], *shape)
    want = _scale_img_torch(x, ratio, gs, flip)
    got = ops.tta_scale_img(x.cuda(), ratio, gs, flip)
    torch.cuda.synchronize()
    got = got.cpu()
    assert tuple(got.shape) == tuple(want.shape) == (*shape[:2], *padded)
    if ratio == 1.0:
        assert torch.equal(got, want)
        return
    H, W = shape[2:]
    hs, ws = int(H * ratio), int(W * ratio)
    pad = torch.ones(padded, dtype=torch.bool)
    pad[:hs, :ws] = False
    assert bool((got[:, :, pad] == np.float32(0.447)).all()), "pad region is not float32(0.447)"
    assert torch.equal(got[:, :, pad], want[:, :, pad])
    err = float((got[:, :, :hs, :ws] - want[:, :, :hs, :ws]).abs().max())
    atol = 2 * max(H, W) * 2.0 ** -23
    print(f"scale_img {shape} r={ratio} flip={flip}: interior max |d| {err:.3e} (bound {atol:.3e})")
    assert err <= atol, (err, atol)


def test_tta_scale_img_rejects_bad_arguments():
    from dedark_yolo_amd import _C, ops
    x = torch.zeros(1, 3, 32, 32, device="cuda")
    out = torch.zeros(1, 3, 32, 32, device="cuda")
    with pytest.raises(RuntimeError, match="flip"):
        _C.call("dy_tta_scale_img", ops.ptr(x), 1, 3, 32, 32, 26, 26, 32, 32, 1, ops.ptr(out), ops.stream())
    with pytest.raises(RuntimeError, match="does not fit"):
        _C.call("dy_tta_scale_img", ops.ptr(x), 1, 3, 32, 32, 26, 26, 24, 32, 0, ops.ptr(out), ops.stream())
    with pytest.raises(ValueError):
        ops.tta_scale_img(x.half(), 0.83, 32, 3)


# ------------------------------------------------------------------------------------------------ 2. dy_detect_decode_tta
MAP_HW = [(16, 20), (8, 10), (4, 5), (2, 3)]
MAP_STRIDES = [8.0, 16.0, 32.0, 64.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("nc", [20, 3], ids=["nc20", "nc3"])
@pytest.mark.parametrize("nl", [3, 4], ids=["nl3", "nl4"])
def test_detect_decode_tta_vs_plain_decode(nl, nc, dtype):
    """Three dy_detect_decode_tta calls into one NaN-filled merged buffer against dy_detect_decode followed by the reference's
    de-scale (`p[:, :4] /= scale`), de-flip and slice in torch on the device.  Every column written exactly once, columns outside a
    call's window untouched, class rows bit-equal, box rows within rtol 1e-6: the kernel divides where torch multiplies by the
    reciprocal, which is a few f32 ulp of the quotient.  In the mirrored row (img - quotient) those ulp are relative to the operands,
    not to a difference that may cancel, so there the bound is 1e-6 * (img + |quotient|)."""
    from dedark_yolo_amd import _C, ops
    ops.set_compute_dtype(dtype)
    B, img_h, img_w = 2, 128.0, 160.0
    gen = np.random.default_rng(900 + nl * 10 + nc)
    maps = [ops.as_nhwc(torch.from_numpy(gen.normal(0, 1.0, (B, 64 + nc, h, w)).astype(np.float32)).cuda(), dtype) for h, w in MAP_HW[:nl]]
    dm = ops.det_maps(maps, MAP_STRIDES[:nl], nc)
    A = sum(h * w for h, w in MAP_HW[:nl])
    plain = torch.empty((B, 4 + nc, A), dtype=torch.float32, device="cuda")
    _C.call("dy_detect_decode", C.byref(dm), ops.ptr(plain), ops.stream())
    g = sum(4 ** k for k in range(nl))
    # (scale, flip, kept anchors): the clip of the first and the last pass; the last one mirrored up-down to cover flip 2
    passes = [(1.0, None, 0, A - A // g), (0.83, 3, 0, A), (0.67, 2, (A // g) * 4 ** (nl - 1), A)]
    a_total = sum(hi - lo for _, _, lo, hi in passes)
    y = torch.full((B, 4 + nc, a_total), float("nan"), dtype=torch.float32, device="cuda")
    col0 = 0
    for scale, flip, lo, hi in passes:
        before = y.clone()
        _C.call("dy_detect_decode_tta", C.byref(dm), ops.ptr(y), a_total, col0, lo, hi, scale, flip or 0, img_h, img_w, ops.stream())
        torch.cuda.synchronize()
        win = torch.zeros(a_total, dtype=torch.bool, device="cuda")
        win[col0:col0 + hi - lo] = True
        assert torch.equal(y[:, :, ~win].view(torch.int32), before[:, :, ~win].view(torch.int32)), "wrote outside its window"
        assert bool(torch.isnan(before[:, :, win]).all()), "window written before its call"
        assert not bool(torch.isnan(y[:, :, win]).any()), "window not fully written"
        # the reference's order of operations on the plain decode
        p = plain.clone()
        p[:, :4] /= scale
        bound = 1e-6 * p[:, :4].abs()
        if flip == 3:
            bound[:, 0] = 1e-6 * (img_w + p[:, 0].abs())
            p[:, 0] = img_w - p[:, 0]
        elif flip == 2:
            bound[:, 1] = 1e-6 * (img_h + p[:, 1].abs())
            p[:, 1] = img_h - p[:, 1]
        want, got = p[:, :, lo:hi], y[:, :, col0:col0 + hi - lo]
        assert torch.equal(got[:, 4:], want[:, 4:]), "class rows are not bit-equal"
        err = (got[:, :4] - want[:, :4]).abs()
        assert bool((err <= bound[:, :, lo:hi]).all()), float((err / bound[:, :, lo:hi].clamp_min(1e-30)).max())
        col0 += hi - lo
    assert col0 == a_total and not bool(torch.isnan(y).any())


def test_detect_decode_tta_rejects_windows_outside_the_buffers():
    from dedark_yolo_amd import _C, ops
    nc, B = 3, 1
    maps = [ops.as_nhwc(torch.zeros(B, 64 + nc, h, w, device="cuda")) for h, w in MAP_HW[:3]]
    dm = ops.det_maps(maps, MAP_STRIDES[:3], nc)
    A = sum(h * w for h, w in MAP_HW[:3])
    y = torch.zeros((B, 4 + nc, A), device="cuda")
    for col0, lo, hi, flip, what in ((1, 0, A, 0, "columns"), (0, 0, A + 1, 0, "anchors"), (0, 5, 4, 0, "anchors"), (0, 0, A, 1, "flip")):
        with pytest.raises(RuntimeError, match=what):
            _C.call("dy_detect_decode_tta", C.byref(dm), ops.ptr(y), A, col0, lo, hi, 1.0, flip, 128.0, 160.0, ops.stream())


# ------------------------------------------------------------------------------------------------ models
def _model(yaml_name, seed, nc=20, confident=False):
    """Tiny detection model with rng_fill weights (the fixtures' weights); confident=True biases the class logits up so that the NMS
    has something to do (as tests/test_gpu_val.py does)."""
    from oracle import model as om
    from parity_helpers import HYP, load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    cfg = load_yaml(yaml_name)
    cfg["scales"]["t"] = list(TINY)
    cfg["scale"] = "t"
    model = DetectionModel(dict(cfg), ch=3, nc=nc)
    model.args = HYP
    sd = om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed)
    if confident:
        for k in sd:
            if ".cv3." in k and k.endswith("2.bias"):
                sd[k] = sd[k] + 4.0
    load_sd(model, sd)
    return model.cuda().eval()


def _compose(model, x):
    """The reference's augmented inference restated with torch operators around three single-scale calls of the model."""
    head = model.model[-1]
    H, W = x.shape[2:]
    gs = int(max(head.strides_as_floats()))
    ys = []
    for s, f in zip(SCALES, FLIPS):
        yi = model(_scale_img_torch(x, s, gs, f).contiguous())[0].clone()
        yi[:, :4] /= s
        bx, by, wh, cls = yi.split((1, 1, 2, yi.shape[1] - 4), 1)
        if f == 2:
            by = H - by
        elif f == 3:
            bx = W - bx
        ys.append(torch.cat((bx, by, wh, cls), 1))
    g = sum(4 ** k for k in range(head.nl))
    ys[0] = ys[0][..., :-(ys[0].shape[-1] // g)]
    ys[-1] = ys[-1][..., (ys[-1].shape[-1] // g) * 4 ** (head.nl - 1):]
    return torch.cat(ys, -1)


FIXTURES = [("g23_tta_ori", "yolov8ori.yaml", 701), ("g23_tta_ll", "yolov8-lowlight.yaml", 701), ("g23_tta_rect", "yolov8ori.yaml", 675),
            ("g23_tta_p6", "yolov8-p6.yaml", 1140), ("g23_tta_p2", "yolov8-p2.yaml", None)]


@pytest.mark.parametrize("name,yml,a_total", FIXTURES, ids=[f[0][8:] for f in FIXTURES])
def test_model_augment_vs_reference_fixture(name, yml, a_total):
    """model(x, augment=True)[0] in fp32 against the reference's (tests/golden/g23_tta_*.npz), with the metric and bound of the
    whole-model eval check of tests/test_gpu_p2p6.py: max |d| / max |y| <= 1e-4 at the tiny scale."""
    from dedark_yolo_amd.nn.tasks import tta_plan
    g = gold(name)
    model = _model(yml, int(g["seed"]))
    B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    head = model.model[-1]
    want_a = tta_plan(H, W, head.strides_as_floats(), head.nl)[1]
    assert want_a == int(g["A"]) and (a_total is None or want_a == a_total)
    x = rnd(int(g["seed"]) + 1, B, 3, H, W).cuda()
    with torch.no_grad():
        y, second = model(x, augment=True)
    assert second is None and tuple(y.shape) == (B, 24, want_a) and y.dtype == torch.float32
    got = y.cpu()[:, :, g["cols"].long()]
    d = (got - g["y"]).abs()
    err = float(d.max()) / float(g["y"].abs().max())
    b1, b2 = (int(v) for v in g["bounds"])
    cols = g["cols"].long()
    per_pass = [float(d[:, :, m].max()) / float(g["y"].abs().max()) for m in (cols < b1, (cols >= b1) & (cols < b2), cols >= b2)]
    print(f"{name}: max |d| / max |y| = {err:.3e}; per pass {['%.3e' % v for v in per_pass]}")
    assert err <= 1e-4, (err, per_pass)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("yml,H,W", [("yolov8-lowlight.yaml", 128, 128), ("yolov8-p2.yaml", 96, 160)], ids=["ll_128", "p2_96x160"])
def test_model_augment_vs_own_composition(yml, H, W, dtype):
    """model(x, augment=True)[0] against three model(xi) calls on torch-prepared inputs merged with torch.  The class rows of the first
    pass (the same image through the same kernels) are bit-equal; everything else carries the scale_img and division differences of
    the kernel tests through the network: max |d| / max |y| <= 1e-4 in fp32; in bf16 the block-forward bound of
    tests/test_gpu_lowprec.py (relative L2 <= 2e-2: inputs that differ in the last f32 bits round differently to bf16)."""
    import dedark_yolo_amd as dy
    from dedark_yolo_amd.nn.tasks import tta_plan
    dy.set_compute_dtype(dtype)
    model = _model(yml, 2311)
    head = model.model[-1]
    x = rnd(2312, 2, 3, H, W).cuda()
    with torch.no_grad():
        y = model(x, augment=True)[0]
        want = _compose(model, x)
        again = model(x, augment=True)[0]
        single = model(x)[0]
    assert torch.equal(y, again), "two augmented runs differ"
    passes, a_total = tta_plan(H, W, head.strides_as_floats(), head.nl)
    assert tuple(y.shape) == tuple(want.shape) == (2, 24, a_total)
    keep0 = passes[0][8]
    assert torch.equal(y[:, 4:, :keep0], want[:, 4:, :keep0]) and torch.equal(y[:, :, :keep0], single[:, :, :keep0])
    if dtype == torch.float32:
        err = float((y - want).abs().max()) / float(want.abs().max())
        print(f"{yml} {H}x{W} fp32: max |d| / max |y| = {err:.3e}")
        assert err <= 1e-4, err
    else:
        err = float((y.double() - want.double()).norm() / want.double().norm())
        print(f"{yml} {H}x{W} bf16: relative L2 = {err:.3e}")
        assert err <= 2e-2, err


def test_asffdetect_model_augments():
    """AsffDetect takes the same path (yolov8-Faster3.0-ThreeHead.yaml: three ASFF-fused levels; fixed widths, so scale l on a
    small image): against the torch composition."""
    from dedark_yolo_amd.nn.modules import AsffDetect
    from dedark_yolo_amd.nn.tasks import DetectionModel, tta_plan
    cfg = load_yaml("yolov8-Faster3.0-ThreeHead.yaml")
    cfg["scale"] = "l"
    torch.manual_seed(5)
    model = DetectionModel(cfg, nc=20).cuda().eval()
    head = model.model[-1]
    assert isinstance(head, AsffDetect)
    x = rnd(2321, 1, 3, 64, 96).cuda()
    with torch.no_grad():
        y = model(x, augment=True)[0]
        want = _compose(model, x)
    assert tuple(y.shape) == tuple(want.shape) == (1, 24, tta_plan(64, 96, head.strides_as_floats(), 3)[1])
    err = float((y - want).abs().max()) / float(want.abs().max())
    print(f"yolov8-Faster3.0-ThreeHead.yaml@l 64x96: max |d| / max |y| = {err:.3e}")
    assert err <= 1e-4, err


def test_augmented_path_launches_no_plain_decode():
    """Three passes = three dy_detect_decode_tta and two dy_tta_scale_img launches; the plain decode does not run as well."""
    from dedark_yolo_amd import _C
    model = _model("yolov8ori.yaml", 2331)
    x = rnd(2332, 2, 3, 128, 128).cuda()
    with torch.no_grad():
        model(x, augment=True)
        _C._prof = []
        try:
            model(x, augment=True)
            torch.cuda.synchronize()
        finally:
            rec, _C._prof = _C._prof, None
    names = [r[0] for r in rec]
    assert names.count("dy_detect_decode_tta") == 3 and names.count("dy_tta_scale_img") == 2
    assert "dy_detect_decode" not in names and "dy_detect_decode_rows" not in names
    assert "_tta_window" not in model.model[-1].__dict__
    with torch.no_grad():
        assert tuple(model(x)[0].shape) == (2, 24, 336)        # the switch is off again


# ------------------------------------------------------------------------------------------------ 5. engine
def test_nms_at_the_merged_anchor_count_of_a_p2_model():
    """A = 62281 (640 x 640, strides 4..32, three passes): the batched NMS against the oracle, bit-exact."""
    from test_gpu_val import _check_nms, _synthetic_pred
    pred = _synthetic_pred(23, 2, 20, 62281, hot=0.002)
    assert _check_nms(pred, 0.25, 0.7) > 100


def test_yolo_predict_augment():
    """YOLO.predict(x, augment=True): Results boxes = NMS on the merged tensor (scaled / clipped like every prediction)."""
    from dedark_yolo_amd.engine.model import YOLO
    from dedark_yolo_amd.utils import ops as uops
    yolo = YOLO("yolov8nori.yaml")
    yolo.model = _model("yolov8ori.yaml", 2341, confident=True)
    x = rnd(2342, 2, 3, 128, 128).cuda()
    res = yolo.predict(x, conf=0.5, augment=True)
    with torch.no_grad():
        merged = yolo.model(x, augment=True)[0]
    assert merged.shape[-1] == 701
    dets = uops.non_max_suppression((merged, None), 0.5, 0.7, max_det=300)
    plain = yolo.predict(x, conf=0.5)
    assert len(res) == 2 and sum(len(r.boxes) for r in res) > 4
    differs = False
    for r, d, p in zip(res, dets, plain):
        d = d.clone()
        uops.scale_boxes((128, 128), d[:, :4], (128, 128))
        assert torch.equal(r.boxes.data, d[:, :6])
        differs |= r.boxes.data.shape != p.boxes.data.shape or not torch.equal(r.boxes.data, p.boxes.data)
    assert differs, "augment=True returned the single-scale detections"
    assert yolo(x, conf=0.5, augment=True)[0].boxes.data.shape == res[0].boxes.data.shape


class _Composed(torch.nn.Module):
    """A model whose forward is the torch composition of the augmented passes, whatever `augment` says."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.model, self.names = inner, inner.model, inner.names

    def forward(self, x, augment=False):
        return _compose(self.inner, x), None


def test_validator_augment():
    """val(augment=True) on a two-batch loader: the metrics of the manual composition, not those of augment=False; the trainer's own
    validation (training=True) ignores the flag.  The labels are the model's own best single-scale detections, so that the metrics
    are far from zero and move when the predictions do."""
    from dedark_yolo_amd.engine.model import YOLO
    from dedark_yolo_amd.engine.trainer import get_cfg
    from dedark_yolo_amd.engine.validator import DetectionValidator
    from dedark_yolo_amd.utils import ops as uops
    model = _model("yolov8ori.yaml", 2351, confident=True)
    S, B = 128, 3
    gen = np.random.default_rng(2352)
    loader = []
    for _ in range(2):
        img = torch.from_numpy((gen.random((B, 3, S, S)) * 255).astype(np.uint8))
        with torch.no_grad():
            dets = uops.non_max_suppression(model((img.float() / 255).cuda()), 0.25, 0.5, max_det=300)
        bi, cls, bb = [], [], []
        for b, d in enumerate(dets):
            for row in d[:4].cpu():
                x1, y1, x2, y2 = (float(v) for v in row[:4].clamp(0, S))
                bi.append(b)
                cls.append(float(row[5]))
                bb.append([(x1 + x2) / 2 / S, (y1 + y2) / 2 / S, (x2 - x1) / S, (y2 - y1) / S])
        assert len(bi) >= B
        loader.append(dict(img=img, batch_idx=torch.tensor(bi, dtype=torch.float32), cls=torch.tensor(cls, dtype=torch.float32).view(-1, 1),
                           bboxes=torch.tensor(bb, dtype=torch.float32), ori_shape=[(S, S)] * B))
    base = DetectionValidator(get_cfg(dict(conf=0.25, iou=0.7)))(model, loader)
    aug = DetectionValidator(get_cfg(dict(conf=0.25, iou=0.7, augment=True)))(model, loader)
    manual = DetectionValidator(get_cfg(dict(conf=0.25, iou=0.7)))(_Composed(model), loader)
    print("val: single-scale", base, "\n     augment", aug, "\n     manual composition", manual)
    assert base["metrics/mAP50(B)"] > 0.2
    assert set(aug) == set(manual) and all(abs(aug[k] - manual[k]) <= 1e-4 for k in aug), (aug, manual)
    assert any(abs(aug[k] - base[k]) > 1e-3 for k in aug), "augment=True changed nothing"
    trainer_side = DetectionValidator(get_cfg(dict(conf=0.25, iou=0.7, augment=True)))
    trainer_side.training = True
    assert trainer_side(model, loader) == base
    yolo = YOLO("yolov8nori.yaml")
    yolo.model = model
    assert yolo.val(loader, conf=0.25, iou=0.7, augment=True) == aug


# ------------------------------------------------------------------------------------------------ 6. fallback
def _tiny(cls, yaml_name, **kw):
    cfg = load_yaml(yaml_name)
    cfg["scales"]["t"] = list(TINY)
    cfg["scale"] = "t"
    torch.manual_seed(7)
    return cls(cfg, **kw).cuda().eval()


@pytest.mark.parametrize("task", ["segment", "pose", "classify"])
def test_other_tasks_warn_and_run_single_scale(task):
    """reference tasks.py:121-127, 358-363, 381-386: no augmented inference for these models; a warning, the single-scale output."""
    from dedark_yolo_amd.nn import tasks
    model = {"segment": lambda: _tiny(tasks.SegmentationModel, "yolov8-seg.yaml", nc=20),
             "pose": lambda: _tiny(tasks.PoseModel, "yolov8-pose.yaml", nc=1),
             "classify": lambda: _tiny(tasks.ClassificationModel, "cls/yolov8-cls.yaml", nc=10)}[task]()
    x = rnd(2361, 2, 3, 64, 64).cuda()
    with torch.no_grad():
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            plain = model(x)
        assert not any("single-scale" in str(w.message) for w in seen)      # the plain call does not warn
        with pytest.warns(UserWarning, match="single-scale"):
            aug = model(x, augment=True)
    first = (lambda o: o[0] if isinstance(o, (tuple, list)) else o)
    assert torch.equal(first(aug), first(plain)) and first(aug).shape[0] == 2
    if task != "classify":
        assert aug[1] is not None                              # the task's own second output, not the detect path's None
