"""GPU tests of segment inference at image resolution: dy_seg_mask_upsample through process_mask(upsample=True),
process_mask_upsample, process_mask_native and process_masks_batched, dy_mask_resize through scale_masks and resize_masks, the
segment validator with gt masks at another resolution and with process_mask_upsample, and YOLO.predict on a segment model, against
the reference's own outputs (tests/golden/make_segpredict_golden.py).

The `unsure` rule: a golden mask comes with the packed set of pixels whose value before the threshold lies within 1e-4 of 0.5.  A
different summation order of the 32-term dot product moves the logit by about 1e-6 relative, the sigmoid by a few 1e-7, and two
bilinear implementations differ by a few ulp more; 1e-4 is two orders above that.  At most 0.1 % of a case's pixels may be unsure
(asserted when the golden is written and again here); every other pixel must be equal."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import gold, load_yaml, make_batch

pytestmark = pytest.mark.gpu

TINY = [0.33, 0.125, 1024]
MARGIN, CAP = 1e-4, 1e-3


@pytest.fixture(autouse=True)
def _fp32():
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(torch.float32)
    yield
    dy.set_compute_dtype(torch.float32)


def unpack(bits, shape):
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(np.asarray(bits))[:n].astype(bool)).view(*shape)


def assert_mask(got, want_bits, unsure_bits, shape, what):
    got = got.cpu()
    assert tuple(got.shape) == tuple(shape), (what, tuple(got.shape), tuple(shape))
    want, unsure = unpack(want_bits, shape), unpack(unsure_bits, shape)
    share = float(unsure.float().mean())
    print(f"{what}: unsure share {share:.3e}, differing pixels {int((got.bool() != want).sum())}")
    assert share <= CAP, (what, share)
    assert want.any(), what
    assert torch.equal(got.bool()[~unsure], want[~unsure]), (what, int((got.bool() != want)[~unsure].sum()))


def dets_of(boxes, coef):
    d = torch.zeros((boxes.shape[0], 38))
    d[:, :4], d[:, 6:] = boxes, coef
    return d.cuda()


MODES = {"input": lambda u, *a: u.process_mask(*a, upsample=True), "upsample": lambda u, *a: u.process_mask_upsample(*a)}


@pytest.mark.parametrize("mode", ["input", "upsample"])
@pytest.mark.parametrize("tag", ["a", "b", "c"], ids=["40x40-160x160", "24x40-96x160", "40x40-100x150"])
def test_upsampled_masks_vs_reference(tag, mode):
    """process_mask(upsample=True) and process_mask_upsample against the reference's (boxes on exact pixel edges, one leaving the
    image, one empty), and the same bytes from process_masks_batched."""
    from dedark_yolo_amd.utils import ops as uops
    g = gold("g18_maskup")
    proto, coef, boxes = g[tag + "_proto"].cuda(), g[tag + "_coef"].cuda(), g[tag + "_boxes"].cuda()
    shape = tuple(int(v) for v in g[tag + "_shape"])
    got = MODES[mode](uops, proto, coef, boxes, shape)
    assert got.dtype == torch.float32 and set(got.unique().tolist()) <= {0.0, 1.0}
    assert_mask(got, g[f"{tag}_{mode}_mask"], g[f"{tag}_{mode}_unsure"], (12, *shape), f"{tag} {mode}")
    assert float(got[2].sum()) == 0.0                                     # the empty box
    b = uops.process_masks_batched(proto[None], [dets_of(g[tag + "_boxes"], g[tag + "_coef"])], shape, mode=mode)[0]
    assert b.dtype == torch.uint8 and torch.equal(b, got.to(torch.uint8))


@pytest.mark.parametrize("tag", ["n0", "n1", "n2"], ids=["211x317", "230x310", "300x180"])
def test_native_masks_vs_reference(tag):
    """process_mask_native (scale_masks' padding crop, then a resize to the original image, horizontal and vertical crops)."""
    from dedark_yolo_amd.utils import ops as uops
    g = gold("g18_maskup")
    shape = tuple(int(v) for v in g[tag + "_shape"])
    got = uops.process_mask_native(g["a_proto"].cuda(), g[tag + "_coef"].cuda(), g[tag + "_boxes"].cuda(), shape)
    assert got.dtype == torch.float32
    assert_mask(got, g[tag + "_mask"], g[tag + "_unsure"], (12, *shape), f"native {shape}")


def test_batched_native_with_one_shape_per_image_equals_the_per_image_calls():
    """four images (one without detections, two of equal original shape) through one process_masks_batched call: the bytes of the
    per-image functions, one launch per distinct shape; the two runs are identical."""
    from dedark_yolo_amd import _C
    from dedark_yolo_amd.utils import ops as uops
    g = gold("g18_maskup")
    proto = torch.stack([g["a_proto"], g["c_proto"], g["a_proto"].flip(0), g["c_proto"].flip(1)]).cuda()
    tags, shapes = ["n0", "n1", None, "n0"], [(211, 317), (230, 310), (64, 64), (211, 317)]
    dets = [dets_of(g[t + "_boxes"], g[t + "_coef"]) if t else torch.zeros((0, 38), device="cuda") for t in tags]
    calls = []
    real = _C.call
    uops.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        out = uops.process_masks_batched(proto, dets, (160, 160), mode="native", out_shapes=shapes)
    finally:
        uops.call = real
    assert calls.count("dy_seg_mask_upsample") == 2, calls
    again = uops.process_masks_batched(proto, dets, (160, 160), mode="native", out_shapes=shapes)
    for i, (t, shape) in enumerate(zip(tags, shapes)):
        assert out[i].dtype == torch.uint8 and tuple(out[i].shape) == ((12 if t else 0), *shape)
        assert torch.equal(out[i], again[i])
        if t:
            one = uops.process_mask_native(proto[i], g[t + "_coef"].cuda(), g[t + "_boxes"].cuda(), shape)
            assert torch.equal(out[i], one.to(torch.uint8)), i
    assert_mask(out[0], g["n0_mask"], g["n0_unsure"], (12, 211, 317), "batched native image 0")


def restate(mode, proto, coef, boxes, shape, window=None):
    """the reference's formulas in torch, f32 on the CPU: the value before the threshold"""
    c, mh, mw = proto.shape
    m = (coef @ proto.view(c, -1)).sigmoid().view(-1, mh, mw)

    def crop(x, b):
        h, w = x.shape[1:]
        r = torch.arange(w, dtype=torch.float32)[None, None, :]
        q = torch.arange(h, dtype=torch.float32)[None, :, None]
        x1, y1, x2, y2 = (b[:, i, None, None] for i in range(4))
        return x * ((r >= x1) * (r < x2) * (q >= y1) * (q < y2))
    if mode == "input":
        b = boxes.clone()
        b[:, [0, 2]] *= mw / shape[1]
        b[:, [1, 3]] *= mh / shape[0]
        return F.interpolate(crop(m, b)[None], shape, mode="bilinear", align_corners=False)[0]
    if mode == "native":
        top, left, bottom, right = window
        m = m[:, top:bottom, left:right]
    return crop(F.interpolate(m[None], shape, mode="bilinear", align_corners=False)[0], boxes)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("mode", ["input", "upsample", "native"])
def test_low_precision_protos(mode, dtype):
    """bf16 / f16 protos: the kernel reads the 16-bit proto and computes in f32, so it must agree with the restatement run on the
    same rounded proto in f32, under the unsure rule computed from the restatement's own value."""
    from dedark_yolo_amd.utils import ops as uops
    g = gold("g18_maskup")
    gen = np.random.default_rng(77)
    proto = (g["c_proto"] + torch.from_numpy(gen.normal(0, 0.01, (32, 40, 40)).astype(np.float32))).to(dtype)
    shape = (211, 317) if mode == "native" else (100, 150)
    tag = "n0" if mode == "native" else "c"
    coef, boxes = g[tag + "_coef"], g[tag + "_boxes"]
    v = restate(mode, proto.float(), coef, boxes, shape, uops.scale_masks_window(40, 40, shape))
    unsure = (v - 0.5).abs() < MARGIN
    share = float(unsure.float().mean())
    p = proto.cuda()[None].contiguous(memory_format=torch.channels_last)
    got = uops.process_masks_batched(p, [dets_of(boxes, coef)], shape, mode=mode, out_shapes=[shape])[0].cpu()
    print(f"{mode} {dtype}: unsure share {share:.3e}, differing pixels {int((got.bool() != (v > 0.5)).sum())}")
    assert share <= CAP, share
    assert (v > 0.5).any() and torch.equal(got.bool()[~unsure], (v > 0.5)[~unsure])
    again = uops.process_masks_batched(p, [dets_of(boxes, coef)], shape, mode=mode, out_shapes=[shape])[0].cpu()
    assert torch.equal(got, again)


@pytest.mark.parametrize("mode,shape", [("input", (25, 30)), ("upsample", (25, 30)), ("native", (30, 22)), ("upsample", (9, 250))],
                         ids=["input-25x30", "upsample-25x30", "native-30x22", "upsample-9x250"])
def test_masks_smaller_than_the_proto(mode, shape):
    """an output smaller than the 40 x 40 proto in one or both axes (a small original image): the launcher shrinks its output tile
    until the proto pixels under it fit; against the restatement under the unsure rule."""
    from dedark_yolo_amd.utils import ops as uops
    g = gold("g18_maskup")
    proto, coef = g["c_proto"], g["c_coef"]
    boxes = g["c_boxes"] * torch.tensor([shape[1] / 150, shape[0] / 100, shape[1] / 150, shape[0] / 100])
    v = restate(mode, proto, coef, boxes, shape, uops.scale_masks_window(40, 40, shape))
    unsure = (v - 0.5).abs() < MARGIN
    share = float(unsure.float().mean())
    got = uops.process_masks_batched(proto.cuda()[None], [dets_of(boxes, coef)], shape, mode=mode, out_shapes=[shape])[0].cpu()
    print(f"{mode} -> {shape}: unsure share {share:.3e}, differing pixels {int((got.bool() != (v > 0.5)).sum())}")
    assert share <= CAP, share
    assert (v > 0.5).any() and torch.equal(got.bool()[~unsure], (v > 0.5)[~unsure])


def test_many_detections_split_into_chunks_give_the_same_bytes():
    """300 detections of one image are walked by several workgroups per tile (det_chunk); row j must not depend on the split."""
    from dedark_yolo_amd.utils import ops as uops
    g = gold("g18_maskup")
    gen = np.random.default_rng(78)
    coef = torch.from_numpy(gen.normal(0, 0.6, (300, 32)).astype(np.float32))
    xy = gen.uniform(0, 110, (300, 2))
    boxes = torch.from_numpy(np.concatenate([xy, xy + gen.uniform(5, 60, (300, 2))], 1).astype(np.float32))
    p = g["a_proto"].cuda()[None]
    full = uops.process_masks_batched(p, [dets_of(boxes, coef)], (160, 160), mode="upsample")[0]
    assert tuple(full.shape) == (300, 160, 160) and full.any()
    for lo, hi in ((0, 7), (120, 131), (293, 300)):
        part = uops.process_masks_batched(p, [dets_of(boxes[lo:hi], coef[lo:hi])], (160, 160), mode="upsample")[0]
        assert torch.equal(part, full[lo:hi]), (lo, hi)


def test_scale_masks_vs_reference():
    """scale_masks on f32 planes (padding crop both ways, two shapes): atol 1e-5."""
    from dedark_yolo_amd.utils import ops as uops
    g = gold("g18_scalemasks")
    x = g["sm_in"].cuda()
    for si in (0, 1):
        for padding in (True, False):
            k = f"sm{si}_{int(padding)}"
            shape = tuple(int(v) for v in g[k + "_shape"])
            got = uops.scale_masks(x, shape, padding=padding)
            assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, *shape)
            err = float((got.cpu() - g[k]).abs().max())
            print(f"scale_masks {k}: max abs err {err:.3e}")
            assert err <= 1e-5, (k, err)


@pytest.mark.parametrize("tag", ["down", "up", "odd"], ids=["160-40", "40-160", "160-96"])
def test_gt_mask_resize_vs_reference(tag):
    """the gt side of the segment validator: a 5-label index map (uint8 and int32) and the same labels as planes (uint8 and f32)
    resized bilinearly and thresholded.  Power-of-two ratios on 0 / 1 inputs are exact in f32: bit-equal with nothing excluded (a
    value of exactly 0.5 must come out 0).  160 -> 96 under the unsure rule."""
    from dedark_yolo_amd.utils import ops as uops
    g = gold("g18_gtresize")
    idx = g[tag + "_idx"]
    out = tuple(int(v) for v in g[tag + "_out"])
    want = unpack(g[tag + "_mask"], (5, *out))
    sure = ~unpack(g["odd_unsure"], (5, *out)) if tag == "odd" else torch.ones_like(want)
    assert float((~sure).float().mean()) <= 2e-4 and want.any()
    planes = torch.stack([(idx == k + 1).to(torch.uint8) for k in range(5)])
    srcs = dict(map_u8=(idx.cuda(), 5), map_i32=(idx.to(torch.int32).cuda(), 5), planes_u8=(planes.cuda(), None),
                planes_f32=(planes.float().cuda(), None))
    for name, (src, m) in srcs.items():
        got = uops.resize_masks(src, out, m=m)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (5, *out)
        assert torch.equal(got.cpu().bool()[sure], want[sure]), name
    v = uops.resize_masks(planes.cuda(), out, binary=False)
    assert v.dtype == torch.float32 and torch.equal((v > 0.5).cpu()[sure], want[sure])
    if tag == "down":
        assert bool((v == 0.5).any())                                      # exact halves occur and are not kept


def _validator(nc, **over):
    from dedark_yolo_amd.engine.trainer import get_cfg
    from dedark_yolo_amd.engine.validator import SegmentationValidator
    v = SegmentationValidator(get_cfg(over))
    v.device = torch.device("cuda")
    v.init_metrics(SimpleNamespace(model=[SimpleNamespace(nc=nc)], names={i: str(i) for i in range(nc)}))
    return v


def _val_batch(g, tag, planes):
    S = int(g["S"])
    counts = [int(v) for v in g[tag + "_pred_counts"]]
    preds = [p.cuda() for p in g[tag + "_preds"].split(counts, 0)]
    idx = g[tag + "_gt_idx"]
    bi = g[tag + "_batch_idx"]
    if planes:
        nb = [int((bi == b).sum()) for b in range(len(counts))]
        masks = torch.cat([torch.stack([(idx[b] == k + 1).to(torch.uint8) for k in range(n)]) for b, n in enumerate(nb)])
    else:
        masks = idx
    rp = g["ratio_pad"].tolist()
    batch = dict(img=torch.zeros(len(counts), 3, S, S, device="cuda"), batch_idx=bi, cls=g[tag + "_cls"], bboxes=g[tag + "_bboxes"],
                 masks=masks, ori_shape=[tuple(int(v) for v in o) for o in g["ori_shape"].tolist()],
                 ratio_pad=[((r[0][0], r[0][1]), (r[1][0], r[1][1])) for r in rp])
    return preds, g[tag + "_proto"].cuda(), batch, counts


@pytest.mark.parametrize("tag", ["a", "b", "c"], ids=["gt128-map", "upsample-gt32-map", "gt128-planes"])
def test_segment_validator_end_to_end_vs_reference(tag):
    """SegmentationValidator.update_metrics + get_stats against the reference validator's on the same fixed NMS outputs, protos and
    batch: (a) gt index maps at 128x128 against process_mask masks at 32x32, (b) save_json -> process_mask_upsample masks at 128x128
    against gt index maps at 32x32, (c) gt planes at 128x128 (overlap_mask False).  The golden script keeps every class-matched
    mask IoU at least 1e-3 away from the ten thresholds, so the `correct` matrices must be equal."""
    g = gold("g18_val_e2e")
    preds, proto, batch, counts = _val_batch(g, tag, planes=tag == "c")
    assert 0 in counts
    v = _validator(int(g["nc"]), save_json=tag == "b", overlap_mask=tag != "c")
    v.update_metrics((preds, proto), batch)
    assert v.seen == int(g[tag + "_seen"])
    stats = [torch.cat(x, 0) for x in zip(*v.stats)]
    assert torch.equal(stats[0], g[tag + "_correct_b"])
    assert torch.equal(stats[1], g[tag + "_correct_m"]), int((stats[1] != g[tag + "_correct_m"]).sum())
    assert g[tag + "_correct_m"].any() and not g[tag + "_correct_m"].all()
    for got, want in zip(stats[2:], (g[tag + "_conf"], g[tag + "_pcls"], g[tag + "_tcls"])):
        assert torch.equal(got.float(), want.float())
    rd = v.get_stats()
    assert list(rd) == [str(k) for k in g[tag + "_metric_keys"]]
    np.testing.assert_allclose(np.array(list(rd.values())), g[tag + "_metric_values"].numpy(), rtol=1e-9, atol=1e-12)


def test_segment_validator_at_the_predicted_resolution_is_the_direct_path():
    """gt masks already at the predicted resolution: the mask `correct` matrices are those of the direct calls
    (process_masks_batched at the proto resolution -> mask_iou_binary on the index map -> match_from_iou), no resize in between."""
    from dedark_yolo_amd import _C
    from dedark_yolo_amd.engine.validator import match_from_iou
    from dedark_yolo_amd.utils import ops as uops
    g = gold("g18_val_e2e")
    preds, proto, batch, counts = _val_batch(g, "b", planes=False)          # gt index maps at 32 x 32 = the proto resolution
    v = _validator(int(g["nc"]))
    calls = []
    real = _C.call
    uops.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        v.update_metrics((preds, proto), batch)
    finally:
        uops.call = real
    assert "dy_mask_resize" not in calls and "dy_seg_mask_upsample" not in calls and "dy_seg_mask_decode" in calls
    pm = uops.process_masks_batched(proto, preds, (128, 128))
    rows = iter(v.stats)
    bi, cls = batch["batch_idx"], batch["cls"]
    for b, n in enumerate(counts):
        if n == 0:
            next(rows)
            continue
        lab = cls[bi == b].view(-1)
        iou = uops.mask_iou_binary(batch["masks"][b].cuda(), pm[b], True, len(lab)).cpu().numpy()
        want = match_from_iou(iou, lab, preds[b][:, 5].cpu(), v.iouv)
        assert torch.equal(next(rows)[1], want), b


def _seg_model(seed, nc=20):
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn.tasks import SegmentationModel
    cfg = load_yaml("yolov8-seg.yaml")
    cfg["scales"]["t"] = TINY
    cfg["scale"] = "t"
    model = SegmentationModel(cfg, nc=nc)
    load_sd(model, om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed))
    return model.cuda()


def test_predict_of_a_segment_model():
    """YOLO(tiny seg).predict on fixed weights: masks at the input shape (default; zero outside the box grown by one proto pixel,
    since the crop happens before the resize) or at orig_shapes[i] (retina_masks; zero outside the scaled box), None for the image
    without detections."""
    from dedark_yolo_amd.engine.model import YOLO
    y = YOLO("yolov8n-seg.yaml")
    y.model = _seg_model(1611)
    # (rng_fill weights make the scores almost independent of the image: a stronger stem and class branch spread them enough for the
    # two images' best scores to differ by about 5e-5, far above f32 noise)
    y.model.model[0].conv.weight.data *= 10.0
    for conv in y.model.model[-1].cv3:
        conv[2].weight.data *= 3.0
    img = make_batch(1612, 2, 128, [3, 2])["img"].pow(3.0).cuda()
    y.model.eval()
    with torch.no_grad():
        pred = y.model(img)[0]
    top = pred[:, 4:24].amax((1, 2)).cpu()
    assert abs(float(top[0]) - float(top[1])) > 1e-5, top
    conf = float(top.min() + top.max()) / 2                                 # one image keeps detections, the other none
    full, empty = int(top.argmax()), int(top.argmin())
    res = y.predict(img, conf=conf)
    assert res[empty].masks is None and len(res[empty].boxes) == 0
    r = res[full]
    n = len(r.boxes)
    assert n > 0 and r.masks is not None and tuple(r.masks.data.shape) == (n, 128, 128) and r.masks.data.dtype == torch.float32
    print(f"predict: conf {conf:.4f}, {n} detections, mask pixels on {r.masks.data.sum((1, 2)).tolist()}")
    assert r.masks.orig_shape == (128, 128) and float(r.masks.data.sum()) > 0
    yy, xx = torch.meshgrid(torch.arange(128.0), torch.arange(128.0), indexing="ij")
    for box, m in zip(r.boxes.xyxy.cpu(), r.masks.data.cpu()):
        inside = (xx >= box[0] - 4) & (xx < box[2] + 4) & (yy >= box[1] - 4) & (yy < box[3] + 4)
        assert float(m[~inside].sum()) == 0.0
    shapes = [(256, 192), (200, 300)]
    res = y.predict(img, conf=conf, orig_shapes=shapes, retina_masks=True)
    assert res[empty].masks is None
    r = res[full]
    H, W = shapes[full]
    assert tuple(r.masks.data.shape) == (n, H, W) and r.masks.orig_shape == (H, W) and float(r.masks.data.sum()) > 0
    yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
    for box, m in zip(r.boxes.xyxy.cpu(), r.masks.data.cpu()):
        inside = (xx >= box[0]) & (xx < box[2]) & (yy >= box[1]) & (yy < box[3])
        assert float(m[~inside].sum()) == 0.0
    res = y.predict(img, conf=conf, orig_shapes=shapes)                     # default: masks stay at the input shape, boxes are scaled
    assert tuple(res[full].masks.data.shape) == (n, 128, 128) and res[full].orig_shape == shapes[full]
    # a lower threshold: many detections in both images, every mask inside its scaled box
    res = y.predict(img, conf=float(top.min()) - 0.03, orig_shapes=shapes, retina_masks=True)
    assert min(len(r.boxes) for r in res) > 1
    for r, (H, W) in zip(res, shapes):
        assert tuple(r.masks.data.shape) == (len(r.boxes), H, W)
        yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
        for box, m in zip(r.boxes.xyxy.cpu(), r.masks.data.cpu()):
            assert float(m[~((xx >= box[0]) & (xx < box[2]) & (yy >= box[1]) & (yy < box[3]))].sum()) == 0.0


@pytest.mark.parametrize("retina", [False, True], ids=["input", "retina"])
def test_segment_postprocess_vs_reference_predictor(retina):
    """the half of predict() after the NMS on the reference predictor's fixed NMS outputs: boxes and masks of
    SegmentationPredictor.postprocess, retina_masks both ways, original shapes that differ from the 128 x 128 input."""
    from dedark_yolo_amd.engine.model import segment_postprocess
    g = gold("g18_predict")
    counts = [int(v) for v in g["pred_counts"]]
    preds = [p.cuda() for p in g["preds"].split(counts, 0)]
    ori = [tuple(int(v) for v in o) for o in g["ori_shape"].tolist()]
    S = int(g["S"])
    res = segment_postprocess(preds, g["proto"].cuda(), (S, S), ori, retina_masks=retina, names={i: str(i) for i in range(int(g["nc"]))})
    assert len(res) == len(counts) and 0 in counts
    for i, r in enumerate(res):
        k = f"r{int(retina)}_{i}_"
        assert r.orig_shape == ori[i]
        assert torch.allclose(r.boxes.data.cpu(), g[k + "boxes"], rtol=0, atol=1e-4), i
        if counts[i] == 0:
            assert r.masks is None
            continue
        shape = tuple(int(v) for v in g[k + "mask_shape"])
        assert shape[1:] == (ori[i] if retina else (S, S))
        assert_mask(r.masks.data, g[k + "mask"], g[k + "unsure"], shape, f"predict retina={retina} image {i}")
