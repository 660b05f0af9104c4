"""GPU tests of the segment task: the Proto's ConvTranspose2d(k=2, s=2) on the conv kernels against torch in float64, the mask loss
(csrc/seg.hip through the C-ABI, via v8SegmentationLoss) against an in-test float64 restatement of the reference's
v8SegmentationLoss on the kernel's own assignment, the Proto block and a whole tiny segmentation model against the reference's
fixtures (tests/golden/make_seg_golden.py), and trainer steps / save / resume on a tiny segmentation model."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import close, gold, load_yaml, make_batch, rnd

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
TINY = [0.33, 0.125, 1024]
STRIDES = (8.0, 16.0, 32.0)


@pytest.fixture(autouse=True)
def _fp32():
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(torch.float32)
    yield
    dy.set_compute_dtype(torch.float32)


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


# ---------------------------------------------------------------------------------------------------- ConvTranspose2d(2, 2)
CONVT = [(1, 64, 64, 20, 20), (1, 256, 256, 80, 80), (2, 20, 36, 9, 7), (2, 36, 20, 5, 11)]


DGRAD_ROUTES = ("v4::conv_kernel", "v5::conv_kernel<", "v5::band_kernel<", "v2::conv_kernel<", "conv_thin_kernel", "conv_igemm_kernel<")


def _convt_case(shape):
    B, c1, c2, H, W = shape
    seed = sum(shape)
    x = rnd(seed, B, c1, H, W, lo=-1, hi=1)
    w = (rnd(seed + 1, c1, c2, 2, 2, lo=-1, hi=1) / c1 ** 0.5).double()
    b = rnd(seed + 2, c2, lo=-1, hi=1).double()
    gy = rnd(seed + 3, B, c2, 2 * H, 2 * W, lo=-1, hi=1)
    return x, w, b, gy


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", CONVT, ids=["64-64@20", "256-256@80", "20-36@9x7", "36-20@5x11"])
def test_conv_transpose_vs_torch(shape, dtype):
    """forward (dy_conv2d_dgrad route + dy_bias_add), data gradient (dy_conv2d_fwd), weight gradient (dy_conv2d_wgrad) and bias
    gradient (dy_bias_grad) of ConvTranspose2d(c1, c2, 2, 2) against F.conv_transpose2d + autograd in float64 on the same
    (dtype-rounded) inputs: relative L2 <= 1e-5 (f32) / 1e-2 (16-bit)."""
    from dedark_yolo_amd import _C, ops
    from dedark_yolo_amd.nn.modules import Tape
    ops.set_compute_dtype(dtype)
    x, w, b, gy = _convt_case(shape)
    xq, gq = x.to(dtype), gy.to(dtype)
    xr = xq.double().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y_ref = F.conv_transpose2d(xr, wr, br, stride=2)
    y_ref.backward(gq.double())
    W32 = torch.nn.Parameter(w.float().cuda())
    B32 = torch.nn.Parameter(b.float().cuda())
    xd = ops.as_nhwc(xq.cuda(), dtype)
    tape = Tape()
    lib = _C.lib()
    lib.dy_clear_last_kernel()
    y0 = ops.conv_transpose2x2_forward(None, xd, W32, None)
    route = lib.dy_last_kernel().decode()
    # the forward is the data gradient of the 2x2 / stride-2 conv: one of the conv kernels that take the parity-class descriptors
    # (none of them gets a shift: the bias is always the separate dy_bias_add pass, so any of these routes is correct)
    assert route.startswith(DGRAD_ROUTES), route
    y = ops.conv_transpose2x2_forward(tape, xd, W32, B32)
    assert lib.dy_last_kernel().decode() == "seg_bias_add_kernel"
    dx = ops.conv_transpose2x2_backward(tape, ops.as_nhwc(gq.cuda(), dtype))
    torch.cuda.synchronize()
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert tuple(y.shape) == tuple(y_ref.shape) and y.dtype == dtype
    assert _rel_l2(y.float(), y_ref) <= tol, ("y", _rel_l2(y.float(), y_ref))
    assert _rel_l2(y0.float(), y_ref - br.detach().view(1, -1, 1, 1)) <= tol
    assert _rel_l2(dx.float(), xr.grad) <= tol, ("dx", _rel_l2(dx.float(), xr.grad))
    assert _rel_l2(tape.pgrads[W32], wr.grad) <= tol, ("dW", _rel_l2(tape.pgrads[W32], wr.grad))
    assert _rel_l2(tape.pgrads[B32], br.grad) <= tol, ("db", _rel_l2(tape.pgrads[B32], br.grad))
    c2 = shape[2]
    cp = ops.round_up(c2, ops.vec_elems(dtype))
    if cp != c2:                                   # the padding lanes stay zero: the next conv reads them
        full = torch.as_strided(y, (y.shape[0], cp, y.shape[2], y.shape[3]), y.stride(), y.storage_offset())
        assert float(full[:, c2:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- mask loss
def _box_masks(batch, B, h, w, overlap):
    """gt masks from the boxes: overlap -> [B, h, w] index map (gt k of an image paints k + 1, later on top); else one plane per gt"""
    bis = batch["batch_idx"].long().tolist()
    planes, idx = [], torch.zeros((B, h, w), dtype=torch.uint8)
    k = [0] * B
    for bi, (cx, cy, bw, bh) in zip(bis, batch["bboxes"].tolist()):
        k[bi] += 1
        x1, x2 = int(round((cx - bw / 2) * w)), int(round((cx + bw / 2) * w))
        y1, y2 = int(round((cy - bh * 0.3) * h)), int(round((cy + bh / 2) * h))        # not the box: pixels inside the crop are 0 too
        pl = torch.zeros((h, w), dtype=torch.uint8)
        pl[max(y1, 0):max(y2, 0), max(x1, 0):max(x2, 0)] = 1
        planes.append(pl)
        idx[bi][pl.bool()] = k[bi]
    if overlap:
        return idx
    return torch.stack(planes) if planes else torch.zeros((0, h, w), dtype=torch.uint8)


def _seg_ref(mc, proto, fg, tgi, tbox, masks, overlap, batch_idx, img_hw, hyp_box):
    """float64 restatement of v8SegmentationLoss's mask term (reference loss.py:252-288, crop_mask ops.py:553-569) on the given
    assignment; returns hyp_box / B * sum_i mean_p l_p.  mc [B, nm, A], proto [B, nm, mh, mw] (float64 leaves)."""
    B, nm, mh, mw = proto.shape
    masks = masks.float()
    if tuple(masks.shape[-2:]) != (mh, mw):
        masks = F.interpolate(masks[None], (mh, mw), mode="nearest")[0]
    H, W = img_hw
    tot = proto.sum() * 0
    for i in range(B):
        f = fg[i]
        if not bool(f.any()):
            continue
        idx = tgi[i][f]
        if overlap:
            gt = (masks[[i]] == (idx + 1).view(-1, 1, 1).float()).double()
        else:
            gt = masks[batch_idx == i][idx].double()
        xyxyn = tbox[i][f].float() / torch.tensor([W, H, W, H], dtype=torch.float32)
        area = ((xyxyn[:, 2] - xyxyn[:, 0]) * (xyxyn[:, 3] - xyxyn[:, 1])).double()
        mxyxy = xyxyn * torch.tensor([mw, mh, mw, mh], dtype=torch.float32)
        x1, y1, x2, y2 = [mxyxy[:, j].view(-1, 1, 1) for j in range(4)]
        r = torch.arange(mw, dtype=torch.float32).view(1, 1, -1)
        c = torch.arange(mh, dtype=torch.float32).view(1, -1, 1)
        crop = ((r >= x1) & (r < x2) & (c >= y1) & (c < y2)).double()
        z = torch.einsum("pn,nhw->phw", mc[i][:, f].t(), proto[i])
        lp = F.binary_cross_entropy_with_logits(z, gt, reduction="none")
        tot = tot + ((lp * crop).mean((1, 2)) / area).mean()
    return tot * (hyp_box / B)


def _crit(nc, overlap):
    from types import SimpleNamespace
    from dedark_yolo_amd.utils.loss import v8SegmentationLoss
    head = SimpleNamespace(stride=torch.tensor(STRIDES), nc=nc, no=64 + nc, reg_max=16, nm=32)
    holder = SimpleNamespace(args=SimpleNamespace(box=7.5, cls=0.5, dfl=1.5, overlap_mask=overlap), model=[head],
                             parameters=lambda: iter([torch.zeros(1, device="cuda")]))
    return v8SegmentationLoss(holder)


def _seg_inputs(seed, B, S, nbox, nc, dtype, mask_scale=1, overlap=True):
    gen = np.random.default_rng(seed)
    maps = [torch.from_numpy(gen.normal(0, 1.0, (B, 64 + nc, S // int(s), S // int(s))).astype(np.float32)).to(dtype) for s in STRIDES]
    A = sum(m.shape[2] * m.shape[3] for m in maps)
    mc = torch.from_numpy(gen.normal(0, 0.5, (B, 32, A)).astype(np.float32)).to(dtype)
    proto = torch.from_numpy(gen.normal(0, 1.0, (B, 32, S // 4, S // 4)).astype(np.float32)).to(dtype)
    batch = make_batch(seed + 1, B, S, nbox, nc)
    batch["masks"] = _box_masks(batch, B, mask_scale * S // 4, mask_scale * S // 4, overlap)
    return maps, mc, proto, batch


def _run_seg(maps, mc, proto, batch, nc, overlap, dtype):
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(dtype)
    crit = _crit(nc, overlap)
    gm = [m.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for m in maps]
    gmc = mc.cuda().requires_grad_(True)
    gp = proto.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    loss, items = crit((gm, gmc, gp), dict(batch))
    loss.backward()
    torch.cuda.synchronize()
    return crit, loss, items, gm, gmc, gp


SEG_CASES = {"overlap": dict(nbox=[3, 2], overlap=True), "per_instance": dict(nbox=[2, 4], overlap=False),
             "masks_2x": dict(nbox=[3, 2], overlap=True, mask_scale=2), "per_instance_2x": dict(nbox=[1, 3], overlap=False, mask_scale=2),
             "image_without_labels": dict(nbox=[3, 0], overlap=True), "no_positives": dict(nbox=[0, 0], overlap=True),
             "no_positives_per_instance": dict(nbox=[0, 0], overlap=False)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", list(SEG_CASES))
def test_mask_loss_vs_float64_restatement(case, dtype):
    """items [box, seg, cls, dfl], the total, d mc, d proto and d maps of v8SegmentationLoss against the detection criterion (box /
    cls / dfl terms and map gradients, same kernels: equal) and a float64 restatement of the reference's mask loop on the kernel's
    own assignment (seg item, d mc, d proto)."""
    from dedark_yolo_amd.utils.loss import RcoveryDetectionLoss
    from types import SimpleNamespace
    kw = SEG_CASES[case]
    nc, B, S = 20, 2, 128
    maps, mc, proto, batch = _seg_inputs(61 + len(case), B, S, kw["nbox"], nc, dtype, kw.get("mask_scale", 1), kw["overlap"])
    crit, loss, items, gm, gmc, gp = _run_seg(maps, mc, proto, batch, nc, kw["overlap"], dtype)
    a = crit.last_assignment
    fg, tgi, tbox = a.fg_mask.cpu().bool(), a.target_gt_idx.cpu().long(), a.target_box.cpu()
    if case.startswith("no_positives"):
        assert not bool(fg.any())
    elif case == "image_without_labels":
        assert bool(fg[0].any()) and not bool(fg[1].any())
    else:
        assert bool(fg.any(1).all())
    # detection terms: the detection criterion's kernels on the same maps
    head = SimpleNamespace(stride=torch.tensor(STRIDES), nc=nc, no=64 + nc, reg_max=16)
    dcrit = RcoveryDetectionLoss(SimpleNamespace(args=SimpleNamespace(box=7.5, cls=0.5, dfl=1.5, lrl=2.0), model=[head],
                                                 parameters=lambda: iter([torch.zeros(1, device="cuda")])))
    dm = [m.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for m in maps]
    dl, di = dcrit(dm, {k: v for k, v in batch.items() if k != "masks"})
    dl.backward()
    torch.cuda.synchronize()
    assert torch.equal(items[[0, 2, 3]].cpu(), di.cpu())
    for g1, g2 in zip(gm, dm):
        assert torch.equal(g1.grad.cpu(), g2.grad.cpu())
    # mask term in float64
    mc64 = mc.double().requires_grad_(True)
    p64 = proto.double().requires_grad_(True)
    want = _seg_ref(mc64, p64, fg, tgi, tbox, batch["masks"], kw["overlap"], batch["batch_idx"].long(), (S, S), 7.5)
    (want * B).backward()
    seg = float(items[1])
    want = want.detach()
    rt = 1e-4 if dtype == torch.float32 else 2e-3
    assert abs(seg - float(want)) <= rt * abs(float(want)) + 1e-7, (seg, float(want))
    assert abs(float(loss) - (float(dl) + seg * B)) <= 1e-5 * abs(float(loss)) + 1e-6
    assert gmc.grad.dtype == dtype and gp.grad.dtype == dtype
    if case.startswith("no_positives"):
        assert float(items[1]) == 0.0 and float(gmc.grad.abs().max()) == 0.0 and float(gp.grad.abs().max()) == 0.0
        return
    gt = 1e-4 if dtype == torch.float32 else 1e-2
    assert _rel_l2(gmc.grad.float(), mc64.grad) <= gt, ("d mc", _rel_l2(gmc.grad.float(), mc64.grad))
    assert _rel_l2(gp.grad.float(), p64.grad) <= gt, ("d proto", _rel_l2(gp.grad.float(), p64.grad))
    nonpos = ~fg
    assert float(gmc.grad.float().cpu().permute(0, 2, 1)[nonpos].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_mask_loss_is_bitwise_deterministic(dtype):
    nc, B, S = 20, 2, 128
    maps, mc, proto, batch = _seg_inputs(77, B, S, [4, 3], nc, dtype)
    r1 = _run_seg(maps, mc, proto, batch, nc, True, dtype)
    r2 = _run_seg(maps, mc, proto, batch, nc, True, dtype)
    assert torch.equal(r1[1].cpu(), r2[1].cpu()) and torch.equal(r1[2].cpu(), r2[2].cpu())
    assert torch.equal(r1[4].grad.cpu(), r2[4].grad.cpu()) and torch.equal(r1[5].grad.cpu(), r2[5].grad.cpu())


def test_mask_loss_rejects_wrong_mask_layouts():
    nc, B, S = 20, 2, 128
    maps, mc, proto, batch = _seg_inputs(5, B, S, [2, 2], nc, torch.float32, overlap=False)
    with pytest.raises(ValueError, match="overlap_mask=True"):
        _run_seg(maps, mc, proto, batch, nc, True, torch.float32)
    batch.pop("masks")
    with pytest.raises(ValueError, match="masks"):
        _run_seg(maps, mc, proto, batch, nc, True, torch.float32)


# ---------------------------------------------------------------------------------------------------- blocks and models
def test_proto_block_golden():
    from test_gpu_parity import _run_block
    from dedark_yolo_amd.nn.modules import Proto
    _run_block("g16_proto", Proto(16, 32, 32))


def _seg_model(seed, nc=20):
    from oracle import model as om
    from parity_helpers import load_sd
    from types import SimpleNamespace
    from dedark_yolo_amd.nn.tasks import SegmentationModel
    cfg = load_yaml("yolov8-seg.yaml")
    cfg["scales"]["t"] = TINY
    cfg["scale"] = "t"
    model = SegmentationModel(cfg, nc=nc)
    model.args = SimpleNamespace(box=7.5, cls=0.5, dfl=1.5, overlap_mask=True)
    load_sd(model, om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed))
    return model.cuda()


def test_tiny_seg_model_step_golden():
    """one training forward / loss / backward of the tiny segmentation model against the reference's (g16_seg_tiny): loss and
    items [box, seg, cls, dfl] within 1e-4 relative, selected gradients; then the eval output layout."""
    g = gold("g16_seg_tiny")
    model = _seg_model(int(g["seed"])).train()
    batch = make_batch(int(g["seed"]) + 1, int(g["B"]), int(g["S"]), [int(v) for v in g["nbox"]])
    batch["img"] = batch["img"].pow(3.0).cuda()
    batch["masks"] = g["masks"]
    loss, items = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    assert float(g["items"][1]) > 0
    close(float(loss.detach()), g["loss"], 1e-4, 1e-4, "loss vs reference golden")
    close(items.float().cpu(), g["items"], 1e-4, 1e-5, "items vs reference golden")
    named = dict(model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in named.values() if p.requires_grad)
    for k, v in g.items():
        if k.startswith("gn:"):
            close(named[k[3:]].grad.norm().cpu(), v, 5e-3, 1e-6, k)
        elif k.startswith("g:"):
            close(named[k[2:]].grad.cpu(), v, 5e-3, 5e-3 * float(v.abs().max()), k)
    model.eval()
    with torch.no_grad():
        y, (maps, mc, p) = model(batch["img"])
    A = sum(m.shape[2] * m.shape[3] for m in maps)
    assert tuple(y.shape) == (2, 4 + 20 + 32, A) and y.dtype == torch.float32
    for got, want, what in ((y[:, :, ::3], g["y"], "eval y"), (p, g["proto"], "eval proto")):        # after the step's BN updates
        err = float((got.float().cpu() - want).abs().max()) / float(want.abs().max())
        assert got.shape == want.shape and err <= 1e-4, (what, err)
    assert tuple(mc.shape) == (2, 32, A) and tuple(p.shape) == (2, 32, 32, 32)
    assert torch.equal(y[:, 24:].cpu(), mc.float().cpu())


@pytest.mark.parametrize("dtype", [torch.bfloat16], ids=["bf16"])
def test_tiny_seg_model_low_precision(dtype):
    import dedark_yolo_amd as dy
    g = gold("g16_seg_tiny")
    dy.set_compute_dtype(dtype)
    model = _seg_model(int(g["seed"])).train()
    batch = make_batch(int(g["seed"]) + 1, int(g["B"]), int(g["S"]), [int(v) for v in g["nbox"]])
    batch["img"] = batch["img"].pow(3.0).cuda()
    batch["masks"] = g["masks"]
    loss, items = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(items).all())
    assert abs(float(loss) - float(g["loss"])) <= 5e-2 * abs(float(g["loss"])), (float(loss), float(g["loss"]))
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.requires_grad)


def test_trainer_steps_save_and_resume_on_a_seg_model(tmp_path):
    """three trainer steps of a tiny segmentation model (branch streams on), save_model, resume_training into a fresh trainer
    (same parameters), one more step there: four finite loss items each step."""
    import bench
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    from dedark_yolo_amd.nn.tasks import SegmentationModel
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint
    cfgd = load_yaml("yolov8-seg.yaml")
    cfgd["scales"]["t"] = TINY
    cfgd["scale"] = "t"

    def trainer():
        torch.manual_seed(3)
        tr = DetectionTrainer(get_cfg(dict(model="tiny", dtype="fp32", optimizer="SGD", batch=64, lowlight_FLAG=False,
                                           dedark_FLAG=False, imgsz=96, deterministic=False)))
        tr.setup(SegmentationModel(dict(cfgd), nc=20))
        return tr

    def step(tr, seed):
        b = bench.synth_batch(seed, 4, 96, 20, "cpu")
        tr.args.dark_param = b.pop("gamma")
        b["masks"] = _box_masks(b, 4, 24, 24, True)
        loss, items = tr.train_step(b, [0.01] * 3, 0.9)
        assert items.numel() == 4 and bool(torch.isfinite(items).all()) and float(items[1]) > 0
        return float(loss)

    tr = trainer()
    losses = [step(tr, 80 + i) for i in range(3)]
    torch.cuda.synchronize()
    assert all(np.isfinite(losses))
    assert bool(torch.isfinite(tr.flat.p).all()) and bool(torch.isfinite(tr.flat.g).all())
    last = tr.save_model(str(tmp_path), epoch=3, fitness=None)
    ck = load_checkpoint(last)
    assert list(ck.model_sd) == list(tr.model.state_dict())
    tr2 = trainer()
    assert tr2.resume_training(last) == 4
    torch.cuda.synchronize()
    assert float((tr2.flat.p - tr.flat.p.half().float()).abs().max()) == 0.0
    assert np.isfinite(step(tr2, 90))
    vb = bench.synth_batch(99, 4, 96, 20, "cpu")
    vb.pop("gamma")
    vb["masks"] = _box_masks(vb, 4, 24, 24, True)
    metrics, fit = tr2.validate([vb])
    for k in ("metrics/precision(M)", "metrics/recall(M)", "metrics/mAP50(M)", "metrics/mAP50-95(M)", "metrics/mAP50(B)"):
        assert k in metrics and np.isfinite(metrics[k]), k
    assert np.isfinite(fit) and abs(fit - metrics["fitness"]) < 1e-12


# ---------------------------------------------------------------------------------------------------- reference fixtures
LOSS_GOLD = ["overlap", "planes", "masks2x", "planes2x", "nolabels1", "nopos", "nopos_planes"]


@pytest.mark.parametrize("tag", LOSS_GOLD)
def test_mask_loss_vs_reference(tag):
    """v8SegmentationLoss against the reference's (g16_segloss_*, float32 on the CPU) on the same random maps / mc / proto / masks:
    loss and items within 1e-4 relative, d mc, d proto and d maps within 1e-3 relative L2."""
    g = gold(f"g16_segloss_{tag}")
    B, S, nc = 2, 128, 20
    gen = np.random.default_rng(int(g["seed"]))
    maps = [torch.from_numpy(gen.normal(0, 1.0, (B, 64 + nc, S // s, S // s)).astype(np.float32)) for s in (8, 16, 32)]
    A = sum(t.shape[2] * t.shape[3] for t in maps)
    mc = torch.from_numpy(gen.normal(0, 0.5, (B, 32, A)).astype(np.float32))
    proto = torch.from_numpy(gen.normal(0, 1.0, (B, 32, S // 4, S // 4)).astype(np.float32))
    batch = make_batch(int(g["seed"]) + 1, B, S, [int(v) for v in g["nbox"]], nc)
    batch["masks"] = g["masks"]
    crit, loss, items, gm, gmc, gp = _run_seg(maps, mc, proto, batch, nc, bool(int(g["overlap"])), torch.float32)
    close(float(loss), g["loss"], 1e-4, 1e-5, f"{tag} loss")
    close(items.cpu(), g["items"], 1e-4, 1e-6, f"{tag} items")
    for got, want, what in [(gmc.grad, g["dmc"], "d mc"), (gp.grad, g["dproto"], "d proto")] + \
            [(gm[i].grad, g[f"dmap{i}"], f"d map{i}") for i in range(3)]:
        if float(want.abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, what
        else:
            assert _rel_l2(got.float(), want) <= 1e-3, (tag, what, _rel_l2(got.float(), want))


def test_segment_block_golden():
    """Segment(20, 32, 32, (32, 64, 64)) against the reference's (g16_segment): train outputs (maps, mc, proto), input and selected
    parameter gradients; eval output cat([y, mc], 1) and proto."""
    from oracle import model as om
    from parity_helpers import load_sd, set_bn
    from dedark_yolo_amd.nn.modules import Segment
    g = gold("g16_segment")
    m = Segment(20, 32, 32, (32, 64, 64))
    load_sd(set_bn(m), om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"])))
    m.stride = torch.tensor([8.0, 16.0, 32.0])
    m = m.cuda().train()
    xs = [g[f"x{i}"].clone().cuda().requires_grad_(True) for i in range(3)]
    maps, mc, p = m(xs)
    ys = list(maps) + [mc, p]
    tot = 0
    for i, t in enumerate(ys):
        close(t.detach().float().cpu(), g[f"y{i}"], 1e-4, 1e-4, f"y{i}")
        tot = tot + (t.float() * rnd(1630 + i, *t.shape, lo=-1, hi=1).cuda()).sum()
    tot.backward()
    torch.cuda.synchronize()
    for i, x in enumerate(xs):
        close(x.grad.float().cpu(), g[f"dx{i}"], 2e-3, 2e-3, f"dx{i}")
    named = dict(m.named_parameters())
    for k, v in g.items():
        if k.startswith("g:"):
            close(named[k[2:]].grad.cpu(), v, 2e-3, 2e-3 * float(v.abs().max()), k)
    m.eval()
    with torch.no_grad():
        ye, (_, _, pe) = m([x.detach() for x in xs])
    close(ye.cpu(), g["y_eval"], 1e-4, 1e-4, "eval y")
    close(pe.float().cpu(), g["p_eval"], 1e-4, 1e-4, "eval proto")


def test_mask_decode_iou_and_correct_matrices_vs_reference():
    """process_mask (dy_seg_mask_decode) on the reference's fixed predictions, equal where |z| >= 1e-5 (sigmoid near 0.5 may round
    either way); mask IoU (dy_seg_mask_iou) on the reference's masks, index map and planes; the correct matrices of the segment
    validator's path (mask_iou_binary + match_from_iou) equal the reference's _process_batch(masks=True)."""
    from dedark_yolo_amd.engine.validator import match_from_iou
    from dedark_yolo_amd.utils import ops as uops
    g = gold("g16_val")
    pm = uops.process_mask(g["proto"].cuda(), g["coef"].cuda(), g["boxes"].cuda(), (128, 128))
    sure = g["z"].abs() >= 1e-5
    assert torch.equal(pm.cpu()[sure], g["masks"][sure])
    masks = g["masks"].to(torch.uint8).cuda()
    iou_pl = uops.mask_iou_binary(g["planes"].cuda(), masks, False, 5)
    iou_ov = uops.mask_iou_binary(g["gt_idx"].cuda(), masks, True, 5)
    assert torch.equal(iou_pl.cpu(), g["iou"]) and torch.equal(iou_ov.cpu(), g["iou"])
    ref_iou = uops.mask_iou(g["planes"].view(5, -1).float().cuda(), g["masks"].view(12, -1).cuda())
    assert torch.equal(ref_iou.cpu(), g["iou"])
    iouv = torch.linspace(0.5, 0.95, 10)
    for got_iou, want in ((iou_ov, g["correct_overlap"]), (iou_pl, g["correct_planes"])):
        assert torch.equal(match_from_iou(got_iou.cpu().numpy(), g["labels"][:, 0], g["dets"][:, 5], iouv), want)
    crop = uops.crop_mask(torch.ones(12, 32, 32, device="cuda"), g["boxes"].cuda() / 4)
    assert float(crop.sum()) > 0 and torch.equal((crop.cpu() > 0) & g["masks"].bool(), g["masks"].bool())


def test_nms_with_mask_columns():
    """non_max_suppression(nc=...) on a [B, 4+nc+nm, A] eval output: the box / class columns equal the detection NMS of the first
    4+nc rows, and the appended columns are the kept anchors' coefficients."""
    from dedark_yolo_amd.utils import ops as uops
    gen = np.random.default_rng(5)
    B, nc, nm, A = 2, 20, 32, 336
    box = torch.from_numpy(gen.uniform(0, 100, (B, 2, A)).astype(np.float32))
    wh = torch.from_numpy(gen.uniform(4, 40, (B, 2, A)).astype(np.float32))
    cls = torch.from_numpy(gen.random((B, nc, A)).astype(np.float32)) ** 4
    mc = torch.from_numpy(gen.normal(0, 1, (B, nm, A)).astype(np.float32))
    pred = torch.cat([box, wh, cls, mc], 1).cuda()
    with_m = uops.non_max_suppression(pred, 0.25, 0.7, multi_label=True, nc=nc)
    plain = uops.non_max_suppression(pred[:, :4 + nc].contiguous(), 0.25, 0.7, multi_label=True)
    _, _, keep = uops.nms_batched(pred[:, :4 + nc], 0.25, 0.7, True, False, 300, 30000, 7680, return_indices=True)
    for i in range(B):
        assert with_m[i].shape[1] == 6 + nm and torch.equal(with_m[i][:, :6], plain[i])
        n = with_m[i].shape[0]
        assert n > 0
        anchors = (keep[i, :n] // nc).cpu()
        assert torch.equal(with_m[i][:, 6:].cpu(), mc[i][:, anchors].t())


def test_product_eval_equals_the_reference_running_our_seg_checkpoint():
    """g16_seg_interop: the reference loaded a tiny seg last.pt this package wrote (EMA weights, rng_fill seed 1722, half) and ran
    eval; the product on the same half-rounded weights gives the same cat([y, mc], 1) and proto."""
    from oracle import model as om
    from parity_helpers import load_sd
    g = gold("g16_seg_interop")
    model = _seg_model(1)
    ema = om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, 1722)
    load_sd(model, {k: (v.half().float() if v.is_floating_point() else v) for k, v in ema.items()})
    model = model.cuda().eval()
    model.fuse()
    x = rnd(int(g["x_seed"]), 2, 3, 128, 128).pow(2.0)
    with torch.no_grad():
        y, (_, _, p) = model(x.cuda())
    for got, want, what in ((y, g["y"], "y"), (p, g["proto"], "proto")):
        err = float((got.float().cpu() - want).abs().max()) / float(want.abs().max())
        assert got.shape == want.shape and err <= 1e-4, (what, err)
