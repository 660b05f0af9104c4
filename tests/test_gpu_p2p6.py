"""GPU tests of the four-level heads and the C2 block: the loss / assigner / decode kernels at four levels (through the C-ABI,
dy_det_maps4) against the oracle criterion and autograd, the gradient maps' extent, the C2 block and whole p2 / p6 / Faster4.0 /
ThreeHead / +RBF models against the reference's fixtures (tests/golden/make_p2p6_golden.py), the 16-bit paths, the product's eval
output on the reference's reading of our p6 checkpoint, and a trainer step / save / resume / validate on a tiny p2 model."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import close, gold, load_yaml, make_batch, rnd

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (strides, image size): P2..P5, P3..P6 and a coarse-to-fine order (as +RBF's / Faster4.0's Detect rows); A = 1360 >= 640 each
LEVELS = [((4.0, 8.0, 16.0, 32.0), 128), ((8.0, 16.0, 32.0, 64.0), 256), ((64.0, 32.0, 16.0, 8.0), 256)]
TINY = [0.33, 0.125, 1024]


@pytest.fixture(autouse=True)
def _fp32():
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(torch.float32)
    yield
    dy.set_compute_dtype(torch.float32)


def _rand_maps(seed, B, S, strides, nc, dtype):
    gen = np.random.default_rng(seed)
    return [torch.from_numpy(gen.normal(0, 1.0, (B, 64 + nc, int(S // s), int(S // s))).astype(np.float32)).to(dtype)
            for s in strides]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", range(len(LEVELS)), ids=["p2", "p6", "coarse_first"])
def test_four_level_loss_vs_oracle(case, dtype):
    """dy_loss_decode / dy_tal_assign / dy_loss_fwd / dy_loss_bwd on four maps: decoded boxes, assignment (bit-exact), loss items and
    every map gradient against oracle.loss.detection_loss + autograd on the same (dtype-rounded) maps."""
    import dedark_yolo_amd as dy
    from types import SimpleNamespace
    from dedark_yolo_amd.utils.loss import RcoveryDetectionLoss
    from oracle import loss as oloss
    strides, S = LEVELS[case]
    nc, B = 20, 3
    maps = _rand_maps(31 + case, B, S, strides, nc, dtype)
    batch = make_batch(41 + case, B, S, [3, 6, 1])
    batch["recovery_loss_batch"] = torch.tensor(0.05)
    om_ = [m.float().clone().requires_grad_(True) for m in maps]
    ol, oi, det = oloss.detection_loss(om_, batch, list(strides), nc, oloss.default_hyp(), details=True)
    ol.backward()
    dy.set_compute_dtype(dtype)
    dmod = SimpleNamespace(stride=torch.tensor(strides), nc=nc, no=64 + nc, reg_max=16)
    holder = SimpleNamespace(args=oloss.default_hyp(), model=[dmod], parameters=lambda: iter([torch.zeros(1, device="cuda")]))
    crit = RcoveryDetectionLoss(holder)
    gm = [m.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for m in maps]
    gb = {k: v for k, v in batch.items() if k != "recovery_loss_batch"}
    loss, items = crit(gm, gb)
    loss.backward()
    torch.cuda.synchronize()
    a = crit.last_assignment
    # decode (grid units) against the oracle's bbox_decode
    no = 64 + nc
    cat = torch.cat([m.float().view(B, no, -1) for m in maps], 2)
    anchors, _ = oloss.make_anchors([m.shape[2:] for m in maps], list(strides))
    want_boxes = oloss.decode_boxes(cat[:, :64].permute(0, 2, 1).contiguous(), anchors)
    close(a.pred_boxes.cpu(), want_boxes, 1e-5, 1e-4, "decoded boxes")
    assert torch.equal(a.fg_mask.cpu().bool(), det["fg_mask"]), "fg_mask differs"
    assert torch.equal(a.target_gt_idx.cpu().long(), det["target_gt_idx"]), "target_gt_idx differs"
    fg = det["fg_mask"]
    assert int(fg.sum()) > 0
    assert torch.equal(a.target_label.cpu().long()[fg], det["target_labels"][fg])
    close(a.norm.cpu(), det["target_scores"].sum(-1), 1e-4, 1e-6, "target score per anchor")
    close(loss.cpu(), ol.detach(), 1e-4, 1e-4, "loss")
    close(items.cpu(), oi, 1e-4, 1e-4, "loss_items")
    rt = {torch.float32: 2e-3, torch.bfloat16: 1.6e-2, torch.float16: 4e-3}[dtype]
    for i in range(4):
        g = gm[i].grad
        assert g.dtype == dtype and tuple(g.shape) == tuple(maps[i].shape)
        scale = float(om_[i].grad.abs().max())
        close(g.float().cpu(), om_[i].grad, rt, 1e-5 + rt * 1e-2 * scale, f"d loss / d map{i}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_loss_bwd_writes_all_four_maps_and_nothing_past_them(dtype):
    """dy_loss_bwd through ctypes with four gradient buffers framed by sentinels: every element of each [B, h*w, ld] map is written
    (padding lanes included) and the guard words before and after are untouched."""
    from dedark_yolo_amd import _C, ops
    from dedark_yolo_amd.utils.loss import assign
    strides, S = LEVELS[0]
    nc, B = 20, 2
    ops.set_compute_dtype(dtype)
    maps = [ops.as_nhwc(m.cuda(), dtype) for m in _rand_maps(7, B, S, strides, nc, dtype)]
    batch = make_batch(8, B, S, [4, 2])
    a = assign(maps, list(strides), nc, batch["batch_idx"], batch["cls"], batch["bboxes"])
    dm = ops.det_maps(maps, list(strides), nc)
    assert isinstance(dm, _C.DetMaps4) and dm.n_levels == 4
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    _C.call("dy_loss_fwd", C.byref(dm), ops.ptr(a.pred_boxes), ops.ptr(a.fg_mask), ops.ptr(a.norm), ops.ptr(a.target_label),
            ops.ptr(a.target_box), ops.ptr(acc), ops.stream())
    ld = 64 + ops.round_up(nc, ops.vec_elems(dtype))
    GUARD, SENT = 64, 4096.0                   # exact in every dtype
    bufs, views = [], []
    for m in maps:
        n = B * m.shape[2] * m.shape[3] * ld
        buf = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device="cuda")
        bufs.append((buf, n))
        views.append(buf[GUARD:GUARD + n])
    arr_p = (C.c_void_p * 4)(*[v.data_ptr() for v in views])
    arr_l = (C.c_int64 * 4)(*([ld] * 4))
    g = torch.ones(1, dtype=torch.float32, device="cuda")
    _C.call("dy_loss_bwd", C.byref(dm), arr_p, arr_l, ops.ptr(a.pred_boxes), ops.ptr(a.fg_mask), ops.ptr(a.norm),
            ops.ptr(a.target_label), ops.ptr(a.target_box), ops.ptr(acc), ops.ptr(g), 7.5, 0.5, 1.5, ops.stream())
    torch.cuda.synchronize()
    for i, (buf, n) in enumerate(bufs):
        body = buf[GUARD:GUARD + n].float()
        assert bool(torch.isfinite(body).all()) and not bool((body == SENT).any()), f"map {i}: elements left unwritten"
        assert bool((buf[:GUARD].float() == SENT).all()) and bool((buf[GUARD + n:].float() == SENT).all()), f"map {i}: wrote outside"
        pad = body.view(-1, ld)[:, 64 + nc:]
        assert bool((pad == 0).all()), f"map {i}: padding lanes not zero"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", range(len(LEVELS)), ids=["p2", "p6", "coarse_first"])
def test_detect_decode_four_levels(case, dtype):
    """dy_detect_decode on four maps: y[B, 4+nc, A] = cat(xywh * stride, sigmoid(cls)) as Detect's eval branch."""
    from dedark_yolo_amd import _C, ops
    from oracle import loss as oloss
    strides, S = LEVELS[case]
    nc, B = 20, 2
    ops.set_compute_dtype(dtype)
    maps = _rand_maps(60 + case, B, S, strides, nc, dtype)
    gm = [ops.as_nhwc(m.cuda(), dtype) for m in maps]
    dm = ops.det_maps(gm, list(strides), nc)
    A = sum(m.shape[2] * m.shape[3] for m in maps)
    y = torch.full((B, 4 + nc, A), float("nan"), dtype=torch.float32, device="cuda")
    _C.call("dy_detect_decode", C.byref(dm), ops.ptr(y), ops.stream())
    torch.cuda.synchronize()
    cat = torch.cat([m.float().view(B, 64 + nc, -1) for m in maps], 2)
    anchors, st = oloss.make_anchors([m.shape[2:] for m in maps], list(strides))
    xyxy = oloss.decode_boxes(cat[:, :64].permute(0, 2, 1).contiguous(), anchors)
    xywh = torch.cat(((xyxy[..., :2] + xyxy[..., 2:]) / 2, xyxy[..., 2:] - xyxy[..., :2]), -1) * st
    want = torch.cat((xywh.permute(0, 2, 1), cat[:, 64:].sigmoid()), 1)
    close(y.cpu(), want, 1e-5, 1e-3, "eval decode")


def test_c_abi_rejects_five_levels():
    from dedark_yolo_amd import ops
    m = torch.zeros((1, 84, 4, 4), device="cuda").contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="1-4"):
        ops.det_maps([m] * 5, [8.0] * 5, 20)


@pytest.mark.parametrize("name,args", [("g15_c2_sc1", (32, 32, 1, True)), ("g15_c2_sc2", (32, 32, 2, True)),
                                       ("g15_c2_nosc1", (48, 32, 1, False)), ("g15_c2_nosc2", (48, 64, 2, False))])
def test_c2_block_golden(name, args):
    from test_gpu_parity import _run_block
    from dedark_yolo_amd.nn.modules import C2
    _run_block(name, C2(*args))


@pytest.mark.parametrize("fused", [False, True], ids=["eval", "eval_fused"])
def test_c2_block_eval_matches_torch(fused):
    """eval / no_grad path of C2 (BN folded into the conv epilogues) equals the block computed with torch ops in float64."""
    from oracle import model as om
    from parity_helpers import load_sd, set_bn
    from dedark_yolo_amd.nn.modules import C2
    g = gold("g15_c2_sc2")
    m = C2(32, 32, 2, True)
    load_sd(set_bn(m), om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"])))
    ref = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.cuda().eval()
    if fused:
        from dedark_yolo_amd.nn.tasks import BaseModel
        holder = BaseModel()
        holder.model = torch.nn.Sequential(m)
        holder.fuse(verbose=False)
        assert holder.is_fused()
    x = g["x0"].cuda()
    with torch.no_grad():
        y = m(x)
    xt = g["x0"].double()
    sd = {k: v.double() for k, v in ref.items()}

    def conv_bn(t, p, k):
        z = F.conv2d(t, sd[p + "conv.weight"], padding=k // 2)
        sc = sd[p + "bn.weight"] / torch.sqrt(sd[p + "bn.running_var"] + 1e-3)
        z = (z - sd[p + "bn.running_mean"].view(1, -1, 1, 1)) * sc.view(1, -1, 1, 1) + sd[p + "bn.bias"].view(1, -1, 1, 1)
        return F.silu(z)
    a, b = conv_bn(xt, "cv1.", 1).chunk(2, 1)
    for i in range(2):
        a = a + conv_bn(conv_bn(a, f"m.{i}.cv1.", 3), f"m.{i}.cv2.", 3)
    want = conv_bn(torch.cat((a, b), 1), "cv2.", 1)
    close(y.double().cpu(), want, 1e-4, 1e-4, "C2 eval")


def _model(yaml_name, scale, scale_def, seed, nc=20):
    from oracle import model as om
    from parity_helpers import HYP, load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    cfg = load_yaml(yaml_name)
    if scale_def is not None:
        cfg["scales"][scale] = list(scale_def)
    cfg["scale"] = scale
    model = DetectionModel(dict(cfg), ch=3, nc=nc)
    model.args = HYP
    load_sd(model, om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed))
    return model.cuda()


def _model_step(name, yaml_name, scale, dtype=torch.float32):
    import dedark_yolo_amd as dy
    g = gold(name)
    sdef = [float(v) for v in g["scale_def"]] if g["scale_def"].numel() == 3 else None
    dy.set_compute_dtype(dtype)
    model = _model(yaml_name, scale, sdef, int(g["seed"])).train()
    batch = make_batch(int(g["seed"]) + 1, int(g["B"]), int(g["S"]), [int(v) for v in g["nbox"]])
    batch["img"] = batch["img"].pow(3.0).cuda()
    batch["recovery_loss_batch"] = torch.tensor(0.0123).cuda()
    loss, items = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    return g, model, batch, loss, items


MODELS = [("g15_p2_tiny", "yolov8-p2.yaml", "t"), ("g15_p6_tiny", "yolov8-p6.yaml", "t"), ("g15_f4_l", "yolov8-Faster4.0.yaml", "l"),
          ("g15_th_l", "yolov8-Faster3.0-ThreeHead.yaml", "l"), ("g15_rbf_l", "yolov8+RBF.yaml", "l")]


@pytest.mark.parametrize("name,yml,scale", MODELS, ids=[m[0][4:] for m in MODELS])
def test_model_step_golden(name, yml, scale):
    g, model, batch, loss, items = _model_step(name, yml, scale)
    close(float(loss.detach()), g["loss"], 1e-4, 1e-4, f"{name} loss vs reference golden")
    close(items.float().cpu(), g["items"], 1e-4, 1e-4, f"{name} items vs reference golden")
    named = dict(model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in named.values() if p.requires_grad)
    # L graphs at 64x64, B=2 are ill-conditioned in fp32 (tests/test_gpu_parity.py::test_model_repo_l_golden): sanity bound there
    gtol = 5e-3 if scale == "t" else 0.5
    msd = model.state_dict()
    for k, v in g.items():
        if k.startswith("gn:"):
            close(named[k[3:]].grad.norm().cpu(), v, gtol, 1e-6, f"{name} {k}")
        elif k.startswith("g:"):
            close(named[k[2:]].grad.cpu(), v, gtol, gtol * float(v.abs().max()), f"{name} {k}")
        elif k.startswith("b:"):
            close(msd[k[2:]].cpu(), v, 1e-4, 1e-4, f"{name} {k}")
    model.eval()
    with torch.no_grad():
        y, maps = model(batch["img"])
    assert len(maps) == model.model[-1].nl
    ytol = 1e-4 if scale == "t" else 2e-2
    err = float((y[:, :, ::7].float().cpu() - g["y"]).abs().max()) / float(g["y"].abs().max())
    assert err <= ytol, err


def _grads(m):
    return torch.cat([p.grad.double().flatten() for p in m.parameters() if p.requires_grad])


def _cos(a, b):
    return float((a @ b) / (a.norm() * b.norm()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name,yml", [("g15_p2_tiny", "yolov8-p2.yaml"), ("g15_p6_tiny", "yolov8-p6.yaml")], ids=["p2", "p6"])
def test_four_level_model_low_precision(name, yml, dtype):
    """16-bit runs of the tiny p2 / p6 models: finite; loss and gradient direction as close to the fp32 path's as the fp32 kernels
    with 16-bit STORAGE get (ops.set_storage_emulation: the rounding any 16-bit implementation has), or within 3 % (bf16) / 2 %
    (f16) and cosine 0.95."""
    from dedark_yolo_amd import ops
    g, m16, _, loss, items = _model_step(name, yml, "t", dtype)
    assert torch.isfinite(loss) and bool(torch.isfinite(items).all())
    a = _grads(m16)
    assert bool(torch.isfinite(a).all())
    _, m32, _, loss32, _ = _model_step(name, yml, "t", torch.float32)
    ops.set_storage_emulation(dtype)
    try:
        _, memu, _, loss_emu, _ = _model_step(name, yml, "t", torch.float32)
    finally:
        ops.set_storage_emulation(None)
    l16, l32, lemu = float(loss), float(loss32), float(loss_emu)
    assert abs(l32 - float(g["loss"])) <= 1e-4 * abs(float(g["loss"]))
    print(f"{name} {dtype}: loss {l16:.4f}, fp32 {l32:.4f}, 16-bit storage emulation {lemu:.4f}")
    # bf16: 3 % as tests/test_gpu_parity.py::test_bf16_step_close_to_fp32_oracle (tiny p6 in bf16 lands about 2 % off)
    tol = 3e-2 if dtype == torch.bfloat16 else 2e-2
    assert abs(l16 - l32) <= max(tol * abs(l32), 2.0 * abs(lemu - l32)), (l16, l32, lemu)
    b, e = _grads(m32), _grads(memu)
    cos, cos_emu = _cos(a, b), _cos(e, b)
    print(f"{name} {dtype}: gradient cosine vs fp32 {cos:.4f}, 16-bit storage emulation {cos_emu:.4f}")
    assert cos >= min(cos_emu, 0.95) - 0.03, (cos, cos_emu)


def test_product_eval_equals_the_reference_running_our_p6_checkpoint():
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    g = gold("g15_p6_interop")
    cfg = load_yaml("yolov8-p6.yaml")
    cfg["scales"]["t"] = TINY
    cfg["scale"] = "t"
    model = DetectionModel(cfg, nc=20)
    ema = om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, 1522)
    load_sd(model, {k: (v.half().float() if v.is_floating_point() else v) for k, v in ema.items()})
    model = model.cuda().eval()
    model.fuse()
    x = rnd(int(g["p6_t_x_seed"]), 2, 3, 128, 128).pow(2.0)
    with torch.no_grad():
        y = model(x.cuda())
    y = y[0] if isinstance(y, (list, tuple)) else y
    want = g["p6_t_y"]
    err = float((y.float().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)
    assert y.shape == want.shape and err <= 1e-4, err


def test_p6_model_rejects_a_640_image():
    m = _model("yolov8-p6.yaml", "t", TINY, 1).eval()
    with torch.no_grad(), pytest.raises(ValueError, match="largest stride 64"):
        m(torch.zeros(1, 3, 640 - 32, 640 - 32, device="cuda"))


def test_trainer_step_save_resume_and_validate_on_a_p2_model(tmp_path):
    """Two trainer steps of a tiny p2 model (four-level loss, branch streams for three side levels), save_model, resume_training
    into a fresh trainer (same parameters), one more step there, and validate()."""
    import bench
    import dedark_yolo_amd as dy
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    from dedark_yolo_amd.nn.tasks import DetectionModel
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint
    dy.set_compute_dtype(torch.float32)
    cfgd = load_yaml("yolov8-p2.yaml")
    cfgd["scales"]["t"] = TINY
    cfgd["scale"] = "t"

    def trainer():
        torch.manual_seed(3)
        tr = DetectionTrainer(get_cfg(dict(model="tiny", dtype="fp32", optimizer="SGD", batch=64, lowlight_FLAG=False,
                                           dedark_FLAG=False, imgsz=64, conf=0.001, iou=0.7)))
        tr.setup(DetectionModel(dict(cfgd), nc=20))
        return tr

    def step(tr, seed):
        b = bench.synth_batch(seed, 4, 96, 20, "cuda")
        tr.args.dark_param = b.pop("gamma")
        b.pop("n_max", None)
        loss, _ = tr.train_step(b, [0.01] * 3, 0.9)
        return float(loss)

    tr = trainer()
    losses = [step(tr, 80 + i) for i in range(2)]
    torch.cuda.synchronize()
    assert all(np.isfinite(losses))
    assert bool(torch.isfinite(tr.flat.p).all()) and bool(torch.isfinite(tr.flat.g).all())
    last = tr.save_model(str(tmp_path), epoch=2, fitness=0.1)
    ck = load_checkpoint(last)
    assert list(ck.model_sd) == list(tr.model.state_dict())
    tr2 = trainer()
    assert tr2.resume_training(last) == 3
    torch.cuda.synchronize()
    assert float((tr2.flat.p - tr.flat.p.half().float()).abs().max()) == 0.0
    assert np.isfinite(step(tr2, 90))
    vb = bench.synth_batch(99, 4, 64, 20, "cpu")
    vb.pop("gamma"), vb.pop("n_max", None)
    vb["ori_shape"] = [(64, 64)] * 4
    metrics, fit = tr2.validate([vb])
    assert np.isfinite(fit) and "metrics/mAP50(B)" in metrics
