"""GPU tests of the pose task: the keypoint loss (csrc/pose.hip through the C-ABI, via v8PoseLoss) against an in-test float64
restatement of the reference's v8PoseLoss keypoint loop on the kernel's own assignment and against the reference's fixtures
(tests/golden/make_pose_golden.py), the 51-channel cv4 chain against float64 torch, the Pose block and whole tiny pose models against
the reference, the OKS kernel, NMS with keypoint columns, trainer steps / save / resume / validate and predict()."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import close, gold, load_yaml

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
TINY = [0.33, 0.125, 1024]
STRIDES = (8.0, 16.0, 32.0)
OKS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


@pytest.fixture(autouse=True)
def _fp32():
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(torch.float32)
    yield
    dy.set_compute_dtype(torch.float32)


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _holder(nc, kpt_shape, crit="pose"):
    from types import SimpleNamespace
    from dedark_yolo_amd.utils.loss import RcoveryDetectionLoss, v8PoseLoss
    head = SimpleNamespace(stride=torch.tensor(STRIDES), nc=nc, no=64 + nc, reg_max=16, kpt_shape=kpt_shape)
    h = SimpleNamespace(args=SimpleNamespace(box=7.5, cls=0.5, dfl=1.5, pose=12.0, kobj=1.0, lrl=2.0), model=[head],
                        parameters=lambda: iter([torch.zeros(1, device="cuda")]))
    return v8PoseLoss(h) if crit == "pose" else RcoveryDetectionLoss(h)


def _levels(kpt, maps):
    """[B, nk, A] rows -> per-level [B, nk, h, w] maps (anchors level by level)"""
    out, o = [], 0
    for m in maps:
        h, w = m.shape[2], m.shape[3]
        out.append(kpt[:, :, o:o + h * w].reshape(kpt.shape[0], kpt.shape[1], h, w))
        o += h * w
    return out


def _case(tag):
    g = gold(f"g17_poseloss_{tag}")
    maps = [g[f"map{i}"] for i in range(3)]
    batch = dict(batch_idx=g["batch_idx"], cls=g["cls"], bboxes=g["bboxes"], keypoints=g["keypoints"])
    return g, maps, g["kpt"], batch, [int(v) for v in g["kpt_shape"]]


def _run_pose(maps, kpt, batch, kpt_shape, dtype, nc=4):
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(dtype)
    crit = _holder(nc, kpt_shape)
    gm = [m.to(dtype).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for m in maps]
    gk = [k.to(dtype).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for k in _levels(kpt, maps)]
    loss, items = crit((gm, gk), dict(batch))
    grads = torch.autograd.grad(loss, gm + gk)
    torch.cuda.synchronize()
    return crit, loss, items, grads[:3], grads[3:]


def _pose_ref(kpt, fg, tgi, tbox, batch, kpt_shape, img_hw, B):
    """float64 restatement of the reference's keypoint loop (loss.py:350-366, KeypointLoss :87-99) on a given assignment:
    returns (sum_i pose_i, sum_i kobj_i) before the gains"""
    K, nd = kpt_shape
    H, W = img_hw
    sig = torch.from_numpy(OKS) if list(kpt_shape) == [17, 3] else torch.ones(K, dtype=torch.float64) / K
    anchors, strides = [], []
    for s in STRIDES:
        h, w = int(H // s), int(W // s)
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
        anchors.append(torch.stack([xx.reshape(-1) + 0.5, yy.reshape(-1) + 0.5], 1))
        strides.append(torch.full((h * w,), s, dtype=torch.float64))
    anc, st = torch.cat(anchors), torch.cat(strides)
    kp = batch["keypoints"].double().clone()
    kp[..., 0] *= W
    kp[..., 1] *= H
    bi = batch["batch_idx"].long()
    pk = kpt.permute(0, 2, 1).reshape(B, -1, K, nd)
    pose = kobj = 0
    for i in range(B):
        f = fg[i]
        if not bool(f.any()):
            continue
        gk = kp[bi == i][tgi[i][f]].clone()
        gk[..., 0] /= st[f].view(-1, 1)
        gk[..., 1] /= st[f].view(-1, 1)
        tb = tbox[i][f].double() / st[f].view(-1, 1)
        area = ((tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])).view(-1, 1)
        p = pk[i][f]
        px = p[..., 0] * 2 + (anc[f, 0:1] - 0.5)
        py = p[..., 1] * 2 + (anc[f, 1:2] - 0.5)
        mask = (gk[..., 2] != 0).double()
        d = (px - gk[..., 0]) ** 2 + (py - gk[..., 1]) ** 2
        e = d / (2 * sig) ** 2 / (area + 1e-9) / 2
        factor = mask.numel() / (mask.sum() + 1e-9)
        pose = pose + factor * ((1 - torch.exp(-e)) * mask).mean()
        if nd == 3:
            kobj = kobj + F.binary_cross_entropy_with_logits(p[..., 2], mask)
    return pose, kobj


LOSS_TAGS = ["normal", "invisible", "nolabels1", "nopos", "k5"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tag", LOSS_TAGS)
def test_pose_loss_vs_float64_restatement(tag, dtype):
    """items [box, pose, kobj, cls, dfl] and the keypoint map gradients of v8PoseLoss against a float64 restatement of the reference's
    keypoint loop on the kernel's own assignment; box / cls / dfl items and map gradients equal the detection criterion's; gradients
    at non-positive anchors and in pad lanes are exactly 0."""
    from dedark_yolo_amd import ops
    g, maps, kpt, batch, ks = _case(tag)
    B, S = 2, 128
    crit, loss, items, dmaps, dks = _run_pose(maps, kpt, batch, ks, dtype)
    a = crit.last_assignment
    fg, tgi, tbox = a.fg_mask.cpu().bool(), a.target_gt_idx.cpu().long(), a.target_box.cpu()
    if tag == "nopos":
        assert not bool(fg.any())
    elif tag == "nolabels1":
        assert bool(fg[0].any()) and not bool(fg[1].any())
    else:
        assert bool(fg.any(1).all())
    dcrit = _holder(4, ks, "det")
    dm = [m.to(dtype).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for m in maps]
    dl, di = dcrit(dm, {k: v for k, v in batch.items() if k != "keypoints"})
    dg = torch.autograd.grad(dl, dm)
    torch.cuda.synchronize()
    assert torch.equal(items[[0, 3, 4]].cpu(), di.cpu())
    for g1, g2 in zip(dmaps, dg):
        assert torch.equal(g1.cpu(), g2.cpu())
    k64 = kpt.to(dtype).double().requires_grad_(True)
    pose, kobj = _pose_ref(k64, fg, tgi, tbox, batch, ks, (S, S), B)
    want_p, want_k = float(pose) * 12.0 / B, float(kobj) * 1.0 / B
    if torch.is_tensor(pose):
        ((pose * 12.0 / B + kobj * 1.0 / B) * B).backward()
    rt = 1e-4 if dtype == torch.float32 else 2e-3
    got_p, got_k = float(items[1]), float(items[2])
    assert abs(got_p - want_p) <= rt * abs(want_p) + 1e-7, (got_p, want_p)
    assert abs(got_k - want_k) <= rt * abs(want_k) + 1e-7, (got_k, want_k)
    if ks[1] == 2:
        assert got_k == 0.0
    assert abs(float(loss) - (float(dl) + (got_p + got_k) * B)) <= 1e-5 * abs(float(loss)) + 1e-6
    nk = ks[0] * ks[1]
    ve = ops.vec_elems(dtype)
    rows, pads = [], []
    for d in dks:
        assert d.dtype == dtype and ops.ld_of(d) == ops.round_up(nk, ve)
        Bq, _, h, w = d.shape
        full = torch.as_strided(d, (Bq, h, w, ops.ld_of(d)), (h * w * ops.ld_of(d), w * ops.ld_of(d), ops.ld_of(d), 1))
        pads.append(full[..., nk:].float().cpu())
        rows.append(full[..., :nk].reshape(Bq, h * w, nk).float().cpu())
    assert all(float(p.abs().max()) == 0.0 for p in pads if p.numel())
    got = torch.cat(rows, 1)                                          # [B, A, nk]
    assert float(got[~fg].abs().max()) == 0.0
    if tag == "nopos":
        assert got_p == 0.0 and got_k == 0.0 and float(got.abs().max()) == 0.0
        return
    want = k64.grad.permute(0, 2, 1)
    gt = 1e-4 if dtype == torch.float32 else 1e-2
    assert _rel_l2(got, want) <= gt, ("d kpt", _rel_l2(got, want))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_pose_loss_is_bitwise_deterministic(dtype):
    _, maps, kpt, batch, ks = _case("normal")
    r1 = _run_pose(maps, kpt, batch, ks, dtype)
    r2 = _run_pose(maps, kpt, batch, ks, dtype)
    assert torch.equal(r1[1].cpu(), r2[1].cpu()) and torch.equal(r1[2].cpu(), r2[2].cpu())
    for a, b in zip(r1[4], r2[4]):
        assert torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("tag", LOSS_TAGS)
def test_pose_loss_vs_reference(tag):
    """v8PoseLoss against the reference's (g17_poseloss_*, float32 on the CPU): loss and items within 1e-4 relative, keypoint and
    Detect map gradients within 1e-3 relative L2."""
    g, maps, kpt, batch, ks = _case(tag)
    crit, loss, items, dmaps, dks = _run_pose(maps, kpt, batch, ks, torch.float32)
    close(float(loss), g["loss"], 1e-4, 1e-5, f"{tag} loss")
    close(items.cpu(), g["items"], 1e-4, 1e-6, f"{tag} items")
    dk = torch.cat([d.float().cpu().reshape(d.shape[0], d.shape[1], -1) for d in dks], 2)
    for got, want, what in [(dk, g["dkpt"], "d kpt")] + [(dmaps[i], g[f"dmap{i}"], f"d map{i}") for i in range(3)]:
        if float(want.abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, what
        else:
            assert _rel_l2(got.float(), want) <= 1e-3, (tag, what, _rel_l2(got.float(), want))


def test_pose_loss_rejects_batches_without_keypoints():
    _, maps, kpt, batch, ks = _case("normal")
    bad = dict(batch)
    bad.pop("keypoints")
    with pytest.raises(ValueError, match="keypoints"):
        _run_pose(maps, kpt, bad, ks, torch.float32)
    bad["keypoints"] = batch["keypoints"][:, :5]
    with pytest.raises(ValueError, match="K=17"):
        _run_pose(maps, kpt, bad, ks, torch.float32)


# ---------------------------------------------------------------------------------------------------- blocks and models
@pytest.mark.parametrize("tag", ["g17_pose_block", "g17_pose_block_k5"])
def test_pose_block_golden(tag):
    """Pose(4, kpt_shape, (32, 64, 64)) train outputs, input / parameter gradients and BN statistics, then the eval output with
    the decoded keypoint rows, against the reference."""
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn.modules import Pose
    g = gold(tag)
    ks = [int(v) for v in g["kpt_shape"]]
    m = Pose(4, ks, (32, 64, 64))
    for x in m.modules():
        if isinstance(x, torch.nn.BatchNorm2d):
            x.eps, x.momentum = 1e-3, 0.03
    load_sd(m, om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"])))
    m = m.cuda()
    m.stride = torch.tensor(STRIDES)
    m.train()
    xs = [g[f"x{i}"].cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for i in range(3)]
    maps, kpt = m(xs)
    assert len(kpt) == 3
    ys = list(maps) + [torch.cat([k.reshape(k.shape[0], k.shape[1], -1) for k in kpt], 2)]
    from util import rnd
    tot = sum((t.float() * rnd(int(g["seed"]) + 10 + i, *t.shape, lo=-1, hi=1).cuda()).sum() for i, t in enumerate(ys))
    tot.backward()
    torch.cuda.synchronize()
    for i, t in enumerate(ys):
        close(t.detach().float().cpu(), g[f"y{i}"], 1e-4, 1e-4, f"y{i}")
    for i, x in enumerate(xs):
        close(x.grad.float().cpu(), g[f"dx{i}"], 1e-3, 1e-4 * float(g[f"dx{i}"].abs().max()), f"dx{i}")
    named = dict(m.named_parameters())
    sd = m.state_dict()
    for k, v in g.items():
        if k.startswith("g:"):
            close(named[k[2:]].grad.cpu(), v, 1e-3, 1e-4 * float(v.abs().max()) + 1e-7, k)
        elif k.startswith("b:"):
            close(sd[k[2:]].cpu(), v, 1e-4, 1e-6, k)
    m.eval()
    with torch.no_grad():
        ye, (_, ke) = m([x.detach() for x in xs])
    close(ye.cpu(), g["y_eval"], 1e-4, 1e-4 * float(g["y_eval"].abs().max()), "eval y")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cv4_chain_51_channels_vs_float64(dtype):
    """the keypoint chain of a scale-n Pose head (Conv 64->51 3x3, Conv 51->51 3x3 with training BatchNorm + SiLU, Conv2d 51->51 1x1)
    against float64 torch on the same (dtype-rounded) input: forward, input and parameter gradients, BatchNorm running statistics
    (momentum 0.03 from (0, 1), unbiased variance); the 51-channel tensors' pad lanes stay 0 and no statistic or gradient past
    channel 51 exists.  The caching allocator is first filled with NaN sentinels, so every intermediate buffer starts with NaN in its
    pad lanes: a pad lane that leaked into an output, a statistic or a gradient would show as a NaN there."""
    import dedark_yolo_amd as dy
    from dedark_yolo_amd import ops
    from dedark_yolo_amd.nn.modules import Pose
    from util import rnd
    dy.set_compute_dtype(dtype)
    torch.manual_seed(0)
    m = Pose(1, [17, 3], (64, 128, 256))
    for x in m.modules():
        if isinstance(x, torch.nn.BatchNorm2d):
            x.eps, x.momentum = 1e-3, 0.03
    ref = [[(c.conv.weight.detach().double().clone(), c.bn.weight.detach().double().clone(), c.bn.bias.detach().double().clone())
            for c in m.cv4[0][:2]], (m.cv4[0][2].weight.detach().double().clone(), m.cv4[0][2].bias.detach().double().clone())]
    m = m.cuda().train()
    m.stride = torch.tensor(STRIDES)
    xs = [rnd(300 + i, 2, c, 16 // 2 ** i, 16 // 2 ** i, lo=-1, hi=1).to(dtype) for i, c in enumerate((64, 128, 256))]
    gx = [x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for x in xs]
    torch.cuda.synchronize()
    poison = [torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda") for n in [64 << 10] * 256 + [8 << 20] * 8]   # NaN in every dtype
    torch.cuda.synchronize()
    del poison
    maps, kpt = m(gx)
    k0 = kpt[0]
    assert k0.shape[1] == 51 and ops.ld_of(k0) == ops.round_up(51, ops.vec_elems(dtype))
    cot = rnd(350, *k0.shape, lo=-1, hi=1)
    (k0.float() * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    B, _, H, W = k0.shape
    ld = ops.ld_of(k0)
    full = torch.as_strided(k0.detach(), (B, H, W, ld), (H * W * ld, W * ld, ld, 1))
    assert float(full[..., 51:].float().abs().max() if ld > 51 else 0.0) == 0.0
    # float64 torch
    x = xs[0].double().requires_grad_(True)
    t, params, zstats = x, [], []
    for w, gam, bet in ref[0]:
        w, gam, bet = w.requires_grad_(True), gam.requires_grad_(True), bet.requires_grad_(True)
        params += [w, gam, bet]
        z = F.conv2d(t, w, padding=1)
        mu, var = z.mean((0, 2, 3), keepdim=True), z.var((0, 2, 3), unbiased=False, keepdim=True)
        zstats.append((mu.detach().view(-1), z.detach().var((0, 2, 3), unbiased=True)))
        t = F.silu((z - mu) / torch.sqrt(var + 1e-3) * gam.view(1, -1, 1, 1) + bet.view(1, -1, 1, 1))
    w3, b3 = ref[1][0].requires_grad_(True), ref[1][1].requires_grad_(True)
    y = F.conv2d(t, w3, b3)
    (y * cot.double()).sum().backward()
    tol_y = 1e-5 if dtype == torch.float32 else 2e-2
    tol_g = 1e-4 if dtype == torch.float32 else 3e-2
    assert _rel_l2(k0.float(), y) <= tol_y, ("y", _rel_l2(k0.float(), y))
    assert _rel_l2(gx[0].grad.float(), x.grad) <= tol_g, ("dx", _rel_l2(gx[0].grad.float(), x.grad))
    mods = [m.cv4[0][0].conv, m.cv4[0][0].bn, m.cv4[0][1].conv, m.cv4[0][1].bn]
    got = [mods[0].weight, mods[1].weight, mods[1].bias, mods[2].weight, mods[3].weight, mods[3].bias]
    for gp, rp, name in zip(got, params, ("w0", "gamma0", "beta0", "w1", "gamma1", "beta1")):
        assert gp.grad is not None and gp.grad.shape == rp.shape, name
        assert _rel_l2(gp.grad.float(), rp.grad) <= tol_g, (name, _rel_l2(gp.grad.float(), rp.grad))
    assert _rel_l2(m.cv4[0][2].weight.grad.float(), w3.grad) <= tol_g and _rel_l2(m.cv4[0][2].bias.grad.float(), b3.grad) <= tol_g
    for bn, (mu, var_u), name in zip((mods[1], mods[3]), zstats, ("bn0", "bn1")):
        assert bn.running_mean.shape == (51,) and bn.running_var.shape == (51,), name
        rm, rv = bn.running_mean.detach().double().cpu(), bn.running_var.detach().double().cpu()
        assert _rel_l2(rm, 0.03 * mu) <= tol_g, (name, "running_mean", _rel_l2(rm, 0.03 * mu))
        assert _rel_l2((rv - 0.97) / 0.03, var_u) <= tol_g, (name, "running_var", _rel_l2((rv - 0.97) / 0.03, var_u))
    for t in [k0, gx[0].grad] + [p.grad for p in m.cv4[0].parameters()]:
        assert bool(torch.isfinite(t).all())


def _pose_model(yml, seed, nc=4):
    from oracle import model as om
    from parity_helpers import load_sd
    from types import SimpleNamespace
    from dedark_yolo_amd.nn.tasks import PoseModel
    cfg = load_yaml(yml)
    cfg["scales"]["t"] = TINY
    cfg["scale"] = "t"
    model = PoseModel(cfg, nc=nc)
    model.args = SimpleNamespace(box=7.5, cls=0.5, dfl=1.5, pose=12.0, kobj=1.0)
    load_sd(model, om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed))
    return model.cuda()


@pytest.mark.parametrize("yml,tag", [("yolov8-pose.yaml", "g17_pose_tiny"), ("yolov8-pose-p6.yaml", "g17_pose_p6_tiny")])
def test_tiny_pose_model_step_golden(yml, tag):
    """one training forward / loss / backward of a tiny pose model against the reference's: loss and items [box, pose, kobj, cls,
    dfl] within 1e-4 relative, selected gradients; then the eval output with the decoded keypoint rows."""
    g = gold(tag)
    model = _pose_model(yml, int(g["seed"])).train()
    batch = dict(img=g["img"].cuda(), batch_idx=g["batch_idx"], cls=g["cls"], bboxes=g["bboxes"], keypoints=g["keypoints"])
    loss, items = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    assert float(g["items"][1]) > 0 and items.numel() == 5
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
        y, (maps, kpt) = model(batch["img"])
    A = sum(m.shape[2] * m.shape[3] for m in maps)
    assert tuple(y.shape) == (2, 4 + 4 + 51, A) and y.dtype == torch.float32
    want = g["y"]
    err = float((y.cpu() - want).abs().max()) / float(want.abs().max())
    assert err <= 1e-4, ("eval y", err)


def _tiny_step(g, dtype, emulate=None):
    import dedark_yolo_amd as dy
    from dedark_yolo_amd import ops
    dy.set_compute_dtype(dtype)
    ops.set_storage_emulation(emulate)
    try:
        model = _pose_model("yolov8-pose.yaml", int(g["seed"])).train()
        batch = dict(img=g["img"].cuda(), batch_idx=g["batch_idx"], cls=g["cls"], bboxes=g["bboxes"], keypoints=g["keypoints"])
        loss, items = model(batch)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.set_storage_emulation(None)
        dy.set_compute_dtype(torch.float32)
    return model, float(loss), items.float().cpu()


def test_tiny_pose_model_bf16():
    """bf16 step of the tiny pose model: box, pose, kobj and dfl items within 5 % of the reference's f32 items.  The cls item (the
    unchanged detection kernels; bit-equal to the detection criterion's in test_pose_loss_vs_float64_restatement) and the total are
    bounded against an f32 run of our own model: within 5 %, or within 2.5x of how far our f32 kernels with bf16 STORAGE
    (ops.set_storage_emulation, the project's low-precision yardstick) move them.  In this random-weight model the BCE sum over every
    anchor and class amplifies the rounding of the whole forward pass: ideal bf16 storage alone moves cls by ~5 %."""
    g = gold("g17_pose_tiny")
    model, loss, got = _tiny_step(g, torch.bfloat16)
    assert bool(torch.isfinite(got).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.requires_grad)
    want = g["items"]
    for j in (0, 1, 2, 4):
        assert abs(float(got[j]) - float(want[j])) <= 5e-2 * abs(float(want[j])), (j, got.tolist(), want.tolist())
    _, loss_f, f32 = _tiny_step(g, torch.float32)
    _, loss_e, emu = _tiny_step(g, torch.float32, torch.bfloat16)
    msg = dict(bf16=got.tolist(), f32=f32.tolist(), emulated=emu.tolist(), loss=(loss, loss_f, loss_e))
    assert abs(float(f32[3]) - float(want[3])) <= 1e-4 * abs(float(want[3])), msg
    for a, b, e in ((float(got[3]), float(f32[3]), float(emu[3])), (loss, loss_f, loss_e)):
        assert abs(a - b) <= max(5e-2 * abs(b), 2.5 * abs(e - b)), msg


# ---------------------------------------------------------------------------------------------------- validation and predict
def test_kpt_oks_kernel_vs_reference():
    from dedark_yolo_amd.utils.metrics import OKS_SIGMA, kpt_iou
    g = gold("g17_pose_val")
    got = kpt_iou(g["gt_kpts"].cuda(), g["pred_kpts"].cuda(), g["area"], OKS_SIGMA)
    close(got.cpu(), g["oks"], 1e-5, 1e-6, "oks")
    got5 = kpt_iou(g["gt_kpts"][:, :5].cuda(), g["pred_kpts"][:, :5, :2].cuda(), g["area"], np.ones(5) / 5)
    close(got5.cpu(), g["oks5"], 1e-5, 1e-6, "oks k5")


def test_nms_with_keypoint_columns():
    """NMS on the box / class rows of a [B, 4+nc+51, A] Pose eval output appends each kept anchor's 51 keypoint values"""
    from dedark_yolo_amd.utils import ops as uops
    gen = np.random.default_rng(5)
    B, nc, A = 2, 3, 400
    xy = gen.uniform(20, 300, (B, 2, A))
    wh = gen.uniform(10, 80, (B, 2, A))
    scores = gen.uniform(0, 1, (B, nc, A)) ** 4
    kp = gen.uniform(0, 320, (B, 51, A))
    pred = torch.from_numpy(np.concatenate([xy, wh, scores, kp], 1).astype(np.float32)).cuda()
    dets = uops.non_max_suppression(pred, 0.25, 0.7, multi_label=True, max_det=300, nc=nc)
    base = uops.non_max_suppression(pred[:, :4 + nc].contiguous(), 0.25, 0.7, multi_label=True, max_det=300)
    for i, (d, b) in enumerate(zip(dets, base)):
        assert d.shape[1] == 6 + 51 and len(d) > 0
        assert torch.equal(d[:, :6].cpu(), b.cpu())
        cx = pred[i, 0]
        for r in d[:5]:
            a = int(torch.nonzero(torch.isclose(cx, (r[0] + r[2]) / 2, atol=1e-3, rtol=0))[0])
            assert torch.equal(r[6:].cpu(), pred[i, 4 + nc:, a].cpu())


def test_trainer_steps_save_resume_and_validate_on_a_pose_model(tmp_path):
    """three trainer steps of a tiny pose model (branch streams on), save_model, resume_training into a fresh trainer (same
    parameters), one more step: five finite loss items each step; then validate() reports box and pose metrics"""
    import bench
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    from dedark_yolo_amd.nn.tasks import PoseModel
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint
    cfgd = load_yaml("yolov8-pose.yaml")
    cfgd["scales"]["t"] = TINY
    cfgd["scale"] = "t"

    def trainer():
        torch.manual_seed(3)
        tr = DetectionTrainer(get_cfg(dict(model="tiny", dtype="fp32", optimizer="SGD", batch=64, lowlight_FLAG=False,
                                           dedark_FLAG=False, imgsz=96, deterministic=False)))
        tr.setup(PoseModel(dict(cfgd), nc=4))
        return tr

    def kbatch(seed):
        b = bench.synth_batch(seed, 4, 96, 4, "cpu")
        b["cls"] = b["cls"] % 4
        g = np.random.default_rng(seed)
        n = b["bboxes"].shape[0]
        ctr = b["bboxes"][:, None, :2].numpy()
        xy = ctr + g.uniform(-0.1, 0.1, (n, 17, 2))
        v = g.integers(0, 3, (n, 17, 1))
        b["keypoints"] = torch.from_numpy(np.concatenate([xy, v], 2).astype(np.float32))
        return b

    def step(tr, seed):
        b = kbatch(seed)
        tr.args.dark_param = b.pop("gamma")
        loss, items = tr.train_step(b, [0.01] * 3, 0.9)
        assert items.numel() == 5 and bool(torch.isfinite(items).all()) and float(items[1]) > 0
        return float(loss)

    tr = trainer()
    losses = [step(tr, 80 + i) for i in range(3)]
    torch.cuda.synchronize()
    assert all(np.isfinite(losses))
    last = tr.save_model(str(tmp_path), epoch=3, fitness=None)
    ck = load_checkpoint(last)
    assert list(ck.model_sd) == list(tr.model.state_dict())
    tr2 = trainer()
    assert tr2.resume_training(last) == 4
    torch.cuda.synchronize()
    assert float((tr2.flat.p - tr.flat.p.half().float()).abs().max()) == 0.0
    assert np.isfinite(step(tr2, 90))
    vb = kbatch(99)
    vb.pop("gamma")
    metrics, fit = tr2.validate([vb])
    for k in ("metrics/precision(P)", "metrics/recall(P)", "metrics/mAP50(P)", "metrics/mAP50-95(P)", "metrics/mAP50(B)"):
        assert k in metrics and np.isfinite(metrics[k]), k
    assert np.isfinite(fit) and abs(fit - metrics["fitness"]) < 1e-12


def test_predict_scales_keypoints_to_orig_shapes():
    """predict() keypoints against a hand-derived letterbox inverse of the eval output's decoded keypoint rows: 128x128 from
    (256, 192) is gain 0.5 and pad (16, 0), so x = (x_in - 16) / 0.5 clipped to [0, 192], y = y_in / 0.5 clipped to [0, 256]."""
    from dedark_yolo_amd.engine.model import YOLO
    y = YOLO("yolov8n-pose.yaml")
    g = gold("g17_pose_tiny")
    y.model = _pose_model("yolov8-pose.yaml", int(g["seed"]))
    y.model.model[-1].cv3[0][2].bias.data[:] = 4.0                 # confident detections
    img = g["img"][:1].cuda()
    res = y.predict(img, conf=0.25, orig_shapes=[(256, 192)])
    r = res[0]
    assert r.keypoints is not None and r.keypoints.data.shape[1:] == (17, 3) and len(r.keypoints) == len(r.boxes) > 0
    y.model.eval()
    with torch.no_grad():
        pred, _ = y.model(img)
    pred = pred[0].cpu()                                             # [4 + nc + 51, A]
    best = pred[4:8].max(0).values
    xy = pred[:4].t()
    boxes = torch.cat([xy[:, :2] - xy[:, 2:] / 2, xy[:, :2] + xy[:, 2:] / 2], 1)         # xyxy at the input size
    boxes = torch.stack([((boxes[:, 0] - 16) / 0.5).clamp(0, 192), (boxes[:, 1] / 0.5).clamp(0, 256),
                         ((boxes[:, 2] - 16) / 0.5).clamp(0, 192), (boxes[:, 3] / 0.5).clamp(0, 256)], 1)
    for det, kp in zip(r.boxes.data.cpu(), r.keypoints.data.cpu()):
        cand = torch.nonzero(best == det[4]).view(-1)                   # the kept anchor: its confidence and its box
        a = [int(c) for c in cand if torch.allclose(boxes[c], det[:4], rtol=0, atol=1e-3)]
        assert len(a) == 1, (det, cand)
        rows = pred[8:, a[0]].view(17, 3)
        want = torch.stack([((rows[:, 0] - 16) / 0.5).clamp(0, 192), (rows[:, 1] / 0.5).clamp(0, 256), rows[:, 2]], 1)
        assert torch.allclose(kp, want, rtol=0, atol=1e-4), (kp, want)
    assert float(r.keypoints.xy[..., 0].max()) <= 192 and float(r.keypoints.xy[..., 1].max()) <= 256
    assert torch.allclose(r.keypoints.xyn[..., 0] * 192, r.keypoints.xy[..., 0])
    assert r.keypoints.conf.shape == (len(r.keypoints), 17)


def test_pose_validator_end_to_end_vs_reference():
    """PoseValidator.update_metrics + get_stats against the reference validator's on the same fixed NMS outputs and batch
    (g17_pose_val_e2e: ori_shape differs from the 128x128 input, ratio_pad set, one image without predictions): the box and pose
    correct matrices, the stats columns and results_dict."""
    from types import SimpleNamespace
    from dedark_yolo_amd.engine.trainer import get_cfg
    from dedark_yolo_amd.engine.validator import PoseValidator
    g = gold("g17_pose_val_e2e")
    S, nc = int(g["S"]), int(g["nc"])
    counts = [int(v) for v in g["pred_counts"]]
    preds = [p.cuda() for p in g["preds"].split(counts, 0)]
    assert 0 in counts
    rp = g["ratio_pad"].tolist()
    batch = dict(img=torch.zeros(len(counts), 3, S, S, device="cuda"), batch_idx=g["batch_idx"], cls=g["cls"], bboxes=g["bboxes"],
                 keypoints=g["keypoints"], ori_shape=[tuple(int(v) for v in o) for o in g["ori_shape"].tolist()],
                 ratio_pad=[((r[0][0], r[0][1]), (r[1][0], r[1][1])) for r in rp])
    v = PoseValidator(get_cfg())
    v.device = torch.device("cuda")
    fake = SimpleNamespace(model=[SimpleNamespace(nc=nc, kpt_shape=[17, 3])], names={i: str(i) for i in range(nc)})
    v.init_metrics(fake)
    v.update_metrics(preds, batch)
    assert v.seen == int(g["seen"])
    stats = [torch.cat(x, 0) for x in zip(*v.stats)]
    assert torch.equal(stats[0], g["correct_b"]) and torch.equal(stats[1], g["correct_p"])
    assert g["correct_p"].any() and not g["correct_p"].all()
    for got, want in zip(stats[2:], (g["conf"], g["pcls"], g["tcls"])):
        assert torch.equal(got.float(), want.float())
    rd = v.get_stats()
    assert list(rd) == [str(k) for k in g["metric_keys"]]
    np.testing.assert_allclose(np.array(list(rd.values())), g["metric_values"].numpy(), rtol=1e-9, atol=1e-12)


def test_product_eval_equals_the_reference_running_our_pose_checkpoint():
    """g17_pose_interop: the reference loaded a tiny pose last.pt this package wrote (EMA weights, rng_fill seed 1922, half) and ran
    eval; the product on the same half-rounded weights gives the same y, decoded keypoint rows included."""
    from oracle import model as om
    from parity_helpers import load_sd
    from util import rnd
    from dedark_yolo_amd.nn.tasks import PoseModel
    g = gold("g17_pose_interop")
    cfg = load_yaml("yolov8-pose.yaml")
    cfg["scales"]["t"] = TINY
    cfg["scale"] = "t"
    model = PoseModel(cfg, nc=4)
    ema = om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, 1922)
    load_sd(model, {k: (v.half().float() if v.is_floating_point() else v) for k, v in ema.items()})
    model = model.cuda().eval()
    model.fuse()
    x = rnd(int(g["x_seed"]), 2, 3, 128, 128).pow(2.0)
    with torch.no_grad():
        y, _ = model(x.cuda())
    want = g["y"]
    assert tuple(y.shape) == tuple(want.shape) == (2, 4 + 4 + 51, 336)
    err = float((y.float().cpu() - want).abs().max()) / float(want.abs().max())
    assert err <= 1e-4, err
    kerr = float((y[:, 8:].float().cpu() - want[:, 8:]).abs().max()) / float(want[:, 8:].abs().max())
    assert kerr <= 1e-4, ("keypoint rows", kerr)
