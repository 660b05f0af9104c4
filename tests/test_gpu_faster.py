"""GPU tests of the FasterNet variants: the PConv kernels (dy_pconv_fwd / dgrad / wgrad through ctypes) against torch F.conv2d,
FasterC2f_N / FasterC2f blocks and whole Faster models against the reference's fixtures (tests/golden/make_faster_golden.py), the
16-bit paths, a trainer step with its checkpoint, and the product's eval output on the reference's reading of our checkpoint."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import close, gold, load_yaml, make_batch, rnd

pytestmark = pytest.mark.gpu

C3S = [4, 8, 12, 16, 20, 24, 32, 40, 48, 64, 72, 80, 128]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
LPAD, RPAD = 3, 5          # foreign lanes on each side of the C-channel views (live neighbours in a concat buffer)


@pytest.fixture(autouse=True)
def _fp32():
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(torch.float32)
    yield
    dy.set_compute_dtype(torch.float32)


def _wide(B, H, W, C, dtype, fill, seed):
    """[B, C, H, W] view into a [B, H, W, LPAD + C + RPAD] buffer: view = uniform(-1, 1) (or `fill`), left lanes NaN, right lanes +inf"""
    buf = torch.empty((B, H, W, LPAD + C + RPAD), dtype=dtype, device="cuda")
    buf[..., :LPAD] = float("nan")
    buf[..., LPAD + C:] = float("inf")
    v = buf[..., LPAD:LPAD + C]
    v.copy_(rnd(seed, B, H, W, C, lo=-1, hi=1) if fill is None else torch.full((B, H, W, C), fill))
    return buf, v.permute(0, 3, 1, 2)


def _sentinels_intact(buf, C):
    return bool(torch.isnan(buf[..., :LPAD]).all()) and bool(torch.isposinf(buf[..., LPAD + C:]).all())


def _call(name, *args):
    from dedark_yolo_amd import _C, ops
    _C.lib().dy_clear_last_kernel()
    _C.call(name, *args, ops.stream())
    return _C.lib().dy_last_kernel().decode()


def _tol(dtype):
    return {torch.float32: 2e-5, torch.bfloat16: 1.6e-2, torch.float16: 2e-3}[dtype]


def _check(got, want, dtype, what):
    got, want = got.double().cpu(), want.double().cpu()
    t = _tol(dtype)
    err = float((got - want).abs().max())
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    assert err <= t * (float(want.abs().max()) + 1.0), f"{what}: max abs err {err:.3e} (ref max {float(want.abs().max()):.3e})"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("c3", C3S)
def test_pconv_kernels_vs_torch(c3, dtype):
    from dedark_yolo_amd import ops
    C = 4 * c3 + (c3 % 3)                      # c3 = C // 4 with C not always a multiple of 4
    # odd sizes with partial MFMA tiles both ways: W = 9 / 37 take 16-column tiles, W = 31 32-column ones
    B, H, W = {16: (2, 11, 37), 64: (2, 11, 31), 128: (2, 5, 31)}.get(c3, (2, 7, 9))
    did = ops.dt_id(dtype)
    ref_dt = torch.float64 if dtype == torch.float32 else torch.float32
    w = (rnd(7 + c3, c3, c3, 3, 3, lo=-1, hi=1) / (3.0 * c3 ** 0.5)).cuda()
    xb, x = _wide(B, H, W, C, dtype, None, 1 + c3)
    yb, y = _wide(B, H, W, C, dtype, 0.0, 0)
    xr = x.to(ref_dt)
    mfma = dtype != torch.float32 and c3 >= 16             # the 16-bit MFMA route; fp32 and c3 < 16 run the VALU kernel
    kname = "pconv_mfma_kernel<" if mfma else "pconv_kernel<"
    wp = wpt = None
    if mfma:
        n_wp = 9 * ((c3 + 31) // 32) * ((c3 + 15) // 16) * 512
        wp, wpt = torch.empty(n_wp, dtype=dtype, device="cuda"), torch.empty(n_wp, dtype=dtype, device="cuda")
        assert _call("dy_pconv_pack", w.data_ptr(), wp.data_ptr(), c3, 0, did) == "pconv_pack_kernel"
        _call("dy_pconv_pack", w.data_ptr(), wpt.data_ptr(), c3, 1, did)
    pw, pwt = (wp.data_ptr(), wpt.data_ptr()) if mfma else (None, None)
    k = _call("dy_pconv_fwd", x.data_ptr(), ops.ld_of(x), y.data_ptr(), ops.ld_of(y), w.data_ptr(), pw, B, H, W, C, c3, did)
    assert k.startswith(kname), k
    torch.cuda.synchronize()
    want = torch.cat([F.conv2d(xr[:, :c3], w.to(ref_dt), padding=1), xr[:, c3:]], 1)
    _check(y, want, dtype, f"fwd c3={c3}")
    assert torch.equal(y[:, c3:], x[:, c3:]), "pass-through lanes must be copied exactly"
    assert _sentinels_intact(yb, C) and _sentinels_intact(xb, C)

    # data gradient: plain, then accumulate + add_src into a slice that already holds values
    gb, g = _wide(B, H, W, C, dtype, None, 100 + c3)
    sb, s = _wide(B, H, W, C, dtype, None, 200 + c3)
    db, dx = _wide(B, H, W, C, dtype, None, 300 + c3)
    gr = g.to(ref_dt)
    dconv = torch.nn.grad.conv2d_input((B, c3, H, W), w.to(ref_dt), gr[:, :c3], padding=1)
    base = torch.cat([dconv, gr[:, c3:]], 1)
    before = dx.to(ref_dt).clone()
    _call("dy_pconv_dgrad", g.data_ptr(), ops.ld_of(g), y.data_ptr(), ops.ld_of(y), w.data_ptr(), pwt, B, H, W, C, c3, 0, None, 0, did)
    torch.cuda.synchronize()
    _check(y, base, dtype, f"dgrad c3={c3}")
    k = _call("dy_pconv_dgrad", g.data_ptr(), ops.ld_of(g), dx.data_ptr(), ops.ld_of(dx), w.data_ptr(), pwt, B, H, W, C, c3, 1,
              s.data_ptr(), ops.ld_of(s), did)
    assert k.startswith(kname), k
    torch.cuda.synchronize()
    _check(dx, before + base + s.to(ref_dt), dtype, f"dgrad accumulate+add_src c3={c3}")
    for b_ in (gb, sb, db, yb):
        assert _sentinels_intact(b_, C)

    # weight gradient: f32, deterministic
    scratch = torch.empty(1 << 22, dtype=torch.float32, device="cuda")
    dw1 = torch.full((c3, c3, 3, 3), float("nan"), device="cuda")
    dw2 = torch.full((c3, c3, 3, 3), float("nan"), device="cuda")
    for dw in (dw1, dw2):
        k = _call("dy_pconv_wgrad", x.data_ptr(), ops.ld_of(x), g.data_ptr(), ops.ld_of(g), dw.data_ptr(), B, H, W, c3,
                  scratch.data_ptr(), scratch.numel(), did)
        assert k.startswith("pconv_wgrad_kernel<"), k
    torch.cuda.synchronize()
    want = torch.nn.grad.conv2d_weight(xr[:, :c3], (c3, c3, 3, 3), gr[:, :c3], padding=1)
    t = 2e-5 if dtype == torch.float32 else 1e-4
    err = float((dw1.double().cpu() - want.double().cpu()).abs().max())
    assert err <= t * (float(want.abs().max()) + 1.0), f"wgrad c3={c3}: {err:.3e}"
    assert torch.equal(dw1, dw2), "weight gradient must be bit-identical run to run"


def test_pconv_wgrad_many_chunks_is_deterministic_and_exact():
    """A map big enough to split the pixels over many chunks (and a scratch that caps their number)."""
    from dedark_yolo_amd import ops
    c3, C, B, H, W = 24, 96, 4, 65, 63
    xb, x = _wide(B, H, W, C, torch.float32, None, 5)
    gb, g = _wide(B, H, W, C, torch.float32, None, 6)
    want = torch.nn.grad.conv2d_weight(x[:, :c3].double(), (c3, c3, 3, 3), g[:, :c3].double(), padding=1)
    outs = []
    for elems in (1 << 22, 9 * c3 * c3 * 3):
        scratch = torch.empty(elems, dtype=torch.float32, device="cuda")
        for _ in range(2):
            dw = torch.empty((c3, c3, 3, 3), device="cuda")
            _call("dy_pconv_wgrad", x.data_ptr(), ops.ld_of(x), g.data_ptr(), ops.ld_of(g), dw.data_ptr(), B, H, W, c3,
                  scratch.data_ptr(), scratch.numel(), 0)
            outs.append(dw)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3])
    for o in (outs[0], outs[2]):
        assert float((o.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_pconv_rejects_bad_arguments():
    from dedark_yolo_amd import _C, ops
    x = torch.zeros((1, 8, 8, 600), device="cuda")
    w = torch.zeros((150, 150, 3, 3), device="cuda")
    with pytest.raises(RuntimeError, match="c3"):
        _C.call("dy_pconv_fwd", x.data_ptr(), 600, x.data_ptr() + 4, 600, w.data_ptr(), None, 1, 8, 8, 600, 150, 0, ops.stream())
    xb = x.to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="packed weights"):          # the 16-bit route has no silent fallback
        _C.call("dy_pconv_fwd", xb.data_ptr(), 600, xb.data_ptr() + 16, 600, w.data_ptr(), None, 1, 8, 8, 600, 32, 1, ops.stream())
    # source and destination lanes that overlap inside one buffer (in place, or halves cut 4 lanes too close) are refused and launch
    # nothing: a thread reads the 3x3 halo that other threads write.  Sibling halves are fine.
    buf = rnd(21, 1, 8, 8, 16, lo=-1, hi=1).cuda()
    w2 = (rnd(22, 2, 2, 3, 3, lo=-1, hi=1) / 4.0).cuda()
    a, b_, c = buf[..., :8], buf[..., 4:12], buf[..., 8:]
    for dst in (a, b_):
        for name, tail in (("dy_pconv_fwd", (0,)), ("dy_pconv_dgrad", (0, None, 0, 0))):
            src, dst_ = (a, dst) if name == "dy_pconv_fwd" else (dst, a)
            _C.lib().dy_clear_last_kernel()
            with pytest.raises(RuntimeError, match="overlap"):
                _C.call(name, src.data_ptr(), 16, dst_.data_ptr(), 16, w2.data_ptr(), None, 1, 8, 8, 8, 2, *tail, ops.stream())
            assert _C.lib().dy_last_kernel().decode() == ""
    xa = a.permute(0, 3, 1, 2).double()
    want = torch.cat([F.conv2d(xa[:, :2], w2.double(), padding=1), xa[:, 2:]], 1)
    assert _call("dy_pconv_fwd", a.data_ptr(), 16, c.data_ptr(), 16, w2.data_ptr(), None, 1, 8, 8, 8, 2, 0).startswith("pconv_kernel<")
    torch.cuda.synchronize()
    _check(c.permute(0, 3, 1, 2), want, torch.float32, "fwd into the sibling half")
    assert torch.equal(a.permute(0, 3, 1, 2).double(), xa)
    g = c.permute(0, 3, 1, 2).double()
    want = torch.cat([torch.nn.grad.conv2d_input((1, 2, 8, 8), w2.double(), g[:, :2], padding=1), g[:, 2:]], 1)
    _call("dy_pconv_dgrad", c.data_ptr(), 16, a.data_ptr(), 16, w2.data_ptr(), None, 1, 8, 8, 8, 2, 0, None, 0, 0)
    torch.cuda.synchronize()
    _check(a.permute(0, 3, 1, 2), want, torch.float32, "dgrad into the sibling half")
    assert torch.equal(c.permute(0, 3, 1, 2).double(), g)


@pytest.mark.parametrize("name,cls,args", [("g14_fasterc2f_n_sc", "FasterC2f_N", (32, 32, 2, True)),
                                           ("g14_fasterc2f_n_nosc", "FasterC2f_N", (48, 32, 1, False)),
                                           ("g14_fasterc2f_n_c6", "FasterC2f_N", (48, 48, 1, True)),
                                           ("g14_fasterc2f_sc", "FasterC2f", (32, 32, 2, True)),
                                           ("g14_fasterc2f_nosc", "FasterC2f", (48, 32, 1, False))])
def test_faster_blocks_golden(name, cls, args):
    from test_gpu_parity import _run_block
    from dedark_yolo_amd.nn import modules
    _run_block(name, getattr(modules, cls)(*args))


@pytest.mark.parametrize("fused", [False, True], ids=["eval", "eval_fused"])
def test_faster_block_eval_matches_torch(fused):
    """eval / no_grad path (BN folded into the conv epilogue, shortcut added after the last 1x1) equals the block computed with torch
    ops in float64 on the same weights -- also after DetectionModel.fuse() has cached the folded affines."""
    from oracle import model as om
    from parity_helpers import load_sd, set_bn
    from dedark_yolo_amd.nn.modules import FasterC2f_N
    g = gold("g14_fasterc2f_n_sc")
    m = FasterC2f_N(32, 32, 2, True)
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
    # the same block by torch ops (eval BN) on the same weights
    xt = g["x0"].double()
    sd = {k: v.double() for k, v in ref.items()}

    def conv_bn(t, p, k):
        z = F.conv2d(t, sd[p + "conv.weight"], padding=k // 2)
        sc = sd[p + "bn.weight"] / torch.sqrt(sd[p + "bn.running_var"] + 1e-3)
        z = (z - sd[p + "bn.running_mean"].view(1, -1, 1, 1)) * sc.view(1, -1, 1, 1) + sd[p + "bn.bias"].view(1, -1, 1, 1)
        return F.silu(z)
    t = conv_bn(xt, "cv1.", 1)
    ys = list(t.split(16, 1))
    for i in range(2):
        u = ys[-1]
        p = f"m.{i}.fasterblock."
        u1 = torch.cat([F.conv2d(u[:, :4], sd[p + "0.patial_conv3.weight"], padding=1), u[:, 4:]], 1)
        u2 = conv_bn(u1, p + "1.", 1)
        ys.append(u + F.conv2d(u2, sd[p + "2.weight"]))
    want = conv_bn(torch.cat(ys, 1), "cv2.", 1)
    close(y.double().cpu(), want, 1e-4, 1e-4, "FasterC2f_N eval")


def _faster_model(yaml_name, scale, scale_def, seed, nc=20):
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
    model = _faster_model(yaml_name, scale, sdef, int(g["seed"])).train()
    batch = make_batch(int(g["seed"]) + 1, int(g["B"]), int(g["S"]), [int(v) for v in g["nbox"]])
    batch["img"] = batch["img"].pow(3.0).cuda()
    batch["recovery_loss_batch"] = torch.tensor(0.0123).cuda()
    loss, items = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    return g, model, batch, loss, items


@pytest.mark.parametrize("name,yml,scale", [("g14_faster_n_tiny", "yolov8-Faster-2.0.yaml", "t"),
                                            ("g14_faster3_l", "yolov8-Faster3.0-twohead.yaml", "l")])
def test_faster_model_step_golden(name, yml, scale):
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
        y = model(batch["img"])
    y = y[0] if isinstance(y, (list, tuple)) else y
    ytol = 1e-4 if scale == "t" else 2e-2
    err = float((y[:, :, ::7].float().cpu() - g["y"]).abs().max()) / float(g["y"].abs().max())
    assert err <= ytol, err


def _grads(m):
    return torch.cat([p.grad.double().flatten() for p in m.parameters() if p.requires_grad])


def _cos(a, b):
    return float((a @ b) / (a.norm() * b.norm()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_faster_model_low_precision(dtype):
    """16-bit runs of yolov8n-Faster-2.0 (tiny): finite, loss within 2 % of the reference's fp32 golden, and the gradient as close
    in direction to the fp32 path's as the fp32 kernels with 16-bit STORAGE get (ops.set_storage_emulation: the rounding any 16-bit
    implementation has, the project's low-precision yardstick; tests/test_gpu_lowprec.py)."""
    from dedark_yolo_amd import ops
    g, m16, _, loss, items = _model_step("g14_faster_n_tiny", "yolov8-Faster-2.0.yaml", "t", dtype)
    assert torch.isfinite(loss) and bool(torch.isfinite(items).all())
    assert abs(float(loss) - float(g["loss"])) <= 2e-2 * abs(float(g["loss"])), (float(loss), float(g["loss"]))
    a = _grads(m16)
    assert bool(torch.isfinite(a).all())
    _, m32, _, _, _ = _model_step("g14_faster_n_tiny", "yolov8-Faster-2.0.yaml", "t", torch.float32)
    ops.set_storage_emulation(dtype)
    try:
        _, memu, _, _, _ = _model_step("g14_faster_n_tiny", "yolov8-Faster-2.0.yaml", "t", torch.float32)
    finally:
        ops.set_storage_emulation(None)
    b, e = _grads(m32), _grads(memu)
    cos, cos_emu = _cos(a, b), _cos(e, b)
    print(f"{dtype}: gradient cosine vs fp32 {cos:.4f}, 16-bit storage emulation {cos_emu:.4f}")
    assert cos >= min(cos_emu, 0.95) - 0.03, (cos, cos_emu)


@pytest.mark.parametrize("tag,name,scale", [("f2_t", "yolov8-Faster-2.0.yaml", "t"), ("f3_l", "yolov8-Faster3.0-twohead.yaml", "l")])
def test_product_eval_equals_the_reference_running_our_faster_checkpoint(tag, name, scale):
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    g = gold("g14_faster_interop")
    cfg = load_yaml(name)
    cfg["scales"]["t"] = [0.33, 0.125, 1024]
    cfg["scale"] = scale
    model = DetectionModel(cfg, nc=20)
    ema = om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, 1422)
    load_sd(model, {k: (v.half().float() if v.is_floating_point() else v) for k, v in ema.items()})
    model = model.cuda().eval()
    model.fuse()
    x = rnd(int(g[f"{tag}_x_seed"]), 2, 3, 64, 64).pow(2.0)
    with torch.no_grad():
        y = model(x.cuda())
    y = y[0] if isinstance(y, (list, tuple)) else y
    want = g[f"{tag}_y"]
    err = float((y.float().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)
    assert y.shape == want.shape and err <= 1e-4, err


def test_trainer_step_and_checkpoint_on_a_faster_model(tmp_path):
    """One trainer step of yolov8-Faster-2.0 (tiny) with the wgrad side stream on, then save_model writes last.pt / best.pt in the
    reference's format and the reader gets the same state back."""
    import bench
    import dedark_yolo_amd as dy
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    from dedark_yolo_amd.nn.tasks import DetectionModel
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint
    dy.set_compute_dtype(torch.float32)
    cfgd = load_yaml("yolov8-Faster-2.0.yaml")
    cfgd["scales"]["t"] = [0.33, 0.125, 1024]
    cfgd["scale"] = "t"
    torch.manual_seed(3)
    tr = DetectionTrainer(get_cfg(dict(model="tiny", dtype="fp32", optimizer="SGD", batch=64, lowlight_FLAG=False, dedark_FLAG=False)))
    tr.setup(DetectionModel(cfgd, nc=20))
    losses = []
    for i in range(2):
        b = bench.synth_batch(80 + i, 4, 96, 20, "cuda")
        tr.args.dark_param = b.pop("gamma")
        b.pop("n_max", None)
        loss, _ = tr.train_step(b, [0.01] * 3, 0.9)
        losses.append(float(loss))
    torch.cuda.synchronize()
    assert all(np.isfinite(losses))
    assert bool(torch.isfinite(tr.flat.p).all()) and bool(torch.isfinite(tr.flat.g).all())
    last = tr.save_model(str(tmp_path), epoch=0, fitness=0.1)
    ck = load_checkpoint(last)
    assert ck.source == "reference-pickle" and (tmp_path / "best.pt").exists()
    assert list(ck.model_sd) == list(tr.model.state_dict())
    assert sum(len(gr["params"]) for gr in ck.optimizer["param_groups"]) == len(tr.flat.slots)
