"""GPU tests of the RepC3 variant (RepConv / RepC3 on the two-branch BatchNorm + activation kernels), modelled on
tests/test_gpu_aifi.py and with its tolerances for the same quantities.

Blocks (fp32) against the reference's fixtures g31_repc3_<block>_<train|eval|fused> (tests/golden/make_repc3_golden.py): outputs
within 1e-4, input and parameter gradients within 2e-3 (test_gpu_parity._run_block's bounds), running buffers within 1e-4; after
fuse_convs() the fused weights and the eval output.  A RepC3 writing into a channel slice with live neighbours.  The whole
yolov8n-RepC3 model at 64x64 against g31_repc3_n_tiny: loss and items within 1e-4, gradients (both branches of a RepConv among
them), running statistics and the three eval maps; fuse() re-parameterises every RepConv and its output stays within
1e-4 max|y| of the unfused one and of the reference's own fused output.  Two trainer steps in fp32, bf16 and fp16 are finite and,
run twice, give identical parameter bytes; one step at scale l.  val() on a 64 x 96 rect batch, predict(augment=True), the last.pt
round trip, and the reference's own eval output of a last.pt written here (g31_repc3_interop).
"""
import numpy as np
import pytest
import torch

from util import close, gold, load_yaml, make_batch, rnd

pytestmark = pytest.mark.gpu

TOL_Y, TOL_G = 1e-4, 2e-3          # test_gpu_parity._run_block
YAML = "yolov8-RepC3.yaml"
BLOCKS = {"repconv16": ("RepConv", (16, 16), {}), "repconv64_id": ("RepConv", (64, 64), dict(act=False)),
          "repc3_32_64n1": ("RepC3", (32, 64, 1), {}), "repc3_64n2": ("RepC3", (64, 64, 2), {})}


@pytest.fixture(autouse=True)
def _fp32():
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(torch.float32)
    yield
    dy.set_compute_dtype(torch.float32)


def _cfg(scale="n"):
    d = load_yaml(YAML)
    d["scale"] = scale
    return d


def _block(name, g):
    from oracle import model as om
    from parity_helpers import load_sd, set_bn
    from dedark_yolo_amd.nn import modules
    cls, args, kw = BLOCKS[name]
    m = set_bn(getattr(modules, cls)(*args, **kw))
    load_sd(m, om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"])))
    return m.cuda()


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_train_golden(name):
    g = gold(f"g31_repc3_{name}_train")
    m = _block(name, g).train()
    x = g["x0"].clone().cuda().requires_grad_(True)
    y = m(x)
    close(y.detach().float().cpu(), g["y0"], TOL_Y, TOL_Y, f"{name} y")
    (y.float() * rnd(900, *y.shape, lo=-1, hi=1).cuda()).sum().backward()
    torch.cuda.synchronize()
    close(x.grad.float().cpu(), g["dx0"], TOL_G, TOL_G, f"{name} dx")
    from dedark_yolo_amd import ops
    ops.flush_bn_counters()                 # num_batches_tracked is bumped lazily; a model's state_dict() does this itself
    named, sd, n = dict(m.named_parameters()), m.state_dict(), 0
    for k, v in g.items():
        if k.startswith("g:"):
            close(named[k[2:]].grad.cpu(), v, TOL_G, TOL_G, f"{name} {k}")
            n += 1
        elif k.startswith("gn:"):
            close(named[k[3:]].grad.norm().cpu(), v, TOL_G, 1e-4, f"{name} {k}")
            n += 1
        elif k.startswith("b:"):
            close(sd[k[2:]].cpu(), v, 1e-4, 1e-4, f"{name} {k}")
    assert n == len(named)                  # every parameter: the conv weight, gamma and beta of both branches of every RepConv
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_eval_and_fused_golden(name):
    g, f = gold(f"g31_repc3_{name}_eval"), gold(f"g31_repc3_{name}_fused")
    m = _block(name, g).eval()
    x = g["x0"].cuda()
    with torch.no_grad():
        y = m(x)
    close(y.float().cpu(), g["y0"], TOL_Y, TOL_Y, f"{name} eval y")
    for k, v in g.items():
        if k.startswith("b:"):
            assert torch.equal(m.state_dict()[k[2:]].cpu(), v), k
    for r in m.modules():
        if hasattr(r, "fuse_convs"):
            r.fuse_convs()
            assert [k for k, _ in r.named_children()] == ["act", "conv"]
    sd = m.state_dict()
    for k, v in f.items():
        if k.startswith("w:"):
            close(sd[k[2:]].cpu(), v, 1e-5, 1e-6, f"{name} {k}")
        elif k.startswith("w4:"):
            close(sd[k[3:]][:4].cpu(), v, 1e-5, 1e-6, f"{name} {k}")
    with torch.no_grad():
        yf = m(x)
    close(yf.float().cpu(), f["y0"], TOL_Y, TOL_Y, f"{name} fused y")
    assert float((yf - y).abs().max()) <= 1e-4 * float(y.abs().max())


def test_block_writes_into_a_slice_with_live_neighbours():
    """out= (the graph places row 12 inside the Concat buffer of row 17): the result is the plain call's, the sibling channels stay;
    in train mode too, where the last kernel is cv2's BatchNorm pass with m(cv1(x)) as its residual"""
    from dedark_yolo_amd import ops
    g = gold("g31_repc3_repc3_32_64n1_eval")
    x = g["x0"].cuda()
    B, _, H, W = x.shape
    C = 64
    for train in (False, True):
        buf = ops.empty_nhwc(B, C + 32, H, W, torch.float32, x.device)
        buf.fill_(7.0)
        with torch.no_grad():
            y0 = _block("repc3_32_64n1", g).train(train)(x)
            y1 = _block("repc3_32_64n1", g).train(train)(x, out=buf[:, 24:24 + C])
        assert torch.equal(buf[:, 24:24 + C], y0) and y1.data_ptr() == buf[:, 24:24 + C].data_ptr()
        assert bool((buf[:, :24] == 7.0).all()) and bool((buf[:, 24 + C:] == 7.0).all())


def _model_step(name, dtype=torch.float32):
    import dedark_yolo_amd as dy
    from oracle import model as om
    from parity_helpers import HYP, load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    g = gold(name)
    dy.set_compute_dtype(dtype)
    model = DetectionModel(_cfg("n"), ch=3, nc=20)
    model.args = HYP
    load_sd(model, om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, int(g["seed"])))
    model = model.cuda().train()
    batch = make_batch(int(g["seed"]) + 1, int(g["B"]), int(g["S"]), [int(v) for v in g["nbox"]])
    batch["img"] = batch["img"].pow(3.0).cuda()
    batch["recovery_loss_batch"] = torch.tensor(0.0123).cuda()
    loss, items = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    return g, model, batch, loss, items


def test_repc3_model_step_golden():
    from dedark_yolo_amd.nn.modules import RepConv
    name = "g31_repc3_n_tiny"
    g, model, batch, loss, items = _model_step(name)
    print(f"{name}: loss {float(loss.detach()):.6f} vs {float(g['loss']):.6f}")
    close(float(loss.detach()), g["loss"], 1e-4, 1e-4, f"{name} loss vs reference golden")
    close(items.float().cpu(), g["items"], 1e-4, 1e-4, f"{name} items vs reference golden")
    named = dict(model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in named.values() if p.requires_grad)
    gtol, msd, n_rep = 5e-3, model.state_dict(), 0
    for k, v in g.items():
        if k.startswith("gn:"):
            close(named[k[3:]].grad.norm().cpu(), v, gtol, 1e-6, f"{name} {k}")
            n_rep += "model.15." in k
        elif k.startswith("g:"):
            close(named[k[2:]].grad.cpu(), v, gtol, gtol * float(v.abs().max()), f"{name} {k}")
            n_rep += "model.15." in k
        elif k.startswith("b:"):
            close(msd[k[2:]].cpu(), v, 1e-4, 1e-4, f"{name} {k}")
    assert n_rep == 12 and "g:model.15.m.0.conv1.bn.weight" in g and "g:model.15.m.0.conv2.bn.weight" in g
    model.eval()
    with torch.no_grad():
        out = model(batch["img"])
    y, maps = out[0], out[1]
    assert abs(float(y.float().sum()) - float(g["ysum"])) <= 1e-4 * float(y.float().abs().sum())
    for i in range(3):
        want = g[f"map{i}"]
        err = float((maps[i].float().cpu() - want).abs().max()) / float(want.abs().max())
        assert maps[i].shape == want.shape and err <= 1e-4, (i, err)
    assert not model.is_fused()
    model.fuse()
    reps = [m for m in model.modules() if isinstance(m, RepConv)]
    assert len(reps) == 4 and all([k for k, _ in r.named_children()] == ["act", "conv"] == [str(s) for s in g["fused_children"]] for r in reps)
    assert model.is_fused()
    with torch.no_grad():
        yf = model(batch["img"])[0]
    assert float((yf.float() - y.float()).abs().max()) <= 1e-4 * float(y.abs().max())     # test_gpu_ghost.py's fuse tolerance
    want = g["y_fused"]
    assert float((yf.float().cpu() - want).abs().max()) <= 1e-4 * float(want.abs().max())


def test_product_eval_equals_the_reference_running_our_checkpoint():
    """the reference loaded a last.pt written by this package (make_repc3_golden.py interop); its eval output, unfused and after its
    own fuse(), is the product's on the same half-rounded weights"""
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    g = gold("g31_repc3_interop")
    model = DetectionModel(_cfg("n"), nc=20)
    ema = om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, 3162)
    load_sd(model, {k: (v.half().float() if v.is_floating_point() else v) for k, v in ema.items()})
    model = model.cuda().eval()
    x = rnd(int(g["x_seed"]), 2, 3, 64, 64).pow(2.0)
    for key in ("y", "y_fused"):
        with torch.no_grad():
            y = model(x.cuda())
        y = y[0] if isinstance(y, (list, tuple)) else y
        want = g[key]
        err = float((y.float().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)
        assert y.shape == want.shape and err <= 1e-4, (key, err)
        model.fuse()


def _trainer(dtype, steps=2, name="yolov8n-RepC3.yaml"):
    import bench
    from dedark_yolo_amd import YOLO
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    torch.manual_seed(3)
    tr = DetectionTrainer(get_cfg(dict(model=name, dtype=dtype, optimizer="SGD", batch=2, lowlight_FLAG=False, dedark_FLAG=False)))
    tr.setup(YOLO(name).model)
    trp = [(k, p) for k, p in tr.model.named_parameters() if k.startswith("model.12.")]
    assert len(trp) == 6 + 6 * len(tr.model.model[12].m) and all(getattr(p, "_dy_direct", False) for _, p in trp)
    losses = []
    for step in range(steps):
        b = bench.synth_batch(80 + step, 2, 64, 20, "cuda")
        tr.args.dark_param = b.pop("gamma")
        b.pop("n_max", None)
        for _, p in trp:
            p.grad.fill_(float("nan"))           # the kernels overwrite the slots of the flat gradient buffer: one that is skipped stays NaN
        loss, _ = tr.train_step(b, [0.01] * 3, 0.9)
        torch.cuda.synchronize()
        losses.append(float(loss))
        for k, p in trp:                         # every parameter of the block received a gradient, both branches of every RepConv
            assert bool(torch.isfinite(p.grad).all()), k
            assert float(p.grad.abs().max()) > 0.0, k
    return tr, losses


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_two_training_steps_are_finite_and_deterministic(dtype):
    tr, losses = _trainer(dtype)
    assert all(np.isfinite(v) for v in losses), losses
    assert bool(torch.isfinite(tr.flat.p).all()) and bool(torch.isfinite(tr.flat.g).all())
    p1, g1 = tr.flat.p.clone(), tr.flat.g.clone()
    tr2, losses2 = _trainer(dtype)
    assert losses2 == losses and torch.equal(p1, tr2.flat.p) and torch.equal(g1, tr2.flat.g), "two identical runs must give identical bytes"


def test_l_scale_trains_one_step():
    """yolov8l-RepC3 (width 512, three RepConv per block) in bf16: one finite trainer step"""
    tr, losses = _trainer("bf16", steps=1, name="yolov8l-RepC3.yaml")
    assert np.isfinite(losses[0]) and bool(torch.isfinite(tr.flat.p).all())


def test_last_pt_round_trip(tmp_path):
    """last.pt of yolov8n-RepC3 in the reference's format, read back by our reader: same keys, the trained weights at half precision,
    and a model built from the file gives, bit for bit, the eval output of those weights"""
    from dedark_yolo_amd.nn.tasks import DetectionModel
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint
    tr, _ = _trainer("fp32", steps=1)
    last = tr.save_model(str(tmp_path / "w"), epoch=0, fitness=0.1)
    ck = load_checkpoint(last)
    assert ck.source == "reference-pickle" and (tmp_path / "w" / "best.pt").exists()
    assert list(ck.model_sd) == list(tr.model.state_dict())
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(torch.float32)
    x = rnd(91, 2, 3, 64, 64).pow(2.0).cuda()

    def eval_of(sd):
        m = DetectionModel(_cfg("n"), nc=20)
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        with torch.no_grad():
            y = m(x)
        return (y[0] if isinstance(y, (list, tuple)) else y).clone()
    trained = {k: (v.detach().cpu().half().float() if v.is_floating_point() else v.detach().cpu()) for k, v in tr.model.state_dict().items()}
    y_file, y_mem = eval_of(ck.model_sd), eval_of(trained)
    assert bool(torch.isfinite(y_file).all()) and torch.equal(y_file, y_mem)


def _yolo(seed):
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.engine.model import YOLO
    yolo = YOLO("yolov8n-RepC3.yaml")
    load_sd(yolo.model, om.rng_fill({k: tuple(v.shape) for k, v in yolo.model.state_dict().items()}, seed))
    yolo.model = yolo.model.cuda().eval()
    return yolo


def test_val_on_a_rect_batch():
    """val() on 64 x 96 images: the RepC3 rows run on 8 x 12, 4 x 6 and 2 x 3 maps"""
    yolo = _yolo(3171)
    S, B = (64, 96), 2
    gen = np.random.default_rng(3172)
    img = torch.from_numpy((gen.random((B, 3, *S)) * 255).astype(np.uint8))
    loader = [dict(img=img, batch_idx=torch.tensor([0.0, 1.0]), cls=torch.tensor([[3.0], [7.0]]),
                   bboxes=torch.tensor([[0.5, 0.5, 0.3, 0.4], [0.4, 0.6, 0.2, 0.2]]), ori_shape=[S] * B)]
    with torch.no_grad():
        y = yolo.model((img.float() / 255).cuda())[0]
    assert y.shape == (B, 24, 8 * 12 + 4 * 6 + 2 * 3) and bool(torch.isfinite(y).all())
    stats = yolo.val(loader, conf=0.001, iou=0.7)
    assert "metrics/mAP50(B)" in stats and all(np.isfinite(v) for v in stats.values())


def test_predict_augment():
    """predict(augment=True): the scaled / flipped passes put other map sizes through the blocks"""
    yolo = _yolo(3173)
    x = rnd(3174, 2, 3, 128, 128).cuda()
    with torch.no_grad():
        merged = yolo.model(x, augment=True)[0]
        plain = yolo.model(x)[0]
    assert merged.shape[0] == 2 and merged.shape[-1] > plain.shape[-1] and bool(torch.isfinite(merged).all())
    res = yolo.predict(x, conf=0.001, augment=True)
    assert len(res) == 2 and all(bool(torch.isfinite(r.boxes.data).all()) for r in res)
