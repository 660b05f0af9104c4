"""GPU tests of the CBAM variants at module and model level (ChannelAttention / SpatialAttention / CBAM on the kernels of
csrc/cbam.hip), modelled on tests/test_gpu_repc3.py.

Blocks (fp32) against the reference's fixtures g33_cbam_<block>_<train|eval> (tests/golden/make_cbam_golden.py): output, input
gradient and every parameter gradient, each measured as max |got - fixture| / max |fixture|.  The allowance is 4 E, E being the
largest such figure, over the block's arrays, of the fixture itself (the formula evaluated by torch in f32 on the CPU) against the
float64 statement tests/cbam_ref.py: a kernel may be four times as far from the f32 run as that run is from the truth.  Every
figure is printed.  The fixtures' seeds keep the two largest channels of every pixel at least 1e-4 max|u| apart, so no element is
left out.

Models (fp32) against g33_cbam_n_tiny (64 x 64), g33_cbam_n_rect (64 x 96) and g33_cbam_ll_n_tiny (yolov8n-lowlight-CBAM, 64 x 64)
with tests/test_gpu_repc3.py's tolerances for the same quantities: loss and items within 1e-4, gradients (the three blocks' among
them) within 5e-3, running statistics within 1e-4, the eval maps within 1e-4 max|map|.  A CBAM row writing into a Concat slice with
a live sibling; trainer steps in fp32, bf16 and fp16 (finite, every block parameter's gradient written, identical bytes when run
twice), one step of yolov8l-lowlight-CBAM in each of the three dtypes, the lowlight graph with a `filters:` key; val() on a rect batch, predict() and predict(augment=True), the last.pt round trip and
the reference's own eval output of a last.pt written here (g33_cbam_interop).
"""
import numpy as np
import pytest
import torch

import cbam_ref as cr
from util import close, gold, load_yaml, make_batch, rnd

pytestmark = pytest.mark.gpu

YAMLS = {"": "yolov8-CBAM.yaml", "ll_": "yolov8-lowlight-CBAM.yaml"}
BLOCKS = {"cbam16_k7": ("cbam", "CBAM", (16, 7)), "cbam64_k3": ("cbam", "CBAM", (64, 3)), "cbam256_k7": ("cbam", "CBAM", (256, 7)),
          "ca32": ("ca", "ChannelAttention", (32,)), "sa7_c24": ("sa", "SpatialAttention", (7,))}


@pytest.fixture(autouse=True)
def _fp32():
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(torch.float32)
    yield
    dy.set_compute_dtype(torch.float32)


def _cfg(prefix="", scale="n"):
    d = load_yaml(YAMLS[prefix])
    d["scale"] = scale
    return d


def _block(name, seed):
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn import modules
    _, cls, args = BLOCKS[name]
    m = getattr(modules, cls)(*args)
    sd = om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed)
    load_sd(m, sd)
    return m.cuda(), sd


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    return float(np.abs(got - want).max() / np.abs(want).max())


_E = {}


def _fixture_error(name):
    """E of the module docstring, once per block: (train arrays' largest figure, the f64 statement's arrays)"""
    if name not in _E:
        tr = gold(f"g33_cbam_{name}_train")
        kind = BLOCKS[name][0]
        _, sd = _block(name, int(tr["seed"]))
        pick = lambda tail: next((v.double().numpy() for k, v in sd.items() if k.endswith(tail)), None)
        dy = rnd(900, *tr["y0"].shape, lo=-1, hi=1)
        out = cr.block(kind, cr.nhwc(tr["x0"].numpy()), cr.nhwc(dy.numpy()), pick("fc.weight"), pick("fc.bias"), pick("cv1.weight"))
        figs = {"y0": _rel(tr["y0"], cr.nchw(out["y"])), "dx0": _rel(tr["dx0"], cr.nchw(out["dx"]))}
        for k, v in tr.items():
            if k.startswith("g:"):
                figs[k] = _rel(v, out["fc_w" if k.endswith("fc.weight") else "fc_b" if k.endswith("fc.bias") else "cv_w"])
        _E[name] = max(figs.values())
        print(f"FIG {name}: E = {_E[name]:.3e} of {figs}")
    return _E[name]


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_train_golden(name):
    g = gold(f"g33_cbam_{name}_train")
    E = _fixture_error(name)
    m, _ = _block(name, int(g["seed"]))
    m.train()
    x = g["x0"].clone().cuda().requires_grad_(True)
    y = m(x)
    (y.float() * rnd(900, *y.shape, lo=-1, hi=1).cuda()).sum().backward()
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    figs = {"y0": _rel(y.detach().float().cpu(), g["y0"]), "dx0": _rel(x.grad.float().cpu(), g["dx0"])}
    for k, v in g.items():
        if k.startswith("g:"):
            figs[k] = _rel(named[k[2:]].grad.cpu(), v)
    assert len(figs) == 2 + len(named)
    print(f"FIG {name}: allowance {4 * E:.3e}, measured {figs}")
    assert all(e <= 4 * E for e in figs.values()), (4 * E, figs)


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_eval_golden(name):
    g = gold(f"g33_cbam_{name}_eval")
    E = _fixture_error(name)
    m, _ = _block(name, int(g["seed"]))
    m.eval()
    with torch.no_grad():
        y = m(g["x0"].cuda())
    e = _rel(y.float().cpu(), g["y0"])
    print(f"FIG {name} eval: allowance {4 * E:.3e}, measured {e:.3e}")
    assert e <= 4 * E


@pytest.mark.parametrize("name", ["cbam16_k7", "ca32", "sa7_c24"])
def test_block_writes_into_a_slice_with_live_neighbours(name):
    """out= (the graph places rows 5 and 8 inside the Concat buffers of rows 17 and 14): the result is the plain call's, the sibling
    channels stay, in eval and in train mode"""
    from dedark_yolo_amd import ops
    g = gold(f"g33_cbam_{name}_eval")
    x = g["x0"].cuda()
    B, C, H, W = x.shape
    for train in (False, True):
        buf = ops.empty_nhwc(B, C + 32, H, W, torch.float32, x.device)
        buf.fill_(7.0)
        with torch.no_grad():
            y0 = _block(name, int(g["seed"]))[0].train(train)(x)
            y1 = _block(name, int(g["seed"]))[0].train(train)(x, out=buf[:, 24:24 + C])
        assert torch.equal(buf[:, 24:24 + C], y0) and y1.data_ptr() == buf[:, 24:24 + C].data_ptr()
        assert bool((buf[:, :24] == 7.0).all()) and bool((buf[:, 24 + C:] == 7.0).all())


def test_cbam_row_fills_its_concat_slice_and_the_sibling_stays():
    """yolov8n-CBAM in eval: row 8 writes into channels [256, 384) of row 14's buffer behind the Upsample's [0, 256); the Concat's
    output is that buffer, and both halves are, bit for bit, what the two modules give when they are called on their own"""
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    model = DetectionModel(_cfg(), nc=20)
    load_sd(model, om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, 3391))
    model = model.cuda().eval()
    seen = {}
    hooks = [model.model[i].register_forward_hook(lambda m, a, o, i=i: seen.__setitem__(i, o)) for i in (7, 8, 12, 13, 14)]
    with torch.no_grad():
        model(rnd(3392, 2, 3, 64, 64).cuda())
    for h in hooks:
        h.remove()
    cat, up, cb = seen[14], seen[13], seen[8]
    assert cat.shape[1] == 384 and up.data_ptr() == cat.data_ptr() and cb.data_ptr() == cat[:, 256:].data_ptr()
    with torch.no_grad():
        cb_alone, up_alone = model.model[8](seen[7]), model.model[13](seen[12])
    assert cb_alone.data_ptr() != cb.data_ptr() and torch.equal(cat[:, 256:], cb_alone) and torch.equal(cat[:, :256], up_alone)


def _model_step(name, prefix):
    import dedark_yolo_amd as dy
    from oracle import model as om
    from parity_helpers import HYP, load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    g = gold(name)
    dy.set_compute_dtype(torch.float32)
    model = DetectionModel(_cfg(prefix), ch=3, nc=20)
    model.args = HYP
    load_sd(model, om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, int(g["seed"])))
    model = model.cuda().train()
    H, W = int(g["H"]), int(g["W"])
    batch = make_batch(int(g["seed"]) + 1, int(g["B"]), max(H, W), [int(v) for v in g["nbox"]])
    batch["img"] = batch["img"][:, :, :H, :W].contiguous().pow(3.0).cuda()
    batch["recovery_loss_batch"] = torch.tensor(0.0123).cuda()
    loss, items = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    return g, model, batch, loss, items


@pytest.mark.parametrize("name,prefix", [("g33_cbam_n_tiny", ""), ("g33_cbam_n_rect", ""), ("g33_cbam_ll_n_tiny", "ll_")])
def test_cbam_model_step_golden(name, prefix):
    g, model, batch, loss, items = _model_step(name, prefix)
    print(f"{name}: loss {float(loss.detach()):.6f} vs {float(g['loss']):.6f}, min top-two gap {float(g['min_gap_rel']):.2e}")
    close(float(loss.detach()), g["loss"], 1e-4, 1e-4, f"{name} loss vs reference golden")
    close(items.float().cpu(), g["items"], 1e-4, 1e-4, f"{name} items vs reference golden")
    named = dict(model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in named.values() if p.requires_grad)
    gtol, msd, n_att = 5e-3, model.state_dict(), 0
    for k, v in g.items():
        if k.startswith("gn:"):
            close(named[k[3:]].grad.norm().cpu(), v, gtol, 1e-6, f"{name} {k}")
            n_att += "attention" in k
        elif k.startswith("g:"):
            close(named[k[2:]].grad.cpu(), v, gtol, gtol * float(v.abs().max()), f"{name} {k}")
            n_att += "attention" in k
        elif k.startswith("b:"):
            close(msd[k[2:]].cpu(), v, 1e-4, 1e-4, f"{name} {k}")
    assert n_att == 9                           # fc.weight, fc.bias and cv1.weight of the three blocks
    model.eval()
    with torch.no_grad():
        out = model(batch["img"])
    y, maps = out[0], out[1]
    assert abs(float(y.float().sum()) - float(g["ysum"])) <= 1e-4 * float(y.float().abs().sum())
    for i in range(3):
        want = g[f"map{i}"]
        err = float((maps[i].float().cpu() - want).abs().max()) / float(want.abs().max())
        assert maps[i].shape == want.shape and err <= 1e-4, (i, err)


def test_product_eval_equals_the_reference_running_our_checkpoint():
    """the reference loaded a last.pt written by this package (make_cbam_golden.py interop); its eval output, unfused and after its
    own fuse(), is the product's on the same half-rounded weights"""
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    g = gold("g33_cbam_interop")
    model = DetectionModel(_cfg(), nc=20)
    ema = om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, 3382)
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


def _trainer(dtype, steps=2, name="yolov8n-CBAM.yaml", row=5):
    import bench
    from dedark_yolo_amd import YOLO
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    torch.manual_seed(3)
    low = "lowlight" in name
    tr = DetectionTrainer(get_cfg(dict(model=name, dtype=dtype, optimizer="SGD", batch=2, lowlight_FLAG=low, dedark_FLAG=low)))
    tr.setup(YOLO(name).model)
    trp = [(k, p) for k, p in tr.model.named_parameters() if "attention" in k]
    assert len(trp) == 9 and all(getattr(p, "_dy_direct", False) for _, p in trp)
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
        for k, p in trp:
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


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_l_scale_lowlight_trains_one_step(dtype):
    """yolov8l-lowlight-CBAM (blocks of 256 / 512 / 512 channels behind the front-end): one finite trainer step in each dtype"""
    tr, losses = _trainer(dtype, steps=1, name="yolov8l-lowlight-CBAM.yaml")
    assert np.isfinite(losses[0]) and bool(torch.isfinite(tr.flat.p).all())


def test_lowlight_cbam_with_a_filters_key():
    """the yaml's top-level `filters:` key still selects the front-end's chain in the CBAM graph: the model builds with the tone
    chain, and one forward + backward gives a finite loss and a gradient for every parameter of the three blocks and of the front-end"""
    from oracle import model as om
    from parity_helpers import HYP, load_sd
    from dedark_yolo_amd.nn.modules import lowlight_recovery
    from dedark_yolo_amd.nn.tasks import DetectionModel
    cfg = _cfg("ll_")
    cfg["filters"] = ["DF", "W", "G", "T", "Ct", "UF"]
    model = DetectionModel(cfg, ch=3, nc=20)
    assert isinstance(model.model[0], lowlight_recovery) and tuple(model.model[0].filter_names) == tuple(cfg["filters"])
    assert tuple(DetectionModel(_cfg("ll_"), ch=3, nc=20).model[0].filter_names) == ("DF", "W", "G", "Ct", "UF")
    model.args = HYP
    load_sd(model, om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, 3397))
    model = model.cuda().train()
    batch = make_batch(3398, 2, 64, [2, 1])
    batch["img"] = batch["img"].pow(3.0).cuda()
    batch["recovery_loss_batch"] = torch.tensor(0.0123).cuda()
    loss, _ = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss.detach()))
    for k, p in model.named_parameters():
        if "attention" in k or k.startswith("model.0."):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, k


def test_last_pt_round_trip(tmp_path):
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
        m = DetectionModel(_cfg(), nc=20)
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
    yolo = YOLO("yolov8n-CBAM.yaml")
    load_sd(yolo.model, om.rng_fill({k: tuple(v.shape) for k, v in yolo.model.state_dict().items()}, seed))
    yolo.model = yolo.model.cuda().eval()
    return yolo


def test_val_on_a_rect_batch():
    """val() on 64 x 96 images: the CBAM rows run on 8 x 12, 4 x 6 and 2 x 3 maps (the last two smaller than the 7 x 7 window)"""
    yolo = _yolo(3393)
    S, B = (64, 96), 2
    gen = np.random.default_rng(3394)
    img = torch.from_numpy((gen.random((B, 3, *S)) * 255).astype(np.uint8))
    loader = [dict(img=img, batch_idx=torch.tensor([0.0, 1.0]), cls=torch.tensor([[3.0], [7.0]]),
                   bboxes=torch.tensor([[0.5, 0.5, 0.3, 0.4], [0.4, 0.6, 0.2, 0.2]]), ori_shape=[S] * B)]
    with torch.no_grad():
        y = yolo.model((img.float() / 255).cuda())[0]
    assert y.shape == (B, 24, 8 * 12 + 4 * 6 + 2 * 3) and bool(torch.isfinite(y).all())
    stats = yolo.val(loader, conf=0.001, iou=0.7)
    assert "metrics/mAP50(B)" in stats and all(np.isfinite(v) for v in stats.values())


def test_predict_and_predict_augment():
    yolo = _yolo(3395)
    x = rnd(3396, 2, 3, 128, 128).cuda()
    with torch.no_grad():
        merged = yolo.model(x, augment=True)[0]
        plain = yolo.model(x)[0]
    assert merged.shape[0] == 2 and merged.shape[-1] > plain.shape[-1] and bool(torch.isfinite(merged).all())
    for aug in (False, True):
        res = yolo.predict(x, conf=0.001, augment=aug)
        assert len(res) == 2 and all(bool(torch.isfinite(r.boxes.data).all()) for r in res)
