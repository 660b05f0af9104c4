"""GPU tests of the transformer encoder layer (AIFI / TransformerEncoderLayer on the fused add+LayerNorm, GELU, position-add and
attention kernels), modelled on tests/test_gpu_c3tr.py.

Blocks (fp32) against the reference's fixtures g30_aifi_<block>_<train|eval> (tests/golden/make_aifi_golden.py): outputs within
1e-4, input and parameter gradients within 2e-3 -- the bounds of test_gpu_parity._run_block, which test_gpu_c3tr.py uses for its
block fixtures.  aifi64_3x5 is the non-square map on which the position table's (iw, ih) order disagrees with the tokens'.
The whole yolov8n-AIFI model at 64x64 (P5 = 4 tokens) and at 64x96 (P5 = 2x3) against g30_aifi_n_tiny / g30_aifi_n_rect: loss and
items within 1e-4, gradients (the layer's among them), running statistics and the three eval maps within the bounds
test_gpu_c3tr.py uses for its whole-model fixture; fuse() leaves the layer alone.  Two trainer steps in fp32, bf16 and fp16 are
finite and, run twice, give identical parameter bytes.  val() on a 64 x 96 rect batch, predict(augment=True), the last.pt round
trip, and the reference's own eval output of a last.pt written here (g30_aifi_interop).
"""
import numpy as np
import pytest
import torch

from aifi_ref import rect_batch
from util import close, gold, load_yaml, rnd

pytestmark = pytest.mark.gpu

TOL_Y, TOL_G = 1e-4, 2e-3          # test_gpu_parity._run_block
YAML = "yolov8-AIFI.yaml"
BLOCKS = {"aifi64_4x4": ("AIFI", (64, 128, 8)), "aifi64_3x5": ("AIFI", (64, 128, 8)), "aifi256_2x2": ("AIFI", (256, 1024, 8)),
          "tel64": ("TransformerEncoderLayer", (64, 128, 4))}


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
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn import modules
    cls, args = BLOCKS[name]
    m = getattr(modules, cls)(*args)
    load_sd(m, om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"])))
    return m.cuda()


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_train_golden(name):
    g = gold(f"g30_aifi_{name}_train")
    m = _block(name, g).train()
    x = g["x0"].clone().cuda().requires_grad_(True)
    y = m(x)
    close(y.detach().float().cpu(), g["y0"], TOL_Y, TOL_Y, f"{name} y")
    (y.float() * rnd(900, *y.shape, lo=-1, hi=1).cuda()).sum().backward()
    torch.cuda.synchronize()
    close(x.grad.float().cpu(), g["dx0"], TOL_G, TOL_G, f"{name} dx")
    named, n = dict(m.named_parameters()), 0
    for k, v in g.items():
        if k.startswith("g:"):
            close(named[k[2:]].grad.cpu(), v, TOL_G, TOL_G, f"{name} {k}")
            n += 1
        elif k.startswith("gn:"):
            close(named[k[3:]].grad.norm().cpu(), v, TOL_G, 1e-4, f"{name} {k}")
            n += 1
    assert n == len(named) == 12           # every parameter, ma.in_proj_weight / in_proj_bias and the four LayerNorm vectors among them


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_eval_golden(name):
    g = gold(f"g30_aifi_{name}_eval")
    m = _block(name, g).eval()
    with torch.no_grad():
        y = m(g["x0"].cuda())
    close(y.float().cpu(), g["y0"], TOL_Y, TOL_Y, f"{name} eval y")


def test_block_writes_into_a_slice_with_live_neighbours():
    """out= (the graph places row 9 inside the head's last Concat buffer): the result is the plain call's, the sibling channels stay"""
    g = gold("g30_aifi_aifi64_3x5_eval")
    m = _block("aifi64_3x5", g).eval()
    x = g["x0"].cuda()
    B, C, H, W = x.shape
    from dedark_yolo_amd import ops
    buf = ops.empty_nhwc(B, C + 32, H, W, torch.float32, x.device)
    buf.fill_(7.0)
    with torch.no_grad():
        y0 = m(x)
        y1 = m(x, out=buf[:, 24:24 + C])
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
    batch = rect_batch(int(g["seed"]) + 1, int(g["B"]), int(g["H"]), int(g["W"]), [int(v) for v in g["nbox"]])
    batch["img"] = batch["img"].pow(3.0).cuda()
    batch["recovery_loss_batch"] = torch.tensor(0.0123).cuda()
    loss, items = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    return g, model, batch, loss, items


@pytest.mark.parametrize("name", ["g30_aifi_n_tiny", "g30_aifi_n_rect"])
def test_aifi_model_step_golden(name):
    g, model, batch, loss, items = _model_step(name)
    print(f"{name}: loss {float(loss.detach()):.6f} vs {float(g['loss']):.6f}")
    close(float(loss.detach()), g["loss"], 1e-4, 1e-4, f"{name} loss vs reference golden")
    close(items.float().cpu(), g["items"], 1e-4, 1e-4, f"{name} items vs reference golden")
    named = dict(model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in named.values() if p.requires_grad)
    gtol, msd, n_tr = 5e-3, model.state_dict(), 0
    is_tr = lambda k: "model.9." in k
    # The layer's vector gradients are measured against the largest of them (test_gpu_c3tr.py's measure for its transformer):
    # norm2.bias adds a per-channel constant in front of the train-mode BatchNorm of the 1x1 convs that read row 9 (through Upsample /
    # Concat), and the k-rows of ma.in_proj_bias a per-query constant inside the softmax, so their true gradient is exactly 0 and the
    # fixture holds the reference's own rounding noise there (7e-7 against 4.1 for norm1.weight): noise has no relative error.
    tr_top = max(float(v.abs().max()) for k, v in g.items() if k.startswith("g:") and is_tr(k))
    assert tr_top > 1.0 and float(g["g:model.9.norm2.bias"].abs().max()) < 1e-5
    for k, v in g.items():
        if k.startswith("gn:"):
            close(named[k[3:]].grad.norm().cpu(), v, gtol, 1e-6, f"{name} {k}")
            n_tr += is_tr(k)
        elif k.startswith("g:"):
            close(named[k[2:]].grad.cpu(), v, gtol, gtol * (tr_top if is_tr(k) else float(v.abs().max())), f"{name} {k}")
            n_tr += is_tr(k)
        elif k.startswith("b:"):
            close(msd[k[2:]].cpu(), v, 1e-4, 1e-4, f"{name} {k}")
    assert n_tr == 12                      # every parameter of the layer
    model.eval()
    with torch.no_grad():
        out = model(batch["img"])
    y, maps = out[0], out[1]
    assert abs(float(y.float().sum()) - float(g["ysum"])) <= 1e-4 * float(y.float().abs().sum())
    for i in range(3):
        want = g[f"map{i}"]
        err = float((maps[i].float().cpu() - want).abs().max()) / float(want.abs().max())
        assert maps[i].shape == want.shape and err <= 1e-4, (i, err)
    before = {k: v.clone() for k, v in model.model[9].state_dict().items()}
    model.fuse()
    assert model.is_fused() and all(torch.equal(v, before[k]) for k, v in model.model[9].state_dict().items())
    with torch.no_grad():
        yf = model(batch["img"])[0]
    assert float((yf.float() - y.float()).abs().max()) <= 1e-4 * float(y.abs().max())     # test_gpu_ghost.py's fuse tolerance


def test_product_eval_equals_the_reference_running_our_checkpoint():
    """the reference loaded a last.pt written by this package (make_aifi_golden.py interop); its eval output is the product's on the
    same half-rounded weights"""
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    g = gold("g30_aifi_interop")
    model = DetectionModel(_cfg("n"), nc=20)
    ema = om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, 3062)
    load_sd(model, {k: (v.half().float() if v.is_floating_point() else v) for k, v in ema.items()})
    model = model.cuda().eval()
    x = rnd(int(g["x_seed"]), 2, 3, 64, 64).pow(2.0)
    with torch.no_grad():
        y = model(x.cuda())
    y = y[0] if isinstance(y, (list, tuple)) else y
    want = g["y"]
    err = float((y.float().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)
    assert y.shape == want.shape and err <= 1e-4, err


def _trainer(dtype, steps=2, name="yolov8n-AIFI.yaml"):
    import bench
    from dedark_yolo_amd import YOLO
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    torch.manual_seed(3)
    tr = DetectionTrainer(get_cfg(dict(model=name, dtype=dtype, optimizer="SGD", batch=2, lowlight_FLAG=False, dedark_FLAG=False)))
    tr.setup(YOLO(name).model)
    trp = [(k, p) for k, p in tr.model.named_parameters() if k.startswith("model.9.")]
    assert len(trp) == 12 and all(getattr(p, "_dy_direct", False) for _, p in trp)
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
        for k, p in trp:                         # every parameter of the layer received a gradient, in_proj rows and LayerNorm vectors included
            assert bool(torch.isfinite(p.grad).all()), k
            assert float(p.grad.abs().max()) > 0.0 or k.endswith("norm2.bias"), k     # (norm2.bias: 0 in theory, see the model test)
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
    """yolov8l-AIFI (width 512, head dim 64) in bf16: one finite trainer step"""
    tr, losses = _trainer("bf16", steps=1, name="yolov8l-AIFI.yaml")
    assert np.isfinite(losses[0]) and bool(torch.isfinite(tr.flat.p).all())


def test_last_pt_round_trip(tmp_path):
    """last.pt of yolov8n-AIFI in the reference's format, read back by our reader: same keys, the trained weights at half precision,
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
    yolo = YOLO("yolov8n-AIFI.yaml")
    load_sd(yolo.model, om.rng_fill({k: tuple(v.shape) for k, v in yolo.model.state_dict().items()}, seed))
    yolo.model = yolo.model.cuda().eval()
    return yolo


def test_val_on_a_rect_batch():
    """val() on 64 x 96 images (P5 = 2 x 3 = 6 tokens, P3 = 8 x 12): the token count and the position table follow the map"""
    from dedark_yolo_amd import ops
    yolo = _yolo(3071)
    S, B = (64, 96), 2
    gen = np.random.default_rng(3072)
    img = torch.from_numpy((gen.random((B, 3, *S)) * 255).astype(np.uint8))
    loader = [dict(img=img, batch_idx=torch.tensor([0.0, 1.0]), cls=torch.tensor([[3.0], [7.0]]),
                   bboxes=torch.tensor([[0.5, 0.5, 0.3, 0.4], [0.4, 0.6, 0.2, 0.2]]), ori_shape=[S] * B)]
    with torch.no_grad():
        y = yolo.model((img.float() / 255).cuda())[0]
    assert y.shape == (B, 24, 8 * 12 + 4 * 6 + 2 * 3) and bool(torch.isfinite(y).all())
    assert any(k[:3] == (3, 2, 256) for k in ops._pos_tables)           # (w, h, C) of the 2 x 3 map
    stats = yolo.val(loader, conf=0.001, iou=0.7)
    assert "metrics/mAP50(B)" in stats and all(np.isfinite(v) for v in stats.values())


def test_predict_augment():
    """predict(augment=True): the scaled / flipped passes put other token counts through the layer (128^2: 16, 9 and 4 tokens)"""
    from dedark_yolo_amd import ops
    yolo = _yolo(3073)
    x = rnd(3074, 2, 3, 128, 128).cuda()
    with torch.no_grad():
        merged = yolo.model(x, augment=True)[0]
        plain = yolo.model(x)[0]
    assert merged.shape[0] == 2 and merged.shape[-1] > plain.shape[-1] and bool(torch.isfinite(merged).all())
    assert {(4, 4, 256), (3, 3, 256), (2, 2, 256)} <= {k[:3] for k in ops._pos_tables}
    res = yolo.predict(x, conf=0.001, augment=True)
    assert len(res) == 2 and all(bool(torch.isfinite(r.boxes.data).all()) for r in res)
