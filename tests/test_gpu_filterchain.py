"""GPU: the four C-ABI entries of csrc/filterchain.hip (dy_tone_params_fwd/bwd, dy_filter_chain_fwd/bwd), each called through
ctypes and compared with the float64 reference of the same operation on the same tensors (tests/filterchain_ref.py), then
lowlight_recovery and the model with a `filters:` chain against the reference's fixtures (tests/golden/g32_fchain_*).

Errors are tests/test_gpu_frontend_kernels.py's measure: max |got - ref| / max |ref| per image (dparams / dtone / dfeat: per
row) and tensor; 16-bit gradients are drawn exactly representable, so the f32 bounds hold for them.  No pixel, row or case is
left out of a comparison.  The bounds are NOT taken from the kernels: E is the worst error of the same formula evaluated by torch
in f32 on the CPU over the group's cases (`python tests/filterchain_ref.py` prints this table; tests/test_filterchain_cpu.py
measures E again and asserts E <= bound), the bound is 4 E rounded up to one significant digit (the 4: another compiler's
contraction and the reduction order), capped at the project's f32 ceilings (forward 1e-4, gradients 2e-3).  Exact and fast math
share their cases, so they share E and the bound.

    group                    E (torch f32)         4 E     bound
    tone_fwd                     6.498e-08   2.599e-07     3e-07
    tone_bwd                     4.798e-07   1.919e-06     2e-06
    chain_fwd                    8.625e-07   3.450e-06     4e-06
    chain_fwd_fast               8.625e-07   3.450e-06     4e-06
    chain_dx                     7.437e-06   2.975e-05     3e-05
    chain_dx_fast                7.437e-06   2.975e-05     3e-05
    chain_dparams                7.771e-06   3.109e-05     4e-05
    chain_dparams_fast           7.771e-06   3.109e-05     4e-05

The parameter gradients (dparams, dtone) are sums of f32 block partials through f64 atomics, the mechanism of the default chain's
dparams: no bit-equality between runs is asserted for them.
"""
import functools

import numpy as np
import pytest
import torch

import filterchain_ref as fc
import frontend_ref as fr
from util import gold

pytestmark = pytest.mark.gpu

BOUNDS = {
    "tone_fwd": 3e-7, "tone_bwd": 2e-6,
    "chain_fwd": 4e-6, "chain_fwd_fast": 4e-6,
    "chain_dx": 3e-5, "chain_dx_fast": 3e-5,
    "chain_dparams": 4e-5, "chain_dparams_fast": 4e-5,
}
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
F64 = torch.float64
CODES = dict(DF=1, W=2, G=3, T=4, Ct=5)             # DY_FILTER_* of include/dedark_yolo.h


def word(names):
    return sum(CODES[n] << (4 * k) for k, n in enumerate(names))


@pytest.fixture(autouse=True)
def _fp32():
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(torch.float32)
    yield
    dy.set_compute_dtype(torch.float32)


def _api():
    from dedark_yolo_amd._C import call
    from dedark_yolo_amd.ops import dt_id, ptr, stream
    return call, ptr, stream, dt_id


def _check(group, got, ref, f32=None, what=""):
    """Print the figure (product, torch f32), then assert the group's bound."""
    e = fr.rel_err(got, ref)
    t = fr.rel_err(f32, ref) if f32 is not None else float("nan")
    print(f"FIG {group} {e:.3e} {t:.3e} {what}")
    assert e <= BOUNDS[group], f"{group} {what}: {e:.3e} > {BOUNDS[group]:.0e} (torch f32: {t:.3e})"


def _sid(s):
    return "x".join(map(str, s))


def _cid(names):
    return "-".join(names)


def _dev(c):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


# ================================================================================================ dy_tone_params_fwd / bwd
@pytest.mark.parametrize("ld", fc.TONE_LD)
@pytest.mark.parametrize("B", fc.TONE_B)
def test_tone_params_fwd(B, ld):
    call, ptr, stream, _ = _api()
    feat, buf, dt = fc.tone_feat_case(B, ld)
    ref, _ = fc.tone_params_fwd_bwd(feat, dt)
    t32, _ = fc.tone_params_fwd_bwd(feat, dt, torch.float32)
    d_buf, tone = buf.cuda(), torch.full((B, 8), 7.0, device="cuda")
    call("dy_tone_params_fwd", ptr(d_buf), ld, ptr(tone), B, stream())
    torch.cuda.synchronize()
    _check("tone_fwd", tone, ref, t32, f"B={B} ld={ld}")


@pytest.mark.parametrize("ld", fc.TONE_LD)
@pytest.mark.parametrize("B", fc.TONE_B)
def test_tone_params_bwd(B, ld):
    """writes columns 5..12 only: every other column of dfeat keeps what dy_filter_params_bwd left there"""
    call, ptr, stream, _ = _api()
    feat, buf, dt = fc.tone_feat_case(B, ld)
    _, ref = fc.tone_params_fwd_bwd(feat, dt)
    _, t32 = fc.tone_params_fwd_bwd(feat, dt, torch.float32)
    d_buf, d_dt, dfeat = buf.cuda(), dt.cuda(), torch.full((B, ld), 7.0, device="cuda")
    call("dy_tone_params_bwd", ptr(d_buf), ld, ptr(d_dt), ptr(dfeat), B, stream())
    torch.cuda.synchronize()
    _check("tone_bwd", dfeat[:, 5:13], ref[:, 5:13], t32[:, 5:13], f"B={B} ld={ld}")
    assert bool((dfeat[:, :5] == 7.0).all()) and bool((dfeat[:, 13:] == 7.0).all()), "columns outside 5..12 were written"


# =============================================================================================== dy_filter_chain_fwd / bwd
@pytest.mark.parametrize("fast", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("aica", [True, False], ids=["aica", "defaults"])
@pytest.mark.parametrize("names", fc.CHAINS, ids=_cid)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=_sid)
def test_chain_fwd(shape, names, aica, fast):
    call, ptr, stream, _ = _api()
    c, ref, t32 = fc.chain_refs(shape, names, aica)
    d = _dev(c)
    B, H, W = shape
    y = torch.full((B, 3, H, W), 7.0, device="cuda")
    call("dy_filter_chain_fwd", ptr(d["x"]), ptr(d["params"]), ptr(d["tone"]), ptr(d["A"]), ptr(d["IcA"]), word(names), ptr(y),
         B, H, W, fast, stream())
    torch.cuda.synchronize()
    _check("chain_fwd_fast" if fast else "chain_fwd", y, ref[0], t32[0], f"{shape} {_cid(names)} aica={aica}")


def _check_param_grads(sfx, names, dp, dp0, dtn, dtn0, ref, t32, what):
    if set(names) - {"T"}:
        _check("chain_dparams" + sfx, (dp.cpu() - dp0)[:, :6], ref[2][:, :6], t32[2][:, :6], what + " dparams")
    else:
        assert torch.equal(dp.cpu()[:, :6], dp0[:, :6]), "a chain of T alone adds nothing to dparams"
    assert torch.equal(dp.cpu()[:, 6:], dp0[:, 6:]), "slots 6, 7 belong to the USM kernel / nobody"
    if "T" in names:
        _check("chain_dparams" + sfx, dtn.cpu() - dtn0, ref[3], t32[3], what + " dtone")
    else:
        assert torch.equal(dtn.cpu(), dtn0), "dtone touched by a chain without T"


@pytest.mark.parametrize("fast", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("aica", [True, False], ids=["aica", "defaults"])
@pytest.mark.parametrize("names", fc.CHAINS, ids=_cid)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=_sid)
def test_chain_bwd(shape, names, aica, fast):
    """the f32 planar upstream gradient (what dy_usm_bwd writes); dx written; dparams / dtone ADDED to a non-zero start"""
    call, ptr, stream, _ = _api()
    c, ref, t32 = fc.chain_refs(shape, names, aica)
    d = _dev(c)
    B, H, W = shape
    g = np.random.default_rng(41 + H * W)
    dp0, dtn0 = torch.from_numpy(g.standard_normal((B, 8))), torch.from_numpy(g.standard_normal((B, 8)))
    dx = torch.full((B, 3, H, W), 7.0, device="cuda")
    dp, dtn = dp0.cuda(), dtn0.cuda()
    call("dy_filter_chain_bwd", ptr(d["x"]), ptr(d["params"]), ptr(d["tone"]), ptr(d["A"]), ptr(d["IcA"]), word(names), ptr(d["g"]),
         None, 0, 0, ptr(dx), ptr(dp), ptr(dtn), B, H, W, 0, fast, stream())
    torch.cuda.synchronize()
    sfx, what = ("_fast" if fast else ""), f"{shape} {_cid(names)} aica={aica}"
    _check("chain_dx" + sfx, dx, ref[1], t32[1], what)
    _check_param_grads(sfx, names, dp, dp0, dtn, dtn0, ref, t32, what)


@functools.lru_cache(maxsize=None)
def _refs16(shape, names, gdt):
    """references for the upstream gradient rounded to `gdt` (the 16-bit layouts carry exactly representable gradients)"""
    c = fc.chain_case(shape, names, True)
    g = c["g"].to(DT[gdt]).float()
    ref = fc.chain_fwd_bwd(c["x"], c["params"], c["tone"], c["A"], c["IcA"], g, names)
    t32 = fc.chain_fwd_bwd(c["x"], c["params"], c["tone"], c["A"], c["IcA"], g, names, torch.float32)
    return c, g, ref, t32


@pytest.mark.parametrize("gdt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("layout", ["planar", "nhwc8", "nhwc16"])
@pytest.mark.parametrize("names", fc.CHAINS, ids=_cid)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=_sid)
def test_chain_bwd_gradient_layouts(shape, names, layout, gdt):
    """a chain without UF takes the stem's gradient as it is: planar [B,3,H,W] (dy_ld = 0) or an NHWC view with pixel stride
    8 / 16, in f32 / bf16 / f16; the pad lanes of the view hold garbage that must not be read"""
    call, ptr, stream, dt_id = _api()
    c, g, ref, t32 = _refs16(shape, names, gdt)
    d = _dev(c)
    B, H, W = shape
    rng = np.random.default_rng(43 + H * W)
    if layout == "planar":
        gy, ld = g.to(DT[gdt]).contiguous().cuda(), 0
    else:
        ld = int(layout[4:])
        buf = torch.from_numpy(rng.uniform(-1, 1, (B, H, W, ld)).astype(np.float32))
        buf[..., :3] = g.permute(0, 2, 3, 1)
        gy = buf.to(DT[gdt]).contiguous().cuda()
    dp0, dtn0 = torch.from_numpy(rng.standard_normal((B, 8))), torch.from_numpy(rng.standard_normal((B, 8)))
    dx = torch.full((B, 3, H, W), 7.0, device="cuda")
    dp, dtn = dp0.cuda(), dtn0.cuda()
    call("dy_filter_chain_bwd", ptr(d["x"]), ptr(d["params"]), ptr(d["tone"]), ptr(d["A"]), ptr(d["IcA"]), word(names), None, ptr(gy),
         ld, dt_id(DT[gdt]), ptr(dx), ptr(dp), ptr(dtn), B, H, W, 0, 0, stream())
    torch.cuda.synchronize()
    what = f"{shape} {_cid(names)} {layout} {gdt}"
    _check("chain_dx", dx, ref[1], t32[1], what)
    _check_param_grads("", names, dp, dp0, dtn, dtn0, ref, t32, what)


@pytest.mark.parametrize("mode", ["accumulate", "no_dx"])
@pytest.mark.parametrize("names", fc.CHAINS, ids=_cid)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=_sid)
def test_chain_bwd_dx_modes(shape, names, mode):
    """dx accumulated onto a non-zero dx / not requested (fast math, A / IcA null)"""
    call, ptr, stream, _ = _api()
    c, ref, t32 = fc.chain_refs(shape, names, False)
    d = _dev(c)
    B, H, W = shape
    g = np.random.default_rng(47 + H * W)
    dx0 = torch.from_numpy(g.uniform(-2, 2, (B, 3, H, W)).astype(np.float32))
    dp0, dtn0 = torch.from_numpy(g.standard_normal((B, 8))), torch.from_numpy(g.standard_normal((B, 8)))
    dx = None if mode == "no_dx" else dx0.cuda()
    dp, dtn = dp0.cuda(), dtn0.cuda()
    call("dy_filter_chain_bwd", ptr(d["x"]), ptr(d["params"]), ptr(d["tone"]), None, None, word(names), ptr(d["g"]), None, 0, 0, ptr(dx),
         ptr(dp), ptr(dtn), B, H, W, int(mode == "accumulate"), 1, stream())
    torch.cuda.synchronize()
    what = f"{shape} {_cid(names)} {mode}"
    if mode == "accumulate":
        _check("chain_dx_fast", dx, dx0.double() + ref[1], dx0.double() + t32[1].double(), what)
    _check_param_grads("_fast", names, dp, dp0, dtn, dtn0, ref, t32, what)


def test_tone_knots_inclusive_clamp():
    """chain [T] with pixels exactly ON the knots i/8: the slope there is (t_{i-1} + t_i) 8 / T, torch.clamp's rule"""
    call, ptr, stream, _ = _api()
    c = fc.knot_case()
    ref = fc.chain_fwd_bwd(c["x"], c["params"], c["tone"], None, None, c["g"], ("T",))
    t32 = fc.chain_fwd_bwd(c["x"], c["params"], c["tone"], None, None, c["g"], ("T",), torch.float32)
    d = _dev(c)
    for fast in (0, 1):
        y, dx = torch.full((1, 3, 4, 9), 7.0, device="cuda"), torch.full((1, 3, 4, 9), 7.0, device="cuda")
        dp, dtn = torch.zeros(1, 8, dtype=F64, device="cuda"), torch.zeros(1, 8, dtype=F64, device="cuda")
        call("dy_filter_chain_fwd", ptr(d["x"]), ptr(d["params"]), ptr(d["tone"]), None, None, word(("T",)), ptr(y), 1, 4, 9, fast, stream())
        call("dy_filter_chain_bwd", ptr(d["x"]), ptr(d["params"]), ptr(d["tone"]), None, None, word(("T",)), ptr(d["g"]), None, 0, 0, ptr(dx),
             ptr(dp), ptr(dtn), 1, 4, 9, 0, fast, stream())
        torch.cuda.synchronize()
        sfx = "_fast" if fast else ""
        _check("chain_fwd" + sfx, y, ref[0], t32[0], "knots")
        _check("chain_dx" + sfx, dx, ref[1], t32[1], "knots")
        _check("chain_dparams" + sfx, dtn, ref[3], t32[3], "knots dtone")


@pytest.mark.parametrize("fast", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("aica", [True, False], ids=["aica", "defaults"])
@pytest.mark.parametrize("shape", fc.SHAPES, ids=_sid)
def test_default_pointwise_chain_agrees_with_the_fused_pair(shape, aica, fast):
    """[DF, W, G, Ct] through the general entry against dy_filters_pointwise_fwd/bwd, within the same bounds"""
    call, ptr, stream, _ = _api()
    names = ("DF", "W", "G", "Ct")
    c = fc.chain_case(shape, names, aica)
    d = _dev(c)
    B, H, W = shape
    z = lambda: torch.full((B, 3, H, W), 7.0, device="cuda")
    zd = lambda: torch.zeros(B, 8, dtype=F64, device="cuda")
    y0, y1, dx0, dx1, dp0, dp1 = z(), z(), z(), z(), zd(), zd()
    call("dy_filters_pointwise_fwd", ptr(d["x"]), ptr(d["params"]), ptr(d["A"]), ptr(d["IcA"]), ptr(y0), B, H, W, fast, stream())
    call("dy_filters_pointwise_bwd", ptr(d["x"]), ptr(d["params"]), ptr(d["A"]), ptr(d["IcA"]), ptr(d["g"]), ptr(dx0), ptr(dp0), B, H, W, 0,
         fast, stream())
    call("dy_filter_chain_fwd", ptr(d["x"]), ptr(d["params"]), None, ptr(d["A"]), ptr(d["IcA"]), word(names), ptr(y1), B, H, W, fast, stream())
    call("dy_filter_chain_bwd", ptr(d["x"]), ptr(d["params"]), None, ptr(d["A"]), ptr(d["IcA"]), word(names), ptr(d["g"]), None, 0, 0, ptr(dx1),
         ptr(dp1), None, B, H, W, 0, fast, stream())
    torch.cuda.synchronize()
    sfx, what = ("_fast" if fast else ""), f"{shape} aica={aica} vs the fused pair"
    _check("chain_fwd" + sfx, y1, y0, None, what)
    _check("chain_dx" + sfx, dx1, dx0, None, what)
    _check("chain_dparams" + sfx, dp1[:, :6], dp0[:, :6], None, what)


def test_bad_chain_words_are_refused():
    """an unknown code, a repeated one, an empty chain, Contrast at W = 2, a tone stage without tone: an error, nothing written"""
    call, ptr, stream, _ = _api()
    x, p, y = torch.zeros(1, 3, 4, 4, device="cuda"), torch.zeros(1, 8, device="cuda"), torch.full((1, 3, 4, 4), 7.0, device="cuda")
    for w_, tone, W in ((0, None, 4), (6, None, 4), (word(("G", "G")), None, 4), (word(("T",)), None, 4), (word(("Ct",)), None, 2),
                        (word(("G",)) | (1 << 8), None, 4)):
        with pytest.raises(RuntimeError):
            call("dy_filter_chain_fwd", ptr(x), ptr(p), ptr(tone), None, None, w_, ptr(y), 1, 4, W, 0, stream())
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ============================================================================================================ module level
FWD_CEILING, GRAD_CEILING, LOSS_CEILING = 1e-4, 2e-3, 1e-4       # the project's f32 ceilings (tests/test_gpu_parity.py)
BLOCKS = [("dwgtcu", ("DF", "W", "G", "T", "Ct", "UF")), ("wgtcu", ("W", "G", "T", "Ct", "UF")), ("tdcwu", ("T", "DF", "Ct", "W", "UF")),
          ("gt", ("G", "T"))]


def _max_err(got, ref):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("aica", [True, False], ids=["aica", "dflt"])
@pytest.mark.parametrize("tag,names", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_module_block_fixture(tag, names, aica):
    """lowlight_recovery(filters=chain) in train mode against what the reference computed with the same chain set in
    filter_cfg.cfg.filters: forward 1e-4, gradients 2e-3 of the tensor's max"""
    from dedark_yolo_amd.nn.modules import lowlight_recovery
    from oracle import model as om
    from parity_helpers import load_sd
    g = gold(f"g32_fchain_{tag}_{'aica' if aica else 'dflt'}")
    assert tuple(g["chain"]) == names
    m = lowlight_recovery(3, 3, filters=list(names))
    load_sd(m, om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"])))
    m = m.cuda().train()
    x = g["x"].clone().cuda().requires_grad_(True)
    out = m(x, g["A"].cuda(), g["IcA"].cuda()) if aica else m(x)
    (out.float() * g["wgt"].cuda()).sum().backward()
    torch.cuda.synchronize()
    e = _max_err(out.float(), g["out"])
    print(f"FIGM {tag} aica={aica} out {e:.3e}")
    assert e <= FWD_CEILING, e
    e = _max_err(x.grad, g["dx"])
    print(f"FIGM {tag} aica={aica} dx {e:.3e}")
    assert e <= GRAD_CEILING, e
    for k, p in m.named_parameters():
        if "g:" + k in g:
            e = _max_err(p.grad, g["g:" + k])
        else:
            e = max(_max_err(p.grad[:2], g["g2:" + k]), abs(float(p.grad.norm()) / float(g["gn:" + k]) - 1.0))
        print(f"FIGM {tag} aica={aica} d {k} {e:.3e}")
        assert e <= GRAD_CEILING, (k, e)
    rows = m.extractor.fc2.weight.grad[5:13].abs().amax(1).cpu()
    assert bool((rows > 0).all()) == ("T" in names) and bool((rows == 0).all()) == ("T" not in names)


def _tone_model(seed, dtype=torch.float32):
    import dedark_yolo_amd as dy
    from dedark_yolo_amd.nn.tasks import DetectionModel
    from oracle import model as om
    from types import SimpleNamespace
    dy.set_compute_dtype(dtype)
    m = DetectionModel("yolov8n-lowlight-tone.yaml", nc=20)
    assert m.model[0].filter_names == ("DF", "W", "G", "T", "Ct", "UF")
    m.load_state_dict(om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed), strict=True)
    m.args = SimpleNamespace(box=7.5, cls=0.5, dfl=1.5, lrl=2.0)
    return m.cuda()


def test_model_step_fixture():
    """yolov8n-lowlight-tone at 64 x 64, B = 2: one training step and the eval output against the reference's"""
    from util import make_batch
    g = gold("g32_fchain_tone_n_tiny")
    m = _tone_model(int(g["seed"])).train()
    batch = make_batch(int(g["seed"]) + 1, int(g["B"]), int(g["S"]), [int(v) for v in g["nbox"]])
    batch["img"] = batch["img"].pow(3.0)
    batch = {k: v.cuda() for k, v in batch.items()}
    batch["recovery_loss_batch"] = torch.tensor(0.0123, device="cuda")
    loss, items = m(batch)
    loss.backward()
    torch.cuda.synchronize()
    e = abs(float(loss) - float(g["loss"])) / max(1.0, abs(float(g["loss"])))
    print(f"FIGM tone model loss {float(loss):.6f} ref {float(g['loss']):.6f} ({e:.2e})")
    assert e <= LOSS_CEILING
    assert _max_err(items.float(), g["items"]) <= LOSS_CEILING
    named = dict(m.named_parameters())
    for k in g:
        if k.startswith("g:"):
            e = _max_err(named[k[2:]].grad, g[k])
        elif k.startswith("gn:"):
            e = abs(float(named[k[3:]].grad.norm()) / float(g[k]) - 1.0)
        else:
            continue
        print(f"FIGM tone model {k} {e:.3e}")
        assert e <= GRAD_CEILING, (k, e)
    sd = m.state_dict()
    for k in g:
        if k.startswith("b:"):
            assert _max_err(sd[k[2:]], g[k]) <= FWD_CEILING, k
    m.eval()
    with torch.no_grad():
        y = m(batch["img"])
    y = y[0] if isinstance(y, (list, tuple)) else y
    e = _max_err(y.float(), g["y"])
    print(f"FIGM tone model eval {e:.3e}")
    assert e <= FWD_CEILING, e


def test_product_eval_equals_the_reference_running_our_checkpoint():
    """tests/golden/g32_fchain_interop.npz: the reference loaded a last.pt of yolov8n-lowlight-tone written here (half-precision
    EMA weights) and ran its eval forward; the product with the same weights computes the same"""
    from oracle import model as om
    from util import rnd
    z = gold("g32_fchain_interop")
    m = _tone_model(1)
    sd = om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(z["sd_seed"]))
    m.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()
    with torch.no_grad():
        y = m(rnd(int(z["x_seed"]), 2, 3, 64, 64).pow(2.0).cuda())
    y = y[0] if isinstance(y, (list, tuple)) else y
    e = _max_err(y.float(), z["y"])
    print(f"FIGM interop eval {e:.3e}")
    assert e <= FWD_CEILING, e


@pytest.mark.parametrize("yaml_name", ["yolov8n-lowlight-tone.yaml", "yolov8n-lowlight-nodedark.yaml"])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_two_training_steps_are_finite(dt, yaml_name):
    import dedark_yolo_amd as dy
    from dedark_yolo_amd.nn.tasks import DetectionModel
    from types import SimpleNamespace
    from util import make_batch
    dy.set_compute_dtype(DT[dt])
    torch.manual_seed(3)
    m = DetectionModel(yaml_name, nc=20)
    m.args = SimpleNamespace(box=7.5, cls=0.5, dfl=1.5, lrl=2.0)
    m = m.cuda().train()
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    batch = {k: v.cuda() for k, v in make_batch(5, 2, 64, [2, 3]).items()}
    batch["recovery_loss_batch"] = torch.tensor(0.01, device="cuda")
    for _ in range(2):
        opt.zero_grad()
        loss, _ = m(batch)
        loss.backward()
        opt.step()
        assert torch.isfinite(loss).all()
    g = m.model[0].extractor.fc2.weight.grad
    assert torch.isfinite(g).all() and bool((g[5:13].abs().amax(1) > 0).all())
    assert all(torch.isfinite(p).all() for p in m.parameters())


def test_yolo_predict_with_a_chain_yaml():
    """YOLO('yolov8n-lowlight-nodedark.yaml').predict, plain and augment=True: Results come back, and they are the NMS of the
    model's own eval output (the chain runs inside the predictor as it does in the bare model)"""
    from dedark_yolo_amd import YOLO
    from dedark_yolo_amd.utils import ops as uops
    from oracle import model as om
    from parity_helpers import load_sd
    from util import rnd
    y = YOLO("yolov8n-lowlight-nodedark.yaml")
    assert y.model.model[0].filter_names == ("W", "G", "T", "Ct", "UF")
    sd = om.rng_fill({k: tuple(v.shape) for k, v in y.model.state_dict().items()}, 31)
    for k in sd:
        if ".cv3." in k and k.endswith("2.bias"):
            sd[k] = sd[k] + 3.0
    load_sd(y.model, sd)
    y.model.cuda()
    x = rnd(32, 2, 3, 128, 128).cuda()
    res, resa = y.predict(x, conf=0.5), y.predict(x, conf=0.5, augment=True)
    with torch.no_grad():
        raw = y.model.eval()(x)[0]
    dets = uops.non_max_suppression((raw, None), 0.5, 0.7, max_det=300)
    assert len(res) == 2 and len(resa) == 2 and sum(len(r.boxes) for r in res) > 4
    for r, d in zip(res, dets):
        d = d.clone()
        uops.scale_boxes((128, 128), d[:, :4], (128, 128))
        assert torch.equal(r.boxes.data, d[:, :6])
    assert all(torch.isfinite(r.boxes.data).all() for r in resa)


def _yolo(yaml_name, seed):
    from dedark_yolo_amd.engine.model import YOLO
    from oracle import model as om
    from parity_helpers import load_sd
    yolo = YOLO(yaml_name)
    load_sd(yolo.model, om.rng_fill({k: tuple(v.shape) for k, v in yolo.model.state_dict().items()}, seed))
    yolo.model = yolo.model.cuda().eval()
    return yolo


@pytest.mark.parametrize("yaml_name,chain", [("yolov8n-lowlight-tone.yaml", ("DF", "W", "G", "T", "Ct", "UF")),
                                             ("yolov8n-lowlight-nodedark.yaml", ("W", "G", "T", "Ct", "UF"))])
def test_val_on_a_rect_batch(yaml_name, chain):
    """YOLO(yaml).val() on a loader of one rect batch (64 x 96 uint8 images with labels and ori_shape): the chain runs inside the
    validator as it does in the bare model, the metrics come back finite"""
    yolo = _yolo(yaml_name, 3271)
    assert yolo.model.model[0].filter_names == chain
    S, B = (64, 96), 2
    gen = np.random.default_rng(3272)
    img = torch.from_numpy((gen.random((B, 3, *S)) * 255).astype(np.uint8))
    loader = [dict(img=img, batch_idx=torch.tensor([0.0, 1.0]), cls=torch.tensor([[3.0], [7.0]]),
                   bboxes=torch.tensor([[0.5, 0.5, 0.3, 0.4], [0.4, 0.6, 0.2, 0.2]]), ori_shape=[S] * B)]
    with torch.no_grad():
        y = yolo.model((img.float() / 255).cuda())[0]
    assert y.shape == (B, 24, 8 * 12 + 4 * 6 + 2 * 3) and bool(torch.isfinite(y).all())
    stats = yolo.val(loader, conf=0.001, iou=0.7)
    assert "metrics/mAP50(B)" in stats and all(np.isfinite(v) for v in stats.values())


def test_model_predict_augment_on_a_rect_image():
    """the augmented eval forward (scaled / flipped passes) of the tone model on a non-square image"""
    m = _tone_model(11).eval()
    from util import rnd
    x = rnd(12, 2, 3, 64, 96).cuda()
    with torch.no_grad():
        y = m(x)
        ya = m(x, augment=True)
    y = y[0] if isinstance(y, (list, tuple)) else y
    ya = ya[0] if isinstance(ya, (list, tuple)) else ya
    assert y.shape[0] == 2 and y.shape[1] == 24 and torch.isfinite(y.float()).all()
    assert ya.shape[:2] == y.shape[:2] and ya.shape[-1] > y.shape[-1] and torch.isfinite(ya.float()).all()
