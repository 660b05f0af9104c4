"""GPU: the eight C-ABI entries of the low-light front-end (csrc/frontend.hip, csrc/usm.hip), each called directly and compared
with a float64 reference of the same operation on the same tensors (tests/frontend_ref.py).

Errors are max |got - ref| / max |ref|, per image and per tensor (dparams / dfeat: per row).  Ceilings are the project's f32
figures (forward 1e-4, gradients 2e-3, tests/test_gpu_parity.py); inside them every group has a fixed bound of 4 x the worst
error the product measured on an MI355X over all cases of the group, rounded up to one significant digit (the 4 covers other
compilers and the arrival order of the f32 atomics of resize_bwd_kernel; the f64 atomics of dparams are order-free).  "torch f32"
is the oracle run in f32 on the CPU on the same cases: the error any f32 evaluation has.

    group                      product      torch f32    bound
    params fwd                 2.0e-07      2.0e-07      8e-07
    params bwd (dfeat)         7.6e-07      5.7e-07      4e-06
    pointwise s4, exact        4.9e-05      4.9e-05      1e-04   (4 x = 2e-04: capped at the forward ceiling)
    pointwise s4, fast math    4.9e-05      4.9e-05      1e-04   (the same)
    pointwise dx, exact        1.5e-04      1.5e-04      6e-04
    pointwise dx, fast math    1.5e-04      1.5e-04      6e-04
    pointwise dparams, exact   8.4e-05      8.5e-05      4e-04
    pointwise dparams, fast    8.4e-05      8.5e-05      4e-04
    usm fwd (out, hp, out8)    3.4e-07      3.8e-07      2e-06
    usm ds4                    9.3e-08      1.3e-07      4e-07
    usm dlambda                1.1e-07      9.7e-08      5e-07
    resize fwd                 2.4e-06      2.4e-06      1e-05
    resize bwd                 1.7e-06      1.7e-06      7e-06

No group is worse than torch's own f32 by more than a factor 1.3.  The pointwise figures are two orders above the others, for
the product and for torch alike, and the same with either math mode: they come from rows whose three luminance pixels are all
clamped (lum ~ 3e-5), where f32 evaluates 0.5 - 0.5 cos(pi lum) as exactly 0 against 3e-9 in f64, which moves the row's contrast
gain K = (1 - alpha) + alpha cl / (lum + 1e-6) by ~ alpha * 8e-5.  That is a property of the reference's formula in f32, not of
the kernels; the input law keeps such rows (it populates every branch), so the pointwise forward bound is the ceiling itself.
16-bit outputs measured at 0.42 .. 0.49 of (bound + 1 ulp): correctly rounded.

16-bit outputs: the f32 bound plus one ulp of the type at the reference value.  16-bit gradients are drawn exactly representable,
so the f32 bounds hold for them.  No pixel, row or case is excluded from a comparison.
"""
import functools

import numpy as np
import pytest
import torch

import frontend_ref as fr
from util import gold

pytestmark = pytest.mark.gpu

BOUNDS = {
    "params_fwd": 8e-7, "params_bwd": 4e-6,
    "pw_fwd": 1e-4, "pw_dx": 6e-4, "pw_dparams": 4e-4,
    "pw_fwd_fast": 1e-4, "pw_dx_fast": 6e-4, "pw_dparams_fast": 4e-4,
    "usm_fwd": 2e-6, "usm_ds4": 4e-7, "usm_dlam": 5e-7,
    "resize_fwd": 1e-5, "resize_bwd": 7e-6,
}
FWD_CEILING, GRAD_CEILING = 1e-4, 2e-3
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
F64 = torch.float64


def test_bounds_respect_the_ceilings():
    for k, v in BOUNDS.items():
        assert v <= (FWD_CEILING if "fwd" in k else GRAD_CEILING), k


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


def _u(g, lo, hi, *shape):
    return torch.from_numpy((lo + (hi - lo) * g.random(shape, dtype=np.float32)).astype(np.float32))


def _check(group, got, ref, f32=None, what=""):
    """Print the figure (product, torch f32), then assert the group's bound."""
    e = fr.rel_err(got, ref)
    t = fr.rel_err(f32, ref) if f32 is not None else float("nan")
    print(f"FIG {group} {e:.3e} {t:.3e} {what}")
    assert e <= BOUNDS[group], f"{group} {what}: {e:.3e} > {BOUNDS[group]:.0e} (torch f32: {t:.3e})"


def _check16(group, got, ref, dtype, what=""):
    """A 16-bit output: within the f32 bound (of the image's max |ref|) plus one ulp of `dtype` at the reference value."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    n = ref.shape[0]
    tol = BOUNDS[group] * ref.reshape(n, -1).abs().amax(1).reshape([n] + [1] * (ref.ndim - 1)) + fr.ulp(ref, dtype)
    over = ((got - ref).abs() / tol).max()
    print(f"FIG16 {group} {dtype} {float(over):.3f} of the allowance {what}")
    assert over <= 1.0, f"{group} {dtype} {what}: {float(over):.3f} x (bound + 1 ulp)"


def _sid(s):
    return "x".join(map(str, s))


# ============================================================================================= dy_filter_params_fwd / bwd
def _feat_case(B, ld):
    g = np.random.default_rng(7000 + 10 * B + ld)
    feat = _u(g, -2.0, 2.0, B, 15)
    sat = torch.from_numpy(g.random((B, 15))) < 0.15                 # saturated tanh
    feat = torch.where(sat, torch.where(torch.from_numpy(g.random((B, 15))) < 0.5, -10.0, 10.0).float(), feat)
    buf = _u(g, -3.0, 3.0, B, ld)                                    # the pad columns hold garbage the kernels must not use
    buf[:, :15] = feat
    dp = torch.from_numpy(g.standard_normal((B, 8)))                 # f64, slot 7 garbage
    return feat, buf, dp


@pytest.mark.parametrize("ld", [15, 16, 24])
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_filter_params_fwd(B, ld):
    call, ptr, stream, _ = _api()
    feat, buf, dp = _feat_case(B, ld)
    ref, _ = fr.params_fwd_bwd(feat, dp)
    t32, _ = fr.params_fwd_bwd(feat, dp, torch.float32)
    d_buf = buf.cuda()
    params = torch.full((B, 8), 7.0, device="cuda")
    call("dy_filter_params_fwd", ptr(d_buf), ld, ptr(params), B, stream())
    torch.cuda.synchronize()
    _check("params_fwd", params[:, :7], ref[:, :7], t32[:, :7], f"B={B} ld={ld}")
    assert bool((params[:, 7] == 0).all())


@pytest.mark.parametrize("ld", [15, 16, 24])
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_filter_params_bwd(B, ld):
    call, ptr, stream, _ = _api()
    feat, buf, dp = _feat_case(B, ld)
    _, ref = fr.params_fwd_bwd(feat, dp)
    _, t32 = fr.params_fwd_bwd(feat, dp, torch.float32)
    d_buf, d_dp = buf.cuda(), dp.cuda()
    dfeat = torch.full((B, ld), 7.0, device="cuda")
    call("dy_filter_params_bwd", ptr(d_buf), ld, ptr(d_dp), ptr(dfeat), B, stream())
    torch.cuda.synchronize()
    _check("params_bwd", dfeat[:, :15], ref, t32, f"B={B} ld={ld}")
    assert bool((ref[:, [1] + list(range(5, 13))] == 0).all())      # the reference agrees these carry no gradient
    assert bool((dfeat[:, 1] == 0).all()), "masked R slot"
    assert bool((dfeat[:, 5:13] == 0).all()), "unused slots 5..12"
    assert bool((dfeat[:, 15:] == 0).all()), "feat_ld pad columns"


# ========================================================================================= dy_filters_pointwise_fwd / bwd
@functools.lru_cache(maxsize=None)
def _pw(shape, aica):
    c = fr.pointwise_case(*shape, aica=aica)
    fr.check_input_law(c, aica)
    ref = fr.pointwise_fwd_bwd(c["x"], c["params"], c["A"], c["IcA"], c["g4"])
    t32 = fr.pointwise_fwd_bwd(c["x"], c["params"], c["A"], c["IcA"], c["g4"], torch.float32)
    return c, ref, t32


def _dev(c):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


@pytest.mark.parametrize("fast", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("aica", [True, False], ids=["aica", "defaults"])
@pytest.mark.parametrize("shape", fr.POINTWISE_SHAPES, ids=_sid)
def test_pointwise_fwd(shape, aica, fast):
    call, ptr, stream, _ = _api()
    c, ref, t32 = _pw(shape, aica)
    d = _dev(c)
    B, H, W = shape
    s4 = torch.full((B, 3, H, W), 7.0, device="cuda")
    call("dy_filters_pointwise_fwd", ptr(d["x"]), ptr(d["params"]), ptr(d["A"]), ptr(d["IcA"]), ptr(s4), B, H, W, fast, stream())
    torch.cuda.synchronize()
    _check("pw_fwd_fast" if fast else "pw_fwd", s4, ref[0], t32[0], f"{shape} aica={aica}")


@pytest.mark.parametrize("mode", ["write", "accumulate", "no_dx"])
@pytest.mark.parametrize("fast", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("aica", [True, False], ids=["aica", "defaults"])
@pytest.mark.parametrize("shape", fr.POINTWISE_SHAPES, ids=_sid)
def test_pointwise_bwd(shape, aica, fast, mode):
    """dx written / accumulated onto a non-zero dx / not requested; dparams slots 0..5 ADDED to a non-zero start, 6..7 untouched."""
    call, ptr, stream, _ = _api()
    c, ref, t32 = _pw(shape, aica)
    d = _dev(c)
    B, H, W = shape
    g = np.random.default_rng(31 + H * W)
    dx0 = _u(g, -2.0, 2.0, B, 3, H, W)
    dp0 = torch.from_numpy(g.standard_normal((B, 8)))
    dx = None if mode == "no_dx" else dx0.cuda()
    dp = dp0.cuda()
    call("dy_filters_pointwise_bwd", ptr(d["x"]), ptr(d["params"]), ptr(d["A"]), ptr(d["IcA"]), ptr(d["g4"]), ptr(dx), ptr(dp),
         B, H, W, int(mode == "accumulate"), fast, stream())
    torch.cuda.synchronize()
    sfx, what = ("_fast" if fast else ""), f"{shape} aica={aica} {mode}"
    if mode == "write":
        _check("pw_dx" + sfx, dx, ref[1], t32[1], what)
    elif mode == "accumulate":
        _check("pw_dx" + sfx, dx, dx0.double() + ref[1], dx0.double() + t32[1].double(), what)
    _check("pw_dparams" + sfx, (dp.cpu() - dp0)[:, :6], ref[2][:, :6], t32[2][:, :6], what)
    assert torch.equal(dp.cpu()[:, 6:], dp0[:, 6:]), "slots 6, 7 belong to the USM kernel / nobody"


# ======================================================================================================= dy_usm_fwd / bwd
USM_SIZES = [(13, 13), (13, 70), (24, 25), (25, 24), (37, 64), (40, 64), (41, 65), (52, 76), (50, 77), (80, 128)]
USM_LAMS = {1: [3.1], 2: [5.0, 0.0], 3: [0.0, 5.0, 2.3]}


@functools.lru_cache(maxsize=None)
def _usm(B, H, W):
    g = np.random.default_rng(9000 + 1000 * B + 7 * H + W)
    s4 = _u(g, -0.2, 1.5, B, 3, H, W)
    params = _u(g, -1.0, 1.0, B, 8)                                  # only slot 6 is the USM kernel's business
    params[:, 6] = torch.tensor(USM_LAMS[B])
    lam = params[:, 6]
    with torch.no_grad():
        hp64 = fr.usm_separable(s4.double(), lam.double()[:, None], hp=True)[1]
    hp32 = hp64.float()
    grad = _u(g, -1.0, 1.0, B, 3, H, W) + hp32                       # correlated with hp: d lambda = sum g hp does not cancel
    pad = _u(g, -1.0, 1.0, B, H, W, 16)                              # garbage for the pad lanes of the NHWC layouts
    return dict(s4=s4, params=params, lam=lam, hp32=hp32, grad=grad, pad=pad)


@functools.lru_cache(maxsize=None)
def _usm_ref(B, H, W, gdt):
    """References for the gradient rounded to `gdt` (the 16-bit layouts carry exactly representable gradients)."""
    c = _usm(B, H, W)
    g = c["grad"].to(DT[gdt]).float()
    out, hp, ds4, _ = fr.usm_fwd_bwd(c["s4"], c["lam"], g)
    t32 = fr.usm_fwd_bwd(c["s4"], c["lam"], g, torch.float32)
    dlam = (g.double() * c["hp32"].double()).sum((1, 2, 3))          # the kernel is handed hp32, not its own hp
    dlam32 = (g * c["hp32"]).sum((1, 2, 3))
    return g, out, hp, ds4, dlam, t32, dlam32


def _usm_fwd_case(B, H, W, combo, dt):
    call, ptr, stream, dt_id = _api()
    c = _usm(B, H, W)
    _, ref_out, ref_hp, _, _, t32, _ = _usm_ref(B, H, W, "f32")
    dtype = DT[dt]
    s4, params = c["s4"].cuda(), c["params"].cuda()
    out = torch.full((B, 3, H, W), 7.0, device="cuda") if combo == "all" else None
    hp = torch.full((B, 3, H, W), 7.0, device="cuda")
    out8 = torch.full((B, H, W, 8), 7.0, device="cuda", dtype=dtype)
    call("dy_usm_fwd", ptr(s4), ptr(params), ptr(out), ptr(out8), ptr(hp), B, H, W, dt_id(dtype), stream())
    torch.cuda.synchronize()
    what = f"B={B} {H}x{W} {combo} {dt}"
    if out is not None:
        _check("usm_fwd", out, ref_out, t32[0], what + " out")
    _check("usm_fwd", hp, ref_hp, t32[1], what + " hp")
    got8 = out8[..., :3].permute(0, 3, 1, 2)
    if dtype == torch.float32:
        _check("usm_fwd", got8, ref_out, t32[0], what + " out8")
    else:
        _check16("usm_fwd", got8, ref_out, dtype, what + " out8")
    assert bool((out8[..., 3:] == 0).all()), "NHWC8 lanes 3..7 are the stem conv's zero padding"


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("combo", ["product", "all"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("size", USM_SIZES, ids=_sid)
def test_usm_fwd(size, B, combo, dt):
    """combo "product": out_nchw = NULL, out_nhwc8 and hp (what lowlight_recovery asks for); "all": the three outputs at once."""
    _usm_fwd_case(B, size[0], size[1], combo, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("combo", ["product", "all"])
def test_usm_fwd_640(combo, dt):
    _usm_fwd_case(2, 640, 640, combo, dt)


# (layout, ld, dtype): NCHW f32 | NHWC with ld == VE (one vector load per pixel: 8 x 16 bit, 4 x f32) | NHWC generic ld |
# planar in the compute dtype (vector loads when W % 4 == 0, scalar staging otherwise: both are in USM_SIZES)
USM_LAYOUTS = [("nchw", 0, "f32"), ("nhwc", 8, "bf16"), ("nhwc", 8, "f16"), ("nhwc", 4, "f32"), ("nhwc", 8, "f32"),
               ("nhwc", 16, "f32"), ("nhwc", 16, "bf16"), ("nhwc", 16, "f16"), ("planar", 0, "f32"), ("planar", 0, "bf16"),
               ("planar", 0, "f16")]


def _usm_bwd_case(B, H, W, layout):
    call, ptr, stream, dt_id = _api()
    kind, ld, dt = layout
    dtype = DT[dt]
    c = _usm(B, H, W)
    g, _, _, ref_ds4, ref_dlam, t32, dlam32 = _usm_ref(B, H, W, dt)
    if kind == "nchw":
        src = g.cuda()
        a_nchw, a_8 = ptr(src), None
    elif kind == "planar":
        src = g.to(dtype).cuda()
        a_nchw, a_8 = None, ptr(src)
    else:
        buf = c["pad"][..., :ld].clone()
        buf[..., :3] = g.permute(0, 2, 3, 1)
        src = buf.to(dtype).contiguous().cuda()
        a_nchw, a_8 = None, ptr(src)
    hp, params = c["hp32"].cuda(), c["params"].cuda()
    dp0 = torch.from_numpy(np.random.default_rng(H + W).standard_normal((B, 8)))
    dp = dp0.cuda()
    ds4 = torch.full((B, 3, H, W), 7.0, device="cuda")
    call("dy_usm_bwd", a_nchw, a_8, ld, ptr(hp), ptr(params), ptr(ds4), ptr(dp), B, H, W, dt_id(dtype), stream())
    torch.cuda.synchronize()
    what = f"B={B} {H}x{W} {kind} ld={ld} {dt}"
    _check("usm_ds4", ds4, ref_ds4, t32[2], what)
    got = dp.cpu()
    _check("usm_dlam", (got - dp0)[:, 6:7], ref_dlam[:, None], dlam32[:, None], what)
    keep = [0, 1, 2, 3, 4, 5, 7]
    assert torch.equal(got[:, keep], dp0[:, keep]), "only slot 6 is the USM kernel's"


@pytest.mark.parametrize("layout", USM_LAYOUTS, ids=lambda l: f"{l[0]}{l[1]}_{l[2]}")
@pytest.mark.parametrize("size", USM_SIZES, ids=_sid)
def test_usm_bwd(size, layout):
    _usm_bwd_case(3, size[0], size[1], layout)


@pytest.mark.parametrize("size", USM_SIZES, ids=_sid)
def test_usm_bwd_single_image(size):
    _usm_bwd_case(1, size[0], size[1], USM_LAYOUTS[0])


@pytest.mark.parametrize("layout", [USM_LAYOUTS[0], USM_LAYOUTS[1], USM_LAYOUTS[9]], ids=lambda l: f"{l[0]}{l[1]}_{l[2]}")
def test_usm_bwd_640(layout):
    _usm_bwd_case(2, 640, 640, layout)


# ====================================================================================== dy_image_to_nhwc8 / dy_resize_bwd
# the bench workload's downsampling, the goldens' upsampling, no resize at all, and two odd small ones (down and up)
RESIZE_CASES = [((640, 640), (256, 256)), ((64, 96), (256, 256)), ((256, 256), (256, 256)), ((33, 47), (16, 20)), ((7, 5), (16, 20))]
_rid = lambda c: f"{c[0][0]}x{c[0][1]}to{c[1][0]}x{c[1][1]}"


@functools.lru_cache(maxsize=None)
def _resize(case):
    (H, W), (Ho, Wo) = case
    B = 2
    g = np.random.default_rng(100 * H + W + Ho)
    x = _u(g, 0.0, 1.0, B, 3, H, W)
    gy = _u(g, -1.0, 1.0, B, 3, Ho, Wo)
    pad = _u(g, -1.0, 1.0, B, Ho, Wo, 16)
    dx0 = _u(g, -1.0, 1.0, B, 3, H, W)
    y, dx = fr.resize_fwd_bwd(x, Ho, Wo, gy)
    y32, dx32 = fr.resize_fwd_bwd(x, Ho, Wo, gy, torch.float32)
    return dict(x=x, gy=gy, pad=pad, dx0=dx0, y=y, dx=dx, y32=y32, dx32=dx32, B=B)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", RESIZE_CASES, ids=_rid)
def test_image_to_nhwc8(case, dt):
    call, ptr, stream, dt_id = _api()
    (H, W), (Ho, Wo) = case
    c = _resize(case)
    dtype = DT[dt]
    x = c["x"].cuda()
    y8 = torch.full((c["B"], Ho, Wo, 8), 7.0, device="cuda", dtype=dtype)
    call("dy_image_to_nhwc8", ptr(x), c["B"], H, W, ptr(y8), Ho, Wo, dt_id(dtype), stream())
    torch.cuda.synchronize()
    got = y8[..., :3].permute(0, 3, 1, 2)
    if dtype == torch.float32:
        _check("resize_fwd", got, c["y"], c["y32"], f"{_rid(case)}")
    else:
        _check16("resize_fwd", got, c["y"], dtype, f"{_rid(case)}")
    assert bool((y8[..., 3:] == 0).all()), "pad lanes"


@pytest.mark.parametrize("ld", [3, 8, 16])
@pytest.mark.parametrize("case", RESIZE_CASES, ids=_rid)
def test_resize_bwd(case, ld):
    """The adjoint of the resize, ADDED onto a non-zero dx (the front-end's backward adds it to the filter chain's dx)."""
    call, ptr, stream, _ = _api()
    (H, W), (Ho, Wo) = case
    c = _resize(case)
    buf = c["pad"][..., :ld].clone()
    buf[..., :3] = c["gy"].permute(0, 2, 3, 1)
    dy, dx = buf.contiguous().cuda(), c["dx0"].cuda()
    call("dy_resize_bwd", ptr(dy), ld, c["B"], H, W, Ho, Wo, ptr(dx), stream())
    torch.cuda.synchronize()
    _check("resize_bwd", dx, c["dx0"].double() + c["dx"], c["dx0"].double() + c["dx32"].double(), f"{_rid(case)} ld={ld}")


# ============================================================================================================ module level
def _module_case(dtype):
    import dedark_yolo_amd as dy
    from dedark_yolo_amd.nn.modules import lowlight_recovery
    from oracle import model as om
    from parity_helpers import load_sd
    g = gold("g19_frontend_aica")
    dy.set_compute_dtype(dtype)
    m = lowlight_recovery(3, 3)
    load_sd(m, om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"])))
    m = m.cuda().train()
    x = g["x"].clone().cuda().requires_grad_(True)
    out = m(x, g["A"].cuda(), g["IcA"].cuda())
    (out.float() * g["wgt"].cuda()).sum().backward()
    torch.cuda.synchronize()
    return g, out, x, dict(m.named_parameters())


def test_module_train_with_A_IcA_golden():
    """lowlight_recovery in train mode with A / IcA supplied (what the trainer runs on every darkened batch) at 50 x 76 -- the
    per-wave reduction path of the pointwise backward -- against the reference fixture, at test_frontend_golden's tolerances."""
    from util import close
    g, out, x, named = _module_case(torch.float32)
    close(out.float().cpu(), g["out"], 1e-4, 2e-4, "front-end out")
    close(x.grad.cpu(), g["dx"], 2e-3, 2e-3, "front-end dx")
    close(named["extractor.fc2.weight"].grad.cpu(), g["d_fc2_w"], 2e-3, 2e-2, "d fc2.w")
    close(named["extractor.fc2.bias"].grad.cpu(), g["d_fc2_b"], 2e-3, 2e-2, "d fc2.b")
    close(named["extractor.fc1.bias"].grad.cpu(), g["d_fc1_b"], 2e-3, 2e-2, "d fc1.b")
    close(named["extractor.conv_layers.0.conv_block.0.weight"].grad.cpu(), g["d_c0_w"], 3e-3, 3e-2, "d conv0.w")
    close(named["extractor.conv_layers.4.conv_block.0.bias"].grad.cpu(), g["d_c4_b"], 3e-3, 3e-2, "d conv4.b")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_module_train_with_A_IcA_low_precision(dt):
    """The same in the 16-bit compute dtypes (fast-math pointwise kernels, planar 16-bit gradient into the USM backward), at the
    bounds of test_frontend_golden_low_precision (relative L2)."""
    g, out, x, _ = _module_case(DT[dt])
    rel = lambda a, b: float((a.double().cpu() - b.double()).norm() / b.double().norm())
    e_y, e_dx = rel(out.float(), g["out"]), rel(x.grad, g["dx"])
    print(f"FIGM front-end (A, IcA) {dt}: out {e_y:.2e} dx {e_dx:.2e}")
    assert e_y <= 2e-2 and e_dx <= 5e-2, (e_y, e_dx)


# ========================================================================================================= argument checks
def _bad_calls():
    """name -> (entry, argument builder, tensors that must stay untouched).  Every tensor is legal in size for the LEGAL
    neighbour of the bad argument, so even a check that failed to fire could not write out of bounds."""
    call, ptr, stream, _ = _api()
    z = lambda *s: torch.full(s, 7.0, device="cuda")
    zd = lambda *s: torch.full(s, 7.0, device="cuda", dtype=F64)
    t = dict(img=z(1, 3, 16, 16), a=z(1, 3, 16, 16), b=z(1, 3, 16, 16), c=z(1, 3, 16, 16), o8=z(1, 16, 16, 8), p=z(1, 8), dp=zd(1, 8),
             feat=z(2, 16), dfeat=z(2, 16), prm=z(2, 8), dpf=zd(2, 8))
    p, st = ptr, stream()
    calls = {
        "usm_fwd_H12": ("dy_usm_fwd", (p(t["img"]), p(t["p"]), p(t["a"]), p(t["o8"]), p(t["b"]), 1, 12, 16, 0, st)),
        "usm_fwd_W12": ("dy_usm_fwd", (p(t["img"]), p(t["p"]), p(t["a"]), p(t["o8"]), p(t["b"]), 1, 16, 12, 0, st)),
        "usm_bwd_H12": ("dy_usm_bwd", (p(t["img"]), None, 0, p(t["b"]), p(t["p"]), p(t["a"]), p(t["dp"]), 1, 12, 16, 0, st)),
        "usm_bwd_W12": ("dy_usm_bwd", (p(t["img"]), None, 0, p(t["b"]), p(t["p"]), p(t["a"]), p(t["dp"]), 1, 16, 12, 0, st)),
        "usm_bwd_both": ("dy_usm_bwd", (p(t["img"]), p(t["c"]), 0, p(t["b"]), p(t["p"]), p(t["a"]), p(t["dp"]), 1, 16, 16, 0, st)),
        "usm_bwd_neither": ("dy_usm_bwd", (None, None, 0, p(t["b"]), p(t["p"]), p(t["a"]), p(t["dp"]), 1, 16, 16, 0, st)),
        "pointwise_fwd_W2": ("dy_filters_pointwise_fwd", (p(t["img"]), p(t["p"]), None, None, p(t["a"]), 1, 16, 2, 0, st)),
        "pointwise_bwd_W2": ("dy_filters_pointwise_bwd", (p(t["img"]), p(t["p"]), None, None, p(t["b"]), p(t["a"]), p(t["dp"]),
                                                          1, 16, 2, 0, 0, st)),
        "params_fwd_ld14": ("dy_filter_params_fwd", (p(t["feat"]), 14, p(t["prm"]), 2, st)),
        "params_bwd_ld14": ("dy_filter_params_bwd", (p(t["feat"]), 14, p(t["dpf"]), p(t["dfeat"]), 2, st)),
    }
    return call, t, calls


@pytest.mark.parametrize("name", ["usm_fwd_H12", "usm_fwd_W12", "usm_bwd_H12", "usm_bwd_W12", "usm_bwd_both", "usm_bwd_neither",
                                  "pointwise_fwd_W2", "pointwise_bwd_W2", "params_fwd_ld14", "params_bwd_ld14"])
def test_argument_checks_raise_and_launch_nothing(name):
    call, t, calls = _bad_calls()
    entry, args = calls[name]
    with pytest.raises(RuntimeError, match=entry):
        call(entry, *args)
    torch.cuda.synchronize()
    for k, v in t.items():
        assert bool((v == 7.0).all()), f"{name}: {k} was written"
