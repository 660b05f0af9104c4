"""GPU tests of the SCConv C2f family.

Kernel level: the C-ABI entries of csrc/cru.hip (dy_cru_conv_pack / fwd / dgrad / wgrad) called directly, each against the float64
statement of tests/scc2f_ref.py on the same tensors (inputs drawn exactly representable in the storage dtype, as
tests/test_gpu_scconv_asff_kernels.py does).  Every operand is a channel slice of a wider parent filled with a sentinel, at lane 8
(16-byte aligned: the vector paths where the widths allow them) or lane 3 (element alignment only); the lanes outside every view
must survive every call.  Shapes: SCConv widths C = 16 / 48 / 80 / 64 (GWC group inputs of 2 / 6 / 10 / 8 channels), B = 2, maps of
5 x 7 and 9 x 12 (borders on all sides, 70 and 216 pixels: no multiple of the 64-pixel tile, two and four blocks), for the up branch
(GWC + PWC1 in one accumulator, 2 groups) and the two kinds of 1x1 (squeeze: C/2 -> C/4, PWC2: C/4 -> 3C/4).

Error measure: scconv_ref.sum_err, |got - ref| / sum |terms| with the terms of the sum that forms the element (K = 11 C/8 + bias
for the up branch forward, 9 C/2 + C for its data gradient, the pixels for the weight gradients).  Bound: the one
test_gpu_scconv_asff_kernels.py holds its f32 running sums to (BOUNDS["moments"] = 2e-6; the MFMA accumulators are k-ordered f32 fma
chains, the weight gradient adds f32 partials in a fixed order); 16-bit outputs get that bound plus one ulp of the type at the
reference value (prior + reference for an accumulating destination), the allowance of that file's _check16.  The worst ratio of
every case is printed.

Module level (fp32): the eight blocks against the reference's fixtures g28_scc2f_<block>_c<c>_<sc|nosc> within the project's block
bound (test_gpu_parity._run_block: 1e-4 outputs, 2e-3 gradients, as test_gpu_ghost / test_gpu_faster); the fixtures' seeds leave
no ambiguous SRU element (tests/golden/g28_scc2f_blocks.json: share 0 <= the 1e-3 cap), so nothing is left out of any comparison.
The whole yolov8n-SCC2f model against g28_scc2f_n_tiny: loss and items within 1e-4, gradients and maps within test_gpu_ghost's
bounds.  A bf16 training smoke at scales n and m and a last.pt round trip.
"""
import numpy as np
import pytest
import torch

import scc2f_ref as sc
import scconv_ref as sr
from util import close, gold, load_yaml, make_batch, rnd

pytestmark = pytest.mark.gpu

from test_gpu_scconv_asff_kernels import BOUNDS as _SCCONV_BOUNDS  # noqa: E402

BOUND = _SCCONV_BOUNDS["moments"]          # f32 running sums
DT = sr.DT
F64 = torch.float64
SENTINEL = 99.0
WIDTHS = (16, 48, 80, 64)
MAPS = ((5, 7), (9, 12))
B = 2


@pytest.fixture(autouse=True)
def _fp32():
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(torch.float32)
    yield
    dy.set_compute_dtype(torch.float32)


def _dims(kind, C):
    """(G, N, C3, C1) of the CRU conv `kind` at SCConv width C"""
    h, q, e = C // 2, C // 4, C // 8
    return dict(up=(2, h, e, q), squeeze=(1, q, 0, h), pwc2=(1, 3 * q, 0, q))[kind]


class View:
    """[B, C, H, W] NHWC view at lanes [c0, c0 + C) of a [B, H, W, ld] parent full of the sentinel"""

    def __init__(self, H, W, C, c0, dtype, fill=float("nan")):
        self.C, self.c0 = C, c0
        self.ld = c0 + C + (8 if c0 % 8 == 0 else 5)
        if c0 % 8 == 0:
            self.ld = (self.ld + 7) // 8 * 8
        self.parent = torch.full((B, H, W, self.ld), SENTINEL, device="cuda", dtype=dtype)
        self.parent[..., c0:c0 + C] = fill.permute(0, 2, 3, 1).to(dtype).cuda() if isinstance(fill, torch.Tensor) else fill
        self.ptr = self.parent.data_ptr() + c0 * self.parent.element_size()

    def get(self):
        return self.parent[..., self.c0:self.c0 + self.C].permute(0, 3, 1, 2).double().cpu()

    def intact(self, what):
        p = self.parent
        assert bool((p[..., :self.c0] == SENTINEL).all()) and bool((p[..., self.c0 + self.C:] == SENTINEL).all()), f"{what}: wrote outside the view"


class Flat:
    """n elements followed by 16 sentinels"""

    def __init__(self, n, dtype, fill=float("nan")):
        self.n = n
        self.buf = torch.full((n + 16,), SENTINEL, device="cuda", dtype=dtype)
        self.buf[:n] = fill
        self.ptr = self.buf.data_ptr()

    def get(self, *shape):
        return self.buf[:self.n].double().cpu().reshape(*shape)

    def intact(self, what):
        assert bool((self.buf[self.n:] == SENTINEL).all()), f"{what}: wrote past the end"


def _ratio(got, ref, terms, dt, what, at=None):
    """worst |got - ref| / allowance; allowance = BOUND * sum |terms| (+ one ulp of a 16-bit output type at the reference value)"""
    got, ref, terms = got.double(), ref.double(), terms.double()
    assert got.shape == ref.shape == terms.shape and torch.isfinite(got).all(), what
    if dt == "f32" or at == "f32":
        e = sr.sum_err(got, ref, terms)
        print(f"FIG {what}: sum_err {e:.3e} = {e / BOUND:.3f} of the bound")
        assert e <= BOUND, f"{what}: {e:.3e} > {BOUND:.0e}"
        return
    tol = BOUND * terms + sr.ulp(ref, DT[dt])
    over = float(((got - ref).abs() / tol).max())
    print(f"FIG16 {what}: {over:.3f} of the allowance")
    assert over <= 1.0, f"{what}: {over:.3f} x (bound + 1 ulp)"


def _call(name, *args):
    from dedark_yolo_amd import _C, ops
    _C.call(name, *args, ops.stream())


def _kernel_case(kind, C, dt, c0, H, W):
    from dedark_yolo_amd import ops
    G, N, C3, C1 = _dims(kind, C)
    GN, K = G * N, 9 * C3 + C1
    dtype, did = DT[dt], ops.dt_id(DT[dt])
    tag = f"{kind} C={C} {dt} lane {c0} {B}x{H}x{W}"
    g = np.random.default_rng(sr._seed("cru_conv", kind, C, dt, H, W))
    x = sr._randn(g, B, C1, H, W, dt=dt)
    w1 = sr._randn(g, GN, C1, 1, 1, dt=dt, scale=K ** -0.5)
    w3 = sr._randn(g, GN, C3, 3, 3, dt=dt, scale=K ** -0.5) if C3 else None
    bias = sr._randn(g, GN, dt=dt, scale=0.3) if C3 else None
    dy = sr._randn(g, B, GN, H, W, dt=dt)
    prior = sr._randn(g, B, C1, H, W, dt=dt)
    x64, w164, dy64 = x.double(), w1.double(), dy.double()
    w364, b64 = (w3.double(), bias.double()) if C3 else (None, None)
    w1d, w3d, bd = w1.cuda(), (w3.cuda() if C3 else None), (bias.cuda() if C3 else None)
    p3, pb = (w3d.data_ptr(), bd.data_ptr()) if C3 else (None, None)

    # weight packs: forward and transposed, exactly G N (9 C3 + C1) elements each
    packs = [Flat(GN * K, dtype) for _ in range(2)]
    for tr, pk in enumerate(packs):
        _call("dy_cru_conv_pack", p3, w1d.data_ptr(), pk.ptr, G, N, C3, C1, tr, did)

    # forward
    xv, yv = View(H, W, C1, c0, dtype, x), View(H, W, GN, c0, dtype)
    _call("dy_cru_conv_fwd", xv.ptr, xv.ld, packs[0].ptr, pb, yv.ptr, yv.ld, B, H, W, G, N, C3, C1, did)
    torch.cuda.synchronize()
    _ratio(yv.get(), sc.cru_conv_ref(x64, w364, b64, w164, G), sc.cru_conv_fwd_terms(x64, w364, b64, w164, G), dt, f"fwd {tag}")
    for v in (xv, yv, *packs):
        v.intact(f"fwd {tag}")

    # data gradient: plain, then adding into a prior
    gv, d0, d1 = View(H, W, GN, c0, dtype, dy), View(H, W, C1, c0, dtype), View(H, W, C1, c0, dtype, prior)
    _call("dy_cru_conv_dgrad", gv.ptr, gv.ld, packs[1].ptr, d0.ptr, d0.ld, B, H, W, G, N, C3, C1, 0, did)
    _call("dy_cru_conv_dgrad", gv.ptr, gv.ld, packs[1].ptr, d1.ptr, d1.ld, B, H, W, G, N, C3, C1, 1, did)
    torch.cuda.synchronize()
    ref = sc.cru_conv_dgrad_ref(dy64, w364, w164, G, x64.shape)
    terms = sc.cru_conv_dgrad_terms(dy64, w364, w164, G, x64.shape)
    _ratio(d0.get(), ref, terms, dt, f"dgrad {tag}")
    _ratio(d1.get(), prior.double() + ref, terms + prior.double().abs(), dt, f"dgrad accumulate {tag}")
    for v in (gv, d0, d1, packs[1]):
        v.intact(f"dgrad {tag}")

    # weight and bias gradients (f32), twice: identical bytes
    scratch = Flat(1 << 20, torch.float32)
    runs = []
    for _ in range(2):
        o3, ob, o1 = (Flat(GN * C3 * 9, torch.float32) if C3 else None), (Flat(GN, torch.float32) if C3 else None), Flat(GN * C1, torch.float32)
        _call("dy_cru_conv_wgrad", xv.ptr, xv.ld, gv.ptr, gv.ld, o3.ptr if C3 else None, ob.ptr if C3 else None, o1.ptr, B, H, W, G, N, C3, C1,
              scratch.ptr, scratch.n, did)
        runs.append((o3, ob, o1))
    torch.cuda.synchronize()
    r3, rb, r1 = sc.cru_conv_wgrad_ref(x64, dy64, None if w3 is None else w3.shape, w1.shape, G)
    t3, tb, t1 = sc.cru_conv_wgrad_terms(x64, dy64, None if w3 is None else w3.shape, w1.shape, G)
    o3, ob, o1 = runs[0]
    _ratio(o1.get(*w1.shape), r1, t1, dt, f"wgrad 1x1 {tag}", at="f32")
    if C3:
        _ratio(o3.get(*w3.shape), r3, t3, dt, f"wgrad 3x3 {tag}", at="f32")
        _ratio(ob.get(GN), rb, tb, dt, f"wgrad bias {tag}", at="f32")
    for a, b_ in zip(runs[0], runs[1]):
        if a is not None:
            assert torch.equal(a.buf, b_.buf), f"wgrad {tag}: two runs differ"
            a.intact(f"wgrad {tag}")
    for v in (xv, gv, scratch):
        v.intact(f"wgrad {tag}")


@pytest.mark.parametrize("c0", [8, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("kind", ["up", "squeeze", "pwc2"])
def test_cru_conv_kernels_vs_f64(kind, C, dt, c0):
    for H, W in MAPS:
        _kernel_case(kind, C, dt, c0, H, W)


def test_cru_wgrad_many_ranges_is_deterministic_and_exact():
    """a map with many pixel ranges, and a scratch that caps their number: each setting bit-identical run to run and within the bound"""
    from dedark_yolo_amd import ops
    C, H, W = 48, 33, 31
    G, N, C3, C1 = _dims("up", C)
    g = np.random.default_rng(11)
    x, dy = sr._randn(g, B, C1, H, W), sr._randn(g, B, G * N, H, W)
    xv, gv = View(H, W, C1, 8, torch.float32, x), View(H, W, G * N, 8, torch.float32, dy)
    r3, rb, r1 = sc.cru_conv_wgrad_ref(x.double(), dy.double(), (G * N, C3, 3, 3), (G * N, C1, 1, 1), G)
    t3, tb, t1 = sc.cru_conv_wgrad_terms(x.double(), dy.double(), (G * N, C3, 3, 3), (G * N, C1, 1, 1), G)
    slab = G * N * (9 * C3 + C1 + 1)
    for elems in (1 << 22, 3 * slab):
        scratch = Flat(elems, torch.float32)
        outs = []
        for _ in range(2):
            o3, ob, o1 = Flat(G * N * C3 * 9, torch.float32), Flat(G * N, torch.float32), Flat(G * N * C1, torch.float32)
            _call("dy_cru_conv_wgrad", xv.ptr, xv.ld, gv.ptr, gv.ld, o3.ptr, ob.ptr, o1.ptr, B, H, W, G, N, C3, C1, scratch.ptr, scratch.n, ops.dt_id(torch.float32))
            outs.append((o3, ob, o1))
        torch.cuda.synchronize()
        assert all(torch.equal(a.buf, b_.buf) for a, b_ in zip(*outs))
        scratch.intact("scratch")
        _ratio(outs[0][0].get(G * N, C3, 3, 3), r3, t3, "f32", f"wgrad 3x3, scratch {elems}")
        _ratio(outs[0][1].get(G * N), rb, tb, "f32", f"wgrad bias, scratch {elems}")
        _ratio(outs[0][2].get(G * N, C1, 1, 1), r1, t1, "f32", f"wgrad 1x1, scratch {elems}")


def test_cru_conv_rejects_bad_arguments():
    from dedark_yolo_amd import _C, ops
    x = torch.zeros((1, 4, 4, 16), device="cuda")
    wp = torch.zeros(4096, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported CRU conv"):      # the 3x3 group inputs do not tile the 1x1 input
        _C.call("dy_cru_conv_fwd", x.data_ptr(), 16, wp.data_ptr(), None, x.data_ptr(), 16, 1, 4, 4, 2, 8, 3, 4, 0, ops.stream())
    with pytest.raises(RuntimeError, match="bad dtype"):
        _C.call("dy_cru_conv_fwd", x.data_ptr(), 16, wp.data_ptr(), None, x.data_ptr(), 16, 1, 4, 4, 1, 8, 0, 8, 7, ops.stream())
    with pytest.raises(RuntimeError, match="bad view"):
        _C.call("dy_cru_conv_dgrad", x.data_ptr(), 4, wp.data_ptr(), x.data_ptr(), 16, 1, 4, 4, 1, 8, 0, 8, 0, 0, ops.stream())
    with pytest.raises(RuntimeError, match="scratch"):
        _C.call("dy_cru_conv_wgrad", x.data_ptr(), 16, x.data_ptr(), 16, None, None, wp.data_ptr(), 1, 4, 4, 1, 8, 0, 8, wp.data_ptr(), 8, 0, ops.stream())
    # source and destination lanes that overlap inside one buffer (in place, or halves cut 4 lanes too close) are refused and launch
    # nothing: a thread reads all channels of a pixel and its 3x3 halo, which other threads write.  Sibling halves are fine.
    G, N, C3, C1, H, W = 2, 4, 4, 8, 8, 8
    g = np.random.default_rng(12)
    buf = sr._randn(g, 1, 16, H, W).permute(0, 2, 3, 1).contiguous().cuda()
    w3, w1 = sr._randn(g, G * N, C3, 3, 3, scale=0.15), sr._randn(g, G * N, C1, 1, 1, scale=0.15)
    w3d, w1d = w3.cuda(), w1.cuda()
    packs = [torch.empty(G * N * (9 * C3 + C1), device="cuda") for _ in range(2)]
    for tr, pk in enumerate(packs):
        _call("dy_cru_conv_pack", w3d.data_ptr(), w1d.data_ptr(), pk.data_ptr(), G, N, C3, C1, tr, 0)
    a, b_, c = buf[..., :8], buf[..., 4:12], buf[..., 8:]
    for dst in (a, b_):
        for name, args in (("dy_cru_conv_fwd", (a.data_ptr(), 16, packs[0].data_ptr(), None, dst.data_ptr(), 16, 1, H, W, G, N, C3, C1, 0)),
                           ("dy_cru_conv_dgrad", (dst.data_ptr(), 16, packs[1].data_ptr(), a.data_ptr(), 16, 1, H, W, G, N, C3, C1, 0, 0))):
            _C.lib().dy_clear_last_kernel()
            with pytest.raises(RuntimeError, match="overlap"):
                _C.call(name, *args, ops.stream())
            assert _C.lib().dy_last_kernel().decode() == ""
    x64 = a.permute(0, 3, 1, 2).double().cpu()
    _call("dy_cru_conv_fwd", a.data_ptr(), 16, packs[0].data_ptr(), None, c.data_ptr(), 16, 1, H, W, G, N, C3, C1, 0)
    torch.cuda.synchronize()
    y = c.permute(0, 3, 1, 2).double().cpu()
    _ratio(y, sc.cru_conv_ref(x64, w3.double(), None, w1.double(), G), sc.cru_conv_fwd_terms(x64, w3.double(), None, w1.double(), G), "f32",
           "fwd into the sibling half")
    assert torch.equal(a.permute(0, 3, 1, 2).double().cpu(), x64)
    _call("dy_cru_conv_dgrad", c.data_ptr(), 16, packs[1].data_ptr(), a.data_ptr(), 16, 1, H, W, G, N, C3, C1, 0, 0)
    torch.cuda.synchronize()
    _ratio(a.permute(0, 3, 1, 2).double().cpu(), sc.cru_conv_dgrad_ref(y, w3.double(), w1.double(), G, x64.shape),
           sc.cru_conv_dgrad_terms(y, w3.double(), w1.double(), G, x64.shape), "f32", "dgrad into the sibling half")
    assert torch.equal(c.permute(0, 3, 1, 2).double().cpu(), y)


# ------------------------------------------------------------------------------------------------ modules
def test_scconv_at_a_width_that_is_no_multiple_of_64():
    """SCConv(48), forward and backward through autograd, against the f64 statement on the same weights (fp32: the block bounds)"""
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn.modules import SCConv, SCConvBottleneck
    m = SCConv(48)
    g = gold(sc.block_name("SCConvBottleneck", 48, True))            # its x0 is an SCConv(48) input without ambiguous elements
    pre = "SandCRblock.0."
    full = om.rng_fill({k: tuple(v.shape) for k, v in SCConvBottleneck(48, 48).state_dict().items()}, int(g["seed"]))
    sd = {k[len(pre):]: v for k, v in full.items() if k.startswith(pre)}
    load_sd(m, sd)
    m = m.cuda().train()
    x = g["x0"].clone().cuda().requires_grad_(True)
    y = m(x)
    wgt = rnd(900, *y.shape, lo=-1, hi=1)
    (y.float() * wgt.cuda()).sum().backward()
    torch.cuda.synchronize()
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xt = g["x0"].double().requires_grad_(True)
    yt, gn, _ = sc.scconv(sd64, "", xt)
    assert int((gn.abs() < sr.AMBIG).sum()) == 0
    (yt * wgt.double()).sum().backward()
    close(y.float().cpu(), yt.detach(), 1e-4, 1e-4, "SCConv(48) y")
    close(x.grad.float().cpu(), xt.grad, 2e-3, 2e-3, "SCConv(48) dx")
    for k, p in m.named_parameters():
        close(p.grad.cpu(), sd64[k].grad, 2e-3, 2e-3, f"SCConv(48) {k}")


@pytest.mark.parametrize("cls,c,shortcut", sc.BLOCK_CASES, ids=[sc.block_name(*k)[10:] for k in sc.BLOCK_CASES])
def test_scc2f_blocks_golden(cls, c, shortcut):
    """output, dx, every parameter gradient and the BatchNorm running statistics after the step, in fp32, within the project's block
    bound (test_gpu_parity._run_block: 1e-4 on outputs, 2e-3 on gradients); nothing is left out (no ambiguous SRU element)"""
    from test_gpu_parity import _run_block
    from dedark_yolo_amd.nn import modules
    _run_block(sc.block_name(cls, c, shortcut), getattr(modules, cls)(*sc.block_args(cls, c, shortcut)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("cls,c", [("SCConvBottleneck", 16), ("SC_PW_Bottleneck", 48), ("Conv3_SC_C2f", 48), ("SCC2f", 64)])
def test_scc2f_blocks_low_precision_match_the_statement(cls, c, dtype):
    """16-bit train-mode forward and backward against the f64 statement on the same weights: test_gpu_ghost's 16-bit block bound
    (4 x its single-kernel tolerance, scaled by the largest value); the fixture inputs have no ambiguous SRU element in f64, and a
    16-bit gate may still fall the other way on elements near zero, which moves values of that size only"""
    import dedark_yolo_amd as dy
    from oracle import model as om
    from parity_helpers import load_sd, set_bn
    from test_gpu_ghost import _tol
    from dedark_yolo_amd.nn import modules
    args = sc.block_args(cls, c, True)
    g = gold(sc.block_name(cls, c, True))
    m = getattr(modules, cls)(*args)
    sd = om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"]))
    load_sd(set_bn(m), sd)
    dy.set_compute_dtype(dtype)
    m = m.cuda().train()
    x = g["x0"].clone().cuda().requires_grad_(True)
    y = m(x)
    wgt = rnd(900, *y.shape, lo=-1, hi=1)
    (y.float() * wgt.cuda()).sum().backward()
    torch.cuda.synchronize()
    sd64 = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in sd.items()}
    xt = g["x0"].double().requires_grad_(True)
    yt = sc.block(cls, args, sd64, xt)
    (yt * wgt.double()).sum().backward()
    t = 4 * _tol(dtype)
    for got, want, what in ((y, yt.detach(), "y"), (x.grad, xt.grad, "dx")):
        err = float((got.double().cpu() - want).abs().max())
        print(f"{cls} c{c} {dtype} {what}: {err:.3e} (ref max {float(want.abs().max()):.3e})")
        assert torch.isfinite(got).all() and err <= t * (float(want.abs().max()) + 1.0), (what, err)
    named = dict(m.named_parameters())
    gtop = max(float(v.grad.abs().max()) for v in sd64.values() if getattr(v, "grad", None) is not None)
    for k, v in sd64.items():
        if getattr(v, "grad", None) is not None:
            err = float((named[k].grad.double().cpu() - v.grad).abs().max())
            assert err <= t * (gtop + 1.0), (k, err, gtop)


# ------------------------------------------------------------------------------------------------ models
def _cfg(scale, block="SCC2f"):
    d = load_yaml("yolov8-SCC2f.yaml")
    d["scale"] = scale
    for row in d["backbone"] + d["head"]:
        if row[2] == "SCC2f":
            row[2] = block
    return d


def test_scc2f_model_step_golden():
    """yolov8n-SCC2f at 64x64, B = 2: loss and items within 1e-4 (the project's parity gate); selected gradients, running statistics
    and the three eval maps within the bounds test_gpu_ghost.py uses for g25_ghost_n_tiny"""
    import dedark_yolo_amd as dy
    from oracle import model as om
    from parity_helpers import HYP, load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    name = "g28_scc2f_n_tiny"
    g = gold(name)
    assert float(g["sru_share"]) <= sr.SHARE_CAP
    dy.set_compute_dtype(torch.float32)
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
    print(f"{name}: loss {float(loss):.6f} vs {float(g['loss']):.6f}")
    close(float(loss.detach()), g["loss"], 1e-4, 1e-4, f"{name} loss vs reference golden")
    close(items.float().cpu(), g["items"], 1e-4, 1e-4, f"{name} items vs reference golden")
    named = dict(model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in named.values() if p.requires_grad)
    gtol = 5e-3
    msd = model.state_dict()
    n_sc = 0
    for k, v in g.items():
        if k.startswith("gn:"):
            close(named[k[3:]].grad.norm().cpu(), v, gtol, 1e-6, f"{name} {k}")
        elif k.startswith("g:"):
            close(named[k[2:]].grad.cpu(), v, gtol, gtol * float(v.abs().max()), f"{name} {k}")
            n_sc += ".CRU." in k or ".SRU." in k
        elif k.startswith("b:"):
            close(msd[k[2:]].cpu(), v, 1e-4, 1e-4, f"{name} {k}")
    assert n_sc >= 32
    model.eval()
    with torch.no_grad():
        out = model(batch["img"])
    y, maps = out[0], out[1]
    assert abs(float(y.float().sum()) - float(g["ysum"])) <= 1e-4 * float(y.float().abs().sum())
    for i in range(3):
        want = g[f"map{i}"]
        err = float((maps[i].float().cpu() - want).abs().max()) / float(want.abs().max())
        assert maps[i].shape == want.shape and err <= 1e-4, (i, err)


@pytest.mark.parametrize("block", ["SC_PW_C2f", "SC_Conv3_C2f", "Conv3_SC_C2f"])
def test_yaml_variants_run_a_step(block):
    from parity_helpers import HYP
    from dedark_yolo_amd.nn.tasks import DetectionModel
    torch.manual_seed(5)
    model = DetectionModel(_cfg("n", block), ch=3, nc=20)
    model.args = HYP
    model = model.cuda().train()
    batch = make_batch(77, 2, 64, [2, 1])
    batch["img"] = batch["img"].cuda()
    batch["recovery_loss_batch"] = torch.tensor(0.0).cuda()
    loss, _ = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.requires_grad)


def _trainer(name, tmp=None):
    import bench
    from dedark_yolo_amd import YOLO
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    torch.manual_seed(3)
    tr = DetectionTrainer(get_cfg(dict(model=name, dtype="bf16", optimizer="SGD", batch=2, lowlight_FLAG=False, dedark_FLAG=False)))
    tr.setup(YOLO(name).model)
    losses = []
    for step in range(2):
        b = bench.synth_batch(80 + step, 2, 64, 20, "cuda")
        tr.args.dark_param = b.pop("gamma")
        b.pop("n_max", None)
        scp = [(k, p) for k, p in tr.model.named_parameters() if ".SRU." in k or ".CRU." in k]
        for _, p in scp:
            p.grad.fill_(float("nan"))           # the kernels overwrite the slots of the flat gradient buffer: one that is skipped stays NaN
        loss, _ = tr.train_step(b, [0.01] * 3, 0.9)
        torch.cuda.synchronize()
        losses.append(float(loss))
        for k, p in scp:                         # every SCConv parameter received a gradient
            assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, k
    return tr, losses


@pytest.mark.parametrize("name", ["yolov8n-SCC2f.yaml", "yolov8m-SCC2f.yaml"])
def test_bf16_training_smoke(name):
    """YOLO(name), two bf16 steps at 64x64, B = 2: finite losses, finite parameters, a gradient for every SCConv parameter"""
    tr, losses = _trainer(name)
    assert all(np.isfinite(v) for v in losses), losses
    assert bool(torch.isfinite(tr.flat.p).all()) and bool(torch.isfinite(tr.flat.g).all())
    n_sc = sum(1 for k, _ in tr.model.named_parameters() if ".CRU.GWC.weight" in k)
    assert n_sc == {"yolov8n-SCC2f.yaml": 6, "yolov8m-SCC2f.yaml": 12}[name]


def test_last_pt_round_trip(tmp_path):
    """last.pt of yolov8n-SCC2f in the reference's format, read back by our reader: same keys, the trained weights at half precision,
    and a model built from the file gives, bit for bit, the eval output of those weights"""
    from dedark_yolo_amd.nn.tasks import DetectionModel
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint
    tr, _ = _trainer("yolov8n-SCC2f.yaml")
    last = tr.save_model(str(tmp_path / "w"), epoch=0, fitness=0.1)
    ck = load_checkpoint(last)
    assert ck.source == "reference-pickle" and list(ck.model_sd) == list(tr.model.state_dict())
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
