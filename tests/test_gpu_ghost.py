"""GPU tests of the Ghost variants: the depthwise kernels (dy_dwconv_fwd / dgrad / wgrad, dy_copy2d_exact through ctypes) against torch's
grouped convolution, the DWConv / GhostConv / GhostBottleneck / C3 / C3Ghost blocks and whole yolov8n-ghost models against the
reference's fixtures (tests/golden/make_ghost_golden.py), the 16-bit paths, fuse(), and a trainer step with its checkpoint."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ghost_ref
from util import close, gold, load_yaml, make_batch, rnd

pytestmark = pytest.mark.gpu

CS = [1, 3, 4, 8, 12, 20, 32, 72, 128]
KS = [(3, 1), (3, 2), (5, 1), (5, 2)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
RPAD = 5                   # foreign lanes on the right of the C-channel views (live neighbours in a concat buffer)
# foreign lanes on the left: 3 = a slice start that is not vector-aligned in any dtype (every access is a single element);
# 8 = a 16-byte aligned start, so the width decides: whole 16-byte vectors, 8-byte halves (4 / 12 / 20 channels in 16-bit) or elements
LPADS = [3, 8]


@pytest.fixture(autouse=True)
def _fp32():
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(torch.float32)
    yield
    dy.set_compute_dtype(torch.float32)


def _wide(B, H, W, C, dtype, fill, seed, lpad):
    """[B, C, H, W] view into a [B, H, W, lpad + C + rpad] buffer: view = uniform(-1, 1) (or `fill`), left lanes NaN, right lanes +inf.
    lpad 8 comes with rpad 8, so that the pixel stride keeps the alignment the width allows"""
    rpad = RPAD if lpad == 3 else 8
    buf = torch.empty((B, H, W, lpad + C + rpad), dtype=dtype, device="cuda")
    buf[..., :lpad] = float("nan")
    buf[..., lpad + C:] = float("inf")
    v = buf[..., lpad:lpad + C]
    v.copy_(rnd(seed, B, H, W, C, lo=-1, hi=1) if fill is None else torch.full((B, H, W, C), fill))
    return (buf, lpad), v.permute(0, 3, 1, 2)


def _sentinels_intact(bl, C):
    buf, lpad = bl
    return bool(torch.isnan(buf[..., :lpad]).all()) and bool(torch.isposinf(buf[..., lpad + C:]).all())


def _call(name, *args):
    from dedark_yolo_amd import _C, ops
    _C.lib().dy_clear_last_kernel()
    _C.call(name, *args, ops.stream())
    return _C.lib().dy_last_kernel().decode()


def _tol(dtype):
    return {torch.float32: 2e-5, torch.bfloat16: 1.6e-2, torch.float16: 2e-3}[dtype]


def _check(got, want, dtype, what):
    got, want = got.double().cpu(), want.double().cpu()
    err = float((got - want).abs().max())
    print(f"{what}: max abs err {err:.3e} (ref max {float(want.abs().max()):.3e})")
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    assert err <= _tol(dtype) * (float(want.abs().max()) + 1.0), f"{what}: max abs err {err:.3e} (ref max {float(want.abs().max()):.3e})"


def _shapes(C):
    s = [(2, 7, 9)]
    if C in (32, 128):
        s.append((2, 11, 37))
    if C == 8:
        s.append((1, 2, 5))        # smaller than the window in one direction
    return s


def _kernel_case(C, k, s, dtype, lpad, B, H, W):
    from dedark_yolo_amd import ops
    did = ops.dt_id(dtype)
    ref_dt = torch.float64 if dtype == torch.float32 else torch.float32
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    tag = f"C={C} k={k} s={s} {B}x{H}x{W} lpad={lpad}"
    w = (rnd(7 + C + k, C, 1, k, k, lo=-1, hi=1) / k).cuda()
    xb, x = _wide(B, H, W, C, dtype, None, 1 + C, lpad)
    yb, y = _wide(B, Ho, Wo, C, dtype, 0.0, 0, lpad)
    xr, wr = x.to(ref_dt).cpu(), w.to(ref_dt).cpu()
    z_true = F.conv2d(xr, wr, None, s, pad, 1, C)

    # forward, epilogue mode: scale / shift + SiLU, LeakyReLU, none (NULL scale = 1)
    scale, shift = rnd(11 + C, C, lo=0.5, hi=1.5).cuda(), rnd(12 + C, C, lo=-0.5, hi=0.5).cuda()
    for act, fn in ((1, F.silu), (2, lambda t: F.leaky_relu(t, 0.1)), (0, lambda t: t)):
        kn = _call("dy_dwconv_fwd", x.data_ptr(), ops.ld_of(x), y.data_ptr(), ops.ld_of(y), w.data_ptr(), B, H, W, C, k, s,
                   scale.data_ptr() if act else None, shift.data_ptr(), act, None, 0, did)
        assert kn.startswith("dwconv_kernel<fwd"), kn
        torch.cuda.synchronize()
        sc = scale.to(ref_dt).cpu().view(1, -1, 1, 1) if act else 1.0
        _check(y, fn(z_true * sc + shift.to(ref_dt).cpu().view(1, -1, 1, 1)), dtype, f"fwd act={act} {tag}")
    assert _sentinels_intact(yb, C) and _sentinels_intact(xb, C)

    # forward, statistics mode: raw z, and the 64 replicas add up to the f64 sums of the accumulators.  The accumulators are f32 FMA
    # chains (relative error ~k*k * 6e-8 of sum |x w| each), so a channel's sum over n pixels is good to ~1e-6 of sum |z| and the sum
    # of squares to ~1e-6 of itself: 1e-5 relative to those two scales.  This is a deliberate reading of "within 1e-5 relative": the
    # plain sum is bounded against sum |z|, not against |sum z|, because the channels of a random input nearly cancel and no f32
    # accumulator can give 1e-5 of a sum that is itself ~1e-3 of sum |z|; the sum of squares, which cannot cancel, is bounded
    # against itself as the words say.
    cpad = ops.round_up(C, 8)
    stats = torch.zeros(64 * 2 * cpad, dtype=torch.float64, device="cuda")
    kn = _call("dy_dwconv_fwd", x.data_ptr(), ops.ld_of(x), y.data_ptr(), ops.ld_of(y), w.data_ptr(), B, H, W, C, k, s, None, None, 0,
               stats.data_ptr(), cpad, did)
    assert kn.startswith("dwconv_kernel<fwd,stats"), kn
    torch.cuda.synchronize()
    _check(y, z_true, dtype, f"fwd raw z {tag}")
    st = stats.view(64, 2, cpad).sum(0).cpu()
    zt = z_true.double()
    s1, s2, sa = zt.sum((0, 2, 3)), (zt * zt).sum((0, 2, 3)), zt.abs().sum((0, 2, 3))
    e1, e2 = (st[0, :C] - s1).abs(), (st[1, :C] - s2).abs()
    print(f"stats {tag}: sum err/scale {float((e1 / (sa + 1e-30)).max()):.3e}, sumsq rel err {float((e2 / (s2 + 1e-30)).max()):.3e}")
    assert bool((e1 <= 1e-5 * sa + 1e-30).all()) and bool((e2 <= 1e-5 * s2 + 1e-30).all())
    assert float(st[:, C:].abs().max()) == 0.0 if cpad > C else True
    assert _sentinels_intact(yb, C)

    # data gradient: plain, then accumulate + add_src into a slice that already holds values
    gb, g = _wide(B, Ho, Wo, C, dtype, None, 100 + C, lpad)
    sb, sv = _wide(B, H, W, C, dtype, None, 200 + C, lpad)
    db, dx = _wide(B, H, W, C, dtype, None, 300 + C, lpad)
    d0b, dx0 = _wide(B, H, W, C, dtype, 0.0, 0, lpad)
    gr = g.to(ref_dt).cpu()
    base = torch.nn.grad.conv2d_input((B, C, H, W), wr, gr, s, pad, 1, C)
    before = dx.to(ref_dt).cpu().clone()
    kn = _call("dy_dwconv_dgrad", g.data_ptr(), ops.ld_of(g), dx0.data_ptr(), ops.ld_of(dx0), w.data_ptr(), B, H, W, C, k, s, 0, None, 0, did)
    assert kn.startswith("dwconv_kernel<dgrad"), kn
    torch.cuda.synchronize()
    _check(dx0, base, dtype, f"dgrad {tag}")
    _call("dy_dwconv_dgrad", g.data_ptr(), ops.ld_of(g), dx.data_ptr(), ops.ld_of(dx), w.data_ptr(), B, H, W, C, k, s, 1,
          sv.data_ptr(), ops.ld_of(sv), did)
    torch.cuda.synchronize()
    _check(dx, before + base + sv.to(ref_dt).cpu(), dtype, f"dgrad accumulate+add_src {tag}")
    for b_ in (gb, sb, db, d0b):
        assert _sentinels_intact(b_, C)

    # weight gradient: f32, two runs bit-identical
    scratch = torch.empty(1 << 20, dtype=torch.float32, device="cuda")
    dws = [torch.full((C, 1, k, k), float("nan"), device="cuda") for _ in range(2)]
    for dw in dws:
        kn = _call("dy_dwconv_wgrad", x.data_ptr(), ops.ld_of(x), g.data_ptr(), ops.ld_of(g), dw.data_ptr(), B, H, W, C, k, s,
                   scratch.data_ptr(), scratch.numel(), did)
        assert kn.startswith("dwconv_wgrad_kernel"), kn
    torch.cuda.synchronize()
    want = torch.nn.grad.conv2d_weight(xr, (C, 1, k, k), gr, s, pad, 1, C)
    t = 2e-5 if dtype == torch.float32 else 1e-4
    err = float((dws[0].double().cpu() - want.double()).abs().max())
    print(f"wgrad {tag}: max abs err {err:.3e} (ref max {float(want.abs().max()):.3e})")
    assert err <= t * (float(want.abs().max()) + 1.0), f"wgrad {tag}: {err:.3e}"
    assert torch.equal(dws[0], dws[1]), "weight gradient must be bit-identical run to run"
    assert _sentinels_intact(xb, C) and _sentinels_intact(gb, C)


@pytest.mark.parametrize("lpad", LPADS, ids=["unaligned", "aligned"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("k,s", KS, ids=[f"k{k}s{s}" for k, s in KS])
@pytest.mark.parametrize("C", CS)
def test_dwconv_kernels_vs_torch(C, k, s, dtype, lpad):
    for B, H, W in _shapes(C):
        _kernel_case(C, k, s, dtype, lpad, B, H, W)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_dwconv_k7_generic_window(dtype):
    _kernel_case(12, 7, 1, dtype, 8, 2, 7, 9)
    _kernel_case(32, 7, 2, dtype, 8, 2, 7, 9)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("C,lpad", [(3, 3), (20, 8), (32, 8)])
def test_dwconv_constant_inputs_count_the_taps(C, lpad, dtype):
    """all-ones input and weights at k = 5, s = 2: every output is the number of taps inside the image at its border position,
    an integer <= 25 that every dtype holds exactly; the same for the data gradient of an all-ones dz"""
    from dedark_yolo_amd import ops
    did, k, s, B, H, W = ops.dt_id(dtype), 5, 2, 1, 7, 9
    Ho, Wo = (H + 4 - k) // s + 1, (W + 4 - k) // s + 1
    w = torch.ones((C, 1, k, k), device="cuda")
    xb, x = _wide(B, H, W, C, dtype, 1.0, 0, lpad)
    yb, y = _wide(B, Ho, Wo, C, dtype, 0.0, 0, lpad)
    _call("dy_dwconv_fwd", x.data_ptr(), ops.ld_of(x), y.data_ptr(), ops.ld_of(y), w.data_ptr(), B, H, W, C, k, s, None, None, 0, None, 0, did)
    gb, g = _wide(B, Ho, Wo, C, dtype, 1.0, 0, lpad)
    db, dx = _wide(B, H, W, C, dtype, 0.0, 0, lpad)
    _call("dy_dwconv_dgrad", g.data_ptr(), ops.ld_of(g), dx.data_ptr(), ops.ld_of(dx), w.data_ptr(), B, H, W, C, k, s, 0, None, 0, did)
    torch.cuda.synchronize()
    ones = torch.ones((B, C, H, W), dtype=torch.float64)
    wd = torch.ones((C, 1, k, k), dtype=torch.float64)
    assert torch.equal(y.double().cpu(), F.conv2d(ones, wd, None, s, 2, 1, C))
    assert torch.equal(dx.double().cpu(), torch.nn.grad.conv2d_input((B, C, H, W), wd, torch.ones((B, C, Ho, Wo), dtype=torch.float64), s, 2, 1, C))
    assert all(_sentinels_intact(b_, C) for b_ in (xb, yb, gb, db))


def test_dwconv_wgrad_many_blocks_is_deterministic_and_exact():
    """a map big enough for many partial blocks, and a scratch that caps their number"""
    from dedark_yolo_amd import ops
    C, B, H, W, k = 24, 4, 65, 63, 5
    xb, x = _wide(B, H, W, C, torch.float32, None, 5, 8)
    gb, g = _wide(B, H, W, C, torch.float32, None, 6, 8)
    want = torch.nn.grad.conv2d_weight(x.double().cpu(), (C, 1, k, k), g.double().cpu(), 1, 2, 1, C)
    outs = []
    for elems in (1 << 20, C * k * k * 3):
        scratch = torch.empty(elems, dtype=torch.float32, device="cuda")
        for _ in range(2):
            dw = torch.empty((C, 1, k, k), device="cuda")
            _call("dy_dwconv_wgrad", x.data_ptr(), ops.ld_of(x), g.data_ptr(), ops.ld_of(g), dw.data_ptr(), B, H, W, C, k, 1,
                  scratch.data_ptr(), scratch.numel(), 0)
            outs.append(dw)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3])
    for o in (outs[0], outs[2]):
        assert float((o.double().cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [1, 4, 12, 13])
def test_copy2d_exact_touches_only_its_lanes(C, dtype):
    from dedark_yolo_amd import ops
    sb, s = _wide(2, 5, 7, C, dtype, None, 40 + C, 3)
    db, d = _wide(2, 5, 7, C, dtype, None, 50 + C, 3)
    before = d.float().clone()
    assert _call("dy_copy2d_exact", s.data_ptr(), ops.ld_of(s), d.data_ptr(), ops.ld_of(d), 2 * 5 * 7, C, 1, ops.dt_id(dtype)) == "copy2d_exact_kernel"
    torch.cuda.synchronize()
    _check(d, before + s.float(), dtype, "copy accumulate")
    _call("dy_copy2d_exact", s.data_ptr(), ops.ld_of(s), d.data_ptr(), ops.ld_of(d), 2 * 5 * 7, C, 0, ops.dt_id(dtype))
    torch.cuda.synchronize()
    assert torch.equal(d, s) and _sentinels_intact(sb, C) and _sentinels_intact(db, C)


def test_dwconv_rejects_bad_arguments():
    from dedark_yolo_amd import _C, ops
    x = torch.zeros((1, 8, 8, 16), device="cuda")
    y = torch.zeros((1, 8, 8, 16), device="cuda")
    w = torch.zeros((16, 1, 4, 4), device="cuda")
    st = torch.zeros(64 * 2 * 16, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="k=4"):
        _C.call("dy_dwconv_fwd", x.data_ptr(), 16, y.data_ptr(), 16, w.data_ptr(), 1, 8, 8, 16, 4, 1, None, None, 0, None, 0, 0, ops.stream())
    with pytest.raises(RuntimeError, match="stride=3"):
        _C.call("dy_dwconv_fwd", x.data_ptr(), 16, y.data_ptr(), 16, w.data_ptr(), 1, 8, 8, 16, 3, 3, None, None, 0, None, 0, 0, ops.stream())
    with pytest.raises(RuntimeError, match="statistics mode"):          # the two forward modes exclude each other
        _C.call("dy_dwconv_fwd", x.data_ptr(), 16, y.data_ptr(), 16, w.data_ptr(), 1, 8, 8, 16, 3, 1, None, None, 1, st.data_ptr(), 16, 0, ops.stream())
    with pytest.raises(RuntimeError, match="bad dtype"):
        _C.call("dy_dwconv_dgrad", x.data_ptr(), 16, y.data_ptr(), 16, w.data_ptr(), 1, 8, 8, 16, 3, 1, 0, None, 0, 7, ops.stream())
    # source and destination lanes that overlap inside one buffer (in place, or halves cut 4 lanes too close) are refused; sibling
    # halves are not
    w3 = torch.zeros((8, 1, 3, 3), device="cuda")
    a, b_, c = x[..., :8], x[..., 4:12], x[..., 8:]
    for dst in (a, b_):
        with pytest.raises(RuntimeError, match="overlap"):
            _C.call("dy_dwconv_fwd", a.data_ptr(), 16, dst.data_ptr(), 16, w3.data_ptr(), 1, 8, 8, 8, 3, 1, None, None, 0, None, 0, 0, ops.stream())
        with pytest.raises(RuntimeError, match="overlap"):
            _C.call("dy_dwconv_dgrad", dst.data_ptr(), 16, a.data_ptr(), 16, w3.data_ptr(), 1, 8, 8, 8, 3, 1, 0, None, 0, 0, ops.stream())
    _C.call("dy_dwconv_fwd", a.data_ptr(), 16, c.data_ptr(), 16, w3.data_ptr(), 1, 8, 8, 8, 3, 1, None, None, 0, None, 0, 0, ops.stream())
    _C.call("dy_dwconv_dgrad", c.data_ptr(), 16, a.data_ptr(), 16, w3.data_ptr(), 1, 8, 8, 8, 3, 1, 0, None, 0, 0, ops.stream())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ modules
@pytest.mark.parametrize("name", sorted(ghost_ref.BLOCKS))
def test_ghost_blocks_golden(name):
    """outputs, dx, every parameter gradient and the BatchNorm running statistics after the step, in fp32, within the project's block
    bound (test_gpu_parity._run_block: 1e-4 on outputs, 2e-3 on gradients, as for the g14_fasterc2f_* fixtures)"""
    from test_gpu_parity import _run_block
    from dedark_yolo_amd.nn import modules
    cls, args, _ = ghost_ref.BLOCKS[name]
    _run_block("g25_ghost_" + name, getattr(modules, cls)(*args))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", ["ghostconv_h4_noact", "ghostconv_s2_h12", "gbottleneck_16", "c3ghost_32"])
def test_ghost_blocks_low_precision_match_the_statement(name, dtype):
    """16-bit train-mode forward and backward of the blocks whose halves are 4 / 12 channels wide (8-byte aligned slices in 16-bit, staged
    through copy_exact) against the f64 statement on the same weights: 16-bit bounds of the kernel tests, scaled by the largest value"""
    import dedark_yolo_amd as dy
    from oracle import model as om
    from parity_helpers import load_sd, set_bn
    from dedark_yolo_amd.nn import modules
    g = gold("g25_ghost_" + name)
    cls, args, fn = ghost_ref.BLOCKS[name]
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
    yt = fn(sd64, xt)
    (yt * wgt.double()).sum().backward()
    # several 16-bit roundings in a row (each conv output, activation and gradient is stored in 16 bits): 4x the single-kernel bound
    t = 4 * _tol(dtype)
    for got, want, what in ((y, yt.detach(), "y"), (x.grad, xt.grad, "dx")):
        err = float((got.double().cpu() - want).abs().max())
        print(f"{name} {dtype} {what}: {err:.3e} (ref max {float(want.abs().max()):.3e})")
        assert torch.isfinite(got).all() and err <= t * (float(want.abs().max()) + 1.0), (what, err)
    named = dict(m.named_parameters())
    gtop = max(float(v.grad.abs().max()) for v in sd64.values() if getattr(v, "grad", None) is not None)
    for k, v in sd64.items():
        if getattr(v, "grad", None) is not None:
            err = float((named[k].grad.double().cpu() - v.grad).abs().max())
            assert err <= t * (gtop + 1.0), (k, err, gtop)


@pytest.mark.parametrize("name", ["gbottleneck_16", "gbottleneck_s2", "c3_32", "c3ghost_32"])
def test_ghost_blocks_skip_the_input_gradient_when_it_is_not_needed(name):
    """an input that needs no gradient (the block as first layer): `needs` reaches the first convs, and every parameter gradient is,
    bit for bit, the one of the run that also computed dx"""
    import dedark_yolo_amd as dy
    from oracle import model as om
    from parity_helpers import load_sd, set_bn
    from dedark_yolo_amd.nn import modules
    g = gold("g25_ghost_" + name)
    cls, args, _ = ghost_ref.BLOCKS[name]
    dy.set_compute_dtype(torch.float32)
    grads = []
    for need in (True, False):
        m = getattr(modules, cls)(*args)
        sd = om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"]))
        load_sd(set_bn(m), sd)
        m = m.cuda().train()
        x = g["x0"].clone().cuda().requires_grad_(need)
        y = m(x)
        (y.float() * rnd(900, *y.shape, lo=-1, hi=1).cuda()).sum().backward()
        torch.cuda.synchronize()
        assert (x.grad is not None) == need
        grads.append({k: p.grad.clone() for k, p in m.named_parameters()})
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in grads[0])


@pytest.mark.parametrize("fused", [False, True], ids=["eval", "eval_fused"])
@pytest.mark.parametrize("name", ["gbottleneck_s2", "c3ghost_32", "ghostconv_h4_noact"])
def test_ghost_block_eval_matches_the_statement(name, fused):
    """eval / no_grad path (BatchNorm folded into the conv and depthwise epilogues) against the f64 statement with running statistics,
    also after fuse() has cached the folded affines"""
    from oracle import model as om
    from parity_helpers import load_sd, set_bn
    from dedark_yolo_amd.nn import modules
    g = gold("g25_ghost_" + name)
    cls, args, fn = ghost_ref.BLOCKS[name]
    m = getattr(modules, cls)(*args)
    sd = om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"]))
    load_sd(set_bn(m), sd)
    m = m.cuda().eval()
    if fused:
        from dedark_yolo_amd.nn.tasks import BaseModel
        holder = BaseModel()
        holder.model = torch.nn.Sequential(m)
        holder.fuse(verbose=False)
        assert holder.is_fused()
    with torch.no_grad():
        y = m(g["x0"].cuda())
        want = fn({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, g["x0"].double(), False)
    close(y.double().cpu(), want, 1e-4, 1e-4, f"{name} eval")


# ------------------------------------------------------------------------------------------------ models
def _ghost_cfg(scale, lowlight_front):
    """yolov8-ghost.yaml, optionally with lowlight_recovery as layer 0 (every absolute `from` shifted by one: the graph of
    tests/golden/make_ghost_golden.py::ghost_dict)"""
    d = load_yaml("yolov8-ghost.yaml")
    d["scale"] = scale
    if lowlight_front:
        def sh(f):
            return f if f < 0 else f + 1
        nb = len(d["backbone"])
        rows = [[[sh(j) for j in f] if isinstance(f, list) else sh(f), n, m, a] for f, n, m, a in d["backbone"] + d["head"]]
        d["backbone"] = [[-1, 1, "lowlight_recovery", [3]]] + rows[:nb]
        d["head"] = rows[nb:]
    return d


def _ghost_model(lowlight_front, seed, nc=20):
    from oracle import model as om
    from parity_helpers import HYP, load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    model = DetectionModel(_ghost_cfg("n", lowlight_front), ch=3, nc=nc)
    model.args = HYP
    load_sd(model, om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed))
    return model.cuda()


def _model_step(name, dtype=torch.float32):
    import dedark_yolo_amd as dy
    g = gold(name)
    dy.set_compute_dtype(dtype)
    model = _ghost_model("_ll_" in name, int(g["seed"])).train()
    batch = make_batch(int(g["seed"]) + 1, int(g["B"]), int(g["S"]), [int(v) for v in g["nbox"]])
    batch["img"] = batch["img"].pow(3.0).cuda()
    batch["recovery_loss_batch"] = torch.tensor(0.0123).cuda()
    loss, items = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    return g, model, batch, loss, items


@pytest.mark.parametrize("name", ["g25_ghost_n_tiny", "g25_ghost_ll_tiny"])
def test_ghost_model_step_golden(name):
    """loss and items within 1e-4; selected gradients, running statistics and the eval output within the bounds
    test_gpu_faster.py uses for g14_faster_n_tiny; the fuse()d eval output equals the unfused one within the same fp32 bound"""
    g, model, batch, loss, items = _model_step(name)
    print(f"{name}: loss {float(loss):.6f} vs {float(g['loss']):.6f}")
    close(float(loss.detach()), g["loss"], 1e-4, 1e-4, f"{name} loss vs reference golden")
    close(items.float().cpu(), g["items"], 1e-4, 1e-4, f"{name} items vs reference golden")
    named = dict(model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in named.values() if p.requires_grad)
    gtol = 5e-3
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
    err = float((y[:, :, ::7].float().cpu() - g["y"]).abs().max()) / float(g["y"].abs().max())
    assert err <= 1e-4, err
    model.fuse()
    assert model.is_fused()
    with torch.no_grad():
        yf = model(batch["img"])
    yf = yf[0] if isinstance(yf, (list, tuple)) else yf
    assert float((yf.float() - y.float()).abs().max()) <= 1e-4 * float(y.abs().max())


def _grads(m):
    return torch.cat([p.grad.double().flatten() for p in m.parameters() if p.requires_grad])


def _cos(a, b):
    return float((a @ b) / (a.norm() * b.norm()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_ghost_model_low_precision(dtype):
    """16-bit runs of yolov8n-ghost at 64x64 (hidden widths down to 4 channels: the 8-byte aligned slices, through the whole stack):
    finite, loss within 2 % of the reference's fp32 golden, and the gradient as close in direction to the fp32 path's as the fp32
    kernels with 16-bit STORAGE get (ops.set_storage_emulation; the bounds of test_gpu_faster.py::test_faster_model_low_precision)"""
    from dedark_yolo_amd import ops
    g, m16, _, loss, items = _model_step("g25_ghost_n_tiny", dtype)
    assert torch.isfinite(loss) and bool(torch.isfinite(items).all())
    assert abs(float(loss) - float(g["loss"])) <= 2e-2 * abs(float(g["loss"])), (float(loss), float(g["loss"]))
    a = _grads(m16)
    assert bool(torch.isfinite(a).all())
    _, m32, _, _, _ = _model_step("g25_ghost_n_tiny", torch.float32)
    ops.set_storage_emulation(dtype)
    try:
        _, memu, _, _, _ = _model_step("g25_ghost_n_tiny", torch.float32)
    finally:
        ops.set_storage_emulation(None)
    b, e = _grads(m32), _grads(memu)
    cos, cos_emu = _cos(a, b), _cos(e, b)
    print(f"{dtype}: gradient cosine vs fp32 {cos:.4f}, 16-bit storage emulation {cos_emu:.4f}")
    assert cos >= min(cos_emu, 0.95) - 0.03, (cos, cos_emu)


def test_product_eval_equals_the_reference_running_our_ghost_checkpoint():
    """the reference loaded a last.pt written by this package (tests/golden/make_ghost_golden.py interop) and its eval output is the
    product's on the same half-rounded weights"""
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    g = gold("g25_ghost_interop")
    model = DetectionModel(_ghost_cfg("n", False), nc=20)
    ema = om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, 2522)
    load_sd(model, {k: (v.half().float() if v.is_floating_point() else v) for k, v in ema.items()})
    model = model.cuda().eval()
    model.fuse()
    x = rnd(int(g["n_x_seed"]), 2, 3, 64, 64).pow(2.0)
    with torch.no_grad():
        y = model(x.cuda())
    y = y[0] if isinstance(y, (list, tuple)) else y
    want = g["n_y"]
    err = float((y.float().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)
    assert y.shape == want.shape and err <= 1e-4, err


def _trainer_run(tmp, tag):
    import bench
    import dedark_yolo_amd as dy
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    from dedark_yolo_amd.nn.tasks import DetectionModel
    dy.set_compute_dtype(torch.float32)
    torch.manual_seed(3)
    tr = DetectionTrainer(get_cfg(dict(model="tiny", dtype="fp32", optimizer="SGD", batch=64, lowlight_FLAG=False, dedark_FLAG=False)))
    tr.setup(DetectionModel(_ghost_cfg("n", False), nc=20))
    assert all(getattr(p, "_dy_direct", False) for p in tr.model.parameters() if p.requires_grad)      # gradients land in the flat buffer
    b = bench.synth_batch(80, 4, 64, 20, "cuda")
    tr.args.dark_param = b.pop("gamma")
    b.pop("n_max", None)
    loss, _ = tr.train_step(b, [0.01] * 3, 0.9)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and bool(torch.isfinite(tr.flat.p).all()) and bool(torch.isfinite(tr.flat.g).all())
    last = tr.save_model(str(tmp / tag), epoch=0, fitness=0.1)
    return tr, last


def test_trainer_step_checkpoint_and_determinism_on_the_ghost_model(tmp_path):
    """One trainer step of yolov8n-ghost with direct gradient placement, last.pt in the reference's format; a model built from the file
    gives, bit for bit, the eval output of the trained weights at the file's half precision; a second identical run gives identical
    parameter bytes (the depthwise weight gradient is deterministic end to end)."""
    from dedark_yolo_amd.nn.tasks import DetectionModel
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint
    tr, last = _trainer_run(tmp_path, "a")
    ck = load_checkpoint(last)
    assert ck.source == "reference-pickle" and (tmp_path / "a" / "best.pt").exists()
    assert list(ck.model_sd) == list(tr.model.state_dict())
    x = rnd(91, 2, 3, 64, 64).pow(2.0).cuda()

    def eval_of(sd):
        m = DetectionModel(_ghost_cfg("n", False), nc=20)
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        with torch.no_grad():
            y = m(x)
        return (y[0] if isinstance(y, (list, tuple)) else y).clone()
    trained = {k: (v.detach().cpu().half().float() if v.is_floating_point() else v.detach().cpu()) for k, v in tr.model.state_dict().items()}
    y_file, y_mem = eval_of(ck.model_sd), eval_of(trained)
    assert bool(torch.isfinite(y_file).all()) and torch.equal(y_file, y_mem)
    assert torch.equal(eval_of(ck.model_sd), y_file)
    p1 = tr.flat.p.clone()
    tr2, _ = _trainer_run(tmp_path, "b")
    assert torch.equal(p1, tr2.flat.p), "two identical runs must give identical parameter bytes"
