"""Training-mode BatchNorm as the product runs it, against plain fp64 references.

The chain is: conv kernel (raw z + per-channel sums of z and z^2 in DY_STATS_REPLICAS f64 replicas) -> dy_bn_finalize (scale,
shift, mean, invstd; running buffers) -> dy_bn_act_fwd (affine + activation + residual); backward dy_bn_act_bwd (reduce + apply).
Reference: nn.BatchNorm2d of the reference repo (eps 1e-3, momentum 0.03, ultralytics/utils/torch_utils.py:263-265) after
F.conv2d, in float64 on the dtype-rounded operands.

(a) the statistics epilogue of every forward route that can take `stats`, (b) the whole chain through ops.conv_forward /
ops.conv_backward over two steps, (c) padded channels (Cout not a multiple of the vector width) must not touch anything past
the layer's per-channel parameters and buffers, (d) dy_bn_finalize on its own."""
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from util import gold, make_batch

pytestmark = pytest.mark.gpu

MOM, EPS = 0.03, 1e-3
BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.fixture(autouse=True)
def _fp32_after():
    import dedark_yolo_amd as dy
    yield
    dy.set_compute_dtype(torch.float32)


def _act(u, act):
    return u * torch.sigmoid(u) if act == 1 else (F.leaky_relu(u, 0.1) if act == 2 else u)


# ---------------------------------------------------------------------------------------------------- (a) statistics epilogue
# Every kernel dy_conv2d_fwd (csrc/conv.hip) can launch with `stats` set, in dispatch order.  Not reachable with statistics:
# the dense kernel (dy_dense_fwd_eligible excludes stats), v3::conv3x3_kernel<64, 0> (dy_conv_v3_eligible needs Cd > 64, and
# the launch picks the 64-wide tile only for Cd <= 64), the parity-class launches (data gradient only) and the tile shapes
# that only DY_V2_EXP / DY_V2_SMALLC select (diagnostics builds).
STATS_ROUTES = {
    "stem_fwd_kernel", "px1x1_kernel", "v4::conv_kernel", "v5::band_kernel<128>", "v5::band_kernel<64>", "v5::conv_kernel<128>",
    "v5::conv_kernel<64>", "v3::conv3x3_kernel<128, 0>", "v2::conv_kernel<256, 256, 0, false, 2>",
    "v2::conv_kernel<128, 128, 0, false, 2>", "v2::conv_kernel<256, 64, 0, false, 2>", "v2::conv_kernel<128, 128, 0, true, 2>",
    "v2::conv_kernel<256, 64, 0, true, 2>", "conv_thin_kernel", "conv_igemm_kernel<BN=32>", "conv_igemm_kernel<BN=64>",
    "conv_igemm_kernel<BN=128>"}

# (route, dtype, B, Cin, Cout, H, W, k, stride, pad, dil, offset).  Cout is mostly not a multiple of 8 (pad channels in z and in
# the replicas) and pixel counts are not multiples of the tiles.  offset (1x1 windows, so no border pixel sees fewer taps):
# x ~ N(mu, 1) and weights whose mean equals their spread, so |mean| / sigma = mu * sqrt(K / 2) = 15 (the sum of squares is
# then 226x the variance).
STATS_CASES = [
    ("stem_fwd_kernel", BF, 2, 3, 14, 64, 96, 3, 2, 1, 1, False),
    ("stem_fwd_kernel", FP, 3, 3, 30, 33, 47, 3, 2, 1, 1, False),
    ("px1x1_kernel", BF, 7, 128, 126, 197, 191, 1, 1, 0, 1, False),              # 263,389 pixels
    ("px1x1_kernel", FP, 7, 64, 58, 197, 191, 1, 1, 0, 1, False),
    ("v4::conv_kernel", BF, 31, 192, 230, 41, 43, 3, 1, 1, 1, False),            # ragged pixels and channels (232 of a 256 tile)
    ("v4::conv_kernel", BF, 13, 512, 250, 64, 64, 1, 1, 0, 1, True),
    ("v5::band_kernel<128>", BF, 17, 128, 118, 63, 61, 3, 1, 1, 1, False),
    ("v5::band_kernel<64>", FP, 120, 64, 62, 33, 17, 3, 1, 1, 1, False),
    ("v5::band_kernel<64>", BF, 120, 64, 50, 33, 17, 3, 1, 1, 1, False),      # Cd = 56
    ("v5::conv_kernel<128>", BF, 4, 64, 126, 255, 257, 3, 2, 1, 1, False),
    ("v5::conv_kernel<64>", BF, 8, 64, 60, 96, 90, 1, 1, 0, 1, False),
    ("v5::conv_kernel<64>", FP, 8, 64, 60, 96, 90, 1, 1, 0, 1, True),
    ("v3::conv3x3_kernel<128, 0>", BF, 2, 64, 126, 40, 40, 3, 1, 1, 1, False),
    ("v3::conv3x3_kernel<128, 0>", FP, 3, 64, 78, 33, 35, 3, 1, 1, 1, False),    # Cd = 80 of a 128 tile
    ("v2::conv_kernel<256, 256, 0, false, 2>", BF, 2, 64, 250, 160, 160, 7, 1, 3, 1, False),   # 7x7: too many taps for v4 / v5
    ("v2::conv_kernel<128, 128, 0, false, 2>", BF, 2, 64, 126, 40, 50, 1, 1, 0, 1, True),
    ("v2::conv_kernel<256, 64, 0, false, 2>", FP, 3, 128, 62, 61, 63, 3, 2, 1, 1, False),
    ("v2::conv_kernel<128, 128, 0, true, 2>", BF, 2, 32, 120, 40, 40, 3, 1, 1, 1, False),
    ("v2::conv_kernel<256, 64, 0, true, 2>", BF, 2, 24, 62, 37, 41, 3, 1, 1, 1, False),
    ("conv_thin_kernel", BF, 4, 16, 20, 40, 40, 3, 1, 1, 1, False),
    ("conv_thin_kernel", BF, 4, 16, 30, 33, 35, 3, 2, 1, 1, False),
    ("conv_igemm_kernel<BN=32>", F32, 2, 16, 18, 9, 7, 3, 1, 1, 1, False),
    ("conv_igemm_kernel<BN=32>", BF, 1, 8, 22, 20, 20, 3, 1, 1, 1, False),
    ("conv_igemm_kernel<BN=64>", BF, 1, 32, 62, 20, 20, 3, 1, 1, 1, False),
    ("conv_igemm_kernel<BN=64>", F32, 2, 24, 42, 13, 11, 3, 2, 1, 1, False),
    ("conv_igemm_kernel<BN=128>", F32, 2, 64, 126, 12, 13, 3, 1, 1, 1, False),
    ("conv_igemm_kernel<BN=128>", F32, 2, 64, 126, 12, 13, 1, 1, 0, 1, True),
    ("conv_igemm_kernel<BN=128>", F32, 1, 32, 250, 19, 17, 3, 1, 2, 2, False),   # dilated, two channel tiles
]


def _case_id(c):
    return f"{c[0]}-{str(c[1])[6:]}-" + "x".join(map(str, c[2:11])) + ("-offset" if c[11] else "")


@pytest.mark.parametrize("case", STATS_CASES, ids=[_case_id(c) for c in STATS_CASES])
def test_stats_epilogue_per_route(case):
    """Sum z and sum z^2 over the replicas against fp64 sums of F.conv2d (float64) on the rounded operands, per channel:
    bound 2e-6 of sum|z| and of sum z^2.  The kernels add f32 partial sums of a tile into f64; measured at most 1.2e-7 (f32
    igemm, 2e-8 on the MFMA tile kernels).  One pixel dropped or counted twice moves a sum by about 1 / M of it: 4e-6 at the
    largest M here (263,389), so the bound catches it on every case.  Mean against fp64 within 2e-5 sigma + 1e-6 |mean|;
    biased variance (s2 / n - mean^2) within 2e-6 of itself (measured <= 2.1e-7), 5e-4 for the offset cases, where s2 is
    226x the variance and the sum-of-squares error is magnified that much (measured <= 5.8e-5).  Replicas of the pad channels
    are exactly 0."""
    from dedark_yolo_amd import _C, ops
    from dedark_yolo_amd.ops import stream
    route, dtype, B, Cin, Cout, H, W, k, s, p, dil, offset = case
    torch.manual_seed(B * 7919 + Cin * 31 + Cout + H)
    K = Cin * k * k
    if offset:
        x = torch.randn(B, Cin, H, W, device="cuda") + 15.0 * (2.0 / K) ** 0.5
        w = (torch.randn(Cout, Cin, k, k, device="cuda") + 1.0) / K ** 0.5
    else:
        x = torch.randn(B, Cin, H, W, device="cuda")
        w = torch.randn(Cout, Cin, k, k, device="cuda") / K ** 0.5
    xn = ops.as_nhwc(x, dtype)
    cin_pad, cout_pad = ops.padded_channels(xn), ops.round_up(Cout, ops.vec_elems(dtype))
    wp = ops._pack(w, cout_pad, cin_pad, False, dtype)
    Ho, Wo = (H + 2 * p - dil * (k - 1) - 1) // s + 1, (W + 2 * p - dil * (k - 1) - 1) // s + 1
    z = ops.empty_nhwc(B, cout_pad, Ho, Wo, dtype, x.device)
    R = _C.STATS_REPLICAS
    stats = torch.zeros(R * 2 * cout_pad, dtype=torch.float64, device="cuda")
    d = ops._conv_desc(xn, wp, z, B, H, W, cin_pad, Ho, Wo, cout_pad, k, k, s, p, dil, None, None, 0, stats, False, dtype)
    _C.lib().dy_clear_last_kernel()
    _C.call("dy_conv2d_fwd", C.byref(d), stream())
    torch.cuda.synchronize()
    got = _C.lib().dy_last_kernel().decode()
    assert got == route, (got, route)
    ref = F.conv2d(x.to(dtype).double(), w.to(dtype).double(), None, s, p, dil)
    n = ref.numel() // Cout
    rep = stats.view(R, 2, cout_pad)
    assert bool((rep[:, :, Cout:] == 0).all()), "pad-channel replicas are not 0"
    t = rep.sum(0)[:, :Cout]
    s1, s2, sa = ref.sum((0, 2, 3)), (ref * ref).sum((0, 2, 3)), ref.abs().sum((0, 2, 3))
    e1, e2 = float(((t[0] - s1).abs() / sa).max()), float(((t[1] - s2).abs() / s2).max())
    mr, vr = ref.mean((0, 2, 3)), ref.var((0, 2, 3), unbiased=False)
    m, v = t[0] / n, t[1] / n - (t[0] / n) ** 2
    em = float(((m - mr).abs() / (2e-5 * vr.sqrt() + 1e-6 * mr.abs())).max())
    ev = float(((v - vr).abs() / vr).max())
    ratio = float((mr.abs() / vr.sqrt()).median())
    print(f"{_case_id(case)}: sum {e1:.2e}, sum sq {e2:.2e}, mean {em:.2f} of bound, var {ev:.2e}, median |mean|/sigma {ratio:.1f}")
    assert e1 <= 2e-6 and e2 <= 2e-6, (e1, e2)
    assert em <= 1.0, em
    assert ev <= (5e-4 if offset else 2e-6), ev
    if offset:
        assert 10.0 <= ratio <= 20.0, ratio


def test_stats_routes_all_covered():
    """Each case above asserts the kernel dy_conv2d_fwd reported; together they must name every statistics route."""
    assert {c[0] for c in STATS_CASES} == STATS_ROUTES


# ------------------------------------------------------------------------------------------- (b) the whole chain, two steps
class _Tape:
    def __init__(self):
        self.stack, self.pgrads = [], {}

    def push(self, c):
        self.stack.append(c)

    def pop(self):
        return self.stack.pop()


def _make_bn(Cout, seed):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(Cout, eps=EPS, momentum=MOM)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.3 * torch.randn(Cout, generator=g))
        bn.bias.copy_(0.2 * torch.randn(Cout, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(Cout, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(Cout, generator=g))
    return bn.cuda()


class _Ref:
    """fp64 autograd twin of conv -> BatchNorm2d(train) -> act -> + residual; running buffers updated by F.batch_norm.

    The product keeps z in the compute dtype and normalises that stored z with statistics of the unrounded f32 accumulators.
    The twin does the same: batch mean / variance (and the running update) from z, the normalised value from z rounded to the
    dtype, passed straight through in the backward.  Without it LeakyReLU's kink turns a rounding of z into an O(1) error of
    act'(u) wherever the two u straddle 0 (bf16: dx off by 7 % of its max)."""

    def __init__(self, w, bn, dtype):
        self.w = w.detach().to(dtype).double()                  # the kernels see the weights rounded to the compute dtype
        self.g, self.b = bn.weight.detach().double(), bn.bias.detach().double()
        self.rm, self.rv = bn.running_mean.detach().double().clone(), bn.running_var.detach().double().clone()

    def step(self, x, res, gy, s, p, act, dtype):
        xd = x.to(dtype).double().requires_grad_(True)
        w, g, b = (t.clone().requires_grad_(True) for t in (self.w, self.g, self.b))
        z = F.conv2d(xd, w, None, s, p)
        F.batch_norm(z.detach(), self.rm, self.rv, None, None, training=True, momentum=MOM, eps=EPS)
        zq = z + (z.detach().to(dtype).double() - z.detach())
        mu, var = z.mean((0, 2, 3), keepdim=True), z.var((0, 2, 3), unbiased=False, keepdim=True)
        u = (zq - mu) * (var + EPS).rsqrt() * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
        y = _act(u, act)
        if res is not None:
            y = y + res.to(dtype).double()
        y.backward(gy.to(dtype).double())
        return dict(y=y.detach(), dx=xd.grad, dw=w.grad, dg=g.grad, db=b.grad, z=z.detach())


def _full(v, C):
    """The cout_pad-wide NHWC tensor behind a [B, Cout, H, W] view of it (pad lanes included)."""
    B, _, H, W = v.shape
    return v.as_strided((B, C, H, W), v.stride())


def _chain_step(x, w, bn, act, s, p, dtype, res, gy, out_full=None, off=0, capture=None):
    from dedark_yolo_amd import ops
    B = x.shape[0]
    Cout = w.shape[0]
    tape = _Tape()
    xn = ops.as_nhwc(x, dtype)
    out = out_full[:, off:off + Cout] if out_full is not None else None
    rn = ops.as_nhwc(res, dtype) if res is not None else None
    y = ops.conv_forward(tape, xn, w, None, bn, act, s, p, 1, True, out=out, residual=rn)
    aff = tape.stack[-1].aff.clone()
    made = []
    real_empty = ops.empty_nhwc

    def spy_empty(*a, **k):
        t = real_empty(*a, **k)
        made.append(t)
        return t
    ops.empty_nhwc = spy_empty
    try:
        dx = ops.conv_backward(tape, ops.as_nhwc(gy, dtype), need_dx=True)
    finally:
        ops.empty_nhwc = real_empty
    torch.cuda.synchronize()
    dz = made[0]                                       # conv_backward's first buffer is dz
    assert tuple(dz.shape) == (B, ops.round_up(Cout, ops.vec_elems(dtype))) + tuple(y.shape[2:])
    return dict(y=y, aff=aff, dx=dx, dw=tape.pgrads[w], dg=tape.pgrads[bn.weight], db=tape.pgrads[bn.bias], dz=dz)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


# (dtype, B, Cin, Cout, H, W, k, stride, pad, act, residual, concat).  Counts of 2 and 8 pixels per channel are P6 maps at B = 2;
# the last case writes 135.8 MB of z (past the 128 MiB threshold of the streaming variants of all three BN kernels).
CHAIN = [
    (F32, 2, 16, 18, 12, 10, 3, 1, 1, 1, False, False),
    (F32, 2, 16, 18, 12, 10, 3, 2, 1, 2, True, True),
    (F32, 2, 32, 18, 1, 1, 1, 1, 0, 0, True, False),
    (BF, 2, 32, 20, 16, 16, 3, 1, 1, 1, False, True),
    (BF, 2, 64, 62, 20, 20, 3, 1, 1, 2, True, False),
    (BF, 2, 64, 20, 2, 2, 3, 1, 1, 1, True, True),
    (BF, 2, 64, 62, 1, 1, 1, 1, 0, 0, False, False),
    (FP, 2, 32, 20, 15, 17, 3, 2, 1, 0, True, True),
    (FP, 2, 64, 62, 2, 2, 1, 1, 0, 1, False, False),
    (FP, 2, 48, 62, 24, 24, 3, 1, 1, 2, False, True),
    (FP, 2, 64, 20, 1, 1, 3, 1, 1, 2, True, False),
    (BF, 1, 16, 64, 1030, 1030, 1, 1, 0, 1, True, False),
]
# bounds relative to max|reference| of each tensor.  f32: exact-f32 MFMA conv and IEEE sigmoid, measured <= 4.3e-7 -> 1e-5.
# 16-bit: the twin rounds z like the product (_Ref); what remains is y and dz stored rounded (2^-9 bf16, 2^-11 f16 relative),
# the rounded gy both sides see, 16-bit operands of the data / weight gradient convs and the fast v_exp / v_rcp sigmoid
# (1e-6): measured <= 4.3e-3 bf16 and 4.5e-4 f16 -> 1e-2 and 2e-3.  Running buffers come from the f32 accumulators whatever the
# dtype: 1e-5 of |value| + sigma (measured <= 2.2e-7).
TOL = {F32: 1e-5, BF: 1e-2, FP: 2e-3}


def _chain_id(c):
    return f"{str(c[0])[6:]}-" + "x".join(map(str, c[1:9])) + f"-act{c[9]}" + ("-res" if c[10] else "") + ("-cat" if c[11] else "")


def _chain_inputs(case, seed):
    dtype, B, Cin, Cout, H, W, k, s, p, act, use_res, cat = case
    torch.manual_seed(seed)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = torch.randn(B, Cin, H, W, device="cuda")
    res = torch.randn(B, Cout, Ho, Wo, device="cuda") if use_res else None
    gy = torch.randn(B, Cout, Ho, Wo, device="cuda")
    return x, res, gy


@pytest.mark.parametrize("case", CHAIN, ids=[_chain_id(c) for c in CHAIN])
def test_conv_bn_act_chain_two_steps(case, monkeypatch):
    """ops.conv_forward / conv_backward with a real nn.BatchNorm2d over two consecutive steps against fp64 autograd: y, both
    running buffers, dx, dW, dgamma, dbeta after each step (bounds at TOL).  The weights are scaled so that the batch variance is
    near eps (1e-3), so eps and the biased / unbiased variance are both visible.  The merged entries must be the ones taken; the
    pad lanes of y and dz are exactly 0; a concat destination is written in its own channels only."""
    from dedark_yolo_amd import ops
    dtype, B, Cin, Cout, H, W, k, s, p, act, use_res, cat = case
    ops.set_compute_dtype(dtype)
    cout_pad = ops.round_up(Cout, ops.vec_elems(dtype))
    torch.manual_seed(Cout * 13 + H)
    w = (torch.randn(Cout, Cin, k, k, device="cuda") * (0.05 / (Cin * k * k) ** 0.5)).requires_grad_(True)
    bn = _make_bn(Cout, Cout + H)
    ref = _Ref(w, bn, dtype)
    names = []
    real_call = ops.call

    def spy(name, *a):
        names.append(name)
        return real_call(name, *a)
    monkeypatch.setattr(ops, "call", spy)
    tol = TOL[dtype]
    for step in range(2):
        x, res, gy = _chain_inputs(case, 100 * step + Cout)
        Ho, Wo = gy.shape[2], gy.shape[3]
        out_full, off = None, 8
        if cat:
            out_full = ops.empty_nhwc(B, cout_pad + 24, Ho, Wo, dtype, x.device)
            out_full.fill_(7.0)
        got = _chain_step(x, w, bn, act, s, p, dtype, res, gy, out_full, off)
        want = ref.step(x, res, gy, s, p, act, dtype)
        errs = {k_: _rel(got[k_], want[k_]) for k_ in ("y", "dx", "dw", "dg", "db")}
        sig = float(want["z"].var((0, 2, 3), unbiased=False).max()) ** 0.5
        e_rm = float(((bn.running_mean.double() - ref.rm).abs() / (ref.rm.abs() + sig)).max())
        e_rv = float(((bn.running_var.double() - ref.rv).abs() / ref.rv).max())
        print(f"{_chain_id(case)} step {step}: {errs}, running mean {e_rm:.2e}, running var {e_rv:.2e}")
        assert max(errs.values()) <= tol, errs
        assert e_rm <= 1e-5 and e_rv <= 1e-5, (e_rm, e_rv)
        yf = _full(got["y"], cout_pad)
        assert bool((yf[:, Cout:] == 0).all()), "pad lanes of y are not 0"
        assert bool((got["dz"][:, Cout:] == 0).all()), "pad lanes of dz are not 0"
        if cat:
            assert bool((out_full[:, :off] == 7.0).all()) and bool((out_full[:, off + cout_pad:] == 7.0).all())
    assert names.count("dy_conv2d_bn_act_fwd_valid") == 2 and names.count("dy_bn_act_bwd_valid") == 2, names
    assert not {"dy_bn_finalize_valid", "dy_bn_act_fwd", "dy_bn_act_bwd_apply_valid"} & set(names), names


@pytest.mark.parametrize("dtype,Cout", [(BF, 20), (FP, 62), (F32, 18)], ids=["bf16-20", "f16-62", "f32-18"])
def test_split_entries_bit_identical_to_merged(dtype, Cout):
    """The per-entry leg (profiling / storage emulation: dy_conv2d_fwd + dy_bn_finalize + dy_bn_act_fwd, reduce + apply) runs
    the same kernels as the merged entries: y, the affine buffer, dz and the gradients are bit-identical."""
    from dedark_yolo_amd import _C, ops
    ops.set_compute_dtype(dtype)
    case = (dtype, 2, 32, Cout, 15, 17, 3, 1, 1, 1, True, True)
    torch.manual_seed(Cout)
    w = (torch.randn(Cout, 32, 3, 3, device="cuda") * (0.05 / 288 ** 0.5)).requires_grad_(True)
    x, res, gy = _chain_inputs(case, 5)
    outs = []
    for split in (False, True):
        bn = _make_bn(Cout, 3)
        _C._prof = [] if split else None
        try:
            outs.append(_chain_step(x, w, bn, 1, 1, 1, dtype, res, gy))
        finally:
            _C._prof = None
        outs[-1]["rm"], outs[-1]["rv"] = bn.running_mean.clone(), bn.running_var.clone()
    a, b = outs
    for k_ in ("y", "aff", "dz", "dx", "dw", "dg", "db", "rm", "rv"):
        assert torch.equal(a[k_], b[k_]), k_


# --------------------------------------------------------------------------------------- (c) padded-channel containment
def _flat_bn(Cout, sentinel, seed):
    """A BatchNorm2d whose gamma, beta and running buffers are slices of two flat tensors, back to back as in FlatState
    (engine/trainer.py), each followed by a block of 16 sentinel floats."""
    bn = _make_bn(Cout, seed)
    pf = torch.full((2 * Cout + 16,), sentinel, device="cuda")
    bf = torch.full((2 * Cout + 16,), sentinel, device="cuda")
    pf[:Cout], pf[Cout:2 * Cout] = bn.weight.detach(), bn.bias.detach()
    bf[:Cout], bf[Cout:2 * Cout] = bn.running_mean, bn.running_var
    bn.weight.data, bn.bias.data = pf[:Cout], pf[Cout:2 * Cout]
    bn.running_mean.data, bn.running_var.data = bf[:Cout], bf[Cout:2 * Cout]
    return bn, pf, bf


def _bits(t):
    return t.view(torch.int32).clone()


@pytest.mark.parametrize("sentinel", [-2.5, float("nan")], ids=["negative", "nan"])
@pytest.mark.parametrize("dtype,Cout", [(BF, 20), (FP, 62), (F32, 18)], ids=["bf16-20", "f16-62", "f32-18"])
def test_padded_channels_stay_inside_the_layer(dtype, Cout, sentinel):
    """Cout not a multiple of the vector width: the views are cout_pad wide, gamma / beta / running buffers Cout long.  Training
    (merged forward + backward) and eval (bn_fold + conv epilogue): the sentinels after the parameters and buffers are
    bit-unchanged; running_var[0:pad], which is where running_mean's overrun would land, matches fp64; the pad lanes of y and dz
    are exactly 0; a following 1x1 conv over y is finite."""
    from dedark_yolo_amd import ops
    ops.set_compute_dtype(dtype)
    cout_pad = ops.round_up(Cout, ops.vec_elems(dtype))
    pad = cout_pad - Cout
    assert pad > 0
    case = (dtype, 2, 32, Cout, 15, 17, 3, 1, 1, 1, False, False)
    torch.manual_seed(Cout + 1)
    w = (torch.randn(Cout, 32, 3, 3, device="cuda") * (0.05 / 288 ** 0.5)).requires_grad_(True)
    w2 = torch.randn(8, Cout, 1, 1, device="cuda")
    bn, pf, bf = _flat_bn(Cout, sentinel, 11)
    ref = _Ref(w, bn, dtype)
    p0, b0 = _bits(pf[2 * Cout:]), _bits(bf[2 * Cout:])
    for step in range(2):
        x, _, gy = _chain_inputs(case, 7 + step)
        got = _chain_step(x, w, bn, 1, 1, 1, dtype, None, gy)
        ref.step(x, None, gy, 1, 1, 1, dtype)
        assert torch.equal(_bits(pf[2 * Cout:]), p0) and torch.equal(_bits(bf[2 * Cout:]), b0), "sentinel overwritten (training)"
        assert torch.allclose(bn.running_var[:pad].double(), ref.rv[:pad], rtol=1e-5, atol=0), (bn.running_var[:pad], ref.rv[:pad])
        assert torch.allclose(bn.running_mean.double(), ref.rm, rtol=1e-4, atol=1e-6)
        assert bool((_full(got["y"], cout_pad)[:, Cout:] == 0).all()), "pad lanes of y (training)"
        assert bool((got["dz"][:, Cout:] == 0).all()), "pad lanes of dz"
        nxt = ops.conv_forward(None, got["y"], w2, None, None, 0, 1, 0, 1, False)
        assert bool(torch.isfinite(nxt).all()), "1x1 conv after the training forward is not finite"
    # eval: running statistics folded into the conv epilogue
    x, _, _ = _chain_inputs(case, 9)
    y = ops.conv_forward(None, ops.as_nhwc(x, dtype), w, None, bn, 1, 1, 1, 1, False)
    torch.cuda.synchronize()
    assert torch.equal(_bits(pf[2 * Cout:]), p0) and torch.equal(_bits(bf[2 * Cout:]), b0), "sentinel overwritten (eval)"
    assert bool((_full(y, cout_pad)[:, Cout:] == 0).all()), "pad lanes of y (eval)"
    z = F.conv2d(x.to(dtype).double(), ref.w, None, 1, 1)
    want = _act(F.batch_norm(z, ref.rm, ref.rv, ref.g, ref.b, training=False, eps=EPS), 1)
    assert _rel(y, want) <= TOL[dtype]
    nxt = ops.conv_forward(None, y, w2, None, None, 0, 1, 0, 1, False)
    assert bool(torch.isfinite(nxt).all()), "1x1 conv after the eval forward is not finite"


def test_p2_model_bn_buffers_do_not_depend_on_flat_state():
    """yolov8-p2 at the tiny scale has a 20-channel Detect branch (cv3 = max(ch[0], nc) with nc = 20), 24 wide in bf16.  One
    train-mode forward + backward from the same weights and batch with and without FlatState (parameters and BN buffers packed
    back to back): every BN running buffer agrees within 1e-6 relative, every BN parameter gradient within 1e-3 of its max."""
    import dedark_yolo_amd as dy
    from dedark_yolo_amd.engine.trainer import FlatState
    from test_gpu_p2p6 import _model
    g = gold("g15_p2_tiny")
    sdef = [float(v) for v in g["scale_def"]] if g["scale_def"].numel() == 3 else None
    dy.set_compute_dtype(BF)
    runs = []
    for flat in (False, True):
        model = _model("yolov8-p2.yaml", "t", sdef, int(g["seed"])).train()
        assert any(isinstance(m, nn.BatchNorm2d) and m.num_features % 8 for m in model.modules())
        if flat:
            FlatState(model, with_ema=False)
        batch = make_batch(int(g["seed"]) + 1, int(g["B"]), int(g["S"]), [int(v) for v in g["nbox"]])
        batch["img"] = batch["img"].pow(3.0).cuda()
        batch["recovery_loss_batch"] = torch.tensor(0.0123).cuda()
        loss, _ = model(batch)
        loss.backward()
        torch.cuda.synchronize()
        bns = [m for m in model.modules() if isinstance(m, nn.BatchNorm2d)]
        runs.append([(m.running_mean.clone(), m.running_var.clone(), m.weight.grad.clone(), m.bias.grad.clone()) for m in bns])
    for i, (a, b) in enumerate(zip(*runs)):
        for j in range(2):
            assert torch.allclose(b[j], a[j], rtol=1e-6, atol=0), (i, j, float((b[j] - a[j]).abs().max()))
        for j in range(2, 4):
            assert float((b[j] - a[j]).abs().max()) <= 1e-3 * max(float(a[j].abs().max()), 1e-12), (i, j)


# ------------------------------------------------------------------------------------------------- (d) dy_bn_finalize
def _finalize(stats, count, C, Cv, gamma, beta, rm, rv):
    from dedark_yolo_amd._C import call
    from dedark_yolo_amd.ops import ptr, stream
    aff = torch.full((4, C), 5.0, device="cuda")
    call("dy_bn_finalize_valid", ptr(stats), count, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), MOM, EPS, ptr(aff[0]), ptr(aff[1]),
         ptr(aff[2]), ptr(aff[3]), C, Cv, stream())
    torch.cuda.synchronize()
    return aff


@pytest.mark.parametrize("count", [2, 8, 3_000_017])
@pytest.mark.parametrize("params", ["affine+running", "no-running", "no-affine"])
def test_bn_finalize_vs_fp64(count, params):
    """Replicated f64 sums of real data (x ~ N(0.5, 2^2) per channel scale) -> scale, shift, mean, invstd and the running buffers
    against the fp64 formulas (biased variance normalises, unbiased n / (n - 1) variance updates running_var, momentum 0.03,
    eps 1e-3): f32 results within 2e-6 relative (shift: of |beta| + |mean * scale|).  NULL running buffers: not updated; NULL
    gamma / beta: 1 / 0.  C = 24 wide with 21 real channels: pad channels all 0, nothing past the 21 touched."""
    from dedark_yolo_amd import _C
    C, Cv, R = 24, 21, _C.STATS_REPLICAS
    torch.manual_seed(count % 1000)
    scale_c = torch.rand(Cv, device="cuda", dtype=torch.float64) * 2 + 0.01
    x = (torch.randn(count, Cv, device="cuda", dtype=torch.float64) * scale_c + 0.5) if count < 10 ** 6 else None
    stats = torch.zeros(R, 2, C, dtype=torch.float64, device="cuda")
    if x is not None:
        for r in range(R):
            stats[r, 0, :Cv], stats[r, 1, :Cv] = x[r::R].sum(0), (x[r::R] ** 2).sum(0)
        s1, s2 = x.sum(0), (x * x).sum(0)
    else:                                        # ~3 M pixels: generated in chunks, one replica each
        for r in range(R):
            n_r = len(range(r, count, R))
            xr = torch.randn(n_r, Cv, device="cuda", dtype=torch.float64) * scale_c + 0.5
            stats[r, 0, :Cv], stats[r, 1, :Cv] = xr.sum(0), (xr * xr).sum(0)
        s1, s2 = stats[:, 0, :Cv].sum(0), stats[:, 1, :Cv].sum(0)
    gamma = 1 + 0.3 * torch.randn(Cv + 8, device="cuda")
    beta = 0.2 * torch.randn(Cv + 8, device="cuda")
    run = torch.cat([0.1 * torch.randn(Cv, device="cuda"), torch.full((8,), -7.0, device="cuda"),
                     0.5 + torch.rand(Cv, device="cuda"), torch.full((8,), -7.0, device="cuda")])
    rm, rv = run[:Cv], run[Cv + 8:2 * Cv + 8]
    run0 = run.clone()
    g_, b_ = (gamma, beta) if params != "no-affine" else (None, None)
    rm_, rv_ = (rm, rv) if params != "no-running" else (None, None)
    aff = _finalize(stats.view(-1), count, C, Cv, g_, b_, rm_, rv_)
    m = s1 / count
    var = (s2 / count - m * m).clamp_min(0)
    inv = 1 / (var + EPS).sqrt()
    gd = gamma[:Cv].double() if g_ is not None else torch.ones_like(m)
    bd = beta[:Cv].double() if b_ is not None else torch.zeros_like(m)
    sc = gd * inv
    sh = bd - m * sc

    def ok(a, b, scale=None):
        scale = b.abs() if scale is None else scale
        return bool(((a.double() - b).abs() <= 2e-6 * scale + 1e-30).all())
    assert ok(aff[0, :Cv], sc) and ok(aff[2, :Cv], m, m.abs() + var.sqrt()) and ok(aff[3, :Cv], inv)
    assert ok(aff[1, :Cv], sh, bd.abs() + (m * sc).abs())
    assert bool((aff[:, Cv:] == 0).all()), "pad channels of scale / shift / mean / invstd"
    if rm_ is None:
        assert torch.equal(run, run0)
    else:
        want_rm = (1 - MOM) * run0[:Cv].double() + MOM * m
        want_rv = (1 - MOM) * run0[Cv + 8:2 * Cv + 8].double() + MOM * var * count / (count - 1)
        assert ok(rm, want_rm, want_rm.abs() + MOM * var.sqrt()) and ok(rv, want_rv)
        assert torch.equal(run[Cv:Cv + 8], run0[Cv:Cv + 8]) and torch.equal(run[2 * Cv + 8:], run0[2 * Cv + 8:])


def test_bn_finalize_count_one_and_bad_args():
    """count = 1 (torch refuses it in training: "Expected more than 1 value per channel"): the kernel takes the variance as 0,
    so invstd = 1 / sqrt(eps), y = beta, and the running variance decays by (1 - momentum) (n / (n - 1) is not applied).
    count = 0 and C_valid outside 1..C are rejected before any launch."""
    from dedark_yolo_amd import _C
    C, R = 8, _C.STATS_REPLICAS
    v = torch.linspace(-3, 4, C, device="cuda", dtype=torch.float64)
    stats = torch.zeros(R, 2, C, dtype=torch.float64, device="cuda")
    stats[5, 0], stats[5, 1] = v, v * v
    gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
    rm, rv = torch.randn(C, device="cuda"), torch.rand(C, device="cuda") + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    aff = _finalize(stats.view(-1), 1, C, C, gamma, beta, rm, rv)
    eps_d = torch.tensor(EPS, dtype=torch.float32).double()           # the kernel widens the f32 eps
    inv = torch.full((C,), float(1 / eps_d.sqrt()), device="cuda")
    assert torch.equal(aff[3], inv) and torch.equal(aff[2], v.float())
    assert torch.allclose(aff[1] + aff[0] * v.float(), beta, rtol=1e-5, atol=1e-5)      # y at the one pixel = beta
    assert torch.allclose(rv, (1 - MOM) * rv0, rtol=1e-6, atol=0)
    assert torch.allclose(rm, (1 - MOM) * rm0 + MOM * v.float(), rtol=1e-6, atol=1e-7)
    for count, Cv in ((0, C), (4, 0), (4, C + 1)):
        with pytest.raises(RuntimeError):
            _finalize(stats.view(-1), count, C, Cv, gamma, beta, rm, rv)


def test_unsuffixed_entries_treat_every_channel_as_real():
    """dy_bn_finalize / dy_bn_fold_eval keep their original signature: bit-identical to the *_valid entries with C_valid = C
    (dy_bn_act_bwd_apply: tests/test_gpu_bn_kernels.py)."""
    from dedark_yolo_amd import _C
    from dedark_yolo_amd._C import call
    from dedark_yolo_amd.ops import ptr, stream
    C, R = 24, _C.STATS_REPLICAS
    torch.manual_seed(3)
    x = torch.randn(640, C, device="cuda", dtype=torch.float64) + 0.3
    stats = torch.stack([torch.stack([x[r::R].sum(0), (x[r::R] ** 2).sum(0)]) for r in range(R)]).view(-1).contiguous()
    gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
    run = torch.cat([torch.randn(C, device="cuda"), torch.rand(C, device="cuda") + 0.5])
    outs = []
    for name, extra in (("dy_bn_finalize", ()), ("dy_bn_finalize_valid", (C,))):
        r = run.clone()
        aff = torch.empty(4, C, device="cuda")
        call(name, ptr(stats), 640, ptr(gamma), ptr(beta), ptr(r[:C]), ptr(r[C:]), MOM, EPS, ptr(aff[0]), ptr(aff[1]), ptr(aff[2]),
             ptr(aff[3]), C, *extra, stream())
        fold = torch.empty(2, C, device="cuda")
        call(name.replace("finalize", "fold_eval"), ptr(gamma), ptr(beta), ptr(r[:C]), ptr(r[C:]), EPS, ptr(fold[0]), ptr(fold[1]), C,
             *extra, stream())
        torch.cuda.synchronize()
        outs.append((aff, r, fold))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ----------------------------------------------------------------- (e) bias + activation backward of a conv without BatchNorm
def _nobn_ref(x, w, b, gy, act, dtype, k, groups=1, round_w=True):
    """fp64 autograd of act(conv2d(x, w) + b) on the operands as the kernels see them (the bias stays f32)"""
    xd = x.to(dtype).double().requires_grad_(True)
    wd = (w.detach().to(dtype) if round_w else w.detach()).double().requires_grad_(True)
    bd = b.detach().double().requires_grad_(True)
    y = _act(F.conv2d(xd, wd, bd, 1, k // 2, 1, groups), act)
    y.backward(gy.to(dtype).double())
    return dict(y=y.detach(), dx=xd.grad, dw=wd.grad, db=bd.grad)


def _spy_calls(monkeypatch):
    from dedark_yolo_amd import ops
    names, real_call = [], ops.call

    def spy(name, *a):
        names.append(name)
        return real_call(name, *a)
    monkeypatch.setattr(ops, "call", spy)
    return names


def _nobn_check(got, want, dtype, what):
    errs = {k_: _rel(got[k_], want[k_]) for k_ in got}
    print(f"{what}: {errs}")
    assert max(errs.values()) <= TOL[dtype], (what, errs)


@pytest.mark.parametrize("act", [0, 2, 1], ids=["none", "leaky", "silu"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("Cout", [8, 20])
@pytest.mark.parametrize("dtype", [F32, BF, FP], ids=["f32", "bf16", "f16"])
def test_conv_bias_act_backward_without_bn(dtype, Cout, k, act, monkeypatch):
    """ops.conv_forward(tape, x, w, bias, None, act, training=False) + ops.conv_backward (Detect heads, ASFF weight_levels, RFB, a
    fused RepConv) against fp64 autograd of act(conv2d(x, w) + b): y, dx, dW, dbias at TOL.  The backward must see act' at the
    pre-activation: for SiLU the forward keeps it (conv with the bias only, then dy_bn_act_fwd); none and LeakyReLU stay one
    dy_conv2d_fwd launch."""
    from dedark_yolo_amd import ops
    ops.set_compute_dtype(dtype)
    B, Cin, H, W = 2, 8, 9, 7
    torch.manual_seed(Cout * 7 + k + act)
    x, gy = torch.randn(B, Cin, H, W, device="cuda"), torch.randn(B, Cout, H, W, device="cuda")
    w = (torch.randn(Cout, Cin, k, k, device="cuda") / (Cin * k * k) ** 0.5).requires_grad_(True)
    b = (0.5 * torch.randn(Cout, device="cuda")).requires_grad_(True)
    names = _spy_calls(monkeypatch)
    tape = _Tape()
    y = ops.conv_forward(tape, ops.as_nhwc(x, dtype), w, b, None, act, 1, k // 2, 1, False)
    fwd = [n for n in names if n != "dy_pack_weight"]
    dx = ops.conv_backward(tape, ops.as_nhwc(gy, dtype), need_dx=True)
    torch.cuda.synchronize()
    got = dict(y=y, dx=dx, dw=tape.pgrads[w], db=tape.pgrads[b])
    _nobn_check(got, _nobn_ref(x, w, b, gy, act, dtype, k), dtype, f"conv {dtype} Cout={Cout} k={k} act={act}")
    assert fwd == (["dy_conv2d_fwd", "dy_bn_act_fwd"] if act == 1 else ["dy_conv2d_fwd"]), fwd


@pytest.mark.parametrize("act", [0, 2, 1], ids=["none", "leaky", "silu"])
@pytest.mark.parametrize("dtype", [F32, BF, FP], ids=["f32", "bf16", "f16"])
def test_conv_without_tape_stays_one_launch(dtype, act, monkeypatch):
    """predict / val / the inference legs of the benchmark: no tape, one dy_conv2d_fwd with bias and activation in its epilogue"""
    from dedark_yolo_amd import ops
    ops.set_compute_dtype(dtype)
    torch.manual_seed(act)
    x = torch.randn(2, 8, 9, 7, device="cuda")
    w, b = torch.randn(20, 8, 3, 3, device="cuda") / 72 ** 0.5, 0.5 * torch.randn(20, device="cuda")
    names = _spy_calls(monkeypatch)
    y = ops.conv_forward(None, ops.as_nhwc(x, dtype), w, b, None, act, 1, 1, 1, False)
    dw = ops.dwconv_forward(None, ops.as_nhwc(x, dtype), w[:8, :1].contiguous(), b[:8], None, act, 1, False)
    torch.cuda.synchronize()
    assert [n for n in names if n != "dy_pack_weight"] == ["dy_conv2d_fwd", "dy_dwconv_fwd"], names
    want = _act(F.conv2d(x.to(dtype).double(), w.to(dtype).double(), b.double(), 1, 1), act)
    assert _rel(y, want) <= TOL[dtype]
    want = _act(F.conv2d(x.to(dtype).double(), w[:8, :1].double(), b[:8].double(), 1, 1, 1, 8), act)
    assert _rel(dw, want) <= TOL[dtype]


@pytest.mark.parametrize("act", [0, 2, 1], ids=["none", "leaky", "silu"])
@pytest.mark.parametrize("dtype", [F32, BF, FP], ids=["f32", "bf16", "f16"])
def test_dwconv_bias_act_backward_without_bn(dtype, act, monkeypatch):
    """the same through ops.dwconv_forward / dwconv_backward: depthwise 3x3 over 12 channels (16 wide in the 16-bit types) with a
    bias and no BatchNorm; the depthwise weights stay f32"""
    from dedark_yolo_amd import ops
    ops.set_compute_dtype(dtype)
    B, Cc, H, W = 2, 12, 9, 7
    torch.manual_seed(40 + act)
    x, gy = torch.randn(B, Cc, H, W, device="cuda"), torch.randn(B, Cc, H, W, device="cuda")
    w = (torch.randn(Cc, 1, 3, 3, device="cuda") / 3.0).requires_grad_(True)
    b = (0.5 * torch.randn(Cc, device="cuda")).requires_grad_(True)
    names = _spy_calls(monkeypatch)
    tape = _Tape()
    y = ops.dwconv_forward(tape, ops.as_nhwc(x, dtype), w, b, None, act, 1, False)
    fwd = list(names)
    dx = ops.dwconv_backward(tape, ops.as_nhwc(gy, dtype), need_dx=True)
    torch.cuda.synchronize()
    got = dict(y=y, dx=dx, dw=tape.pgrads[w], db=tape.pgrads[b])
    _nobn_check(got, _nobn_ref(x, w, b, gy, act, dtype, 3, groups=Cc, round_w=False), dtype, f"dwconv {dtype} act={act}")
    assert fwd.count("dy_dwconv_fwd") == 1 and fwd.count("dy_bn_act_fwd") == (1 if act == 1 else 0), fwd


def test_fused_repconv_backward_with_a_tape():
    """RepConv after fuse_convs() is one 3x3 conv with a bias and SiLU in front of frozen weights; run with a tape its data
    gradient must be that of SiLU(conv2d(x, W) + b)"""
    from dedark_yolo_amd import ops
    from dedark_yolo_amd.nn.modules import RepConv
    dtype = F32
    ops.set_compute_dtype(dtype)
    torch.manual_seed(11)
    m = RepConv(8, 8).cuda()
    for br_ in (m.conv1, m.conv2):
        with torch.no_grad():
            br_.bn.weight.copy_(1.0 + 0.3 * torch.randn(8))
            br_.bn.bias.copy_(0.3 * torch.randn(8))
            br_.bn.running_mean.copy_(0.1 * torch.randn(8))
            br_.bn.running_var.copy_(0.5 + torch.rand(8))
            br_.conv.weight.mul_(3.0)
    m.eval()
    m.fuse_convs()
    x, gy = torch.randn(2, 8, 9, 7, device="cuda"), torch.randn(2, 8, 9, 7, device="cuda")
    tape = _Tape()
    y = m._fwd(tape, ops.as_nhwc(x, dtype))
    dx = m._bwd(tape, ops.as_nhwc(gy, dtype))
    torch.cuda.synchronize()
    assert not tape.stack and not tape.pgrads                   # the fused weights are frozen
    want = _nobn_ref(x, m.conv.weight, m.conv.bias, gy, 1, dtype, 3)
    _nobn_check(dict(y=y, dx=dx), {k_: want[k_] for k_ in ("y", "dx")}, dtype, "fused RepConv")
