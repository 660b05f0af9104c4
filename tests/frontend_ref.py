"""float64 references of the low-light front-end kernels (csrc/frontend.hip, csrc/usm.hip) and the input law of their tests.

Shared by tests/test_frontend_cpu.py and tests/test_gpu_frontend_kernels.py.  Everything here runs oracle/frontend.py (dtype
generic, autograd friendly) in torch.float64 on the CPU; the kernels' f32 inputs are generated in f32 and upcast, so that the
reference and the kernel see the same values.

Input law of the pointwise chain.  The chain has gradient kinks at s2 = 1e-4 (the clamp under the gamma power: with gamma < 1 the
derivative jumps by ~1e4^(1-gamma) there), at tx = 0.01 (the transmission clamp) and at lum = 1 (the clamp of the contrast
filter's per-row luminance).  f32 and f64 disagree at any pixel that lands on one, whatever the implementation, so the inputs
are CONSTRUCTED to populate every branch while staying clear of the kinks: a target s1 is drawn per pixel from a "clamped"
population (s1 < 0 -> s2 < 1e-4) and a "live" one, and x is solved from it.  `check_input_law` asserts that on the f64
reference; no pixel or row is ever left out of a comparison.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import frontend as ofe

F64 = torch.float64

# (B, H, W): both H % 4 reduction paths of pointwise_bwd_kernel, W < 64, W = 64, W = 65, W not a multiple of 64, and the
# smallest legal width 3 (every pixel feeds `lum`)
POINTWISE_SHAPES = [(2, 13, 13), (3, 37, 70), (2, 64, 96), (1, 41, 131), (2, 25, 24), (2, 6, 3), (1, 5, 64), (1, 8, 65)]


def pointwise_seed(B, H, W, aica):
    return 1000 * H + 10 * W + B + (0 if aica else 500000)


# ---------------------------------------------------------------------------------------------------------------- parameters
def params_from_feat(feat):
    """regress() as a [B,8] tensor in the kernels' slot order: omega, wb[3], gamma, alpha, lam, 0."""
    p = ofe.regress(feat)
    return torch.cat([p["omega"], p["wb"], p["gamma"], p["alpha"], p["lam"], torch.zeros_like(p["lam"])], 1)


def leaf_params(params):
    """params [B,8] -> dict of f64 LEAF tensors shaped as regress() returns them (so d loss / d param is read off .grad)."""
    q = params.detach().to(F64)
    sl = dict(omega=slice(0, 1), wb=slice(1, 4), gamma=slice(4, 5), alpha=slice(5, 6), lam=slice(6, 7))
    return {k: q[:, s].clone().requires_grad_(True) for k, s in sl.items()}


def dparams_of(p, B):
    """The .grad of leaf_params() in the layout of the kernels' dparams[B,8] (slot 7 unused)."""
    d = torch.zeros(B, 8, dtype=F64)
    for k, s in (("omega", slice(0, 1)), ("wb", slice(1, 4)), ("gamma", slice(4, 5)), ("alpha", slice(5, 6)), ("lam", slice(6, 7))):
        if p[k].grad is not None:
            d[:, s] = p[k].grad
    return d


def params_fwd_bwd(feat, dparams, dtype=F64):
    """regress and its adjoint in `dtype`: feat [B,15] f32, dparams [B,8] f64 -> (params [B,8], dfeat [B,15])."""
    f = feat.detach().to(dtype).requires_grad_(True)
    pr = params_from_feat(f)
    (pr[:, :7] * dparams[:, :7].to(dtype)).sum().backward()
    return pr.detach(), f.grad


# ---------------------------------------------------------------------------------------------------------- pointwise chain
def chain_stages(x, p, A, IcA):
    """DeDark -> white balance -> gamma -> contrast for given per-image parameters; returns (s1, s2, s3, s4)."""
    s1 = ofe.f_dedark(x, p["omega"], A, IcA)
    s2 = ofe.f_wb(s1, p["wb"])
    s3 = ofe.f_gamma(s2, p["gamma"])
    s4 = ofe.f_contrast(s3, p["alpha"])
    return s1, s2, s3, s4


def default_aica(B, H, W, dtype=F64):
    """The kernels' nullptr defaults: A = 0.8f, IcA = 0.5f (the f32 values, upcast)."""
    return torch.full((B, 3), 0.8, dtype=torch.float32).to(dtype), torch.full((B, 1, H, W), 0.5, dtype=torch.float32).to(dtype)


def pointwise_fwd_bwd(x, params, A, IcA, g4, dtype=F64):
    """Reference of dy_filters_pointwise_fwd/bwd in `dtype` (f64: the yardstick; f32: torch's own f32 error on the same case).
    A / IcA None = the defaults 0.8 / 0.5.  Returns s4, dx, dparams[B,8] for the loss sum(s4 * g4)."""
    B, _, H, W = x.shape
    if A is None:
        A, IcA = default_aica(B, H, W, dtype)
    xx = x.detach().to(dtype).requires_grad_(True)
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in leaf_params(params).items()}
    s4 = chain_stages(xx, p, A.to(dtype), IcA.to(dtype))[3]
    (s4 * g4.to(dtype)).sum().backward()
    return s4.detach(), xx.grad, dparams_of(p, B)


def _lraw(x, params, A, IcA):
    p = leaf_params(params)
    with torch.no_grad():
        s3 = chain_stages(x.to(F64), p, A.to(F64), IcA.to(F64))[2]
    return 0.27 * s3[..., 0] + 0.67 * s3[..., 1] + 0.06 * s3[..., 2]           # [B,3,H]


def pointwise_case(B, H, W, aica=True):
    """Inputs of one pointwise case, all f32: x, feat, params (f64 regress rounded once to f32), A, IcA (None when `aica` is
    false: the kernels' nullptr defaults), g4 (the upstream gradient).  The seed is chosen per case: the first of base, base + 1,
    ... whose draw meets the law (small cases can come out without a row of lum > 1)."""
    base = pointwise_seed(B, H, W, aica)
    for seed in range(base, base + 64):
        c = _draw_case(B, H, W, aica, seed)
        try:
            check_input_law(c, aica)
        except AssertionError:
            continue
        return c
    raise AssertionError(f"no seed in [{base}, {base + 64}) meets the input law for {(B, H, W, aica)}")


def _draw_case(B, H, W, aica, seed):
    g = np.random.default_rng(seed)
    u = lambda lo, hi, *s: torch.from_numpy((lo + (hi - lo) * g.random(s, dtype=np.float32)).astype(np.float32))
    feat = u(-1.5, 1.5, B, 15)
    feat[0, 0] = 4.0                                   # image 0: omega ~ 0.9993, its IcA = 1 lattice clamps tx
    params = params_from_feat(feat.to(F64)).float()
    if aica:
        A = u(0.5, 1.0, B, 3)
        IcA = u(0.0, 0.9, B, 1, H, W)
        IcA[:, :, 2::5, 1::7] = 1.0
        A_, I_ = A, IcA
    else:
        A = IcA = None
        A_, I_ = default_aica(B, H, W, torch.float32)
    clamped = u(0.0, 1.0, B, 3, H, W) < 0.3
    s1 = torch.where(clamped, u(-0.55, -0.05, B, 3, H, W), u(0.05, 1.2, B, 3, H, W)).to(F64)
    g4 = u(-1.0, 1.0, B, 3, H, W)
    om = params[:, 0].to(F64)[:, None, None, None]
    tx = (1.0 - om * I_.to(F64)).clamp(min=0.01)
    A4 = A_.to(F64)[:, :, None, None]
    solve = lambda t: ((t - A4) * tx + A4).float()     # x = (s1 - A) max(tx, 0.01) + A in f64, rounded once
    x = solve(s1)
    # rows whose luminance (columns 0..2 of the gamma stage) would sit on the lum = 1 kink: rescale those three targets, re-solve
    for _ in range(8):
        bad = (_lraw(x, params, A_, I_) - 1.0).abs() < 0.05
        if not bad.any():
            break
        s1[..., :3] = torch.where(bad[..., None] & (s1[..., :3] > 0), s1[..., :3] * 0.7, s1[..., :3])
        x = solve(s1)
    return dict(x=x, feat=feat, params=params, A=A, IcA=IcA, g4=g4, seed=seed)


def check_input_law(c, aica=True):
    """The conditions of the input law, asserted on the f64 reference of case `c`.  Returns the branch populations."""
    x, params = c["x"], c["params"]
    B, _, H, W = x.shape
    A, IcA = (c["A"], c["IcA"]) if c["A"] is not None else default_aica(B, H, W)
    p = leaf_params(params)
    with torch.no_grad():
        s1, s2, s3, _ = chain_stages(x.to(F64), p, A.to(F64), IcA.to(F64))
        tx = 1.0 - p["omega"][:, :, None, None] * IcA.to(F64)
    lraw = 0.27 * s3[..., 0] + 0.67 * s3[..., 1] + 0.06 * s3[..., 2]
    n_s2 = int(((s2 - 1e-4).abs() < 1e-2).sum())
    n_tx = int(((tx - 0.01).abs() < 5e-3).sum())
    n_lum = int(((lraw - 1.0).abs() < 0.02).sum())
    assert n_s2 == 0, f"{n_s2} pixels within 1e-2 of the s2 = 1e-4 kink"
    assert n_tx == 0, f"{n_tx} pixels within 5e-3 of the tx = 0.01 kink"
    assert n_lum == 0, f"{n_lum} rows within 0.02 of the lum = 1 kink"
    pop = dict(s2_clamped=float((s2 < 1e-4).double().mean()), tx_clamped=int((tx < 0.01).sum()),
               lum_above=int((lraw > 1).sum()), lum_below=int((lraw < 1).sum()))
    assert pop["s2_clamped"] >= 0.20 and pop["s2_clamped"] <= 0.80, pop
    if aica:                                         # with the defaults tx = 1 - 0.5 omega >= 0.5: that branch cannot be reached
        assert pop["tx_clamped"] >= 1, pop
    assert pop["lum_above"] >= 1 and pop["lum_below"] >= 1, pop
    return pop


# ------------------------------------------------------------------------------------------------------------------- USM
def usm_separable(img, lam, hp=False):
    """f_usm as two 25-tap passes over the reflect-padded image (the gaussian of filtersB.py is an outer product), in the
    dtype of `img` (f64: the yardstick).  The dense 625-tap f_usm is the definition; this is for shapes where it is slow.  lam [B,1]."""
    k = ofe.gaussian_taps(img.dtype)
    R = ofe.USM_RADIUS
    b, c, h, w = img.shape
    pad = F.pad(img, (R,) * 4, mode="reflect").reshape(b * c, 1, h + 2 * R, w + 2 * R)
    blur = F.conv2d(F.conv2d(pad, k.view(1, 1, 1, -1)), k.view(1, 1, -1, 1)).reshape(b, c, h, w)
    out = (img - blur) * lam[:, :, None, None] + img
    return (out, img - blur) if hp else out


def usm_fwd_bwd(s4, lam, g, dtype=F64):
    """Reference of dy_usm_fwd/bwd in `dtype`: s4 [B,3,H,W], lam [B], g = d loss / d out.  Returns out, hp, ds4, dlam[B]."""
    s = s4.detach().to(dtype).requires_grad_(True)
    l = lam.detach().to(dtype).reshape(-1, 1).requires_grad_(True)
    out, hp = usm_separable(s, l, hp=True)
    (out * g.to(dtype)).sum().backward()
    return out.detach(), hp.detach(), s.grad, l.grad[:, 0]


def blur_matrix(n):
    """The n x n matrix of (reflect-pad 12, 25-tap gaussian) along one axis, f64 numpy."""
    R = ofe.USM_RADIUS
    k = ofe.gaussian_taps(F64).numpy()
    M = np.zeros((n, n))
    for m in range(n):
        for d in range(-R, R + 1):
            i = m + d
            i = -i if i < 0 else (2 * (n - 1) - i if i >= n else i)
            M[m, i] += k[d + R]
    return M


# ----------------------------------------------------------------------------------------------------------------- resize
def resize_fwd_bwd(x, Ho, Wo, gy, dtype=F64):
    """Bilinear (align_corners=False) resize and its adjoint in `dtype`: x [B,3,H,W], gy [B,3,Ho,Wo] -> y, dx."""
    xx = x.detach().to(dtype).requires_grad_(True)
    if (Ho, Wo) == tuple(x.shape[2:]):
        y = xx * 1.0
    else:
        y = F.interpolate(xx, size=(Ho, Wo), mode="bilinear", align_corners=False)
    (y * gy.to(dtype)).sum().backward()
    return y.detach(), xx.grad


# ------------------------------------------------------------------------------------------------------------------ errors
def rel_err(got, ref):
    """max |got - ref| / max |ref| per leading index (image / row), worst over them; f64 on the CPU."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), "non-finite values"
    n = ref.shape[0]
    e = (got - ref).reshape(n, -1).abs().amax(1)
    d = ref.reshape(n, -1).abs().amax(1).clamp_min(1e-30)
    return float((e / d).max())


def ulp(ref, dtype):
    """One unit in the last place of `dtype` at each value of `ref` (f64)."""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.frexp(ref.abs().clamp_min(2.0 ** emin))[1] - 1
    return torch.pow(torch.tensor(2.0, dtype=F64), (e - mant).double())
