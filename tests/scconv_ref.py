"""float64 references of the SCConv kernels (csrc/scconv.hip) and of the ASFF blend (csrc/pool.hip), their error measures and the
input laws of their tests.  Shared by tests/test_scconv_ref_cpu.py and tests/test_gpu_scconv_asff_kernels.py; nothing here needs a GPU.

Layouts: SCConv tensors are [N, HW, C] (pixels x channels of every image, the kernels' NHWC views flattened), ASFF tensors
[pixels, C].  The kernels' inputs are generated in f32 (16-bit cases: exactly representable in the type) and upcast, so that the
reference and the kernel see the same values.

The SRU gate.  m = sigmoid(t) >= 0.5 with t = gn * gamma / sum(gamma) is a hard decision: an f32 evaluation can take it the other
way when gn is within its own rounding error of 0, and then moves gn between channel c and c + C/2.  An element is AMBIGUOUS when
|gn_ref| < AMBIG = 1e-4 (~100 x the f32 error of gn for |x| <= 4).  Channels with gamma == 0 and beta == 0 are not ambiguous:
gn == 0 and t == 0 there in every precision, sigmoid(0) = 0.5 passes the gate, and the forward routes a zero either way.  Forward
comparisons leave out the (pixel, c / c + C/2) pairs with an ambiguous member (share capped at SHARE_CAP per case); backward
comparisons leave out nothing, because the generator sets dy[c] = dy[c + C/2] on those pairs, which makes dgn the same whichever
way the gate falls.  Every other element must carry |t| >= MARGIN = 2.5e-7: the f32 gate 1 / (1 + expf(-t)) >= 0.5 is true for
t >= -1.2e-7 (1 + expf(-t) rounds to 2), so a negative t closer to 0 than that would be gated differently without being "ambiguous".
`check_sru_law` asserts all of it on the reference alone, and the generators walk seeds until it holds.
"""
import functools
import zlib

import numpy as np
import torch

from frontend_ref import rel_err, ulp  # noqa: F401  (re-exported: the same measures as the front-end tests)

F64 = torch.float64
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
AMBIG, SHARE_CAP, MARGIN = 1e-4, 1e-3, 2.5e-7


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31)


def _randn(g, *shape, dt="f32", scale=1.0, shift=0.0):
    """N(shift, scale) drawn in f32, rounded once to `dt`, returned as f32: exactly representable in `dt`."""
    v = torch.from_numpy((shift + scale * g.standard_normal(shape)).astype(np.float32))
    return v.to(DT[dt]).float()


# ------------------------------------------------------------------------------------------------------------------ errors
def sum_err(got, ref, terms):
    """Sums that cancel: max over the keys of |got - ref| / sum |terms|."""
    got, ref, terms = (torch.as_tensor(t).detach().double().cpu() for t in (got, ref, terms))
    assert got.shape == ref.shape == terms.shape, (tuple(got.shape), tuple(ref.shape), tuple(terms.shape))
    assert torch.isfinite(got).all(), "non-finite values"
    return float(((got - ref).abs() / terms.clamp_min(1e-300)).max())


def masked_rel_err(got, ref, keep):
    """rel_err over the elements where `keep` is set (the others count as exact; max |ref| is taken over all of them)."""
    got = torch.as_tensor(got).detach().double().cpu()
    assert torch.isfinite(got).all(), "non-finite values"
    return rel_err(torch.where(keep, got, ref.double()), ref)


# ----------------------------------------------------------------------------------------------------------------- moments
def moments_ref(x, dtype=F64):
    """[N, HW, C] -> [N, C, 2] = (sum x, sum x^2) over the pixels of every image."""
    x = x.to(dtype)
    return torch.stack((x.sum(1), (x * x).sum(1)), -1)


def moments_terms(x):
    x = x.double()
    return torch.stack((x.abs().sum(1), (x * x).sum(1)), -1)


# (N, C, HW, dtypes): 12 / 6 vectors (threads without a row) with three images; one pixel; the 1024-block cap (grid-stride trips,
# cross-block atomics); 260 vectors (a second s0 pass of 4 slots)
MOMENT_CASES = {
    "c48": (3, 48, 37, ("f32", "bf16", "f16")),
    "c8_hw1": (2, 8, 1, ("f32", "bf16", "f16")),
    "hw70000": (1, 64, 70000, ("f32",)),
    "c1040": (2, 1040, 6, ("f32",)),
}


@functools.lru_cache(maxsize=None)
def moments_case(name, dt):
    """x = 50 + offset(image, channel) + N(0, 1): a wrong image key or channel shows in the first moment, and neither moment is
    a cancelling sum.  `prior` is what the destination holds before the call (the entry ADDS)."""
    N, C, HW, _ = MOMENT_CASES[name]
    g = np.random.default_rng(_seed("moments", name, dt))
    off = torch.from_numpy(g.uniform(-3, 3, (N, 1, C)).astype(np.float32))
    x = (50.0 + off + _randn(g, N, HW, C)).to(DT[dt]).float()
    prior = torch.from_numpy(g.standard_normal((N, C, 2)) * 10.0)
    return dict(x=x, prior=prior, N=N, C=C, HW=HW)


# --------------------------------------------------------------------------------------------------------------------- SRU
def _swap(t):
    h = t.shape[-1] // 2
    return torch.cat((t[..., h:], t[..., :h]), -1)


def group_norm(x, groups, eps):
    """(x - mean_g) / (std_g + eps), mean and UNBIASED std over the pixels and channels of each of `groups` channel groups of
    every image; eps outside the root.  A constant group has std 0 and contributes no gradient through std.  Returns xhat, std."""
    N, HW, C = x.shape
    xg = x.reshape(N, HW, groups, C // groups)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).sum((1, 3), keepdim=True) / (HW * (C // groups) - 1)
    sd = torch.where(var > 0, var.clamp_min(torch.finfo(var.dtype).tiny).sqrt(), torch.zeros_like(var))
    return ((xg - mean) / (sd + eps)).reshape(N, HW, C), sd.reshape(N, groups)


def sru_ref(x, gamma, beta, groups, eps, dtype=F64):
    """SRU forward in `dtype`: y, gn and the gate margin t = gn * gamma / sum(gamma); the gate is sigmoid(t) >= 0.5."""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    gn = group_norm(x, groups, eps)[0] * gamma + beta
    t = gn * (gamma / gamma.sum())
    m = torch.sigmoid(t) >= 0.5
    keep, rest = gn * m, gn * ~m
    return keep + _swap(rest), gn, t


def sru_dx_from_red(x, dgn, gamma, groups, eps, red):
    """dx from the reduced sums red[N, C, 2] the apply pass is handed (what the entry holds in `red` after its first pass, any
    prior content included): dx = (dxhat - mean_g dxhat) / (std + eps) - xhat sum_c gamma red1 / ((cnt - 1) std), dxhat = dgn gamma."""
    N, HW, C = x.shape
    cpg = C // groups
    x, dgn, gamma = x.double(), dgn.double(), gamma.double()
    xhat, sd = group_norm(x, groups, eps)
    cnt = HW * cpg
    gr = (gamma[None, :, None] * red).reshape(N, groups, cpg, 2).sum(2)
    m1 = gr[..., 0] / cnt
    k = torch.where(sd > 0, gr[..., 1] / ((cnt - 1) * sd.clamp_min(1e-300)), torch.zeros_like(sd))
    per_c = lambda v: v.repeat_interleave(cpg, 1)[:, None, :]
    return (dgn * gamma - per_c(m1)) / (per_c(sd) + eps) - xhat * per_c(k)


def sru_bwd_ref(x, dy, gamma, beta, groups, eps, prior=None, dtype=F64):
    """dx, red[N, C, 2] = (sum dgn, sum dgn xhat) with dgn[c] = m[c] ? dy[c] : dy[c'], and sum |terms| of red.  dx is autograd
    through sru_ref (the mask is a constant there); with a `prior` content of red, the apply pass sees prior + red."""
    xl = x.to(dtype).requires_grad_(True)
    y, _, t = sru_ref(xl, gamma, beta, groups, eps, dtype)
    (y * dy.to(dtype)).sum().backward()
    with torch.no_grad():
        m = torch.sigmoid(t) >= 0.5
        dgn = torch.where(m, dy.to(dtype), _swap(dy.to(dtype)))
        xhat = group_norm(x.to(dtype), groups, eps)[0]
        red = torch.stack((dgn.sum(1), (dgn * xhat).sum(1)), -1)
        terms = torch.stack((dgn.abs().sum(1), (dgn * xhat).abs().sum(1)), -1)
        dx = xl.grad if prior is None else sru_dx_from_red(x, dgn, gamma, groups, eps, prior + red)
    return dx, red, terms


# (N, C, G, HW), eps, sign of sum(gamma), special, dtypes.  eps = 1e-10 is GroupBatchnorm2d's; the larger ones make "eps outside the
# root" visible in f32 (1 / (std + 0.25) against rsqrt(var + 0.25)) and keep 1 / (0 + eps) of the constant group inside f16.
SRU_CASES = {
    "golden_shape": ((2, 64, 4, 63), 1e-10, +1, None, ("f32", "bf16", "f16")),
    "c48": ((2, 48, 4, 35), 0.25, +1, None, ("f32", "bf16", "f16")),                 # 6 / 3 vectors per half
    "g16_blocks": ((3, 96, 16, 1100), 1e-10, +1, None, ("f32", "bf16", "f16")),      # several blocks per image
    "g64": ((2, 128, 64, 40), 1e-10, +1, None, ("f32", "bf16", "f16")),              # the LDS array bound, cpg = 2
    "c2080": ((1, 2080, 4, 6), 1e-10, +1, None, ("f32",)),                           # 260 vectors per half: second s0 pass
    "neg_wsum": ((2, 64, 4, 63), 1e-10, -1, None, ("f32", "bf16", "f16")),           # the gate follows -gn
    "zero_channel": ((2, 64, 4, 63), 1e-10, +1, "zero_channel", ("f32", "bf16", "f16")),
    "const_group": ((2, 64, 4, 63), 0.25, +1, "const_group", ("f32", "bf16", "f16")),
}
ZERO_CHANNELS = (5, 41)            # one in each half, not a pair


def _draw_sru(name, dt, seed):
    (N, C, G, HW), eps, sign, special, _ = SRU_CASES[name]
    g = np.random.default_rng(seed)
    x = _randn(g, N, HW, C).clamp(-4, 4).to(DT[dt]).float()
    gamma = torch.from_numpy(g.standard_normal(C).astype(np.float32))
    beta = torch.from_numpy((0.3 * g.standard_normal(C)).astype(np.float32))
    if float(gamma.double().sum()) * sign < 0:
        gamma = -gamma
    if special == "zero_channel":
        for c in ZERO_CHANNELS:
            gamma[c] = beta[c] = 0.0
    if special == "const_group":
        cpg = C // G
        x[0, :, cpg:2 * cpg] = 1.5                                   # image 0, group 1: mean 1.5 and std 0 exactly
    eps = float(np.float32(eps))
    with torch.no_grad():
        _, gn, t = sru_ref(x, gamma, beta, G, eps)
    amb = ambiguous(gn, gamma, beta)
    pair = amb | _swap(amb)
    dy = _randn(g, N, HW, C, dt=dt)
    h = C // 2
    dy[..., h:] = torch.where(pair[..., :h], dy[..., :h], dy[..., h:])
    red_prior = torch.from_numpy(g.standard_normal((N, C, 2)))
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, eps=eps, N=N, C=C, G=G, HW=HW, sign=sign, special=special, seed=seed,
                red_prior=red_prior)


def ambiguous(gn, gamma, beta):
    live = ~((gamma == 0) & (beta == 0))
    return (gn.abs() < AMBIG) & live


def check_sru_law(c):
    """The conditions of the SRU input law on the f64 reference of case `c`; returns the figures."""
    with torch.no_grad():
        _, gn, t = sru_ref(c["x"], c["gamma"], c["beta"], c["G"], c["eps"])
    amb = ambiguous(gn, c["gamma"], c["beta"])
    pair = amb | _swap(amb)
    share = float(pair.double().mean())
    assert share <= SHARE_CAP, f"ambiguous share {share:.2e}"
    wsum = float(c["gamma"].double().sum())
    assert abs(wsum) >= 0.5 and wsum * c["sign"] > 0, f"sum gamma {wsum}"
    live = ~((c["gamma"] == 0) & (c["beta"] == 0))
    clear = ~amb & live
    margin = float(t.abs()[clear.expand_as(t)].min())
    assert margin >= MARGIN, f"gate margin {margin:.2e} on an unambiguous element"
    m = t >= 0
    h = c["C"] // 2
    for part in (m[..., :h], m[..., h:]):
        assert bool(part.any()) and not bool(part.all()), "a channel half with one mask value only"
    assert float(c["x"].abs().max()) <= 4.0
    assert bool((c["dy"][..., :h][pair[..., :h]] == c["dy"][..., h:][pair[..., :h]]).all())
    return dict(share=share, wsum=wsum, margin=margin, n_ambiguous=int(amb.sum()))


@functools.lru_cache(maxsize=None)
def sru_case(name, dt):
    base = _seed("sru", name, dt)
    for seed in range(base, base + 64):
        c = _draw_sru(name, dt, seed)
        try:
            check_sru_law(c)
        except AssertionError:
            continue
        return c
    raise AssertionError(f"no seed in [{base}, {base + 64}) meets the SRU input law for {name} {dt}")


def gate_flips(y_got, gn, m_ref, pair_ambiguous, tol):
    """Gate decisions of the kernel that differ from the reference on unambiguous pairs, recomputed from its output: of the four
    routings of a pair (gn[c], gn[c']) the one nearest to (y[c], y[c']) is the kernel's; a flip is a pair whose nearest routing is
    not the reference's while the reference's own is further away than `tol` (elementwise, [N, HW, C/2])."""
    h = gn.shape[-1] // 2
    a, b = gn[..., :h], gn[..., h:]
    z = torch.zeros_like(a)
    cand = {(1, 1): (a, b), (1, 0): (a + b, z), (0, 1): (z, a + b), (0, 0): (b, a)}
    ya, yb = y_got[..., :h].double(), y_got[..., h:].double()
    dist = {k: torch.maximum((ya - u).abs(), (yb - v).abs()) for k, (u, v) in cand.items()}
    ma, mb = m_ref[..., :h], m_ref[..., h:]
    d_ref = torch.zeros_like(a)
    for (ka, kb), d in dist.items():
        d_ref = torch.where((ma == bool(ka)) & (mb == bool(kb)), d, d_ref)
    d_min = torch.stack(list(dist.values())).amin(0)
    flipped = (d_ref > d_min) & (d_ref > tol) & ~pair_ambiguous[..., :h]
    return int(flipped.sum())


# ---------------------------------------------------------------------------------------------------------------- CRU tail
def cru_fuse_ref(o, dtype=F64):
    """o [N, HW, 2C] -> res [N, HW, C] = o[c] s[c] + o[c + C] s[c + C], s = softmax over the 2C per-image pixel means; returns res, s."""
    o = o.to(dtype)
    C = o.shape[-1] // 2
    s = torch.softmax(o.mean(1), -1)
    w = o * s[:, None, :]
    return w[..., :C] + w[..., C:], s


def cru_fuse_bwd_ref(o, dres, ds_prior=None, dtype=F64):
    """dout [N, HW, 2C], ds [N, 2C] = sum over pixels of dres[c(k)] o[k], and sum |terms| of ds.
    dout[k] = dres[c(k)] s[k] + s[k] (ds[k] - sum_j s[j] ds[j]) / HW; with a `ds_prior`, the apply pass sees prior + ds."""
    o, dres = o.to(dtype), dres.to(dtype)
    HW = o.shape[1]
    _, s = cru_fuse_ref(o, dtype)
    d2 = torch.cat((dres, dres), -1)
    ds = (d2 * o).sum(1)
    terms = (d2 * o).abs().sum(1)
    tot = ds if ds_prior is None else ds + ds_prior.to(dtype)
    dot = (s * tot).sum(-1, keepdim=True)
    dout = d2 * s[:, None, :] + (s * (tot - dot) / HW)[:, None, :]
    return dout, ds, terms


# (N, C, HW), kind, dtypes.  K = 2C < 256: idle threads feed -inf / 0 into the wave reductions; K = 512: strided softmax loop;
# several blocks; the contract's limit C = 2048 (four s0 passes of the moments and two of ds, 16 / 32 KB of LDS)
CRU_CASES = {
    "c16": ((2, 16, 35), "normal", ("f32", "bf16", "f16")),
    "c48": ((2, 48, 35), "normal", ("f32", "bf16", "f16")),
    "c256": ((2, 256, 400), "normal", ("f32", "bf16", "f16")),
    "c64_blocks": ((2, 64, 3000), "normal", ("f32", "bf16", "f16")),
    "c2048": ((1, 2048, 2), "normal", ("f32",)),
    "offsets": ((2, 48, 35), "offsets", ("f32", "bf16", "f16")),
    "equal_means": ((2, 48, 36), "equal", ("f32", "bf16", "f16")),
}
CRU_OFFSETS = {3: 100.0, 50: 99.5, 77: 98.0, 20: 50.0}        # channel of the 2C -> offset of its pooled mean


@functools.lru_cache(maxsize=None)
def cru_case(name, dt):
    (N, C, HW), kind, _ = CRU_CASES[name]
    g = np.random.default_rng(_seed("cru", name, dt))
    off = torch.from_numpy(g.standard_normal((N, 1, 2 * C)).astype(np.float32))
    if kind == "offsets":
        for k, v in CRU_OFFSETS.items():
            off[:, :, k] += v
    o = (off + _randn(g, N, HW, 2 * C)).to(DT[dt]).float()
    if kind == "equal":                                           # pixel p + HW/2 = -pixel p: every pooled mean is exactly 0
        o[:, HW // 2:] = -o[:, :HW // 2]
    dres = _randn(g, N, HW, C, dt=dt)
    ds_prior = torch.from_numpy(g.standard_normal((N, 2 * C, 2)))
    return dict(o=o, dres=dres, ds_prior=ds_prior, N=N, C=C, HW=HW, kind=kind)


# -------------------------------------------------------------------------------------------------------------------- ASFF
def asff_ref(xs, logits, dtype=F64):
    """out = sum_k w_k x_k, w = softmax over the first len(xs) logits of every pixel; returns out, w."""
    k = len(xs)
    w = torch.softmax(logits[:, :k].to(dtype), -1)
    return sum(x.to(dtype) * w[:, j:j + 1] for j, x in enumerate(xs)), w


def asff_bwd_ref(xs, logits, dout, priors=None, dtype=F64):
    """dx_k = [prior_k +] dout w_k, dlogits_k = w_k (d_k - sum_j w_j d_j) with d_k = sum_c dout x_k; priors[k] None = written."""
    k = len(xs)
    _, w = asff_ref(xs, logits, dtype)
    dout = dout.to(dtype)
    d = torch.stack([(dout * x.to(dtype)).sum(-1) for x in xs], -1)
    dlog = w * (d - (w * d).sum(-1, keepdim=True))
    dxs = [dout * w[:, j:j + 1] for j in range(k)]
    if priors is not None:
        dxs = [dx if p is None else dx + p.to(dtype) for dx, p in zip(dxs, priors)]
    return dxs, dlog


# (pixels, C) per dtype family: one pixel; three (a normal, a saturated and an all-equal row); more pixels than 4096 blocks x 4
# waves (second grid-stride trip); 66 vectors (the second lane trip has 2 lanes); 16 / 32 vectors
ASFF_SHAPES = {"p1": (1, 16, 16), "p3": (3, 16, 16), "p16389": (16389, 16, 16), "v66": (37, 264, 528), "c128": (37, 128, 128)}
ASFF_LOGIT_KINDS = ("normal", "mixed", "offset")


@functools.lru_cache(maxsize=None)
def asff_case(shape, nsrc, ldl, kind, dt):
    """Sources, logits [P, ldl] (columns >= nsrc hold garbage the kernels must not use), dout and priors, all exactly representable
    in `dt`.  kind "mixed": row 3i+1 has one logit 80 above the others (weights saturate), row 3i+2 all logits equal; "offset":
    the same plus a common offset of +1000 (f16: +100), rounded to `dt` (the rounded values ARE the inputs)."""
    P, c32, c16 = ASFF_SHAPES[shape]
    C = c32 if dt == "f32" else c16
    g = np.random.default_rng(_seed("asff", shape, nsrc, ldl, kind, dt))
    xs = [_randn(g, P, C, dt=dt) for _ in range(nsrc)]
    lg = torch.from_numpy((2.0 * g.standard_normal((P, ldl))).astype(np.float32))
    if kind != "normal":
        r = torch.arange(P)
        sat = r % 3 == 1
        lg[sat, (r[sat] // 3) % nsrc] += 80.0
        eq = r % 3 == 2
        lg[eq, :nsrc] = lg[eq, :1]
    if kind == "offset":
        lg[:, :nsrc] += 100.0 if dt == "f16" else 1000.0
    lg = lg.to(DT[dt]).float()
    dout = _randn(g, P, C, dt=dt)
    priors = [_randn(g, P, C, dt=dt) for _ in range(nsrc)]
    return dict(xs=xs, logits=lg, dout=dout, priors=priors, P=P, C=C, nsrc=nsrc, ldl=ldl)
