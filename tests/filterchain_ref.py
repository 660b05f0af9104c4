"""float64 reference of an arbitrary front-end filter chain (csrc/filterchain.hip), the input law of its tests and the measured
error of the same formulas in torch f32.

Shared by tests/test_filterchain_cpu.py and tests/test_gpu_filterchain.py.  A chain is a tuple of the reference filters' short
names (DF, W, G, T, Ct, UF).  The stages are oracle.frontend.f_dedark / f_wb / f_gamma / f_contrast / f_usm plus f_tone below
(filtersB.py:262-286); everything is generic over dtype and works with autograd.  The kernels' f32 inputs are generated in f32
and upcast, so that the reference and the kernel see the same values.

Input law.  It is the law of tests/frontend_ref.py -- populate every branch, stay clear of every kink, leave no pixel or row out
of a comparison -- carried over to any stage order, plus the tone filter's kinks:
  * gamma: the clamp at 1e-4 under the power; no value entering G within 1e-2 of it, between 10 % and 90 % of them clamped;
  * dedark: the transmission clamp tx = 0.01; none within 5e-3 of it, at least one pixel clamped when IcA is given;
  * contrast: clamp(lum, 0, 1); no row's raw luminance within 0.02 of 0 or of 1, rows inside (0, 1) present, and rows above 1
    unless a tone stage precedes the contrast (the curve ends at 1);
  * tone: the nine knots i/8 of the curve; no value entering T within KNOT_MARGIN of a knot, every one of the eight segments
    populated, values above 1 present, values below 0 present when the chain can produce them (no gamma in front of T: a power
    is positive).  A pixel that the gamma clamp floored enters a later T as the constant pow(1e-4, gamma), which for gamma >= 0.68
    lies within KNOT_MARGIN of knot 0; the chains that feed G into T therefore draw feature 4 from [-1.5, -0.5], gamma in
    [0.37, 0.60], which puts the floor at 4e-3 .. 3.3e-2, inside segment 0 and clear of both its knots.  gamma > 1 is covered by
    the chain [G] and by the fixtures.  No pixel is exempt from the margin.
x is drawn from a "negative" and a "live" population (through the inverse of a leading DF, as frontend_ref solves x from s1);
pixels that violate a margin are re-drawn until none does, then `check_chain_law` asserts all of the above on the f64 reference.

`python tests/filterchain_ref.py` prints, per group of the GPU test, the worst error E of the same formula evaluated by torch in
f32 on the CPU over the group's cases, and the bound 4 E rounded up to one significant digit and capped at the project ceilings.
"""
import functools
import math
import os
import sys

import numpy as np
import torch

if __name__ == "__main__":                          # run as a script: the repository root (oracle/) is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import frontend as ofe
import frontend_ref as fr

F64 = torch.float64
NAMES = ("DF", "W", "G", "T", "Ct", "UF")
DEFAULT = ("DF", "W", "G", "Ct", "UF")
STEPS = 8                     # cfg.curve_steps (filter_cfg.py:28)
TONE_BEGIN = 5                # cfg.tone_begin_param (filter_cfg.py:23)
TONE_RANGE = (0.5, 2.0)       # cfg.tone_curve_range (filter_cfg.py:34)
KNOT_MARGIN = 2e-3

# the GPU test's cases (the issue's): both H % 4 reduction paths, W below / at-and-past 64, the minimum width
SHAPES = [(2, 13, 13), (3, 37, 70), (1, 41, 131), (2, 6, 3), (1, 8, 65)]
CHAINS = [("T",), ("G",), ("W", "G", "T", "Ct"), ("DF", "W", "G", "T", "Ct"), ("Ct", "T"), ("T", "DF", "Ct", "W")]
TONE_B, TONE_LD = [1, 64, 65, 130], [15, 16, 24]
FWD_CEILING, GRAD_CEILING = 1e-4, 2e-3
GROUPS = ("tone_fwd", "tone_bwd", "chain_fwd", "chain_fwd_fast", "chain_dx", "chain_dx_fast", "chain_dparams", "chain_dparams_fast")


# ----------------------------------------------------------------------------------------------------------------- stages
def tone_from_feat(feat):
    """ToneFilter.filter_param_regressor (filtersB.py:271-274): t[B,8] = tanh_range(0.5, 2)(feat[:, 5:13])."""
    return ofe.squash(feat[:, TONE_BEGIN:TONE_BEGIN + STEPS], *TONE_RANGE)


def f_tone(img, t):
    """filtersB.py:276-286, restated: y = (8 / T) sum_i clamp(v - i/8, 0, 1/8) t_i with T = sum t_i + 1e-30; t [B,8], the same
    eight values for all three channels; torch.clamp passes the gradient on both bounds."""
    T = t.sum(1) + 1e-30
    tot = img * 0
    for i in range(STEPS):
        tot = tot + torch.clamp(img - 1.0 * i / STEPS, 0, 1.0 / STEPS) * t[:, i, None, None, None]
    return tot * STEPS / T[:, None, None, None]


def f_tone_reference_loop(img, feat_tone):
    """the reference's own lines (filtersB.py:271-286) on its own 5-d parameter layout; only for the autograd comparison"""
    param = ofe.squash(feat_tone.view(-1, 1, STEPS).unsqueeze(1).unsqueeze(2), *TONE_RANGE)
    s = torch.sum(param, dim=4) + 1e-30
    total = img * 0
    for i in range(STEPS):
        total = total + torch.clamp(img - 1.0 * i / STEPS, 0, 1.0 / STEPS) * param[:, :, :, :, i]
    return total * STEPS / s


def chain_forward(x, p, A, IcA, names, taps=None):
    """The chain on x; p: dict omega, wb, gamma, alpha, lam (as oracle.frontend.regress) and tone [B,8].  A filter sees the output
    of the filter before it.  `taps` (a dict) receives the input of every stage under its name."""
    v = x
    for n in names:
        if taps is not None:
            taps[n] = v
        if n == "DF":
            v = ofe.f_dedark(v, p["omega"], A, IcA)
        elif n == "W":
            v = ofe.f_wb(v, p["wb"])
        elif n == "G":
            v = ofe.f_gamma(v, p["gamma"])
        elif n == "T":
            v = f_tone(v, p["tone"])
        elif n == "Ct":
            v = ofe.f_contrast(v, p["alpha"])
        elif n == "UF":
            v = ofe.f_usm(v, p["lam"])
        else:
            raise ValueError(n)
    return v


def regress_all(feat):
    p = ofe.regress(feat)
    p["tone"] = tone_from_feat(feat)
    return p


def lowlight(sd, prefix, x, names, A=None, IcA=None):
    """oracle.frontend.lowlight_recovery with a chain: resize -> extractor -> chain_forward (llie.py:17-54)."""
    import torch.nn.functional as F
    B, _, H, W = x.shape
    if A is None:
        A = torch.full((B, 3), 0.8, dtype=x.dtype)
    if IcA is None:
        IcA = torch.full((B, 1, H, W), 0.5, dtype=x.dtype)
    r = F.interpolate(x, size=(256, 256), mode="bilinear", align_corners=False)
    feat = ofe.extractor(sd, prefix + "extractor.", r)
    return chain_forward(x, regress_all(feat), A, IcA, names), feat


def _leafs(params, tone, dtype):
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in fr.leaf_params(params).items()}
    p["tone"] = tone.detach().to(dtype).clone().requires_grad_(True)
    return p


def chain_fwd_bwd(x, params, tone, A, IcA, g, names, dtype=F64, forward=chain_forward):
    """Reference of dy_filter_chain_fwd/bwd in `dtype` (f64: the yardstick; f32: torch's own f32 error on the same case).  A / IcA
    None = the defaults 0.8 / 0.5.  Returns y, dx, dparams[B,8], dtone[B,8] for the loss sum(y * g)."""
    B, _, H, W = x.shape
    if A is None:
        A, IcA = fr.default_aica(B, H, W, dtype)
    xx = x.detach().to(dtype).requires_grad_(True)
    p = _leafs(params, tone, dtype)
    y = forward(xx, p, A.to(dtype), IcA.to(dtype), names)
    (y * g.to(dtype)).sum().backward()
    dtone = p["tone"].grad if p["tone"].grad is not None else torch.zeros(B, STEPS, dtype=dtype)
    dx = xx.grad if xx.grad is not None else torch.zeros_like(xx)
    return y.detach(), dx, fr.dparams_of(p, B), dtone


def tone_params_fwd_bwd(feat, dtone, dtype=F64):
    """tone_from_feat and its adjoint in `dtype`: feat [B,15] f32, dtone [B,8] f64 -> (tone [B,8], dfeat [B,15])."""
    f = feat.detach().to(dtype).requires_grad_(True)
    t = tone_from_feat(f)
    (t * dtone.to(dtype)).sum().backward()
    return t.detach(), f.grad


# ---------------------------------------------------------------------------------------------------------------- the law
def _stage_inputs(c, names):
    x, params, tone = c["x"], c["params"], c["tone"]
    B, _, H, W = x.shape
    A, IcA = (c["A"], c["IcA"]) if c["A"] is not None else fr.default_aica(B, H, W)
    p = {k: v.detach() for k, v in fr.leaf_params(params).items()}
    p["tone"] = tone.to(F64)
    taps = {}
    with torch.no_grad():
        chain_forward(x.to(F64), p, A.to(F64), IcA.to(F64), names, taps)
        tx = 1.0 - p["omega"][:, :, None, None] * IcA.to(F64)
    return taps, tx, p


def _gamma_feeds_tone(names):
    return "G" in names and "T" in names and names.index("G") < names.index("T")


def _violations(c, names):
    """(bad pixel mask [B,3,H,W], taps, tx): pixels within a margin of a kink; a row whose luminance is, through its columns 0..2"""
    taps, tx, _ = _stage_inputs(c, names)
    bad = torch.zeros_like(c["x"], dtype=torch.bool)
    if "G" in names:
        bad |= (taps["G"] - 1e-4).abs() < 1e-2
    if "T" in names:
        v = taps["T"]
        near = torch.zeros_like(bad)
        for i in range(STEPS + 1):
            near |= (v - i / STEPS).abs() < KNOT_MARGIN
        bad |= near
    if "Ct" in names:
        v = taps["Ct"]
        lraw = 0.27 * v[..., 0] + 0.67 * v[..., 1] + 0.06 * v[..., 2]
        row = ((lraw - 1.0).abs() < 0.02) | (lraw.abs() < 0.02)
        bad[..., :3] |= row[..., None]
    return bad, taps, tx


def _draw_case(B, H, W, names, aica, seed):
    g = np.random.default_rng(seed)
    u = lambda lo, hi, *s: torch.from_numpy((lo + (hi - lo) * g.random(s, dtype=np.float32)).astype(np.float32))
    feat = u(-1.5, 1.5, B, 15)
    feat[0, 0] = 4.0                                   # image 0: omega ~ 0.9993, its IcA = 1 lattice clamps tx
    if _gamma_feeds_tone(names):
        feat[:, 4] = u(-1.5, -0.5, B)                  # gamma in [0.37, 0.60]: the clamp's floor pow(1e-4, gamma) clears knot 0
    params = fr.params_from_feat(feat.to(F64)).float()
    tone = tone_from_feat(feat.to(F64)).float()
    if aica:
        A = u(0.5, 1.0, B, 3)
        IcA = u(0.0, 0.9, B, 1, H, W)
        IcA[:, :, 2::5, 1::7] = 1.0
        A_, I_ = A, IcA
    else:
        A = IcA = None
        A_, I_ = fr.default_aica(B, H, W, torch.float32)
    om = params[:, 0].to(F64)[:, None, None, None]
    tx = (1.0 - om * I_.to(F64)).clamp(min=0.01)
    A4 = A_.to(F64)[:, :, None, None]

    def draw():                                        # the value entering the first stage behind a leading DF, else x itself
        neg = u(0.0, 1.0, B, 3, H, W) < 0.28
        t = torch.where(neg, u(-0.55, -0.05, B, 3, H, W), u(0.05, 1.35, B, 3, H, W)).to(F64)
        return ((t - A4) * tx + A4).float() if names[0] == "DF" else t.float()
    c = dict(x=draw(), feat=feat, params=params, tone=tone, A=A, IcA=IcA, g=u(-1.0, 1.0, B, 3, H, W), seed=seed)
    for _ in range(60):
        bad, _, _ = _violations(c, names)
        if not bad.any():
            break
        c["x"] = torch.where(bad, draw(), c["x"])
    return c


def check_chain_law(c, names, aica=True):
    """The conditions of the input law, asserted on the f64 reference of case `c`.  Returns the branch populations."""
    bad, taps, tx = _violations(c, names)
    assert not bad.any(), f"{int(bad.sum())} pixels within a margin of a kink"
    pop = {}
    if "DF" in names:
        n_tx = int(((tx - 0.01).abs() < 5e-3).sum())
        assert n_tx == 0, f"{n_tx} pixels within 5e-3 of the tx = 0.01 kink"
        pop["tx_clamped"] = int((tx < 0.01).sum())
        if aica:                                     # with the defaults tx = 1 - 0.5 omega >= 0.5: that branch cannot be reached
            assert pop["tx_clamped"] >= 1, pop
    if "G" in names:
        pop["gamma_clamped"] = float((taps["G"] < 1e-4).double().mean())
        assert 0.10 <= pop["gamma_clamped"] <= 0.90, pop
    if "Ct" in names:
        v = taps["Ct"]
        lraw = 0.27 * v[..., 0] + 0.67 * v[..., 1] + 0.06 * v[..., 2]
        pop["lum_above"], pop["lum_inside"] = int((lraw > 1).sum()), int(((lraw > 0) & (lraw < 1)).sum())
        assert pop["lum_inside"] >= 1, pop
        if "T" not in names[:names.index("Ct")]:     # a tone curve ends at 1: nothing behind it is above
            assert pop["lum_above"] >= 1, pop
    if "T" in names:
        v = taps["T"]
        for i in range(STEPS + 1):
            d = (v - i / STEPS).abs()
            assert float(d.min()) >= KNOT_MARGIN, (i, float(d.min()))
        pop["tone_segments"] = [int(((v > i / STEPS) & (v < (i + 1) / STEPS)).sum()) for i in range(STEPS)]
        pop["tone_below"], pop["tone_above"] = int((v < 0).sum()), int((v > 1).sum())
        assert min(pop["tone_segments"]) >= 1 and pop["tone_above"] >= 1, pop
        if "G" not in names[:names.index("T")]:
            assert pop["tone_below"] >= 1, pop
    return pop


def chain_seed(B, H, W, names, aica):
    return 100000 * (1 + sum((NAMES.index(n) + 1) * 7 ** k for k, n in enumerate(names)) % 997) + 1000 * H + 10 * W + B + (0 if aica else 500)


@functools.lru_cache(maxsize=None)
def chain_case(shape, names, aica=True):
    """Inputs of one chain case, all f32: x, feat, params, tone (f64 regressors rounded once to f32), A, IcA (None when `aica` is
    false: the kernels' nullptr defaults), g (the upstream gradient).  The seed is the first of base, base + 1, ... whose draw
    meets the law."""
    B, H, W = shape
    base = chain_seed(B, H, W, names, aica)
    for seed in range(base, base + 64):
        c = _draw_case(B, H, W, names, aica, seed)
        try:
            check_chain_law(c, names, aica)
        except AssertionError:
            continue
        return c
    raise AssertionError(f"no seed in [{base}, {base + 64}) meets the input law for {(shape, names, aica)}")


@functools.lru_cache(maxsize=None)
def chain_refs(shape, names, aica=True):
    """(case, f64 reference, the same formula in torch f32) of one chain case; computed once, shared, never modified"""
    c = chain_case(shape, names, aica)
    ref = chain_fwd_bwd(c["x"], c["params"], c["tone"], c["A"], c["IcA"], c["g"], names)
    t32 = chain_fwd_bwd(c["x"], c["params"], c["tone"], c["A"], c["IcA"], c["g"], names, torch.float32)
    return c, ref, t32


def tone_feat_case(B, ld):
    """features with saturated tanh slots, inside a buffer whose pad columns hold garbage the kernels must not use"""
    g = np.random.default_rng(7100 + 10 * B + ld)
    u = lambda lo, hi, *s: torch.from_numpy((lo + (hi - lo) * g.random(s, dtype=np.float32)).astype(np.float32))
    feat = u(-2.0, 2.0, B, 15)
    sat = torch.from_numpy(g.random((B, 15))) < 0.15
    feat = torch.where(sat, torch.where(torch.from_numpy(g.random((B, 15))) < 0.5, -10.0, 10.0).float(), feat)
    buf = u(-3.0, 3.0, B, ld)
    buf[:, :15] = feat
    dt = torch.from_numpy(g.standard_normal((B, STEPS)))
    return feat, buf, dt


def knot_case():
    """Chain [T] alone with pixels exactly ON the knots i/8 (and just beside them): pins the inclusive-clamp rule -- at a knot the
    derivative is (t_{i-1} + t_i) 8 / T, outside [0, 1] it is 0 -- against torch autograd in f64.  B = 1, 3 x 4 x 9."""
    g = np.random.default_rng(8801)
    knots = torch.arange(STEPS + 1, dtype=torch.float32) / STEPS         # exact in f32
    x = torch.stack([knots, knots, knots - 0.25, knots + 0.25]).repeat(3, 1, 1)[None].contiguous()      # [1,3,4,9]
    feat = torch.from_numpy(g.uniform(-1.5, 1.5, (1, 15)).astype(np.float32))
    return dict(x=x, feat=feat, params=fr.params_from_feat(feat.to(F64)).float(), tone=tone_from_feat(feat.to(F64)).float(), A=None, IcA=None,
                g=torch.from_numpy(g.uniform(-1, 1, (1, 3, 4, 9)).astype(np.float32)))


# ------------------------------------------------------------------------------------------------------------- the bounds
def round_up_1sig(v):
    e = math.floor(math.log10(v))
    m = math.ceil(v / 10 ** e - 1e-9)
    return float(f"{m}e{e}") if m < 10 else float(f"1e{e + 1}")


def measure_E():
    """Per group: the worst error of the same formula evaluated by torch in f32 on the CPU over the group's cases (exact and fast
    groups share their cases, so they share E)."""
    E = dict.fromkeys(GROUPS, 0.0)
    for B in TONE_B:
        for ld in TONE_LD:
            feat, _, dt = tone_feat_case(B, ld)
            ref, t32 = tone_params_fwd_bwd(feat, dt), tone_params_fwd_bwd(feat, dt, torch.float32)
            E["tone_fwd"] = max(E["tone_fwd"], fr.rel_err(t32[0], ref[0]))
            E["tone_bwd"] = max(E["tone_bwd"], fr.rel_err(t32[1][:, TONE_BEGIN:TONE_BEGIN + STEPS], ref[1][:, TONE_BEGIN:TONE_BEGIN + STEPS]))
    for shape in SHAPES:
        for names in CHAINS:
            for aica in (True, False):
                _, ref, t32 = chain_refs(shape, names, aica)
                for grp, e in (("chain_fwd", fr.rel_err(t32[0], ref[0])), ("chain_dx", fr.rel_err(t32[1], ref[1])),
                               ("chain_dparams", max(fr.rel_err(t32[2][:, :6], ref[2][:, :6]) if set(names) - {"T"} else 0.0,
                                                     fr.rel_err(t32[3], ref[3]) if "T" in names else 0.0))):
                    E[grp] = E[grp + "_fast"] = max(E[grp], e)
    return E


def bounds_from(E):
    return {k: min(round_up_1sig(4 * v), FWD_CEILING if "fwd" in k else GRAD_CEILING) for k, v in E.items()}


if __name__ == "__main__":
    E = measure_E()
    Bd = bounds_from(E)
    print(f"{'group':<22}{'E (torch f32)':>16}{'4 E':>12}{'bound':>10}")
    for k in GROUPS:
        print(f"{k:<22}{E[k]:>16.3e}{4 * E[k]:>12.3e}{Bd[k]:>10.0e}")
