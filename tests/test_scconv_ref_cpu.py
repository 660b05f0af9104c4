"""CPU: ties the float64 references of tests/scconv_ref.py to recorded results and to autograd, and checks the input laws of the
GPU cases of tests/test_gpu_scconv_asff_kernels.py on the reference alone.

  * composed with f64 convolutions the references reproduce the reference project's SCConv and ASFF blocks (tests/golden/g2_scconv,
    g2_asff0, g2_asff2_0) at the bounds of tests/test_oracle_golden.py (1e-4 forward, 1e-3 input gradients);
  * the hand formulas (red, ds, dlogits, dx from red, dout) equal f64 autograd to 1e-12;
  * every SRU case keeps its gate-ambiguous share under the cap, |sum gamma| >= 0.5 with both signs present over the cases, both
    mask values in both channel halves, and a gate margin no f32 evaluation can cross on every unambiguous element.
"""
import pytest
import torch
import torch.nn.functional as F

import scconv_ref as sr
from oracle import model as om
from util import close, gold, rnd

F64 = torch.float64


def _shapes(spec):
    spec = dict(i=0, **spec)
    return {k[len("model.0."):]: v for k, v in om.param_shapes([spec]).items()}


def _sd64(shapes, seed):
    sd = om.rng_fill(shapes, seed)
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _rows(t):                                    # [N, C, H, W] -> [N, HW, C]
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1])


def _nchw(t, H, W):                              # [N, HW, C] -> [N, C, H, W]
    return t.reshape(t.shape[0], H, W, t.shape[2]).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------- composition vs the goldens
def test_references_compose_to_the_scconv_golden():
    g = gold("g2_scconv")
    sd = _sd64(_shapes(dict(kind="SCConv", c=64)), int(g["seed"]))
    x = g["x0"].double().requires_grad_(True)
    N, C, H, W = x.shape
    h = C // 2
    y, _, _ = sr.sru_ref(_rows(x), sd["SRU.gn.weight"].flatten(), sd["SRU.gn.bias"].flatten(), 4, 1e-10)
    y = _nchw(y, H, W)
    up = F.conv2d(y[:, :h], sd["CRU.squeeze1.weight"])
    low = F.conv2d(y[:, h:], sd["CRU.squeeze2.weight"])
    y1 = F.conv2d(up, sd["CRU.GWC.weight"], sd["CRU.GWC.bias"], 1, 1, 1, 2) + F.conv2d(up, sd["CRU.PWC1.weight"])
    o = torch.cat((y1, F.conv2d(low, sd["CRU.PWC2.weight"]), low), 1)
    s_from_moments = torch.softmax(sr.moments_ref(_rows(o))[..., 0] / (H * W), -1)
    res, s = sr.cru_fuse_ref(_rows(o))
    close(s, s_from_moments, 1e-12, 1e-15, "pooled softmax from moments_ref")
    out = _nchw(res, H, W)
    close(out, g["y0"], 1e-4, 1e-4, "scconv y0")
    (out * rnd(900, *out.shape, lo=-1, hi=1)).sum().backward()
    close(x.grad, g["dx0"], 1e-3, 1e-3, "scconv dx0")


def _asff_block(name, spec, nin, prepare):
    g = gold(name)
    sd = _sd64(_shapes(spec), int(g["seed"]))
    xs = [g[f"x{i}"].double().requires_grad_(True) for i in range(nin)]
    rs = prepare(sd, xs)
    w = torch.cat([om.conv_bn_leaky(sd, f"weight_level_{j}.", r, 1, 1, True) for j, r in enumerate(rs)], 1)
    logits = F.conv2d(w, sd["weight_levels.weight"], sd["weight_levels.bias"])
    H, W = logits.shape[2:]
    fused, _ = sr.asff_ref([_rows(r).flatten(0, 1) for r in rs], _rows(logits).flatten(0, 1))
    fused = _nchw(fused.reshape(logits.shape[0], H * W, -1), H, W)
    y = om.conv_bn_leaky(sd, "expand.", fused, 3, 1, True)
    close(y, g["y0"], 1e-4, 1e-4, f"{name} y0")
    (y * rnd(900, *y.shape, lo=-1, hi=1)).sum().backward()
    for i, x in enumerate(xs):
        close(x.grad, g[f"dx{i}"], 1e-3, 1e-3, f"{name} dx{i}")


def test_asff_reference_composes_to_the_three_level_golden():
    def prepare(sd, xs):
        x0, x1, x2 = xs
        return x0, F.max_pool2d(x1, 2, 2), om.conv_bn_leaky(sd, "stride_level_2.", F.max_pool2d(x2, 3, 2, 1), 3, 2, True)
    _asff_block("g2_asff0", dict(kind="AsffTribeLevel", level=0), 3, prepare)


def test_asff_reference_composes_to_the_two_level_golden():
    def prepare(sd, xs):
        return xs[0], om.conv_bn_leaky(sd, "stride_level_1.", xs[1], 3, 2, True)
    _asff_block("g2_asff2_0", dict(kind="AsffDoubLevel", level=0), 2, prepare)


# --------------------------------------------------------------------------------------------------- hand formulas vs autograd
def _close12(a, b, what):
    a, b = a.detach().double(), b.detach().double()
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert err <= 1e-12, f"{what}: {err:.2e}"


@pytest.mark.parametrize("name", ["golden_shape", "c48", "g64", "neg_wsum", "zero_channel"])
def test_sru_reduced_sums_and_dx_formula_match_autograd(name):
    c = sr.sru_case(name, "f32")
    gamma = c["gamma"].double().requires_grad_(True)
    beta = c["beta"].double().requires_grad_(True)
    x = c["x"].double().requires_grad_(True)
    y, _, _ = sr.sru_ref(x, gamma, beta, c["G"], c["eps"])
    (y * c["dy"].double()).sum().backward()
    dx, red, _ = sr.sru_bwd_ref(c["x"], c["dy"], c["gamma"], c["beta"], c["G"], c["eps"])
    _close12(dx, x.grad, "dx")
    # d gamma has a second path through the gate weight gamma / sum(gamma), but the gate is piecewise constant: no gradient
    _close12(red.sum(0)[:, 0], beta.grad, "d beta = sum_n red0")
    _close12(red.sum(0)[:, 1], gamma.grad, "d gamma = sum_n red1")
    zero = torch.zeros_like(c["red_prior"])
    dx2, _, _ = sr.sru_bwd_ref(c["x"], c["dy"], c["gamma"], c["beta"], c["G"], c["eps"], prior=zero)
    _close12(dx2, x.grad, "dx from red")


def test_sru_constant_group_is_finite_and_matches_autograd_elsewhere():
    c = sr.sru_case("const_group", "f32")
    dx, red, _ = sr.sru_bwd_ref(c["x"], c["dy"], c["gamma"], c["beta"], c["G"], c["eps"])
    dx2, _, _ = sr.sru_bwd_ref(c["x"], c["dy"], c["gamma"], c["beta"], c["G"], c["eps"], prior=torch.zeros_like(c["red_prior"]))
    assert torch.isfinite(dx).all() and torch.isfinite(red).all()
    _close12(dx2, dx, "dx from red, constant group")
    cpg = c["C"] // c["G"]
    y, gn, _ = sr.sru_ref(c["x"], c["gamma"], c["beta"], c["G"], c["eps"])
    assert torch.equal(gn[0, :, cpg:2 * cpg], c["beta"].double()[cpg:2 * cpg].expand(c["HW"], cpg)), "xhat == 0 in the constant group"


@pytest.mark.parametrize("name", ["c16", "c48", "offsets", "equal_means"])
def test_cru_ds_and_dout_formula_match_autograd(name):
    c = sr.cru_case(name, "f32")
    o = c["o"].double().requires_grad_(True)
    res, s = sr.cru_fuse_ref(o)
    assert torch.isfinite(res).all()
    (res * c["dres"].double()).sum().backward()
    dout, ds, _ = sr.cru_fuse_bwd_ref(c["o"], c["dres"])
    _close12(dout, o.grad, "dout")
    sl = s.detach().requires_grad_(True)                            # ds = d loss / d s at fixed o
    w = c["o"].double() * sl[:, None, :]
    ((w[..., :c["C"]] + w[..., c["C"]:]) * c["dres"].double()).sum().backward()
    _close12(ds, sl.grad, "ds")


@pytest.mark.parametrize("nsrc", [3, 2])
@pytest.mark.parametrize("kind", sr.ASFF_LOGIT_KINDS)
def test_asff_gradients_match_autograd(nsrc, kind):
    c = sr.asff_case("c128", nsrc, 4, kind, "f32")
    xs = [x.double().requires_grad_(True) for x in c["xs"]]
    lg = c["logits"].double().requires_grad_(True)
    out, w = sr.asff_ref(xs, lg)
    assert torch.isfinite(out).all()
    (out * c["dout"].double()).sum().backward()
    dxs, dlog = sr.asff_bwd_ref(c["xs"], c["logits"], c["dout"])
    for k in range(nsrc):
        _close12(dxs[k], xs[k].grad, f"dx{k}")
    _close12(dlog, lg.grad[:, :nsrc], "dlogits")
    assert bool((lg.grad[:, nsrc:] == 0).all())
    # the blend as the oracle writes it (oracle/model.py asff / asff2 / mfru), on the same tensors
    ws = F.softmax(c["logits"].double()[:, :nsrc], dim=1)
    fused = sum(c["xs"][k].double() * ws[:, k:k + 1] for k in range(nsrc))
    _close12(out, fused, "blend")


def test_asff_special_rows_are_what_they_claim():
    c = sr.asff_case("p3", 3, 4, "offset", "f32")
    _, w = sr.asff_ref(c["xs"], c["logits"])
    assert float(c["logits"][:, :3].min()) > 900
    assert float(w[1].max()) == 1.0 and 0 < float(w[1].min()) < 1e-30 and torch.equal(w[2], torch.full((3,), 1 / 3, dtype=F64))
    for dt in ("bf16", "f16"):
        lg = sr.asff_case("p3", 2, 2, "offset", dt)["logits"]
        assert torch.equal(lg.to(sr.DT[dt]).float(), lg), "logits exactly representable"


# ------------------------------------------------------------------------------------------------ input laws of the GPU cases
@pytest.mark.parametrize("name,dt", [(n, dt) for n, v in sr.SRU_CASES.items() for dt in v[4]])
def test_sru_cases_meet_the_input_law(name, dt):
    c = sr.sru_case(name, dt)
    f = sr.check_sru_law(c)
    print(f"LAW sru {name} {dt}: seed {c['seed']} share {f['share']:.2e} ({f['n_ambiguous']} ambiguous) sum gamma {f['wsum']:.3f} "
          f"margin {f['margin']:.2e}")
    assert f["share"] <= sr.SHARE_CAP and abs(f["wsum"]) >= 0.5
    for k in ("x", "dy"):
        assert torch.equal(c[k].to(sr.DT[dt]).float(), c[k]), f"{k} exactly representable in {dt}"


def test_sru_cases_cover_both_signs_of_sum_gamma():
    signs = {name: float(sr.sru_case(name, "f32")["gamma"].double().sum()) for name in sr.SRU_CASES}
    assert min(signs.values()) <= -0.5 and max(signs.values()) >= 0.5, signs


def test_sru_special_cases_are_what_they_claim():
    c = sr.sru_case("zero_channel", "f32")
    _, gn, t = sr.sru_ref(c["x"], c["gamma"], c["beta"], c["G"], c["eps"])
    for ch in sr.ZERO_CHANNELS:
        assert bool((gn[..., ch] == 0).all()) and bool((t[..., ch] == 0).all())
    c = sr.sru_case("const_group", "f32")
    cpg = c["C"] // c["G"]
    _, sd = sr.group_norm(c["x"].double(), c["G"], c["eps"])
    assert float(sd[0, 1]) == 0.0 and float(sd[0, 0]) > 0 and float(sd[1, 1]) > 0
    m = sr.moments_ref(c["x"])[0, cpg:2 * cpg]
    cnt = cpg * c["HW"]
    assert float(m[:, 0].sum()) == 1.5 * cnt and float(m[:, 1].sum()) == 2.25 * cnt       # the kernel's var is exactly 0 too


def test_cru_special_cases_are_what_they_claim():
    c = sr.cru_case("offsets", "f32")
    means = c["o"].double().mean(1)
    assert float(means.max()) > 95 and float(torch.exp(means).max()) > 1e38            # exp without max-subtraction overflows f32
    res, s = sr.cru_fuse_ref(c["o"])
    assert torch.isfinite(res).all() and torch.isfinite(s).all()
    for dt in ("f32", "bf16", "f16"):
        e = sr.cru_case("equal_means", dt)
        assert bool((sr.moments_ref(e["o"])[..., 0] == 0).all())
        assert torch.equal(sr.cru_fuse_ref(e["o"])[1], torch.full((e["N"], 2 * e["C"]), 1.0 / (2 * e["C"]), dtype=F64))


def test_sixteen_bit_cases_are_exactly_representable():
    for dt in ("bf16", "f16"):
        for name, v in sr.MOMENT_CASES.items():
            if dt in v[3]:
                x = sr.moments_case(name, dt)["x"]
                assert torch.equal(x.to(sr.DT[dt]).float(), x)
        for name, v in sr.CRU_CASES.items():
            if dt in v[2]:
                c = sr.cru_case(name, dt)
                assert torch.equal(c["o"].to(sr.DT[dt]).float(), c["o"]) and torch.equal(c["dres"].to(sr.DT[dt]).float(), c["dres"])
        c = sr.asff_case("v66", 3, 4, "offset", dt)
        for t in c["xs"] + c["priors"] + [c["logits"], c["dout"]]:
            assert torch.equal(t.to(sr.DT[dt]).float(), t)
