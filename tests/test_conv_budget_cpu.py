"""The element-wise conv budgets of conv_budget_ref.py have teeth: an f32-accumulate, round-to-dtype emulation of the four
results on the CPU (blocked summation orders: 16-channel K-steps, one slab per image) is inside the budget on every element,
and each single-term mutant of that emulation is over it on more than a quarter of the elements it touches.  These are
mutations of reference arithmetic; no kernel runs here."""
import pytest
import torch
import torch.nn.functional as F

import conv_budget_ref as R

# the shape of the issue's worked example (M = 51,200 pixels), a ragged 1x1 and a stride-2 shape with odd extents
SHAPES = [(8, 64, 64, 80, 80, 3, 1, 1), (2, 24, 16, 9, 7, 1, 1, 0), (2, 16, 32, 13, 21, 3, 2, 1)]
CASES = [(n, s) for n in ("bf16", "f16") for s in SHAPES]
_cache = {}


def _setup(name, shape, which=("z", "dx", "dw", "db")):
    """Rounded operands (f32 tensors holding dtype values), the fp64 references and the honest emulation's f32 accumulators,
    computed once per case and shared (nothing below writes to them)."""
    key = (name, shape, which)
    if key not in _cache:
        dtype = R.DTYPES[name]
        B, Cin, Cout, H, W, kh, kw, s, p, d, Ho, Wo = R.geometry(shape)
        x, w, bias, gy = R.make_operands(shape, dtype, "cpu")
        x, w, gy = x.to(dtype).float(), w.to(dtype).float(), gy.to(dtype).float()
        _cache[key] = dict(dtype=dtype, x=x, w=w, bias=bias, gy=gy, geo=(s, p, d), refs=R.conv_refs(x, w, gy, bias, s, p, d, which))
    return _cache[key]


def _z_acc(x, w, bias, geo):
    """f32 accumulators of the forward, summed over 16-channel K-steps"""
    acc = None
    for c0 in range(0, x.shape[1], 16):
        part = F.conv2d(x[:, c0:c0 + 16], w[:, c0:c0 + 16], None, *geo)
        acc = part if acc is None else acc + part
    return acc + bias.view(1, -1, 1, 1)


def _dx_acc(x, w, gy, geo):
    acc = None
    for c0 in range(0, w.shape[0], 16):
        part = torch.nn.grad.conv2d_input(x.shape, w[c0:c0 + 16], gy[:, c0:c0 + 16], *geo)
        acc = part if acc is None else acc + part
    return acc


def _dw_acc(x, w, gy, geo):
    """f32 weight gradient as split slabs: one partial per image, added in a fixed order"""
    acc = None
    for n in range(x.shape[0]):
        part = torch.nn.grad.conv2d_weight(x[n:n + 1], w.shape, gy[n:n + 1], *geo)
        acc = part if acc is None else acc + part
    return acc


def _db_acc(gy):
    acc = None
    for n in range(gy.shape[0]):
        part = gy[n].sum((1, 2))
        acc = part if acc is None else acc + part
    return acc


def _check(name, got, c, shape, out_dtype):
    ref, S = c["refs"][name]
    return R.compare(name, got, ref, S, R.C_OF[name], out_dtype, R.terms(name, shape))


def _over_on(name, got, c, out_dtype, touched):
    """share of the `touched` elements of a mutant that are over budget"""
    ref, S = c["refs"][name]
    b = R.budget(ref, S, R.C_OF[name], out_dtype)
    over = ((got.double() - ref).abs() > b) & touched
    return float(over.sum()) / max(int(touched.sum()), 1)


@pytest.mark.parametrize("name,shape", CASES, ids=[n + ":" + "x".join(map(str, s)) for n, s in CASES])
def test_honest_emulation_is_within_budget(name, shape):
    c = _setup(name, shape)
    dt = c["dtype"]
    got = {"z": _z_acc(c["x"], c["w"], c["bias"], c["geo"]).to(dt), "dx": _dx_acc(c["x"], c["w"], c["gy"], c["geo"]).to(dt),
           "dw": _dw_acc(c["x"], c["w"], c["gy"], c["geo"]), "db": _db_acc(c["gy"])}
    for k, v in got.items():
        r = _check(k, v, c, shape, dt if k in ("z", "dx") else torch.float32)
        print(name, shape, r)
        assert r.worst <= 1.0, str(r)


def _flat_pixels(gy):
    B, C, Ho, Wo = gy.shape
    return gy.permute(0, 2, 3, 1).reshape(B * Ho * Wo, C)


def _unflat(flat, like):
    B, C, Ho, Wo = like.shape
    return flat.reshape(B, Ho, Wo, C).permute(0, 3, 1, 2).contiguous()


def _dw_reach(c, delta):
    """weight-gradient elements that the pixels where `delta` (a dz-shaped tensor) is non-zero contribute to"""
    return torch.nn.grad.conv2d_weight(c["x"].abs().double(), c["w"].shape, delta.abs().double(), *c["geo"]) > 0


@pytest.mark.parametrize("name,shape", CASES, ids=[n + ":" + "x".join(map(str, s)) for n, s in CASES])
def test_mutants_are_over_budget(name, shape):
    c = _setup(name, shape)
    dt = c["dtype"]
    x, w, bias, gy, geo = c["x"], c["w"], c["bias"], c["gy"], c["geo"]
    s, p, d = geo
    B, Cout, Ho, Wo = gy.shape
    shares = {}
    # (1) one pixel removed from the dW sum
    m = gy.clone()
    m[B // 2, :, Ho // 2, Wo // 2] = 0
    shares["dw, one pixel removed"] = _over_on("dw", _dw_acc(x, w, m, geo), c, torch.float32, _dw_reach(c, gy - m))
    # (2) one input channel of one tap removed from z on the last output column (tap row `p` / column 0: inside the image)
    ci, th, tw = x.shape[1] - 1, min(p, w.shape[2] - 1), 0
    ih = torch.arange(Ho) * s - p + th * d
    iw = (Wo - 1) * s - p + tw * d
    assert 0 <= iw < x.shape[3] and int(ih.min()) >= 0 and int(ih.max()) < x.shape[2]
    acc = _z_acc(x, w, bias, geo)
    acc[:, :, :, Wo - 1] -= x[:, ci, ih, iw].unsqueeze(1) * w[:, ci, th, tw].view(1, -1, 1)
    touched = torch.zeros_like(acc, dtype=torch.bool)
    touched[:, :, :, Wo - 1] = True
    shares["z, one channel of one tap removed on the last column"] = _over_on("z", acc.to(dt), c, dt, touched)
    # (3) the last 16 pixels counted twice in dW
    flat = _flat_pixels(gy).clone()
    flat[-16:] *= 2
    m = _unflat(flat, gy)
    shares["dw, last 16 pixels twice"] = _over_on("dw", _dw_acc(x, w, m, geo), c, torch.float32, _dw_reach(c, m - gy))
    # (4) one pixel row missing from db
    m = gy.clone()
    m[B - 1, :, Ho - 1, :] = 0
    shares["db, one pixel row missing"] = _over_on("db", _db_acc(m), c, torch.float32, torch.ones(Cout, dtype=torch.bool))
    print(name, shape, {k: f"{v:.0%}" for k, v in shares.items()})
    for k, v in shares.items():
        assert v > 0.25, (k, v)


# the GPU cases whose dW power margin is below 4 (M from 128,000 pixels up: ONE dropped pixel is inside the budget there)
WEAK_DW = [("bf16", (7, 128, 64, 197, 191, 1, 1, 0)), ("f16", (2, 64, 64, 320, 320, 3, 1, 1)), ("bf16", (24, 124, 64, 80, 72, 3, 1, 1)),
           ("f16", (24, 128, 128, 80, 72, 3, 1, 1)), ("bf16", (6, 60, 62, 150, 147, 3, 1, 1)), ("bf16", (5, 64, 128, 320, 320, 3, 2, 1))]


@pytest.mark.parametrize("name,shape", WEAK_DW, ids=[n + ":" + "x".join(map(str, s)) for n, s in WEAK_DW])
def test_weak_weight_gradient_cases_still_catch_a_pixel_tail(name, shape):
    """What the weak dW cases do catch: dropping the ragged tail past the last whole 32-pixel step (29 pixels at M = 263,389),
    or the last 32 pixels where M is a multiple of 32, is over budget on more than a quarter of the dW elements those pixels
    reach; the honest emulation stays inside and its power margin is indeed below 4."""
    c = _setup(name, shape, ("dw",))
    B, Cout, Ho, Wo = c["gy"].shape
    tail = (B * Ho * Wo) % 32 or 32
    flat = _flat_pixels(c["gy"]).clone()
    flat[-tail:] = 0
    m = _unflat(flat, c["gy"])
    share = _over_on("dw", _dw_acc(c["x"], c["w"], m, c["geo"]), c, torch.float32, _dw_reach(c, c["gy"] - m))
    rep = _check("dw", _dw_acc(c["x"], c["w"], c["gy"], c["geo"]), c, shape, torch.float32)
    print(name, shape, rep, f"; {tail}-pixel tail dropped: {share:.0%} over budget")
    assert rep.worst <= 1.0 and rep.margin < 4
    assert share > 0.25, share


def test_constants_are_eight_times_the_measurement():
    assert (R.C_FWD, R.C_DGRAD, R.C_WGRAD, R.C_BGRAD) == (8 * R.MEASURED_FWD, 8 * R.MEASURED_DGRAD, 8 * R.MEASURED_WGRAD, 8 * R.MEASURED_BGRAD)
    assert min(R.C_OF.values()) > 0


def test_case_list_names_every_snapshot_symbol():
    """Per entry and dtype, the symbols the budget cases are listed under are the ones golden/g22_conv_routes.json holds (the
    GPU module asserts each); the cases the snapshot cannot key add the stem forward and pixel-streaming kernels."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_conv_routes.json")) as f:
        want, have, unkeyed = R.snapshot_coverage(json.load(f))
    assert have - unkeyed == want, (sorted(want - have), sorted(have - unkeyed - want))
    assert len(unkeyed) == 6, unkeyed
