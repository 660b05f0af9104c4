"""GPU tests of csrc/bn2act.hip through the C-ABI in fp32, bf16 and fp16 against the float64 statement tests/repc3_ref.py computed
from the same (rounded) inputs: dy_bn2_act_fwd and dy_bn2_act_bwd, each with SiLU, no activation and LeakyReLU(0.1).

Views: u, dy and du are C-channel slices at channel 8 of [pixels, C + 16] buffers, v, y and dv of [pixels, C + 8] buffers, all
filled with a sentinel; every element outside a written slice and every input must be unchanged after every call.  The f32 outputs
(dgamma, dbeta, workspace) carry a sentinel tail.

Shapes: pixels in {1, 7, 64, 257, 4100} (one pixel: variance 0; below one wave; not a multiple of any tile; more pixels than one
workgroup walks) x C in {8, 24, 72, 264} (one vector in the 16-bit types; three vectors; nine; 33 vectors in bf16 and 66 in f32,
so pixels share a workgroup unevenly), plus 4 and 12 in f32.  scale / shift / mean / invstd are what dy_bn_finalize_valid would
give for u and v (eps 1e-3), rounded to f32; the reference reads the same f32 values.  One case per dtype has branches that
nearly cancel, so the measure's denominator (the magnitudes of the terms, not of the result) matters.

LeakyReLU: act' jumps at z = 0, so an element whose z the kernel rounds to the other side would be off by 0.9 |dy|.  No element is
left out of a comparison; instead the inputs of every LeakyReLU case are moved away from the kink on the host (v is nudged where
|z| < 2e-3; seeds alone cannot do it: at 4100 x 264 about 500 elements land within 1e-3 of 0 for any seed) and the test asserts
that the float64 reference has no |z| < 1e-3 before it compares.

Error measure: |got - ref64| / sum |terms| (tests/test_gpu_layernorm.py's; the terms are repc3_ref's *_terms).  Rule: 2e-6 for f32
outputs, the same plus one ulp of the type at the reference value for 16-bit outputs.  E is the error in the same measure of
repc3_ref's formula run by torch on the CPU in f32 on the same rounded inputs (16-bit modes: outputs rounded to the type); the
kernel is allowed max(rule, 4 E).  Every case prints its measured error / allowance.  Every backward runs twice: identical bytes.
With v = 0 and scale_v = shift_v = 0 the stage is the single-branch one: y and du equal dy_bn_act_fwd / dy_bn_act_bwd_valid's
within the same allowance.
"""
import zlib

import numpy as np
import pytest
import torch

import repc3_ref as rr
from frontend_ref import ulp

pytestmark = pytest.mark.gpu

RULE = 2e-6
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ACTS = {"silu": rr.ACT_SILU, "none": rr.ACT_NONE, "leaky": rr.ACT_LEAKY}
SENTINEL = 99.0
C0 = 8
CASES = [(px, C, dt) for px in (1, 7, 64, 257, 4100) for C in (8, 24, 72, 264) for dt in DT] + \
        [(px, C, "f32") for px in (1, 7, 64, 257, 4100) for C in (4, 12)]


class Slice:
    """C channels at channel 8 of a [pixels, ld] sentinel-filled parent, ld = C + 16 or C + 8"""

    def __init__(self, rows, C, dtype, ld, fill=None):
        assert ld in (C + 16, C + 8)
        self.C, self.ld = C, ld
        self.parent = torch.full((rows, ld), SENTINEL, device="cuda", dtype=dtype)
        if fill is not None:
            self.parent[:, C0:C0 + C] = fill.reshape(rows, C).to(dtype).cuda()
        self.before = self.parent.clone()

    @property
    def ptr(self):
        return self.parent.data_ptr() + C0 * self.parent.element_size()

    def get(self):
        return self.parent[:, C0:C0 + self.C].double().cpu()

    def guards_intact(self, what):
        p = self.parent
        assert bool((p[:, :C0] == SENTINEL).all()) and bool((p[:, C0 + self.C:] == SENTINEL).all()), f"{what}: wrote outside its slice"

    def unchanged(self, what):
        assert torch.equal(self.parent, self.before), f"{what}: an input changed"


def _tail(n):
    return torch.full((n + 16,), SENTINEL, device="cuda", dtype=torch.float32)


def _call(name, *args):
    from dedark_yolo_amd import _C, ops
    _C.call(name, *args, ops.stream())


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _rn(g, dt, *shape, scale=1.0, shift=0.0):
    return torch.from_numpy((shift + scale * g.standard_normal(shape)).astype(np.float32)).to(DT[dt]).float()


def _measure(got, ref, terms, dt):
    got, ref, terms = (torch.as_tensor(t).double().cpu() for t in (got, ref, terms))
    assert got.shape == ref.shape == terms.shape, (got.shape, ref.shape, terms.shape)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    if dt == "f32":
        return float(((got - ref).abs() / terms.clamp_min(1e-300)).max())
    return float(((got - ref).abs() / (RULE * terms + ulp(ref, DT[dt]))).max())


def _check(what, got, ref, terms, emu, dt, figs):
    rule = RULE if dt == "f32" else 1.0
    e, E = _measure(got, ref, terms, dt), _measure(emu, ref, terms, dt)
    bound = max(rule, 4 * E)
    print(f"FIG {what}: err {e:.3e} bound {bound:.3e} (rule {rule:.0e}, E {E:.3e}) ratio {e / bound:.3f}")
    figs.append((what, e, bound))


def _report(figs):
    bad = [f"{w}: {e:.3e} > {b:.3e}" for w, e, b in figs if not e <= b]
    assert not bad, "; ".join(bad)


def _branch(x, gamma, beta):
    """(scale, shift, mean, invstd, gamma) as f32 values: what dy_bn_finalize_valid hands the stage for the raw map x"""
    return tuple(t.float() for t in (*rr.bn_stats(x, gamma, beta), gamma))


def _z64(u, v, bu, bv):
    return u.double() * bu[0].double() + bu[1].double() + v.double() * bv[0].double() + bv[1].double()


def _off_the_kink(u, v, bu, bv, dt):
    """v with the elements whose z lies within 2e-3 of LeakyReLU's kink moved away from it (the statistics stay as given)"""
    v = v.clone()
    for _ in range(40):
        z = _z64(u, v, bu, bv)
        bad = z.abs() < 2e-3
        if not bool(bad.any()):
            break
        step = (4e-3 / bv[0].double().abs()).expand_as(z)
        if dt != "f32":
            step = torch.maximum(step, 2 * ulp(v.double(), DT[dt]))
        sgn = torch.where(z >= 0, 1.0, -1.0) * torch.sign(bv[0].double())
        v = torch.where(bad, (v.double() + sgn * step).float().to(DT[dt]).float(), v)
    return v


def _inputs(px, C, dt, code, key, cancel=False):
    g = _rng(key, px, C, dt, code)
    gu, gv = _rn(g, "f32", C, shift=1.0, scale=0.3), _rn(g, "f32", C, shift=1.0, scale=0.3)
    beu, bev = _rn(g, "f32", C, scale=0.3), _rn(g, "f32", C, scale=0.3)
    u = _rn(g, dt, px, C, scale=1.5, shift=0.3)
    dy = _rn(g, dt, px, C)
    if not cancel:
        v = _rn(g, dt, px, C, scale=0.7, shift=-0.2)
        bu, bv = _branch(u, gu, beu), _branch(v, gv, bev)
    else:                                    # scale_u u + shift_u ~ -(scale_v v + shift_v): z is 0.01 N of terms of magnitude ~2
        bu = _branch(u, gu, beu)
        sv, hv = gv, bev                     # any scale / shift: v is solved for them, then given statistics that reproduce them
        v = ((-(u * bu[0] + bu[1]) - hv + 0.01 * _rn(g, "f32", px, C)) / sv).to(DT[dt]).float()
        mean = v.double().mean(0)
        invstd = 1.0 / torch.sqrt(((v.double() - mean) ** 2).mean(0) + rr.BN_EPS)
        bv = (sv, hv, mean.float(), invstd.float(), (sv.double() / invstd).float())
    if code == rr.ACT_LEAKY:
        v = _off_the_kink(u, v, bu, bv, dt)
        assert float(_z64(u, v, bu, bv).abs().min()) >= 1e-3, "LeakyReLU case: an element sits on the kink"
    return u, v, dy, bu, bv


def _round(t, dt):
    return t if dt == "f32" else t.to(DT[dt]).float()


def _dev(vecs):
    return [t.contiguous().cuda() for t in vecs]


def _stage_case(tag, px, C, dt, code, u, v, dy, bu, bv, figs):
    """one forward and two backward runs of one operand set; appends the figures; returns (y, du) as float64"""
    from dedark_yolo_amd import ops
    dtype, did = DT[dt], ops.dt_id(DT[dt])
    uv, vv, dyv = Slice(px, C, dtype, C + 16, u), Slice(px, C, dtype, C + 8, v), Slice(px, C, dtype, C + 16, dy)
    yv = Slice(px, C, dtype, C + 8)
    du_, dv_ = _dev(bu), _dev(bv)                                   # scale, shift, mean, invstd, gamma of each branch
    _call("dy_bn2_act_fwd", uv.ptr, uv.ld, vv.ptr, vv.ld, du_[0].data_ptr(), du_[1].data_ptr(), dv_[0].data_ptr(), dv_[1].data_ptr(), code,
          yv.ptr, yv.ld, px, C, did)
    torch.cuda.synchronize()
    uv.unchanged(tag + " fwd u")
    vv.unchanged(tag + " fwd v")
    yv.guards_intact(tag + " fwd y")
    fa = (u, v, bu[0], bu[1], bv[0], bv[1], code)
    _check(tag + " y", yv.get(), rr.bn2_forward(*fa), rr.bn2_forward_terms(*fa), _round(rr.bn2_forward(*fa, dt=torch.float32), dt), dt, figs)

    n_ws = ops.bn2_act_bwd_workspace(px, C, dtype)
    assert 6 * C <= n_ws <= 3 * C * 1025
    runs = []
    for _ in range(2):
        duv, dvv = Slice(px, C, dtype, C + 16), Slice(px, C, dtype, C + 8)
        outs = [_tail(C) for _ in range(4)]                             # dgamma_u, dbeta_u, dgamma_v, dbeta_v
        ws = _tail(n_ws)
        _call("dy_bn2_act_bwd", dyv.ptr, dyv.ld, uv.ptr, uv.ld, vv.ptr, vv.ld, *(t.data_ptr() for t in du_), *(t.data_ptr() for t in dv_), code,
              duv.ptr, duv.ld, dvv.ptr, dvv.ld, *(t.data_ptr() for t in outs), ws.data_ptr(), n_ws, px, C, did)
        torch.cuda.synchronize()
        duv.guards_intact(tag + " bwd du")
        dvv.guards_intact(tag + " bwd dv")
        for t, n in [(o, C) for o in outs] + [(ws, n_ws)]:
            assert bool((t[n:] == SENTINEL).all()), f"{tag}: an f32 output was written past its end"
        runs.append((duv, dvv, *outs))
    for s in (uv, vv, dyv):
        s.unchanged(tag + " bwd")
    for x0, x1 in zip(runs[0], runs[1]):
        x0, x1 = (getattr(t, "parent", t) for t in (x0, x1))
        assert torch.equal(x0.view(torch.uint8), x1.view(torch.uint8)), f"{tag}: two backward runs differ"
    ba = (dy, u, v, bu, bv, code)
    ref, terms, emu = rr.bn2_backward(*ba), rr.bn2_backward_terms(*ba), rr.bn2_backward(*ba, dt=torch.float32)
    duv, dvv, dgu, dbu, dgv, dbv = runs[0]
    assert torch.equal(dbu[:C], dbv[:C])                                # the sum of g is shared
    _check(tag + " du", duv.get(), ref[0], terms[0], _round(emu[0], dt), dt, figs)
    _check(tag + " dv", dvv.get(), ref[1], terms[1], _round(emu[1], dt), dt, figs)
    for name, got, i in (("dgamma_u", dgu, 2), ("dbeta", dbu, 3), ("dgamma_v", dgv, 4)):
        _check(f"{tag} {name}", got[:C].double().cpu(), ref[i], terms[i], emu[i], "f32", figs)
    return yv.get(), duv.get()


@pytest.mark.parametrize("px,C,dt", CASES)
def test_bn2_act_kernels(px, C, dt):
    figs = []
    for name, code in ACTS.items():
        u, v, dy, bu, bv = _inputs(px, C, dt, code, "bn2")
        _stage_case(f"px={px} C={C} {dt} {name}", px, C, dt, code, u, v, dy, bu, bv, figs)
    _report(figs)


@pytest.mark.parametrize("dt", list(DT))
def test_bn2_act_cancelling_branches(dt):
    """scale_u u + shift_u ~ -(scale_v v + shift_v): |z| ~ 0.01 from terms of magnitude ~2"""
    px, C = 257, 72
    figs = []
    for name, code in ACTS.items():
        u, v, dy, bu, bv = _inputs(px, C, dt, code, "cancel", cancel=True)
        z, tz = _z64(u, v, bu, bv), (u * bu[0]).abs() + bu[1].abs() + (v * bv[0]).abs() + bv[1].abs()
        assert float((z.abs() / tz.double()).median()) < 0.02          # the branches do cancel
        _stage_case(f"cancel {dt} {name}", px, C, dt, code, u, v, dy, bu, bv, figs)
    _report(figs)


@pytest.mark.parametrize("dt", list(DT))
def test_bn2_act_fp16_style_scaled_gradient(dt):
    """a gradient that arrives multiplied by a loss scale of 1024: the stage is linear in dy"""
    px, C = 64, 24
    figs = []
    u, v, dy, bu, bv = _inputs(px, C, dt, rr.ACT_SILU, "scaled")
    _stage_case(f"scaled {dt}", px, C, dt, rr.ACT_SILU, u, v, dy * 1024.0, bu, bv, figs)
    _report(figs)


@pytest.mark.parametrize("px,C", [(257, 72), (4100, 24)])
@pytest.mark.parametrize("dt", list(DT))
def test_one_branch_equals_the_single_branch_kernels(px, C, dt):
    """v = 0, scale_v = shift_v = 0: y and du are dy_bn_act_fwd's / dy_bn_act_bwd_valid's within the allowance against float64"""
    from dedark_yolo_amd import _C, ops
    dtype, did = DT[dt], ops.dt_id(DT[dt])
    figs = []
    for name, code in ACTS.items():
        u, _, dy, bu, _ = _inputs(px, C, dt, code, "one")
        zero = torch.zeros(C)
        v, bv = torch.zeros(px, C), (zero, zero, zero, zero, torch.ones(C))
        if code == rr.ACT_LEAKY:             # the kink again, by moving u: v is pinned to 0 here
            for _ in range(40):
                bad = _z64(u, v, bu, bv).abs() < 2e-3
                if not bool(bad.any()):
                    break
                u = torch.where(bad, (u + 0.0625).to(dtype).float(), u)
            assert float(_z64(u, v, bu, bv).abs().min()) >= 1e-3
        tag = f"one-branch px={px} C={C} {dt} {name}"
        y_new, du_new = _stage_case(tag, px, C, dt, code, u, v, dy, bu, bv, figs)
        uv, dyv = Slice(px, C, dtype, C + 16, u), Slice(px, C, dtype, C + 16, dy)
        yv, dzv = Slice(px, C, dtype, C + 8), Slice(px, C, dtype, C + 8)
        aff = torch.stack([t for t in bu[:4]]).contiguous().cuda()
        gamma = bu[4].contiguous().cuda()
        _call("dy_bn_act_fwd", uv.ptr, uv.ld, aff[0].data_ptr(), aff[1].data_ptr(), code, None, 0, yv.ptr, yv.ld, px, C, did)
        sums = torch.zeros(2 * C * _C.BN_BWD_REPLICAS, dtype=torch.float64, device="cuda")
        dg, db = _tail(C), _tail(C)
        _call("dy_bn_act_bwd_valid", dyv.ptr, dyv.ld, uv.ptr, uv.ld, aff.data_ptr(), gamma.data_ptr(), code, sums.data_ptr(), dzv.ptr, dzv.ld,
              dg.data_ptr(), db.data_ptr(), px, C, C, did)
        torch.cuda.synchronize()
        fa = (u, v, bu[0], bu[1], bv[0], bv[1], code)
        ba = (dy, u, v, bu, bv, code)
        # new against old in the same measure, with the allowance of the comparison against float64
        rule = RULE if dt == "f32" else 1.0
        for what, new, old, ref, terms, emu in (("y", y_new, yv.get(), rr.bn2_forward(*fa), rr.bn2_forward_terms(*fa), rr.bn2_forward(*fa, dt=torch.float32)),
                                                ("du", du_new, dzv.get(), rr.bn2_backward(*ba)[0], rr.bn2_backward_terms(*ba)[0],
                                                 rr.bn2_backward(*ba, dt=torch.float32)[0])):
            e, bound = _measure(new, old, terms, dt), max(rule, 4 * _measure(_round(emu, dt), ref, terms, dt))
            print(f"FIG {tag} {what} new-vs-old: err {e:.3e} bound {bound:.3e} ratio {e / bound:.3f}")
            figs.append((f"{tag} {what} new-vs-old", e, bound))
    _report(figs)
