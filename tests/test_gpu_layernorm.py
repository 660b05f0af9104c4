"""GPU tests of csrc/layernorm.hip through the C-ABI, per entry point, in fp32, bf16 and fp16 against the float64 statement
tests/aifi_ref.py computed from the same (rounded) inputs: dy_add_layernorm_fwd / _bwd, dy_gelu_fwd / _bwd, dy_add_pos.

Views: every tensor operand is a C-channel slice at channel c0 of a [rows, c0 + C + 8] buffer filled with a sentinel (guards on
both sides of every row, ld > C); the guards and every input must be unchanged after every call.  c0 = 8 keeps 16-byte alignment
wherever C allows it (the vector path); c0 = 3 forces the element path in every dtype.  The f32 outputs (stats, dgamma, dbeta,
scratch) carry a sentinel tail.

LayerNorm shapes: C in {4, 8, 72, 256, 576, 640, 2048} (4: the smallest, below a vector in the 16-bit types; 72: not a power of two,
most lanes idle; 576 / 640: the m / x scale; 2048: the only width a whole workgroup owns, with 1024 < C) x rows in {1, 7, 130} (one
wave; two workgroups with an idle wave; 33 workgroups), each with b null and non-null and accumulate 0 and 1.  Special rows: a
constant row (variance 0: y = beta, dz finite) and, in f32, rows of mean 1e3 and unit spread, which an E[z^2] - mean^2 kernel
fails by orders of magnitude.  Every backward runs twice: identical bytes.

Error measure: |got - ref64| / sum |terms| (tests/test_gpu_attn.py's measure; the terms are aifi_ref's *_terms).  Rule: 2e-6 for
f32 outputs, the same plus one ulp of the type at the reference value for 16-bit outputs.  E is the error in the same measure of
torch's own CPU f32 F.layer_norm / F.gelu and their autograd on the same rounded inputs (16-bit modes: outputs rounded to the
type); the kernel is allowed max(rule, 4 E), the factor test_gpu_attn.py and test_gpu_optimizers.py use against a reference f32
run.  Every case prints its measured error / allowance.
"""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aifi_ref as ar
from frontend_ref import ulp

pytestmark = pytest.mark.gpu

RULE = 2e-6
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENTINEL = 99.0
GUARD = 8
EPS = 1e-5

LN_CASES = [(C, rows, dt, GUARD) for C in (4, 8, 72, 256, 576, 640, 2048) for rows in (1, 7, 130) for dt in DT] + \
           [(C, 7, dt, 3) for C in (72, 2048) for dt in DT]
GELU_CASES = [(C, px, dt, GUARD) for C in (4, 24, 1024) for px in (1, 130) for dt in DT] + [(24, 130, dt, 3) for dt in DT]


class Slice:
    """C channels at channel c0 of a [rows, c0 + C + GUARD] sentinel-filled parent"""

    def __init__(self, rows, C, dtype, c0, fill=None):
        self.C, self.c0, self.ld = C, c0, c0 + C + GUARD
        self.parent = torch.full((rows, self.ld), SENTINEL, device="cuda", dtype=dtype)
        if fill is not None:
            self.parent[:, c0:c0 + C] = fill.reshape(rows, C).to(dtype).cuda()
        self.before = self.parent.clone()

    @property
    def ptr(self):
        return self.parent.data_ptr() + self.c0 * self.parent.element_size()

    def get(self):
        return self.parent[:, self.c0:self.c0 + self.C].double().cpu()

    def guards_intact(self, what):
        p = self.parent
        assert bool((p[:, :self.c0] == SENTINEL).all()) and bool((p[:, self.c0 + self.C:] == SENTINEL).all()), f"{what}: guard changed"

    def unchanged(self, what):
        assert torch.equal(self.parent, self.before), f"{what}: buffer changed"


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


def _torch_ln(a, b, gamma, beta, dy, dz_old, dt):
    """torch CPU f32: F.layer_norm of a + b and its autograd; 16-bit modes round y and dz to the type"""
    rd = (lambda t: t) if dt == "f32" else (lambda t: t.to(DT[dt]).float())
    z = (a if b is None else a + b).clone().requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.layer_norm(z, (z.shape[-1],), gm, bt, EPS)
    y.backward(dy)
    zd = z.detach()
    mean = zd.mean(-1)
    rstd = torch.rsqrt(zd.var(-1, unbiased=False) + EPS)
    dz = z.grad if dz_old is None else z.grad + dz_old
    return rd(y.detach()), mean, rstd, rd(dz), gm.grad, bt.grad


def _ln_case(tag, a, b, gamma, beta, dy, dz_old, dt, c0, figs):
    """one forward and two backward runs of one operand set; appends the figures"""
    from dedark_yolo_amd import ops
    rows, C = a.shape
    dtype, did = DT[dt], ops.dt_id(DT[dt])
    y64, m64, r64 = ar.ln_forward(a, b, gamma, beta, EPS)
    ty, tm, tr = ar.ln_forward_terms(a, b, gamma, beta, EPS)
    emu = _torch_ln(a, b, gamma, beta, dy, dz_old, dt)
    av, bv = Slice(rows, C, dtype, c0, a), (None if b is None else Slice(rows, C, dtype, c0, b))
    yv = Slice(rows, C, dtype, c0)
    gm_d, bt_d = gamma.cuda(), beta.cuda()
    stats = _tail(2 * rows)
    _call("dy_add_layernorm_fwd", av.ptr, av.ld, None if bv is None else bv.ptr, 0 if bv is None else bv.ld, gm_d.data_ptr(), bt_d.data_ptr(),
          yv.ptr, yv.ld, stats.data_ptr(), rows, C, EPS, did)
    torch.cuda.synchronize()
    av.unchanged(tag + " fwd a")
    bv is None or bv.unchanged(tag + " fwd b")
    yv.guards_intact(tag + " fwd y")
    assert bool((stats[2 * rows:] == SENTINEL).all()), "stats: wrote past the end"
    st = stats[:2 * rows].double().cpu().reshape(rows, 2)
    _check(tag + " y", yv.get(), y64, ty, emu[0], dt, figs)
    _check(tag + " mean", st[:, 0], m64, tm, emu[1], "f32", figs)
    _check(tag + " rstd", st[:, 1], r64, tr, emu[2], "f32", figs)

    # the backward's inputs: the statistics as a forward would have stored them (f32); the reference uses the same
    m_in, r_in = m64.float(), r64.float()
    stats_d = torch.stack([m_in, r_in], 1).contiguous().cuda()
    dyv = Slice(rows, C, dtype, c0, dy)
    parts = ops.ln_parts(rows, C)
    runs = []
    for _ in range(2):
        dzv = Slice(rows, C, dtype, c0, dz_old)
        dg, db, scratch = _tail(C), _tail(C), _tail(parts * 2 * C)
        _call("dy_add_layernorm_bwd", av.ptr, av.ld, None if bv is None else bv.ptr, 0 if bv is None else bv.ld, stats_d.data_ptr(),
              gm_d.data_ptr(), dyv.ptr, dyv.ld, dzv.ptr, dzv.ld, 0 if dz_old is None else 1, dg.data_ptr(), db.data_ptr(), scratch.data_ptr(),
              parts * 2 * C, rows, C, did)
        torch.cuda.synchronize()
        dzv.guards_intact(tag + " bwd dz")
        for t, n in ((dg, C), (db, C), (scratch, parts * 2 * C)):
            assert bool((t[n:] == SENTINEL).all()), f"{tag}: an f32 output was written past its end"
        runs.append((dzv, dg, db))
    for s in (av, bv, dyv):
        s is None or s.unchanged(tag + " bwd")
    for x0, x1 in zip(runs[0], runs[1]):
        x0, x1 = (getattr(t, "parent", t) for t in (x0, x1))
        assert torch.equal(x0.view(torch.uint8), x1.view(torch.uint8)), f"{tag}: two backward runs differ"
    args = (a, b, m_in, r_in, gamma, dy, dz_old)
    dz64, dg64, db64 = ar.ln_backward(*args)
    tdz, tdg, tdb = ar.ln_backward_terms(*args)
    _check(tag + " dz", runs[0][0].get(), dz64, tdz, emu[3], dt, figs)
    _check(tag + " dgamma", runs[0][1][:C].double().cpu(), dg64, tdg, emu[4], "f32", figs)
    _check(tag + " dbeta", runs[0][2][:C].double().cpu(), db64, tdb, emu[5], "f32", figs)
    return yv.get(), runs[0][0].get()


@pytest.mark.parametrize("C,rows,dt,c0", LN_CASES)
def test_add_layernorm_kernels(C, rows, dt, c0):
    g = _rng("ln", C, rows, dt, c0)
    gamma, beta = _rn(g, "f32", C, shift=1.0, scale=0.3), _rn(g, "f32", C, scale=0.3)
    a, b, dy, old = (_rn(g, dt, rows, C) for _ in range(4))
    figs = []
    for with_b in (False, True):
        for acc in (False, True):
            _ln_case(f"C={C} rows={rows} {dt} lane {c0} b={int(with_b)} acc={int(acc)}", a, b if with_b else None, gamma, beta, dy,
                     old if acc else None, dt, c0, figs)
    _report(figs)


@pytest.mark.parametrize("dt", list(DT))
def test_add_layernorm_constant_row(dt):
    """rows of one value (a alone, and a + b): variance 0, so y = beta; dz is finite"""
    C, rows = 72, 7
    g = _rng("const", dt)
    gamma, beta = _rn(g, "f32", C, shift=1.0, scale=0.3), _rn(g, "f32", C, scale=0.3)
    a = torch.full((rows, C), 3.0) * torch.arange(1, rows + 1)[:, None]
    b = torch.full((rows, C), -1.25)
    dy = _rn(g, dt, rows, C)
    figs = []
    for bb in (None, b):
        y, dz = _ln_case(f"constant rows {dt} b={int(bb is not None)}", a, bb, gamma, beta, dy, None, dt, GUARD, figs)
        assert bool(torch.isfinite(dz).all())
        assert torch.equal(ar.ln_forward(a, bb, gamma, beta, EPS)[0], beta.double().expand(rows, C)), "the yardstick's y is not beta"
        assert torch.equal(y, beta.to(DT[dt]).double().expand(rows, C)), "y != beta on a constant row"      # (the row sums are exact)
    _report(figs)


def test_add_layernorm_large_mean_f32():
    """f32 rows of mean 1e3 and unit spread (a alone; a + b = 600 + 400): the variance must be taken of the centred values"""
    C, rows = 256, 7
    g = _rng("mean1e3")
    gamma, beta = _rn(g, "f32", C, shift=1.0, scale=0.3), _rn(g, "f32", C, scale=0.3)
    dy = _rn(g, "f32", rows, C)
    figs = []
    _ln_case("mean 1e3 b=0", _rn(g, "f32", rows, C, shift=1e3), None, gamma, beta, dy, None, "f32", GUARD, figs)
    _ln_case("mean 1e3 b=1", _rn(g, "f32", rows, C, shift=600.0), _rn(g, "f32", rows, C, shift=400.0), gamma, beta, dy, None, "f32", GUARD, figs)
    _report(figs)


@pytest.mark.parametrize("C,px,dt,c0", GELU_CASES)
def test_gelu_kernels(C, px, dt, c0):
    from dedark_yolo_amd import ops
    dtype, did = DT[dt], ops.dt_id(DT[dt])
    g = _rng("gelu", C, px, dt, c0)
    u = torch.from_numpy(g.uniform(-10.0, 10.0, (px, C)).astype(np.float32))
    u[0, :4] = torch.tensor([0.0, -0.0, 10.0, -10.0])
    u = u.to(dtype).float()
    dy = _rn(g, dt, px, C)
    tag = f"gelu C={C} px={px} {dt} lane {c0}"
    rd = (lambda t: t) if dt == "f32" else (lambda t: t.to(dtype).float())
    ue = u.clone().requires_grad_(True)
    ye = F.gelu(ue)
    ye.backward(dy)
    uv, dyv, yv, duv = Slice(px, C, dtype, c0, u), Slice(px, C, dtype, c0, dy), Slice(px, C, dtype, c0), Slice(px, C, dtype, c0)
    _call("dy_gelu_fwd", uv.ptr, uv.ld, yv.ptr, yv.ld, px, C, did)
    _call("dy_gelu_bwd", uv.ptr, uv.ld, dyv.ptr, dyv.ld, duv.ptr, duv.ld, px, C, did)
    torch.cuda.synchronize()
    uv.unchanged(tag)
    dyv.unchanged(tag)
    yv.guards_intact(tag + " y")
    duv.guards_intact(tag + " du")
    figs = []
    _check(tag + " y", yv.get(), ar.gelu_forward(u), ar.gelu_forward_terms(u), rd(ye.detach()), dt, figs)
    _check(tag + " du", duv.get(), ar.gelu_backward(u, dy), ar.gelu_backward_terms(u, dy), rd(ue.grad), dt, figs)
    assert bool((yv.get()[0, :2] == 0).all()), "gelu(+-0) != 0"
    _report(figs)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("c0", (GUARD, 3))
def test_add_pos_bytes(dt, c0):
    """y = x + pos on (B, H, W, C) = (2, 3, 5, 64): the f32 sum rounded once, byte for byte"""
    from dedark_yolo_amd import ops
    B, H, W, C = 2, 3, 5, 64
    dtype, did = DT[dt], ops.dt_id(DT[dt])
    g = _rng("pos", dt)
    x = _rn(g, dt, B * H * W, C)
    pos = ops.sincos_pos_table(W, H, C).to(dtype)
    assert torch.equal(ops.sincos_pos_table(W, H, C), ar.pos_table(W, H, C))
    want = (x.reshape(B, H * W, C) + pos.float()[None]).to(dtype).reshape(B * H * W, C)
    xv, yv = Slice(B * H * W, C, dtype, c0, x), Slice(B * H * W, C, dtype, c0)
    pos_d = pos.cuda().contiguous()
    _call("dy_add_pos", xv.ptr, xv.ld, pos_d.data_ptr(), yv.ptr, yv.ld, B, H * W, C, did)
    torch.cuda.synchronize()
    xv.unchanged("add_pos x")
    yv.guards_intact("add_pos y")
    got = yv.parent[:, c0:c0 + C].cpu().contiguous()
    assert torch.equal(got.view(torch.uint8), want.contiguous().view(torch.uint8))


@pytest.mark.parametrize("dt", list(DT))
def test_layernorm_bad_arguments(dt):
    """C % 4, C > 2048, ld < C, null pointers: the error code, nothing written"""
    from dedark_yolo_amd import ops
    dtype, did = DT[dt], ops.dt_id(DT[dt])
    rows = 3
    for C, short, null in ((6, False, False), (2052, False, False), (64, True, False), (64, False, True)):
        z = torch.zeros(rows, C)
        av, bv, yv, dzv = (Slice(rows, C, dtype, GUARD, z) for _ in range(4))
        gm = torch.ones(C, device="cuda")
        stats, dg, db, scratch = _tail(2 * rows), _tail(C), _tail(2 * C), _tail(2 * C)
        ld = C - 4 if short else av.ld
        a_ptr = None if null else av.ptr
        with pytest.raises(RuntimeError, match="dy_add_layernorm_fwd"):
            _call("dy_add_layernorm_fwd", a_ptr, ld, bv.ptr, bv.ld, gm.data_ptr(), gm.data_ptr(), yv.ptr, yv.ld, stats.data_ptr(), rows, C, EPS, did)
        with pytest.raises(RuntimeError, match="dy_add_layernorm_bwd"):
            _call("dy_add_layernorm_bwd", a_ptr, ld, bv.ptr, bv.ld, stats.data_ptr(), gm.data_ptr(), yv.ptr, yv.ld, dzv.ptr, dzv.ld, 0,
                  dg.data_ptr(), db.data_ptr(), scratch.data_ptr(), 2 * C, rows, C, did)
        with pytest.raises(RuntimeError, match="dy_gelu_fwd"):
            _call("dy_gelu_fwd", a_ptr, ld, yv.ptr, yv.ld, rows, C if C != 2052 else 2050, did)
        with pytest.raises(RuntimeError, match="dy_gelu_bwd"):
            _call("dy_gelu_bwd", a_ptr, ld, bv.ptr, bv.ld, dzv.ptr, dzv.ld, rows, C if C != 2052 else 2050, did)
        with pytest.raises(RuntimeError, match="dy_add_pos"):
            _call("dy_add_pos", a_ptr, ld, bv.ptr, yv.ptr, yv.ld, 1, rows, C if C != 2052 else 2050, did)
        torch.cuda.synchronize()
        for s in (av, bv, yv, dzv):
            s.unchanged(f"C={C} {dt}")
        for t, n in ((stats, 0), (dg, 0), (db, 0), (scratch, 0)):
            assert bool((t == SENTINEL).all())
    # a scratch that is too small for the partials
    C = 64
    z = torch.zeros(rows, C)
    av, yv, dzv = (Slice(rows, C, dtype, GUARD, z) for _ in range(3))
    gm, stats = torch.ones(C, device="cuda"), torch.zeros(2 * rows, device="cuda")
    dg, db, scratch = _tail(C), _tail(C), _tail(2 * C)
    with pytest.raises(RuntimeError, match="scratch"):
        _call("dy_add_layernorm_bwd", av.ptr, av.ld, None, 0, stats.data_ptr(), gm.data_ptr(), yv.ptr, yv.ld, dzv.ptr, dzv.ld, 0,
              dg.data_ptr(), db.data_ptr(), scratch.data_ptr(), 2 * C - 1, rows, C, did)
    torch.cuda.synchronize()
    dzv.unchanged("scratch")
    assert bool((dg == SENTINEL).all()) and bool((db == SENTINEL).all())
