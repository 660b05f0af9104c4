"""GPU: the five C-ABI entries of csrc/scconv.hip (dy_chan_moments, dy_sru_fwd / bwd, dy_cru_fuse_fwd / bwd) and the ASFF blend of
csrc/pool.hip (dy_asff_fuse_fwd / bwd), each called directly and compared with a float64 reference of the same operation on the same
tensors (tests/scconv_ref.py; tests/test_scconv_ref_cpu.py ties those references to the goldens and to autograd).

Errors.  Elementwise outputs: max |got - ref| / max |ref| per image (ASFF: per tensor).  Sums (moments, red, ds): |got - ref| /
sum |terms| per key, worst key, because the sums cancel.  Ceilings are the project's f32 figures (forward 1e-4, gradients 2e-3,
tests/test_gpu_parity.py); inside them every group has a fixed bound of 4 x the worst error the product measured on an MI355X
over all cases of the group, rounded up to one significant digit (the 4 covers other compilers and the arrival order of the f64
atomics, whose terms are f32 block sums).  "torch f32" is the same operation evaluated by torch in f32 on the CPU on the same cases.

    group            product      torch f32    bound
    moments          4.2e-07      2.3e-07      2e-06
    sru_fwd          1.2e-07      7.4e-07      5e-07
    sru_dx           1.2e-07      6.7e-07      5e-07
    sru_red          2.0e-07      2.3e-07      8e-07
    cru_fwd          1.2e-06      3.0e-06      5e-06
    cru_dout         2.6e-06      6.5e-06      2e-05
    cru_ds           1.4e-07      1.3e-07      6e-07
    asff_fwd         1.5e-07      1.5e-07      7e-07
    asff_dx          1.1e-07      1.1e-07      5e-07
    asff_dlogits     4.6e-07      4.6e-07      2e-06

No group is worse than torch's own f32 by more than a factor 1.9 (moments: the rows of a block are added one after the other in
f32, torch sums pairwise); the SRU rows are below torch's, since the kernels take their group statistics from f64 moments.  The CRU
rows are an order above the others, for torch alike: they come from the "offsets" case, where one f32 ulp of a pooled mean near
100 (8e-6) is a relative error of that size in every softmax weight.  Gate flips on unambiguous elements: 0 in all 22 SRU forward
cases; excluded shares 0 .. 9.9e-4.
16-bit outputs measured at 0.37 .. 0.49 of (bound + 1 ulp): correctly rounded.

Operands are channel slices [8, 8 + C) of wider parents filled with a sentinel, each operand of a call with its own ld; the lanes
outside every view must survive every call.  Destinations an entry overwrites start as NaN; destinations it adds to (moments,
red, ds, and dx_k with its acc flag) start from known non-zero values and must end at prior + reference: SCConv._fwd / _bwd rely
on handing these entries zeroed sums.  The apply passes of dy_sru_bwd / dy_cru_fuse_bwd read the sums back, prior included, and
the references do the same.

The SRU gate is a hard decision; scconv_ref's docstring says how it is handled (ambiguous pairs left out of the forward, capped at
1e-3 of the elements; nothing left out of the backward; gate flips on unambiguous elements counted from the kernel's y: 0).

16-bit outputs: the f32 bound plus one ulp of the type at the reference value (for an accumulating destination at prior + ref);
16-bit inputs and incoming gradients are drawn exactly representable.
"""
import functools

import pytest
import torch

import scconv_ref as sr

pytestmark = pytest.mark.gpu

BOUNDS = {
    "moments": 2e-6, "sru_fwd": 5e-7, "sru_dx": 5e-7, "sru_red": 8e-7, "cru_fwd": 5e-6, "cru_dout": 2e-5, "cru_ds": 6e-7,
    "asff_fwd": 7e-7, "asff_dx": 5e-7, "asff_dlogits": 2e-6,
}
FWD_GROUPS = ("moments", "sru_fwd", "cru_fwd", "asff_fwd")
FWD_CEILING, GRAD_CEILING = 1e-4, 2e-3
DT = sr.DT
F64 = torch.float64
SENTINEL = 99.0                 # exact in all three dtypes
C0 = 8                          # every view starts at lane 8 of its parent


def test_bounds_respect_the_ceilings():
    for k, v in BOUNDS.items():
        assert v <= (FWD_CEILING if k in FWD_GROUPS else GRAD_CEILING), k


def _api():
    from dedark_yolo_amd._C import call
    from dedark_yolo_amd.ops import dt_id, ptr, stream
    return call, ptr, stream, dt_id


class View:
    """[rows, C] at lanes [C0, C0 + C) of a [rows, ld] parent full of the sentinel; `fill` is a tensor, or NaN for a destination."""

    def __init__(self, rows, C, ld, dtype, fill=float("nan")):
        assert ld >= C0 + C and ld % 8 == 0
        self.C, self.ld = C, ld
        self.parent = torch.full((rows, ld), SENTINEL, device="cuda", dtype=dtype)
        self.parent[:, C0:C0 + C] = fill.reshape(rows, C).to(dtype).cuda() if isinstance(fill, torch.Tensor) else fill
        self.ptr = self.parent.data_ptr() + C0 * self.parent.element_size()

    def get(self, *shape):
        v = self.parent[:, C0:C0 + self.C].double().cpu()
        return v.reshape(*shape) if shape else v

    def intact(self, what):
        p = self.parent
        assert bool((p[:, :C0] == SENTINEL).all()) and bool((p[:, C0 + self.C:] == SENTINEL).all()), f"{what}: wrote outside the view"


class Sums:
    """An f64 destination the entry adds to: `prior` followed by 16 sentinels."""

    def __init__(self, prior):
        self.n, self.shape = prior.numel(), prior.shape
        self.buf = torch.full((self.n + 16,), SENTINEL, device="cuda", dtype=F64)
        self.buf[:self.n] = prior.flatten().cuda()
        self.ptr = self.buf.data_ptr()

    def get(self):
        return self.buf[:self.n].cpu().reshape(self.shape)

    def intact(self, what):
        assert bool((self.buf[self.n:] == SENTINEL).all()), f"{what}: wrote past the sums"


def _check(group, e, t, what):
    """Print the figure (product, torch f32), then assert the group's bound."""
    print(f"FIG {group} {e:.3e} {t:.3e} {what}")
    assert e <= BOUNDS[group], f"{group} {what}: {e:.3e} > {BOUNDS[group]:.0e} (torch f32: {t:.3e})"


def _check16(group, got, ref, dtype, what, keep=None):
    """A 16-bit output [N, ...]: within the f32 bound (of the image's max |ref|) plus one ulp of `dtype` at the reference value."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    n = ref.shape[0]
    tol = BOUNDS[group] * ref.reshape(n, -1).abs().amax(1).reshape([n] + [1] * (ref.ndim - 1)) + sr.ulp(ref, dtype)
    over = (got - ref).abs() / tol
    if keep is not None:
        over = over * keep
    over = float(over.max())
    print(f"FIG16 {group} {dtype} {over:.3f} of the allowance {what}")
    assert over <= 1.0, f"{group} {dtype} {what}: {over:.3f} x (bound + 1 ulp)"


def _elementwise(group, got, ref, t32, dt, what, keep=None):
    if dt != "f32":
        return _check16(group, got, ref, DT[dt], what, keep)
    if keep is None:
        return _check(group, sr.rel_err(got, ref), sr.rel_err(t32, ref) if t32 is not None else float("nan"), what)
    _check(group, sr.masked_rel_err(got, ref, keep), sr.masked_rel_err(t32, ref, keep), what)


def _cases(table, col):
    return [(n, dt) for n, v in table.items() for dt in v[col]]


# ========================================================================================================= dy_chan_moments
@pytest.mark.parametrize("name,dt", _cases(sr.MOMENT_CASES, 3))
def test_chan_moments(name, dt):
    call, ptr, stream, dt_id = _api()
    c = sr.moments_case(name, dt)
    N, C, HW, x = c["N"], c["C"], c["HW"], c["x"]
    xv = View(N * HW, C, C + 24, DT[dt], x)
    out = Sums(c["prior"])
    call("dy_chan_moments", xv.ptr, xv.ld, N, HW, C, out.ptr, dt_id(DT[dt]), stream())
    torch.cuda.synchronize()
    terms = sr.moments_terms(x) + c["prior"].abs()
    e = sr.sum_err(out.get(), c["prior"] + sr.moments_ref(x), terms)
    t = sr.sum_err(c["prior"] + sr.moments_ref(x, torch.float32).double(), c["prior"] + sr.moments_ref(x), terms)
    _check("moments", e, t, f"{name} {dt}")
    xv.intact(name)
    out.intact(name)


# ==================================================================================================== dy_sru_fwd / dy_sru_bwd
@functools.lru_cache(maxsize=None)
def _sru_fwd_ref(name, dt):
    c = sr.sru_case(name, dt)
    with torch.no_grad():
        y, gn, t = sr.sru_ref(c["x"], c["gamma"], c["beta"], c["G"], c["eps"])
        y32 = sr.sru_ref(c["x"], c["gamma"], c["beta"], c["G"], c["eps"], torch.float32)[0]
    amb = sr.ambiguous(gn, c["gamma"], c["beta"])
    pair = amb | sr._swap(amb)
    return y, gn, t >= 0, pair, y32


@pytest.mark.parametrize("name,dt", _cases(sr.SRU_CASES, 4))
def test_sru_fwd(name, dt):
    call, ptr, stream, dt_id = _api()
    c = sr.sru_case(name, dt)
    N, C, G, HW = c["N"], c["C"], c["G"], c["HW"]
    y, gn, m, pair, y32 = _sru_fwd_ref(name, dt)
    mom = sr.moments_ref(c["x"]).cuda()
    mom0 = mom.clone()
    gamma, beta = c["gamma"].cuda(), c["beta"].cuda()
    xv = View(N * HW, C, C + 16, DT[dt], c["x"])
    yv = View(N * HW, C, C + 24, DT[dt])
    call("dy_sru_fwd", xv.ptr, xv.ld, yv.ptr, yv.ld, N, HW, C, G, ptr(mom), ptr(gamma), ptr(beta), c["eps"], dt_id(DT[dt]), stream())
    torch.cuda.synchronize()
    got = yv.get(N, HW, C)
    share = float(pair.double().mean())
    ymax = y.abs().max()
    tol = BOUNDS["sru_fwd"] * float(ymax) + (0.0 if dt == "f32" else float(sr.ulp(ymax, DT[dt])))
    flips = sr.gate_flips(got, gn, m, pair, tol)
    print(f"GATE sru_fwd {name} {dt}: excluded share {share:.2e}, gate flips on unambiguous pairs {flips}")
    assert share <= sr.SHARE_CAP
    assert flips == 0, f"{flips} gate decisions differ from the reference on unambiguous elements"
    _elementwise("sru_fwd", got, y, y32, dt, f"{name} {dt}", keep=~pair)
    xv.intact(name)
    yv.intact(name)
    assert torch.equal(mom, mom0)


@functools.lru_cache(maxsize=None)
def _sru_bwd_ref(name, dt, with_prior):
    c = sr.sru_case(name, dt)
    args = (c["x"], c["dy"], c["gamma"], c["beta"], c["G"], c["eps"])
    dx, red, terms = sr.sru_bwd_ref(*args, prior=c["red_prior"] if with_prior else None)
    dx32, red32, _ = sr.sru_bwd_ref(*args, dtype=torch.float32)
    return dx, red, terms, (None if with_prior else dx32), red32.double()


@pytest.mark.parametrize("prior", ["zeroed", "prior"])
@pytest.mark.parametrize("name,dt", _cases(sr.SRU_CASES, 4))
def test_sru_bwd(name, dt, prior):
    """red is ADDED to (zeros: the module's use, dx against autograd; a non-zero prior: prior + reference, and the apply pass reads
    that total); dx is written."""
    call, ptr, stream, dt_id = _api()
    c = sr.sru_case(name, dt)
    N, C, G, HW = c["N"], c["C"], c["G"], c["HW"]
    with_prior = prior == "prior"
    dx, red, terms, dx32, red32 = _sru_bwd_ref(name, dt, with_prior)
    p0 = c["red_prior"] if with_prior else torch.zeros_like(c["red_prior"])
    mom = sr.moments_ref(c["x"]).cuda()
    gamma, beta = c["gamma"].cuda(), c["beta"].cuda()
    xv = View(N * HW, C, C + 16, DT[dt], c["x"])
    dyv = View(N * HW, C, C + 24, DT[dt], c["dy"])
    dxv = View(N * HW, C, C + 32, DT[dt])
    rd = Sums(p0)
    call("dy_sru_bwd", xv.ptr, xv.ld, dyv.ptr, dyv.ld, dxv.ptr, dxv.ld, N, HW, C, G, ptr(mom), ptr(gamma), ptr(beta), c["eps"], rd.ptr,
         dt_id(DT[dt]), stream())
    torch.cuda.synchronize()
    what = f"{name} {dt} {prior}"
    tm = terms + p0.abs()
    _check("sru_red", sr.sum_err(rd.get(), p0 + red, tm), sr.sum_err(p0 + red32, p0 + red, tm), what)
    got = dxv.get(N, HW, C)
    assert torch.isfinite(got).all()
    _elementwise("sru_dx", got, dx, dx32, dt, what)
    for v in (xv, dyv, dxv, rd):
        v.intact(what)


# ========================================================================================== dy_cru_fuse_fwd / dy_cru_fuse_bwd
@pytest.mark.parametrize("name,dt", _cases(sr.CRU_CASES, 2))
def test_cru_fuse_fwd(name, dt):
    call, ptr, stream, dt_id = _api()
    c = sr.cru_case(name, dt)
    N, C, HW = c["N"], c["C"], c["HW"]
    with torch.no_grad():
        ref = sr.cru_fuse_ref(c["o"])[0]
        t32 = sr.cru_fuse_ref(c["o"], torch.float32)[0]
    mom = sr.moments_ref(c["o"]).cuda()
    ov = View(N * HW, 2 * C, 2 * C + 16, DT[dt], c["o"])
    rv = View(N * HW, C, C + 24, DT[dt])
    call("dy_cru_fuse_fwd", ov.ptr, ov.ld, rv.ptr, rv.ld, N, HW, C, ptr(mom), dt_id(DT[dt]), stream())
    torch.cuda.synchronize()
    _elementwise("cru_fwd", rv.get(N, HW, C), ref, t32, dt, f"{name} {dt}")
    ov.intact(name)
    rv.intact(name)


@pytest.mark.parametrize("prior", ["zeroed", "prior"])
@pytest.mark.parametrize("name,dt", _cases(sr.CRU_CASES, 2))
def test_cru_fuse_bwd(name, dt, prior):
    """ds[n][k][0] is ADDED to and read back by the apply pass; slot 1 of ds belongs to the shared reduction and gains exactly 0."""
    call, ptr, stream, dt_id = _api()
    c = sr.cru_case(name, dt)
    N, C, HW = c["N"], c["C"], c["HW"]
    p0 = c["ds_prior"] if prior == "prior" else torch.zeros_like(c["ds_prior"])
    with torch.no_grad():
        dout, ds, terms = sr.cru_fuse_bwd_ref(c["o"], c["dres"], p0[..., 0])
        dout32, ds32, _ = sr.cru_fuse_bwd_ref(c["o"], c["dres"], p0[..., 0], torch.float32)
    mom = sr.moments_ref(c["o"]).cuda()
    ov = View(N * HW, 2 * C, 2 * C + 16, DT[dt], c["o"])
    dv = View(N * HW, C, C + 24, DT[dt], c["dres"])
    gv = View(N * HW, 2 * C, 2 * C + 32, DT[dt])
    sd = Sums(p0)
    call("dy_cru_fuse_bwd", ov.ptr, ov.ld, dv.ptr, dv.ld, gv.ptr, gv.ld, N, HW, C, ptr(mom), sd.ptr, dt_id(DT[dt]), stream())
    torch.cuda.synchronize()
    what = f"{name} {dt} {prior}"
    got = sd.get()
    tm = terms + p0[..., 0].abs()
    _check("cru_ds", sr.sum_err(got[..., 0], p0[..., 0] + ds, tm), sr.sum_err(p0[..., 0] + ds32.double(), p0[..., 0] + ds, tm), what)
    assert torch.equal(got[..., 1], p0[..., 1]), "slot 1 of ds"
    _elementwise("cru_dout", gv.get(N, HW, 2 * C), dout, dout32, dt, what)
    for v in (ov, dv, gv, sd):
        v.intact(what)


# ======================================================================================== dy_asff_fuse_fwd / dy_asff_fuse_bwd
ASFF_MODES = [(3, 3), (3, 8), (2, 2), (2, 4), (2, 8)]          # (sources, ld of the logits)


def _asff_views(c, dt):
    P, C = c["P"], c["C"]
    xs = [View(P, C, C + 16 + 8 * k, DT[dt], x) for k, x in enumerate(c["xs"])]
    xs += [None] * (3 - len(xs))
    lg = c["logits"].to(DT[dt]).cuda()
    arg = lambda v: (v.ptr, v.ld) if v is not None else (None, 0)
    return xs, lg, arg


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", sr.ASFF_LOGIT_KINDS)
@pytest.mark.parametrize("mode", ASFF_MODES, ids=lambda m: f"{m[0]}src_ldl{m[1]}")
@pytest.mark.parametrize("shape", list(sr.ASFF_SHAPES))
def test_asff_fuse_fwd(shape, mode, kind, dt):
    call, ptr, stream, dt_id = _api()
    nsrc, ldl = mode
    c = sr.asff_case(shape, nsrc, ldl, kind, dt)
    P, C = c["P"], c["C"]
    ref = sr.asff_ref(c["xs"], c["logits"])[0]
    t32 = sr.asff_ref(c["xs"], c["logits"], torch.float32)[0]
    xs, lg, arg = _asff_views(c, dt)
    ov = View(P, C, C + 48, DT[dt])
    call("dy_asff_fuse_fwd", *arg(xs[0]), *arg(xs[1]), *arg(xs[2]), ptr(lg), ldl, ov.ptr, ov.ld, P, C, dt_id(DT[dt]), stream())
    torch.cuda.synchronize()
    what = f"{shape} {nsrc}src ldl={ldl} {kind} {dt}"
    _elementwise("asff_fwd", ov.get(1, P, C), ref[None], t32[None], dt, what)
    for v in xs[:nsrc] + [ov]:
        v.intact(what)


def _asff_bwd_case(shape, nsrc, ldl, lddl, kind, acc, dt):
    call, ptr, stream, dt_id = _api()
    c = sr.asff_case(shape, nsrc, ldl, kind, dt)
    P, C = c["P"], c["C"]
    priors = [c["priors"][k] if acc[k] else None for k in range(nsrc)]
    dxs, dlog = sr.asff_bwd_ref(c["xs"], c["logits"], c["dout"], priors)
    dxs32, dlog32 = sr.asff_bwd_ref(c["xs"], c["logits"], c["dout"], priors, torch.float32)
    xs, lg, arg = _asff_views(c, dt)
    gv = View(P, C, C + 48, DT[dt], c["dout"])
    dv = [View(P, C, C + 56 + 8 * k, DT[dt], *([priors[k]] if priors[k] is not None else [])) for k in range(nsrc)]
    dv += [None] * (3 - nsrc)
    written = min(lddl, 8)
    dl = torch.full((P, lddl), SENTINEL, device="cuda", dtype=DT[dt])
    dl[:, :written] = float("nan")
    call("dy_asff_fuse_bwd", gv.ptr, gv.ld, *arg(xs[0]), *arg(xs[1]), *arg(xs[2]), ptr(lg), ldl, *arg(dv[0]), *arg(dv[1]), *arg(dv[2]),
         ptr(dl), lddl, P, C, acc[0], acc[1], acc[2], dt_id(DT[dt]), stream())
    torch.cuda.synchronize()
    what = f"{shape} {nsrc}src ldl={ldl} lddl={lddl} {kind} acc={acc} {dt}"
    for k in range(nsrc):
        _elementwise("asff_dx", dv[k].get(1, P, C), dxs[k][None], dxs32[k][None], dt, what + f" dx{k}")
    got = dl.double().cpu()
    _elementwise("asff_dlogits", got[None, :, :nsrc], dlog[None], dlog32[None], dt, what)
    assert bool((got[:, nsrc:written] == 0).all()), "dlogits: the two-level column 2 and the pad columns up to 8 are written as 0"
    assert bool((got[:, written:] == SENTINEL).all()), "dlogits: columns >= 8 are not the entry's"
    for v in xs[:nsrc] + dv[:nsrc] + [gv]:
        v.intact(what)


ACC3 = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]
ACC2 = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)]


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", ["normal", "offset"])
@pytest.mark.parametrize("acc", ACC3, ids=lambda a: "acc" + "".join(map(str, a)))
@pytest.mark.parametrize("shape", list(sr.ASFF_SHAPES))
def test_asff_fuse_bwd_three_sources(shape, acc, kind, dt):
    _asff_bwd_case(shape, 3, 4, 4, kind, acc, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", ["normal", "offset"])
@pytest.mark.parametrize("acc", ACC2, ids=lambda a: "acc" + "".join(map(str, a)))
@pytest.mark.parametrize("shape,ldl", list(zip(sr.ASFF_SHAPES, [2, 4, 8, 2, 4])))
def test_asff_fuse_bwd_two_sources(shape, ldl, acc, kind, dt):
    """x2 = NULL, ld2 = 0, dx2 = NULL; acc2 is ignored."""
    _asff_bwd_case(shape, 2, ldl, ldl, kind, acc, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("nsrc", [3, 2])
@pytest.mark.parametrize("lddl", [3, 4, 8, 16])
def test_asff_dlogits_width(lddl, nsrc, dt):
    """Columns [0, 3) the gradient (column 2 is 0 with two sources), [3, min(lddl, 8)) zeros, >= 8 untouched."""
    _asff_bwd_case("c128", nsrc, 4, lddl, "mixed", (0, 0, 0), dt)


# ============================================================================ ops.asff_fuse_forward / ops.asff_fuse_backward
def _nhwc(v, C=None):
    """A View, or a plain [P, ld] tensor with its first C columns, as the NHWC view [1, C, P, 1] the ops wrappers take."""
    t, c0, C = (v.parent, C0, v.C) if isinstance(v, View) else (v, 0, C)
    return t.view(1, t.shape[0], 1, t.shape[1]).permute(0, 3, 1, 2)[:, c0:c0 + C]


def _bytes(t):
    return t.contiguous().view(torch.uint8)


ASFF_WRAPPER_INTO = {3: [None, (1, 0, 1), (1, 1, 1)], 2: [None, (0, 1), (1, 1)]}


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("nsrc,ldl,into", [(n, ldl, a) for n, ldl in ((3, 4), (2, 2)) for a in ASFF_WRAPPER_INTO[n]],
                         ids=lambda v: "into" + ("".join(map(str, v)) if v else "None") if not isinstance(v, int) else str(v))
@pytest.mark.parametrize("shape", ["p1", "p3"])
def test_asff_wrappers_are_the_direct_calls(shape, nsrc, ldl, into, dt):
    """ops.asff_fuse_forward / asff_fuse_backward on NHWC views of the same strided operands: within the groups' budgets of the f64
    reference, and byte for byte what the direct call gives; `into` selects the kernel's acc flags and comes back as the result."""
    from dedark_yolo_amd import ops
    call, ptr, stream, dt_id = _api()
    c = sr.asff_case(shape, nsrc, ldl, "mixed", dt)
    P, C = c["P"], c["C"]
    what = f"wrapper {shape} {nsrc}src ldl={ldl} into={into} {dt}"
    xs, lg, arg = _asff_views(c, dt)
    src, logits = [_nhwc(v) for v in xs[:nsrc]], _nhwc(lg, nsrc)
    # forward: a fresh output, and `out=` a strided view
    ref, t32 = sr.asff_ref(c["xs"], c["logits"])[0], sr.asff_ref(c["xs"], c["logits"], torch.float32)[0]
    ov, wv = View(P, C, C + 48, DT[dt]), View(P, C, C + 48, DT[dt])
    call("dy_asff_fuse_fwd", *arg(xs[0]), *arg(xs[1]), *arg(xs[2]), ptr(lg), ldl, ov.ptr, ov.ld, P, C, dt_id(DT[dt]), stream())
    fresh = ops.asff_fuse_forward(src, logits)
    assert ops.asff_fuse_forward(src, logits, out=_nhwc(wv)).data_ptr() == wv.ptr
    torch.cuda.synchronize()
    assert tuple(fresh.shape) == (1, C, P, 1) and fresh.dtype == DT[dt]
    _elementwise("asff_fwd", wv.get(1, P, C), ref[None], t32[None], dt, what)
    assert torch.equal(_bytes(ov.parent), _bytes(wv.parent)) and torch.equal(_bytes(fresh.permute(0, 2, 3, 1).reshape(P, C)), _bytes(ov.parent[:, C0:C0 + C]))
    # backward
    acc = tuple(into or (0,) * nsrc) + (0,) * (3 - nsrc)
    priors = [c["priors"][k] if acc[k] else None for k in range(nsrc)]
    dxs, dlog = sr.asff_bwd_ref(c["xs"], c["logits"], c["dout"], priors)
    dxs32, dlog32 = sr.asff_bwd_ref(c["xs"], c["logits"], c["dout"], priors, torch.float32)
    gv = View(P, C, C + 48, DT[dt], c["dout"])
    mk = lambda: [View(P, C, C + 56 + 8 * k, DT[dt], *([priors[k]] if priors[k] is not None else [])) for k in range(nsrc)] + [None] * (3 - nsrc)
    dv, wd = mk(), mk()
    lddl = ops.ld_of(logits)                                  # the wrapper's dlogits buffer is as wide as the logits' own
    dl = torch.full((P, lddl), float("nan"), device="cuda", dtype=DT[dt])
    call("dy_asff_fuse_bwd", gv.ptr, gv.ld, *arg(xs[0]), *arg(xs[1]), *arg(xs[2]), ptr(lg), ldl, *arg(dv[0]), *arg(dv[1]), *arg(dv[2]),
         ptr(dl), lddl, P, C, *acc, dt_id(DT[dt]), stream())
    got, gl = ops.asff_fuse_backward(_nhwc(gv), src, logits, into=into and [_nhwc(wd[k]) if acc[k] else None for k in range(nsrc)])
    torch.cuda.synchronize()
    assert len(got) == nsrc and tuple(gl.shape) == (1, nsrc, P, 1) and ops.ld_of(gl) == lddl
    for k in range(nsrc):
        assert tuple(got[k].shape) == (1, C, P, 1) and (got[k].data_ptr() == wd[k].ptr) == bool(acc[k]), f"{what}: dx{k} is into[{k}] when given"
        flat = got[k].permute(0, 2, 3, 1).reshape(P, C)
        _elementwise("asff_dx", flat.double().cpu()[None], dxs[k][None], dxs32[k][None], dt, what + f" dx{k}")
        assert torch.equal(_bytes(flat), _bytes(dv[k].parent[:, C0:C0 + C])), f"{what}: dx{k} differs from the direct call"
    flat = gl.permute(0, 2, 3, 1).reshape(P, nsrc)
    _elementwise("asff_dlogits", flat.double().cpu()[None], dlog[None], dlog32[None], dt, what)
    assert torch.equal(_bytes(flat), _bytes(dl[:, :nsrc])), f"{what}: dlogits differ from the direct call"
    for v in xs[:nsrc] + [gv, ov, wv] + [wd[k] for k in range(nsrc) if acc[k]]:
        v.intact(what)


def test_asff_wrappers_refuse_mismatched_operands():
    from dedark_yolo_amd import ops
    x = [ops.empty_nhwc(1, 16, 2, 2, torch.float32, "cuda") for _ in range(4)]
    lg = ops.empty_nhwc(1, 4, 2, 2, torch.float32, "cuda")
    with pytest.raises(RuntimeError, match="two or three sources"):
        ops.asff_fuse_forward(x[:1], lg[:, :1])
    with pytest.raises(RuntimeError, match="two or three sources"):
        ops.asff_fuse_forward(x, lg)
    with pytest.raises(RuntimeError, match="two or three sources"):
        ops.asff_fuse_forward([x[0], x[1][:, :8]], lg[:, :2])
    with pytest.raises(RuntimeError, match="two or three sources"):
        ops.asff_fuse_forward(x[:2], lg[:, :2], out=x[2].half())
    with pytest.raises(RuntimeError, match="need logits"):
        ops.asff_fuse_forward(x[:3], lg[:, :2])
    with pytest.raises(RuntimeError, match="two or three sources"):
        ops.asff_fuse_backward(x[3][:, :8], x[:3], lg[:, :3])


# ========================================================================================================= argument checks
def _bad_calls():
    """name -> (entry, arguments).  Every tensor holds 7 and is large enough for the call as written, so even a check that
    failed to fire would stay in bounds."""
    call, ptr, stream, _ = _api()
    z = lambda *s: torch.full(s, 7.0, device="cuda")
    zd = lambda *s: torch.full(s, 7.0, device="cuda", dtype=F64)
    ROWS, LD, BIG = 4, 1056, 8240
    t = dict(a=z(ROWS, LD), b=z(ROWS, LD), c=z(ROWS, LD), o=z(2, BIG), r=z(2, BIG), g=z(2, BIG), mom=zd(BIG * 2), red=zd(BIG * 2),
             gam=z(LD), bet=z(LD), x0=z(ROWS, 32), x1=z(ROWS, 32), x2=z(ROWS, 32), d0=z(ROWS, 32), d1=z(ROWS, 32), d2=z(ROWS, 32),
             go=z(ROWS, 32), out=z(ROWS, 32), lg=z(ROWS, 8), dlg=z(ROWS, 8))
    p, st = (lambda k: ptr(t[k])), stream()
    sru_f = lambda C, G, HW=ROWS, mom="mom": ("dy_sru_fwd", (p("a"), LD, p("b"), LD, 1, HW, C, G, mom and p(mom), p("gam"), p("bet"), 1e-10, 0, st))
    sru_b = lambda C, G, HW=ROWS, mom="mom", red="red": ("dy_sru_bwd", (p("a"), LD, p("b"), LD, p("c"), LD, 1, HW, C, G, mom and p(mom), p("gam"),
                                                                        p("bet"), 1e-10, red and p(red), 0, st))
    cru_f = lambda C, mom="mom": ("dy_cru_fuse_fwd", (p("o"), BIG, p("r"), BIG, 1, 2, C, mom and p(mom), 0, st))
    cru_b = lambda C, mom="mom", ds="red": ("dy_cru_fuse_bwd", (p("o"), BIG, p("r"), BIG, p("g"), BIG, 1, 2, C, mom and p(mom), ds and p(ds), 0, st))
    asff_f = lambda ldl, lg="lg": ("dy_asff_fuse_fwd", (p("x0"), 32, p("x1"), 32, p("x2"), 32, lg and p(lg), ldl, p("out"), 32, ROWS, 16, 0, st))
    asff_b = lambda ldl, lddl, lg="lg", dlg="dlg": ("dy_asff_fuse_bwd", (p("go"), 32, p("x0"), 32, p("x1"), 32, p("x2"), 32, lg and p(lg), ldl,
                                                                         p("d0"), 32, p("d1"), 32, p("d2"), 32, dlg and p(dlg), lddl, ROWS, 16,
                                                                         0, 0, 0, 0, st))
    calls = {
        "sru_fwd_groups65": sru_f(520, 65), "sru_bwd_groups65": sru_b(520, 65),
        "sru_fwd_C_not_groups": sru_f(64, 5), "sru_bwd_C_not_groups": sru_b(64, 5),
        "sru_fwd_half_not_vec": sru_f(12, 4), "sru_bwd_half_not_vec": sru_b(12, 4),
        "sru_fwd_one_element_group": sru_f(8, 8, HW=1), "sru_bwd_one_element_group": sru_b(8, 8, HW=1),
        "sru_fwd_null_moments": sru_f(64, 4, mom=None), "sru_bwd_null_moments": sru_b(64, 4, mom=None),
        "sru_bwd_null_red": sru_b(64, 4, red=None),
        "moments_null_out": ("dy_chan_moments", (p("a"), LD, 1, ROWS, 64, None, 0, st)),
        "cru_fwd_C2056": cru_f(2056), "cru_bwd_C2056": cru_b(2056),
        "cru_fwd_null_moments": cru_f(64, mom=None), "cru_bwd_null_moments": cru_b(64, mom=None), "cru_bwd_null_ds": cru_b(64, ds=None),
        "asff_fwd_ldl2_three": asff_f(2), "asff_bwd_ldl2_three": asff_b(2, 4), "asff_bwd_lddl2_three": asff_b(4, 2),
        "asff_fwd_null_logits": asff_f(4, lg=None), "asff_bwd_null_logits": asff_b(4, 4, lg=None),
        "asff_bwd_null_dlogits": asff_b(4, 4, dlg=None),
    }
    return call, t, calls


@pytest.mark.parametrize("name", ["sru_fwd_groups65", "sru_bwd_groups65", "sru_fwd_C_not_groups", "sru_bwd_C_not_groups",
                                  "sru_fwd_half_not_vec", "sru_bwd_half_not_vec", "sru_fwd_one_element_group",
                                  "sru_bwd_one_element_group", "sru_fwd_null_moments", "sru_bwd_null_moments", "sru_bwd_null_red",
                                  "moments_null_out", "cru_fwd_C2056", "cru_bwd_C2056", "cru_fwd_null_moments", "cru_bwd_null_moments",
                                  "cru_bwd_null_ds", "asff_fwd_ldl2_three", "asff_bwd_ldl2_three", "asff_bwd_lddl2_three",
                                  "asff_fwd_null_logits", "asff_bwd_null_logits", "asff_bwd_null_dlogits"])
def test_argument_checks_raise_and_launch_nothing(name):
    call, t, calls = _bad_calls()
    entry, args = calls[name]
    with pytest.raises(RuntimeError, match=entry + " failed.*" + entry):
        call(entry, *args)
    torch.cuda.synchronize()
    for k, v in t.items():
        assert bool((v == 7.0).all()), f"{name}: {k} was written"
