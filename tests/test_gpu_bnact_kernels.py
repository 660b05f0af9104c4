"""GPU tests of csrc/bnact.hip through the C-ABI in fp32, bf16 and fp16 against the float64 statement tests/bnact_ref.py computed
from the same (rounded) inputs: dy_bn_act_fwd, dy_bn_act_bwd_reduce, dy_bn_act_bwd_apply_valid / dy_bn_act_bwd_apply and the
merged dy_bn_act_bwd_valid / dy_bn_act_bwd, each with SiLU, no activation and LeakyReLU(0.1).  (The non-temporal variants for
tensors past 128 MB stay with tests/test_gpu_bn_kernels.py.)

Views (the conventions and helpers of tests/test_gpu_bn2act.py): z, dy and y are C-channel slices at channel 8 of [pixels, C + 16]
buffers, res and dz of [pixels, C + 8] buffers, all filled with a sentinel; every element outside a written slice and every input
must be unchanged after every call.  The f32 per-channel outputs and the f64 `sums` carry a sentinel tail; with C_valid < C gamma,
dgamma and dbeta are C_valid long plus that tail, and the merged entry runs with a NaN tail behind gamma.

Shapes: pixels in {1, 7, 64, 257, 4100} x C in {8, 24, 48, 72, 264} (16-bit) / {4, 12, 24, 72, 264} (f32): C / VE = 1 (one
channel group, 256 pixel rows per block), 3, 6, 9 and 33 / 66 (groups that do not divide the 256 threads: idle threads), pixel
counts below the rows of a block, and 4100 pixels, where the second slot of the two-pixels-in-flight loop is filled for some
threads only.  One case per dtype has C / VE = 257 at 9 pixels: two channel blocks, the second with one live group.

Modes per shape and activation: forward with and without the residual; backward with BatchNorm at C_valid = C and C_valid =
C - 3 (C - 1 for C = 4), scale / shift / mean / invstd being what dy_bn_finalize_valid would give for z (eps 1e-3; 0 on the pad
channels) rounded to f32; backward without BatchNorm (has_bn = 0, NULL scale / shift / mean / invstd / gamma: the bias gradient
and activation backward of a conv without BatchNorm); pixels = 0 (apply writes dbeta / dgamma from the given sums and nothing
else; forward and reduce return 0 and touch nothing).  `sums` is compared as the total over its DY_BN_BWD_REPLICAS replicas.
Repeated runs are not compared bit for bit (the cross-block f64 atomics promise no order); dy_bn_act_bwd_apply and
dy_bn_act_bwd_apply_valid(C_valid = C) run from one `sums` of one reduce and must give identical bytes.

LeakyReLU: the inputs are moved off the kink on the host as in test_gpu_bn2act.py and the test asserts that the float64
reference has no |u| < 1e-3 on a real channel (pad channels have u = 0 * z + 0 exactly, in the kernel as in the reference, and both
take the slope 0.1 there).  No element is left out of a comparison.

Error measure: |got - ref64| / sum |terms| (bnact_ref's *_terms).  Rule: 2e-6 for f32 outputs, the same plus one ulp of the type
at the reference value for 16-bit outputs.  E is the error in the same measure of bnact_ref's formula run by torch on the CPU in
f32 on the same rounded inputs (16-bit outputs rounded to the type), against float64; the kernel is allowed max(rule, 4 E).
Every case prints its FIG line.  Measured worst error / allowance (f32 / bf16 / f16): dy_bn_act_fwd 0.084 / 0.25 / 0.25,
dy_bn_act_bwd_reduce 0.082 / 0.081 / 0.174, dy_bn_act_bwd_apply_valid 0.238 / 0.25 / 0.25, dy_bn_act_bwd[_valid] 0.072 / 0.25 /
0.25 (0.25 in a 16-bit type: the kernel's rounded output differs from float64 exactly as the f32 run's does).
"""
import re

import pytest
import torch

import bnact_ref as br
from repc3_ref import ACT_LEAKY
from frontend_ref import ulp
from test_gpu_bn2act import ACTS, DT, SENTINEL, Slice, _call, _check, _report, _rn, _rng, _round, _tail

pytestmark = pytest.mark.gpu

PX = (1, 7, 64, 257, 4100)
C_OF = {"bf16": (8, 24, 48, 72, 264), "f16": (8, 24, 48, 72, 264), "f32": (4, 12, 24, 72, 264)}
CASES = [(px, C, dt) for px in PX for dt in DT for C in C_OF[dt]] + [(9, 1028, "f32"), (9, 2056, "bf16"), (9, 2056, "f16")]
F32 = torch.float32


def _replicas():
    from dedark_yolo_amd import _C
    return _C.BN_BWD_REPLICAS


def _sums(C):
    """zeroed [replica][2C] f64 accumulators with a sentinel tail"""
    t = torch.zeros(_replicas() * 2 * C + 16, dtype=torch.float64, device="cuda")
    t[-16:] = SENTINEL
    return t


def _vec(v, fill=SENTINEL):
    """the f32 per-channel input `v` on the device, exactly len(v) long with 16 floats of `fill` right behind it"""
    t = torch.full((v.numel() + 16,), fill, device="cuda", dtype=F32)
    t[:v.numel()] = v.float().cuda()
    return t


def _off_the_kink(z, scale, shift, dt):
    """z with the elements whose u = z scale + shift lies within 2e-3 of LeakyReLU's kink moved away from it (scale / shift stay)"""
    z = z.clone()
    sc = torch.ones(z.shape[1], dtype=torch.float64) if scale is None else scale.double()
    for _ in range(40):
        u = br._u(z.double(), None if scale is None else sc, None if shift is None else shift.double())
        bad = (u.abs() < 2e-3) & (sc != 0)
        if not bool(bad.any()):
            break
        step = (4e-3 / sc.abs().clamp_min(1e-30)).expand_as(u)
        if dt != "f32":
            step = torch.maximum(step, 2 * ulp(z.double(), DT[dt]))
        sgn = torch.where(u >= 0, 1.0, -1.0) * torch.sign(sc)
        z = torch.where(bad, _round((z.double() + sgn * step).float(), dt), z)
    return z


def _stats(z, gamma, beta, Cv):
    """(scale, shift, mean, invstd) as f32 [C] vectors: dy_bn_finalize_valid's for the raw map z with Cv real channels"""
    C = z.shape[1]
    out = [torch.zeros(C) for _ in range(4)]
    for dst, src in zip(out, br.bn_stats(z[:, :Cv], gamma[:Cv], beta[:Cv])):
        dst[:Cv] = src.float()
    return out


def _inputs(px, C, dt, code, key):
    g = _rng(key, px, C, dt, code)
    gamma, beta = _rn(g, "f32", C, shift=1.0, scale=0.3), _rn(g, "f32", C, scale=0.3)
    z = _rn(g, dt, px, C, scale=1.5, shift=0.3)
    return z, _rn(g, dt, px, C), _rn(g, dt, px, C), gamma, beta


def _assert_off_kink(code, z, scale, shift, Cv):
    if code == ACT_LEAKY:
        u = br._u(z.double(), None if scale is None else scale.double(), None if shift is None else shift.double())
        assert float(u[:, :Cv].abs().min()) >= 1e-3, "LeakyReLU case: an element sits on the kink"


def _same_bytes(a, b, what):
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), what


def _tails_intact(tag, *pairs):
    for t, n in pairs:
        assert bool((t[n:] == SENTINEL).all()), f"{tag}: a per-channel output was written past its end"


def _forward_modes(tag, px, C, dt, code, z, res, stats, figs):
    from dedark_yolo_amd import ops
    dtype, did = DT[dt], ops.dt_id(DT[dt])
    sc, sh = stats[0], stats[1]
    _assert_off_kink(code, z, sc, sh, C)
    zv, rv = Slice(px, C, dtype, C + 16, z), Slice(px, C, dtype, C + 8, res)
    dsc, dsh = _vec(sc), _vec(sh)
    for name, r, rslice in (("y", None, None), ("y+res", res, rv)):
        yv = Slice(px, C, dtype, C + 16)
        _call("dy_bn_act_fwd", zv.ptr, zv.ld, dsc.data_ptr(), dsh.data_ptr(), code, rslice.ptr if rslice else None, rslice.ld if rslice else 0,
              yv.ptr, yv.ld, px, C, did)
        torch.cuda.synchronize()
        zv.unchanged(f"{tag} fwd z")
        rv.unchanged(f"{tag} fwd res")
        yv.guards_intact(f"{tag} fwd y")
        fa = (z, sc, sh, code, r)
        _check(f"{tag} fwd {name}", yv.get(), br.forward(*fa), br.forward_terms(*fa), _round(br.forward(*fa, dt=F32), dt), dt, figs)
    yv = Slice(px, C, dtype, C + 16)
    _call("dy_bn_act_fwd", zv.ptr, zv.ld, dsc.data_ptr(), dsh.data_ptr(), code, rv.ptr, rv.ld, yv.ptr, yv.ld, 0, C, did)      # pixels = 0
    torch.cuda.synchronize()
    yv.unchanged(f"{tag} fwd pixels=0")


def _backward_modes(tag, px, C, Cv, dt, code, has_bn, z, dy, stats, gamma, figs):
    """reduce -> apply_valid (-> apply from the same sums when Cv == C) -> pixels = 0 -> the merged entries (BatchNorm only)"""
    from dedark_yolo_amd import ops
    dtype, did, R = DT[dt], ops.dt_id(DT[dt]), _replicas()
    if has_bn:
        sc, sh, mu, inv = stats
        gm = gamma[:Cv]
    else:
        sc = sh = mu = inv = gm = None
    _assert_off_kink(code, z, sc, sh, Cv)
    ba = (dy, z, sc, sh, mu, inv, gm, code, has_bn, Cv)
    ref, terms, emu = br.backward(*ba), br.backward_terms(*ba), br.backward(*ba, dt=F32)
    zv, dyv = Slice(px, C, dtype, C + 16, z), Slice(px, C, dtype, C + 16, dy)
    aff = torch.stack(stats).contiguous().cuda() if has_bn else None               # [4, C]: scale | shift | mean | invstd
    ap = [aff[i].data_ptr() for i in range(4)] if has_bn else [None] * 4
    dgm = _vec(gm) if has_bn else None
    pgm = dgm.data_ptr() if has_bn else None

    def inputs_unchanged(step):
        zv.unchanged(f"{tag} {step} z")
        dyv.unchanged(f"{tag} {step} dy")
        if has_bn:
            assert torch.equal(aff.cpu(), torch.stack(stats)) and torch.equal(dgm[:Cv].cpu(), gm), f"{tag} {step}: a per-channel input changed"

    sums = _sums(C)
    _call("dy_bn_act_bwd_reduce", dyv.ptr, dyv.ld, zv.ptr, zv.ld, *ap, code, has_bn, sums.data_ptr(), 0, C, did)             # pixels = 0
    torch.cuda.synchronize()
    assert bool((sums[:-16] == 0).all()), f"{tag}: reduce with 0 pixels wrote sums"
    _call("dy_bn_act_bwd_reduce", dyv.ptr, dyv.ld, zv.ptr, zv.ld, *ap, code, has_bn, sums.data_ptr(), px, C, did)
    torch.cuda.synchronize()
    inputs_unchanged("reduce")
    _tails_intact(tag + " reduce", (sums, R * 2 * C))
    rep = sums[:R * 2 * C].view(R, 2, C)
    tot = rep.sum(0).cpu()
    _check(f"{tag} S0", tot[0], ref[3], terms[3], emu[3], "f32", figs)
    if has_bn:
        _check(f"{tag} S1", tot[1], ref[4], terms[4], emu[4], "f32", figs)
    else:
        assert bool((rep[:, 1] == 0).all()), f"{tag}: the second half of a replica was written without BatchNorm"
    sums0 = sums.clone()

    def apply(name, pixels, dz_ptr, dz_ld, extra):
        dg, db = _tail(Cv), _tail(Cv)
        _call(name, dyv.ptr, dyv.ld, zv.ptr, zv.ld, *ap, pgm, code, has_bn, sums.data_ptr(), dz_ptr, dz_ld, dg.data_ptr(), db.data_ptr(),
              pixels, C, *extra, did)
        torch.cuda.synchronize()
        inputs_unchanged(name)
        assert torch.equal(sums, sums0), f"{tag} {name}: sums changed"
        _tails_intact(f"{tag} {name}", (dg, Cv), (db, Cv))
        return dg, db

    def compare(what, dzv, dg, db):
        dzv.guards_intact(f"{tag} {what} dz")
        got = dzv.get()
        if has_bn:
            assert bool((got[:, Cv:] == 0).all()), f"{tag} {what}: dz of a pad channel is not 0"
        _check(f"{tag} {what} dz", got, ref[0], terms[0], _round(emu[0], dt), dt, figs)
        _check(f"{tag} {what} dbeta", db[:Cv].cpu(), ref[2], terms[2], emu[2], "f32", figs)
        if has_bn:
            _check(f"{tag} {what} dgamma", dg[:Cv].cpu(), ref[1], terms[1], emu[1], "f32", figs)
        else:
            assert bool((dg == SENTINEL).all()), f"{tag} {what}: dgamma written without BatchNorm"

    dzv = Slice(px, C, dtype, C + 8)
    dg, db = apply("dy_bn_act_bwd_apply_valid", px, dzv.ptr, dzv.ld, (Cv,))
    compare("apply_valid", dzv, dg, db)
    if Cv == C:                                 # the unsuffixed entry from the same sums: the same bytes
        dzu = Slice(px, C, dtype, C + 8)
        dgu, dbu = apply("dy_bn_act_bwd_apply", px, dzu.ptr, dzu.ld, ())
        dzu.guards_intact(f"{tag} apply dz")
        for a, b, w in ((dzu.parent, dzv.parent, "dz"), (dgu, dg, "dgamma"), (dbu, db, "dbeta")):
            _same_bytes(a, b, f"{tag}: dy_bn_act_bwd_apply and _valid(C_valid = C) differ in {w}")
    # pixels = 0: only the parameter gradients.  Without BatchNorm dz is dy itself, as ops._act_backward passes it for ACT_NONE.
    dz0 = Slice(px, C, dtype, C + 8)
    dg0, db0 = apply("dy_bn_act_bwd_apply_valid", 0, dz0.ptr if has_bn else dyv.ptr, dz0.ld if has_bn else dyv.ld, (Cv,))
    dz0.unchanged(f"{tag} apply pixels=0 dz")
    _same_bytes(db0, db, f"{tag}: dbeta of the pixels = 0 call")
    _same_bytes(dg0, dg, f"{tag}: dgamma of the pixels = 0 call")
    if not has_bn:
        return
    # the merged entries run their own reduce: compared with float64 only.  C_valid < C: a NaN tail right behind gamma.
    for name, extra in (("dy_bn_act_bwd_valid", (Cv,)),) + ((("dy_bn_act_bwd", ()),) if Cv == C else ()):
        gmm = _vec(gm, float("nan")) if Cv < C else dgm
        dzm, dgm_, dbm, sm = Slice(px, C, dtype, C + 8), _tail(Cv), _tail(Cv), _sums(C)
        _call(name, dyv.ptr, dyv.ld, zv.ptr, zv.ld, aff.data_ptr(), gmm.data_ptr(), code, sm.data_ptr(), dzm.ptr, dzm.ld, dgm_.data_ptr(),
              dbm.data_ptr(), px, C, *extra, did)
        torch.cuda.synchronize()
        inputs_unchanged(name)
        _tails_intact(f"{tag} {name}", (dgm_, Cv), (dbm, Cv), (sm, R * 2 * C))
        compare(name[3:], dzm, dgm_, dbm)


@pytest.mark.parametrize("px,C,dt", CASES)
def test_bn_act_kernels(px, C, dt):
    figs = []
    Cv = C - 1 if C == 4 else C - 3
    for name, code in ACTS.items():
        tag = f"px={px} C={C} {dt} {name}"
        z, dy, res, gamma, beta = _inputs(px, C, dt, code, "bnact")
        full, part = _stats(z, gamma, beta, C), _stats(z, gamma, beta, Cv)
        z_bn, z_id = z, z
        if code == ACT_LEAKY:                   # (the statistics stay as given: the stage takes them as inputs)
            z_bn, z_id = _off_the_kink(z, full[0], full[1], dt), _off_the_kink(z, None, None, dt)
        _forward_modes(tag, px, C, dt, code, z_bn, res, full, figs)
        _backward_modes(f"{tag} bn Cv={C}", px, C, C, dt, code, 1, z_bn, dy, full, gamma, figs)
        _backward_modes(f"{tag} bn Cv={Cv}", px, C, Cv, dt, code, 1, z_bn, dy, part, gamma, figs)
        _backward_modes(f"{tag} nobn Cv={C}", px, C, C, dt, code, 0, z_id, dy, None, None, figs)
        _backward_modes(f"{tag} nobn Cv={Cv}", px, C, Cv, dt, code, 0, z_id, dy, None, None, figs)
    _report(figs)


# ---------------------------------------------------------------------------------------------------------- bad arguments
_ENTRIES = {
    "dy_bn_act_fwd": "z z_ld sc sh act res res_ld y y_ld px C did",
    "dy_bn_act_bwd_reduce": "dy dy_ld z z_ld sc sh mu inv act has_bn sums px C did",
    "dy_bn_act_bwd_apply_valid": "dy dy_ld z z_ld sc sh mu inv gamma act has_bn sums dz dz_ld dg db px C Cv did",
    "dy_bn_act_bwd_apply": "dy dy_ld z z_ld sc sh mu inv gamma act has_bn sums dz dz_ld dg db px C did",
    "dy_bn_act_bwd_valid": "dy dy_ld z z_ld aff gamma act sums dz dz_ld dg db px C Cv did",
    "dy_bn_act_bwd": "dy dy_ld z z_ld aff gamma act sums dz dz_ld dg db px C did",
}
_BWD = ("dy_bn_act_bwd_reduce", "dy_bn_act_bwd_apply_valid", "dy_bn_act_bwd_apply", "dy_bn_act_bwd_valid", "dy_bn_act_bwd")


@pytest.mark.parametrize("dt", list(DT))
def test_bn_act_bad_arguments(dt):
    """C not a whole number of vectors, ld < C, a pointer off 16 bytes, NULL sums, has_bn = 1 with NULL mean, C_valid outside 1..C,
    NULL aff: a non-zero return whose message starts with the entry's name (the merged entries may name the pass that refused),
    and nothing written: not the outputs, not their guards, not sums."""
    from dedark_yolo_amd import ops
    dtype, did = DT[dt], ops.dt_id(DT[dt])
    px, C, ve = 5, 24, ops.vec_elems(DT[dt])
    es = torch.empty(0, dtype=dtype).element_size()
    g = _rng("bad", dt)
    z, dy, res = (_rn(g, dt, px, C) for _ in range(3))
    zv, dyv, rv = Slice(px, C, dtype, C + 16, z), Slice(px, C, dtype, C + 16, dy), Slice(px, C, dtype, C + 8, res)
    yv, dzv = Slice(px, C, dtype, C + 16), Slice(px, C, dtype, C + 8)
    aff = torch.stack(_stats(z, torch.ones(C), torch.zeros(C), C)).contiguous().cuda()
    gamma, sums, dg, db = _vec(torch.ones(C)), _sums(C), _tail(C), _tail(C)
    sums0 = sums.clone()
    good = dict(z=zv.ptr, z_ld=zv.ld, dy=dyv.ptr, dy_ld=dyv.ld, res=rv.ptr, res_ld=rv.ld, y=yv.ptr, y_ld=yv.ld, dz=dzv.ptr, dz_ld=dzv.ld,
                sc=aff[0].data_ptr(), sh=aff[1].data_ptr(), mu=aff[2].data_ptr(), inv=aff[3].data_ptr(), aff=aff.data_ptr(),
                gamma=gamma.data_ptr(), sums=sums.data_ptr(), dg=dg.data_ptr(), db=db.data_ptr(), act=1, has_bn=1, px=px, C=C, Cv=C, did=did)
    bad = [("C not whole vectors", dict(C=ve + ve // 2, Cv=ve), tuple(_ENTRIES)),
           ("ld < C (z)", dict(z_ld=C - ve), tuple(_ENTRIES)),
           ("ld < C (dy)", dict(dy_ld=C - ve), _BWD),
           ("ld < C (y)", dict(y_ld=C - ve), ("dy_bn_act_fwd",)),
           ("ld < C (res)", dict(res_ld=C - ve), ("dy_bn_act_fwd",)),
           ("ld < C (dz)", dict(dz_ld=C - ve), _BWD[1:]),
           ("z off 16 bytes", dict(z=zv.ptr + es), tuple(_ENTRIES)),
           ("y off 16 bytes", dict(y=yv.ptr + es), ("dy_bn_act_fwd",)),
           ("dz off 16 bytes", dict(dz=dzv.ptr + es), _BWD[1:]),
           ("NULL sums", dict(sums=None), _BWD),
           ("has_bn with NULL mean", dict(mu=None), _BWD[:3]),
           ("C_valid = 0", dict(Cv=0), ("dy_bn_act_bwd_apply_valid", "dy_bn_act_bwd_valid")),
           ("C_valid = C + 1", dict(Cv=C + 1), ("dy_bn_act_bwd_apply_valid", "dy_bn_act_bwd_valid")),
           ("NULL aff", dict(aff=None), ("dy_bn_act_bwd_valid", "dy_bn_act_bwd"))]
    for what, change, entries in bad:
        for name in entries:
            a = dict(good, **change)
            with pytest.raises(RuntimeError) as ei:
                _call(name, *(a[k] for k in _ENTRIES[name].split()))
            msg = re.sub(r"^.*?\(rc=-?\d+\): ", "", str(ei.value))                   # the library's own message
            base = name[:-len("_valid")] if name.endswith("_valid") else name
            assert msg.startswith(base), f"{what}: {name} said {msg!r}"
            torch.cuda.synchronize()
            for s in (zv, dyv, rv, yv, dzv):
                s.unchanged(f"{what}: {name}")
            assert torch.equal(sums, sums0), f"{what}: {name} wrote sums"
            assert bool((dg == SENTINEL).all()) and bool((db == SENTINEL).all()), f"{what}: {name} wrote a parameter gradient"
    # and the same arguments unchanged are accepted
    for name in _ENTRIES:
        _call(name, *(good[k] for k in _ENTRIES[name].split()))
    torch.cuda.synchronize()
