"""GPU tests of the channel / spatial attention kernels (csrc/cbam.hip) through the C-ABI, every entry alone, in fp32, bf16 and fp16
against the float64 statement tests/cbam_ref.py computed from the same (rounded) inputs: dy_chan_pool_fwd, dy_chan_gate_fwd, dy_spatial_stats_fwd,
dy_spatial_gate_fwd, dy_spatial_gate_bwd_px, dy_spatial_conv_bwd, dy_spatial_gate_bwd_reduce and dy_spatial_gate_bwd_apply (the last
two also without planes: ChannelAttention's backward).  Each backward entry is fed the statement's planes rounded to f32, as a
forward would have stored them, so an entry answers for its own arithmetic only.

Views: x / y / dy / dx are C-channel slices of sentinel-filled [B, H W, C + 16] parents, a / da / dpool slices of [B, C + 16] ones, 8
guard channels on both sides; guards and inputs must be unchanged after every call.  One case per dtype is shifted to lane 3, where
neither pointer nor pitch allows a 16-byte access (the element path).

Shapes (B, H, W, C): (1, 1, 1, 8) a map smaller than the tap radius; (2, 3, 5, 24) both extents below 7, C / VE not a power of two;
(3, 9, 11, 64); (2, 17, 33, 16): 17 x 33 is one pixel more than the plane convolution's 16 x 16 tile in each direction (two tiles
and a one-pixel rest along W) and, for the 8 x 8 tile of the gate forward, 2 and 4 tiles plus one pixel; (1, 20, 20, 256);
(1, 4, 4, 2048) the widest map (f32: 512 groups, two workgroups along the channels).  k = 3 and 7, gate present and absent.

Inputs: "random" N(0, 1); "negative": every x < 0 (a running maximum that started from 0 would win); "equal": no gate and all
channels equal, so the tie rule decides every pixel; "saturated": logits of +-40.  Random inputs are adjusted BEFORE anything is
computed so that the f64 gap between the largest and the second largest u_c is at least 1e-3 max|u| at every pixel (the runner-up
is bumped down where it is not): a near-tie would move a whole dmax between two channels and say nothing about the kernel.

Measure: |got - ref64| / sum |terms| (tests/test_gpu_attn.py's).  Rule: 2e-6 for f32 outputs, the same plus one ulp of the type at
the reference value for 16-bit outputs.  The rule does not cover the sigmoid (an f32 error of its argument is a relative error of
its value), so E, the error in the same measure of a torch CPU f32 run of the same formula (outputs rounded to the type in the
16-bit modes), is computed per case and the kernel is allowed max(rule, 4 E).  Every case prints error / allowance.  The argmax
plane must equal the statement's exactly, and two runs of every backward entry must give identical bytes.
"""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cbam_ref as cr
from frontend_ref import ulp

pytestmark = pytest.mark.gpu

RULE = 2e-6
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENTINEL = 99.0
GUARD = 8
GAP = 1e-3

SHAPES = [(1, 1, 1, 8), (2, 3, 5, 24), (3, 9, 11, 64), (2, 17, 33, 16), (1, 20, 20, 256), (1, 4, 4, 2048)]
CASES = [("random", s, k, gated, dt, GUARD) for s in SHAPES for k in (3, 7) for gated in (True, False) for dt in DT]
CASES += [(kind, s, 7, kind != "equal", dt, GUARD) for kind in ("negative", "equal", "saturated") for s in ((2, 3, 5, 24), (3, 9, 11, 64))
          for dt in DT]
CASES += [("random", (3, 9, 11, 64), k, True, dt, 3) for k in (3, 7) for dt in DT] + [("random", (2, 3, 5, 24), 7, False, dt, 3) for dt in DT]


def _round(t, dt):
    return torch.as_tensor(np.asarray(t, dtype=np.float64)).to(DT[dt]).double().numpy()


def _inputs(kind, shape, k, gated, dt):
    B, H, W, C = shape
    g = np.random.default_rng(zlib.crc32(repr((kind, shape, k, gated, dt)).encode()))
    x = g.standard_normal((B, H, W, C))
    a = g.standard_normal((B, C)) if gated else None
    if kind == "negative":
        x = -(np.abs(x) + 0.1)
    elif kind == "equal":
        x = np.repeat(x[..., :1], C, -1)
    elif kind == "saturated":
        x = np.abs(x) + 0.1                       # the two largest u_c of a pixel then lie among the +40 channels (0 and 1 at least)
        a = np.where(g.random((B, C)) < 0.5, 40.0, -40.0)
        a[:, :2] = 40.0
    x = _round(x, dt)
    a = None if a is None else _round(a, dt)
    if kind != "equal" and C > 1:
        gg = cr.gate(a, x)
        for it in range(40):
            u = x * gg
            thr = GAP * np.abs(u).max()
            order = np.argsort(u, -1)
            top, second = order[..., -1:], order[..., -2:-1]
            gap = (np.take_along_axis(u, top, -1) - np.take_along_axis(u, second, -1))[..., 0]
            bad = gap < thr
            if not bad.any():
                break
            gs = np.take_along_axis(np.broadcast_to(gg, x.shape), second, -1)
            bumped = np.take_along_axis(x, second, -1) - (2.0 ** it) * 2 * thr / gs
            np.put_along_axis(x, second, np.where(bad[..., None], bumped, np.take_along_axis(x, second, -1)), -1)
            x = _round(x, dt)
        else:
            raise AssertionError("could not separate the two largest channels")
        if kind == "negative":
            assert (x < 0).all()
    w = g.standard_normal((1, 2, k, k)).astype(np.float32).astype(np.float64) * 0.2
    w = w.astype(np.float32).astype(np.float64)
    dy = _round(g.standard_normal((B, H, W, C)), dt)
    dpool = _round(g.standard_normal((B, C)) * H * W, dt) if gated else None
    prior = _round(g.standard_normal((B, H, W, C)), dt) if k == 3 else None
    return x, a, w, dy, dpool, prior


class Slice:
    """a [..., C] slice at lane c0 of a sentinel-filled [..., c0 + C + 8] parent"""

    def __init__(self, lead, C, dtype, c0, fill=None):
        self.C, self.c0, self.ld = C, c0, c0 + C + GUARD
        self.parent = torch.full((*lead, self.ld), SENTINEL, device="cuda", dtype=dtype)
        if fill is not None:
            self.parent[..., c0:c0 + C] = torch.as_tensor(fill).to(dtype).cuda()
        self.before = self.parent.clone()

    @property
    def ptr(self):
        return self.parent.data_ptr() + self.c0 * self.parent.element_size()

    def get(self):
        return self.parent[..., self.c0:self.c0 + self.C].double().cpu().numpy()

    def guards_intact(self, what):
        p = self.parent
        assert bool((p[..., :self.c0] == SENTINEL).all()) and bool((p[..., self.c0 + self.C:] == SENTINEL).all()), f"{what}: guard changed"

    def unchanged(self, what):
        assert torch.equal(self.parent, self.before), f"{what}: input buffer changed"


class Plane:
    """a dense f32 / int32 plane with 16 sentinel elements behind it"""

    def __init__(self, n, fill=None, dtype=torch.float32):
        self.n = n
        self.buf = torch.full((n + 16,), 77, device="cuda", dtype=dtype)
        if fill is not None:
            self.buf[:n] = torch.as_tensor(np.asarray(fill)).reshape(-1).to(dtype).cuda()
        self.before = self.buf.clone()

    ptr = property(lambda self: self.buf.data_ptr())

    def get(self, shape):
        return self.buf[:self.n].double().cpu().numpy().reshape(shape)

    def tail_intact(self, what):
        assert bool((self.buf[self.n:] == 77).all()), f"{what}: wrote past the end of a plane"

    def unchanged(self, what):
        assert torch.equal(self.buf, self.before), f"{what}: input plane changed"


def _call(name, *args):
    from dedark_yolo_amd import _C, ops
    _C.call(name, *args, ops.stream())
    torch.cuda.synchronize()


def _measure(got, ref, terms, dt):
    got, ref, terms = (torch.as_tensor(np.asarray(t, dtype=np.float64)) for t in (got, ref, terms))
    assert got.shape == ref.shape == terms.shape, (got.shape, ref.shape, terms.shape)
    assert bool(torch.isfinite(got).all())
    if dt == "f32":
        return float(((got - ref).abs() / terms.clamp_min(1e-300)).max())
    return float(((got - ref).abs() / (RULE * terms + ulp(ref, DT[dt]))).max())


def _check(what, got, ref, terms, emu, dt, figs):
    rule = RULE if dt == "f32" else 1.0
    e, E = _measure(got, ref, terms, dt), _measure(emu, ref, terms, dt)
    bound = max(rule, 4 * E)
    print(f"FIG {what}: err {e:.3e} bound {bound:.3e} (rule {rule:.0e}, E {E:.3e}) ratio {e / bound:.3f}")
    figs.append((what, e, bound))


def _emulate(x, a, w, dy, pl, dpool, prior, dt):
    """torch CPU, f32 arithmetic, the kernels' formulas on the same inputs; the 16-bit modes round the map outputs to the type"""
    t32 = lambda v: None if v is None else torch.as_tensor(np.asarray(v, dtype=np.float64)).float()
    rd = (lambda t: t) if dt == "f32" else (lambda t: t.to(DT[dt]).float())
    x, a, w, dy, dpool, prior = (t32(v) for v in (x, a, w, dy, dpool, prior))
    pl = {k: (torch.as_tensor(v) if k == "arg" else t32(v)) for k, v in pl.items()}
    B, H, W, C = x.shape
    k = w.shape[-1]
    g = torch.sigmoid(a).reshape(B, 1, 1, C) if a is not None else torch.ones(B, 1, 1, C)
    u = x * g
    out = dict(mean=u.mean(-1), mx=u.max(-1).values)
    m = torch.stack([pl["mean"], pl["mx"]], 1)
    s = torch.sigmoid(F.conv2d(m, w, padding=k // 2)[:, 0])
    out.update(s=s, y=rd(u * s[..., None]), cy=rd(u))
    out["dpre"] = (dy * u).sum(-1) * (pl["s"] * (1 - pl["s"]))
    dm = F.conv_transpose2d(pl["dpre"][:, None], w, padding=k // 2)
    out.update(dmean=dm[:, 0], dmx=dm[:, 1], dw=torch.nn.grad.conv2d_weight(m, w.shape, pl["dpre"][:, None], padding=k // 2))
    hot = torch.arange(C).reshape(1, 1, 1, C) == pl["arg"][..., None]
    du = dy * pl["s"][..., None] + pl["dmean"][..., None] / C + hot * pl["dmx"][..., None]
    for tag, d in (("", du), ("c", dy)):
        if a is not None:
            out[tag + "da"] = rd(torch.sigmoid(a) * torch.sigmoid(-a) * (d * x).sum((1, 2)))
        dx = d * g
        if dpool is not None:
            dx = dx + dpool.reshape(B, 1, 1, C) / (H * W)
        if prior is not None:
            dx = dx + prior
        out[tag + "dx"] = rd(dx)
    return {k: v.double().numpy() for k, v in out.items()}


@pytest.mark.parametrize("kind,shape,k,gated,dt,c0", CASES, ids=lambda p: "x".join(map(str, p)) if isinstance(p, tuple) else str(p))
def test_cbam_kernels(kind, shape, k, gated, dt, c0):
    from dedark_yolo_amd import _C, ops
    B, H, W, C = shape
    HW, n = H * W, B * H * W
    dtype, did = DT[dt], ops.dt_id(DT[dt])
    tag = f"{kind} {shape} k={k} gate={gated} {dt} lane {c0}"
    x, a, w, dy, dpool, prior = _inputs(kind, shape, k, gated, dt)
    f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)

    # the statement, stage by stage, each stage from the previous one's planes as a forward would have stored them (f32)
    st = cr.stats(x, a)
    if kind != "equal":
        assert float(st["gap"].min()) >= GAP * np.abs(x * cr.gate(a, x)).max() * 0.999
    else:
        assert not st["arg"].any(), "first-index ties"
    mean_in, mx_in = f32(st["mean"]), f32(st["mx"])
    y64, s64, y_terms = cr.spatial_gate(x, a, mean_in, mx_in, w)
    pre_terms = cr.conv_planes(mean_in, mx_in, w)[1]
    s_in = f32(s64)
    dpre64, dpre_terms = cr.bwd_px(dy, x, a, s_in)
    dpre_in = f32(dpre64)
    dmean64, dmx64, dw64, dmean_t, dmx_t, dw_t = cr.conv_bwd(dpre_in, mean_in, mx_in, w)
    planes = dict(s=s_in, dmean=f32(dmean64), dmx=f32(dmx64), arg=st["arg"])
    emu = _emulate(x, a, w, dy, dict(planes, mean=mean_in, mx=mx_in, dpre=dpre_in), dpool, prior, dt)
    figs = []

    xv, dyv = Slice((B, HW), C, dtype, c0, x.reshape(B, HW, C)), Slice((B, HW), C, dtype, c0, dy.reshape(B, HW, C))
    av = Slice((B,), C, dtype, c0, a) if gated else None
    a_args = (av.ptr, av.ld) if gated else (None, 0)
    wd = torch.as_tensor(w, dtype=torch.float32).cuda().contiguous()
    inputs = [xv, dyv] + ([av] if gated else [])

    def intact(what, *outs):
        for v in inputs:
            v.unchanged(f"{tag} {what}")
        for o in outs:
            o.guards_intact(f"{tag} {what}") if isinstance(o, Slice) else o.tail_intact(f"{tag} {what}")

    # dy_spatial_stats_fwd
    mean_p, mx_p, arg_p = Plane(n), Plane(n), Plane(n, dtype=torch.int32)
    _call("dy_spatial_stats_fwd", xv.ptr, xv.ld, *a_args, mean_p.ptr, mx_p.ptr, arg_p.ptr, B, HW, C, did)
    intact("stats", mean_p, mx_p, arg_p)
    _check(tag + " mean", mean_p.get((B, H, W)), st["mean"], st["mean_terms"], emu["mean"], "f32", figs)
    _check(tag + " max", mx_p.get((B, H, W)), st["mx"], st["mx_terms"], emu["mx"], "f32", figs)
    assert np.array_equal(arg_p.get((B, H, W)).astype(np.int64), st["arg"].astype(np.int64)), f"{tag}: argmax plane differs"
    mx2 = Plane(n)
    _call("dy_spatial_stats_fwd", xv.ptr, xv.ld, *a_args, mean_p.ptr, mx2.ptr, None, B, HW, C, did)         # eval: no argmax plane
    assert torch.equal(mx2.buf, mx_p.buf)

    # dy_spatial_gate_fwd
    mean_d, mx_d = Plane(n, mean_in), Plane(n, mx_in)
    yv, s_p = Slice((B, HW), C, dtype, c0), Plane(n)
    _call("dy_spatial_gate_fwd", xv.ptr, xv.ld, *a_args, mean_d.ptr, mx_d.ptr, wd.data_ptr(), k, yv.ptr, yv.ld, s_p.ptr, B, H, W, C, did)
    intact("gate fwd", yv, s_p)
    mean_d.unchanged(tag), mx_d.unchanged(tag)
    _check(tag + " y", yv.get().reshape(B, H, W, C), y64, y_terms, emu["y"], dt, figs)
    _check(tag + " s", s_p.get((B, H, W)), s64, s64 * (1 + (1 - s64) * pre_terms), emu["s"], "f32", figs)
    y2 = Slice((B, HW), C, dtype, c0)
    _call("dy_spatial_gate_fwd", xv.ptr, xv.ld, *a_args, mean_d.ptr, mx_d.ptr, wd.data_ptr(), k, y2.ptr, y2.ld, None, B, H, W, C, did)   # eval: s not kept
    assert torch.equal(y2.parent.view(torch.uint8), yv.parent.view(torch.uint8))

    # dy_spatial_gate_bwd_px
    s_d = Plane(n, s_in)
    runs = []
    for _ in range(2):
        dpre_p = Plane(n)
        _call("dy_spatial_gate_bwd_px", dyv.ptr, dyv.ld, xv.ptr, xv.ld, *a_args, s_d.ptr, dpre_p.ptr, B, HW, C, did)
        intact("bwd px", dpre_p)
        runs.append(dpre_p)
    assert torch.equal(runs[0].buf.view(torch.uint8), runs[1].buf.view(torch.uint8)), f"{tag}: two dpre runs differ"
    _check(tag + " dpre", runs[0].get((B, H, W)), dpre64, dpre_terms, emu["dpre"], "f32", figs)

    # dy_spatial_conv_bwd
    dpre_d = Plane(n, dpre_in)
    need = int(_C.lib().dy_spatial_conv_bwd_workspace(B, H, W, k))
    assert need == B * -(-H // 16) * -(-W // 16) * 2 * k * k
    runs = []
    for _ in range(2):
        dmean_p, dmx_p, dw_p, ws = Plane(n), Plane(n), Plane(2 * k * k), Plane(need)
        _call("dy_spatial_conv_bwd", dpre_d.ptr, mean_d.ptr, mx_d.ptr, wd.data_ptr(), k, dmean_p.ptr, dmx_p.ptr, dw_p.ptr, ws.ptr, need, B, H, W)
        intact("conv bwd", dmean_p, dmx_p, dw_p, ws)
        runs.append((dmean_p, dmx_p, dw_p))
    for p, q in zip(*runs):
        assert torch.equal(p.buf.view(torch.uint8), q.buf.view(torch.uint8)), f"{tag}: two plane-convolution backward runs differ"
    _check(tag + " dmean", runs[0][0].get((B, H, W)), dmean64, dmean_t, emu["dmean"], "f32", figs)
    _check(tag + " dmax", runs[0][1].get((B, H, W)), dmx64, dmx_t, emu["dmx"], "f32", figs)
    _check(tag + " dw", runs[0][2].get((1, 2, k, k)), dw64, dw_t, emu["dw"], "f32", figs)

    # dy_spatial_gate_bwd_reduce / _apply, with the planes (CBAM, SpatialAttention) and without (ChannelAttention)
    dmean_d, dmx_d, arg_d = Plane(n, planes["dmean"]), Plane(n, planes["dmx"]), Plane(n, planes["arg"], torch.int32)
    pool_v = Slice((B,), C, dtype, c0, dpool) if gated else None
    pool_args = (pool_v.ptr, pool_v.ld) if gated else (None, 0)
    for pre, pl, pargs in (("", planes, (s_d.ptr, dmean_d.ptr, dmx_d.ptr, arg_d.ptr)), ("c", None, (None, None, None, None))):
        if pre == "c" and not gated:
            continue
        if gated:
            need = int(_C.lib().dy_cbam_reduce_workspace(B, HW, C, did))
            runs = []
            for _ in range(2):
                da_v, ws = Slice((B,), C, dtype, c0), Plane(need)
                _call("dy_spatial_gate_bwd_reduce", dyv.ptr, dyv.ld, xv.ptr, xv.ld, av.ptr, av.ld, *pargs, da_v.ptr, da_v.ld, ws.ptr, need, B, HW,
                      C, did)
                intact(pre + "reduce", da_v, ws)
                runs.append(da_v)
            assert torch.equal(runs[0].parent.view(torch.uint8), runs[1].parent.view(torch.uint8)), f"{tag}: two {pre}da runs differ"
            da64, da_t = cr.gate_reduce(dy, x, a, pl)
            _check(f"{tag} {pre}da", runs[0].get(), da64, da_t, emu[pre + "da"], dt, figs)
        runs = []
        for _ in range(2):
            dx_v = Slice((B, HW), C, dtype, c0, None if prior is None else prior.reshape(B, HW, C))
            _call("dy_spatial_gate_bwd_apply", dyv.ptr, dyv.ld, *a_args, *pargs, *pool_args, dx_v.ptr, dx_v.ld, 0 if prior is None else 1, B, HW, C, did)
            intact(pre + "apply", dx_v)
            runs.append(dx_v)
        assert torch.equal(runs[0].parent.view(torch.uint8), runs[1].parent.view(torch.uint8)), f"{tag}: two {pre}dx runs differ"
        dx64, dx_t = cr.gate_apply(dy, a, pl, dpool, prior)
        _check(f"{tag} {pre}dx", runs[0].get().reshape(B, H, W, C), dx64, dx_t, emu[pre + "dx"], dt, figs)
    for p in (s_d, dpre_d, dmean_d, dmx_d, arg_d, mean_d, mx_d) + ((pool_v,) if gated else ()):
        p.unchanged(tag)

    # dy_chan_pool_fwd (the pool in front of the fc), twice: identical bytes
    need = int(_C.lib().dy_cbam_reduce_workspace(B, HW, C, did))
    runs = []
    for _ in range(2):
        pv, ws = Slice((B,), C, dtype, c0), Plane(need)
        _call("dy_chan_pool_fwd", xv.ptr, xv.ld, pv.ptr, pv.ld, ws.ptr, need, B, HW, C, did)
        intact("pool", pv, ws)
        runs.append(pv)
    assert torch.equal(runs[0].parent.view(torch.uint8), runs[1].parent.view(torch.uint8)), f"{tag}: two pool runs differ"
    x32 = torch.as_tensor(x).float()
    pe = x32.mean((1, 2))
    _check(tag + " pool", runs[0].get(), x.mean((1, 2)), np.abs(x).mean((1, 2)), (pe if dt == "f32" else pe.to(dtype).float()).double().numpy(), dt, figs)

    # dy_chan_gate_fwd
    if gated:
        cy = Slice((B, HW), C, dtype, c0)
        _call("dy_chan_gate_fwd", xv.ptr, xv.ld, av.ptr, av.ld, cy.ptr, cy.ld, B, HW, C, did)
        intact("chan gate", cy)
        c64, c_t = cr.chan_gate(x, a)
        _check(tag + " chan y", cy.get().reshape(B, H, W, C), c64, c_t, emu["cy"], dt, figs)

    bad = [f"{wh}: {e:.3e} > {b:.3e}" for wh, e, b in figs if not e <= b]
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("dt", list(DT))
def test_cbam_bad_arguments(dt):
    """C = 12, C = 2056, k = 5 and a pitch smaller than the slice: an error code, nothing launched (outputs keep the sentinel)"""
    from dedark_yolo_amd import ops
    dtype, did = DT[dt], ops.dt_id(DT[dt])
    B, H, W = 1, 3, 3
    for C, k, short in ((12, 7, False), (2056, 7, False), (16, 5, False), (16, 7, True)):
        xv, yv, av = Slice((B, H * W), C, dtype, GUARD, 0.0), Slice((B, H * W), C, dtype, GUARD), Slice((B,), C, dtype, GUARD, 0.0)
        p, q, s = Plane(B * H * W, 0.0), Plane(B * H * W, 0.0), Plane(B * H * W)
        wd = torch.zeros(2 * 49, device="cuda")
        pitch = C - 8 if short else yv.ld
        with pytest.raises(RuntimeError, match="dy_spatial_gate_fwd"):
            _call("dy_spatial_gate_fwd", xv.ptr, xv.ld, av.ptr, av.ld, p.ptr, q.ptr, wd.data_ptr(), k, yv.ptr, pitch, s.ptr, B, H, W, C, did)
        if k == 7:
            with pytest.raises(RuntimeError, match="dy_spatial_stats_fwd"):
                _call("dy_spatial_stats_fwd", xv.ptr, C - 8 if short else xv.ld, av.ptr, av.ld, s.ptr, s.ptr, None, B, H * W, C, did)
            with pytest.raises(RuntimeError, match="dy_chan_gate_fwd"):
                _call("dy_chan_gate_fwd", xv.ptr, xv.ld, av.ptr, av.ld, yv.ptr, pitch, B, H * W, C, did)
            with pytest.raises(RuntimeError, match="dy_spatial_gate_bwd_apply"):
                _call("dy_spatial_gate_bwd_apply", xv.ptr, xv.ld, av.ptr, av.ld, None, None, None, None, None, 0, yv.ptr, pitch, 0, B, H * W, C, did)
        for v in (xv, yv, av, p, q, s):
            v.unchanged(f"C={C} k={k} {dt}")
