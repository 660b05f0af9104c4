"""GPU tests of the fused attention kernels (csrc/attn.hip) through the C-ABI: dy_attn_fwd and dy_attn_bwd in fp32, bf16 and fp16
against the float64 statement tests/attn_ref.py, computed from the same (rounded) inputs.

Views: Q | K | V are the three C-channel slices of ONE [B, L, 3C + 16] buffer filled with a sentinel, 8 guard channels on both sides
(so guards also lie between consecutive tokens and between the batches); O and dO are slices of [B, L, C + 16] buffers and
dQ | dK | dV slices of a second [B, L, 3C + 16] one.  Every guard element and every input must be unchanged after every call.  One case
per dtype shifts the slices to lane 3, where neither pointer nor pitch allow a 16-byte load.

Shapes (L, D, H, B): L = 1; 9; 63 / 64 / 65 around the 64-row tile (65 with D = 72, the m scale's head: D padded to 96 in LDS, two
query tiles, a swept tile with one live key); 130 (three tiles); 400 (the P5 map at 640^2); D = 8 (the smallest), 32, 72, 128 (the
largest); H = 1 and 4; B = 1 and 3.

Inputs: "random" N(0, 1); "equal": all keys equal, so every row of logits is constant (P = 1 / L exactly representable or not);
"spike_last" / "spike_first": one key whose logit is 60 above the rest after scaling, in the last / the first swept tile (the
running maximum jumps at the end / never moves again); "big" (fp32 only): scale * S of standard deviation 80.

Error measure: |got - ref64| / sum |terms| (tests/test_gpu_scc2f.py's measure; the terms are attn_ref.forward_terms /
backward_terms).  Rule: 2e-6 for f32 outputs (the bound tests/test_gpu_scc2f.py holds f32 MFMA sums to), the same plus one ulp of
the type at the reference value for 16-bit outputs.  That rule does not cover the exp evaluation (an f32 error of S times scale is a
RELATIVE error of P) nor the rounding of P / dS to the operand type in the 16-bit modes, so E, the error in the same measure of a
torch CPU run of the same formula in f32 (16-bit modes: P, dS and the outputs rounded to the type), is computed per case and the
kernel is allowed max(rule, 4 E) (tests/test_gpu_optimizers.py's form; the 4 leaves room for another summation order, no more).
Every case prints its measured error / allowance.
"""
import numpy as np
import pytest
import torch

import attn_ref as ar
from frontend_ref import ulp

pytestmark = pytest.mark.gpu

RULE = 2e-6
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENTINEL = 99.0
GUARD = 8

#          L,  D, H, B
SHAPES = [(1, 8, 1, 1), (9, 32, 4, 3), (63, 72, 1, 1), (64, 128, 1, 3), (65, 72, 4, 3), (130, 32, 4, 1), (400, 32, 4, 1), (400, 128, 1, 1),
          (130, 8, 4, 3)]
SPECIAL = [("equal", (65, 72, 4, 3)), ("equal", (64, 128, 1, 3)), ("spike_last", (130, 32, 4, 1)), ("spike_first", (130, 32, 4, 1)),
           ("spike_last", (65, 72, 4, 3)), ("spike_last", (9, 32, 4, 3))]
CASES = [("random", s, dt, GUARD) for s in SHAPES for dt in DT] + [(kind, s, dt, GUARD) for kind, s in SPECIAL for dt in DT] + \
        [("big", (130, 32, 4, 1), "f32", GUARD), ("big", (65, 72, 4, 3), "f32", GUARD)] + [("random", (65, 72, 4, 3), dt, 3) for dt in DT]


def _inputs(kind, L, D, H, B, dt):
    import zlib
    g = np.random.default_rng(zlib.crc32(repr((kind, L, D, H, B, dt)).encode()))
    C = H * D

    def rn(*shape, scale=1.0):
        return torch.from_numpy((scale * g.standard_normal(shape)).astype(np.float32)).to(DT[dt]).float()

    q, k, v, do = rn(B, L, C), rn(B, L, C), rn(B, L, C), rn(B, L, C)
    if kind == "equal":
        k = k[:, :1].expand(B, L, C).contiguous()
    elif kind in ("spike_last", "spike_first"):
        # every query of a head is the ones vector: logit_j = scale * sum_d k_jd; the spike key carries 60 / (scale D) per channel
        q = torch.ones(B, L, C)
        k = rn(B, L, C, scale=0.25)
        j = L - 1 if kind == "spike_last" else 0
        k[:, j] = torch.tensor(60.0 / (D ** -0.5 * D)).to(DT[dt]).float()
    elif kind == "big":
        q, k = rn(B, L, C, scale=80 ** 0.5), rn(B, L, C, scale=80 ** 0.5)
    return q, k, v, do


class Slices:
    """n slices of C channels in one [B, L, c0 + n C + tail] sentinel-filled parent"""

    def __init__(self, B, L, C, n, dtype, c0, fills=None):
        self.C, self.n, self.c0 = C, n, c0
        self.ld = c0 + n * C + GUARD
        self.parent = torch.full((B, L, self.ld), SENTINEL, device="cuda", dtype=dtype)
        for i, f in enumerate(fills or ()):
            self.parent[..., c0 + i * C:c0 + (i + 1) * C] = f.to(dtype).cuda()
        self.before = self.parent.clone()

    def ptr(self, i):
        return self.parent.data_ptr() + (self.c0 + i * self.C) * self.parent.element_size()

    def get(self, i):
        return self.parent[..., self.c0 + i * self.C:self.c0 + (i + 1) * self.C].double().cpu().numpy()

    def guards_intact(self, what):
        p = self.parent
        assert bool((p[..., :self.c0] == SENTINEL).all()) and bool((p[..., self.c0 + self.n * self.C:] == SENTINEL).all()), f"{what}: guard changed"

    def unchanged(self, what):
        assert torch.equal(self.parent, self.before), f"{what}: input buffer changed"


def _call(name, *args):
    from dedark_yolo_amd import _C, ops
    _C.call(name, *args, ops.stream())


def _measure(got, ref, terms, dt):
    """f32: max |got - ref| / terms (to be compared with RULE); 16-bit: max |got - ref| / (RULE terms + ulp(ref)) (with 1)"""
    got, ref, terms = (torch.as_tensor(np.asarray(t, dtype=np.float64)) for t in (got, ref, terms))
    assert got.shape == ref.shape == terms.shape and bool(torch.isfinite(got).all())
    if dt == "f32":
        return float(((got - ref).abs() / terms.clamp_min(1e-300)).max())
    return float(((got - ref).abs() / (RULE * terms + ulp(ref, DT[dt]))).max())


def _check(what, got, ref, terms, emu, dt, figs):
    rule = RULE if dt == "f32" else 1.0
    e, E = _measure(got, ref, terms, dt), _measure(emu, ref, terms, dt)
    bound = max(rule, 4 * E)
    print(f"FIG {what}: err {e:.3e} bound {bound:.3e} (rule {rule:.0e}, E {E:.3e}) ratio {e / bound:.3f}")
    figs.append((what, e, bound))


def _emulate(q, k, v, o, do, lse, H, dt):
    """torch CPU, f32 arithmetic, the kernel's formula; 16-bit modes round P, dS and the outputs to the type"""
    B, L, C = q.shape
    D = C // H
    scale = D ** -0.5
    rd = (lambda t: t) if dt == "f32" else (lambda t: t.to(DT[dt]).float())
    hd = lambda t: t.float().reshape(B, L, H, D).permute(0, 2, 1, 3)
    tk = lambda t: t.permute(0, 2, 1, 3).reshape(B, L, C)
    qh, kh, vh, oh, doh = hd(q), hd(k), hd(v), hd(o), hd(do)
    s = (qh @ kh.transpose(2, 3)) * scale
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    out = rd(tk((rd(e) @ vh) / l))
    lse_e = (m + torch.log(l))[..., 0]
    p = torch.exp(s - lse.float()[..., None])
    ds = p * (doh @ vh.transpose(2, 3) - (doh * oh).sum(-1, keepdim=True))
    p, ds = rd(p), rd(ds)
    dv = rd(tk(p.transpose(2, 3) @ doh))
    dq = rd(tk(ds @ kh) * scale)
    dk = rd(tk(ds.transpose(2, 3) @ qh) * scale)
    return [t.double().numpy() for t in (out, lse_e, dq, dk, dv)]


@pytest.mark.parametrize("kind,shape,dt,c0", CASES, ids=lambda p: "x".join(map(str, p)) if isinstance(p, tuple) else str(p))
def test_attn_kernels(kind, shape, dt, c0):
    from dedark_yolo_amd import ops
    L, D, H, B = shape
    C, dtype, did, scale = H * D, DT[dt], ops.dt_id(DT[dt]), D ** -0.5
    tag = f"{kind} L={L} D={D} H={H} B={B} {dt} lane {c0}"
    q, k, v, do = _inputs(kind, L, D, H, B, dt)
    o64, lse64, p64 = ar.forward(q.numpy(), k.numpy(), v.numpy(), H)
    if kind == "big":
        assert float(np.abs(scale * np.einsum("bihd,bjhd->bhij", q.reshape(B, L, H, D).numpy(), k.reshape(B, L, H, D).numpy())).max()) > 80
    if kind.startswith("spike"):
        srt = np.sort(np.log(p64.clip(1e-300)), -1)
        assert float((srt[..., -1] - srt[..., -2]).min()) > 55, "the spike is not 60 above the rest"

    # forward
    qkv = Slices(B, L, C, 3, dtype, c0, (q, k, v))
    ov = Slices(B, L, C, 1, dtype, c0)
    lse = torch.full((B * H * L + 16,), SENTINEL, device="cuda", dtype=torch.float32)
    _call("dy_attn_fwd", qkv.ptr(0), qkv.ld, qkv.ptr(1), qkv.ld, qkv.ptr(2), qkv.ld, ov.ptr(0), ov.ld, lse.data_ptr(), B, L, H, D, scale, did)
    torch.cuda.synchronize()
    qkv.unchanged(tag + " fwd")
    ov.guards_intact(tag + " fwd o")
    assert bool((lse[B * H * L:] == SENTINEL).all()), "lse: wrote past the end"

    # the backward's inputs: O and LSE as a forward would have stored them (rounded), the reference uses the same
    o_in = torch.from_numpy(o64).to(dtype).float()
    lse_in = torch.from_numpy(lse64).float()
    emu = _emulate(q, k, v, o_in, do, lse_in, H, dt)
    figs = []
    _check(tag + " O", ov.get(0), o64, ar.forward_terms(p64, v.numpy(), H), emu[0], dt, figs)
    # LSE (f32 in every mode): the logits' terms are scale sum_d |q_id| |k_jd|, the largest over j bounds the error of the log-sum-exp
    qa, ka = np.abs(q.numpy()).reshape(B, L, H, D), np.abs(k.numpy()).reshape(B, L, H, D)
    lt = scale * np.einsum("bihd,bjhd->bhij", qa, ka).max(-1) + 1.0
    _check(tag + " LSE", lse[:B * H * L].double().cpu().numpy().reshape(B, H, L), lse64, lt, emu[1], "f32", figs)

    # backward, twice: identical bytes
    o_v = Slices(B, L, C, 1, dtype, c0, (o_in,))
    do_v = Slices(B, L, C, 1, dtype, c0, (do,))
    lse_d = lse_in.cuda().contiguous()
    runs = []
    for _ in range(2):
        gv = Slices(B, L, C, 3, dtype, c0)
        _call("dy_attn_bwd", qkv.ptr(0), qkv.ld, qkv.ptr(1), qkv.ld, qkv.ptr(2), qkv.ld, o_v.ptr(0), o_v.ld, do_v.ptr(0), do_v.ld, lse_d.data_ptr(),
              gv.ptr(0), gv.ld, gv.ptr(1), gv.ld, gv.ptr(2), gv.ld, B, L, H, D, scale, did)
        torch.cuda.synchronize()
        gv.guards_intact(tag + " bwd")
        runs.append(gv)
    for s in (qkv, o_v, do_v):
        s.unchanged(tag + " bwd")
    assert torch.equal(runs[0].parent.view(torch.uint8), runs[1].parent.view(torch.uint8)), f"{tag}: two backward runs differ"
    args = (q.numpy(), k.numpy(), v.numpy(), o_in.numpy(), do.numpy(), lse_in.numpy(), H)
    refs = ar.backward(*args)[:3]
    terms = ar.backward_terms(*args)
    for i, name in enumerate(("dQ", "dK", "dV")):
        _check(f"{tag} {name}", runs[0].get(i), refs[i], terms[i], emu[2 + i], dt, figs)
    bad = [f"{w}: {e:.3e} > {b:.3e}" for w, e, b in figs if not e <= b]
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("dt", list(DT))
def test_attn_bad_arguments(dt):
    """D = 12, D = 136 and a pitch smaller than the slice: an error code, nothing launched (outputs keep the sentinel)"""
    from dedark_yolo_amd import ops
    dtype, did = DT[dt], ops.dt_id(DT[dt])
    B, L, H = 1, 9, 2
    for D, short in ((12, False), (136, False), (16, True)):
        C = H * D
        z = torch.zeros(B, L, C)
        qkv = Slices(B, L, C, 3, dtype, GUARD, (z, z, z))
        ov, gv = Slices(B, L, C, 1, dtype, GUARD), Slices(B, L, C, 3, dtype, GUARD)
        lse = torch.full((B * H * L,), SENTINEL, device="cuda", dtype=torch.float32)
        pitch = C - 8 if short else qkv.ld
        with pytest.raises(RuntimeError, match="dy_attn_fwd"):
            _call("dy_attn_fwd", qkv.ptr(0), pitch, qkv.ptr(1), qkv.ld, qkv.ptr(2), qkv.ld, ov.ptr(0), ov.ld, lse.data_ptr(), B, L, H, D, D ** -0.5, did)
        with pytest.raises(RuntimeError, match="dy_attn_bwd"):
            _call("dy_attn_bwd", qkv.ptr(0), qkv.ld, qkv.ptr(1), qkv.ld, qkv.ptr(2), qkv.ld, ov.ptr(0), ov.ld, ov.ptr(0), ov.ld, lse.data_ptr(),
                  gv.ptr(0), gv.ld, gv.ptr(1), pitch if short else gv.ld, gv.ptr(2), gv.ld, B, L, H, D, D ** -0.5, did)
        torch.cuda.synchronize()
        for s in (qkv, ov, gv):
            s.unchanged(f"D={D} {dt}")
        assert bool((lse == SENTINEL).all())
