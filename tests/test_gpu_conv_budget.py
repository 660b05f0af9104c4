"""Every convolution kernel, per C-ABI entry, dtype and kernel symbol, against float64 on an element-wise error budget.

tests/conv_budget_ref.py states the budget, derives its constants from torch's f32 CPU convolution (not from these kernels)
and lists the cases: per entry (dy_conv2d_fwd / dy_conv2d_dgrad / dy_conv2d_wgrad) and dtype, every kernel symbol of
golden/g22_conv_routes.json on the smallest shape that reaches it, plus the dense, stem-forward, pixel-streaming and masked
parity-fallback kernels.  The reference is F.conv2d / torch.nn.grad in float64 on the GPU on the dtype-rounded operands,
evaluated in FULL for every case (the largest is 60 GFLOP per result): no probe set, every element of z, dx, dW and db is held
to its budget.

Per case: (1) z, dx, dW, db through ops.conv_forward / ops.conv_backward / dy_conv2d_wgrad, dW pre-filled with NaN and
bit-identical on a repeat; (2) the forward from a channel slice (NaN in the foreign lanes) into a channel slice of a wider
buffer (+inf in the foreign lanes on both sides), raw through ops.conv_forward(out=) and with scale / shift + SiLU through
the descriptor; (3) the data gradient from such a slice into a slice that holds values, with accumulate + add_src, and each
alone; (4) ragged channel counts: the pad lanes of z and dx are exactly 0 (what ops promises; the operands' own pad lanes
must be 0 by contract -- ops.padded_channels, dy_conv2d_wgrad in include/dedark_yolo.h -- so no garbage is placed there)
and the real rows and columns of dW are within budget.

Each line printed per check gives the worst ratio to the budget and the power margin: the mean single term (S / terms: one
pixel of dW or db, one channel of one tap of z or dx) over the budget, at the median element.  Below 4, one dropped term
sits inside the budget; the line then names the tail length estimated to stand out (random-sign terms add as sqrt(n): an
estimate, not a mutant that was run; tests/test_conv_budget_cpu.py runs a 32-pixel-tail mutant on the weak dW shapes).  The
margin is taken at the median element, which departs from the issue's "smallest contribution"; the 1st percentile is printed
next to it (conv_budget_ref.Report)."""
import ctypes as C
import json
import math
import os

import pytest
import torch

import conv_budget_ref as R

pytestmark = pytest.mark.gpu

ENTRIES = (R.FWD, R.DGRAD, R.WGRAD)
# data-gradient kernels that add `add_src` in their own epilogue (kRoutes of csrc/conv.hip: fuses_add; never for the parity
# classes of a stride-2 problem).  Every other route stores dx rounded and adds the view in a second pass (dy_copy2d): the
# budget of that result carries one more output rounding (conv_budget_ref.budget: rounded_before).
FUSES_ADD = ("px1x1_kernel", "v4::", "v5::")
# 16-bit kernels whose epilogue stages the finished tile in LDS in the OUTPUT type (conv_epilogue.h: store_tile / store_image /
# store_rows read the 16-bit image back, add the destination's old value and the addend in f32 and round again): with
# `accumulate` or a fused `add_src` the data gradient itself is rounded once before the sum is, so that result's budget carries
# u_out * |dx| on top.  The term is read off that code and c is untouched; what a run of this test recorded without it (up to
# 149 budgets at elements where dx + old + add cancels) is a finding about the kernels, not where the bound comes from.  px1x1_kernel, the conv_small.hip and dense.hip kernels and the f32 generic
# kernel add in f32 registers and get no such term.
STAGES_16BIT = ("conv_igemm_kernel", "conv_thin_kernel", "v2::", "v3::", "v4::", "v5::")
# forward kernels that take a raw epilogue only (dy_conv_stem_fwd_eligible, dy_conv_px_eligible: no scale / shift / act): the
# affine + SiLU run of their cases goes to another route, every other slice run stays on the kernel of the plain run
RAW_ONLY = ("stem_fwd_kernel", "px1x1_kernel")
_figures = {}          # entry -> [largest worst ratio, smallest power margin], for the closing printout


class _Tape:
    def __init__(self):
        self.stack, self.pgrads = [], {}

    def push(self, c):
        self.stack.append(c)

    def pop(self):
        return self.stack.pop()


class _Routes:
    """{C-ABI entry: kernel symbol it reported} of the ops calls inside the block"""

    def __enter__(self):
        from dedark_yolo_amd import _C
        _C._prof = []
        self.seen = {}
        return self.seen

    def __exit__(self, *exc):
        from dedark_yolo_amd import _C
        torch.cuda.synchronize()
        for name, _e0, _e1, _meta, kern in _C._prof:
            self.seen[name] = kern
        _C._prof = None


def _full(v, Cp):
    """the Cp-wide NHWC tensor behind a [B, C, H, W] view of its first lanes"""
    B, _, H, W = v.shape
    return v.as_strided((B, Cp, H, W), v.stride())


def _framed(v, Cp, fill):
    """v [B, C, H, W] copied into lanes [off, off + C) of a wider NHWC buffer (pad lanes up to off + Cp zero, every other lane
    `fill`): (buffer as [B, H, W, ld], the [B, C, H, W] view, off)"""
    from dedark_yolo_amd import ops
    B, Cc, H, W = v.shape
    ve = ops.vec_elems(v.dtype)
    off = 2 * ve
    wide = torch.full((B, H, W, off + Cp + ve), fill, dtype=v.dtype, device=v.device)
    wide[..., off:off + Cp] = 0
    wide[..., off:off + Cc] = v.permute(0, 2, 3, 1)
    return wide, wide.permute(0, 3, 1, 2)[:, off:off + Cc], off


def _foreign_untouched(wide, off, Cp, fill):
    lanes = torch.cat([wide[..., :off], wide[..., off + Cp:]], -1)
    return bool(torch.isnan(lanes).all()) if fill != fill else bool((lanes == fill).all())


def _note(cid, tag, entry, rep, sym=""):
    weak = ""
    if rep.margin < 4:
        weak = f"  WEAK: one term is inside the budget; estimated (not run as a mutant) that a tail of {math.ceil((4 / rep.margin) ** 2)} terms is not"
    print(f"{cid} {tag} [{sym}] {rep}{weak}")
    f = _figures.setdefault(entry, [0.0, float("inf"), "", ""])
    if rep.worst > f[0]:
        f[0], f[2] = rep.worst, f"{cid} {tag}"
    if rep.margin < f[1]:
        f[1], f[3] = rep.margin, f"{cid} {tag}"
    assert rep.worst <= 1.0, f"{cid} {tag} [{sym}] {rep}"


class _Case:
    """Operands, fp64 references (shared by every check of the case, never written to) and the plain run."""

    def __init__(self, case, cin_cut=0, cout_cut=0):
        from dedark_yolo_amd import ops
        self.name, self.shape, self.syms, self.has_bias = case
        self.cid = R.case_id(case) + (f"-cut{cin_cut}.{cout_cut}" if cin_cut or cout_cut else "")
        self.cuts = (cin_cut, cout_cut)
        self.dtype = dt = R.DTYPES[self.name]
        B, Cin, Cout, H, W, kh, kw, s, p, d, Ho, Wo = R.geometry(self.shape)
        self.Cin, self.Cout = Cin - cin_cut, Cout - cout_cut
        self.geo, self.k = (s, p, d), (kh, kw)
        self.dims = (B, H, W, Ho, Wo)
        ve = ops.vec_elems(dt)
        self.cin_pad, self.cout_pad = ops.round_up(self.Cin, ve), ops.round_up(self.Cout, ve)
        x, w, bias, gy = R.make_operands(self.shape, dt, "cuda", cin_cut, cout_cut)
        self.w = w
        self.bias = bias.requires_grad_(True) if self.has_bias else None
        self.xn, self.gn = ops.as_nhwc(x, dt), ops.as_nhwc(gy, dt)
        refs = R.conv_refs(x.to(dt), w.to(dt), gy.to(dt), None, s, p, d)
        self.acc, self.S_acc = refs["z"]                       # without the shift
        self.refs = refs
        if self.has_bias:
            b = bias.detach().double().view(1, -1, 1, 1)
            refs["z"] = (self.acc + b, self.S_acc + b.abs())
        self.planar = dt != torch.float32 and self.Cin <= 4      # ops.conv_backward writes the stem's dx planar

    def terms(self, name):
        return R.terms(name, self.shape, *self.cuts)

    def check(self, tag, name, got, sym="", ref=None, S=None, gain=1.0, rounded_before=None):
        if ref is None:
            ref, S = self.refs[name]
        out_dtype = self.dtype if name in ("z", "dx") else torch.float32
        rep = R.compare(name, got, ref, S, R.C_OF[name], out_dtype, self.terms(name), gain, rounded_before)
        _note(self.cid, tag, {"z": R.FWD, "dx": R.DGRAD, "dw": R.WGRAD, "db": "bias gradient"}[name], rep, sym)

    def wgrad(self, x, dz):
        """dy_conv2d_wgrad called directly into a NaN-filled dW: (dW, symbol)"""
        from dedark_yolo_amd import _C, ops
        B, H, W, Ho, Wo = self.dims
        (kh, kw), (s, p, d) = self.k, self.geo
        st = ops.stream()
        scratch = ops.wgrad_scratch(x.device, tag=st)
        gw = torch.full((self.Cout, self.Cin, kh, kw), float("nan"), device="cuda")
        _C.lib().dy_clear_last_kernel()
        _C.call("dy_conv2d_wgrad", ops.ptr(x), ops.ld_of(x), B, H, W, self.cin_pad, ops.ptr(dz), ops.ld_of(dz), Ho, Wo, self.cout_pad, kh, kw,
                s, p, d, self.Cout, self.Cin, ops.ptr(scratch), scratch.numel(), ops.ptr(gw), ops.dt_id(self.dtype), st)
        torch.cuda.synchronize()
        return gw, _C.lib().dy_last_kernel().decode()

    def plain(self):
        """(1): z, dx, db through ops, dW through the entry; the symbols the case is listed under; pad lanes of z and dx 0.
        Returns the context of the forward (the slice checks push it again) and the symbols taken."""
        from dedark_yolo_amd import ops
        s, p, d = self.geo
        tape = _Tape()
        with _Routes() as seen:
            y = ops.conv_forward(tape, self.xn, self.w, self.bias, None, 0, s, p, d, False)
            ctx = tape.stack[-1]
            dx = ops.conv_backward(tape, self.gn, need_dx=True)
        gw, wsym = self.wgrad(self.xn, self.gn)
        got = (seen.get(R.FWD, ""), seen.get(R.DGRAD, ""), wsym)
        for entry, want, have in zip(ENTRIES, self.syms, got):
            assert want is None or have == want, (self.cid, entry, want, have)
        self.check("plain", "z", y, got[0])
        self.check("plain", "dx", dx, got[1])
        self.check("plain", "dw", gw, got[2])
        again, _ = self.wgrad(self.xn, self.gn)
        assert torch.equal(gw, again), f"{self.cid}: dW differs between two runs"
        if self.has_bias:
            self.check("plain", "db", tape.pgrads[self.bias])
        if self.cout_pad != self.Cout:
            assert bool((_full(y, self.cout_pad)[:, self.Cout:] == 0).all()), f"{self.cid}: pad lanes of z are not 0"
        if self.cin_pad != self.Cin and not self.planar:
            assert bool((_full(dx, self.cin_pad)[:, self.Cin:] == 0).all()), f"{self.cid}: pad lanes of dx are not 0"
        if self.planar:
            assert tuple(dx.shape) == (self.dims[0], self.Cin) + self.dims[1:3] and dx.is_contiguous()
        return ctx, got

    def forward_slices(self, syms):
        """(2): both runs stay on the kernel of the plain run (asserted), except the affine run of a raw-only kernel (RAW_ONLY)."""
        from dedark_yolo_amd import _C, ops
        B, H, W, Ho, Wo = self.dims
        (kh, kw), (s, p, d) = self.k, self.geo
        dt = self.dtype
        inf = float("inf")
        _xw, xs, _ = _framed(self.xn, self.cin_pad, float("nan"))
        if syms[0] == "":                # dense.hip reads whole rows of taps (src_ld == Cs): full-width source, sliced destination
            xs = self.xn
        blank = torch.zeros(B, self.Cout, Ho, Wo, dtype=dt, device="cuda")
        # raw (the epilogue of the plain run), through ops
        wide, out, off = _framed(blank, self.cout_pad, inf)
        with _Routes() as seen:
            y = ops.conv_forward(None, xs, self.w, self.bias, None, 0, s, p, d, False, out=out)
        assert y.data_ptr() == out.data_ptr()
        assert seen.get(R.FWD, "") == syms[0], (self.cid, "slice raw", seen, syms[0])
        self.check("slice raw", "z", out, syms[0])
        assert _foreign_untouched(wide, off, self.cout_pad, inf), f"{self.cid}: forward wrote outside its channel slice"
        assert bool((wide[..., off + self.Cout:off + self.cout_pad] == 0).all()), f"{self.cid}: pad lanes of the slice are not 0"
        # scale / shift + SiLU, through the descriptor
        g = torch.Generator().manual_seed(self.Cout)
        scale, shift = torch.zeros(self.cout_pad, device="cuda"), torch.zeros(self.cout_pad, device="cuda")
        scale[:self.Cout] = (0.5 + torch.rand(self.Cout, generator=g)) * (1 - 2 * (torch.arange(self.Cout) % 3 == 0).float())
        shift[:self.Cout] = torch.randn(self.Cout, generator=g)
        wide, out, off = _framed(blank, self.cout_pad, inf)
        wp = ops._pack(self.w, self.cout_pad, self.cin_pad, False, dt)
        desc = ops._conv_desc(xs, wp, out, B, H, W, self.cin_pad, Ho, Wo, self.cout_pad, kh, kw, s, p, d, scale, shift, 1, None, False, dt)
        _C.lib().dy_clear_last_kernel()
        _C.call("dy_conv2d_fwd", C.byref(desc), ops.stream())
        torch.cuda.synchronize()
        sym = _C.lib().dy_last_kernel().decode()
        assert sym == syms[0] or syms[0] in RAW_ONLY, (self.cid, "slice affine+SiLU", sym, syms[0])
        sc, sh = scale[:self.Cout].double().view(1, -1, 1, 1), shift[:self.Cout].double().view(1, -1, 1, 1)
        self.check("slice affine+SiLU", "z", out, sym, ref=R.act_ref(sc * self.acc + sh, 1), S=sc.abs() * self.S_acc + sh.abs(), gain=R.LIPSCHITZ[1])
        assert _foreign_untouched(wide, off, self.cout_pad, inf), f"{self.cid}: forward (affine) wrote outside its channel slice"
        assert bool((wide[..., off + self.Cout:off + self.cout_pad] == 0).all()), f"{self.cid}: pad lanes of the slice are not 0 (affine)"

    def dgrad_slices(self, ctx, syms):
        """(3): dx_out a slice that holds values; accumulate + add_src, then each alone."""
        from dedark_yolo_amd import ops
        B, H, W, Ho, Wo = self.dims
        dt = self.dtype
        inf = float("inf")
        g = torch.Generator().manual_seed(self.Cin + 7)
        old = torch.randn(B, self.Cin, H, W, generator=g).to("cuda").to(dt)
        add = torch.randn(B, self.Cin, H, W, generator=g).to("cuda").to(dt)
        _gw, gs, _ = _framed(self.gn, self.cout_pad, float("nan"))
        _aw, adds, _ = _framed(add, self.cin_pad, float("nan"))
        dx_ref, S_dx = self.refs["dx"]
        for tag, acc, use_add in (("acc+add", True, True), ("acc", True, False), ("add", False, True)):
            wide, dxs, off = _framed(old, self.cin_pad, inf)
            tape = _Tape()
            tape.push(ctx)
            with _Routes() as seen:
                ops.conv_backward(tape, gs, need_dx=True, dx_out=dxs, accumulate=acc, add_src=adds if use_add else None)
            sym = seen.get(R.DGRAD, "")
            assert sym == syms[1], (self.cid, tag, sym, syms[1])
            two_pass = use_add and not (sym.startswith(FUSES_ADD) and self.geo[0] == 1)
            ref, S = dx_ref, S_dx
            before = torch.zeros_like(ref)                  # magnitudes stored in the output type before the last sum
            if (acc or (use_add and not two_pass)) and dt != torch.float32 and sym.startswith(STAGES_16BIT):
                before = before + ref.abs()
            if acc:
                ref, S = ref + old.double(), S + old.double().abs()
            if two_pass:
                before = before + ref.abs()
            if use_add:
                ref, S = ref + add.double(), S + add.double().abs()
            self.check("slice dgrad " + tag, "dx", dxs, sym, ref=ref, S=S, rounded_before=before)
            assert _foreign_untouched(wide, off, self.cin_pad, inf), f"{self.cid}: data gradient ({tag}) wrote outside its channel slice"
            assert bool((wide[..., off + self.Cin:off + self.cin_pad] == 0).all()), f"{self.cid}: pad lanes of dx are not 0 ({tag})"


def _cuts(case):
    """real channels to drop so that Cin and Cout are no multiples of the vector width (none where they already are not)"""
    ve = 4 if case[0] == "f32" else 8
    Cin, Cout = case[1][1], case[1][2]
    return (1 if Cin % ve == 0 else 0), (3 if Cout % ve == 0 else 0)


@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_conv_budget(case):
    """Checks (1) to (3) of the module docstring on the listed shape."""
    c = _Case(case)
    ctx, syms = c.plain()
    c.forward_slices(syms)
    # (the planar stem data gradient of the plain run takes neither accumulate nor add_src; with dx_out ops.conv_backward hands the
    #  same kernels an NHWC8 destination, which takes both)
    c.dgrad_slices(ctx, syms)
    # the weight gradient from sliced operands (NaN in the foreign lanes)
    _xw, xs, _ = _framed(c.xn, c.cin_pad, float("nan"))
    _gw, gs, _ = _framed(c.gn, c.cout_pad, float("nan"))
    gw, sym = c.wgrad(xs, gs)
    assert sym == syms[2], (c.cid, "slice wgrad", sym, syms[2])
    c.check("slice wgrad", "dw", gw, sym)


RAGGED = [c for c in R.CASES if _cuts(c) != (0, 0)]          # (the others are ragged as listed: test_conv_budget checks their pad lanes)


@pytest.mark.parametrize("case", RAGGED, ids=[R.case_id(c) for c in RAGGED])
def test_conv_budget_ragged_channels(case):
    """Check (4): the same routes (dispatch sees the padded counts) with Cin and Cout that are no multiples of the vector width."""
    c = _Case(case, *_cuts(case))
    assert c.cin_pad != c.Cin and c.cout_pad != c.Cout
    c.plain()


def test_budget_cases_cover_every_snapshot_symbol():
    """The symbols the cases are listed under (each case asserts them) are, per entry and dtype, the set in
    golden/g22_conv_routes.json: a new route cannot arrive untested."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_conv_routes.json")) as f:
        want, have, unkeyed = R.snapshot_coverage(json.load(f))
    assert have - unkeyed == want, (sorted(want - have), sorted(have - unkeyed - want))
    assert len(unkeyed) == 6, unkeyed
    for f in sorted(_figures):
        v = _figures[f]
        print(f"{f}: largest worst ratio {v[0]:.3g} ({v[2]}), smallest power margin {v[1]:.3g} ({v[3]})")
