"""Every C-ABI entry of csrc/seg.hip and csrc/pose.hip through ctypes against the float64 statement and budgets of tests/segpose_ref.py,
on its case list: a frozen hand-written assignment (129 and 64 positives in an image, a gt row of -1, a target_gt_idx past n_max),
rectangular proto maps and levels, masks at other resolutions, int32 index maps, crop edges on the f32 traps.  Inputs are channel slices
[VE, VE + width) of buffers 2 VE lanes wider than needed with NaN in every other lane; float outputs are pre-filled with NaN, integer
outputs with a value the kernels never write; every element is compared and everything outside the payload must be what was put there.
Each test prints the worst ratio to the budget and the power margin per result; the last one the largest ratio per entry."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import segpose_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32 = torch.float32
SEG_DT = [(r, dn) for dn in R.DTYPES for r in R.SEG_RUNS]
SEG_IDS = [f"{R.run_id(r)}-{dn}" for r, dn in SEG_DT]
POSE_DT = [(r, dn) for dn in R.DTYPES for r in R.POSE_RUNS]
POSE_IDS = [f"{R.run_id(r)}-{dn}" for r, dn in POSE_DT]
ENTRIES = ("dy_seg_positives", "dy_seg_gt_rows", "dy_seg_loss_fwd", "dy_seg_loss_bwd", "dy_bias_add", "dy_bias_grad", "dy_seg_mask_decode",
           "dy_seg_crop_mask", "dy_seg_mask_iou", "dy_pose_loss_fwd", "dy_pose_loss_bwd", "dy_pose_kpt_decode", "dy_kpt_oks")
_figures = {}          # entry -> [largest worst ratio, its result, smallest power margin, its result]


def _ok(entry, rep):
    print(rep)
    f = _figures.setdefault(entry, [0.0, "", float("inf"), ""])
    if rep.worst > f[0]:
        f[0], f[1] = rep.worst, rep.name
    if rep.margin < f[2]:
        f[2], f[3] = rep.margin, rep.name
    assert rep.worst <= 1.0, str(rep)


def _exact(entry, name, ok):
    """An entry whose result is discrete: equal (ratio 0) or not."""
    _ok(entry, R.Report(name, 0.0 if ok else float("inf"), (), float("inf"), 1))


def _sliced(t, dtype):
    """t [..., w] on the device as the channel slice [VE, VE + w) of a buffer [..., round_up(w, VE) + 2 VE] of `dtype`, NaN elsewhere:
    (buffer, pointer to the slice, ld)."""
    from dedark_yolo_amd import ops
    ve, w = ops.vec_elems(dtype), t.shape[-1]
    ld = ops.round_up(w, ve) + 2 * ve
    buf = torch.full((*t.shape[:-1], ld), NAN, dtype=dtype, device="cuda")
    buf[..., ve:ve + w] = t.to(dtype).cuda()
    return buf, buf.data_ptr() + ve * buf.element_size(), ld


def _untouched(buf, lo, hi, what):
    """Every lane outside [lo, hi) of the last axis is still NaN."""
    assert bool(torch.isnan(buf[..., :lo]).all()) and bool(torch.isnan(buf[..., hi:]).all()), f"{what}: wrote outside the payload"


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- dy_seg_positives ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 63, 64, 65, 255, 256, 257, 600])
def test_seg_positives(A):
    """pos[b][:npos[b]] = the ascending nonzero indices, npos exact, pos past npos untouched; fg bytes of 1, 2 and 255."""
    from dedark_yolo_amd import _C, ops
    g = torch.Generator().manual_seed(A)
    rand = (torch.rand(A, generator=g) < 0.4).to(torch.uint8) * torch.tensor([1, 2, 255], dtype=torch.uint8)[torch.randint(0, 3, (A,), generator=g)]
    last = torch.zeros(A, dtype=torch.uint8)
    last[-1] = 7
    for rows in ((torch.zeros(A, dtype=torch.uint8), torch.ones(A, dtype=torch.uint8), rand), (last, rand.flip(0), torch.full((A,), 255, dtype=torch.uint8))):
        fg = torch.stack(rows).cuda()
        pos = torch.full((3, A), -7, dtype=torch.int32, device="cuda")
        npos = torch.full((3,), -7, dtype=torch.int32, device="cuda")
        _C.call("dy_seg_positives", ops.ptr(fg), 3, A, ops.ptr(pos), ops.ptr(npos), ops.stream())
        torch.cuda.synchronize()
        ok = True
        for b in range(3):
            want = rows[b].nonzero().squeeze(1).int()
            n = want.numel()
            ok &= int(npos[b]) == n and torch.equal(pos[b, :n].cpu(), want) and bool((pos[b, n:] == -7).all())
        _exact("dy_seg_positives", f"positives A={A}", ok)


# ---- dy_seg_gt_rows -----------------------------------------------------------------------------------------------------------------
def test_seg_gt_rows():
    """Unsorted batch_idx, an image with more labels than n_max (the first n_max kept), one with none (all -1), ids outside [0, B),
    no targets at all with a null pointer, B = 65 (the second block); the words after the table untouched."""
    from dedark_yolo_amd import _C, ops
    g = torch.Generator().manual_seed(2)
    runs = [(torch.tensor([2., 0, 5, 2, -1, 2, 0, 0, 3, -3]), 4, 2), (torch.zeros(0), 3, 2),
            (torch.randint(-2, 68, (300,), generator=g).float(), 65, 4), (torch.tensor([1., 1, 1]), 2, 1)]
    for bi, B, n_max in runs:
        n = bi.numel()
        rows = torch.full((B * n_max + 8,), -7, dtype=torch.int32, device="cuda")
        d = bi.cuda()
        _C.call("dy_seg_gt_rows", ops.ptr(d) if n else None, n, B, n_max, ops.ptr(rows), ops.stream())
        torch.cuda.synchronize()
        want = R.gt_rows_ref(bi, B, n_max).int()
        got = rows.cpu()
        _exact("dy_seg_gt_rows", f"gt_rows n={n} B={B} n_max={n_max}", torch.equal(got[:B * n_max].view(B, n_max), want) and bool((got[B * n_max:] == -7).all()))
    assert R.gt_rows_ref(runs[0][0], 4, 2).tolist() == [[1, 6], [-1, -1], [0, 3], [8, -1]]


# ---- segment loss ---------------------------------------------------------------------------------------------------------------------
_seg = {}
GO = 0.37


def _seg_chain(run, dn):
    """positives -> gt rows -> forward (twice) -> backward (twice, grad_out 0.37) on the device, once per run and dtype."""
    if (run, dn) in _seg:
        return _seg[(run, dn)]
    from dedark_yolo_amd import _C, ops
    dtype = R.DTYPES[dn]
    case = R.make_seg_case(run[0], run[1], dtype)
    B, A, mh, mw = case.B, case.A, case.mh, case.mw
    st_ = ops.stream()
    k = SimpleNamespace(case=case, dtype=dtype)
    k.mc, p_mc, ld_mc = _sliced(case.mc, dtype)
    k.proto, p_pr, ld_pr = _sliced(case.proto, dtype)
    fg8 = case.fg.to(torch.uint8)
    fg8[case.fg] = torch.tensor([1, 3, 255], dtype=torch.uint8)[torch.arange(int(case.fg.sum())) % 3]
    k.fg, k.gi, k.tbox, k.masks = fg8.cuda(), case.gi.int().cuda(), case.tbox.cuda().contiguous(), case.masks.cuda().contiguous()
    k.pos = torch.full((B, A), -7, dtype=torch.int32, device="cuda")
    k.npos = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    _C.call("dy_seg_positives", ops.ptr(k.fg), B, A, ops.ptr(k.pos), ops.ptr(k.npos), st_)
    k.rows = torch.full((B, case.n_max), -7, dtype=torch.int32, device="cuda")
    k.bidx = case.batch_idx.cuda()
    _C.call("dy_seg_gt_rows", ops.ptr(k.bidx) if k.bidx.numel() else None, k.bidx.numel(), B, case.n_max, ops.ptr(k.rows), st_)
    d = _C.SegDesc()
    d.mc, d.mc_ld, d.proto, d.proto_ld = p_mc, ld_mc, p_pr, ld_pr
    d.B, d.A, d.nm, d.mh, d.mw = B, A, R.NM, mh, mw
    d.target_gt_idx, d.fg_mask, d.target_box = ops.ptr(k.gi), ops.ptr(k.fg), ops.ptr(k.tbox)
    d.masks, d.mask_dtype, d.mask_h, d.mask_w = ops.ptr(k.masks), int(case.masks.dtype == torch.int32), case.mask_h, case.mask_w
    d.overlap, d.gt_rows, d.n_max = int(case.overlap), (None if case.overlap else ops.ptr(k.rows)), case.n_max
    d.img_h, d.img_w, d.pos, d.npos, d.dtype = case.img_h, case.img_w, ops.ptr(k.pos), ops.ptr(k.npos), ops.dt_id(dtype)
    k.desc = d
    k.det = torch.tensor(R.DET_OUT, device="cuda")
    k.fwd = []
    for _ in range(2):
        lossp = torch.full((B * A + B,), NAN, device="cuda")
        out = torch.full((5,), NAN, device="cuda")
        _C.call("dy_seg_loss_fwd", C.byref(d), R.HYP_BOX, ops.ptr(lossp), ops.ptr(k.det), ops.ptr(out), st_)
        k.fwd.append((lossp, out))
    ve = ops.vec_elems(dtype)
    k.ve, k.go = ve, torch.tensor([GO], device="cuda")
    k.bwd = []
    for _ in range(2):
        dmc = torch.full((B, A, R.NM + 2 * ve), NAN, dtype=dtype, device="cuda")
        dpr = torch.full((B, mh, mw, R.NM + 2 * ve), NAN, dtype=dtype, device="cuda")
        off = ve * dmc.element_size()
        _C.call("dy_seg_loss_bwd", C.byref(d), ops.ptr(k.go), R.HYP_BOX, dmc.data_ptr() + off, R.NM + 2 * ve, dpr.data_ptr() + off, R.NM + 2 * ve, st_)
        k.bwd.append((dmc, dpr))
    torch.cuda.synchronize()
    k.st = R.seg_statement(case)
    k.st_g = R.seg_statement(case, grad_out=GO)
    _seg[(run, dn)] = k
    return k


@pytest.mark.parametrize("run,dn", SEG_DT, ids=SEG_IDS)
def test_seg_loss_fwd(run, dn):
    """lossp per positive in slot order, the per-image means and out[0..4] under budget; lossp past npos untouched; two runs agree bit
    for bit; the inputs' foreign lanes still NaN."""
    k = _seg_chain(run, dn)
    c, st = k.case, k.st
    name = f"{R.run_id(run)} {dn}"
    B, A = c.B, c.A
    assert k.npos.cpu().tolist() == st["npos"]
    for b in range(B):
        assert torch.equal(k.pos[b, :st["npos"][b]].cpu().long(), c.fg[b].nonzero().squeeze(1))
    if not c.overlap:
        assert torch.equal(k.rows.cpu().long(), c.rows)
    lossp, out = k.fwd[0]
    lp = lossp[:B * A].view(B, A).cpu()
    live = torch.zeros(B, A, dtype=torch.bool)
    for b, n in enumerate(st["npos"]):
        live[b, :n] = True
    assert bool(torch.isnan(lp[~live]).all()), "lossp written past npos"
    ref, m = st["lossp"]
    _ok("dy_seg_loss_fwd", R.compare("lossp " + name, lp[live], ref[live], m[live], R.C["seg_lossp"], n_terms=32))
    _ok("dy_seg_loss_fwd", R.compare("means " + name, lossp[B * A:].cpu(), *st["means"], R.C["seg_means"], n_terms=max(1, max(st["npos"]))))
    _ok("dy_seg_loss_fwd", R.compare("out " + name, out.cpu(), *st["out"], R.C["seg_out"], n_terms=B))
    assert torch.equal(out[[1, 3, 4]].cpu(), torch.tensor(R.DET_OUT)[[1, 2, 3]])
    for b, n in enumerate(st["npos"]):
        if n == 0:
            assert float(lossp[B * A + b]) == 0.0
    assert _same_bytes(lossp, k.fwd[1][0]) and _same_bytes(out, k.fwd[1][1]), "two forward runs differ"
    _untouched(k.mc, k.ve, k.ve + R.NM, "mc")
    _untouched(k.proto, k.ve, k.ve + R.NM, "proto")


@pytest.mark.parametrize("run,dn", SEG_DT, ids=SEG_IDS)
def test_seg_loss_bwd(run, dn):
    """d mc of every positive and every d proto element under budget for grad_out 0.37; rows of other anchors and the lanes around both
    payloads keep their NaN (the contract the wrapper's torch.zeros relies on); d proto written for every pixel of every image, zero for
    an image without positives; two runs agree bit for bit."""
    k = _seg_chain(run, dn)
    c, st, ve = k.case, k.st_g, k.ve
    name = f"{R.run_id(run)} {dn}"
    dmc, dpr = k.bwd[0]
    _untouched(dmc, ve, ve + R.NM, "d mc")
    _untouched(dpr, ve, ve + R.NM, "d proto")
    got = dmc[..., ve:ve + R.NM].float().cpu()
    assert bool(torch.isnan(got[~c.fg]).all()), "d mc rows of non-positive anchors written"
    ref, m = st["dmc"]
    _ok("dy_seg_loss_bwd", R.compare("d mc " + name, got[c.fg], ref[c.fg], m[c.fg], R.C["seg_dmc"], k.dtype, n_terms=32))
    gp = dpr[..., ve:ve + R.NM].float().cpu()
    assert bool(torch.isfinite(gp).all()), "d proto: a pixel was not written"
    _ok("dy_seg_loss_bwd", R.compare("d proto " + name, gp, *st["dproto"], R.C["seg_dproto"], k.dtype, n_terms=32))
    for b, n in enumerate(st["npos"]):
        if n == 0:
            assert float(gp[b].abs().max()) == 0.0
    assert _same_bytes(dmc, k.bwd[1][0]) and _same_bytes(dpr, k.bwd[1][1]), "two backward runs differ"


# ---- ConvTranspose2d bias -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", list(R.DTYPES))
@pytest.mark.parametrize("C_", R.BIAS_CS)
def test_bias_add_and_grad(C_, dn):
    """x + bias in place and the column sums, ld > C, pixels 0 .. 5000 (at 5000 the last of the 2048 chunks start past the end); the pad
    lanes keep their NaN; pixels = 0: nothing written, exact zeros; a scratch buffer one float too small is refused."""
    from dedark_yolo_amd import _C, ops
    dtype = R.DTYPES[dn]
    ve = ops.vec_elems(dtype)
    for pixels in R.BIAS_PIXELS:
        x, bias = R.bias_inputs(C_, pixels, dtype)
        ref = R.bias_ref(x, bias)
        buf, p, ld = _sliced(x if pixels else torch.zeros(1, C_), dtype)
        before = buf.clone()
        db = torch.full((C_ + 4,), NAN, device="cuda")
        scratch = torch.full((_C.BIAS_GRAD_CHUNKS * C_,), NAN, device="cuda")
        dbias = bias.cuda()
        _C.call("dy_bias_grad", p, ld, pixels, C_, ops.dt_id(dtype), ops.ptr(scratch), scratch.numel(), ops.ptr(db), ops.stream())
        _C.call("dy_bias_add", p, ld, ops.ptr(dbias), pixels, C_, ops.dt_id(dtype), ops.stream())
        torch.cuda.synchronize()
        name = f"C={C_} pixels={pixels} {dn}"
        assert bool(torch.isnan(db[C_:]).all())
        _untouched(buf, ve, ve + C_, "x")
        if pixels == 0:
            assert _same_bytes(buf, before) and bool((db[:C_] == 0).all()), name
            continue
        _ok("dy_bias_grad", R.compare("db " + name, db[:C_].cpu(), *ref["db"], R.C["bias_db"], n_terms=pixels))
        _ok("dy_bias_add", R.compare("x + bias " + name, buf[..., ve:ve + C_].float().cpu(), *ref["add"], R.C["bias_add"], dtype, n_terms=2))
    with pytest.raises(RuntimeError, match="dy_bias_grad: scratch needs"):
        _C.call("dy_bias_grad", p, ld, 1, C_, ops.dt_id(dtype), ops.ptr(scratch), scratch.numel() - 1, ops.ptr(db), ops.stream())


# ---- validation: decode, crop, IoU -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", list(R.DTYPES))
@pytest.mark.parametrize("shape", [(9, 7, 11), (26, 21, 7)], ids=["9x7", "26x21"])
def test_seg_mask_decode(shape, dn):
    """Bytes equal the statement wherever |z| exceeds the f32 dot product's error; det_ld = 45, det_img out of order over three images,
    box edges on the f32 traps, one detection with all coefficients zero (sigmoid = 0.5 is not > 0.5: empty)."""
    from dedark_yolo_amd import _C, ops
    mh, mw, n = shape
    dtype = R.DTYPES[dn]
    proto, det, det_img, (W, H) = R.decode_inputs(mh, mw, n, dtype)
    sx, sy = float(mw / W), float(mh / H)
    want, sure = R.decode_ref(proto, det, det_img, sx, sy)
    buf, p, ld = _sliced(proto, dtype)
    d45 = torch.full((n, 45), NAN)
    d45[:, :38] = det
    d45, dimg = d45.cuda(), det_img.cuda()
    out = torch.full((n * mh * mw + 64,), 7, dtype=torch.uint8, device="cuda")
    _C.call("dy_seg_mask_decode", p, ld, R.NM, mh, mw, ops.ptr(d45), 45, ops.ptr(dimg), n, sx, sy, ops.dt_id(dtype), ops.ptr(out), ops.stream())
    _C.call("dy_seg_mask_decode", p, ld, R.NM, mh, mw, ops.ptr(d45), 45, ops.ptr(dimg), 0, sx, sy, ops.dt_id(dtype), None, ops.stream())
    torch.cuda.synchronize()
    got = out[:n * mh * mw].view(n, mh, mw).cpu()
    assert int(got.max()) <= 1 and bool((out[n * mh * mw:] == 7).all())
    assert int(got[1].sum()) == 0 and bool(sure[[j for j in range(n) if j != 1]].float().mean() >= 0.999)
    sure[1] = True
    _exact("dy_seg_mask_decode", f"mask decode {mh}x{mw} {dn}", torch.equal(got[sure], want[sure]))
    assert int(want.sum()) > 0 and int(want[2].sum()) == 0            # the third box holds no column


def test_seg_crop_mask():
    """h != w, NaN and negative values inside and outside the boxes: equal to masks * crop on the CPU, NaN positions included; n = 0
    touches nothing."""
    from dedark_yolo_amd import _C, ops
    g = torch.Generator().manual_seed(9)
    n, h, w = 5, 13, 22
    m = torch.randn(n, h, w, generator=g)
    m[torch.rand(n, h, w, generator=g) < 0.1] = NAN
    boxes = torch.tensor([[3.0, 2.0, 15.0, 9.0], [3.25, 2.0, 3.75, 9.0], [-4.0, -2.0, 40.0, 30.0], [5.0, 4.0, 5.0, 4.0], [0.0, 12.0, 21.5, 13.0]])
    x1, y1, x2, y2 = [boxes[:, j].view(-1, 1, 1) for j in range(4)]
    r, c = torch.arange(w, dtype=F32).view(1, 1, -1), torch.arange(h, dtype=F32).view(1, -1, 1)
    want = m * ((r >= x1) * (r < x2) * (c >= y1) * (c < y2))
    d, db = m.cuda(), boxes.cuda()
    _C.call("dy_seg_crop_mask", ops.ptr(d), ops.ptr(db), n, h, w, ops.stream())
    torch.cuda.synchronize()
    got = d.cpu()
    ok = torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(123.0), want.nan_to_num(123.0))
    assert bool(want.isnan().any()) and bool((want[~want.isnan()] < 0).any()) and bool(want[0, 0, 0].isnan() or want[0, 0, 0] == 0)
    d2 = m.cuda()
    _C.call("dy_seg_crop_mask", ops.ptr(d2), ops.ptr(db), 0, h, w, ops.stream())
    torch.cuda.synchronize()
    _exact("dy_seg_crop_mask", "crop_mask 13x22", ok and _same_bytes(d2.cpu(), m))


def test_seg_mask_iou():
    """hw = 35 * 29: index maps uint8 (m = 1, 5) and int32 (m = 300, values above m ignored), planes uint8; an empty prediction, an empty
    gt and both; bit for bit the f32 ratio of the integer counts; n = 0 or m = 0 returns early."""
    from dedark_yolo_amd import _C, ops
    g = torch.Generator().manual_seed(4)
    hw, n = 35 * 29, 6
    pred = (torch.rand(n, hw, generator=g) < 0.4).to(torch.uint8)
    pred[2] = 0
    runs = []
    for m_ in (1, 5):
        runs.append((torch.randint(0, 7, (hw,), generator=g).to(torch.uint8), 0, 1, m_))
    big = torch.randint(0, 304, (hw,), generator=g).int()
    big[big == 17] = 1000                                                    # label 16 has no pixel; 1000 and 301 .. 303 are ignored
    runs.append((big, 1, 1, 300))
    planes = (torch.rand(4, hw, generator=g) < 0.3).to(torch.uint8)
    planes[1] = 0
    runs.append((planes, 0, 0, 4))
    for gt, gdt, overlap, m_ in runs:
        iou = torch.full((m_ * n + 4,), NAN, device="cuda")
        work = torch.full((m_ * n + n,), -7, dtype=torch.int32, device="cuda")
        dp, dg = pred.cuda(), gt.cuda()
        _C.call("dy_seg_mask_iou", ops.ptr(dp), n, ops.ptr(dg), gdt, overlap, m_, hw, ops.ptr(work), ops.ptr(iou), ops.stream())
        torch.cuda.synchronize()
        want = R.mask_iou_ref(pred, gt, overlap, m_)
        got = iou[:m_ * n].view(m_, n).cpu()
        assert bool(torch.isnan(iou[m_ * n:]).all()) and bool((want[:, 2] == 0).all()) and float(want.max()) > 0
        _exact("dy_seg_mask_iou", f"mask IoU overlap={overlap} i32={gdt} m={m_}", torch.equal(got, want))
        for n0, m0 in ((0, m_), (n, 0)):
            iou.fill_(NAN)
            _C.call("dy_seg_mask_iou", ops.ptr(dp), n0, ops.ptr(dg), gdt, overlap, m0, hw, ops.ptr(work), ops.ptr(iou), ops.stream())
            torch.cuda.synchronize()
            assert bool(torch.isnan(iou).all())
    assert float(R.mask_iou_ref(pred, planes, 0, 4)[1, 2]) == 0.0            # an empty gt against an empty prediction: 0 / 1e-7


# ---- pose loss ----------------------------------------------------------------------------------------------------------------------------
_pose = {}
GUARD, SENT = 64, 4096.0


def _pose_desc(k, case, dtype, loss=True):
    from dedark_yolo_amd import _C, ops
    d = _C.PoseDesc()
    k.maps = []
    for i, (lvl, (h, w, s)) in enumerate(zip(R.pose_level_maps(case), case.levels)):
        buf, p, ld = _sliced(lvl, dtype)
        k.maps.append(buf)
        d.kpt[i], d.kpt_ld[i], d.h[i], d.w[i], d.stride[i] = p, ld, h, w, s
    d.n_levels, d.B, d.A, d.K, d.ndim, d.dtype = len(case.levels), case.B, case.A, case.K, case.ndim, ops.dt_id(dtype)
    if loss:
        d.target_gt_idx, d.fg_mask, d.target_box = ops.ptr(k.gi), ops.ptr(k.fg), ops.ptr(k.tbox)
        d.keypoints, d.n_targets = (ops.ptr(k.kp) if k.kp.numel() else None), k.kp.shape[0]
        d.gt_rows, d.n_max, d.img_h, d.img_w = ops.ptr(k.rows), case.n_max, case.img_h, case.img_w
        d.sigma, d.pos, d.npos = ops.ptr(k.sigma), ops.ptr(k.pos), ops.ptr(k.npos)
    return d


def _pose_chain(run, dn):
    """positives -> gt rows -> forward (twice) on the device, once per run and dtype."""
    if (run, dn) in _pose:
        return _pose[(run, dn)]
    from dedark_yolo_amd import _C, ops
    dtype = R.DTYPES[dn]
    case = R.make_pose_case(run[0], run[1], dtype)
    B, A = case.B, case.A
    st_ = ops.stream()
    k = SimpleNamespace(case=case, dtype=dtype, ve=ops.vec_elems(dtype))
    fg8 = case.fg.to(torch.uint8)
    fg8[case.fg] = torch.tensor([1, 3, 255], dtype=torch.uint8)[torch.arange(int(case.fg.sum())) % 3]
    k.fg, k.gi, k.tbox = fg8.cuda(), case.gi.int().cuda(), case.tbox.cuda().contiguous()
    k.kp, k.sigma, k.bidx = case.keypoints.cuda().contiguous(), case.sigma.float().cuda(), case.batch_idx.cuda()
    k.pos = torch.full((B, A), -7, dtype=torch.int32, device="cuda")
    k.npos = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    _C.call("dy_seg_positives", ops.ptr(k.fg), B, A, ops.ptr(k.pos), ops.ptr(k.npos), st_)
    k.rows = torch.full((B, case.n_max), -7, dtype=torch.int32, device="cuda")
    _C.call("dy_seg_gt_rows", ops.ptr(k.bidx) if k.bidx.numel() else None, k.bidx.numel(), B, case.n_max, ops.ptr(k.rows), st_)
    k.desc = _pose_desc(k, case, dtype)
    k.det = torch.tensor(R.DET_OUT, device="cuda")
    k.fwd = []
    for _ in range(2):
        work = torch.full((3 * B * A + 3 * B,), NAN, device="cuda")
        out = torch.full((6,), NAN, device="cuda")
        _C.call("dy_pose_loss_fwd", C.byref(k.desc), R.HYP_POSE, R.HYP_KOBJ, ops.ptr(work), ops.ptr(k.det), ops.ptr(out), st_)
        k.fwd.append((work, out))
    torch.cuda.synchronize()
    k.st = R.pose_statement(case)
    _pose[(run, dn)] = k
    return k


@pytest.mark.parametrize("run,dn", POSE_DT, ids=POSE_IDS)
def test_pose_loss_fwd(run, dn):
    """work (three planes, slot order, untouched past npos), img (three planes) and out[0..5] under budget; kobj 0 for ndim 2; two runs
    agree bit for bit."""
    k = _pose_chain(run, dn)
    c, st = k.case, k.st
    name = f"{R.run_id(run)} {dn}"
    B, A = c.B, c.A
    assert k.npos.cpu().tolist() == st["npos"] and torch.equal(k.rows.cpu().long(), c.rows)
    work, out = k.fwd[0]
    w3 = work[:3 * B * A].view(3, B, A).cpu()
    live = torch.zeros(3, B, A, dtype=torch.bool)
    for b, n in enumerate(st["npos"]):
        live[:, b, :n] = True
    assert bool(torch.isnan(w3[~live]).all()), "work written past npos"
    ref, m = st["work"]
    _ok("dy_pose_loss_fwd", R.compare("work " + name, w3[live], ref[live], m[live], R.C["pose_work"], n_terms=c.K))
    assert torch.equal(w3[1][live[1]], ref[1][live[1]].float())                          # the visible counts are exact
    _ok("dy_pose_loss_fwd", R.compare("img " + name, work[3 * B * A:].view(3, B).cpu(), *st["img"], R.C["pose_img"], n_terms=max(1, max(st["npos"]))))
    _ok("dy_pose_loss_fwd", R.compare("out " + name, out.cpu(), *st["out"], R.C["pose_out"], n_terms=B))
    assert torch.equal(out[[1, 4, 5]].cpu(), torch.tensor(R.DET_OUT)[[1, 2, 3]])
    if c.ndim == 2:
        assert float(out[3]) == 0.0
    assert _same_bytes(work, k.fwd[1][0]) and _same_bytes(out, k.fwd[1][1]), "two forward runs differ"
    for buf in k.maps:
        _untouched(buf, k.ve, k.ve + c.K * c.ndim, "kpt map")


@pytest.mark.parametrize("run,dn", POSE_DT, ids=POSE_IDS)
def test_pose_loss_bwd(run, dn):
    """Every element of every level's gradient map written: under budget at the positives' K * ndim lanes, exact zeros at the other
    anchors and lanes; dk_ld the padded width and VE wider; grad_out 1 and 0.37; guard words around each map untouched; two runs agree bit
    for bit."""
    from dedark_yolo_amd import _C, ops
    k = _pose_chain(run, dn)
    c, dtype, ve = k.case, k.dtype, k.ve
    nk = c.K * c.ndim
    work = k.fwd[0][0]
    for extra, go in ((0, 1.0), (ve, 0.37)):
        dk_ld = ops.round_up(nk, ve) + extra
        st = k.st if go == 1.0 else R.pose_statement(c, grad_out=go)
        g = torch.tensor([go], device="cuda")
        runs = []
        for _ in range(2):
            bufs = []
            for h, w, _s in c.levels:
                n = c.B * h * w * dk_ld
                buf = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device="cuda")
                buf[GUARD:GUARD + n] = NAN
                bufs.append((buf, n))
            arr = (C.c_void_p * len(bufs))(*[b.data_ptr() + GUARD * b.element_size() for b, _ in bufs])
            _C.call("dy_pose_loss_bwd", C.byref(k.desc), ops.ptr(work), ops.ptr(g), R.HYP_POSE, R.HYP_KOBJ, arr, dk_ld, ops.stream())
            runs.append(bufs)
        torch.cuda.synchronize()
        got = []
        for i, ((buf, n), (h, w, _s)) in enumerate(zip(runs[0], c.levels)):
            assert bool((buf[:GUARD].float() == SENT).all()) and bool((buf[GUARD + n:].float() == SENT).all()), f"map {i}: wrote outside"
            assert _same_bytes(buf, runs[1][i][0]), "two backward runs differ"
            body = buf[GUARD:GUARD + n].float().view(c.B, h * w, dk_ld).cpu()
            assert bool((body[..., nk:] == 0).all()), f"map {i}: lanes past K * ndim not zero"
            got.append(body[..., :nk])
        got = torch.cat(got, 1)
        assert bool((got[~c.fg] == 0).all()), "non-positive anchors not exactly zero"
        ref, m = st["dkpt"]
        _ok("dy_pose_loss_bwd", R.compare(f"d kpt {R.run_id(run)} {dn} dk_ld {dk_ld} grad_out {go}", got[c.fg], ref[c.fg], m[c.fg], R.C["pose_dkpt"],
                                         dtype, n_terms=2))


@pytest.mark.parametrize("dn", list(R.DTYPES))
@pytest.mark.parametrize("cid", ["rect2", "one", "four"])
def test_pose_kpt_decode(cid, dn):
    """nc = 3: rows [4 + nc, 4 + nc + K * ndim) under budget, rows [0, 4 + nc) keep their NaN."""
    from dedark_yolo_amd import _C, ops
    k = _pose_chain((cid, "wide"), dn)
    c = k.case
    nc, nk = 3, c.K * c.ndim
    kk = SimpleNamespace()
    d = _pose_desc(kk, c, k.dtype, loss=False)
    y = torch.full((c.B, 4 + nc + nk, c.A), NAN, device="cuda")
    _C.call("dy_pose_kpt_decode", C.byref(d), nc, ops.ptr(y), ops.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[:, :4 + nc]).all()), "rows of dy_detect_decode written"
    _ok("dy_pose_kpt_decode", R.compare(f"y {cid} {dn}", y[:, 4 + nc:].cpu(), *k.st["y"], R.C["pose_y"], n_terms=2))


@pytest.mark.parametrize("pred_dim", [2, 3])
def test_kpt_oks(pred_dim):
    """7 x 41 (two blocks): a gt with no visible keypoint (exact 0), a gt with area 0; N = 0 or M = 0 leaves the output untouched."""
    from dedark_yolo_amd import _C, ops
    gt, pred, area = R.oks_inputs(pred_dim)
    N, M, K = gt.shape[0], pred.shape[0], gt.shape[1]
    out = torch.full((N * M + 4,), NAN, device="cuda")
    dg, dp, da, ds = gt.cuda(), pred.cuda(), area.cuda(), R.OKS_SIGMA.float().cuda()
    _C.call("dy_kpt_oks", ops.ptr(dg), N, ops.ptr(dp), M, pred_dim, ops.ptr(da), ops.ptr(ds), K, 1e-7, ops.ptr(out), ops.stream())
    torch.cuda.synchronize()
    got = out[:N * M].view(N, M).cpu()
    assert bool(torch.isnan(out[N * M:]).all()) and bool((got[2] == 0).all()) and float(got.max()) > 0.1
    ref, m = R.oks_ref(gt, pred, area, R.OKS_SIGMA.float())
    _ok("dy_kpt_oks", R.compare(f"OKS pred_dim {pred_dim}", got, ref, m, R.C["oks"], n_terms=K))
    for n0, m0 in ((0, M), (N, 0)):
        out.fill_(NAN)
        _C.call("dy_kpt_oks", ops.ptr(dg), n0, ops.ptr(dp), m0, pred_dim, ops.ptr(da), ops.ptr(ds), K, 1e-7, ops.ptr(out), ops.stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())


# ---- rejections ------------------------------------------------------------------------------------------------------------------------------
def _rejected(bad):
    """Each call raises with the entry's name in the text, and no kernel was noted: the launcher returned before any launch."""
    from dedark_yolo_amd import _C
    lib = _C.lib()
    for msg, call in bad:
        lib.dy_clear_last_kernel()
        with pytest.raises(RuntimeError, match=msg):
            _C.call(*call)
        assert call[0] in msg and lib.dy_last_kernel().decode() == "", (msg, lib.dy_last_kernel().decode())
    torch.cuda.synchronize()


def _copy_desc(d, **kw):
    e = type(d)()
    C.memmove(C.byref(e), C.byref(d), C.sizeof(d))
    for name, v in kw.items():
        setattr(e, name, v)
    return e


def test_bad_seg_arguments_are_rejected():
    from dedark_yolo_amd import ops
    k = _seg_chain(("chunks", "unit"), "f32")
    d, s = k.desc, ops.stream()
    f = torch.zeros(4096, device="cuda")
    i8 = torch.zeros(64, dtype=torch.uint8, device="cuda")
    fwd = lambda e: ("dy_seg_loss_fwd", C.byref(e), 7.5, ops.ptr(f), ops.ptr(k.det), ops.ptr(f), s)                # noqa: E731
    bwd = lambda e, dmc=ops.ptr(f), ld=32: ("dy_seg_loss_bwd", C.byref(e), ops.ptr(k.go), 7.5, dmc, ld, ops.ptr(f), 32, s)       # noqa: E731
    _rejected([
        ("dy_seg_loss_fwd: nm=16", fwd(_copy_desc(d, nm=16))),
        ("dy_seg_loss_fwd: mc_ld / proto_ld below nm", fwd(_copy_desc(d, mc_ld=28))),
        ("dy_seg_loss_fwd: mc / proto rows must be 16-byte aligned", fwd(_copy_desc(d, mc=d.mc + 4))),
        ("dy_seg_loss_fwd: mc / proto rows must be 16-byte aligned", fwd(_copy_desc(d, proto_ld=d.proto_ld + 1))),
        ("dy_seg_loss_fwd: bad gt masks", fwd(_copy_desc(d, mask_dtype=2))),
        ("dy_seg_loss_bwd: per-instance masks need gt_rows", bwd(_copy_desc(d, gt_rows=None))),
        ("dy_seg_loss_fwd: bad image size", fwd(_copy_desc(d, img_w=0.0))),
        ("dy_seg_loss_fwd: null pointer", fwd(_copy_desc(d, pos=None))),
        ("dy_seg_loss_fwd: null output", ("dy_seg_loss_fwd", C.byref(d), 7.5, None, ops.ptr(k.det), ops.ptr(f), s)),
        ("dy_seg_loss_bwd: null output", bwd(d, dmc=None)),
        ("dy_seg_loss_bwd: dmc_ld / dproto_ld below nm", bwd(d, ld=31)),
        ("dy_seg_positives: bad args", ("dy_seg_positives", ops.ptr(i8), 1, 64, None, ops.ptr(f), s)),
        ("dy_seg_gt_rows: bad args", ("dy_seg_gt_rows", None, 3, 2, 2, ops.ptr(f), s)),
        ("dy_bias_add: bad args", ("dy_bias_add", ops.ptr(f), 3, ops.ptr(f), 1, 4, 0, s)),
        ("dy_bias_grad: bad args", ("dy_bias_grad", ops.ptr(f), 4, 1, 4, 0, None, 8192, ops.ptr(f), s)),
        ("dy_seg_mask_decode: nm=16", ("dy_seg_mask_decode", ops.ptr(f), 32, 16, 4, 4, ops.ptr(f), 38, ops.ptr(f), 1, 0.25, 0.25, 0, ops.ptr(i8), s)),
        ("dy_seg_mask_decode: bad geometry", ("dy_seg_mask_decode", ops.ptr(f), 32, 32, 4, 4, ops.ptr(f), 37, ops.ptr(f), 1, 0.25, 0.25, 0, ops.ptr(i8), s)),
        ("dy_seg_mask_decode: null pointer", ("dy_seg_mask_decode", ops.ptr(f), 32, 32, 4, 4, ops.ptr(f), 38, ops.ptr(f), 1, 0.25, 0.25, 0, None, s)),
        ("dy_seg_crop_mask: bad geometry", ("dy_seg_crop_mask", ops.ptr(f), ops.ptr(f), 1, 0, 4, s)),
        ("dy_seg_crop_mask: null pointer", ("dy_seg_crop_mask", None, ops.ptr(f), 1, 4, 4, s)),
        ("dy_seg_mask_iou: bad args", ("dy_seg_mask_iou", ops.ptr(i8), 1, ops.ptr(i8), 2, 1, 1, 16, ops.ptr(f), ops.ptr(f), s)),
        ("dy_seg_mask_iou: per-instance gt planes must be uint8", ("dy_seg_mask_iou", ops.ptr(i8), 1, ops.ptr(i8), 1, 0, 1, 16, ops.ptr(f), ops.ptr(f), s)),
        ("dy_seg_mask_iou: null pointer", ("dy_seg_mask_iou", ops.ptr(i8), 1, ops.ptr(i8), 0, 1, 1, 16, None, ops.ptr(f), s)),
    ])


def test_bad_pose_arguments_are_rejected():
    from dedark_yolo_amd import ops
    k = _pose_chain(("rect2", "unit"), "f32")
    d, s = k.desc, ops.stream()
    f = torch.zeros(4096, device="cuda")
    work = k.fwd[0][0]
    fwd = lambda e: ("dy_pose_loss_fwd", C.byref(e), 12.0, 1.0, ops.ptr(f), ops.ptr(k.det), ops.ptr(f), s)          # noqa: E731
    arr = (C.c_void_p * 4)(*([f.data_ptr()] * 4))
    arr0 = (C.c_void_p * 4)(f.data_ptr(), None, None, None)
    g = torch.ones(1, device="cuda")
    _rejected([
        ("dy_pose_loss_fwd: A=76 but the levels hold 75", fwd(_copy_desc(d, A=76))),
        (r"dy_pose_loss_fwd: bad B / K / ndim \(2, 17, 4\)", fwd(_copy_desc(d, ndim=4))),
        ("dy_pose_loss_fwd: bad descriptor / level count", fwd(_copy_desc(d, n_levels=5))),
        ("dy_pose_loss_fwd: bad level 1", fwd(_copy_desc(d, kpt_ld=(C.c_int64 * 4)(d.kpt_ld[0], 50, 0, 0)))),
        ("dy_pose_loss_fwd: null pointer", fwd(_copy_desc(d, sigma=None))),
        ("dy_pose_loss_fwd: null keypoints", fwd(_copy_desc(d, keypoints=None))),
        ("dy_pose_loss_fwd: bad image size", fwd(_copy_desc(d, img_h=0.0))),
        ("dy_pose_loss_fwd: null output", ("dy_pose_loss_fwd", C.byref(d), 12.0, 1.0, None, ops.ptr(k.det), ops.ptr(f), s)),
        ("dy_pose_loss_bwd: dk_ld 51 below the padded keypoint width", ("dy_pose_loss_bwd", C.byref(d), ops.ptr(work), ops.ptr(g), 12.0, 1.0, arr, 51, s)),
        ("dy_pose_loss_bwd: null gradient map 1", ("dy_pose_loss_bwd", C.byref(d), ops.ptr(work), ops.ptr(g), 12.0, 1.0, arr0, 52, s)),
        ("dy_pose_loss_bwd: null argument", ("dy_pose_loss_bwd", C.byref(d), None, ops.ptr(g), 12.0, 1.0, arr, 52, s)),
        ("dy_pose_kpt_decode: bad args", ("dy_pose_kpt_decode", C.byref(d), 3, None, s)),
        ("dy_pose_kpt_decode: bad descriptor / level count", ("dy_pose_kpt_decode", C.byref(_copy_desc(d, n_levels=0)), 3, ops.ptr(f), s)),
        ("dy_kpt_oks: bad sizes", ("dy_kpt_oks", ops.ptr(f), 1, ops.ptr(f), 1, 4, ops.ptr(f), ops.ptr(f), 17, 1e-7, ops.ptr(f), s)),
        ("dy_kpt_oks: null pointer", ("dy_kpt_oks", ops.ptr(f), 1, ops.ptr(f), 1, 3, ops.ptr(f), None, 17, 1e-7, ops.ptr(f), s)),
    ])


def test_zz_largest_ratio_per_entry():
    """Closing line of the module: per entry, the largest ratio to its budget and the smallest power margin seen above."""
    for e in sorted(_figures):
        v = _figures[e]
        print(f"{e}: largest ratio to budget {v[0]:.3g} ({v[1]}), smallest power margin {v[2]:.3g} ({v[3]})")
    assert sorted(_figures) == sorted(ENTRIES), sorted(set(ENTRIES) ^ set(_figures))
    assert all(v[0] <= 1.0 for v in _figures.values())
