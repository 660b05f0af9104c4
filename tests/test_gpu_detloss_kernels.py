"""Every C-ABI entry of csrc/loss.hip through ctypes against the float64 statement and budgets of tests/detloss_ref.py, on its case
list: rectangular maps, one / two / four levels, the top-k path switch at 640 anchors, ragged class runs, map views that are channel
slices of a wider buffer with NaN around them, both ends of the DFL clamp, tss < 1.  Every element of every output is compared;
outputs are pre-filled with NaN (integer outputs with values the kernels never write).  The fp32 CPU oracle stays the judge of the
assigner's discrete outcome, on the inputs the assigner was given.  Each test prints the worst ratio to the budget and the power
margin per result; the last one the largest ratio per entry."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import detloss_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
RUN_DT = [(r, dn) for dn in R.DTYPES for r in R.RUNS]
RUN_IDS = [f"{R.run_id(r)}-{dn}" for r, dn in RUN_DT]
_figures = {}          # entry -> [largest worst ratio, its result, smallest power margin, its result]


def _ok(entry, rep):
    print(rep)
    f = _figures.setdefault(entry, [0.0, "", float("inf"), ""])
    if rep.worst > f[0]:
        f[0], f[1] = rep.worst, rep.name
    if rep.margin < f[2]:
        f[2], f[3] = rep.margin, rep.name
    assert rep.worst <= 1.0, str(rep)


def _dev_maps(case, dtype):
    """The run's maps on the device as channel slices [VE, VE + 64 + nc) of wider NHWC buffers (ld = padded width + 2 VE), every
    other lane NaN."""
    from dedark_yolo_amd import ops
    ve, no = ops.vec_elems(dtype), 64 + case.nc
    ld = 64 + ops.round_up(case.nc, ve) + 2 * ve
    views, bufs = [], []
    for lvl in R.level_maps(case):
        B, h, w, _ = lvl.shape
        buf = torch.full((B, h, w, ld), NAN, dtype=dtype, device="cuda")
        buf[..., ve:ve + no] = lvl.to(dtype).cuda()
        bufs.append(buf)
        views.append(buf.permute(0, 3, 1, 2)[:, ve:ve + no])
    dm = ops.det_maps(views, [s for _, _, s in case.levels], case.nc)
    assert all(dm.map_ld[i] == ld for i in range(min(3, len(views)))) and dm.n_levels == len(views)
    return dm, bufs


def _assign_outputs(B, A):
    return dict(gi=torch.full((B, A), -7, dtype=torch.int32, device="cuda"), fg=torch.full((B, A), 77, dtype=torch.uint8, device="cuda"),
                norm=torch.full((B, A), NAN, device="cuda"), label=torch.full((B, A), -7, dtype=torch.int32, device="cuda"),
                tbox=torch.full((B, A, 4), NAN, device="cuda"))


def _work(B, n_max, A):
    n_max = max(n_max, 1)
    R_ = B * n_max * A
    return (torch.empty(2 * R_ + 2 * B * n_max, device="cuda"), torch.empty(R_, dtype=torch.int32, device="cuda"),
            torch.empty(R_, dtype=torch.uint8, device="cuda"))


_chains = {}


def _chain(run, dn):
    """prepare targets -> decode -> eval decode -> assign -> forward (twice) on the device, once per run and dtype, with the oracle's
    assignment on the same inputs and the fp64 statement under it."""
    if (run, dn) in _chains:
        return _chains[(run, dn)]
    from dedark_yolo_amd import _C, ops
    dtype = R.DTYPES[dn]
    case = R.make_case(run[0], run[1], dtype)
    B, A, nc = case.B, case.A, case.nc
    st_ = ops.stream()
    dm, bufs = _dev_maps(case, dtype)
    k = SimpleNamespace()
    k.case, k.dm, k.bufs, k.dtype = case, dm, bufs, dtype
    n_t = case.batch_idx.numel()
    n_max = int(torch.bincount(case.batch_idx.long(), minlength=B).max())
    k.n_max = n_max
    bi, cl, bb = case.batch_idx.cuda(), case.cls.view(-1).cuda(), case.bboxes.cuda().contiguous()
    k.n_rows = max(n_max, 1)                                  # a batch without boxes keeps one zero row per image, as the criterion does
    k.gt = torch.full((B, k.n_rows, 5), NAN, device="cuda")
    k.counts = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    _C.call("dy_loss_prepare_targets", ops.ptr(bi) if n_t else None, ops.ptr(cl) if n_t else None, ops.ptr(bb) if n_t else None, n_t, B, k.n_rows,
            float(case.img_w), float(case.img_h), ops.ptr(k.gt), ops.ptr(k.counts), st_)
    k.pred = torch.full((B, A, 4), NAN, device="cuda")
    _C.call("dy_loss_decode", C.byref(dm), ops.ptr(k.pred), st_)
    k.y = torch.full((B, 4 + nc, A), NAN, device="cuda")
    _C.call("dy_detect_decode", C.byref(dm), ops.ptr(k.y), st_)
    k.out = _assign_outputs(B, A)
    wf, wi, wb = _work(B, n_max, A)
    _C.call("dy_tal_assign", C.byref(dm), ops.ptr(k.pred), ops.ptr(k.gt), ops.ptr(k.counts), n_max, ops.ptr(wf), ops.ptr(wi), ops.ptr(wb),
            ops.ptr(k.out["gi"]), ops.ptr(k.out["fg"]), ops.ptr(k.out["norm"]), ops.ptr(k.out["label"]), ops.ptr(k.out["tbox"]), st_)
    k.acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    args = (C.byref(dm), ops.ptr(k.pred), ops.ptr(k.out["fg"]), ops.ptr(k.out["norm"]), ops.ptr(k.out["label"]), ops.ptr(k.out["tbox"]))
    _C.call("dy_loss_fwd", *args, ops.ptr(k.acc), st_)
    k.acc1 = k.acc.clone()
    _C.call("dy_loss_fwd", *args, ops.ptr(k.acc), st_)
    torch.cuda.synchronize()
    k.scores = k.y[:, 4:].permute(0, 2, 1).contiguous()                 # the kernels' own sigmoid
    k.asg = R.assignment(case, gt=k.gt.cpu(), pred=k.pred.cpu(), scores=k.scores.cpu())
    k.st = R.statement(case, k.asg)
    _chains[(run, dn)] = k
    return k


# ---- dy_loss_prepare_targets ----------------------------------------------------------------------------------------------------------
def _targets_ref(bi, cl, bb, B, n_max, W, H):
    """float64 rows [B, n_max, 5] and the counts: rank by order of appearance, the first n_max of an image kept, ids outside [0, B)
    dropped, unused rows zero."""
    gt, counts = torch.zeros(B, n_max, 5, dtype=torch.float64), [0] * B
    for t in range(len(bi)):
        b = int(bi[t])
        if not 0 <= b < B:
            continue
        if counts[b] < n_max:
            cx, cy, w, h = (float(bb[t][0]) * W, float(bb[t][1]) * H, float(bb[t][2]) * W, float(bb[t][3]) * H)
            gt[b, counts[b]] = torch.tensor([float(cl[t]), cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], dtype=torch.float64)
        counts[b] += 1
    return gt, counts


def _check_targets(got, counts, bi, cl, bb, B, n_max, W, H, what):
    ref, cref = _targets_ref(bi.tolist(), cl.tolist(), bb.tolist(), B, n_max, W, H)
    got = got.cpu().double()
    assert counts.cpu().tolist() == cref, (what, counts.cpu().tolist(), cref)
    assert torch.equal(got[..., 0], ref[..., 0]), f"{what}: labels / row order"
    ulp = 2.0 ** (np.floor(np.log2(max(W, H))) - 23)
    err = (got[..., 1:] - ref[..., 1:]).abs()
    print(f"{what}: largest coordinate error {float(err.max()) / ulp:.3g} ulp at image scale")
    assert bool(torch.isfinite(got).all()) and float(err.max()) <= 4 * ulp, what
    used = torch.zeros(B, n_max, dtype=torch.bool)
    for b in range(B):
        used[b, :min(cref[b], n_max)] = True
    assert bool((got[~used] == 0).all()), f"{what}: unused rows not zero"


def test_prepare_targets():
    from dedark_yolo_amd import _C, ops
    for cid in R.CASES:                                       # every case's batch: unsorted ids, an image without boxes
        k = _chain((cid, "unit"), "f32")
        c = k.case
        _check_targets(k.gt, k.counts, c.batch_idx, c.cls.view(-1), c.bboxes, c.B, k.n_rows, c.img_w, c.img_h, cid)
    # counts > n_max (the first n_max stay), ids outside [0, B), an image without boxes
    bi = torch.tensor([2., 0, 5, 2, -1, 2, 0, 0, 3])
    g = torch.Generator().manual_seed(3)
    cl, bb = torch.arange(9.0) + 1, torch.rand(9, 4, generator=g) * 0.5 + 0.1
    B, n_max, W, H = 3, 2, 568.0, 72.0
    gt = torch.full((B, n_max, 5), NAN, device="cuda")
    counts = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    dbi, dcl, dbb = bi.cuda(), cl.cuda(), bb.cuda()
    _C.call("dy_loss_prepare_targets", ops.ptr(dbi), ops.ptr(dcl), ops.ptr(dbb), 9, B, n_max, W, H, ops.ptr(gt), ops.ptr(counts), ops.stream())
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [3, 0, 3]
    _check_targets(gt, counts, bi, cl, bb, B, n_max, W, H, "truncated")
    gt.fill_(NAN)
    counts.fill_(-7)
    _C.call("dy_loss_prepare_targets", None, None, None, 0, B, n_max, W, H, ops.ptr(gt), ops.ptr(counts), ops.stream())
    torch.cuda.synchronize()
    assert bool((gt == 0).all()) and counts.cpu().tolist() == [0, 0, 0]


# ---- decodes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run,dn", RUN_DT, ids=RUN_IDS)
def test_decodes(run, dn):
    """dy_loss_decode, dy_detect_decode, dy_detect_decode_rows (rows = 4 + nc + 5, the extra rows left as they were) and the identity
    pass of dy_detect_decode_tta, on sliced views with NaN in every foreign lane."""
    from dedark_yolo_amd import _C, ops
    k = _chain(run, dn)
    c, nc = k.case, k.case.nc
    _ok("dy_loss_decode", R.compare(f"decode {R.run_id(run)} {dn}", k.pred.cpu(), *k.st["pred"], R.C["decode"], n_terms=17))
    _ok("dy_detect_decode", R.compare(f"y {R.run_id(run)} {dn}", k.y.cpu(), *k.st["y"], R.C["y"], n_terms=17))
    rows = 4 + nc + 5
    y2 = torch.full((c.B, rows, c.A), NAN, device="cuda")
    _C.call("dy_detect_decode_rows", C.byref(k.dm), ops.ptr(y2), rows, ops.stream())
    y3 = torch.full((c.B, 4 + nc, c.A), NAN, device="cuda")
    _C.call("dy_detect_decode_tta", C.byref(k.dm), ops.ptr(y3), c.A, 0, 0, c.A, 1.0, 0, float(c.img_h), float(c.img_w), ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(y2[:, :4 + nc], k.y), "dy_detect_decode_rows differs from dy_detect_decode"
    assert bool(torch.isnan(y2[:, 4 + nc:]).all()), "dy_detect_decode_rows wrote past row 4 + nc"
    assert torch.equal(y3, k.y), "the identity pass of dy_detect_decode_tta differs from dy_detect_decode"
    _ok("dy_detect_decode_rows", R.compare(f"y rows {R.run_id(run)} {dn}", y2[:, :4 + nc].cpu(), *k.st["y"], R.C["y"], n_terms=17))


# ---- assigner ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run,dn", RUN_DT, ids=RUN_IDS)
def test_assigner(run, dn):
    """dy_tal_assign: the discrete outcome bit-exact against the oracle on the same inputs (639, 640 and 641 anchors included), norm
    under the fp64 budget given that outcome; dy_tal_assign_decoded on the same problem agrees bit for bit."""
    from dedark_yolo_amd import _C, ops
    k = _chain(run, dn)
    c, a, o = k.case, k.asg, k.out
    fg = a.fg
    assert torch.equal(o["fg"].cpu().bool(), fg) and int(o["fg"].max()) <= 1, "fg_mask differs"
    assert torch.equal(o["gi"].cpu().long(), a.gt_idx), "target_gt_idx differs"
    assert torch.equal(o["label"].cpu().long()[fg], a.label[fg]), "labels on the foreground differ"
    assert int(o["label"].min()) >= 0 and int(o["label"].max()) < c.nc
    assert torch.equal(o["tbox"].cpu(), a.tbox), "target_box differs"
    for b, want in enumerate(c.spec["min_pos"]):
        n = int(fg[b].sum())
        assert (n == want) if want <= 1 else (n >= want), (b, n)
    _ok("dy_tal_assign", R.compare(f"norm {R.run_id(run)} {dn}", o["norm"].cpu(), *k.st["norm"], R.C["norm"], n_terms=3))
    px = (c.anchors * c.stride).cuda().contiguous()
    boxes = (k.pred * c.stride.cuda()).contiguous()
    o2 = _assign_outputs(c.B, c.A)
    wf, wi, wb = _work(c.B, k.n_max, c.A)
    _C.call("dy_tal_assign_decoded", ops.ptr(k.scores), ops.ptr(boxes), ops.ptr(px), ops.ptr(k.gt), ops.ptr(k.counts), c.B, c.A, c.nc, k.n_max,
            ops.ptr(wf), ops.ptr(wi), ops.ptr(wb), ops.ptr(o2["gi"]), ops.ptr(o2["fg"]), ops.ptr(o2["norm"]), ops.ptr(o2["label"]),
            ops.ptr(o2["tbox"]), ops.stream())
    torch.cuda.synchronize()
    for name in o:
        assert torch.equal(o[name], o2[name]), f"dy_tal_assign_decoded: {name} differs from dy_tal_assign"
    _ok("dy_tal_assign_decoded", R.compare(f"norm (decoded entry) {R.run_id(run)} {dn}", o2["norm"].cpu(), *k.st["norm"], R.C["norm"], n_terms=3))


# ---- forward sums, finish ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run,dn", RUN_DT, ids=RUN_IDS)
def test_loss_fwd(run, dn):
    k = _chain(run, dn)
    c = k.case
    acc, (ref, m) = k.acc1.cpu(), k.st["acc"]
    terms = (c.B * c.A, c.B * c.A * c.nc, max(1, int(k.asg.fg.sum())), max(1, int(k.asg.fg.sum())))
    for i, key in enumerate(R.ACC_KEYS):
        _ok("dy_loss_fwd", R.compare(f"{key} {R.run_id(run)} {dn}", acc[i], ref[i], m[i], R.C[key], n_terms=terms[i]))
    two = k.acc.cpu()
    assert bool(((two - 2 * acc).abs() <= 1e-12 * (2 * acc).abs()).all()), (two, acc)
    if "weak" in c.spec["conds"]:
        assert 0.0 < float(acc[0]) < 1.0


def _finish_ref(acc, rec, hb, hc, hd, lrl, B):
    """loss_finish_kernel in numpy f32; the two results of `total += lrl * rec` (contracted to one multiply-add, or not)."""
    f = np.float32
    tss = max(f(acc[0]), f(1))
    box, cls, dfl = f(acc[2]) / tss * f(hb), f(acc[1]) / tss * f(hc), f(acc[3]) / tss * f(hd)
    total = (box + cls + dfl) * f(B)
    if rec is None:
        return [(total, box, cls, dfl)]
    prod = f(lrl) * f(rec)
    exact = np.float64(f(lrl)) * np.float64(f(rec))
    return [(total + prod, box, cls + prod, dfl), (f(np.float64(total) + exact), box, f(np.float64(cls) + exact), dfl),
            (total + prod, box, f(np.float64(cls) + exact), dfl), (f(np.float64(total) + exact), box, cls + prod, dfl)]


@pytest.mark.parametrize("rec", [None, 0.05])
@pytest.mark.parametrize("acc", [(5.17, 31.3, 2.9, 6.1), (0.408, 12.7, 0.21, 0.9), (0.0, 3.3, 0.0, 0.0)], ids=["tss5", "tss_below_1", "no_positives"])
def test_loss_finish_exact(acc, rec):
    from dedark_yolo_amd import _C, ops
    for (hb, hc, hd), lrl, B in ((R.HYP, 2.0, 3), (R.HYP2, 0.7, 1)):
        d_acc = torch.tensor(acc, dtype=torch.float64, device="cuda")
        d_rec = None if rec is None else torch.tensor([rec], device="cuda")
        out = torch.full((4,), NAN, device="cuda")
        _C.call("dy_loss_finish", ops.ptr(d_acc), ops.ptr(d_rec), hb, hc, hd, lrl, B, ops.ptr(out[0:1]), ops.ptr(out[1:4]), ops.stream())
        torch.cuda.synchronize()
        got = tuple(np.float32(v) for v in out.cpu().tolist())
        want = _finish_ref(acc, rec, hb, hc, hd, lrl, B)
        assert got in want, (got, want)


@pytest.mark.parametrize("run,dn", [(("sq84", "unit"), "f32"), (("two", "unit"), "bf16"), (("rect840", "init"), "f16")])
def test_loss_finish_on_the_runs(run, dn):
    """loss and items from the device accumulators against the fp64 statement: each item inherits the budgets of its accumulator and
    of tss."""
    from dedark_yolo_amd import _C, ops
    k = _chain(run, dn)
    out = torch.full((4,), NAN, device="cuda")
    _C.call("dy_loss_finish", ops.ptr(k.acc1), None, *R.HYP, 0.0, k.case.B, ops.ptr(out[0:1]), ops.ptr(out[1:4]), ops.stream())
    torch.cuda.synchronize()
    ref, m = k.st["acc"]
    tss = max(float(ref[0]), 1.0)
    m_items = torch.stack([R.HYP[j] * m[i] / tss * (R.C[R.ACC_KEYS[i]] + R.C["acc_ts"] + 8) for j, i in ((0, 2), (1, 1), (2, 3))])
    _ok("dy_loss_finish", R.compare(f"items {R.run_id(run)} {dn}", out[1:4].cpu(), k.st["items"], m_items, 1.0))
    _ok("dy_loss_finish", R.compare(f"loss {R.run_id(run)} {dn}", out[0].cpu(), k.st["loss"], m_items.sum() * k.case.B, 1.0))


# ---- backward ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run,dn", RUN_DT, ids=RUN_IDS)
def test_loss_bwd(run, dn):
    """Every gradient element of every level under budget, for grad_out null, 1 and 0.37 and two sets of gains; pad lanes exactly 0;
    the guard words around each buffer untouched."""
    from dedark_yolo_amd import _C, ops
    k = _chain(run, dn)
    c, dtype, o = k.case, k.dtype, k.out
    no, ld = 64 + c.nc, 64 + ops.round_up(c.nc, ops.vec_elems(dtype))
    GUARD, SENT = 64, 4096.0
    cs = R.grad_constants(c.nc)
    for hyp, go in ((R.HYP, None), (R.HYP, 1.0), (R.HYP2, 0.37)):
        st = k.st if (hyp, go) == (R.HYP, 1.0) or go is None else R.statement(c, k.asg, hyp=hyp, grad_out=go)
        bufs = []
        for h, w, _ in c.levels:
            n = c.B * h * w * ld
            buf = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device="cuda")
            buf[GUARD:GUARD + n] = NAN
            bufs.append((buf, n))
        arr_p = (C.c_void_p * len(bufs))(*[b.data_ptr() + GUARD * b.element_size() for b, _ in bufs])
        arr_l = (C.c_int64 * len(bufs))(*([ld] * len(bufs)))
        g = None if go is None else torch.tensor([go], device="cuda")
        _C.call("dy_loss_bwd", C.byref(k.dm), arr_p, arr_l, ops.ptr(k.pred), ops.ptr(o["fg"]), ops.ptr(o["norm"]), ops.ptr(o["label"]),
                ops.ptr(o["tbox"]), ops.ptr(k.acc1), ops.ptr(g), *hyp, ops.stream())
        torch.cuda.synchronize()
        got = []
        for i, ((buf, n), (h, w, _)) in enumerate(zip(bufs, c.levels)):
            assert bool((buf[:GUARD].float() == SENT).all()) and bool((buf[GUARD + n:].float() == SENT).all()), f"map {i}: wrote outside"
            body = buf[GUARD:GUARD + n].float().view(c.B, h * w, ld)
            assert bool((body[..., no:] == 0).all()), f"map {i}: pad lanes not zero"
            got.append(body[..., :no].cpu())
        got = torch.cat(got, 1)
        ref, m = st["grad"]
        name = f"{R.run_id(run)} {dn} gains {hyp} grad_out {go}"
        _ok("dy_loss_bwd", R.compare("d loss / d dist " + name, got[..., :64], ref[..., :64], m[..., :64], cs[:64], dtype, n_terms=3))
        _ok("dy_loss_bwd", R.compare("d loss / d cls " + name, got[..., 64:], ref[..., 64:], m[..., 64:], cs[64:], dtype, n_terms=2))


# ---- stand-alone terms -------------------------------------------------------------------------------------------------------------------------
def _tile(t, n):
    return t[torch.arange(n) % t.shape[0]].contiguous()


@pytest.mark.parametrize("n", [0, 1, 255, 257, 1000])
def test_bbox_iou_entries(n):
    """dy_bbox_ciou and the eight modes of dy_bbox_iou: value and gradient under budget on the case list's positives and the edge
    boxes (the last n of the list, so that the edge boxes are in every size), gradient pointer null and given."""
    from dedark_yolo_amd import _C, ops
    for xywh in (0, 1):
        b1, b2 = R.iou_inputs(xywh)
        b1, b2 = _tile(b1.flip(0), n), _tile(b2.flip(0), n)
        d1, d2 = b1.cuda(), b2.cuda()
        for kind in range(4):
            key = R.iou_key(xywh, kind)
            out0, out1 = torch.full((max(n, 1),), NAN, device="cuda"), torch.full((max(n, 1),), NAN, device="cuda")
            grad = torch.full((max(n, 1), 4), NAN, device="cuda")
            p = (lambda t: ops.ptr(t) if n else None)
            _C.call("dy_bbox_iou", p(d1), p(d2), n, xywh, kind, 1e-7, p(out0), None, ops.stream())
            _C.call("dy_bbox_iou", p(d1), p(d2), n, xywh, kind, 1e-7, p(out1), p(grad), ops.stream())
            outs = [(out0, None), (out1, grad)]
            if key == "ciou_xyxy":
                oc0, oc1, gc = torch.full_like(out0, NAN), torch.full_like(out0, NAN), torch.full_like(grad, NAN)
                _C.call("dy_bbox_ciou", p(d1), p(d2), n, p(oc0), None, ops.stream())
                _C.call("dy_bbox_ciou", p(d1), p(d2), n, p(oc1), p(gc), ops.stream())
                outs += [(oc0, None), (oc1, gc)]
            torch.cuda.synchronize()
            if n == 0:
                assert all(bool(torch.isnan(v).all()) and (g is None or bool(torch.isnan(g).all())) for v, g in outs)
                continue
            ref, m, gref, gm = R.iou_ref(b1, b2, xywh, kind)
            for j, (v, g) in enumerate(outs):
                entry = "dy_bbox_ciou" if j >= 2 else "dy_bbox_iou"
                _ok(entry, R.compare(f"{key} n={n}", v.cpu(), ref, m, R.C[key], n_terms=3))
                if g is not None:
                    _ok(entry, R.compare(f"{key} gradient n={n}", g.cpu(), gref, gm, R.C[key + "_grad"], n_terms=3))


@pytest.mark.parametrize("n", [0, 1, 255, 257, 1000])
def test_dfl_entry(n):
    from dedark_yolo_amd import _C, ops
    _, _, ds, ts = R.standalone_inputs()
    ds, ts = _tile(ds.flip(0), n), _tile(ts.flip(0), n)
    dd, dt = ds.cuda(), ts.cuda()
    out0, out1 = torch.full((max(n, 1),), NAN, device="cuda"), torch.full((max(n, 1),), NAN, device="cuda")
    grad = torch.full((max(n, 1), 4, 16), NAN, device="cuda")
    p = (lambda t: ops.ptr(t) if n else None)
    _C.call("dy_dfl_loss", p(dd), p(dt), n, p(out0), None, ops.stream())
    _C.call("dy_dfl_loss", p(dd), p(dt), n, p(out1), p(grad), ops.stream())
    torch.cuda.synchronize()
    if n == 0:
        assert bool(torch.isnan(out0).all()) and bool(torch.isnan(out1).all()) and bool(torch.isnan(grad).all())
        return
    ref, m, gref, gm = R.dfl_ref(ds, ts)
    _ok("dy_dfl_loss", R.compare(f"dfl n={n}", out0.cpu(), ref, m, R.C["dfl"], n_terms=4))
    _ok("dy_dfl_loss", R.compare(f"dfl (with gradient) n={n}", out1.cpu(), ref, m, R.C["dfl"], n_terms=4))
    _ok("dy_dfl_loss", R.compare(f"dfl gradient n={n}", grad.cpu(), gref, gm, R.C["dfl_grad"], n_terms=2))


# ---- dy_preprocess_batch ---------------------------------------------------------------------------------------------------------------------
# f32 roundings behind one block's partial at n = 4807: 16 pixels and a tail pixel per thread at most (9 additions), 8 levels of the
# block sum; the blocks' partials then add up in f64.  48 leaves the order of the additions open.
C_MSE = 48.0


@pytest.mark.parametrize("flags", [(1, 1), (1, 0), (0, 0)], ids=["lowlight_dedark", "lowlight", "plain"])
def test_preprocess_batch_tail_and_unaligned(flags):
    """n = 16 k + 7 with the input, or an output, one element off 16-byte alignment (the scalar path), and aligned (vector path and
    scalar tail): outputs equal the 256-entry table exactly, mse_acc under budget, mse_acc and clean_out null."""
    from dedark_yolo_amd import _C, ops
    lowlight, dedark = flags
    gamma = 2.2
    st_ = ops.stream()
    ramp = torch.arange(256, dtype=torch.uint8, device="cuda")
    t_img, t_clean = torch.full((256,), NAN, device="cuda"), torch.full((256,), NAN, device="cuda")
    _C.call("dy_preprocess_batch", ops.ptr(ramp), ops.ptr(t_img), ops.ptr(t_clean), gamma, lowlight, dedark, None, 256, st_)
    torch.cuda.synchronize()
    # the table itself: v / 255 correctly rounded, the power within 4 ulp of the fp64 power of that f32 value
    v = (torch.arange(256, dtype=torch.float32) / 255).double()
    want_clean = v ** gamma if (lowlight and dedark) else v
    want_img = v ** gamma if lowlight else v
    tol = 8 * R.EPS32 if lowlight else 0.0
    assert bool(((t_clean.cpu().double() - want_clean).abs() <= (tol if dedark else 0.0) * want_clean).all())
    assert bool(((t_img.cpu().double() - want_img).abs() <= tol * want_img).all())
    n = 16 * 300 + 7
    g = torch.Generator().manual_seed(11)
    pix = torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8)
    d2 = ((t_img.cpu() - t_clean.cpu()) ** 2).double()[pix.long()]          # the f32 terms the kernel adds
    for off_in, off_img, off_clean, with_clean, with_mse in ((0, 0, 0, 1, 1), (1, 0, 0, 1, 1), (0, 1, 0, 1, 0), (0, 0, 1, 1, 1), (0, 0, 0, 0, 1)):
        src = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        src[off_in:off_in + n] = pix.cuda()
        o_img, o_clean = torch.full((n + 8,), NAN, device="cuda"), torch.full((n + 8,), NAN, device="cuda")
        acc = torch.zeros(1, dtype=torch.float64, device="cuda")
        _C.call("dy_preprocess_batch", src.data_ptr() + off_in, o_img.data_ptr() + 4 * off_img, (o_clean.data_ptr() + 4 * off_clean) if with_clean else None,
                gamma, lowlight, dedark, ops.ptr(acc) if with_mse else None, n, st_)
        torch.cuda.synchronize()
        what = f"offsets {off_in} {off_img} {off_clean} clean {with_clean} mse {with_mse}"
        assert torch.equal(o_img[off_img:off_img + n], t_img[pix.cuda().long()]), what
        assert bool(torch.isnan(o_img[:off_img]).all()) and bool(torch.isnan(o_img[off_img + n:]).all()), what
        if with_clean:
            assert torch.equal(o_clean[off_clean:off_clean + n], t_clean[pix.cuda().long()]), what
            assert bool(torch.isnan(o_clean[:off_clean]).all()) and bool(torch.isnan(o_clean[off_clean + n:]).all()), what
        else:
            assert bool(torch.isnan(o_clean).all()), what
        if with_mse:
            _ok("dy_preprocess_batch", R.compare("mse_acc " + what, acc.cpu()[0], d2.sum(), d2.sum(), C_MSE, n_terms=n))
            if lowlight and dedark:
                assert float(acc) == 0.0


# ---- rejections ----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected():
    """One bad argument per entry; the launcher raises before anything runs."""
    from dedark_yolo_amd import _C, ops
    k = _chain(("sq84", "unit"), "f32")
    c, o, s = k.case, k.out, ops.stream()
    dm = k.dm
    f = torch.zeros(64, device="cuda")
    tiny = torch.zeros((1, 84, 3, 3), device="cuda").contiguous(memory_format=torch.channels_last)
    dm9 = ops.det_maps([tiny], [8.0], 20)                                  # 9 anchors
    wide16 = torch.zeros((1, 84, 4, 4), device="cuda").contiguous(memory_format=torch.channels_last)
    narrow = ops.det_maps([wide16], [8.0], 20)
    narrow.map_ld[0] = 83                                                  # ld < 64 + nc
    wf, wi, wb = _work(c.B, k.n_max, c.A)
    a5 = (ops.ptr(o["gi"]), ops.ptr(o["fg"]), ops.ptr(o["norm"]), ops.ptr(o["label"]), ops.ptr(o["tbox"]))
    fwd = (ops.ptr(k.pred), ops.ptr(o["fg"]), ops.ptr(o["norm"]), ops.ptr(o["label"]), ops.ptr(o["tbox"]))
    arr_p = (C.c_void_p * 3)(*([f.data_ptr()] * 3))
    arr_l = (C.c_int64 * 3)(83, 84, 84)
    bad = [
        ("bad args", ("dy_loss_prepare_targets", ops.ptr(f), ops.ptr(f), ops.ptr(f), 1, 2, 2, 64.0, 64.0, None, ops.ptr(f), s)),
        ("null targets", ("dy_loss_prepare_targets", None, ops.ptr(f), ops.ptr(f), 1, 2, 2, 64.0, 64.0, ops.ptr(f), ops.ptr(f), s)),
        ("dy_loss_decode: null", ("dy_loss_decode", C.byref(dm), None, s)),
        (r"empty problem \(A=9\)", ("dy_tal_assign", C.byref(dm9), ops.ptr(k.pred), ops.ptr(k.gt), ops.ptr(k.counts), k.n_max, ops.ptr(wf), ops.ptr(wi),
                                    ops.ptr(wb), *a5, s)),
        ("null work buffers", ("dy_tal_assign", C.byref(dm), ops.ptr(k.pred), ops.ptr(k.gt), ops.ptr(k.counts), k.n_max, None, ops.ptr(wi), ops.ptr(wb),
                               *a5, s)),
        (r"empty problem \(A=9\)", ("dy_tal_assign_decoded", ops.ptr(f), ops.ptr(f), ops.ptr(f), ops.ptr(k.gt), ops.ptr(k.counts), 1, 9, 2, 1, ops.ptr(wf),
                                    ops.ptr(wi), ops.ptr(wb), *a5, s)),
        ("bad level 0", ("dy_loss_fwd", C.byref(narrow), *fwd, ops.ptr(k.acc), s)),
        ("dy_loss_fwd: null", ("dy_loss_fwd", C.byref(dm), *fwd, None, s)),
        ("dy_loss_finish: null", ("dy_loss_finish", None, None, 7.5, 0.5, 1.5, 0.0, 2, ops.ptr(f), ops.ptr(f), s)),
        ("bad dmap 0", ("dy_loss_bwd", C.byref(dm), arr_p, arr_l, *fwd, ops.ptr(k.acc1), None, 7.5, 0.5, 1.5, s)),
        ("dy_bbox_ciou: null operand", ("dy_bbox_ciou", ops.ptr(f), None, 1, ops.ptr(f), None, s)),
        ("kind 4", ("dy_bbox_iou", ops.ptr(f), ops.ptr(f), 1, 0, 4, 1e-7, ops.ptr(f), None, s)),
        ("dy_dfl_loss: null operand", ("dy_dfl_loss", ops.ptr(f), ops.ptr(f), 1, None, None, s)),
        ("rows < 4", ("dy_detect_decode_rows", C.byref(dm), ops.ptr(f), 4 + c.nc - 1, s)),
        ("null output", ("dy_detect_decode", C.byref(dm), None, s)),
        (r"outside the pass's 84", ("dy_detect_decode_tta", C.byref(dm), ops.ptr(f), 100, 0, 0, 85, 1.0, 0, 64.0, 64.0, s)),
        ("dy_preprocess_batch: bad args", ("dy_preprocess_batch", ops.ptr(f), ops.ptr(f), None, 2.2, 1, 1, None, 0, s)),
    ]
    for msg, call in bad:
        with pytest.raises(RuntimeError, match=msg):
            _C.call(*call)
    torch.cuda.synchronize()


def test_zz_largest_ratio_per_entry():
    """Closing line of the module: per entry, the largest ratio to its budget and the smallest power margin seen above."""
    for e in sorted(_figures):
        v = _figures[e]
        print(f"{e}: largest ratio to budget {v[0]:.3g} ({v[1]}), smallest power margin {v[2]:.3g} ({v[3]})")
    assert all(v[0] <= 1.0 for v in _figures.values())
