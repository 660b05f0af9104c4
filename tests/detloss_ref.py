"""Float64 statement of the detection criterion (csrc/loss.hip) with element-wise error budgets, and the case list that the CPU and
GPU tests share.  Plain torch on the CPU; nothing here calls a dedark_yolo_amd kernel.

For maps rounded to the compute dtype and a FROZEN discrete assignment (fg_mask, target_gt_idx, target_label, target_box: the fp32
oracle's, oracle/loss.py::tal_assign) `statement()` returns, each with the magnitude sum M of its terms (the same expression on
absolute values): the decoded boxes (grid units), the per-anchor target score norm = align * pos_overlap / (pos_align + 1e-9) with
align = sigmoid(cls)^0.5 * max(CIoU, 0)^6, the four accumulators [sum norm, sum BCE, sum (1 - CIoU) w, sum DFL w], loss / items of
dy_loss_finish, d loss / d map by autograd (CIoU's alpha constant, as the reference has it) and the eval decode y.  `iou_ref()` and
`dfl_ref()` do the same for the stand-alone entries.  The budget of element i follows tests/conv_budget_ref.py:

    |got_i - ref_i| <= u_out * |ref_i| + (1 + u_out) * c * 2^-24 * M_i          (+ 2^-25 for f16 outputs: subnormal floor)

u_out: unit roundoff of the output type; only the gradient maps are 16-bit.  M: class gradient go hc (sigma + t); distribution
gradient kd (p_k + wl + wr) + |p_k (k - e) dd_s|; a sum: the sum of |terms|; a decoded coordinate: anchor + distance; norm: the
value times its first-order condition number 1 + 6 R_a + (1 + 6 R) at the group's best align + R at its best overlap, R = (iou +
rho2 / c2 + v alpha) / CIoU; IoU values: iou + |penalty terms|; IoU gradients: the sum of the |gradients| of those terms.

c is one constant per result class and is NOT tuned on the kernels: 8 times the largest |r32 - r64| / (2^-24 M) that the SAME
statement reaches in fp32 on the CPU (oracle/loss.py's decode_boxes / ciou / bbox_iou / dfl_loss and torch's own softmax, sigmoid and
autograd) over RUNS x {f32, bf16, f16}; `python tests/detloss_ref.py` re-measures (under a minute).  The factor 8 as for the convs:
the kernels sum in another order and use the device's expf / logf / atanf / powf.

    result class        measured   c = 8 x
    decode                 5.160       41.28
    norm                  15.500      124.00
    bce                   60.600      484.80   one BCE element, log1p form
    acc_ts                29.400      235.20
    acc_bce               11.800       94.40   log1p form
    acc_iou               31.100      248.80
    acc_dfl               30.400      243.20
    grad_cls              83.000      664.00   carries 1 / tss
    grad_dist            419.000     3352.00   rect840:peaked; 30 .. 210 on the other laws
    y                      4.340       34.72
    dfl                    1.670       13.36
    dfl_grad              17.400      139.20
    iou_xyxy               3.330       26.64
    giou_xyxy              0.775        6.20
    diou_xyxy              3.670       29.36
    ciou_xyxy              3.790       30.32
    iou_xywh               5.790       46.32
    giou_xywh              1.090        8.72
    diou_xywh              5.040       40.32
    ciou_xywh              4.350       34.80
    iou_xyxy_grad          4.580       36.64
    giou_xyxy_grad         1.480       11.84
    diou_xyxy_grad        35.500      284.00
    ciou_xyxy_grad        28.000      224.00
    iou_xywh_grad          6.770       54.16
    giou_xywh_grad         2.380       19.04
    diou_xywh_grad        57.300      458.40
    ciou_xywh_grad        57.300      458.40
    bce (torch formula)   16800000        -    = 2^24: the element is lost entirely
    acc_bce (torch f.)     11700        -    empty:init, where no positive's x t term carries the sum (13.7 elsewhere)

BCE: torch's fp32 binary_cross_entropy_with_logits computes log(exp(-m) + exp(-x - m)), which loses the whole element once
exp(-|x|) < 2^-24 and most of it before (`init` law: class logits N(-11.5, 1), what the Detect bias init produces; `wide` law).  As a
yardstick it is useless, for one element and for the sum of a batch without positives (empty:init).  Both BCE constants are therefore
taken from the same expressions evaluated as max(x, 0) - x t + log1p(exp(-|x|)) in fp32, which is still torch on the CPU and not the
code under test.  M of one BCE element: max(x, 0) + |x t| + log1p(exp(-|x|)).
"""
import math
import os
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import loss as oloss              # noqa: E402
from oracle.model import make_anchors         # noqa: E402

EPS32 = 2.0 ** -24
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
F16_FLOOR = 2.0 ** -25
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
REG = 16
HYP = (7.5, 0.5, 1.5)
HYP2 = (0.05, 3.0, 0.4)
KINDS = ("iou", "giou", "diou", "ciou")

# largest |r32 - r64| / (2^-24 M) over RUNS x dtypes (measure() below); C = 8 x
MEASURED = {
    "decode": 5.16, "norm": 15.5, "bce": 60.6, "acc_ts": 29.4, "acc_bce": 11.8,
    "acc_iou": 31.1, "acc_dfl": 30.4, "grad_cls": 83.0, "grad_dist": 419, "y": 4.34,
    "dfl": 1.67, "dfl_grad": 17.4, "iou_xyxy": 3.33, "giou_xyxy": 0.775, "diou_xyxy": 3.67,
    "ciou_xyxy": 3.79, "iou_xywh": 5.79, "giou_xywh": 1.09, "diou_xywh": 5.04, "ciou_xywh": 4.35,
    "iou_xyxy_grad": 4.58, "giou_xyxy_grad": 1.48, "diou_xyxy_grad": 35.5, "ciou_xyxy_grad": 28.0, "iou_xywh_grad": 6.77,
    "giou_xywh_grad": 2.38, "diou_xywh_grad": 57.3, "ciou_xywh_grad": 57.3,
}
MEASURED_TORCH_BCE = {"acc_bce": 11700, "bce": 16800000}         # torch's fp32 BCE formula on the same sums / elements: reported, not used
C = {k: 8.0 * v for k, v in MEASURED.items()}

# ---- cases -------------------------------------------------------------------------------------------------------------------
# levels: (h, w, stride); boxes: (image, class, x1, y1, x2, y2) in pixels, in the order they appear in the batch (batch_idx is
# unsorted on purpose); conds: the conditions the CPU test shows to occur; min_pos: positives expected per image.
_SQ = [(8, 8, 8.0), (4, 4, 16.0), (2, 2, 32.0)]
_SQ_BOXES = [(2, 3, -40.0, -10.0, 50.0, 60.0),        # partly outside the image
             (0, 5, 11.7, 10.0, 27.0, 30.0),          # left edge 0.3 px from the anchor centres at x = 12
             (0, 1, 41.0, 41.0, 43.0, 43.0),          # holds no anchor centre
             (0, 2, 34.0, 6.0, 62.0, 34.0),           # two identical boxes, two classes
             (0, 7, 34.0, 6.0, 62.0, 34.0)]
CASES = {
    "sq84": dict(levels=_SQ, nc=20, B=3, boxes=_SQ_BOXES, min_pos=[10, 0, 10],
                 conds=("lower_clamp", "empty_gt", "tie_first", "outside", "empty_image", "unsorted")),
    "rect840": dict(levels=[(20, 32, 8.0), (10, 16, 16.0), (5, 8, 32.0)], nc=3, B=2, min_pos=[10, 10],
                    boxes=[(1, 2, 99.7, 51.7, 131.0, 91.0), (0, 0, 3.0, 20.0, 253.0, 140.0), (1, 1, 200.0, 100.0, 300.0, 200.0)],
                    conds=("lower_clamp", "outside", "unsorted")),
    "one639": dict(levels=[(9, 71, 8.0)], nc=20, B=2, min_pos=[10, 10],
                   boxes=[(0, 4, 100.0, 10.0, 200.0, 60.0), (1, 11, 250.0, 20.0, 330.0, 60.0), (0, 9, 300.0, -20.0, 420.0, 50.0),
                          (0, 0, 10.0, 2.0, 560.0, 70.0)],
                   conds=("upper_clamp", "outside", "unsorted")),
    "one640": dict(levels=[(20, 32, 8.0)], nc=20, B=2, min_pos=[10, 10],
                   boxes=[(1, 2, 99.7, 51.7, 131.0, 91.0), (0, 0, 3.0, 5.0, 253.0, 155.0), (0, 7, 60.0, 40.0, 120.0, 100.0)],
                   conds=("upper_clamp", "lower_clamp", "unsorted")),
    "one641": dict(levels=[(1, 641, 8.0)], nc=20, B=2, min_pos=[10, 10],
                   boxes=[(0, 1, 100.0, -30.0, 400.0, 38.0), (1, 19, 2000.0, -40.0, 2300.0, 48.0), (0, 6, 1000.0, -20.0, 1100.0, 28.0),
                          (0, 3, 3000.0, -50.0, 3500.0, 58.0)],
                   conds=("upper_clamp", "outside", "unsorted")),
    "two": dict(levels=[(8, 6, 16.0), (4, 3, 32.0)], nc=1, B=2, min_pos=[1, 0],
                boxes=[(0, 0, 17.0, 17.0, 39.0, 39.0)],          # holds the one centre (24, 24): a single weak positive
                conds=("weak", "empty_image")),
    "four": dict(levels=[(24, 32, 4.0), (12, 16, 8.0), (6, 8, 16.0), (3, 4, 32.0)], nc=80, B=2, min_pos=[10, 10],
                 boxes=[(1, 41, 30.0, 20.0, 100.0, 80.0), (0, 79, 10.0, 10.0, 70.0, 60.0), (1, 17, -10.0, 40.0, 40.0, 110.0),
                        (0, 0, 64.0, 30.0, 120.0, 90.0)],
                 conds=("outside", "unsorted")),
    # no box at all: the assigner's n_max = 0 path, and sums that the negatives alone carry (on the `init` law the BCE sum is made of
    # elements of 1e-5 and less, where a formula that rounds 1 + exp(-|x|) first is off by 1e-3 of the sum and more)
    "empty": dict(levels=_SQ, nc=20, B=2, boxes=[], min_pos=[0, 0], conds=()),
    "nc81": dict(levels=_SQ, nc=81, B=3, boxes=[(b[0], b[1] * 11 + 3, *b[2:]) for b in _SQ_BOXES], min_pos=[10, 0, 10],
                 conds=("lower_clamp", "empty_gt", "tie_first", "outside", "empty_image", "unsorted")),
}
LAWS = ("unit", "init", "peaked", "wide")
RUNS = [(c, "unit") for c in CASES] + [(c, l) for l in ("init", "peaked") for c in ("rect840", "sq84")] + [("sq84", "wide"), ("empty", "init")]
# (case, law) -> seed offset, where the first seed put a positive's predicted edge within 1e-4 grid units of a target edge (the CPU
# test's kink condition): rect840:peaked had a gap of 2.5e-6, seeds +1 .. +4 gaps of 3.7e-5 .. 2.6e-4, +5 has 5.6e-4
SEED = {("rect840", "peaked"): 5}


def run_id(r):
    return f"{r[0]}:{r[1]}"


def make_case(cid, law, dtype):
    """The inputs of one run: X [B, A, 64 + nc] f32 holding values of `dtype` (anchors of all levels in a row, as the kernels
    number them), the batch (batch_idx, cls, normalised xywh boxes, f32) and the geometry."""
    spec = CASES[cid]
    levels, nc, B = spec["levels"], spec["nc"], spec["B"]
    A = sum(h * w for h, w, _ in levels)
    img_w, img_h = levels[0][1] * levels[0][2], levels[0][0] * levels[0][2]
    anchors, stride = make_anchors([(h, w) for h, w, _ in levels], [s for _, _, s in levels])
    g = torch.Generator().manual_seed(1000 * list(CASES).index(cid) + 10 * LAWS.index(law) + SEED.get((cid, law), 0) + 7)
    dist = torch.randn(B, A, 4 * REG, generator=g)
    cls = torch.randn(B, A, nc, generator=g)
    if law == "init":
        dist, cls = dist * 0.1, cls - 11.5
    elif law == "peaked":
        bins = torch.randint(0, REG, (B, A, 4), generator=g)
        dist = (dist.view(B, A, 4, REG) + 12.0 * F.one_hot(bins, REG)).view(B, A, 4 * REG)
        cls = cls - 4.0
        px = anchors * stride
        for b, c, x1, y1, x2, y2 in reversed(spec["boxes"]):          # the first box that holds the anchor names its class
            inside = (px[:, 0] > x1) & (px[:, 0] < x2) & (px[:, 1] > y1) & (px[:, 1] < y2)
            cls[b, inside] = torch.randn(int(inside.sum()), nc, generator=g) - 4.0
            cls[b, inside, c] += 12.0
    elif law == "wide":
        cls = (torch.rand(B, A, nc, generator=g) * 2 - 1) * 60.0
    if cid == "two":          # the one anchor inside the box predicts (0, 0, 1, 1) cells around its centre: IoU about 0.4, a weak positive
        dist.view(B, A, 4, REG)[0, 7, [0, 1, 2, 3], [0, 0, 1, 1]] += 12.0
    X = torch.cat((dist, cls), 2).to(dtype).float()
    bx = torch.tensor([b[2:] for b in spec["boxes"]], dtype=torch.float64).view(-1, 4)
    xywh = torch.stack(((bx[:, 0] + bx[:, 2]) / 2 / img_w, (bx[:, 1] + bx[:, 3]) / 2 / img_h, (bx[:, 2] - bx[:, 0]) / img_w,
                        (bx[:, 3] - bx[:, 1]) / img_h), 1).float()
    return SimpleNamespace(id=cid, law=law, dtype=dtype, levels=levels, nc=nc, B=B, A=A, img_w=img_w, img_h=img_h, anchors=anchors,
                           stride=stride, X=X, batch_idx=torch.tensor([float(b[0]) for b in spec["boxes"]]),
                           cls=torch.tensor([float(b[1]) for b in spec["boxes"]]).view(-1, 1), bboxes=xywh, spec=spec)


def level_maps(case):
    """X split into the per-level maps [B, h, w, 64 + nc] (NHWC)."""
    out, a0 = [], 0
    for h, w, _ in case.levels:
        out.append(case.X[:, a0:a0 + h * w].view(case.B, h, w, -1))
        a0 += h * w
    return out


def assignment(case, gt=None, pred=None, scores=None):
    """The fp32 CPU oracle's targets and assignment for the run: the judge of the discrete outcome.  gt [B, n, 5], pred [B, A, 4]
    (grid units) and scores [B, A, nc] replace the oracle's own target rows, decode and sigmoid where a test has them from the
    kernels under test, so that the assigner is judged on the inputs it was given."""
    X = case.X
    tg = oloss.pad_targets(case.batch_idx, case.cls, case.bboxes, case.B, (case.img_w, case.img_h)) if gt is None else gt
    gt_labels, gt_boxes = tg[..., :1], tg[..., 1:]
    mask_gt = (gt_boxes.sum(2, keepdim=True) > 0).float()
    if pred is None:
        pred = oloss.decode_boxes(X[..., :4 * REG].contiguous(), case.anchors)
    inputs = (X[..., 4 * REG:].sigmoid() if scores is None else scores, pred * case.stride, case.anchors * case.stride)
    lab, tbox, ts, fg, gi = oloss.tal_assign(*inputs, gt_labels, gt_boxes, mask_gt, case.nc)
    return SimpleNamespace(inputs=inputs, gt=tg, counts=torch.bincount(case.batch_idx.long(), minlength=case.B).int(), fg=fg, gt_idx=gi,
                           label=lab.long(), tbox=tbox, norm32=ts.sum(-1), pred32=pred, n_max=tg.shape[1])


def ciou_mag(b1, b2, eps=1e-7):
    """iou + rho2 / c2 + v alpha of CIoU(b1, b2), xyxy: the magnitude sum of its value."""
    x1, y1, x2, y2 = b1.unbind(-1)
    X1, Y1, X2, Y2 = b2.unbind(-1)
    w1, h1, w2, h2 = x2 - x1, y2 - y1 + eps, X2 - X1, Y2 - Y1 + eps
    inter = (torch.minimum(x2, X2) - torch.maximum(x1, X1)).clamp(min=0) * (torch.minimum(y2, Y2) - torch.maximum(y1, Y1)).clamp(min=0)
    iou = inter / (w1 * h1 + w2 * h2 - inter + eps)
    c2 = (torch.maximum(x2, X2) - torch.minimum(x1, X1)) ** 2 + (torch.maximum(y2, Y2) - torch.minimum(y1, Y1)) ** 2 + eps
    rho2 = ((X1 + X2 - x1 - x2) ** 2 + (Y1 + Y2 - y1 - y2) ** 2) / 4
    v = (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
    return iou + rho2 / c2 + v * (v / (v - iou + (1 + eps)))


def bce_torch(x, t):
    return F.binary_cross_entropy_with_logits(x, t, reduction="none")


def bce_log1p(x, t):
    return x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))


def statement(case, asg, dt=torch.float64, hyp=HYP, grad_out=1.0, bce=bce_log1p, ciou=oloss.ciou, dfl=oloss.dfl_loss, label_shift=0,
              norm_overlap=True, clamp_hi=REG - 1 - 0.01):
    """{name: (value, M)} of the module docstring, computed in `dt`.  The trailing arguments exist for the CPU test's wrong
    variants."""
    B, A, nc = case.B, case.A, case.nc
    hb, hc, hd = hyp
    X = case.X.to(dt).clone().requires_grad_(True)
    anc, st = case.anchors.to(dt), case.stride.to(dt)
    dist = X[..., :4 * REG]
    p = dist.view(B, A, 4, REG).softmax(3)
    k = torch.arange(REG, dtype=dt)
    d = p.matmul(k)                                                        # oracle.loss.decode_boxes, with d kept for its gradient
    d.retain_grad()
    pred = torch.cat((anc - d[..., :2], anc + d[..., 2:]), -1)
    out = {"pred": (pred.detach(), torch.cat((anc + d[..., :2], anc + d[..., 2:]), -1).detach())}
    fg, gi, n = asg.fg, asg.gt_idx, asg.gt.shape[1]
    bi, ai = fg.nonzero(as_tuple=True)
    norm, m_norm = torch.zeros(B, A, dtype=dt), torch.zeros(B, A, dtype=dt)
    with torch.no_grad():
        sig = X[..., 4 * REG:].sigmoid()
        if bi.numel():
            j = gi[bi, ai]
            gtb = asg.gt[..., 1:].to(dt)[bi, j]
            lab = asg.gt[..., 0].long().clamp(0, nc - 1)[bi, j]
            pbox = pred[bi, ai] * st[ai]
            o = ciou(gtb, pbox).squeeze(-1).clamp(min=0)
            R = torch.where(o > 0, ciou_mag(gtb, pbox) / o.clamp_min(1e-300), torch.zeros_like(o))
            al = sig[bi, ai, lab].pow(oloss.ALPHA) * o.pow(oloss.BETA)
            grp = bi * n + j
            nv, mv = torch.zeros_like(al), torch.zeros_like(al)
            for gidx in grp.unique():
                sel = (grp == gidx).nonzero().squeeze(1)
                ia, io = al[sel].argmax(), o[sel].argmax()
                po = o[sel][io] if norm_overlap else torch.ones((), dtype=dt)
                nv[sel] = al[sel] * po / (al[sel][ia] + oloss.TAL_EPS)
                mv[sel] = nv[sel] * ((1 + 6 * R[sel]) + (1 + 6 * R[sel][ia]) + R[sel][io])
            norm[bi, ai], m_norm[bi, ai] = nv, mv
    out["norm"] = (norm, m_norm)
    t = torch.zeros(B, A, nc, dtype=dt)
    if bi.numel():
        t[bi, ai, (asg.label[bi, ai] + label_shift).clamp(max=nc - 1)] = norm[bi, ai]
    w = norm[bi, ai]
    e_bce = bce(X[..., 4 * REG:], t)
    tb = asg.tbox.to(dt) / st
    if bi.numel():
        e_iou = (1.0 - ciou(pred[bi, ai], tb[bi, ai])).squeeze(-1) * w
        ltrb = torch.cat((anc - tb[..., :2], tb[..., 2:] - anc), -1).clamp(0, clamp_hi)[bi, ai]
        e_dfl = dfl(dist[bi, ai].reshape(-1, REG), ltrb).squeeze(-1) * w
    else:
        e_iou = e_dfl = ltrb = torch.zeros(0, dtype=dt)
    xc = X[..., 4 * REG:].detach()
    out["bce"] = (e_bce.detach(), xc.clamp(min=0) + (xc * t).abs() + torch.log1p(torch.exp(-xc.abs())))
    acc = torch.stack((norm.sum(), e_bce.sum(), e_iou.sum(), e_dfl.sum()))
    out["acc"] = (acc.detach(), torch.stack((norm.abs().sum(), e_bce.abs().sum(), e_iou.abs().sum(), e_dfl.abs().sum())).detach())
    tss = acc[0].detach().clamp(min=1.0)
    items = torch.stack((acc[2] * hb, acc[1] * hc, acc[3] * hd)) / tss
    loss = items.sum() * B
    out["items"], out["loss"] = items.detach(), loss.detach()
    (loss * grad_out).backward()
    grad = X.grad
    dd = d.grad if d.grad is not None else torch.zeros_like(d)
    go = abs(grad_out) * B / tss
    with torch.no_grad():
        m_cls = go * hc * (sig + t)
        kd = torch.zeros(B, A, dtype=dt)
        wlr = torch.zeros(B, A, 4, REG, dtype=dt)
        if bi.numel():
            kd[bi, ai] = go * hd * w * 0.25
            tl = ltrb.long().clamp(max=REG - 2)
            wl = (tl + 1) - ltrb
            sub = torch.zeros(bi.numel(), 4, REG, dtype=dt)
            sub.scatter_(2, tl.unsqueeze(-1), wl.unsqueeze(-1))
            sub.scatter_(2, (tl + 1).unsqueeze(-1), (1 - wl).unsqueeze(-1))
            wlr[bi, ai] = sub
        m_dist = kd[..., None, None] * (p + wlr) + (p * (k - d.unsqueeze(-1)) * dd.unsqueeze(-1)).abs()
        out["grad"] = (grad.detach(), torch.cat((m_dist.view(B, A, 4 * REG), m_cls), 2))
        x1, y1, x2, y2 = pred.unbind(-1)
        s1 = st.squeeze(-1)
        y_box = torch.stack(((x1 + x2) / 2 * s1, (y1 + y2) / 2 * s1, (x2 - x1) * s1, (y2 - y1) * s1), 1)
        ax, ay = anc[:, 0], anc[:, 1]
        m_box = torch.stack(((ax + (d[..., 0] + d[..., 2]) / 2) * s1, (ay + (d[..., 1] + d[..., 3]) / 2) * s1,
                             (2 * ax + d[..., 0] + d[..., 2]) * s1, (2 * ay + d[..., 1] + d[..., 3]) * s1), 1)
        out["y"] = (torch.cat((y_box, sig.permute(0, 2, 1)), 1), torch.cat((m_box, sig.permute(0, 2, 1)), 1))
        out["ltrb"] = ltrb
    return out


# which constant judges which part of a statement result
def grad_constants(nc):
    return torch.cat((torch.full((4 * REG,), C["grad_dist"]), torch.full((nc,), C["grad_cls"])))


ACC_KEYS = ("acc_ts", "acc_bce", "acc_iou", "acc_dfl")


# ---- stand-alone terms ---------------------------------------------------------------------------------------------------------
def _iou_terms(cor1, wh1, cor2, wh2, kind, eps):
    """The value of oracle.loss.bbox_iou split into its terms (iou, -penalty...), same formulas, as a function of box 1's corners
    (x1, y1, x2, y2) and of its (w, h) as they enter the areas and the aspect term; and gterms: scalar functions whose gradients are
    the additive pieces of the value's gradient (quotient rule written out with detached factors), so that the sum of their
    |gradients| is the magnitude sum of the gradient."""
    x1, y1, x2, y2 = cor1.unbind(-1)
    X1, Y1, X2, Y2 = cor2.unbind(-1)
    (w1, h1), (w2, h2) = wh1.unbind(-1), wh2.unbind(-1)
    inter = (torch.minimum(x2, X2) - torch.maximum(x1, X1)).clamp(min=0) * (torch.minimum(y2, Y2) - torch.maximum(y1, Y1)).clamp(min=0)
    union = w1 * h1 + w2 * h2 - inter + eps
    terms = [inter / union]
    ud, idt, a1 = union.detach(), inter.detach(), w1 * h1
    gterms = [inter / ud, -(idt / ud ** 2) * a1, (idt / ud ** 2) * inter]
    cw, chh = torch.maximum(x2, X2) - torch.minimum(x1, X1), torch.maximum(y2, Y2) - torch.minimum(y1, Y1)
    if kind == 1:
        c_area = cw * chh + eps
        cad = c_area.detach()
        terms += [-c_area / c_area, union / c_area]
        gterms += [a1 / cad, -inter / cad, -(ud / cad ** 2) * c_area]
    elif kind >= 2:
        c2 = cw ** 2 + chh ** 2 + eps
        rho2 = ((X1 + X2 - x1 - x2) ** 2 + (Y1 + Y2 - y1 - y2) ** 2) / 4
        terms.append(-rho2 / c2)
        gterms += [-rho2 / c2.detach(), (rho2.detach() / c2.detach() ** 2) * c2]
        if kind == 3:
            v = (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
            with torch.no_grad():
                a = v / (v - terms[0] + (1 + eps))
            terms.append(-v * a)
            gterms.append(-v * a)
    return terms, gterms


def _corners(b, xywh, eps):
    if xywh:
        x, y, w, h = b.unbind(-1)
        return torch.stack((x - w / 2, y - h / 2, x + w / 2, y + h / 2), -1), torch.stack((w, h), -1)
    return b, torch.stack((b[..., 2] - b[..., 0], b[..., 3] - b[..., 1] + eps), -1)


def iou_ref(b1, b2, xywh, kind, dt=torch.float64, eps=1e-7, fn=oloss.bbox_iou):
    """(value, M, d sum(value) / d b1, M of the gradient) of bbox_iou mode (xywh, kind) in `dt`.  The gradient's M: the |gradient|
    pieces wrt the corners and wrt (w, h), each carried to b1's own coordinates with the absolute values of the chain rule's
    weights (xywh: a corner is centre -/+ half the extent; xyxy: w = x2 - x1, h = y2 - y1 + eps)."""
    b1 = b1.to(dt).clone().requires_grad_(True)
    b2 = b2.to(dt)
    val = fn(b1, b2, xywh=bool(xywh), GIoU=kind == 1, DIoU=kind == 2, CIoU=kind == 3, eps=eps).squeeze(-1)
    g, = torch.autograd.grad(val.sum(), b1)
    cor1, wh1 = (t.detach().clone().requires_grad_(True) for t in _corners(b1, xywh, eps))
    cor2, wh2 = _corners(b2, xywh, eps)
    terms, gterms = _iou_terms(cor1, wh1, cor2, wh2, kind, eps)
    mc, mwh = torch.zeros_like(cor1), torch.zeros_like(wh1)
    for tm in gterms:
        gc, gw = torch.autograd.grad(tm.sum(), (cor1, wh1), retain_graph=True, allow_unused=True)
        mc = mc + (gc.abs() if gc is not None else 0)
        mwh = mwh + (gw.abs() if gw is not None else 0)
    if xywh:
        mg = torch.stack((mc[:, 0] + mc[:, 2], mc[:, 1] + mc[:, 3], (mc[:, 0] + mc[:, 2]) / 2 + mwh[:, 0], (mc[:, 1] + mc[:, 3]) / 2 + mwh[:, 1]), 1)
    else:
        mg = mc + torch.stack((mwh[:, 0], mwh[:, 1], mwh[:, 0], mwh[:, 1]), 1)
    return val.detach(), sum(tm.detach().abs() for tm in terms), g, mg


def dfl_ref(pred, target, dt=torch.float64, fn=oloss.dfl_loss):
    """(value [N], M, d sum(value) / d pred [N, 4, 16], M) of BboxLoss._df_loss; pred [N, 4, 16] logits, target [N, 4]."""
    x = pred.to(dt).clone().requires_grad_(True)
    t = target.to(dt)
    val = fn(x.view(-1, REG), t).squeeze(-1)
    g, = torch.autograd.grad(val.sum(), x)
    with torch.no_grad():
        tl = t.long().clamp(max=REG - 2)
        wl = (tl + 1) - t
        lse = x.logsumexp(-1).abs()
        xl, xr = x.gather(2, tl.unsqueeze(-1)).squeeze(-1).abs(), x.gather(2, (tl + 1).unsqueeze(-1)).squeeze(-1).abs()
        m_val = ((lse + xl) * wl + (lse + xr) * (1 - wl)).mean(-1)
        oh = torch.zeros_like(x)
        oh.scatter_(2, tl.unsqueeze(-1), wl.unsqueeze(-1))
        oh.scatter_(2, (tl + 1).unsqueeze(-1), (1 - wl).unsqueeze(-1))
        m_g = 0.25 * (x.softmax(-1) + oh)
    return val.detach(), m_val, g, m_g


def xyxy_to_xywh(b):
    return torch.stack(((b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]), 1)


# identical, nested (both ways), disjoint, touching edges, shared edges (gradient ties split 1/2), zero width, a point
EDGE_B1 = torch.tensor([[2., 3, 7, 9], [1, 1, 9, 9], [3, 4, 6, 7], [0, 0, 2, 2], [0, 0, 4, 4], [0, 0, 4, 4], [3, 1, 3, 5], [3, 3, 3, 3]])
EDGE_B2 = torch.tensor([[2., 3, 7, 9], [3, 4, 6, 7], [1, 1, 9, 9], [5, 6, 8, 9], [4, 0, 8, 4], [0, 1, 4, 3], [2, 0, 6, 6], [1, 1, 6, 5]])
N_EDGE_XYWH = 7                       # the point box has w = h = 0, which xywh (no eps) turns into 0 / 0
EDGE_T = torch.tensor([[0.0, REG - 1 - 0.01, 0.0375, 3.0], [14.0, 0.5, 7.999, 14.5]])

_pairs = {}


def standalone_inputs():
    """(b1, b2 xyxy [N, 4], dist [N, 4, 16], ltrb [N, 4]) f32: the positives of the sq84 and rect840 runs (predicted box against target box in
    grid units, their distribution logits and DFL targets) followed by the edge inputs."""
    if not _pairs:
        b1, b2, ds, ts = [], [], [], []
        for cid, law in (("sq84", "unit"), ("rect840", "peaked"), ("rect840", "init"), ("one640", "unit")):
            case = make_case(cid, law, torch.float32)
            asg = assignment(case)
            bi, ai = asg.fg.nonzero(as_tuple=True)
            b1.append(asg.pred32[bi, ai])
            b2.append((asg.tbox / case.stride)[bi, ai])
            ds.append(case.X[bi, ai, :4 * REG].view(-1, 4, REG))
            ts.append(torch.cat((case.anchors[ai] - b2[-1][:, :2], b2[-1][:, 2:] - case.anchors[ai]), -1).clamp(0, REG - 1 - 0.01))
        g = torch.Generator().manual_seed(5)
        ds.append(torch.randn(2, 4, REG, generator=g) * 3)
        ts.append(EDGE_T)
        _pairs["v"] = (torch.cat(b1 + [EDGE_B1]), torch.cat(b2 + [EDGE_B2]), torch.cat(ds), torch.cat(ts))
    return _pairs["v"]


def iou_inputs(xywh):
    b1, b2, _, _ = standalone_inputs()
    if xywh:
        n = b1.shape[0] - (EDGE_B1.shape[0] - N_EDGE_XYWH)
        return xyxy_to_xywh(b1[:n]), xyxy_to_xywh(b2[:n])
    return b1, b2


def iou_key(xywh, kind):
    return f"{KINDS[kind]}_{'xywh' if xywh else 'xyxy'}"


def conditions(case, asg, ltrb):
    """Which of the named conditions of the case list occur in a run (ltrb: the DFL targets of the positives, statement()['ltrb'])."""
    img = torch.tensor([0.0, 0.0, case.img_w, case.img_h])
    px = case.anchors * case.stride
    npos = lambda b, j: int((asg.fg[b] & (asg.gt_idx[b] == j)).sum())                    # noqa: E731
    out = dict(upper_clamp=bool((ltrb >= REG - 1 - 0.011).any()), lower_clamp=bool((ltrb < 0.0625).any()), empty_gt=False, tie_first=False,
               outside=False, unsorted=bool((case.batch_idx[1:] < case.batch_idx[:-1]).any()),
               empty_image=bool(((asg.counts == 0) & (asg.fg.sum(1) == 0)).any() and (asg.counts > 0).any()),
               weak=bool(int(asg.fg.sum()) == 1 and 0.0 < float(asg.norm32.sum()) < 1.0))
    for b in range(case.B):
        for j in range(int(asg.counts[b])):
            x1, y1, x2, y2 = asg.gt[b, j, 1:].tolist()
            holds = int(((px[:, 0] > x1) & (px[:, 0] < x2) & (px[:, 1] > y1) & (px[:, 1] < y2)).sum())
            out["empty_gt"] |= holds == 0 and npos(b, j) == 0
            out["outside"] |= (x1 < 0 or y1 < 0 or x2 > img[2] or y2 > img[3]) and npos(b, j) > 0
            for i in range(j):
                if torch.equal(asg.gt[b, i, 1:], asg.gt[b, j, 1:]) and asg.gt[b, i, 0] != asg.gt[b, j, 0]:
                    # the anchors that each of the two would take alone, and that both would: all of those went to the first
                    alone = [oloss.tal_assign(*(t[b:b + 1] if t.dim() == 3 else t for t in asg.inputs), asg.gt[b:b + 1, k:k + 1, :1],
                                              asg.gt[b:b + 1, k:k + 1, 1:], torch.ones(1, 1, 1), case.nc)[3][0] for k in (i, j)]
                    both = alone[0] & alone[1]
                    out["tie_first"] |= bool(both.any() and (asg.fg[b][both]).all() and (asg.gt_idx[b][both] == i).all())
    return out


def kink_gap(case, asg, pred64):
    """Smallest distance (grid units) between a predicted edge and a target edge of the same axis over the positives: the max / min
    kinks of CIoU, where fp32 and fp64 may take different branches."""
    bi, ai = asg.fg.nonzero(as_tuple=True)
    if not bi.numel():
        return float("inf")
    p, t = pred64[bi, ai], (asg.tbox.double() / case.stride.double())[bi, ai]
    gaps = [(p[:, i] - t[:, k]).abs().min() for i, k in ((0, 0), (0, 2), (2, 0), (2, 2), (1, 1), (1, 3), (3, 1), (3, 3))]
    return float(torch.stack(gaps).min())


# ---- budget -----------------------------------------------------------------------------------------------------------------------
def budget(ref, M, c, out_dtype=torch.float32):
    u = U_OUT[out_dtype]
    b = u * ref.abs() + (1.0 + u) * c * EPS32 * M
    return b + F16_FLOOR if out_dtype == torch.float16 else b


class Report:
    """worst: largest |got - ref| / budget, at index `where`; margin: the power margin, the mean single term M / n_terms over the
    budget at the median element (what dropping one term changes, against what the budget lets pass)."""

    def __init__(self, name, worst, where, margin, n):
        self.name, self.worst, self.where, self.margin, self.n = name, worst, where, margin, n

    def __str__(self):
        weak = "  WEAK: median power margin below 4" if self.margin < 4 else ""
        return f"{self.name}: worst {self.worst:.3g} of budget at {self.where}, power margin {self.margin:.3g}, {self.n} elements{weak}"


def compare(name, got, ref, M, c, out_dtype=torch.float32, n_terms=1):
    """Every element of `got` against its budget; NaN or inf in `got` counts as infinitely far off."""
    got, ref, M = torch.as_tensor(got).double(), torch.as_tensor(ref).double(), torch.as_tensor(M).double()
    assert got.shape == ref.shape == M.shape, (name, got.shape, ref.shape, M.shape)
    if got.numel() == 0:
        return Report(name, 0.0, (), float("inf"), 0)
    b = budget(ref, M, c, out_dtype) if not torch.is_tensor(c) else budget(ref, M, c.double(), out_dtype)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where((err == 0) & (b == 0), torch.zeros_like(err), err / b.clamp_min(1e-300))
    flat = int(ratio.argmax())
    where, rest = [], flat
    for n in reversed(ratio.shape):
        where.insert(0, rest % n)
        rest //= n
    power = ((M / n_terms) / b.clamp_min(1e-300))[M > 0]
    margin = float(power.median()) if power.numel() else float("inf")
    return Report(name, float(ratio.reshape(-1)[flat]), tuple(where), margin, ratio.numel())


def _ratio(r32, r64, M):
    err = (r32.double() - r64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / (EPS32 * M.double()).clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def measure(runs=None, dtypes=("f32", "bf16", "f16"), standalone=True, log=print):
    """The largest |r32 - r64| / (2^-24 M) of the fp32 CPU statement per result class (the keys of MEASURED), and of torch's fp32 BCE
    formula under "acc_bce_torch"."""
    worst = {k: 0.0 for k in MEASURED}
    worst["acc_bce_torch"] = worst["bce_torch"] = 0.0

    def up(k, v):
        worst[k] = max(worst[k], v)
    for run in (RUNS if runs is None else runs):
        for dn in dtypes:
            case = make_case(run[0], run[1], DTYPES[dn])
            asg = assignment(case)
            r64 = statement(case, asg)
            r32 = statement(case, asg, torch.float32)
            rt = statement(case, asg, torch.float32, bce=bce_torch)
            line = {}
            for k, name in (("pred", "decode"), ("norm", "norm"), ("y", "y"), ("bce", "bce")):
                line[name] = _ratio(r32[k][0], r64[k][0], r64[k][1])
            line["bce_torch"] = _ratio(rt["bce"][0], r64["bce"][0], r64["bce"][1])
            for i, name in enumerate(ACC_KEYS):
                line[name] = _ratio(r32["acc"][0][i], r64["acc"][0][i], r64["acc"][1][i])
            line["acc_bce_torch"] = _ratio(rt["acc"][0][1], r64["acc"][0][1], r64["acc"][1][1])
            g32, (g64, m64) = r32["grad"][0], r64["grad"]
            line["grad_dist"] = _ratio(g32[..., :4 * REG], g64[..., :4 * REG], m64[..., :4 * REG])
            line["grad_cls"] = _ratio(g32[..., 4 * REG:], g64[..., 4 * REG:], m64[..., 4 * REG:])
            for k, v in line.items():
                up(k, v)
            log(run_id(run), dn, " ".join(f"{k} {v:.3g}" for k, v in line.items()))
    if standalone:
        for xywh in (0, 1):
            b1, b2 = iou_inputs(xywh)
            for kind in range(4):
                v64, m64, g64, mg64 = iou_ref(b1, b2, xywh, kind)
                v32, _, g32, _ = iou_ref(b1, b2, xywh, kind, torch.float32)
                up(iou_key(xywh, kind), _ratio(v32, v64, m64))
                up(iou_key(xywh, kind) + "_grad", _ratio(g32, g64, mg64))
        _, _, ds, ts = standalone_inputs()
        v64, m64, g64, mg64 = dfl_ref(ds, ts)
        v32, _, g32, _ = dfl_ref(ds, ts, torch.float32)
        up("dfl", _ratio(v32, v64, m64))
        up("dfl_grad", _ratio(g32, g64, mg64))
    return worst


if __name__ == "__main__":
    w = measure()
    for k_, v_ in w.items():
        print(f"    {k_:<22s} {v_:10.3f} {'' if k_.endswith('_torch') else f'{8 * v_:12.3f}'}")
