"""Float64 statement of the segment and pose kernels (csrc/seg.hip, csrc/pose.hip) with element-wise error budgets, and the case list
that the CPU and GPU tests share.  Plain torch on the CPU; nothing here calls a dedark_yolo_amd kernel.

The statement works on a FROZEN assignment that the case list writes by hand (fg_mask, target_gt_idx, target_box): no assigner runs,
which is what makes 129 positives in one image, a target_gt_idx past n_max or a gt row of -1 reachable.  The discrete parts are decided
by the reference's own f32 expressions on the CPU: crop membership `r >= x1 & r < x2` on xyxy / imgsz * (mw, mh) in f32 (crop_mask),
the nearest source index of F.interpolate(mode="nearest") on f32 planes, the gt value and the visibility `!= 0`.  Everything
continuous is float64 on inputs rounded to the compute dtype.  Each result comes with the magnitude sum M of its terms (the same
expression on absolute values), and the budget of element i is tests/detloss_ref.py's (`budget`, `compare`, `Report` are imported):

    |got_i - ref_i| <= u_out * |ref_i| + (1 + u_out) * c * 2^-24 * M_i          (+ 2^-25 for f16 outputs)

u_out: unit roundoff of the compute dtype for d mc, d proto, d kpt and the dy_bias_add output, 0 for the f32 results.

M, with z = c_p . P[pix], Z = sum_k |c_pk P_k| and t the gt value:
    BCE element          Z + Z t + log1p(exp(-|z|))                 (max(z, 0) and z t on absolute values)
    l_p, means, items    the sums of the BCE elements' M with the same positive factors
    d mc, d proto        sum of (sigma + t + sigma (1 - sigma) Z) w |P_k| (|c_k|): the last term carries the rounding of z itself into
                         the sigmoid, which is what is left of the element once sigma or 1 - sigma is tiny (`wide` law)
    pose, per keypoint   E = e + (|dx| (|px| + |gx|) + |dy| (|py| + |gy|)) / (2 sigma)^2 / (area + 1e-9) + e R is the first-order error
                         magnitude of the exponent e: the differences px - gx cancel, and so do the box sides behind the area
                         (R = (|x2| + |x1|) / |x2 - x1| + (|y2| + |y1|) / |y2 - y1|); 1 - exp(-e) has M = 1 + exp(-e) (1 + E)
    d kpt (x, y)         W exp(-e) ((|p| + |g|) + |d| E), W the positive factors; visibility: g hyp_kobj (sigma + vis) / (n K)
    decoded keypoints    (2 |raw| + (anchor - 0.5)) stride; sigma(raw) for the visibility rows
    OKS                  sum exp(-e) (1 + E) vis / (cnt + eps), E without the area part (the area is an input)
    db                   sum |dy|;  x + bias: |x| + |bias|.  The fp32 statement of db adds the pixels from left to right: the entry promises
                         a fixed pixel order, and against torch.sum's cascade (measured 0.202, c = 1.6) a correct kernel that adds
                         2048 chunk sums in order reached 1.71 of the budget (C = 257, pixels = 2048, f32)
An f32 factor below the normal range (exp(-e) for e > 87, sigma(z) for z < -87) may come out as 0: in the M of d mc, d proto, d kpt and
OKS such a factor counts as itself + 2^-102, so that the budget never falls below c * 2^-126 times the other factors.

c is one constant per result class and is NOT tuned on the kernels: 8 times the largest |r32 - r64| / (2^-24 M) that the SAME
statement reaches in fp32 on the CPU over the case list x {unit, wide} x {f32, bf16, f16}; `python tests/segpose_ref.py` re-measures
and prints this table.  The fp32 BCE is max(x, 0) - x t + log1p(exp(-|x|)), for the reason tests/detloss_ref.py gives.  The factor 8
is the margin for another summation order and the device's expf / log1pf.

    result class        measured   c = 8 x
    seg_lossp                 1.9       15.200
    seg_means               0.187        1.496
    seg_out                 0.184        1.472
    seg_dmc                     2       16.000
    seg_dproto               4.77       38.160
    pose_work                2.03       16.240
    pose_img                 2.51       20.080
    pose_out                 1.33       10.640
    pose_dkpt                2.47       19.760
    pose_y                   1.98       15.840
    oks                     0.651        5.208
    bias_add                    1        8.000
    bias_db                  2.76       22.080
"""
import os
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from detloss_ref import DTYPES, EPS32, Report, _ratio, budget, compare          # noqa: E402,F401  (the budget is detloss_ref's, re-exported)

NM = 32
HYP_BOX = 7.5
HYP_POSE, HYP_KOBJ = 12.0, 1.0
DET_OUT = (3.25, 1.5, 0.75, 0.5)              # stands for dy_loss_finish's (total, box, cls, dfl)
OKS_SIGMA = torch.tensor([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89], dtype=torch.float64) / 10.0
LAWS = ("unit", "wide")
TINY = 2.0 ** -102                             # 2^-126 / 2^-24: what stands for an f32 value that may be flushed to zero

# largest |r32 - r64| / (2^-24 M) over the runs x dtypes (measure() below); C = 8 x
MEASURED = {
    "seg_lossp": 1.9, "seg_means": 0.187, "seg_out": 0.184, "seg_dmc": 2.0, "seg_dproto": 4.77,
    "pose_work": 2.03, "pose_img": 2.51, "pose_out": 1.33, "pose_dkpt": 2.47, "pose_y": 1.98,
    "oks": 0.651, "bias_add": 1.0, "bias_db": 2.76,
}
C = {k: 8.0 * v for k, v in MEASURED.items()}


# ---- segment cases -------------------------------------------------------------------------------------------------------------
# gts: (image, x1, y1, x2, y2) in pixels in batch order (batch_idx unsorted on purpose); gt k of an image is its k-th row.
# pos: (image, anchor, target_gt_idx[, explicit target box]); without a box the positive takes its gt's.
def _spread(n, A, seed):
    g = torch.Generator().manual_seed(seed)
    return sorted(torch.randperm(A, generator=g)[:n].tolist())


_CHUNK_GTS = [(1, 10.0, 6.0, 70.0, 80.0), (0, 8.0, 12.0, 76.0, 90.0), (0, 20.0, 4.0, 92.0, 70.0), (1, 30.0, 22.0, 90.0, 94.0)]
_EDGE_GTS = [(0, 12.0, 28.0, 24.0, 56.0),          # x 12 -> 4 (exact 3), y 28 -> 8 (7), y 56 -> 15 (14)
             (0, 44.0, 10.0, 48.0, 90.0),          # x 44 and 48
             (0, 13.0, 30.0, 15.0, 70.0),          # empty: 3.25 .. 3.75 holds no column
             (0, 11.0, 11.0, 13.0, 13.0),          # one pixel: column 3, row 3
             (1, -10.0, -20.0, 100.0, 130.0),      # reaches outside: the whole map
             (1, 32.0, 52.0, 64.0, 104.0),         # exact integers the usual way: columns 8 .. 15, rows 13 .. 25
             (1, 20.0, 20.0, 60.0, 80.0)]
SEG_CASES = {
    # 16 x 16 proto: HW = 256, exactly one block of the proto-gradient kernel
    "sq": dict(B=2, A=84, proto=(16, 16), img=(64, 64), mask=(16, 16), overlap=True, mdt=torch.uint8,
               gts=[(1, 4.0, 6.0, 40.0, 50.0), (0, 10.0, 10.0, 50.0, 40.0), (0, 30.0, 20.0, 62.0, 60.0), (1, 20.0, 30.0, 60.0, 62.0),
                    (0, 2.0, 40.0, 30.0, 63.0)],
               pos=[(0, 3, 0), (0, 17, 1), (0, 40, 0), (0, 70, 2), (0, 83, 1), (1, 0, 0), (1, 41, 1), (1, 42, 1)], npos=[5, 3]),
    # 24 x 24 proto: HW = 576, three blocks, the last partial; 129 = two full chunks of 64 plus one, 64 = exactly one chunk;
    # n_max = 2 -> grid 20 -> the slot loop of the forward / d mc kernels takes 7 trips
    "chunks": dict(B=2, A=300, proto=(24, 24), img=(96, 96), mask=(12, 12), overlap=False, mdt=torch.uint8, gts=_CHUNK_GTS,
                   pos=[(0, a, i % 2) for i, a in enumerate(_spread(129, 300, 1))] + [(1, a, (i // 3) % 2) for i, a in enumerate(_spread(64, 300, 2))],
                   npos=[129, 64]),
    "edges": dict(B=2, A=60, proto=(26, 21), img=(104, 84), mask=(26, 21), overlap=True, mdt=torch.int32, gts=_EDGE_GTS, big_id=(1, 300),
                  pos=[(0, 1, 0), (0, 7, 1), (0, 8, 2), (0, 30, 3), (0, 59, 0), (1, 0, 0), (1, 13, 1), (1, 14, 2), (1, 40, 299, (8.0, 8.0, 70.0, 90.0))],
                  npos=[5, 4]),
    # 62 -> 14 rows, 84 -> 20 columns: ATen's floor(f32(o) * f32(in / out)) gives row 30 at o = 7 and column 62 at o = 15 where integer
    # arithmetic gives 31 and 63; the gt of label 0 starts at row 31 / column 63, so the two disagree on a whole row and column
    "nearest_ov": dict(B=1, A=40, proto=(14, 20), img=(56, 80), mask=(62, 84), overlap=True, mdt=torch.uint8,
                       gts=[(0, 4.0, 4.0, 76.0, 52.0), (0, 10.0, 8.0, 40.0, 30.0)], paint=[(31, 50, 63, 80), (5, 20, 10, 40)],
                       pos=[(0, 2, 0), (0, 11, 1), (0, 39, 0)], npos=[3]),
    "nearest_pl": dict(B=1, A=40, proto=(14, 20), img=(56, 80), mask=(62, 84), overlap=False, mdt=torch.uint8,
                       gts=[(0, 4.0, 4.0, 76.0, 52.0), (0, 10.0, 8.0, 40.0, 30.0)], paint=[(31, 50, 63, 80), (5, 20, 10, 40)],
                       pos=[(0, 2, 0), (0, 11, 1), (0, 39, 0)], npos=[3]),
    # image 1 without positives; image 2: a positive whose gt row is -1 (target_gt_idx 1 of an image with one label) and one with
    # target_gt_idx >= n_max; unsorted batch_idx
    "holes": dict(B=3, A=50, proto=(9, 7), img=(36, 28), mask=(9, 7), overlap=False, mdt=torch.uint8,
                  gts=[(2, 2.0, 3.0, 20.0, 30.0), (0, 5.0, 5.0, 25.0, 33.0), (0, 1.0, 10.0, 14.0, 20.0)],
                  pos=[(0, 4, 0), (0, 5, 1), (0, 49, 1), (2, 0, 0), (2, 20, 1, (4.0, 4.0, 24.0, 30.0)), (2, 33, 5, (3.0, 8.0, 27.0, 35.0))],
                  npos=[3, 0, 3]),
    "nopos_ov": dict(B=2, A=30, proto=(9, 7), img=(36, 28), mask=(9, 7), overlap=True, mdt=torch.uint8, gts=[(0, 2.0, 3.0, 20.0, 30.0)], pos=[],
                     npos=[0, 0]),
    "nopos_pl": dict(B=2, A=30, proto=(9, 7), img=(36, 28), mask=(9, 7), overlap=False, mdt=torch.uint8, gts=[], pos=[], npos=[0, 0]),
}
SEG_RUNS = [(c, l) for c in SEG_CASES for l in LAWS if not (c.startswith("nopos") and l == "wide")]


def run_id(r):
    return f"{r[0]}:{r[1]}"


def gt_rows_ref(batch_idx, B, n_max):
    """dy_seg_gt_rows: rows[b][j] = index of the j-th row with batch_idx == b (the first n_max kept), -1 past the image's count."""
    rows = torch.full((B, n_max), -1, dtype=torch.int64)
    cnt = [0] * B
    for t, v in enumerate(batch_idx.tolist()):
        b = int(v)                                       # truncates toward zero, as the kernel's cast does
        if 0 <= b < B and cnt[b] < n_max:
            rows[b, cnt[b]] = t
            cnt[b] += 1
    return rows


def make_seg_case(cid, law, dtype):
    """The inputs of one segment run: mc [B, A, 32] and proto [B, mh, mw, 32] f32 holding values of `dtype`, the frozen assignment,
    the gt masks (index map [B, h, w] or planes [N, h, w], painted off the boxes so that pixels inside a crop are 0 as well)."""
    s = SEG_CASES[cid]
    B, A, (mh, mw), (H, W), (kh, kw) = s["B"], s["A"], s["proto"], s["img"], s["mask"]
    g = torch.Generator().manual_seed(100 * list(SEG_CASES).index(cid) + LAWS.index(law) + 3)
    mc = torch.randn(B, A, NM, generator=g) * (3.0 if law == "wide" else 1.0)
    proto = torch.randn(B, mh, mw, NM, generator=g)
    if s["pos"]:                                   # one positive predicts nothing: z = 0 everywhere, sigmoid exactly 0.5
        b0, a0 = s["pos"][-1][:2]
        mc[b0, a0] = 0.0
    gts = s["gts"]
    bidx = torch.tensor([float(t[0]) for t in gts])
    per = [[t[1:] for t in gts if t[0] == b] for b in range(B)]
    n_max = max(1, max(len(p) for p in per))
    planes = torch.zeros(max(len(gts), 1), kh, kw, dtype=torch.int64)
    index = torch.zeros(B, kh, kw, dtype=torch.int64)
    seen = [0] * B
    for t, (b, x1, y1, x2, y2) in enumerate(gts):
        if "paint" in s:
            r0, r1, c0, c1 = s["paint"][t]
        else:                                      # not the box: shifted down and cut on the right
            r0, r1 = int(round((y1 + 0.2 * (y2 - y1)) / H * kh)), int(round(y2 / H * kh))
            c0, c1 = int(round(x1 / W * kw)), int(round((x2 - 0.3 * (x2 - x1)) / W * kw))
        r0, r1, c0, c1 = max(r0, 0), max(r1, 0), max(c0, 0), max(c1, 0)
        planes[t, r0:r1, c0:c1] = 1
        seen[b] += 1
        index[b][planes[t].bool()] = seen[b]
    if "big_id" in s:                              # a label id past 255: needs the int32 map
        b, v = s["big_id"]
        index[b, 2:kh - 3, 1:kw // 2] = v
    fg = torch.zeros(B, A, dtype=torch.bool)
    gi = torch.zeros(B, A, dtype=torch.int64)
    tbox = torch.zeros(B, A, 4)
    for p in s["pos"]:
        b, a, k = p[:3]
        fg[b, a], gi[b, a] = True, k
        tbox[b, a] = torch.tensor(p[3] if len(p) > 3 else per[b][k])
    masks = (index if s["overlap"] else planes).to(s["mdt"])
    return SimpleNamespace(id=cid, law=law, dtype=dtype, B=B, A=A, mh=mh, mw=mw, img_h=float(H), img_w=float(W), mask_h=kh, mask_w=kw,
                           mc=mc.to(dtype).float(), proto=proto.to(dtype).float(), fg=fg, gi=gi, tbox=tbox, masks=masks,
                           overlap=s["overlap"], batch_idx=bidx, n_max=n_max, rows=gt_rows_ref(bidx, B, n_max), spec=s)


def nearest_index(o, n_in, n_out, integer=False):
    """Source index of F.interpolate(mode='nearest') for output indices o (ATen: floor(f32(o) * f32(in / out)) clamped); integer:
    the o * in // out that it is not."""
    if integer:
        return (o * n_in // n_out).clamp(max=n_in - 1)
    sc = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
    return (o.float() * sc).floor().long().clamp(max=n_in - 1)


def crop_edges(case, b, idx, mode="ref"):
    """The scaled box [n, 4] (x1, y1, x2, y2) in proto pixels, f32.  ref: xyxy / imgsz * (mw, mh) in this order; reassoc: xyxy * ((mw,
    mh) / imgsz), which differs at some edges."""
    img = torch.tensor([case.img_w, case.img_h, case.img_w, case.img_h], dtype=torch.float32)
    m = torch.tensor([case.mw, case.mh, case.mw, case.mh], dtype=torch.float32)
    t = case.tbox[b][idx].float()
    return t * (m / img) if mode == "reassoc" else t / img * m


def seg_discrete(case, b, idx, crop="ref", nearest="aten", swap=False):
    """(crop [n, mh, mw] bool, gt [n, mh, mw] f32) of the positives idx of image b, by the reference's own f32 expressions."""
    mh, mw = case.mh, case.mw
    e = crop_edges(case, b, idx, crop)
    if crop == "floor":
        e = e.floor()
    x1, y1, x2, y2 = [e[:, j].view(-1, 1, 1) for j in range(4)]
    r = torch.arange(mw, dtype=torch.float32).view(1, 1, -1)
    c = torch.arange(mh, dtype=torch.float32).view(1, -1, 1)
    cr = (r >= x1) & (r < x2) & (c >= y1) & (c < y2)
    m = case.masks.float()
    if (case.mask_h, case.mask_w) != (mh, mw):
        if nearest == "aten":
            m = F.interpolate(m[None], (mh, mw), mode="nearest")[0]
        else:
            sy = nearest_index(torch.arange(mh), case.mask_h, mh, True)
            sx = nearest_index(torch.arange(mw), case.mask_w, mw, True)
            m = m[:, sy][:, :, sx]
    if swap:                                                   # the lookup at (x, y) instead of (y, x)
        yy = torch.arange(mh).view(-1, 1).expand(mh, mw)
        xx = torch.arange(mw).view(1, -1).expand(mh, mw)
        m = m[:, xx.clamp(max=mh - 1), yy.clamp(max=mw - 1)]
    g = case.gi[b][idx]
    if case.overlap:
        gt = (m[b][None] == (g + 1).view(-1, 1, 1).float()).float()
    else:
        row = torch.where((g >= 0) & (g < case.n_max), case.rows[b][g.clamp(0, case.n_max - 1)], torch.full_like(g, -1))
        gt = torch.where((row >= 0).view(-1, 1, 1), m[row.clamp(min=0)], torch.zeros(()))
    return cr, gt


def bce_log1p(x, t):
    return x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))


def seg_statement(case, dt=torch.float64, hyp_box=HYP_BOX, grad_out=1.0, det=DET_OUT, crop="ref", nearest="aten", swap=False, drop=None,
                  use_area=True, mean=True):
    """{name: (value, M)}: lossp [B, A] (slot order, zero past npos), means [B], out [5], dmc [B, A, 32] (zero off the positives),
    dproto [B, mh, mw, 32]; npos.  The trailing arguments are the CPU test's wrong variants."""
    B, A, mh, mw = case.B, case.A, case.mh, case.mw
    z0 = lambda *s: torch.zeros(*s, dtype=dt)                                           # noqa: E731
    lossp, m_lossp, means, m_means = z0(B, A), z0(B, A), z0(B), z0(B)
    dmc, m_dmc, dpr, m_dpr = z0(B, A, NM), z0(B, A, NM), z0(B, mh, mw, NM), z0(B, mh, mw, NM)
    npos = []
    for b in range(B):
        idx = case.fg[b].nonzero().squeeze(1)
        n = idx.numel()
        npos.append(n)
        if n == 0:
            continue
        cr, gt = seg_discrete(case, b, idx, crop, nearest, swap)
        cr, t = cr.to(dt), gt.to(dt)
        c, P = case.mc[b, idx].to(dt), case.proto[b].to(dt)
        z = torch.einsum("nk,hwk->nhw", c, P)
        Z = torch.einsum("nk,hwk->nhw", c.abs(), P.abs())
        sp = torch.log1p(torch.exp(-z.abs()))
        tb = case.tbox[b][idx].to(dt)
        area = ((tb[:, 2] / case.img_w - tb[:, 0] / case.img_w) * (tb[:, 3] / case.img_h - tb[:, 1] / case.img_h)) if use_area else torch.ones(n, dtype=dt)
        lp = ((z.clamp(min=0) - z * t + sp) * cr).sum((1, 2)) / (mh * mw) / area
        mlp = ((Z + Z * t + sp) * cr).sum((1, 2)) / (mh * mw) / area
        lossp[b, :n], m_lossp[b, :n] = lp, mlp
        means[b], m_means[b] = (lp.sum() / n, mlp.sum() / n) if mean else (lp.sum(), mlp.sum())
        w = (abs(grad_out) * hyp_box / (n if mean else 1) / (mh * mw) / area).view(-1, 1, 1)
        sg = torch.sigmoid(z)
        dz = (sg - t) * cr * w * (1.0 if grad_out >= 0 else -1.0)
        mdz = (sg + TINY + t + sg * (1 - sg) * Z) * cr * w
        dmc[b, idx], m_dmc[b, idx] = torch.einsum("nhw,hwk->nk", dz, P), torch.einsum("nhw,hwk->nk", mdz, P.abs())
        if drop is not None and drop < n:
            dz = dz.clone()
            dz[drop] = 0
        dpr[b], m_dpr[b] = torch.einsum("nhw,nk->hwk", dz, c), torch.einsum("nhw,nk->hwk", mdz, c.abs())
    d = torch.tensor(det, dtype=dt)
    item, m_item = means.sum() * (hyp_box / B), m_means.sum() * (hyp_box / B)
    out = torch.stack((d[0] + item * B, d[1], item, d[2], d[3]))
    m_out = torch.stack((d[0].abs() + m_item * B, d[1].abs(), m_item, d[2].abs(), d[3].abs()))
    return dict(lossp=(lossp, m_lossp), means=(means, m_means), out=(out, m_out), dmc=(dmc, m_dmc), dproto=(dpr, m_dpr), npos=npos)


SEG_KEYS = ("lossp", "means", "out", "dmc", "dproto")


# ---- pose cases ----------------------------------------------------------------------------------------------------------------
# levels: (h, w, stride); gts: (image, x1, y1, x2, y2); pos: (image, anchor, target_gt_idx[, box]); vis: how the visibility column of
# the gt keypoints is drawn
_RECT2 = [(6, 10, 8.0), (3, 5, 16.0)]
POSE_CASES = {
    "rect2": dict(levels=_RECT2, ks=(17, 3), B=2, gts=[(1, 4.0, 2.0, 70.0, 44.0), (0, 10.0, 6.0, 60.0, 40.0), (0, 30.0, 10.0, 78.0, 46.0)],
                  pos=[(0, 3, 0), (0, 14, 1), (0, 37, 0), (0, 61, 1), (0, 74, 0), (1, 0, 0), (1, 25, 0), (1, 66, 0)], vis="mixed"),
    "one": dict(levels=[(5, 7, 32.0)], ks=(5, 2), B=2, gts=[(0, 20.0, 10.0, 200.0, 150.0), (1, 40.0, 30.0, 180.0, 120.0)],
                pos=[(0, 0, 0), (0, 17, 0), (0, 34, 0), (1, 9, 0), (1, 10, 0)], vis="mixed"),
    "four": dict(levels=[(8, 6, 4.0), (4, 3, 8.0), (2, 2, 16.0), (1, 1, 32.0)], ks=(1, 3), B=2,
                 gts=[(0, 2.0, 3.0, 22.0, 30.0), (1, 1.0, 1.0, 23.0, 31.0), (0, 6.0, 8.0, 20.0, 20.0)],
                 pos=[(0, 5, 0), (0, 47, 1), (0, 50, 0), (0, 62, 1), (0, 64, 0), (1, 13, 0), (1, 60, 0), (1, 63, 0)], vis="mixed"),
    # 300 positives: the second block of pose_pos_kernel (slots 256 ..) and the strided loop of pose_image_kernel
    "many": dict(levels=[(16, 20, 8.0), (8, 10, 16.0)], ks=(17, 3), B=2,
                 gts=[(0, 4.0, 4.0, 156.0, 124.0), (1, 20.0, 10.0, 140.0, 110.0), (0, 10.0, 20.0, 150.0, 100.0)],
                 pos=[(0, a, i % 2) for i, a in enumerate(_spread(300, 400, 5))] + [(1, 399, 0)], vis="mixed"),
    "invisible": dict(levels=_RECT2, ks=(17, 3), B=2, gts=[(0, 10.0, 6.0, 60.0, 40.0), (1, 4.0, 2.0, 70.0, 44.0)],
                      pos=[(0, 3, 0), (0, 14, 0), (0, 70, 0), (1, 0, 0), (1, 25, 0)], vis="image0_none"),
    # a positive whose gt row is missing (target_gt_idx 1 in an image with one label), image 1 without positives, a box of half a
    # pixel, visibility logits of +-30
    "holes": dict(levels=_RECT2, ks=(17, 3), B=3, gts=[(2, 4.0, 2.0, 70.0, 44.0), (0, 10.0, 6.0, 60.0, 40.0), (0, 33.0, 21.0, 33.5, 21.5)],
                  pos=[(0, 3, 0), (0, 34, 1), (0, 61, 0), (2, 0, 0), (2, 25, 1, (8.0, 8.0, 40.0, 40.0)), (2, 66, 0)], vis="mixed", logit30=True),
    "nopos": dict(levels=_RECT2, ks=(17, 3), B=2, gts=[(0, 10.0, 6.0, 60.0, 40.0)], pos=[], vis="mixed"),
}
POSE_RUNS = [(c, l) for c in POSE_CASES for l in LAWS if not (c == "nopos" and l == "wide")]


def sigmas_of(ks):
    return OKS_SIGMA.clone() if tuple(ks) == (17, 3) else torch.full((ks[0],), 1.0 / ks[0], dtype=torch.float64)


def anchor_table(levels):
    """Per anchor (numbered level by level): x index, y index, stride, level."""
    xs, ys, st, lv = [], [], [], []
    for i, (h, w, s) in enumerate(levels):
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        xs.append(xx.reshape(-1)), ys.append(yy.reshape(-1)), st.append(torch.full((h * w,), s)), lv.append(torch.full((h * w,), i))
    return torch.cat(xs).float(), torch.cat(ys).float(), torch.cat(st), torch.cat(lv)


def make_pose_case(cid, law, dtype):
    """The inputs of one pose run: kpt [B, A, K * ndim] f32 holding values of `dtype`, the frozen assignment, gt keypoints [N, K, 3]
    (normalised x, y; visibility 0, 1, 2 and, in `mixed`, one negative value)."""
    s = POSE_CASES[cid]
    levels, (K, nd), B = s["levels"], s["ks"], s["B"]
    A = sum(h * w for h, w, _ in levels)
    H, W = levels[0][0] * levels[0][2], levels[0][1] * levels[0][2]
    ax, ay, st, _ = anchor_table(levels)
    g = torch.Generator().manual_seed(100 * list(POSE_CASES).index(cid) + LAWS.index(law) + 11)
    sc = 3.0 if law == "wide" else 1.0
    kpt = torch.randn(B, A, K, nd, generator=g) * sc
    if s.get("logit30") and nd == 3:
        kpt[..., 2] = torch.where(torch.rand(B, A, K, generator=g) < 0.3, torch.sign(kpt[..., 2]) * 30.0, kpt[..., 2])
    kpt = kpt.view(B, A, K * nd).to(dtype).float()
    gts = s["gts"]
    bidx = torch.tensor([float(t[0]) for t in gts])
    per = [[t[1:] for t in gts if t[0] == b] for b in range(B)]
    rows_of = [[t for t, q in enumerate(gts) if q[0] == b] for b in range(B)]
    n_max = max(1, max(len(p) for p in per))
    fg = torch.zeros(B, A, dtype=torch.bool)
    gi = torch.zeros(B, A, dtype=torch.int64)
    tbox = torch.zeros(B, A, 4)
    kp = torch.rand(max(len(gts), 1), K, 3, generator=g)
    done = set()
    for p in s["pos"]:
        b, a, k = p[:3]
        fg[b, a], gi[b, a] = True, k
        tbox[b, a] = torch.tensor(p[3] if len(p) > 3 else per[b][k])
        if k < len(per[b]) and (b, k) not in done:          # the gt keypoints sit near this positive's prediction
            done.add((b, k))
            r = kpt[b, a].view(K, nd)
            noise = torch.randn(K, 2, generator=g) * (0.4 * sc)
            kp[rows_of[b][k], :, 0] = ((r[:, 0] * 2 + ax[a] + noise[:, 0]) * st[a]) / W
            kp[rows_of[b][k], :, 1] = ((r[:, 1] * 2 + ay[a] + noise[:, 1]) * st[a]) / H
    vis = torch.randint(0, 3, (kp.shape[0], K), generator=g).float()
    if s["vis"] == "image0_none":
        for t, q in enumerate(gts):
            if q[0] == 0:
                vis[t] = 0.0
    elif len(gts):
        vis[0, 0], vis[-1, K - 1] = -1.0, 2.0               # a negative visibility counts as visible (vis != 0)
    kp[..., 2] = vis
    return SimpleNamespace(id=cid, law=law, dtype=dtype, levels=levels, K=K, ndim=nd, B=B, A=A, img_h=float(H), img_w=float(W), kpt=kpt, fg=fg,
                           gi=gi, tbox=tbox, keypoints=kp if len(gts) else kp[:0], batch_idx=bidx, n_max=n_max, rows=gt_rows_ref(bidx, B, n_max),
                           sigma=sigmas_of((K, nd)), spec=s)


def pose_level_maps(case):
    """kpt split into the per-level maps [B, h, w, K * ndim] (NHWC)."""
    out, a0 = [], 0
    for h, w, _ in case.levels:
        out.append(case.kpt[:, a0:a0 + h * w].view(case.B, h, w, -1))
        a0 += h * w
    return out


def pose_statement(case, dt=torch.float64, hyp=(HYP_POSE, HYP_KOBJ), grad_out=1.0, det=DET_OUT, factor=True, kobj_div_k=True, vis_ne=True):
    """{name: (value, M)}: work [3, B, A] (slot order), img [3, B], out [6], dkpt [B, A, K * ndim], y [B, K * ndim, A] (decoded rows);
    npos.  The trailing arguments are the CPU test's wrong variants."""
    B, A, K, nd = case.B, case.A, case.K, case.ndim
    hp, hk = hyp
    z0 = lambda *s: torch.zeros(*s, dtype=dt)                                           # noqa: E731
    ax, ay, st, _ = (t.to(dt) for t in anchor_table(case.levels))
    sig2 = (2.0 * case.sigma.to(dt)) ** 2
    raw = case.kpt.to(dt).view(B, A, K, nd)
    work, m_work, img, m_img = z0(3, B, A), z0(3, B, A), z0(3, B), z0(3, B)
    dk, m_dk = z0(B, A, K, nd), z0(B, A, K, nd)
    npos = []
    sgn = 1.0 if grad_out >= 0 else -1.0
    for b in range(B):
        idx = case.fg[b].nonzero().squeeze(1)
        n = idx.numel()
        npos.append(n)
        if n == 0:
            continue
        g = case.gi[b][idx]
        row = torch.where((g >= 0) & (g < case.n_max), case.rows[b][g.clamp(0, case.n_max - 1)], torch.full_like(g, -1))
        have = (row >= 0).view(-1, 1)
        gk = case.keypoints[row.clamp(min=0)] if case.keypoints.shape[0] else torch.zeros(n, K, 3)
        v32 = gk[..., 2]
        vis = (((v32 != 0) if vis_ne else (v32 > 0)) & have).to(dt)
        s = st[idx].view(-1, 1)
        gx = torch.where(have, gk[..., 0].to(dt) * case.img_w / s, z0(1))
        gy = torch.where(have, gk[..., 1].to(dt) * case.img_h / s, z0(1))
        r = raw[b, idx]
        px, py = r[..., 0] * 2 + ((ax[idx] + 0.5) - 0.5).view(-1, 1), r[..., 1] * 2 + ((ay[idx] + 0.5) - 0.5).view(-1, 1)
        apx, apy = r[..., 0].abs() * 2 + ax[idx].view(-1, 1), r[..., 1].abs() * 2 + ay[idx].view(-1, 1)
        tb = case.tbox[b][idx].to(dt) / s
        area = ((tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])).view(-1, 1)
        R = ((tb[:, 2].abs() + tb[:, 0].abs()) / (tb[:, 2] - tb[:, 0]).abs() + (tb[:, 3].abs() + tb[:, 1].abs()) / (tb[:, 3] - tb[:, 1]).abs()).view(-1, 1)
        dx, dy = px - gx, py - gy
        e = (dx * dx + dy * dy) / sig2 / (area + 1e-9) / 2
        E = e + (dx.abs() * (apx + gx.abs()) + dy.abs() * (apy + gy.abs())) / sig2 / (area + 1e-9) + e * R
        ex = torch.exp(-e)
        work[0, b, :n], m_work[0, b, :n] = ((1 - ex) * vis).sum(1), ((1 + ex * (1 + E)) * vis).sum(1)
        work[1, b, :n] = m_work[1, b, :n] = vis.sum(1)
        if nd == 3:
            x = r[..., 2]
            work[2, b, :n] = bce_log1p(x, vis).sum(1)
            m_work[2, b, :n] = (x.clamp(min=0) + (x * vis).abs() + torch.log1p(torch.exp(-x.abs()))).sum(1)
        nk, nnz = float(n * K), vis.sum()
        fac = nk / (nnz + 1e-9) if factor else 1.0
        img[0, b], m_img[0, b] = fac * (work[0, b, :n].sum() / nk), fac * (m_work[0, b, :n].sum() / nk)
        kd = nk if kobj_div_k else float(n)
        img[1, b], m_img[1, b] = work[2, b, :n].sum() / kd, m_work[2, b, :n].sum() / kd
        img[2, b] = m_img[2, b] = nnz
        wg1 = abs(grad_out) * hp * vis / (nnz + 1e-9) * 2.0 * 2.0 / sig2 / (area + 1e-9) / 2.0
        wgt, wgm = wg1 * ex, wg1 * (ex + TINY)
        dk[b, idx, :, 0], dk[b, idx, :, 1] = sgn * wgt * dx, sgn * wgt * dy
        m_dk[b, idx, :, 0], m_dk[b, idx, :, 1] = wgm * ((apx + gx.abs()) + dx.abs() * E), wgm * ((apy + gy.abs()) + dy.abs() * E)
        if nd == 3:
            sg = torch.sigmoid(r[..., 2])
            dk[b, idx, :, 2], m_dk[b, idx, :, 2] = sgn * abs(grad_out) * hk * (sg - vis) / nk, abs(grad_out) * hk * (sg + vis) / nk
    d = torch.tensor(det, dtype=dt)
    pose, kobj = img[0].sum() * (hp / B), img[1].sum() * (hk / B)
    m_pose, m_kobj = m_img[0].sum() * (hp / B), m_img[1].sum() * (hk / B)
    out = torch.stack((d[0] + (pose + kobj) * B, d[1], pose, kobj, d[2], d[3]))
    m_out = torch.stack((d[0].abs() + (m_pose + m_kobj) * B, d[1].abs(), m_pose, m_kobj, d[2].abs(), d[3].abs()))
    s_all = st.view(1, A, 1)
    y, m_y = z0(B, A, K, nd), z0(B, A, K, nd)
    y[..., 0], y[..., 1] = (raw[..., 0] * 2 + ((ax + 0.5) - 0.5).view(1, A, 1)) * s_all, (raw[..., 1] * 2 + ((ay + 0.5) - 0.5).view(1, A, 1)) * s_all
    m_y[..., 0], m_y[..., 1] = (raw[..., 0].abs() * 2 + ax.view(1, A, 1)) * s_all, (raw[..., 1].abs() * 2 + ay.view(1, A, 1)) * s_all
    if nd == 3:
        y[..., 2] = m_y[..., 2] = torch.sigmoid(raw[..., 2])
    perm = lambda t: t.view(B, A, K * nd).permute(0, 2, 1).contiguous()                 # noqa: E731
    return dict(work=(work, m_work), img=(img, m_img), out=(out, m_out), dkpt=(dk.view(B, A, K * nd), m_dk.view(B, A, K * nd)),
                y=(perm(y), perm(m_y)), npos=npos)


POSE_KEYS = ("work", "img", "out", "dkpt", "y")


# ---- stand-alone entries ---------------------------------------------------------------------------------------------------------
def oks_inputs(pred_dim, seed=0):
    """gt [7, 17, 3], pred [41, 17, pred_dim], area [7] f32: gt 2 has no visible keypoint, gt 5 has area 0."""
    g = torch.Generator().manual_seed(40 + seed + pred_dim)
    N, M, K = 7, 41, 17
    gt = torch.rand(N, K, 3, generator=g) * 100.0
    gt[..., 2] = torch.randint(0, 3, (N, K), generator=g).float()
    gt[2, :, 2] = 0.0
    gt[0, 0, 2] = -1.0
    pred = gt[torch.arange(M) % N][..., :2] + torch.randn(M, K, 2, generator=g) * 6.0
    if pred_dim == 3:
        pred = torch.cat((pred, torch.rand(M, K, 1, generator=g)), 2)
    area = torch.rand(N, generator=g) * 3000.0 + 500.0
    area[5] = 0.0
    return gt, pred.contiguous(), area


def oks_ref(gt, pred, area, sigma, eps=1e-7, dt=torch.float64):
    """(OKS [N, M], M) of kpt_iou."""
    g, q, a = gt.to(dt), pred.to(dt), area.to(dt)
    sig2 = (2.0 * sigma.to(dt)) ** 2
    dx, dy = g[:, None, :, 0] - q[None, :, :, 0], g[:, None, :, 1] - q[None, :, :, 1]
    ar = (a + eps).view(-1, 1, 1)
    e = (dx * dx + dy * dy) / sig2 / ar / 2
    E = e + (dx.abs() * (g[:, None, :, 0].abs() + q[None, :, :, 0].abs()) + dy.abs() * (g[:, None, :, 1].abs() + q[None, :, :, 1].abs())) / sig2 / ar
    vis = (gt[:, None, :, 2] != 0).to(dt)
    ex = torch.exp(-e)
    cnt = vis.sum(-1) + eps
    return (ex * vis).sum(-1) / cnt, ((ex + TINY) * (1 + E) * vis).sum(-1) / cnt


def bias_inputs(C_, pixels, dtype, seed=0):
    """x [pixels, C] f32 holding values of `dtype`, bias [C] f32."""
    g = torch.Generator().manual_seed(7 * C_ + pixels % 1000 + seed)
    return (torch.randn(pixels, C_, generator=g) * 2.0).to(dtype).float(), torch.randn(C_, generator=g)


def bias_ref(x, bias, dt=torch.float64):
    """{add: (x + bias, M), db: (column sums of x, M)}.  dy_bias_grad promises a fixed pixel order, so the fp32 statement of db adds the
    pixels from left to right in f32; torch.sum is a cascade that no fixed-order kernel reproduces (module docstring)."""
    xd, bd = x.to(dt), bias.to(dt)
    if dt == torch.float64:
        db = xd.sum(0)
    else:
        db = torch.zeros(x.shape[1], dtype=dt)
        for p in range(x.shape[0]):
            db = db + xd[p]
    return dict(add=(xd + bd, xd.abs() + bd.abs()), db=(db, xd.abs().sum(0)))


BIAS_CS = (1, 3, 32, 257)
BIAS_PIXELS = (0, 1, 2047, 2048, 2049, 5000)
BIAS_SHAPES = [(c, p) for c in BIAS_CS for p in BIAS_PIXELS if p]


def decode_inputs(mh, mw, n, dtype, seed=0):
    """proto [3, mh, mw, 32] f32 holding values of `dtype`, det [n, 38] f32 (x1, y1, x2, y2, conf, cls, 32 coefficients; boxes in
    image pixels of an image 4 x the proto), det_img [n] out of order; detection 1 has all coefficients zero."""
    g = torch.Generator().manual_seed(900 + mh + seed)
    proto = torch.randn(3, mh, mw, NM, generator=g).to(dtype).float()
    det = torch.zeros(n, 6 + NM)
    det[:, 6:] = torch.randn(n, NM, generator=g)
    det[1, 6:] = 0.0
    W, H = 4.0 * mw, 4.0 * mh
    traps = [(12.0, 28.0, 24.0, 56.0), (44.0, 10.0, 48.0, 90.0), (13.0, 30.0, 15.0, 70.0), (-10.0, -20.0, 2 * W, 2 * H), (32.0, 52.0, 64.0, 104.0)]
    for j in range(n):
        if j < len(traps):
            det[j, :4] = torch.tensor(traps[j])
        else:
            x1, y1 = float(torch.rand((), generator=g)) * W * 0.5, float(torch.rand((), generator=g)) * H * 0.5
            det[j, :4] = torch.tensor([x1, y1, x1 + W * 0.4, y1 + H * 0.45])
    det[:, 4], det[:, 5] = 0.9, 1.0
    det_img = torch.tensor([(2 * j + 1) % 3 for j in range(n)], dtype=torch.int32)
    return proto, det, det_img, (W, H)


def decode_ref(proto, det, det_img, sx, sy):
    """process_mask(upsample=False): (mask [n, mh, mw] uint8, sure [n, mh, mw] bool).  z in float64; a pixel is `sure` where |z| exceeds
    64 * 2^-24 * sum_k |c_k P_k|, twice the worst-case error of the 32-term f32 dot product, so that sigmoid(z) > 0.5 <=> z > 0 holds
    for any f32 evaluation order."""
    _, mh, mw, _ = proto.shape
    P = proto[det_img.long()].double()
    c = det[:, 6:].double()
    z = torch.einsum("nk,nhwk->nhw", c, P)
    Z = torch.einsum("nk,nhwk->nhw", c.abs(), P.abs())
    bx = det[:, :4].float() * torch.tensor([sx, sy, sx, sy], dtype=torch.float32)
    x1, y1, x2, y2 = [bx[:, j].view(-1, 1, 1) for j in range(4)]
    r = torch.arange(mw, dtype=torch.float32).view(1, 1, -1)
    cc = torch.arange(mh, dtype=torch.float32).view(1, -1, 1)
    crop = (r >= x1) & (r < x2) & (cc >= y1) & (cc < y2)
    return ((z > 0) & crop).to(torch.uint8), (z.abs() > 64 * EPS32 * Z) | ~crop


def mask_iou_ref(pred, gt, overlap, m):
    """f32 inter / ((area_g + area_p) - inter + 1e-7) [m, n] of the integer counts; pred [n, hw] uint8, gt an index map [hw] (label k is
    k + 1, other values ignored) or planes [m, hw]."""
    p = pred.bool()
    planes = torch.stack([gt == k + 1 for k in range(m)]) if overlap else gt.bool()
    inter = (planes[:, None] & p[None]).sum(-1).float()
    ag, ap = planes.sum(-1).float().view(-1, 1), p.sum(-1).float().view(1, -1)
    return inter / (((ag + ap) - inter) + torch.tensor(1e-7))


# ---- measurement -----------------------------------------------------------------------------------------------------------------
def measure(log=print):
    """The largest |r32 - r64| / (2^-24 M) of the fp32 CPU statement per result class (the keys of MEASURED)."""
    worst = {}

    def up(k, a, b):
        worst[k] = max(worst.get(k, 0.0), _ratio(a, b[0], b[1]))
    for run in SEG_RUNS:
        for dn, dtype in DTYPES.items():
            case = make_seg_case(run[0], run[1], dtype)
            r64, r32 = seg_statement(case), seg_statement(case, torch.float32)
            for k in SEG_KEYS:
                up("seg_" + k, r32[k][0], r64[k])
    for run in POSE_RUNS:
        for dn, dtype in DTYPES.items():
            case = make_pose_case(run[0], run[1], dtype)
            r64, r32 = pose_statement(case), pose_statement(case, torch.float32)
            for k in POSE_KEYS:
                up("pose_" + k, r32[k][0], r64[k])
    for pd in (2, 3):
        gt, pred, area = oks_inputs(pd)
        up("oks", oks_ref(gt, pred, area, OKS_SIGMA, dt=torch.float32)[0], oks_ref(gt, pred, area, OKS_SIGMA))
    for C_, pixels in BIAS_SHAPES:
        for dtype in DTYPES.values():
            x, bias = bias_inputs(C_, pixels, dtype)
            r64, r32 = bias_ref(x, bias), bias_ref(x, bias, torch.float32)
            up("bias_add", r32["add"][0], r64["add"])
            up("bias_db", r32["db"][0], r64["db"])
    for k, v in worst.items():
        log(f"    {k:<18s} {v:10.3g} {8 * float(f'{v:.3g}'):12.3f}")
    return worst


if __name__ == "__main__":
    measure()
