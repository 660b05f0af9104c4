"""The yardstick of tests/segpose_ref.py, proved without a GPU: the float64 statement reproduces the reference's recorded mask and keypoint
losses (g16_segloss_*, g17_poseloss_*) on the CPU oracle's assignment; the committed constants are what measure() gives; the conditions
the case list is there for occur; wrong variants of the statement, written in torch fp32, exceed the budgets.

Weak result classes (median power margin, Report.margin, below 4: dropping one mean term of an element would pass its budget):
none.  The smallest median margins are 256 (pose_dkpt), 1.4e3 (seg_dproto) and 3.1e3 (seg_dmc); every other class is above 8e5.
"""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import detloss_ref as D
import segpose_ref as R
from oracle.model import make_anchors
from util import close, gold, make_batch

F32 = torch.float32


def _rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _oracle_assignment(maps, batch, nc):
    """The fp32 CPU oracle's assignment (oracle/loss.py::tal_assign) on three square levels of a 128 x 128 input."""
    B = maps[0].shape[0]
    shapes = [tuple(m.shape[2:]) for m in maps]
    anchors, stride = make_anchors(shapes, [8.0, 16.0, 32.0])
    X = torch.cat([m.reshape(B, 64 + nc, -1) for m in maps], 2).permute(0, 2, 1).contiguous()
    case = SimpleNamespace(X=X, B=B, nc=nc, anchors=anchors, stride=stride, batch_idx=batch["batch_idx"], cls=batch["cls"],
                           bboxes=batch["bboxes"], img_w=128.0, img_h=128.0)
    return D.assignment(case)


# ---- the statement equals the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["overlap", "planes", "masks2x", "planes2x", "nolabels1", "nopos", "nopos_planes"])
def test_seg_statement_reproduces_the_recorded_reference(tag):
    """seg item within 1e-4 relative, d mc and d proto within 1e-3 relative L2 of the reference's v8SegmentationLoss: the tolerances of
    test_mask_loss_vs_reference."""
    g = gold(f"g16_segloss_{tag}")
    B, S, nc = 2, 128, 20
    gen = np.random.default_rng(int(g["seed"]))
    maps = [torch.from_numpy(gen.normal(0, 1.0, (B, 64 + nc, S // s, S // s)).astype(np.float32)) for s in (8, 16, 32)]
    A = sum(t.shape[2] * t.shape[3] for t in maps)
    mc = torch.from_numpy(gen.normal(0, 0.5, (B, 32, A)).astype(np.float32))
    proto = torch.from_numpy(gen.normal(0, 1.0, (B, 32, S // 4, S // 4)).astype(np.float32))
    batch = make_batch(int(g["seed"]) + 1, B, S, [int(v) for v in g["nbox"]], nc)
    asg = _oracle_assignment(maps, batch, nc)
    n_max = max(asg.n_max, 1)
    masks = g["masks"]
    if masks.shape[0] == 0:
        masks = torch.zeros(1, 32, 32, dtype=torch.uint8)
    case = SimpleNamespace(B=B, A=A, mh=32, mw=32, img_h=128.0, img_w=128.0, mask_h=masks.shape[1], mask_w=masks.shape[2],
                           mc=mc.permute(0, 2, 1).contiguous(), proto=proto.permute(0, 2, 3, 1).contiguous(), fg=asg.fg, gi=asg.gt_idx,
                           tbox=asg.tbox, masks=masks, overlap=bool(int(g["overlap"])), batch_idx=batch["batch_idx"], n_max=n_max,
                           rows=R.gt_rows_ref(batch["batch_idx"], B, n_max))
    st = R.seg_statement(case)
    close(st["out"][0][2], g["items"][1], 1e-4, 1e-6, f"{tag} seg item")
    for got, want, what in ((st["dmc"][0].permute(0, 2, 1), g["dmc"], "d mc"), (st["dproto"][0].permute(0, 3, 1, 2), g["dproto"], "d proto")):
        if float(want.abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, what
        else:
            assert _rel_l2(got, want) <= 1e-3, (tag, what, _rel_l2(got, want))
    if tag.startswith("nopos"):
        assert st["npos"] == [0, 0]
    else:
        assert sum(st["npos"]) > 0 and float(g["items"][1]) > 0


@pytest.mark.parametrize("tag", ["normal", "invisible", "nolabels1", "nopos", "k5"])
def test_pose_statement_reproduces_the_recorded_reference(tag):
    """pose and kobj items within 1e-4 relative, d kpt within 1e-3 relative L2 of the reference's v8PoseLoss: the tolerances of
    test_pose_loss_vs_reference."""
    g = gold(f"g17_poseloss_{tag}")
    maps = [g[f"map{i}"] for i in range(3)]
    batch = dict(batch_idx=g["batch_idx"], cls=g["cls"], bboxes=g["bboxes"])
    K, nd = (int(v) for v in g["kpt_shape"])
    B, nc = 2, 4
    asg = _oracle_assignment(maps, batch, nc)
    n_max = max(asg.n_max, 1)
    kpt = g["kpt"].permute(0, 2, 1).contiguous()
    case = SimpleNamespace(levels=[(16, 16, 8.0), (8, 8, 16.0), (4, 4, 32.0)], K=K, ndim=nd, B=B, A=kpt.shape[1], img_h=128.0, img_w=128.0,
                           kpt=kpt, fg=asg.fg, gi=asg.gt_idx, tbox=asg.tbox, keypoints=g["keypoints"], batch_idx=g["batch_idx"],
                           n_max=n_max, rows=R.gt_rows_ref(g["batch_idx"], B, n_max), sigma=R.sigmas_of((K, nd)))
    st = R.pose_statement(case)
    close(st["out"][0][2:4], g["items"][1:3], 1e-4, 1e-6, f"{tag} pose / kobj items")
    got, want = st["dkpt"][0].permute(0, 2, 1), g["dkpt"]
    if float(want.abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0
    else:
        assert _rel_l2(got, want) <= 1e-3, (tag, _rel_l2(got, want))


# ---- constants -------------------------------------------------------------------------------------------------------------------------
def test_committed_constants_are_eight_times_the_measurement():
    got = R.measure(log=lambda *a: None)
    assert set(got) == set(R.MEASURED)
    for k, v in got.items():
        assert float(f"{v:.3g}") == R.MEASURED[k], (k, v, R.MEASURED[k])
        assert R.C[k] == 8.0 * R.MEASURED[k]
    doc = R.__doc__
    for k, v in R.MEASURED.items():
        assert f"    {k:<18s} {v:10.3g} {8 * v:12.3f}" in doc, k


# ---- the conditions of the case list occur ---------------------------------------------------------------------------------------------
def _crop(case, b, a, mode="ref"):
    return R.seg_discrete(case, b, torch.tensor([a]), crop=mode)[0][0]


def test_seg_case_conditions_occur():
    for cid, law in R.SEG_RUNS:
        for dtype in D.DTYPES.values():
            case = R.make_seg_case(cid, law, dtype)
            st = R.seg_statement(case)
            assert st["npos"] == case.spec["npos"], cid
            assert all(bool(torch.isfinite(st[k][0]).all()) and bool(torch.isfinite(st[k][1]).all()) for k in R.SEG_KEYS), (cid, law)
    c = R.make_seg_case("sq", "unit", F32)
    assert c.mh * c.mw == 256
    c = R.make_seg_case("chunks", "unit", F32)
    n0, n1 = c.spec["npos"]
    assert (n0 // 64, n0 % 64, n1 // 64, n1 % 64) == (2, 1, 1, 0)                      # two full chunks plus one; exactly one chunk
    grid = min(10 * c.n_max, c.A)
    assert c.n_max == 2 and grid == 20 and math.ceil(n0 / grid) == 7
    assert (c.mh * c.mw) % 256 != 0 and math.ceil(c.mh * c.mw / 256) == 3
    assert (c.mask_h, c.mask_w) == (12, 12) and not c.overlap and bool((c.batch_idx[1:] < c.batch_idx[:-1]).any())
    cr, _ = R.seg_discrete(c, 0, c.fg[0].nonzero().squeeze(1))
    assert int(cr.sum(0).max()) >= 100                                                      # many positives hit the same proto pixel
    # edges
    c = R.make_seg_case("edges", "unit", F32)
    assert c.masks.dtype == torch.int32 and int(c.masks.max()) == 300 and int(c.gi[1, 40]) == 299
    f = lambda t, img, m: (torch.tensor(float(t)) / torch.tensor(float(img)) * torch.tensor(float(m))).item()       # noqa: E731
    for t in (12, 24, 44, 48):
        assert math.ceil(f(t, 84, 21)) == math.ceil(Fraction(t * 21, 84)) + 1 == math.ceil(t * (21 / 84)) + 1, t
    for t in (28, 56):
        assert math.ceil(f(t, 104, 26)) == math.ceil(Fraction(t * 26, 104)) + 1 == math.ceil(t * (26 / 104)) + 1, t
    assert (math.ceil(f(12, 84, 21)), math.ceil(f(28, 104, 26)), math.ceil(f(56, 104, 26))) == (4, 8, 15)
    assert int(_crop(c, 0, 8).sum()) == 0                                                    # the empty crop
    one = _crop(c, 0, 30)
    assert int(one.sum()) == 1 and bool(one[3, 3])
    assert bool(_crop(c, 1, 0).all()) and float(c.tbox[1, 0].min()) < 0 and float(c.tbox[1, 0, 2]) > c.img_w        # clamped to the whole map
    e = R.crop_edges(c, 1, torch.tensor([13]))[0]
    assert e.tolist() == [8.0, 13.0, 16.0, 26.0]                                             # exact integers: low edge in, high edge out
    ex = _crop(c, 1, 13)
    assert bool(ex[13:26, 8:16].all()) and int(ex.sum()) == 13 * 8
    assert not torch.equal(_crop(c, 0, 1), _crop(c, 0, 1, "reassoc")) and not torch.equal(_crop(c, 0, 7), _crop(c, 0, 7, "reassoc"))
    # nearest
    for cid in ("nearest_ov", "nearest_pl"):
        c = R.make_seg_case(cid, "unit", F32)
        assert int(R.nearest_index(torch.tensor([7]), 62, 14)) == 30 and int(R.nearest_index(torch.tensor([7]), 62, 14, True)) == 31
        assert int(R.nearest_index(torch.tensor([15]), 84, 20)) == 62 and int(R.nearest_index(torch.tensor([15]), 84, 20, True)) == 63
        idx = c.fg[0].nonzero().squeeze(1)
        (cr, g_aten), (_, g_int) = R.seg_discrete(c, 0, idx), R.seg_discrete(c, 0, idx, nearest="int")
        diff = (g_aten != g_int) & cr
        assert bool(diff[0, 7].any()) and bool(diff[0, :, 15].any()) and not bool(diff[0, :7].any())
    # holes
    c = R.make_seg_case("holes", "unit", F32)
    assert c.rows.tolist() == [[1, 2], [-1, -1], [0, -1]] and c.batch_idx.tolist() == [2.0, 0.0, 0.0]
    assert int(c.gi[2, 20]) == 1 and int(c.rows[2, 1]) == -1 and int(c.gi[2, 33]) >= c.n_max
    _, gt = R.seg_discrete(c, 2, c.fg[2].nonzero().squeeze(1))
    assert float(gt[0].sum()) > 0 and float(gt[1].sum()) == 0 and float(gt[2].sum()) == 0
    st = R.seg_statement(c)
    assert float(st["means"][0][1]) == 0 and float(st["dproto"][0][1].abs().max()) == 0 and float(st["dproto"][0][2].abs().max()) > 0
    for cid in ("nopos_ov", "nopos_pl"):
        st = R.seg_statement(R.make_seg_case(cid, "unit", F32))
        assert float(st["out"][0][2]) == 0 and float(st["dproto"][0].abs().max()) == 0 and float(st["dmc"][0].abs().max()) == 0


def test_pose_case_conditions_occur():
    seen_levels = set()
    for cid, law in R.POSE_RUNS:
        for dtype in D.DTYPES.values():
            case = R.make_pose_case(cid, law, dtype)
            st = R.pose_statement(case)
            assert all(bool(torch.isfinite(st[k][0]).all()) and bool(torch.isfinite(st[k][1]).all()) for k in R.POSE_KEYS), (cid, law)
            assert case.A == sum(h * w for h, w, _ in case.levels)
            seen_levels.add(len(case.levels))
    assert seen_levels == {1, 2, 4}
    assert any(h != w for h, w, _ in R.POSE_CASES["rect2"]["levels"])
    assert R.POSE_CASES["four"]["ks"] == (1, 3) and R.POSE_CASES["one"]["ks"] == (5, 2)
    c = R.make_pose_case("rect2", "unit", F32)
    assert bool((c.keypoints[..., 2] < 0).any()) and bool((c.keypoints[..., 2] == 2).any())
    st = R.pose_statement(c)
    e_small = float((st["work"][0][0] / st["work"][0][1].clamp(min=1)).min())
    assert e_small < 0.9, e_small                                                            # not every exponent is saturated
    c = R.make_pose_case("many", "unit", F32)
    st = R.pose_statement(c)
    assert st["npos"] == [300, 1] and c.A == 400
    c = R.make_pose_case("invisible", "unit", F32)
    st = R.pose_statement(c)
    assert float(st["img"][0][2, 0]) == 0 and float(st["img"][0][0, 0]) == 0 and float(st["img"][0][2, 1]) > 0      # nnz = 0: pose 0
    g0 = st["dkpt"][0][0].view(c.A, c.K, 3)
    assert float(g0[..., :2].abs().max()) == 0 and float(g0[..., 2].abs().max()) > 0 and bool(torch.isfinite(g0).all())
    c = R.make_pose_case("holes", "unit", F32)
    st = R.pose_statement(c)
    assert st["npos"] == [3, 0, 3] and int(c.gi[2, 25]) == 1 and int(c.rows[2, 1]) == -1
    assert float(st["work"][0][1, 2, 1]) == 0                                                # the missing row: nothing visible
    t = c.tbox[0, 34]
    assert float((t[2] - t[0]) * (t[3] - t[1])) == 0.25                                      # half a pixel each way
    assert float(c.kpt.view(c.B, c.A, c.K, 3)[..., 2].abs().max()) == 30.0
    st = R.pose_statement(R.make_pose_case("nopos", "unit", F32))
    assert st["npos"] == [0, 0] and float(st["out"][0][2]) == 0 and float(st["dkpt"][0].abs().max()) == 0


@pytest.mark.parametrize("shape", [(9, 7, 11), (26, 21, 7)])
def test_decode_inputs_leave_few_pixels_undecided(shape):
    """The share of pixels the mask-decode test leaves out (|z| within the f32 dot product's error of 0) is at most 0.1 %."""
    mh, mw, n = shape
    assert (n * mh * mw) % 256 != 0
    for dtype in D.DTYPES.values():
        proto, det, det_img, (W, H) = R.decode_inputs(mh, mw, n, dtype)
        mask, sure = R.decode_ref(proto, det, det_img, float(mw / W), float(mh / H))
        share = 1.0 - float(sure.float().mean())
        # detection 1 has z = 0 everywhere: decided (not > 0.5) and therefore not among the unsure
        assert int(mask[1].sum()) == 0
        unsure_other = float((~sure).float()[[j for j in range(n) if j != 1]].mean())
        print(f"proto {mh}x{mw} {dtype}: undecided share {unsure_other:.2e} (with the all-zero detection {share:.2e})")
        assert unsure_other <= 1e-3
        assert sorted(set(det_img.tolist())) == [0, 1, 2] and det_img.tolist() != sorted(det_img.tolist())


# ---- power: wrong variants in torch fp32 exceed the budget -----------------------------------------------------------------------------
def _seg_worst(cid, keys, law="unit", **wrong):
    worst = 0.0
    for dn, dtype in D.DTYPES.items():
        case = R.make_seg_case(cid, law, dtype)
        ref, got = R.seg_statement(case), R.seg_statement(case, F32, **wrong)
        for k in keys:
            out_dt = dtype if k in ("dmc", "dproto") else F32
            worst = max(worst, D.compare(f"{cid} {k}", got[k][0], *ref[k], R.C["seg_" + k], out_dt).worst)
    return worst


def _pose_worst(cid, keys, law="unit", **wrong):
    worst = 0.0
    for dn, dtype in D.DTYPES.items():
        case = R.make_pose_case(cid, law, dtype)
        ref, got = R.pose_statement(case), R.pose_statement(case, F32, **wrong)
        for k in keys:
            worst = max(worst, D.compare(f"{cid} {k}", got[k][0], *ref[k], R.C["pose_" + k], dtype if k == "dkpt" else F32).worst)
    return worst


def test_right_statement_in_fp32_passes_every_budget():
    """An eighth of the budget at most, by construction (times 1.005: the constants are committed to three digits)."""
    for cid, law in R.SEG_RUNS:
        assert _seg_worst(cid, R.SEG_KEYS, law) <= 1.005 / 8, (cid, law)
    for cid, law in R.POSE_RUNS:
        assert _pose_worst(cid, R.POSE_KEYS, law) <= 1.005 / 8, (cid, law)


SEG_MUTANTS = [("crop with floor instead of ceil", "edges", ("lossp", "dmc", "dproto"), dict(crop="floor")),
               ("crop from t * (mw / img)", "edges", ("lossp", "dmc", "dproto"), dict(crop="reassoc")),
               ("nearest index by integer arithmetic (index map)", "nearest_ov", ("lossp", "dmc", "dproto"), dict(nearest="int")),
               ("nearest index by integer arithmetic (planes)", "nearest_pl", ("lossp", "dmc", "dproto"), dict(nearest="int")),
               ("y / x swapped in the gt lookup", "edges", ("lossp", "dmc", "dproto"), dict(swap=True)),
               ("positive number 64 dropped from d proto", "chunks", ("dproto",), dict(drop=64)),
               ("1 / area missing", "sq", ("lossp", "dmc", "dproto"), dict(use_area=False)),
               ("per-image mean replaced by a sum", "sq", ("means", "out", "dmc", "dproto"), dict(mean=False))]
POSE_MUTANTS = [("factor n K / nnz dropped", "rect2", ("img", "out"), dict(factor=False)),
                ("kobj divided by n instead of n K", "rect2", ("img", "out"), dict(kobj_div_k=False)),
                ("visibility > 0 instead of != 0", "rect2", ("work", "img", "out", "dkpt"), dict(vis_ne=False))]


@pytest.mark.parametrize("name,cid,keys,wrong", SEG_MUTANTS, ids=[m[0] for m in SEG_MUTANTS])
def test_wrong_seg_variants_exceed_the_budget(name, cid, keys, wrong):
    for k in keys:
        r = _seg_worst(cid, (k,), **wrong)
        print(f"{name}: {k} on {cid}: {r:.3g} of budget")
        assert r > 1.0, (name, k, r)


@pytest.mark.parametrize("name,cid,keys,wrong", POSE_MUTANTS, ids=[m[0] for m in POSE_MUTANTS])
def test_wrong_pose_variants_exceed_the_budget(name, cid, keys, wrong):
    for k in keys:
        r = _pose_worst(cid, (k,), **wrong)
        print(f"{name}: {k} on {cid}: {r:.3g} of budget")
        assert r > 1.0, (name, k, r)


# ---- power margins -------------------------------------------------------------------------------------------------------------------
def power_margins():
    """Median power margin (Report.margin) per result class: the smallest over the runs and dtypes, of the fp32 statement against the
    float64 one.  n_terms: 32 products behind a gradient element, one term else."""
    out = {}
    for runs, make, stmt, keys, pre in ((R.SEG_RUNS, R.make_seg_case, R.seg_statement, R.SEG_KEYS, "seg_"),
                                        (R.POSE_RUNS, R.make_pose_case, R.pose_statement, R.POSE_KEYS, "pose_")):
        for cid, law in runs:
            for dn, dtype in D.DTYPES.items():
                case = make(cid, law, dtype)
                ref, got = stmt(case), stmt(case, F32)
                for k in keys:
                    out_dt = dtype if k in ("dmc", "dproto", "dkpt") else F32
                    rep = D.compare(k, got[k][0], *ref[k], R.C[pre + k], out_dt)
                    if rep.n and math.isfinite(rep.margin):
                        out[pre + k] = min(out.get(pre + k, float("inf")), rep.margin)
    return out


def test_weak_classes_are_the_listed_ones():
    m = power_margins()
    for k, v in sorted(m.items()):
        print(f"{k}: smallest median power margin {v:.3g}")
    weak = sorted(k for k, v in m.items() if v < 4)
    listed = sorted(line.split()[0] for line in __doc__.split("below 4: dropping one mean term of an element would pass its budget):")[1].splitlines()
                    if line.startswith("    ") and line.split())
    assert weak == listed, (weak, listed)


def test_every_seg_and_pose_entry_is_named_in_the_gpu_test():
    import os
    import re

    import test_gpu_segpose_kernels as T
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dedark_yolo_amd", "csrc")
    names = []
    for f in ("seg.hip", "pose.hip"):
        with open(os.path.join(src, f)) as fh:
            names += re.findall(r'extern "C" int (dy_\w+)\(', fh.read())
    assert len(names) == 13 and sorted(names) == sorted(T.ENTRIES)
