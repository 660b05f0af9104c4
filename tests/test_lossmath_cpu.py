"""csrc/dy_lossmath.h on the host, against the float64 statement of tests/detloss_ref.py and under its budgets; the case list's own
conditions; wrong variants that the budgets must catch; the committed constants against a re-measurement.  No GPU: a small shim is
compiled with the host compiler into tmp_path and loaded with ctypes."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detloss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dedark_yolo_amd", "csrc")

SHIM = r"""
#include "dy_lossmath.h"
extern "C" {
void sh_ciou(const float* b1, const float* b2, long n, float* out, float* g) {
  for (long i = 0; i < n; ++i) out[i] = g ? dy_ciou_grad(b1 + 4 * i, b2 + 4 * i, g + 4 * i) : dy_ciou(b1 + 4 * i, b2 + 4 * i);
}
void sh_iou_any(const float* b1, const float* b2, long n, int xywh, int kind, float eps, float* out, float* g) {
  for (long i = 0; i < n; ++i) out[i] = dy_box_iou_any(b1 + 4 * i, b2 + 4 * i, xywh, kind, eps, g ? g + 4 * i : nullptr);
}
void sh_softmax_expect(const float* x, long n, float* p, float* e) {
  for (long i = 0; i < n; ++i) e[i] = dy_softmax_expect(x + 16 * i, 16, p + 16 * i);
}
void sh_dfl_side(const float* x, const float* t, long n, float* out, float* wl, int* tl) {
  for (long i = 0; i < n; ++i) out[i] = dy_dfl_side(x + 16 * i, t[i], wl + i, tl + i);
}
void sh_bce(const float* x, const float* t, long n, float* out) {
  for (long i = 0; i < n; ++i) out[i] = dy_bce(x[i], t[i]);
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("lossmath")
    src, so = os.path.join(d, "shim.cpp"), os.path.join(d, "liblossmath_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(t):
    return np.ascontiguousarray(t.detach().numpy().astype(np.float32))


def _check(rep):
    print(rep)
    assert rep.worst <= 1.0, str(rep)


_runs = {}


def _run(run, dn):
    """(case, assignment, fp64 statement) of one run, computed once."""
    if (run, dn) not in _runs:
        case = R.make_case(run[0], run[1], R.DTYPES[dn])
        asg = R.assignment(case)
        _runs[(run, dn)] = (case, asg, R.statement(case, asg))
    return _runs[(run, dn)]


# ---- the case list ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", R.RUNS, ids=R.run_id)
def test_case_conditions_occur(run):
    """Every condition a case is listed for occurs in each dtype; positives where they are expected (at least 10, exactly one for
    the weak case, none in an empty image); no positive on a CIoU kink; everything finite (the `wide` law in f16 too)."""
    for dn in R.DTYPES:
        case, asg, st = _run(run, dn)
        got = R.conditions(case, asg, st["ltrb"])
        for name in case.spec["conds"]:
            assert got[name], (R.run_id(run), dn, name)
        for b, want in enumerate(case.spec["min_pos"]):
            n = int(asg.fg[b].sum())
            assert (n == want) if want <= 1 else (n >= want), (R.run_id(run), dn, b, n)
        assert R.kink_gap(case, asg, st["pred"][0]) >= 1e-4, (R.run_id(run), dn)
        assert all(bool(torch.isfinite(st[k][0]).all()) for k in ("pred", "norm", "acc", "grad", "y"))
        assert bool(torch.isfinite(case.X.to(R.DTYPES[dn])).all())


def test_case_list_reaches_the_paths_it_is_there_for():
    A = {k: sum(h * w for h, w, _ in v["levels"]) for k, v in R.CASES.items()}
    assert (A["one639"], A["one640"], A["one641"], A["sq84"], A["rect840"], A["two"], A["four"]) == (639, 640, 641, 84, 840, 60, 1020)
    assert {len(v["levels"]) for v in R.CASES.values()} == {1, 2, 3, 4}
    assert {v["nc"] for v in R.CASES.values()} == {1, 3, 20, 80, 81} and not R.CASES["empty"]["boxes"]
    assert any(h != w for v in R.CASES.values() for h, w, _ in v["levels"])
    # a box wider than 2 * 15 cells of the finest level, in the cases listed for the upper clamp
    for k, v in R.CASES.items():
        if "upper_clamp" in v["conds"]:
            assert any(b[4] - b[2] > 2 * 15 * v["levels"][0][2] for b in v["boxes"]), k


# ---- dy_lossmath.h against the statement ------------------------------------------------------------------------------------------------
def _host_iou(shim, b1, b2, xywh, kind, grad, ciou_entry=False):
    a, b = _f32(b1), _f32(b2)
    out = np.full(a.shape[0], np.nan, np.float32)
    g = np.full(a.shape, np.nan, np.float32) if grad else None
    if ciou_entry:
        shim.sh_ciou(_p(a), _p(b), C.c_long(a.shape[0]), _p(out), _p(g) if grad else None)
    else:
        shim.sh_iou_any(_p(a), _p(b), C.c_long(a.shape[0]), xywh, kind, C.c_float(1e-7), _p(out), _p(g) if grad else None)
    return torch.from_numpy(out), (torch.from_numpy(g) if grad else None)


def test_ciou_and_ciou_grad(shim):
    b1, b2 = R.iou_inputs(0)
    ref, m, gref, gm = R.iou_ref(b1, b2, 0, 3)
    v0, _ = _host_iou(shim, b1, b2, 0, 3, False, ciou_entry=True)
    v1, g1 = _host_iou(shim, b1, b2, 0, 3, True, ciou_entry=True)
    _check(R.compare("dy_ciou", v0, ref, m, R.C["ciou_xyxy"], n_terms=3))
    _check(R.compare("dy_ciou_grad value", v1, ref, m, R.C["ciou_xyxy"], n_terms=3))
    _check(R.compare("dy_ciou_grad gradient", g1, gref, gm, R.C["ciou_xyxy_grad"], n_terms=3))


@pytest.mark.parametrize("xywh", [0, 1], ids=["xyxy", "xywh"])
@pytest.mark.parametrize("kind", range(4), ids=R.KINDS)
def test_box_iou_any(shim, kind, xywh):
    """All eight modes on the case list's positives and the edge boxes (identical, nested, disjoint, touching, shared edges with the
    gradient tie split in half, zero width), the same boxes as xyxy and as xywh."""
    b1, b2 = R.iou_inputs(xywh)
    ref, m, gref, gm = R.iou_ref(b1, b2, xywh, kind)
    key = R.iou_key(xywh, kind)
    v0, _ = _host_iou(shim, b1, b2, xywh, kind, False)
    v1, g1 = _host_iou(shim, b1, b2, xywh, kind, True)
    assert torch.equal(v0, v1)
    _check(R.compare(key, v1, ref, m, R.C[key], n_terms=3))
    _check(R.compare(key + " gradient", g1, gref, gm, R.C[key + "_grad"], n_terms=3))
    if not xywh:          # shared edges (row 5 of the edge set): the x gradients are half of what either branch alone would give
        row = b1.shape[0] - R.EDGE_B1.shape[0] + 5
        assert float(gref[row, 0]) != 0.0 and abs(float(g1[row, 0]) / float(gref[row, 0]) - 1) < 1e-3


def test_softmax_expect_decodes_the_boxes(shim):
    for run, dn in ((("sq84", "unit"), "f32"), (("rect840", "peaked"), "bf16"), (("four", "unit"), "f16")):
        case, asg, st = _run(run, dn)
        x = _f32(case.X[..., :64].reshape(-1, 16))
        p, e = np.full(x.shape, np.nan, np.float32), np.full(x.shape[0], np.nan, np.float32)
        shim.sh_softmax_expect(_p(x), C.c_long(x.shape[0]), _p(p), _p(e))
        d = torch.from_numpy(e).view(case.B, case.A, 4)
        pred = torch.cat((case.anchors - d[..., :2], case.anchors + d[..., 2:]), -1)           # f32, as decode_kernel
        _check(R.compare(f"decode {R.run_id(run)} {dn}", pred, *st["pred"], R.C["decode"], n_terms=17))
        assert np.allclose(p.sum(1), 1.0, atol=1e-5)


def test_dfl_side(shim):
    _, _, ds, ts = R.standalone_inputs()
    ref, m, _, _ = R.dfl_ref(ds, ts)
    x, t = _f32(ds.reshape(-1, 16)), _f32(ts.reshape(-1))
    out, wl, tl = np.full(t.shape, np.nan, np.float32), np.full(t.shape, np.nan, np.float32), np.full(t.shape, -1, np.int32)
    shim.sh_dfl_side(_p(x), _p(t), C.c_long(t.shape[0]), _p(out), _p(wl), _p(tl))
    val = torch.from_numpy(out).view(-1, 4)
    val = (val[:, 0] + val[:, 1] + val[:, 2] + val[:, 3]) * 0.25
    _check(R.compare("dy_dfl_side", val, ref, m, R.C["dfl"], n_terms=4))
    assert np.array_equal(tl, t.astype(np.int32)) and np.array_equal(wl, (tl + 1).astype(np.float32) - t)
    assert tl.max() == 14 and tl.min() == 0          # both ends of the clamp are among the targets


@pytest.mark.parametrize("run", R.RUNS, ids=R.run_id)
def test_bce_elements(shim, run):
    """dy_bce on every class logit of the run against the fp64 element, the target the oracle's fp32 score."""
    for dn in R.DTYPES:
        case, asg, st = _run(run, dn)
        t = torch.zeros(case.B, case.A, case.nc)
        bi, ai = asg.fg.nonzero(as_tuple=True)
        t[bi, ai, asg.label[bi, ai]] = asg.norm32[bi, ai]
        x = case.X[..., 64:]
        ref = R.bce_log1p(x.double(), t.double())
        m = x.double().clamp(min=0) + (x.double() * t.double()).abs() + torch.log1p(torch.exp(-x.double().abs()))
        a, b = _f32(x.reshape(-1)), _f32(t.reshape(-1))
        out = np.full(a.shape, np.nan, np.float32)
        shim.sh_bce(_p(a), _p(b), C.c_long(a.shape[0]), _p(out))
        _check(R.compare(f"dy_bce {R.run_id(run)} {dn}", torch.from_numpy(out).view_as(x), ref, m, R.C["bce"], n_terms=1))


# ---- the budgets can fail -----------------------------------------------------------------------------------------------------------
def _ciou_var(eps_w=False, alpha_grad=False, kink_full=False):
    """bbox_iou(xywh=False, CIoU=True) with one thing wrong, in the signature of oracle.loss.bbox_iou."""
    def mx(a, b):
        return torch.where(a >= b, a, b) if kink_full else torch.maximum(a, b)

    def mn(a, b):
        return torch.where(a <= b, a, b) if kink_full else torch.minimum(a, b)

    def fn(b1, b2, xywh=False, GIoU=False, DIoU=False, CIoU=True, eps=1e-7):
        x1, y1, x2, y2 = b1.unbind(-1)
        X1, Y1, X2, Y2 = b2.unbind(-1)
        ew = eps if eps_w else 0.0
        w1, h1, w2, h2 = x2 - x1 + ew, y2 - y1 + eps, X2 - X1 + ew, Y2 - Y1 + eps
        inter = (mn(x2, X2) - mx(x1, X1)).clamp(min=0) * (mn(y2, Y2) - mx(y1, Y1)).clamp(min=0)
        union = w1 * h1 + w2 * h2 - inter + eps
        iou = inter / union
        c2 = (mx(x2, X2) - mn(x1, X1)) ** 2 + (mx(y2, Y2) - mn(y1, Y1)) ** 2 + eps
        rho2 = ((X1 + X2 - x1 - x2) ** 2 + (Y1 + Y2 - y1 - y2) ** 2) / 4
        v = (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
        a = v / (v - iou + (1 + eps))
        return (iou - (rho2 / c2 + v * (a if alpha_grad else a.detach()))).unsqueeze(-1)
    return fn


def _dfl_var(swap=False, side_scale=0.25):
    def fn(pred, target):
        tl = target.long().clamp(max=15)
        tr = (tl + 1).clamp(max=15)
        wl = (tl + 1) - target
        wr = 1 - wl
        if swap:
            wl, wr = wr, wl
        lp = -F.log_softmax(pred, -1).view(*target.shape, 16)
        return (lp.gather(2, tl.unsqueeze(-1)).squeeze(-1) * wl + lp.gather(2, tr.unsqueeze(-1)).squeeze(-1) * wr).sum(-1, keepdim=True) * side_scale
    return fn


def _iou_grad_worst(fn):
    b1, b2 = R.iou_inputs(0)
    ref, m, gref, gm = R.iou_ref(b1, b2, 0, 3)
    v, _, g, _ = R.iou_ref(b1, b2, 0, 3, torch.float32, fn=fn)
    return R.compare("value", v, ref, m, R.C["ciou_xyxy"]).worst, R.compare("gradient", g, gref, gm, R.C["ciou_xyxy_grad"]).worst


def test_right_variants_pass_the_budgets():
    """The variant code with nothing switched on is under budget in fp32, so a variant that fails does so for what is wrong in it."""
    assert max(_iou_grad_worst(_ciou_var())) <= 1.0
    _, _, ds, ts = R.standalone_inputs()
    ref, m, gref, gm = R.dfl_ref(ds, ts)
    v, _, g, _ = R.dfl_ref(ds, ts, torch.float32, fn=_dfl_var())
    assert R.compare("dfl", v, ref, m, R.C["dfl"]).worst <= 1.0 and R.compare("dfl gradient", g, gref, gm, R.C["dfl_grad"]).worst <= 1.0


def test_wrong_ciou_variants_exceed_the_budget():
    v, g = _iou_grad_worst(_ciou_var(eps_w=True))
    print("eps on w as well: value", v, "gradient", g)
    assert v > 1.0
    v, g = _iou_grad_worst(_ciou_var(alpha_grad=True))
    print("alpha differentiated: value", v, "gradient", g)
    assert v <= 1.0 and g > 1.0
    v, g = _iou_grad_worst(_ciou_var(kink_full=True))
    print("kink weight 1: value", v, "gradient", g)
    assert v <= 1.0 and g > 1.0


def test_wrong_dfl_variants_exceed_the_budget():
    _, _, ds, ts = R.standalone_inputs()
    ref, m, _, _ = R.dfl_ref(ds, ts)
    for name, fn in (("wl and wr swapped", _dfl_var(swap=True)), ("a side's 0.25 dropped", _dfl_var(side_scale=1.0))):
        v, _, _, _ = R.dfl_ref(ds, ts, torch.float32, fn=fn)
        w = R.compare(name, v, ref, m, R.C["dfl"]).worst
        print(name, w)
        assert w > 1.0


def _acc_worst(st32, st64):
    return [R.compare(k, st32["acc"][0][i], st64["acc"][0][i], st64["acc"][1][i], R.C[k]).worst for i, k in enumerate(R.ACC_KEYS)]


def test_wrong_criterion_variants_exceed_the_budget():
    """Clamp at 15.0 (on a case where the upper clamp is hit), the BCE target on label + 1, norm without pos_overlap: the fp32
    statement with the fault against the fp64 one; the same fp32 statement without the fault stays under budget."""
    case, asg, st = _run(("one640", "unit"), "f32")
    assert max(_acc_worst(R.statement(case, asg, torch.float32, dfl=_dfl_var()), st)) <= 1.0
    w = _acc_worst(R.statement(case, asg, torch.float32, dfl=_dfl_var(), clamp_hi=15.0), st)
    print("clamp at 15.0:", w)
    assert w[3] > 1.0 and max(w[:3]) <= 1.0
    case, asg, st = _run(("sq84", "unit"), "f32")
    bad = R.statement(case, asg, torch.float32, label_shift=1)
    w = _acc_worst(bad, st)
    g = R.compare("grad", bad["grad"][0], *st["grad"], R.grad_constants(case.nc)).worst
    print("BCE target on label + 1:", w, g)
    assert w[1] > 1.0 and g > 1.0
    bad = R.statement(case, asg, torch.float32, norm_overlap=False)
    w = R.compare("norm", bad["norm"][0], *st["norm"], R.C["norm"]).worst
    print("norm without pos_overlap:", w)
    assert w > 1.0


# ---- the constants ---------------------------------------------------------------------------------------------------------------------
def test_committed_constants_are_eight_times_the_measurement():
    """On a fast subset of the runs (and all of the stand-alone inputs) the re-measured yardsticks are at most the committed ones, the
    constants are 8 times those, and torch's fp32 BCE formula loses whole elements on the init law."""
    found = R.measure(runs=[("sq84", "unit"), ("rect840", "init"), ("two", "unit"), ("empty", "init")], dtypes=("f32", "bf16"), log=lambda *a: None)
    for k, v in R.MEASURED.items():
        assert R.C[k] == 8.0 * v
        assert R.C[k] >= 8.0 * found[k], (k, found[k], v)
    assert found["bce_torch"] > 1e4 and R.MEASURED_TORCH_BCE["bce"] > 1e4 and found["acc_bce_torch"] > 1e3
    # the stand-alone yardsticks are measured in full here: the committed figures are not stale (half of them is reached)
    for k in ("dfl", "dfl_grad") + tuple(R.iou_key(x, kd) + s for x in (0, 1) for kd in range(4) for s in ("", "_grad")):
        assert found[k] > 0.5 * R.MEASURED[k], (k, found[k], R.MEASURED[k])


# ---- bookkeeping -----------------------------------------------------------------------------------------------------------------------
def test_every_loss_entry_is_named_in_the_gpu_test():
    with open(os.path.join(CSRC, "loss.hip")) as f:
        entries = set(re.findall(r'extern "C" int (dy_\w+)\(', f.read()))
    assert len(entries) >= 14 and "dy_loss_prepare_targets" in entries
    with open(os.path.join(ROOT, "tests", "test_gpu_detloss_kernels.py")) as f:
        called = set(re.findall(r'call\("(dy_\w+)"', f.read()))
    assert entries <= called, sorted(entries - called)


def test_header_names_this_harness():
    with open(os.path.join(CSRC, "dy_lossmath.h")) as f:
        assert "tests/test_lossmath_cpu.py" in f.readline()
