"""GPU tests of the classify task: every entry point of csrc/classify.hip through the C-ABI against float64 torch on the same stored
(already rounded) inputs (tests/classify_ref.py), the reference's fixtures (tests/golden/make_classify_golden.py), the Classify head
and whole tiny models against the reference, low-precision steps against the fp32 HIP path, and the trainer / validator / predict()
surface.

Tolerances.  u = 2^-24 (f32), 2^-8 (bf16: 8 significant bits), 2^-11 (f16).  A value the kernel rounds ONCE into a 16-bit type may
differ from the float64 reference by u |ref| (a bound on half an ulp), on top of what its f32 arithmetic contributes:
  pool forward   HW f32 additions of |x| <= 1: HW 2^-24 mean|x| (<= 3e-6 at HW = 49), then the output rounding
  pool backward  one f32 division, then the output rounding
  loss           util.close's standing 1e-4 / 1e-5; gradient the same for f32, plus the output rounding for the 16-bit types
  f16 outputs below 2^-14 are subnormal: their spacing is 2^-24 whatever the value, so half of it (2^-25) is added to the rounding term
  soft-max       z - m is exact to 2^-24 |z - m| (|z - m| <= 25 here: 1.5e-6 relative after exp), expf 2 ulp, the sum of nc terms in a
                 64-lane tree (6 + nc / 64) 2^-24 <= 1.4e-6, one division: together below 4e-6, bound 1e-5 relative
"""

import numpy as np
import pytest
import torch

import classify_ref as cr
from util import close, gold, load_yaml, rnd

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
ULP = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUBNORMAL = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
TINY = [0.33, 0.125, 1024]


@pytest.fixture(autouse=True)
def _fp32():
    import dedark_yolo_amd as dy
    dy.set_compute_dtype(torch.float32)
    yield
    dy.set_compute_dtype(torch.float32)


def _call(name, *args):
    from dedark_yolo_amd import _C
    _C.call(name, *args)


def _st():
    from dedark_yolo_amd.ops import stream
    return stream()


def _did(dtype):
    from dedark_yolo_amd.ops import dt_id
    return dt_id(dtype)


def _ve(dtype):
    return 4 if dtype == torch.float32 else 8


def _within(got, ref, tol, what):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.3e}, max ref {float(ref.abs().max()):.3e}"


def _rows(x, ld, poison):
    """x [B, n] (already in its dtype) inside a [B, ld] device buffer whose other columns hold `poison`; returns (buffer, view)"""
    B, n = x.shape
    buf = torch.full((B, ld), poison, dtype=x.dtype, device="cuda")
    buf[:, :n] = x.cuda()
    return buf, buf[:, :n]


# ---------------------------------------------------------------------------------------------------- pool
POOL_SHAPES = [(N, HW, Cc, pad) for N in (1, 5) for HW in (1, 4, 9, 49) for Cc in (8, 1280) for pad in (16,)] + [(2, 9, 13, 3), (3, 4, 20, 16)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pool_forward_and_backward_vs_float64(dtype):
    """dy_gap_fwd / dy_gap_bwd on a channel slice of a wider buffer (x_ld = C + pad; C = 13 and an odd pad take the scalar paths):
    values against float64 on the stored inputs, and the bytes beyond C in every pixel / row untouched."""
    u, did = ULP[dtype], _did(dtype)
    for ci, (N, HW, Cc, pad) in enumerate(POOL_SHAPES):
        ld = Cc + pad
        x = rnd(300 + ci, N, HW, Cc, lo=-1, hi=1).to(dtype)
        xb = torch.full((N, HW, ld), 7.0, dtype=dtype, device="cuda")
        xb[:, :, :Cc] = x.cuda()
        yb = torch.full((N, ld), -3.0, dtype=dtype, device="cuda")
        _call("dy_gap_fwd", xb.data_ptr(), ld, N, HW, Cc, did, yb.data_ptr(), ld, _st())
        ref = cr.gap_fwd(x)
        tol = HW * 2.0 ** -24 * x.double().abs().mean(1) + u * ref.abs() + SUBNORMAL[dtype] + 1e-12
        _within(yb[:, :Cc], ref, tol, f"pool fwd {N, HW, Cc, pad}")
        assert bool((yb[:, Cc:] == -3.0).all()) and bool((xb[:, :, Cc:] == 7.0).all()), (N, HW, Cc, pad)
        dy = rnd(400 + ci, N, Cc, lo=-1, hi=1).to(dtype)
        dyb = torch.full((N, ld), 9.0, dtype=dtype, device="cuda")
        dyb[:, :Cc] = dy.cuda()
        dxb = torch.full((N, HW, ld), 5.0, dtype=dtype, device="cuda")
        _call("dy_gap_bwd", dyb.data_ptr(), ld, N, HW, Cc, did, dxb.data_ptr(), ld, _st())
        ref = cr.gap_bwd(dy, HW)
        _within(dxb[:, :, :Cc], ref, (u + 2.0 ** -23) * ref.abs() + SUBNORMAL[dtype] + 1e-12, f"pool bwd {N, HW, Cc, pad}")
        assert bool((dxb[:, :, Cc:] == 5.0).all()), (N, HW, Cc, pad)
    torch.cuda.synchronize()


def test_pool_wrappers_make_nhwc_views():
    from dedark_yolo_amd import ops
    x = rnd(77, 2, 16, 3, 3, lo=-1, hi=1).cuda().contiguous(memory_format=torch.channels_last)
    y = ops.gap_fwd(x)
    assert tuple(y.shape) == (2, 16, 1, 1)
    close(y[:, :, 0, 0].cpu(), x.cpu().double().mean((2, 3)), 1e-5, 1e-6, "gap_fwd")
    dx = ops.gap_bwd(y, 3, 3)
    close(dx.cpu(), (y.cpu().double() / 9).expand(2, 16, 3, 3), 1e-6, 1e-9, "gap_bwd")


# ---------------------------------------------------------------------------------------------------- loss
def _xent(zv, cls, dtype, dpad=None):
    """the two entry points on logits rows `zv` ([B, nc] view, any leading dimension): loss [1], row_lse, full gradient buffer"""
    from dedark_yolo_amd import ops
    B, nc, ld = ops.row_matrix(zv)
    lse = torch.empty(B, dtype=torch.float32, device="cuda")
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    _call("dy_cls_xent_fwd", zv.data_ptr(), ld, _did(dtype), cls.data_ptr(), B, nc, lse.data_ptr(), loss.data_ptr(), _st())
    dld = ops.round_up(nc, _ve(dtype)) + (_ve(dtype) if dpad is None else dpad)
    d = torch.full((B, dld), float("nan"), dtype=dtype, device="cuda")
    gout = torch.ones(1, dtype=torch.float32, device="cuda")
    _call("dy_cls_xent_bwd", zv.data_ptr(), ld, _did(dtype), cls.data_ptr(), lse.data_ptr(), gout.data_ptr(), B, nc, d.data_ptr(), dld, _st())
    return loss, lse, d


def _labels(B, nc, seed):
    g = np.random.default_rng(seed)
    cls = torch.from_numpy(g.integers(0, nc, B).astype(np.int64))
    if B >= 5:
        cls[1] = -100                    # torch's ignore_index
    if B >= 70:
        cls[3] = nc + 3                  # outside the classes (device labels are not checked on the host): adds 0, indexes nothing
        cls[4] = -7
    return cls


def _grad_tol(ref, dtype):
    t = 1e-5 + 1e-4 * ref.abs()
    return t if dtype == torch.float32 else t + ULP[dtype] * ref.abs()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_xent_vs_float64(dtype):
    """nc 1 / 3 / 10 / 1000 / 1003 (a vector tail, more than one pass per wave), B 1 / 5 / 70 (more than one block), ld > nc, labels
    of -100 and outside [0, nc): loss, gradient, exactly-zero pad columns, identical bytes on a second run."""
    ve = _ve(dtype)
    for ci, (nc, B) in enumerate((nc, B) for nc in (1, 3, 10, 1000, 1003) for B in (1, 5, 70)):
        z = (torch.from_numpy(np.random.default_rng(500 + ci).normal(0, 3, (B, nc)).astype(np.float32))).to(dtype)
        ld = (nc + ve - 1) // ve * ve + (ve if ci % 2 == 0 else 3)       # aligned and unaligned leading dimensions
        _, zv = _rows(z, ld, float("nan"))
        cls = _labels(B, nc, 600 + ci)
        dpad = 3 if ci % 4 == 1 else None                               # ... and of the gradient buffer
        loss, lse, d = _xent(zv, cls.cuda(), dtype, dpad)
        rl, rg = cr.xent(z, cls)
        close(loss.cpu(), rl, 1e-4, 1e-5, f"loss nc={nc} B={B}")
        _within(d[:, :nc], rg, _grad_tol(rg, dtype), f"gradient nc={nc} B={B}")
        assert bool((d[:, nc:] == 0).all()), f"pad columns nc={nc} B={B}"
        _within(lse, torch.logsumexp(z.double(), 1), 1e-5 + 1e-6 * torch.logsumexp(z.double(), 1).abs(), f"row_lse nc={nc} B={B}")
        if B >= 5:
            assert float(d[1].abs().max()) == 0.0
        loss2, lse2, d2 = _xent(zv, cls.cuda(), dtype, dpad)
        assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(lse.view(torch.int32), lse2.view(torch.int32))
        assert torch.equal(d.view(torch.uint8), d2.view(torch.uint8)), f"two runs differ nc={nc} B={B}"
    torch.cuda.synchronize()


def test_xent_stays_finite_at_large_logits():
    """f32 logits up to +-80 (exp overflows f16 and underflows in f32 without the running maximum) and f16 logits at +-6e4.  row_lse
    is an f32 of magnitude max|z|: half an ulp of it, 2^-24 max|z|, moves exp(z - lse) by that relative amount (0.4 % at 6e4), which
    the gradient bound gains as 2^-23 max|z| (|ref| + 1 / 64)."""
    g = np.random.default_rng(7)
    for dtype, amp in ((torch.float32, 80.0), (torch.float16, 6.0e4), (torch.bfloat16, 3.0e4)):
        z = torch.from_numpy((g.choice([-1.0, 1.0], (6, 37)) * g.uniform(0.5, 1.0, (6, 37)) * amp).astype(np.float32)).to(dtype)
        _, zv = _rows(z, 48, float("nan"))
        cls = torch.from_numpy(g.integers(0, 37, 6).astype(np.int64))
        loss, lse, d = _xent(zv, cls.cuda(), dtype)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(d.float()).all()), dtype
        rl, rg = cr.xent(z, cls)
        close(loss.cpu(), rl, 1e-4, 1e-5, f"loss {dtype}")
        _within(d[:, :37], rg, _grad_tol(rg, dtype) + 2.0 ** -23 * amp * (rg.abs() + 1 / 64), f"gradient {dtype}")


@pytest.mark.parametrize("tag", ["normal", "ignore", "big"])
def test_classification_loss_vs_reference(tag):
    """v8ClassificationLoss (the autograd.Function over both entry points) on the reference's fixtures: loss, items, gradient; the
    gradient arrives as rows of a padded buffer whose pad columns are zero, scaled by the incoming gradient on the device."""
    from dedark_yolo_amd.utils.loss import v8ClassificationLoss
    g = gold(f"g21_clsloss_{tag}")
    z = g["logits"].cuda().requires_grad_(True)
    loss, items = v8ClassificationLoss()(z, dict(cls=g["cls"]))
    assert loss.dim() == 0 and items.dim() == 0 and not items.requires_grad
    (loss * 3.0).backward()
    close(loss.detach().cpu(), g["loss"], 1e-4, 1e-5, "loss")
    close(items.cpu(), g["items"], 1e-4, 1e-5, "items")
    close(z.grad.cpu() / 3.0, g["dlogits"], 1e-4, 1e-5, "dlogits")
    if tag == "ignore":
        assert float(z.grad[1].abs().max()) == 0.0
    with pytest.raises(ValueError):
        v8ClassificationLoss()(z.detach(), dict(cls=torch.full_like(g["cls"], z.shape[1])))


# ---------------------------------------------------------------------------------------------------- soft-max
def _rowsum_bound(nc):
    """|sum_j p_j - 1| within f32 rounding, in units of 2^-24, worst case.  sum_j p_j - 1 = sum_j p_j d_j, d_j the relative error of p_j:
      write pass   the rounding of z - m moves exp by |z - m| 2^-24; weighted by p that is (m - sum_j p_j z_j) <= ln(nc); expf 2; the
                   division 1: ln(nc) + 3
      the sum s    per lane nc / 64 terms, each an add (1/2) and at worst a rescale (expf 2, multiply 1/2, its argument 1): 4 nc / 64;
                   the terms' own expf and argument rounding 2 + ln(nc); the butterfly's 6 merges of two expf, two multiplies and an
                   add, 3.5 each: 21
    together 2 ln(nc) + 26 + 4 nc / 64 (26 at nc = 1, 103 at nc = 1003)."""
    return (2.0 * np.log(nc) + 26.0 + 4.0 * nc / 64.0) * 2.0 ** -24


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_softmax_vs_float64(dtype):
    from dedark_yolo_amd import ops
    ve = _ve(dtype)
    for ci, (nc, B) in enumerate((nc, B) for nc in (1, 3, 10, 1000, 1003) for B in (1, 5, 70)):
        z = (torch.from_numpy(np.random.default_rng(700 + ci).normal(0, 3, (B, nc)).astype(np.float32))).to(dtype)
        ld = (nc + ve - 1) // ve * ve + (ve if ci % 2 == 0 else 3)
        _, zv = _rows(z, ld, float("nan"))
        p = ops.cls_softmax(zv)
        assert p.dtype == torch.float32 and tuple(p.shape) == (B, nc)
        ref = cr.softmax(z)
        _within(p, ref, 1e-5 * ref + 1e-30, f"softmax nc={nc} B={B}")
        rowsum = float((p.double().sum(1) - 1).abs().max())
        print(f"softmax nc={nc} B={B}: |row sum - 1| = {rowsum:.3e}, bound {_rowsum_bound(nc):.3e}")
        assert rowsum <= _rowsum_bound(nc), (nc, B, rowsum)
    z = torch.tensor([[80.0, -80.0, 79.0], [-6e4, 6e4, 0.0]]).to(dtype)
    p = ops.cls_softmax(z.cuda())
    assert bool(torch.isfinite(p).all())
    _within(p, cr.softmax(z), 1e-5 * cr.softmax(z) + 1e-30, "softmax at large logits")


# ---------------------------------------------------------------------------------------------------- top-k
def _topk_rows(B, nc, dtype, seed):
    g = np.random.default_rng(seed)
    if dtype == torch.float32:
        return torch.from_numpy(g.normal(0, 1, (B, nc)).astype(np.float32))
    x = torch.from_numpy(g.uniform(-3, 3, (B, nc)).astype(np.float32)).to(dtype)
    plant = torch.tensor([8.0, 7.0, 6.0, 5.0, 4.5, 4.0][:min(nc, 6)]).to(dtype)      # exactly representable, above the rest
    for b in range(B):
        pos = torch.from_numpy(g.permutation(nc)[:len(plant)])
        x[b, pos] = plant
    return x


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_topk_vs_torch_topk_without_ties(dtype):
    from dedark_yolo_amd import ops
    ve = _ve(dtype)
    for ci, nc in enumerate((1, 3, 5, 6, 1000, 1003)):
        B, k = 7, min(nc, 5)
        x = _topk_rows(B, nc, dtype, 800 + ci)
        top = torch.sort(x.float(), 1, descending=True).values[:, :min(nc, k + 1)]
        assert bool((top[:, :-1] > top[:, 1:]).all()), "the k + 1 largest stored values of every row must be distinct"
        ld = (nc + ve - 1) // ve * ve + (ve if ci % 2 == 0 else 3)
        _, xv = _rows(x, ld, float("inf"))               # a read beyond nc would rank first
        idx = ops.cls_topk(xv)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (B, k)
        assert torch.equal(idx.cpu().long(), torch.topk(x.float(), k, dim=1).indices), nc
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_topk_tie_rule(dtype):
    """equal values rank by ascending index (a stable descending sort), NaN below every number, -0 equal to +0"""
    from dedark_yolo_amd import ops
    nan, inf = float("nan"), float("inf")
    rows = [[0.0] * 9,                                                  # an all-zero row
            [1.0, 3.0, 0.5, 3.0, 2.0, 0.0, -1.0, 0.25, 0.75],           # two equal maxima
            [9.0, 8.0, 7.0, 6.0, 5.0, 5.0, 5.0, 1.0, 0.0],              # equal values straddling rank k
            [2.0, 2.0, 2.0, 2.0, 1.0, 2.0, 2.0, 0.0, 2.0],
            [nan, -inf, 1.0, nan, -0.0, 0.0, nan, nan, nan],            # numbers (a real -inf too) before NaN, NaN by index
            [-0.0, 0.0, -0.0, 0.0, -1.0, -1.0, -2.0, -3.0, -4.0]]
    x = torch.tensor(rows).to(dtype)
    want = cr.topk(x, 5)
    assert torch.equal(want[:4], torch.sort(x[:4].float(), dim=1, descending=True, stable=True).indices[:, :5])
    assert want[4].tolist() == [2, 4, 5, 1, 0] and want[5].tolist() == [0, 1, 2, 3, 4]
    got = ops.cls_topk(x.cuda())
    assert torch.equal(got.cpu().long(), want), (got.tolist(), want.tolist())
    six = torch.tensor([[0.0] * 6, [1.0, 3.0, 3.0, 0.0, 2.0, 2.0], [5.0, 4.0, 3.0, 2.0, 1.0, 1.0], [nan, -inf, 1.0, nan, -0.0, 0.0]]).to(dtype)
    hand = [[0, 1, 2, 3, 4], [1, 2, 4, 5, 0], [0, 1, 2, 3, 4], [2, 4, 5, 1, 0]]             # written out by hand: pins the restatement too
    assert cr.topk(six, 5).tolist() == hand and ops.cls_topk(six.cuda()).cpu().tolist() == hand
    wide = torch.zeros(3, 1003).to(dtype)                               # ties across lanes and passes
    wide[1, [1001, 700, 3]] = 1.0
    wide[2, 500:] = 2.0
    assert torch.equal(ops.cls_topk(wide.cuda()).cpu().long(), cr.topk(wide, 5))


# ---------------------------------------------------------------------------------------------------- metrics
@pytest.mark.parametrize("nc", [3, 12])
def test_metrics_vs_reference(nc):
    """g21_cls_metrics through ClassificationValidator.update_metrics / get_stats: the top-k indices, the integer counts and the
    confusion matrix equal the reference's, top-1 / top-5 / fitness within 1e-6 (its float32 mean of 0 / 1 values)."""
    from types import SimpleNamespace
    from dedark_yolo_amd.engine.trainer import get_cfg
    from dedark_yolo_amd.engine.validator import ClassificationValidator
    from dedark_yolo_amd import ops
    g = gold("g21_cls_metrics")
    p = f"nc{nc}_"
    sizes = [int(v) for v in g[p + "batch_sizes"]]
    v = ClassificationValidator(get_cfg())
    v.device = torch.device("cuda")
    v.init_metrics(SimpleNamespace(names={i: str(i) for i in range(nc)}))
    for probs, cls in zip(g[p + "probs"].split(sizes), g[p + "cls"].split(sizes)):
        v.update_metrics(probs.cuda(), dict(cls=cls.cuda()))
    assert torch.equal(ops.cls_topk(g[p + "probs"].cuda()).cpu().long(), g[p + "pred"].long())
    rd = v.get_stats()
    want = cr.metrics(g[p + "pred"].numpy(), g[p + "cls"].numpy(), nc)
    assert v.counts.cpu().tolist() == want["counts"].tolist()
    assert v.confusion_matrix.dtype.kind == "i" and np.array_equal(v.confusion_matrix, g[p + "confusion"].numpy())
    assert list(rd) == [str(s) for s in g[p + "metric_keys"]]
    np.testing.assert_allclose(list(rd.values()), g[p + "metric_values"].numpy(), rtol=0, atol=1e-6)


def test_metrics_skip_labels_outside_the_classes():
    from dedark_yolo_amd import ops
    idx = torch.tensor([[0, 1], [1, 0], [2, 1], [1, 2]], dtype=torch.int32, device="cuda")
    cls = torch.tensor([0, -100, 7, 2], dtype=torch.int64, device="cuda")
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    cm = torch.zeros((3, 3), dtype=torch.int32, device="cuda")
    ops.cls_metrics_update(idx, cls, 3, counts, cm)
    ops.cls_metrics_update(idx, cls, 3, counts, None)
    assert counts.cpu().tolist() == [4, 2, 4] and cm.cpu().tolist() == [[1, 0, 0], [0, 0, 1], [0, 0, 0]]


# ---------------------------------------------------------------------------------------------------- head and tiny models
def test_classify_head_golden():
    """Classify(32, 10) on [3, 32, 3, 3]: train logits, input / parameter gradients under the fixture's cotangent, BN running
    statistics (torch's eps 1e-5 / momentum 0.1), then the eval soft-max, against the reference."""
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn.modules import Classify
    g = gold("g21_cls_head")
    seed = int(g["seed"])
    m = Classify(32, 10)
    load_sd(m, om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed))
    m = m.cuda().train()
    x = g["x"].cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = m(x)
    assert tuple(y.shape) == (3, 10) and y.stride(1) == 1
    (y.float() * rnd(seed + 2, 3, 10, lo=-1, hi=1).cuda()).sum().backward()
    torch.cuda.synchronize()
    close(y.detach().float().cpu(), g["y"], 1e-4, 1e-4, "logits")
    close(x.grad.float().cpu(), g["dx"], 1e-3, 1e-4 * float(g["dx"].abs().max()), "dx")
    named, sd = dict(m.named_parameters()), m.state_dict()
    for k, v in g.items():
        if k.startswith("g:"):
            close(named[k[2:]].grad.cpu(), v, 1e-3, 1e-4 * float(v.abs().max()) + 1e-7, k)
        elif k.startswith("b:"):
            close(sd[k[2:]].cpu(), v, 1e-4, 1e-6, k)
    m.eval()
    with torch.no_grad():
        ye = m(x.detach())
    assert ye.dtype == torch.float32 and tuple(ye.shape) == (3, 10)
    close(ye.cpu(), g["y_eval"], 1e-4, 1e-4 * float(g["y_eval"].abs().max()), "eval probabilities")
    with pytest.raises(NotImplementedError):
        m([x.detach(), x.detach()])
    m.drop.p = 0.2
    with pytest.raises(NotImplementedError):
        m(x.detach())


def _cls_model(seed, nc=10):
    from oracle import model as om
    from parity_helpers import load_sd
    from dedark_yolo_amd.nn.tasks import ClassificationModel
    cfg = load_yaml("cls/yolov8-cls.yaml")
    cfg["scales"]["t"] = TINY
    cfg["scale"] = "t"
    model = ClassificationModel(cfg, nc=nc)
    load_sd(model, om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed))
    return model.cuda()


@pytest.mark.parametrize("S", [64, 96])
def test_tiny_cls_model_step_golden(S):
    """one training forward / loss / backward of a tiny classify model (2x2 and 3x3 head inputs) against the reference's: loss,
    selected gradients, BN running statistics after the step (eps 1e-5 / momentum 0.1, started at (0, 1)), eval probabilities; fuse()
    leaves the probabilities where they were."""
    g = gold("g21_cls_tiny")
    p = f"s{S}_"
    model = _cls_model(int(g[p + "seed"])).train()
    loss, items = model(dict(img=g[p + "img"].cuda(), cls=g[p + "cls"]))
    loss.backward()
    torch.cuda.synchronize()
    print("tiny", S, float(loss.detach()), float(g[p + "loss"]))
    close(float(loss.detach()), g[p + "loss"], 1e-4, 1e-4, "loss vs reference golden")
    close(items.float().cpu(), g[p + "items"], 1e-4, 1e-5, "items vs reference golden")
    named, sd = dict(model.named_parameters()), model.state_dict()
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in named.values() if q.requires_grad)
    for k, v in g.items():
        if not k.startswith(p):
            continue
        k = k[len(p):]
        if k.startswith("gn:"):
            close(named[k[3:]].grad.norm().cpu(), v, 5e-3, 1e-6, k)
        elif k.startswith("g:"):
            close(named[k[2:]].grad.cpu(), v, 5e-3, 5e-3 * float(v.abs().max()), k)
        elif k.startswith("b:"):
            print(k, float((sd[k[2:]].cpu() - v).abs().max()), float(v.abs().max()))
            close(sd[k[2:]].cpu(), v, 1e-4, 1e-5 * float(v.abs().max()) + 1e-6, k)
    model.eval()
    with torch.no_grad():
        probs = model(g[p + "img"].cuda())
    want = g[p + "probs"]
    assert tuple(probs.shape) == (4, 10) and probs.dtype == torch.float32
    err = float((probs.cpu() - want).abs().max()) / float(want.abs().max())
    assert err <= 1e-4, ("eval probabilities", err)
    # fuse(): the eval forward above folded every BatchNorm lazily; drop those caches as an optimizer step does, fold them all up
    # front, and the fused forward launches no fold kernel and gives the same bits (tests/test_gpu_val.py's fuse yardstick)
    from dedark_yolo_amd import _C, ops
    ops.bump_weights_epoch()
    assert not model.is_fused()
    model.fuse()
    assert model.is_fused()
    calls, orig = [], _C.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)
    ops.call = spy
    try:
        with torch.no_grad():
            fused = model(g[p + "img"].cuda())
    finally:
        ops.call = orig
    assert calls and not any(c.startswith("dy_bn_fold_eval") for c in calls)
    assert torch.equal(fused, probs), float((fused - probs).abs().max())


def _tiny_step(g, p, dtype, emulate=None):
    import dedark_yolo_amd as dy
    from dedark_yolo_amd import ops
    dy.set_compute_dtype(dtype)
    ops.set_storage_emulation(emulate)
    try:
        model = _cls_model(int(g[p + "seed"])).train()
        loss, _ = model(dict(img=g[p + "img"].cuda(), cls=g[p + "cls"]))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.set_storage_emulation(None)
        dy.set_compute_dtype(torch.float32)
    return model, float(loss.detach())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_tiny_cls_model_low_precision(dtype):
    """a 16-bit step of the tiny model against the fp32 HIP path: the loss within 5 %, or within 2.5x of how far the f32 kernels with
    storage rounded to that type (ops.set_storage_emulation, the project's low-precision yardstick) move it; finite gradients."""
    g = gold("g21_cls_tiny")
    p = "s96_"
    model, loss = _tiny_step(g, p, dtype)
    assert np.isfinite(loss)
    assert all(bool(torch.isfinite(q.grad).all()) for q in model.parameters() if q.requires_grad)
    _, loss_f = _tiny_step(g, p, torch.float32)
    _, loss_e = _tiny_step(g, p, torch.float32, dtype)
    msg = dict(low=loss, f32=loss_f, emulated=loss_e)
    print(msg)
    assert abs(loss_f - float(g[p + "loss"])) <= 1e-4 * abs(float(g[p + "loss"])) + 1e-4, msg
    assert abs(loss - loss_f) <= max(5e-2 * abs(loss_f), 2.5 * abs(loss_e - loss_f)), msg


# ---------------------------------------------------------------------------------------------------- trainer, validator, predict
def _batch(seed, B=4, S=64, nc=10, uint8=True):
    g = np.random.default_rng(seed)
    img = torch.from_numpy(g.integers(0, 256, (B, 3, S, S)).astype(np.uint8))
    return dict(img=img if uint8 else img.float() / 255, cls=torch.from_numpy(g.integers(0, nc, B).astype(np.int64)))


def _trainer(dtype="fp32", optimizer="SGD", **kw):
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    from dedark_yolo_amd.nn.tasks import ClassificationModel
    cfg = load_yaml("cls/yolov8-cls.yaml")
    cfg["scales"]["t"] = TINY
    cfg["scale"] = "t"
    torch.manual_seed(3)
    tr = DetectionTrainer(get_cfg(dict(model="tiny", dtype=dtype, optimizer=optimizer, batch=64, imgsz=64, deterministic=True,
                                       lowlight_FLAG=True, dedark_FLAG=True, **kw)))
    tr.setup(ClassificationModel(cfg, nc=10), total_iterations=100)
    return tr


@pytest.mark.parametrize("dtype,optimizer", [("fp32", "SGD"), ("fp32", "AdamW"), ("fp16", "SGD"), ("bf16", "auto")])
def test_trainer_two_steps(dtype, optimizer):
    """two trainer steps: one finite loss column, parameters move, no clean_img / recovery term in the batch, a float image passes
    through; fp16 carries the loss scale through the criterion's grad_out; optimizer auto sees nc = 10 (Classify has no .nc)."""
    tr = _trainer(dtype, optimizer)
    if optimizer == "auto":
        assert tr.opt_name == "AdamW" and tr.lr0 == round(0.002 * 5 / (4 + 10), 6)
    p0 = tr.flat.p.clone()
    for i in range(2):
        b = tr.preprocess_batch(_batch(20 + i, uint8=(i == 0)))
        assert set(b) == {"img", "cls"} and b["img"].dtype == torch.float32 and b["img"].is_cuda and b["cls"].dtype == torch.int64
        assert 0.0 <= float(b["img"].min()) and float(b["img"].max()) <= 1.0
        loss, items = tr.train_step(_batch(20 + i, uint8=(i == 0)), [0.01] * 3, 0.9)
        assert items.numel() == 1 and np.isfinite(float(items)) and float(loss) == float(items) > 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.flat.p).all())
    skipped = float(tr.loss_scale[2]) if dtype == "fp16" else 0.0       # an overflowing fp16 step is skipped and halves the scale
    assert float((tr.flat.p - p0).abs().max()) > 0 or skipped == 2.0
    if dtype == "fp16":
        assert float(tr.loss_scale[0]) == 65536.0 * 0.5 ** skipped
    with pytest.raises(ValueError):
        tr.preprocess_batch(dict(img=_batch(1)["img"], cls=torch.tensor([0, 10, 1, 2])))


def test_trainer_rejects_dropout():
    with pytest.raises(NotImplementedError):
        _trainer(dropout=0.1)


def test_trainer_save_resume_validate(tmp_path):
    """three steps, save_model (the reference's pickle layout), resume_training into fresh trainers: the half-rounded parameters, and
    the same next step from both; validate() reports the two accuracies and takes fitness from the metrics."""
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint
    tr = _trainer()
    for i in range(3):
        tr.train_step(_batch(40 + i), [0.01] * 3, 0.9)
    last = tr.save_model(str(tmp_path), epoch=3, fitness=None)
    ck = load_checkpoint(last)
    assert list(ck.model_sd) == list(tr.model.state_dict()) and ck.source == "reference-pickle"
    nxt = []
    for _ in range(2):
        t2 = _trainer()
        assert t2.resume_training(last) == 4
        torch.cuda.synchronize()
        assert float((t2.flat.p - tr.flat.p.half().float()).abs().max()) == 0.0
        loss, _ = t2.train_step(_batch(50), [0.01] * 3, 0.9)
        nxt.append((float(loss), t2.flat.p.clone()))
    # deterministic=True: two trainers resumed from the same file take the identical next step, bit for bit
    assert np.isfinite(nxt[0][0]) and nxt[0][0] == nxt[1][0], (nxt[0][0], nxt[1][0])
    assert torch.equal(nxt[0][1], nxt[1][1]), int((nxt[0][1] != nxt[1][1]).sum())
    metrics, fit = t2.validate([_batch(60, B=16), _batch(61, B=5)])
    assert set(metrics) == {"metrics/accuracy_top1", "metrics/accuracy_top5", "fitness"}
    assert 0.0 <= metrics["metrics/accuracy_top1"] <= metrics["metrics/accuracy_top5"] <= 1.0
    assert abs(fit - (metrics["metrics/accuracy_top1"] + metrics["metrics/accuracy_top5"]) / 2) < 1e-12
    assert t2.model.training


def test_validator_counts_a_perfect_and_a_wrong_model():
    """the whole validator loop on a model whose head bias decides the class: every image gets class 3"""
    from dedark_yolo_amd.engine.trainer import get_cfg
    from dedark_yolo_amd.engine.validator import ClassificationValidator
    model = _cls_model(5)
    with torch.no_grad():
        model.model[-1].linear.weight.zero_()
        model.model[-1].linear.bias.copy_(torch.tensor([0.0, 1.0, 2.0, 9.0, 3.0, 4.0, 5.0, -1.0, -2.0, -3.0]))
    b1, b2 = _batch(70, B=6), _batch(71, B=3, uint8=False)
    b1["cls"] = torch.tensor([3, 3, 6, 5, 0, 3])          # top-5 = {3, 6, 5, 4, 2}
    b2["cls"] = torch.tensor([4, 1, 3])
    v = ClassificationValidator(get_cfg())
    rd = v(model, [b1, b2])
    assert rd["metrics/accuracy_top1"] == pytest.approx(4 / 9) and rd["metrics/accuracy_top5"] == pytest.approx(7 / 9)
    assert rd["fitness"] == pytest.approx((4 / 9 + 7 / 9) / 2)
    cm = v.confusion_matrix
    assert cm.shape == (10, 10) and int(cm.sum()) == 9 and cm[3].tolist() == [1, 1, 0, 4, 1, 1, 1, 0, 0, 0]


def test_predict_returns_probs():
    from dedark_yolo_amd.engine.model import YOLO
    from dedark_yolo_amd.engine.results import Probs
    y = YOLO("yolov8n-cls.yaml")
    y.model = _cls_model(9)
    y.model.train()
    b = _batch(80)
    res = y.predict(b["img"], orig_shapes=[(100, 80)] * 4)
    assert y.model.training and len(res) == 4
    y.model.eval()
    xf = b["img"].float() / 255
    with torch.no_grad():
        want = y.model(xf.cuda())
    res_f = y.predict(xf)
    for i, r in enumerate(res):
        assert isinstance(r.probs, Probs) and r.boxes is None and len(r) == 10 and r.orig_shape == (100, 80)
        assert torch.equal(res_f[i].probs.data, want[i])                 # a float image passes through as it is
        close(r.probs.data.cpu(), want[i].cpu(), 1e-5, 1e-7, "uint8 image: / 255 on the device")
        got = r.probs.data.cpu()
        order = torch.sort(got, descending=True, stable=True).indices[:5].tolist()
        assert r.probs.top5 == order and r.probs.top1 == order[0]
        assert float(r.probs.top1conf) == float(got[order[0]]) and torch.equal(r.probs.top5conf.cpu(), got[order])
        assert abs(float(got.sum()) - 1.0) < 1e-5


def test_product_eval_equals_the_reference_running_our_checkpoint():
    """g21_cls_interop: the reference loaded a tiny last.pt this package wrote (EMA weights, rng_fill seed 2182, half) and ran eval;
    the product on the same half-rounded weights gives the same probabilities."""
    from oracle import model as om
    from parity_helpers import load_sd
    g = gold("g21_cls_interop")
    model = _cls_model(1)
    ema = om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, 2182)
    load_sd(model, {k: (v.half().float() if v.is_floating_point() else v) for k, v in ema.items()})
    model = model.cuda().eval()
    model.fuse()
    x = rnd(int(g["x_seed"]), 4, 3, 64, 64).pow(2.0)
    with torch.no_grad():
        y = model(x.cuda())
    want = g["y"]
    assert tuple(y.shape) == tuple(want.shape) == (4, 10)
    err = float((y.cpu() - want).abs().max()) / float(want.abs().max())
    assert err <= 1e-4, err


def test_reference_written_checkpoint_predicts():
    import os
    from util import GOLD
    from dedark_yolo_amd.engine.model import YOLO
    y = YOLO(os.path.join(GOLD, "g21_ref_cls_last.pt"))
    y.model.cuda()
    res = y.predict(_batch(90)["img"])
    assert len(res) == 4 and all(len(r.probs) == 10 and abs(float(r.probs.data.sum()) - 1) < 1e-5 for r in res)
