"""csrc/valmatch.hip on the GPU: dy_val_box_match against the host path (utils/ops.scale_boxes, metrics.box_iou,
engine/validator.match_predictions, the numpy ConfusionMatrix.process_batch) bit for bit, tests/golden/g27_valmatch.npz (the reference's
`correct` and confusion matrices) through the validator, dy_val_iou_match against match_from_iou, the accumulation of the confusion
matrix over batches, and DetectionValidator end to end (metrics, confusion matrix, print_results, save_txt / save_json)."""
import json
import logging
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import valmatch_ref as vr
from util import gold, load_yaml

pytestmark = pytest.mark.gpu
IOUV = torch.linspace(0.5, 0.95, 10)
TINY = (0.33, 0.125, 1024)


# ------------------------------------------------------------------------------------------------ batches and their host results
def _grid_boxes(gen, k, S):
    """k xyxy boxes on a 4-pixel grid inside S x S, sizes 8..40"""
    wh = gen.choice([8, 12, 16, 20, 40], (k, 2))
    xy = np.stack([gen.integers(0, (S - wh[:, 0]) // 4 + 1) * 4, gen.integers(0, (S - wh[:, 1]) // 4 + 1) * 4], 1)
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def _grid_image(gen, m, n, nc, S):
    """labels [m, 5] (cls, xyxy px) and detections [n, 6]: grid boxes, duplicates, and crops of 20-wide labels to 9 / 10 / 15 columns
    (IoU exactly 0.45 / 0.5 / 0.75); confidences on both sides of 0.25 and on it"""
    lab = np.concatenate([gen.integers(0, nc, (m, 1)).astype(np.float32), _grid_boxes(gen, m, S)], 1)
    det = np.concatenate([_grid_boxes(gen, n, S), gen.choice([0.05, 0.25, 0.26, 0.6, 0.9], (n, 1)), gen.integers(0, nc, (n, 1))], 1).astype(np.float32)
    for j in range(n):
        if m and j % 3 != 2:
            i = int(gen.integers(0, m))
            det[j, :4], det[j, 5] = lab[i, 1:], lab[i, 0] if j % 5 else (lab[i, 0] + 1) % nc
            if j % 3 == 1:
                w = lab[i, 3] - lab[i, 1]
                det[j, 2] = det[j, 0] + w * gen.choice([0.45, 0.5, 0.75])      # w = 20 or 40: whole pixels
    return lab, det[np.argsort(-det[:, 4], kind="stable")]


def _pack(images, S_hw, max_det, ori=None, ratio_pad=None, device="cuda"):
    """images: (lab [m, 5] with xyxy in input pixels, det [n, 6]) -> det [B, max_det, 6], cnt, and the validator's batch dict"""
    H, W = S_hw
    B = len(images)
    det = torch.zeros((B, max_det, 6), dtype=torch.float32)
    bi, cls, bb = [], [], []
    for b, (lab, d) in enumerate(images):
        det[b, :len(d)] = torch.from_numpy(d)
        x1, y1, x2, y2 = (lab[:, k].astype(np.float64) for k in range(1, 5))
        bb.append(np.stack([(x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H], 1))
        cls.append(lab[:, 0])
        bi += [b] * len(lab)
    batch = dict(img=torch.zeros(B, 3, H, W), batch_idx=torch.tensor(bi, dtype=torch.float32),
                 cls=torch.from_numpy(np.concatenate(cls).astype(np.float32)).view(-1, 1),
                 bboxes=torch.from_numpy(np.concatenate(bb).astype(np.float32)), ori_shape=ori or [(H, W)] * B)
    if ratio_pad is not None:
        batch["ratio_pad"] = ratio_pad
    cnt = torch.tensor([len(d) for _, d in images], dtype=torch.int32)
    return det.to(device), cnt.to(device), batch


def _host(det, cnt, batch, nc, single_cls=False):
    """the parent's per-image host path: scale_boxes, box_iou, match_predictions, plus the numpy ConfusionMatrix"""
    from dedark_yolo_amd.engine.validator import match_predictions
    from dedark_yolo_amd.utils import ops as uops
    from dedark_yolo_amd.utils.metrics import ConfusionMatrix
    det, cnt = det.cpu(), cnt.cpu().tolist()
    H, W = batch["img"].shape[2:]
    cm = ConfusionMatrix(nc=nc)
    B, max_det = det.shape[:2]
    correct, predn = torch.zeros(B, max_det, 10, dtype=torch.bool), torch.zeros(B, max_det, 4)
    tboxes = []
    for si in range(B):
        idx = batch["batch_idx"] == si
        cls, bbox = batch["cls"][idx], batch["bboxes"][idx]
        shape = batch["ori_shape"][si]
        rp = batch["ratio_pad"][si] if "ratio_pad" in batch else None
        tbox = uops.xywh2xyxy(bbox) * torch.tensor((W, H, W, H), dtype=torch.float32)
        uops.scale_boxes((H, W), tbox, shape, ratio_pad=rp)
        tboxes.append(tbox)
        n = cnt[si]
        pred = det[si, :n].clone()
        if single_cls:
            pred[:, 5] = 0
        uops.scale_boxes((H, W), pred[:, :4], shape, ratio_pad=rp)
        predn[si, :n] = pred[:, :4]
        labelsn = torch.cat((cls, tbox), 1)
        if n == 0:
            if len(cls):
                cm.process_batch(None, cls.squeeze(-1))
            continue
        if len(cls):
            correct[si, :n] = match_predictions(pred, labelsn, IOUV)
            cm.process_batch(pred, labelsn)
    return correct, predn, torch.cat(tboxes), cm.matrix


def _device(det, cnt, batch, nc, single_cls=False):
    from dedark_yolo_amd import ops as kops
    from dedark_yolo_amd.engine.validator import scale_record
    B = det.shape[0]
    H, W = batch["img"].shape[2:]
    bi = batch["batch_idx"]
    loff = torch.searchsorted(bi.contiguous(), torch.arange(B + 1, dtype=torch.float32)).to(torch.int32)
    rec = torch.tensor([scale_record((H, W), batch["ori_shape"][si], batch["ratio_pad"][si] if "ratio_pad" in batch else None)
                        for si in range(B)], dtype=torch.float32)
    conf = torch.zeros((nc + 1, nc + 1), dtype=torch.int32, device="cuda")
    out = kops.val_box_match(det, cnt, batch["cls"].view(-1).cuda(), batch["bboxes"].cuda(), loff.cuda(), (H, W), rec.cuda(), IOUV.cuda(),
                             single_cls, conf)
    torch.cuda.synchronize()
    return (*(t.cpu() for t in out), conf.cpu())


@pytest.fixture(scope="module")
def grid_batch():
    gen = np.random.default_rng(2710)
    S, nc = 128, 4
    sizes = [(0, 40), (1, 1), (63, 0), (64, 700), (65, 40), (300, 700)]            # (N, M)
    det, cnt, batch = _pack([_grid_image(gen, m, n, nc, S) for n, m in sizes], (S, S), 300)
    return det, cnt, batch, nc, _host(det, cnt, batch, nc)


def test_box_match_on_an_integer_grid_equals_the_host_path(grid_batch):
    """B = 6, N in {0, 1, 63, 64, 65, 300}, M in {0, 1, 40, 700} (more labels than a workgroup has threads); IoU values exactly on
    0.45 / 0.5 / 0.75 and many exact ties.  Integer outputs and f32 boxes must be equal, not close: the kernel does the host's f32
    operations in the host's order."""
    det, cnt, batch, nc, (want_c, want_p, want_t, want_m) = grid_batch
    # the case holds what it claims
    lab0 = want_t[(batch["batch_idx"] == 5)]
    iou = vr.box_iou(lab0.numpy(), want_p[5].numpy())
    for v in (0.45, 0.5, 0.75):
        assert (iou == np.float32(v)).any(), v
    cand = iou[iou > np.float32(0.45)]
    assert len(np.unique(cand)) < len(cand) / 4
    correct, predn, tboxn, conf = _device(det, cnt, batch, nc)
    assert correct.dtype == torch.uint8 and tuple(correct.shape) == (6, 300, 10)
    assert torch.equal(predn, want_p) and torch.equal(tboxn, want_t)
    assert torch.equal(correct.bool(), want_c), int((correct.bool() != want_c).sum())
    assert want_c.any() and not want_c[5].all() and want_c[..., 9].sum() < want_c[..., 0].sum()
    assert conf.dtype == torch.int32 and np.array_equal(conf.numpy(), want_m), np.abs(conf.numpy() - want_m).sum()
    assert want_m[nc].sum() > 0 and want_m[:, nc].sum() > 0 and np.trace(want_m) > 0
    # two runs: identical bytes
    again = _device(det, cnt, batch, nc)
    for a, b in zip((correct, predn, tboxn, conf), again):
        assert a.numpy().tobytes() == b.numpy().tobytes()


def test_box_match_random_boxes_single_cls_letterbox():
    """random (non-grid) boxes, single_cls, a rectangular 96 x 160 input with real letterbox pads from three original shapes"""
    gen = np.random.default_rng(2711)
    H, W, nc = 96, 160, 5
    ori = [(480, 800), (300, 640), (427, 500)]
    rp = []
    for h0, w0 in ori:
        gain = min(H / h0, W / w0)
        rp.append(((gain, gain), ((W - w0 * gain) / 2, (H - h0 * gain) / 2)))
    images = []
    for n, m in ((37, 9), (0, 3), (130, 21)):
        lab = np.concatenate([np.zeros((m, 1)), gen.uniform(0, 0.6, (m, 2)) * [W, H], np.zeros((m, 2))], 1)
        lab[:, 3:] = lab[:, 1:3] + gen.uniform(0.1, 0.4, (m, 2)) * [W, H]
        d = np.zeros((n, 6))
        for j in range(n):
            d[j, :4] = lab[j % m, 1:] + gen.normal(0, 2.0 + j // m, 4)
        d[:, 4], d[:, 5] = gen.uniform(0.02, 1, n), gen.integers(0, nc, n)
        d[::7, :4] += 60                                                   # some leave the image: the clamp works
        images.append((lab.astype(np.float32), d[np.argsort(-d[:, 4])].astype(np.float32)))
    det, cnt, batch = _pack(images, (H, W), 130, ori=ori, ratio_pad=rp)
    want_c, want_p, want_t, want_m = _host(det, cnt, batch, nc, single_cls=True)
    correct, predn, tboxn, conf = _device(det, cnt, batch, nc, single_cls=True)
    assert torch.equal(predn, want_p) and torch.equal(tboxn, want_t)
    assert (want_p == 0).any() and (want_p[2, :, 2] == 500).any()              # both sides of the clamp
    assert torch.equal(correct.bool(), want_c) and want_c.any()
    assert np.array_equal(conf.numpy(), want_m) and want_m[0, 0] > 0 and want_m[1:nc].sum() == 0


def test_box_match_without_a_confusion_matrix_and_argument_checks():
    from dedark_yolo_amd import ops as kops
    gen = np.random.default_rng(2712)
    det, cnt, batch = _pack([_grid_image(gen, 5, 9, 3, 64)], (64, 64), 9)
    want_c = _host(det, cnt, batch, 3)[0]
    loff = torch.tensor([0, 5], dtype=torch.int32).cuda()
    rec = torch.tensor([[1, 0, 0, 64, 64]], dtype=torch.float32).cuda()
    correct, _, _ = kops.val_box_match(det, cnt, batch["cls"].view(-1).cuda(), batch["bboxes"].cuda(), loff, (64, 64), rec, IOUV.cuda())
    assert torch.equal(correct.cpu().bool(), want_c)
    with pytest.raises(RuntimeError, match="iouv"):
        kops.val_box_match(det, cnt, batch["cls"].view(-1).cuda(), batch["bboxes"].cuda(), loff, (64, 64), rec, torch.zeros(17).cuda())


def test_per_detection_state_in_the_global_workspace():
    """max_det = 2100: the per-detection state (20 bytes each) no longer fits the 40 KiB of LDS the kernels use, the wrappers pass a
    global workspace.  One image fills all 2100 rows.  Both entry points against the host functions."""
    from dedark_yolo_amd import ops as kops
    from dedark_yolo_amd.engine.validator import match_from_iou
    assert kops._val_match_ws(2, 2048, "cpu") is None and kops._val_match_ws(2, 2100, "cpu").numel() == 2 * 2100 * 5
    gen = np.random.default_rng(2716)
    nc = 3
    det, cnt, batch = _pack([_grid_image(gen, 5, 70, nc, 128), _grid_image(gen, 30, 2100, nc, 128)], (128, 128), 2100)
    want_c, want_p, want_t, want_m = _host(det, cnt, batch, nc)
    correct, predn, tboxn, conf = _device(det, cnt, batch, nc)
    assert torch.equal(predn, want_p) and torch.equal(tboxn, want_t)
    assert torch.equal(correct.bool(), want_c) and want_c[1].any() and not correct[0, 70:].any()
    assert np.array_equal(conf.numpy(), want_m) and np.trace(want_m) > 0
    mats = [torch.from_numpy(vr.box_iou(want_t[:5].numpy(), want_p[0, :70].numpy())), torch.from_numpy(vr.box_iou(want_t[5:].numpy(), want_p[1].numpy()))]
    got = kops.val_iou_match(torch.cat([m.reshape(-1) for m in mats]).cuda(), torch.tensor([0, 5 * 70]).cuda(), det, cnt,
                             batch["cls"].view(-1).cuda(), torch.tensor([0, 5, 35], dtype=torch.int32).cuda(), IOUV.cuda()).cpu()
    for b, n in enumerate((70, 2100)):
        lab = batch["cls"].view(-1)[:5] if b == 0 else batch["cls"].view(-1)[5:]
        assert torch.equal(got[b, :n].bool(), match_from_iou(mats[b].numpy(), lab, det[b, :n, 5].cpu(), IOUV))
    assert torch.equal(got.bool(), want_c)                    # the box IoU fed back in: the same `correct` as dy_val_box_match


# ------------------------------------------------------------------------------------------------ g27 through the validator
def _validator(nc, cls=None, **over):
    from dedark_yolo_amd.engine.trainer import get_cfg
    from dedark_yolo_amd.engine.validator import DetectionValidator
    v = (cls or DetectionValidator)(get_cfg(over))
    v.device = torch.device("cuda")
    v.init_metrics(SimpleNamespace(model=[SimpleNamespace(nc=nc)], names={i: f"c{i}" for i in range(nc)}))
    return v


@pytest.fixture(scope="module")
def sets():
    return vr.fixture_sets(gold("g27_valmatch"))


def test_reference_fixture_through_the_kernel(sets):
    """g27: the reference's `correct` rows, stats columns and confusion matrices, exactly"""
    for s in sets:
        v = _validator(s["nc"])
        assert not v._confusion.any()
        v.update_metrics([p.cuda() for p in s["preds"]], s["batch"])
        assert v.seen == s["seen"]
        stats = [torch.cat(x, 0) for x in zip(*v.stats)]
        assert torch.equal(stats[0], s["correct"].bool()), int((stats[0] != s["correct"].bool()).sum())
        for got, want in zip(stats[1:], (s["conf"], s["pcls"], s["tcls"])):
            assert torch.equal(got.float(), want.float())
        v.get_stats()
        assert np.array_equal(v.confusion_matrix.matrix, s["matrix"].numpy()) and v.confusion_matrix.matrix.dtype == np.float64
        assert v.metrics.confusion_matrix is v.confusion_matrix
        tp, fp = v.confusion_matrix.tp_fp()
        assert np.array_equal(tp, s["tp"].numpy()) and np.array_equal(fp, s["fp"].numpy())
        assert np.array_equal(v.nt_per_class, np.bincount(s["tcls"].numpy().astype(int), minlength=s["nc"]))


def test_confusion_matrix_accumulates_in_any_order(sets):
    """the same two batches fed in either order give the same matrix, the sum of theirs; a fresh validator starts from zeros"""
    a, b = sets[1], sets[2]
    mats = []
    for order in ((a, b), (b, a)):
        v = _validator(80)
        for s in order:
            v.update_metrics([p.cuda() for p in s["preds"]], s["batch"])
        v.get_stats()
        mats.append(v.confusion_matrix.matrix)
    assert np.array_equal(mats[0], mats[1]) and np.array_equal(mats[0], a["matrix"].numpy() + b["matrix"].numpy())
    v = _validator(80)
    rd = v.get_stats()
    assert not v.confusion_matrix.matrix.any() and v.confusion_matrix.matrix.shape == (81, 81) and not v.nt_per_class.any()
    assert all(val == 0 for val in rd.values())


# ------------------------------------------------------------------------------------------------ dy_val_iou_match
def _iou_case(gen, sizes, nc, ties):
    mats, lcls = [], []
    nmax = max([n for _, n in sizes] + [1])
    det = torch.zeros((len(sizes), nmax, 7), dtype=torch.float32)          # a wider row than 6: the stride is honoured
    for b, (m, n) in enumerate(sizes):
        iou = gen.choice([0.0, 0.3, 0.5, 0.55, 0.75, 0.95, 1.0], (m, n)) if ties else gen.random((m, n))
        mats.append(torch.from_numpy(iou.astype(np.float32)))
        lcls.append(torch.from_numpy(gen.integers(0, nc, m).astype(np.float32)))
        det[b, :n, 5] = torch.from_numpy(gen.integers(0, nc, n).astype(np.float32))
    return mats, lcls, det


@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
@pytest.mark.parametrize("sizes", [[(0, 40), (1, 1), (40, 0), (700, 64), (40, 65), (700, 300)], [(0, 5), (3, 0), (0, 0)]],
                         ids=["mixed", "all-empty"])
def test_iou_match_equals_match_from_iou(sizes, ties):
    """packed [M_i, N_i] matrices (M_i = 0, N_i = 0 and a batch where every matrix is empty included) against the host loop"""
    from dedark_yolo_amd import ops as kops
    from dedark_yolo_amd.engine.validator import match_from_iou
    gen = np.random.default_rng(2713 + int(ties))
    nc = 3
    mats, lcls, det = _iou_case(gen, sizes, nc, ties)
    numel = [m.numel() for m in mats]
    moff = torch.tensor([sum(numel[:b]) for b in range(len(mats))], dtype=torch.int64)
    flat = torch.cat([m.reshape(-1) for m in mats]) if sum(numel) else torch.zeros(1)
    loff = torch.tensor([0] + list(np.cumsum([m for m, _ in sizes])), dtype=torch.int32)
    cnt = torch.tensor([n for _, n in sizes], dtype=torch.int32)
    got = kops.val_iou_match(flat.cuda(), moff.cuda(), det.cuda(), cnt.cuda(), torch.cat(lcls).cuda(), loff.cuda(), IOUV.cuda())
    torch.cuda.synchronize()
    got = got.cpu()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(sizes), det.shape[1], 10)
    total = 0
    for b, (m, n) in enumerate(sizes):
        want = match_from_iou(mats[b].numpy(), lcls[b], det[b, :n, 5], IOUV)
        assert torch.equal(got[b, :n].bool(), want), (b, int((got[b, :n].bool() != want).sum()))
        assert not got[b, n:].any()
        total += int(want.sum())
    assert (total > 0) == (sum(numel) > 0)


# ------------------------------------------------------------------------------------------------ end to end
def _tiny_model(seed, nc):
    from oracle import model as om
    from parity_helpers import HYP, load_sd
    from dedark_yolo_amd.nn.tasks import DetectionModel
    cfg = load_yaml("yolov8ori.yaml")
    cfg["scales"]["t"] = list(TINY)
    cfg["scale"] = "t"
    model = DetectionModel(dict(cfg), ch=3, nc=nc)
    model.args = HYP
    load_sd(model, om.rng_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed))
    return model.cuda().eval()


def test_detection_validator_end_to_end(tmp_path, caplog):
    """tiny yolov8ori graph, fixed random weights, 64 x 64, two batches of 4, conf = 0.001: the validator's metrics, stats and
    confusion matrix equal those built by the host functions from the SAME NMS outputs (recorded from the validator's own
    postprocess); print_results logs the `all` row and one row per class; save_txt / save_json write the host formatting of predn."""
    import dedark_yolo_amd as dy
    from dedark_yolo_amd.engine.trainer import get_cfg
    from dedark_yolo_amd.engine.validator import DetectionValidator, match_predictions, pred_to_json, save_one_txt
    from dedark_yolo_amd.utils import ops as uops
    from dedark_yolo_amd.utils.metrics import ConfusionMatrix, DetMetrics
    dy.set_compute_dtype(torch.float32)
    S, B, nc = 64, 4, 3
    model = _tiny_model(2714, nc)
    gen = np.random.default_rng(2715)
    loader = []
    for k in range(2):
        img = torch.from_numpy((gen.random((B, 3, S, S)) * 255).astype(np.uint8))
        with torch.no_grad():
            dets = uops.non_max_suppression(model((img.float() / 255).cuda()), 0.001, 0.7, multi_label=True, max_det=300)
        bi, cls, bb = [], [], []
        for b, d in enumerate(dets):                          # labels: some of the model's own detections, so that the metrics are not zero
            for row in d[1:12:4].cpu():
                x1, y1, x2, y2 = (float(v) for v in row[:4].clamp(0, S))
                bi.append(b)
                cls.append(float(row[5]))
                bb.append([(x1 + x2) / 2 / S, (y1 + y2) / 2 / S, (x2 - x1) / S, (y2 - y1) / S])
        loader.append(dict(img=img, batch_idx=torch.tensor(bi, dtype=torch.float32), cls=torch.tensor(cls, dtype=torch.float32).view(-1, 1),
                           bboxes=torch.tensor(bb, dtype=torch.float32), ori_shape=[(S + 16 * k, S)] * B,
                           im_file=[f"/data/{'%012d' % (4 * k + b) if b % 2 else 'img_%d' % (4 * k + b)}.jpg" for b in range(B)]))
    v = DetectionValidator(get_cfg(dict(conf=0.001, iou=0.7, save_txt=True, save_conf=True, save_json=True, save_dir=str(tmp_path / "run"))))
    recorded = []
    post = v.postprocess
    v.postprocess = lambda preds: (recorded.append(post(preds)), recorded[-1])[1]
    got = v(model, loader)
    assert len(recorded) == 2 and all(tuple(out.shape) == (B, 300, 6) and out.is_cuda and cnt.is_cuda for out, cnt in recorded)
    # the host construction on the recorded NMS outputs
    stats, cm, files, records = [], ConfusionMatrix(nc=nc), {}, []
    for (out, cnt), batch in zip(recorded, loader):
        out, cnt = out.cpu(), cnt.cpu().tolist()
        for si in range(B):
            idx = batch["batch_idx"] == si
            c, bx = batch["cls"][idx], batch["bboxes"][idx]
            shape = batch["ori_shape"][si]
            d = out[si, :cnt[si]]
            if cnt[si] == 0:
                if len(c):
                    stats.append((torch.zeros(0, 10, dtype=torch.bool), torch.zeros(0), torch.zeros(0), c.squeeze(-1)))
                    cm.process_batch(None, c.squeeze(-1))
                continue
            dn = d.clone()
            uops.scale_boxes((S, S), dn[:, :4], shape)
            correct = torch.zeros(len(d), 10, dtype=torch.bool)
            if len(c):
                tbox = uops.xywh2xyxy(bx) * torch.tensor((S, S, S, S), dtype=torch.float32)
                uops.scale_boxes((S, S), tbox, shape)
                labelsn = torch.cat((c, tbox), 1)
                correct = match_predictions(dn, labelsn, IOUV)
                cm.process_batch(dn, labelsn)
            stats.append((correct, d[:, 4], d[:, 5], c.squeeze(-1)))
            stem = batch["im_file"][si].split("/")[-1][:-4]
            f = tmp_path / f"want_{stem}.txt"
            save_one_txt(dn, True, shape, f)
            files[stem] = f.read_text()
            records += pred_to_json(dn, batch["im_file"][si])
    assert sum(len(s[1]) for s in stats) > 200, "the test is vacuous without detections"
    assert len(v.stats) == len(stats) and v.seen == 2 * B
    for a, b in zip(v.stats, stats):
        assert all(torch.equal(x, y.to(x.dtype)) for x, y in zip(a, b))
    m = DetMetrics(names=v.names)
    m.process(*[torch.cat(x, 0).numpy() for x in zip(*stats)])
    want = {k: float(val) for k, val in m.results_dict.items()}
    assert got == want and got["metrics/mAP50(B)"] > 0.05, (got, want)
    assert np.array_equal(v.confusion_matrix.matrix, cm.matrix) and np.trace(cm.matrix) > 0 and cm.matrix[:, nc].sum() > 0
    assert np.array_equal(v.nt_per_class, np.bincount(torch.cat([b["cls"].view(-1) for b in loader]).numpy().astype(int), minlength=nc))
    # print_results: the `all` row and one row per class
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="dedark_yolo_amd"):
        v.print_results()
    rows = [r.getMessage() for r in caplog.records]
    assert len(rows) == 1 + len(v.metrics.ap_class_index) and len(v.metrics.ap_class_index) > 1
    assert rows[0].split()[:3] == ["all", str(2 * B), str(int(v.nt_per_class.sum()))] and rows[1].split()[0] == v.names[v.metrics.ap_class_index[0]]
    # saved predictions
    for stem, text in files.items():
        assert (tmp_path / "run" / "labels" / f"{stem}.txt").read_text() == text
    assert len(list((tmp_path / "run" / "labels").iterdir())) == len(files)
    saved = json.loads((tmp_path / "run" / "predictions.json").read_text())
    assert saved == records and {type(r["image_id"]) for r in saved} == {int, str}
    # YOLO.val returns the same dict of floats and keeps its validator
    from dedark_yolo_amd.engine.model import YOLO
    yolo = YOLO("yolov8nori.yaml")
    yolo.model = model
    assert yolo.validator is None
    assert yolo.val(loader, conf=0.001, iou=0.7) == got
    assert np.array_equal(yolo.validator.confusion_matrix.matrix, cm.matrix) and np.array_equal(yolo.validator.nt_per_class, v.nt_per_class)
    # without a save_dir or the file names the request is an error, not a silent no-op
    v2 = DetectionValidator(get_cfg(dict(conf=0.001, iou=0.7, save_txt=True)))
    with pytest.raises(ValueError, match="save_dir"):
        v2(model, loader[:1])
