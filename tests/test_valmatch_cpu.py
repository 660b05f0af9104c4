"""Validation matching and the detection confusion matrix on the CPU (no GPU needed): utils/metrics.ConfusionMatrix.process_batch
(the host statement of the rule csrc/valmatch.hip applies) against the reference's matrices of tests/golden/g27_valmatch.npz, its
quirks and its tie rule; the f32 numpy statement of the box scaling, the IoU and the kernel's form of the matching (valmatch_ref.py)
against utils/ops.scale_boxes + metrics.box_iou bit for bit and against the reference's `_process_batch`; the save_txt lines and the
predictions.json records."""
import json
import logging

import numpy as np
import pytest
import torch

import valmatch_ref as vr
from util import gold

IOUV = torch.linspace(0.5, 0.95, 10)


@pytest.fixture(scope="module")
def sets():
    return vr.fixture_sets(gold("g27_valmatch"))


def _feed(cm, s):
    """the calls the reference validator makes for the images of one set (detect/val.py:83-108)"""
    for im in s["images"]:
        n, m = len(im["predn"]), len(im["cls"])
        if n == 0 and m:
            cm.process_batch(None, im["cls"])
        elif n and m:
            cm.process_batch(im["predn"], im["labelsn"])


def test_confusion_matrix_equals_the_reference(sets):
    from dedark_yolo_amd.utils.metrics import ConfusionMatrix
    assert [s["nc"] for s in sets] == [3, 80, 80]
    for s in sets:
        cm = ConfusionMatrix(nc=s["nc"])
        assert cm.matrix.shape == (s["nc"] + 1, s["nc"] + 1) and cm.matrix.dtype == np.float64 and not cm.matrix.any()
        _feed(cm, s)
        want = s["matrix"].numpy()
        assert want.dtype == cm.matrix.dtype and want[s["nc"]].sum() > 0 and want[:, s["nc"]].sum() > 0 and want[:-1, :-1].sum() > 0
        assert np.array_equal(cm.matrix, want)
        tp, fp = cm.tp_fp()
        assert tp.shape == (s["nc"],) and np.array_equal(tp, s["tp"].numpy()) and np.array_equal(fp, s["fp"].numpy())
    # one matrix over several batches = the sum of theirs
    cm = ConfusionMatrix(nc=80)
    _feed(cm, sets[1])
    _feed(cm, sets[2])
    assert np.array_equal(cm.matrix, sets[1]["matrix"].numpy() + sets[2]["matrix"].numpy())


def _cm(nc=3):
    from dedark_yolo_amd.utils.metrics import ConfusionMatrix
    return ConfusionMatrix(nc=nc)


def _det(*rows):
    return torch.tensor(rows, dtype=torch.float32).view(-1, 6)


def _lab(*rows):
    return torch.tensor(rows, dtype=torch.float32).view(-1, 5)


def test_confusion_matrix_surface():
    from dedark_yolo_amd.utils.metrics import ConfusionMatrix
    cm = ConfusionMatrix(4)
    assert (cm.nc, cm.conf, cm.iou_thres, cm.task) == (4, 0.25, 0.45, "detect") and cm.matrix.shape == (5, 5)
    cc = ConfusionMatrix(4, task="classify")
    assert cc.matrix.shape == (4, 4)
    cc.process_cls_preds([torch.tensor([[1, 0], [2, 3]]), torch.tensor([[1, 2]])], [torch.tensor([1, 3]), torch.tensor([0])])
    want = np.zeros((4, 4))
    want[1, 1] = want[2, 3] = want[1, 0] = 1
    assert np.array_equal(cc.matrix, want)
    tp, fp = cc.tp_fp()
    assert tp.shape == (4,) and tp.tolist() == [0, 1, 0, 0] and fp.tolist() == [0, 1, 1, 0]


def test_confusion_matrix_print(caplog):
    cm = _cm(2)
    cm.process_batch(None, torch.tensor([1.0, 1.0]))
    with caplog.at_level(logging.INFO, logger="dedark_yolo_amd"):
        cm.print()
    assert [r.getMessage() for r in caplog.records] == ["0.0 0.0 0.0", "0.0 0.0 0.0", "0.0 2.0 0.0"]


def test_quirk_confidence_threshold_is_strict():
    cm = _cm()
    lab = _lab([1, 0, 0, 10, 10])
    cm.process_batch(_det([0, 0, 10, 10, 0.25, 2]), lab)                  # conf == 0.25 does not count: the label is missed
    assert cm.matrix[3, 1] == 1 and cm.matrix.sum() == 1
    cm.process_batch(_det([0, 0, 10, 10, 0.2500001, 2]), lab)
    assert cm.matrix[2, 1] == 1 and cm.matrix.sum() == 2


def test_quirk_iou_threshold_is_strict_and_ignores_classes():
    lab = _lab([0, 0, 0, 20, 10])
    for width, hit in ((9, False), (10, True)):                            # IoU 0.45 = f32(0.45) exactly is no candidate; 0.5 is
        cm = _cm()
        d = _det([0, 0, width, 10, 0.9, 2])
        iou = float(vr.box_iou(lab[:, 1:].numpy(), d[:, :4].numpy())[0, 0])
        assert (iou > np.float32(0.45)) == hit
        cm.process_batch(d, lab)
        assert cm.matrix[2, 0] == (1 if hit else 0) and cm.matrix[3, 0] == (0 if hit else 1) and cm.matrix.sum() == 1
    # 9 x 20 against 20 x 20 inside it: IoU = 0.45 in f32 arithmetic, on the threshold: not above it
    cm = _cm()
    d, lab = _det([0, 0, 9, 20, 0.9, 1]), _lab([0, 0, 0, 20, 20])
    assert vr.box_iou(lab[:, 1:].numpy(), d[:, :4].numpy())[0, 0] == np.float32(0.45)
    cm.process_batch(d, lab)
    assert cm.matrix[3, 0] == 1 and cm.matrix.sum() == 1


def test_quirk_unmatched_detections_count_only_with_a_match():
    lab = _lab([0, 0, 0, 10, 10])
    stray = [50, 50, 60, 60, 0.9, 1]
    cm = _cm()
    cm.process_batch(_det(stray), lab)                                      # no match in the image: the stray adds nothing
    assert cm.matrix[3, 0] == 1 and cm.matrix.sum() == 1
    cm = _cm()
    cm.process_batch(_det([0, 0, 10, 10, 0.8, 0], stray, [70, 70, 80, 80, 0.1, 2]), lab)   # with a match it does; conf 0.1 never counts
    assert cm.matrix[0, 0] == 1 and cm.matrix[1, 3] == 1 and cm.matrix.sum() == 2


def test_quirk_labels_without_detections_and_detections_without_labels():
    cm = _cm()
    cm.process_batch(None, torch.tensor([2.0, 2.0, 0.0]))
    assert cm.matrix[3].tolist() == [1, 0, 2, 0] and cm.matrix.sum() == 3
    cm.process_batch(_det(), _lab([1, 0, 0, 5, 5]))                         # an empty detection tensor is the same
    assert cm.matrix[3, 1] == 1 and cm.matrix.sum() == 4
    cm.process_batch(_det([0, 0, 10, 10, 0.9, 1]), _lab())                  # detections, no labels: nothing
    assert cm.matrix.sum() == 4


def test_quirk_classes_are_truncated():
    cm = _cm()
    cm.process_batch(_det([0, 0, 10, 10, 0.9, 1.9]), _lab([2.7, 0, 0, 10, 10]))
    assert cm.matrix[1, 2] == 1 and cm.matrix.sum() == 1


def test_second_step_takes_the_best_overlap_not_the_lowest_index():
    """two detections choose the same label: the confusion rule keeps the better-overlapping one (index 1), the `correct` rule the
    lower index"""
    from dedark_yolo_amd.engine.validator import match_predictions
    lab = _lab([0, 0, 0, 10, 10])
    det = _det([0, 0, 10, 6, 0.9, 1], [0, 0, 10, 10, 0.8, 0])               # IoU 0.6, 1.0
    cm = _cm()
    cm.process_batch(det, lab)
    assert cm.matrix[0, 0] == 1 and cm.matrix[1, 3] == 1 and cm.matrix.sum() == 2
    det[:, 5] = 0
    assert match_predictions(det, lab, IOUV)[:, 0].tolist() == [True, False]


def test_tie_rule_on_an_integer_grid():
    """exact IoU ties: a detection prefers the lower label index, a label the lower detection index"""
    # duplicate labels (classes 0 and 1), one detection on top of both: label 0 is matched, label 1 is missed
    cm = _cm()
    cm.process_batch(_det([0, 0, 8, 8, 0.9, 2]), _lab([0, 0, 0, 8, 8], [1, 0, 0, 8, 8]))
    assert cm.matrix[2, 0] == 1 and cm.matrix[3, 1] == 1 and cm.matrix.sum() == 2
    # duplicate detections (classes 1 and 2) on one label: detection 0 is matched, detection 1 is a false positive
    cm = _cm()
    cm.process_batch(_det([0, 0, 8, 8, 0.9, 1], [0, 0, 8, 8, 0.9, 2]), _lab([0, 0, 0, 8, 8]))
    assert cm.matrix[1, 0] == 1 and cm.matrix[2, 3] == 1 and cm.matrix.sum() == 2
    # both: labels A = B, detections P = Q at IoU 0.5 with both: P and Q choose A; A keeps P; B is missed; Q is a false positive
    cm = _cm()
    cm.process_batch(_det([0, 0, 8, 4, 0.9, 1], [0, 0, 8, 4, 0.6, 2]), _lab([0, 0, 0, 8, 8], [0, 0, 0, 8, 8]))
    assert cm.matrix[1, 0] == 1 and cm.matrix[3, 0] == 1 and cm.matrix[2, 3] == 1 and cm.matrix.sum() == 3
    # the kernel's form of the rule (valmatch_ref.confusion) decides all three the same way
    for det, lab in ((_det([0, 0, 8, 8, 0.9, 2]), _lab([0, 0, 0, 8, 8], [1, 0, 0, 8, 8])),
                     (_det([0, 0, 8, 8, 0.9, 1], [0, 0, 8, 8, 0.9, 2]), _lab([0, 0, 0, 8, 8])),
                     (_det([0, 0, 8, 4, 0.9, 1], [0, 0, 8, 4, 0.6, 2]), _lab([0, 0, 0, 8, 8], [0, 0, 0, 8, 8]))):
        cm = _cm()
        cm.process_batch(det, lab)
        m = vr.confusion(np.zeros((4, 4), dtype=np.int64), vr.box_iou(lab[:, 1:].numpy(), det[:, :4].numpy()), det[:, 4].numpy(),
                         lab[:, 0].numpy(), det[:, 5].numpy())
        assert np.array_equal(m, cm.matrix)


def _grid_case(gen, m, n, nc=3):
    """boxes on an integer grid with duplicates: many exact IoU ties, IoU values on 0.5 and 0.75"""
    def boxes(k):
        xy = gen.integers(0, 6, (k, 2)) * 4
        wh = gen.choice([4, 8, 12, 16], (k, 2))
        return np.concatenate([xy, xy + wh], 1).astype(np.float32)
    lab = np.concatenate([gen.integers(0, nc, (m, 1)).astype(np.float32), boxes(m)], 1)
    det = np.concatenate([boxes(n), gen.choice([0.1, 0.25, 0.3, 0.9], (n, 1)), gen.integers(0, nc, (n, 1))], 1).astype(np.float32)
    if m and n:
        k = min(m, n) // 2
        det[:k, :4] = lab[:k, 1:]
        det[:k, 5] = lab[:k, 0]
        det[k:2 * k] = det[:k]
    return torch.from_numpy(det), torch.from_numpy(lab)


def test_kernel_form_of_both_rules_equals_the_host_statements_on_ties():
    """valmatch_ref.match / .confusion evaluate the rules the way the kernel does; on tie-laden integer-grid cases they agree with
    match_predictions and ConfusionMatrix.process_batch"""
    from dedark_yolo_amd.engine.validator import match_predictions
    gen = np.random.default_rng(271)
    ties = 0
    for m, n in ((1, 1), (3, 7), (9, 20), (16, 12), (5, 40)):
        for _ in range(6):
            det, lab = _grid_case(gen, m, n)
            iou = vr.box_iou(lab[:, 1:].numpy(), det[:, :4].numpy())
            ties += int(len(np.unique(iou[iou > 0.45])) < int((iou > 0.45).sum()))
            assert np.array_equal(vr.match(iou, lab[:, 0].numpy(), det[:, 5].numpy(), IOUV.numpy()), match_predictions(det, lab, IOUV).numpy())
            cm = _cm()
            cm.process_batch(det, lab)
            got = vr.confusion(np.zeros((4, 4), dtype=np.int64), iou, det[:, 4].numpy(), lab[:, 0].numpy(), det[:, 5].numpy())
            assert np.array_equal(got, cm.matrix)
    assert ties > 20


@pytest.mark.parametrize("with_ratio_pad", [False, True])
def test_numpy_scaling_and_iou_equal_scale_boxes_and_box_iou_bit_for_bit(with_ratio_pad):
    from dedark_yolo_amd.engine.validator import scale_record
    from dedark_yolo_amd.utils import ops as uops
    from dedark_yolo_amd.utils.metrics import box_iou
    gen = np.random.default_rng(272)
    H, W = 96, 160
    for h0, w0 in ((480, 800), (300, 640), (427, 640), (96, 160), (77, 333)):
        gain = min(H / h0, W / w0)
        rp = ((gain, gain), ((W - w0 * gain) / 2, (H - h0 * gain) / 2)) if with_ratio_pad else None
        rec = vr.scale_record((H, W), (h0, w0), rp)
        assert np.array_equal(rec, np.array(scale_record((H, W), (h0, w0), rp), dtype=np.float32))
        det = torch.from_numpy(gen.uniform(-5, 165, (50, 4)).astype(np.float32))
        det[:, 2:] += det[:, :2].abs()
        xywh = torch.from_numpy(gen.uniform(0.02, 0.98, (30, 4)).astype(np.float32))
        want_d = uops.scale_boxes((H, W), det.clone(), (h0, w0), ratio_pad=rp)
        tbox = uops.xywh2xyxy(xywh) * torch.tensor((W, H, W, H), dtype=torch.float32)
        want_l = uops.scale_boxes((H, W), tbox, (h0, w0), ratio_pad=rp)
        got_d, got_l = vr.scale_xyxy(det.numpy(), rec), vr.label_boxes(xywh.numpy(), H, W, rec)
        assert got_d.tobytes() == want_d.numpy().tobytes() and got_l.tobytes() == want_l.numpy().tobytes()
        assert (got_d == 0).any() and (got_d == np.float32(w0)).any()                  # the clamp is exercised
        assert vr.box_iou(got_l, got_d).tobytes() == box_iou(want_l, want_d).numpy().tobytes()


def test_numpy_statement_gives_the_reference_results(sets):
    """g27 through valmatch_ref alone: native boxes, `correct` rows and confusion matrices as the reference computed them"""
    for s in sets:
        rows, matrix = [], np.zeros((s["nc"] + 1, s["nc"] + 1), dtype=np.int64)
        for im, pred in zip(s["images"], s["preds"]):
            rec = vr.scale_record((s["H"], s["W"]), im["ori_shape"], im["ratio_pad"])
            predn, tbox = vr.scale_xyxy(pred[:, :4].numpy(), rec), vr.label_boxes(im["bboxes"].numpy(), s["H"], s["W"], rec)
            if len(pred):
                assert predn.tobytes() == im["predn"][:, :4].numpy().tobytes()
            if len(pred) and len(tbox):
                assert tbox.tobytes() == im["labelsn"][:, 1:].numpy().tobytes()
            iou = vr.box_iou(tbox, predn)
            if len(pred):
                rows.append(vr.match(iou, im["cls"].numpy(), pred[:, 5].numpy(), IOUV.numpy()))
            vr.confusion(matrix, iou, pred[:, 4].numpy(), im["cls"].numpy(), pred[:, 5].numpy())
        assert np.array_equal(np.concatenate(rows), s["correct"].numpy().astype(bool))
        assert np.array_equal(matrix, s["matrix"].numpy())


def test_match_predictions_gives_the_reference_correct_rows(sets):
    from dedark_yolo_amd.engine.validator import match_predictions
    for s in sets:
        rows = [match_predictions(im["predn"], im["labelsn"], IOUV) if len(im["labelsn"]) else torch.zeros(len(im["predn"]), 10, dtype=torch.bool)
                for im in s["images"] if len(im["predn"])]
        assert torch.equal(torch.cat(rows), s["correct"].bool())


def test_save_txt_lines_and_json_records_equal_the_reference(sets, tmp_path):
    from dedark_yolo_amd.engine.validator import pred_to_json, save_one_txt
    id_types = set()
    for k, s in enumerate(sets):
        records = []
        for b, im in enumerate(s["images"]):
            if len(im["predn"]) == 0:
                assert str(s["txt"][b]) == ""
                continue
            for save_conf, want in ((False, s["txt"]), (True, s["txt_conf"])):
                f = tmp_path / f"{k}_{b}_{int(save_conf)}.txt"
                save_one_txt(im["predn"], save_conf, im["ori_shape"], f)
                assert f.read_text() == str(want[b])
                assert len(f.read_text().splitlines()[0].split()) == (6 if save_conf else 5)
            records += pred_to_json(im["predn"], s["batch"]["im_file"][b])
        want = json.loads(str(s["json"]))
        assert records == want and len(want) == sum(len(im["predn"]) for im in s["images"])
        id_types |= {type(r["image_id"]) for r in want}
    assert id_types == {int, str}                      # numeric stems became integers, the others stayed names
