"""Classify task on the CPU (no GPU needed): the float64 restatement (tests/classify_ref.py) against the reference's loss, gradient,
metrics and confusion fixtures (tests/golden/make_classify_golden.py), yolov8-cls.yaml against the reference's state_dict layout,
counts and optimizer groups, the Classify registry rule, task detection and the YOLO facade, Probs, ClassifyMetrics, the checkpoint
writer's classes for a classify model, reading a checkpoint the reference wrote, and the library's new symbols."""
import json
import os

import numpy as np
import pytest
import torch

import classify_ref as cr
from util import GOLD, close, gold, load_yaml


def _model(scale, nc=None):
    from dedark_yolo_amd.nn.tasks import ClassificationModel
    cfg = load_yaml("cls/yolov8-cls.yaml")
    cfg["scale"] = scale
    return ClassificationModel(cfg, nc=nc)


def _opt_groups(m):
    bn_types = tuple(v for k, v in torch.nn.__dict__.items() if "Norm" in k and isinstance(v, type))
    g = [0, 0, 0]
    for mname, mod in m.named_modules():
        for pname, _ in mod.named_parameters(recurse=False):
            full = f"{mname}.{pname}" if mname else pname
            g[2 if "bias" in full else 1 if isinstance(mod, bn_types) else 0] += 1
    return g


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("tag", ["normal", "ignore", "big"])
def test_restatement_reproduces_the_reference_loss_and_gradient(tag):
    g = gold(f"g21_clsloss_{tag}")
    loss, grad = cr.xent(g["logits"], g["cls"])
    close(loss, g["loss"], 1e-6, 1e-7, "loss")
    close(loss, g["items"], 1e-6, 1e-7, "items")
    close(grad, g["dlogits"], 1e-5, 1e-8, "dlogits")
    if tag == "ignore":
        assert int(g["cls"][1]) == -100 and float(g["dlogits"][1].abs().max()) == 0.0
        assert float(grad[1].abs().max()) == 0.0
    if tag == "big":
        assert float(g["logits"].abs().max()) > 60.0


@pytest.mark.parametrize("nc", [3, 12])
def test_restatement_reproduces_the_reference_metrics(nc):
    g = gold("g21_cls_metrics")
    p = f"nc{nc}_"
    k = min(nc, 5)
    probs = g[p + "probs"]
    # no ties among the k + 1 largest of any row: the reference's (unstable) argsort and the stable rule agree
    top = torch.sort(probs, 1, descending=True).values[:, :min(nc, k + 1)]
    assert bool((top[:, :-1] > top[:, 1:]).all())
    pred = cr.topk(probs, k)
    assert torch.equal(pred, g[p + "pred"].long())
    m = cr.metrics(pred.numpy(), g[p + "cls"].numpy(), nc)
    keys = [str(s) for s in g[p + "metric_keys"]]
    assert keys == ["metrics/accuracy_top1", "metrics/accuracy_top5", "fitness"]
    want = g[p + "metric_values"].numpy()
    np.testing.assert_allclose([m["top1"], m["top5"], m["fitness"]], want, rtol=0, atol=1e-6)
    assert abs(want[2] - (want[0] + want[1]) / 2) < 1e-9               # the code's rule, not the docstring's
    assert np.array_equal(m["confusion"], g[p + "confusion"].numpy())
    assert int(m["confusion"].sum()) == int(g[p + "batch_sizes"].sum())


# ---------------------------------------------------------------------------------------------------- graph
@pytest.mark.parametrize("scale,nc", [("n", 1000), ("l", 1000), ("n", 10)])
def test_cls_graph_matches_the_reference(scale, nc):
    g = gold("g21_cls_keys")
    m = _model(scale, nc)
    sd = m.state_dict()
    p = f"cls_{scale}_{nc}_"
    assert list(sd.keys()) == [str(k) for k in g[p + "keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g[p + "shapes"]]
    assert sum(q.numel() for q in m.parameters()) == int(g[p + "n_params"])
    assert len(m.model) == int(g[p + "n_layers"])
    assert [sum(q.numel() for q in L.parameters()) for L in m.model] == g[p + "layer_np"].tolist()
    assert _opt_groups(m) == g[p + "opt_groups"].tolist()
    assert m.stride.tolist() == g[p + "stride"].tolist() == [1.0]
    bns = sorted({(x.eps, x.momentum) for x in m.modules() if isinstance(x, torch.nn.BatchNorm2d)})
    assert bns == [tuple(r) for r in g[p + "bn_eps_momentum"].tolist()] == [(1e-5, 0.1)]
    assert hasattr(m.model[-1], "nc") == bool(g[p + "has_nc_attr"]) is False
    assert m.names == {i: str(i) for i in range(nc)}
    assert all(float(b.abs().max()) == 0 for k, b in sd.items() if k.endswith("running_mean"))      # no warm-up passes


def test_classify_head_layout_and_rule():
    from dedark_yolo_amd.nn.modules import Classify, Detect
    from dedark_yolo_amd.nn.tasks import ClassificationModel, DetectionModel
    head = _model("n", 10).model[-1]
    assert isinstance(head, Classify) and not isinstance(head, Detect)
    assert list(head.state_dict()) == ["conv.conv.weight", "conv.bn.weight", "conv.bn.bias", "conv.bn.running_mean", "conv.bn.running_var",
                                       "conv.bn.num_batches_tracked", "linear.weight", "linear.bias"]
    assert tuple(head.linear.weight.shape) == (10, 1280) and head.conv.conv.in_channels == 256
    assert head.drop.p == 0.0 and isinstance(head.pool, torch.nn.AdaptiveAvgPool2d)
    assert _model("l").model[-1].conv.conv.in_channels == 1024 and _model("l").model[-1].linear.out_features == 1000
    with pytest.raises(ValueError):
        ClassificationModel(load_yaml("yolov8.yaml"))
    cfg = load_yaml("cls/yolov8-cls.yaml")
    cfg["nc"] = None
    with pytest.raises(ValueError):
        ClassificationModel(cfg)
    assert isinstance(DetectionModel(load_yaml("yolov8.yaml")), DetectionModel)


def test_task_detection():
    from dedark_yolo_amd.nn.tasks import all_tasks, guess_model_task, task_table, yaml_model_load
    assert guess_model_task(yaml_model_load("yolov8n-cls.yaml")) == "classify"
    assert guess_model_task(_model("n", 10)) == "classify"
    for yml, task in (("yolov8n.yaml", "detect"), ("yolov8n-seg.yaml", "segment"), ("yolov8n-pose.yaml", "pose")):
        assert guess_model_task(yaml_model_load(yml)) == task
    assert list(all_tasks()) == ["segment", "pose", "detect", "classify"] and list(task_table()) == ["segment", "pose", "detect"]
    with pytest.raises(NotImplementedError):
        guess_model_task(dict(head=[[-1, 1, "RTDETRDecoder", [80]]]))


def test_yolo_facade_builds_the_classify_task():
    from dedark_yolo_amd.engine.model import YOLO
    from dedark_yolo_amd.nn.tasks import ClassificationModel
    y = YOLO("yolov8n-cls.yaml")
    assert y.task == "classify" and isinstance(y.model, ClassificationModel)
    assert YOLO("yolov8s-cls.yaml", task="classify").task == "classify"
    for task in ("detect", "segment", "pose"):
        with pytest.raises(NotImplementedError):
            YOLO("yolov8n-cls.yaml", task=task)
    for yml in ("yolov8n.yaml", "yolov8n-seg.yaml", "yolov8n-pose.yaml"):
        with pytest.raises(NotImplementedError):
            YOLO(yml, task="classify")
    with pytest.raises(NotImplementedError):
        YOLO("yolov8n-cls.yaml", task="obb")
    with pytest.raises(RuntimeError, match="GPU"):          # val() dispatches to the classify validator, which runs on the device
        y.val(loader=[])


def test_loss_rejects_host_labels_outside_the_classes():
    from dedark_yolo_amd.utils.loss import v8ClassificationLoss
    crit = v8ClassificationLoss()
    for bad in (10, -1, -99):
        with pytest.raises(ValueError):
            crit(torch.zeros(3, 10), dict(cls=torch.tensor([1, bad, 2])))


# ---------------------------------------------------------------------------------------------------- results and metrics
def test_probs_members_on_the_host():
    from dedark_yolo_amd.engine.results import Probs, Results
    p = torch.tensor([0.05, 0.3, 0.3, 0.02, 0.03, 0.2, 0.1])
    pr = Probs(p)
    assert pr.top1 == 1 and pr.top5 == [1, 2, 5, 6, 0]                  # the tie keeps ascending index order
    assert float(pr.top1conf) == pytest.approx(0.3) and torch.equal(pr.top5conf, p[[1, 2, 5, 6, 0]])
    assert len(pr) == 7 and pr.data is p and torch.equal(pr.cpu().data, p)
    assert Probs(torch.tensor([0.2, 0.7, 0.1])).top5 == [1, 0, 2]       # k = min(nc, 5)
    r = Results((64, 48), names={i: str(i) for i in range(7)}, probs=p)
    assert r.boxes is None and r.keypoints is None and r.masks is None and len(r) == 7 and r.probs.top1 == 1
    r = Results((64, 48), torch.zeros(2, 6))
    assert r.probs is None and len(r) == 2


def test_classify_metrics_object():
    from dedark_yolo_amd.utils.metrics import ClassifyMetrics
    g = gold("g21_cls_metrics")
    for nc in (3, 12):
        p = f"nc{nc}_"
        sizes = [int(v) for v in g[p + "batch_sizes"]]
        m = ClassifyMetrics()
        assert m.keys == ["metrics/accuracy_top1", "metrics/accuracy_top5"] and m.results_dict["fitness"] == 0
        m.process(list(g[p + "cls"].split(sizes)), list(g[p + "pred"].split(sizes)))
        rd = m.results_dict
        assert list(rd) == [str(s) for s in g[p + "metric_keys"]]
        np.testing.assert_allclose(list(rd.values()), g[p + "metric_values"].numpy(), rtol=0, atol=1e-6)
        assert m.fitness == (m.top1 + m.top5) / 2


# ---------------------------------------------------------------------------------------------------- checkpoints
def test_reference_checkpoint_writer_layout_matches_the_reference_for_classify():
    """What save_reference_checkpoint pickles for yolov8n-cls is, module by module, what the reference pickles for it
    (tests/golden/g21_cls_skeleton.json): class paths (ClassificationModel, Classify, torch's AdaptiveAvgPool2d / Dropout / Linear),
    plain attributes, parameter / buffer names, shapes and dtypes, children."""
    from test_host_cpu import _written_skeleton
    from dedark_yolo_amd.utils.checkpoint import reference_module_object
    with open(os.path.join(GOLD, "g21_cls_skeleton.json")) as f:
        want = json.load(f)["cls_n"]
    obj = reference_module_object(_model("n"))
    assert type(obj).__module__ == "ultralytics.nn.tasks" and type(obj).__name__ == "ClassificationModel"
    head = obj._modules["model"]._modules["9"]
    assert type(head).__module__ == "ultralytics.nn.modules.head" and type(head).__name__ == "Classify"
    assert [type(c).__module__ + "." + type(c).__name__ for c in head._modules.values()] == [
        "ultralytics.nn.modules.conv.Conv", "torch.nn.modules.pooling.AdaptiveAvgPool2d", "torch.nn.modules.dropout.Dropout",
        "torch.nn.modules.linear.Linear"]
    got = _written_skeleton(obj)
    bad = []

    def walk(a, b, path):
        if a["cls"] != b["cls"]:
            bad.append((path, "class", a["cls"], b["cls"]))
        for k in set(a["attrs"]) | set(b["attrs"]):
            if k not in ("yaml",) and a["attrs"].get(k, "<absent>") != b["attrs"].get(k, "<absent>"):
                bad.append((path, k, a["attrs"].get(k, "<absent>"), b["attrs"].get(k, "<absent>")))
        for f_ in ("params", "buffers"):
            if a[f_] != b[f_]:
                bad.append((path, f_, a[f_], b[f_]))
        if list(a["children"]) != list(b["children"]):
            bad.append((path, "children", list(a["children"]), list(b["children"])))
        for k, c in a["children"].items():
            if c is not None and b["children"].get(k) is not None:
                walk(c, b["children"][k], path + "." + k)
    assert want["children"]["model"]["children"]["9"]["cls"].endswith("Classify")
    walk(want, got, "cls_n")
    assert not bad, bad[:10]


def test_writes_and_reads_back_a_classify_checkpoint(tmp_path):
    from dedark_yolo_amd.engine.model import YOLO
    from dedark_yolo_amd.nn.tasks import ClassificationModel
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint, save_reference_checkpoint
    cfg = load_yaml("cls/yolov8-cls.yaml")
    cfg["scales"]["u"] = [0.33, 0.03125, 1024]
    cfg["scale"] = "u"
    m = ClassificationModel(cfg, nc=7)
    p = save_reference_checkpoint(str(tmp_path / "last.pt"), m, epoch=2)
    ck = load_checkpoint(p)
    assert ck.source == "reference-pickle" and ck.nc == 7 and ck.epoch == 2
    assert list(ck.state_dict) == list(m.state_dict())
    y = YOLO(p)
    assert y.task == "classify" and isinstance(y.model, ClassificationModel) and y.model.model[-1].linear.out_features == 7
    for k, v in y.model.state_dict().items():
        assert torch.equal(v.float(), m.state_dict()[k].half().float()), k


def test_reads_a_classify_checkpoint_the_reference_wrote():
    """tests/golden/g21_ref_cls_last.pt: written by the reference's own classes (trainer.save_model layout, no EMA)."""
    from dedark_yolo_amd.engine.model import YOLO
    from dedark_yolo_amd.nn.tasks import ClassificationModel
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint
    p = os.path.join(GOLD, "g21_ref_cls_last.pt")
    ck = load_checkpoint(p)
    assert ck.source == "reference-pickle"
    cfg = load_yaml("cls/yolov8-cls.yaml")
    cfg["scales"]["u"] = [0.33, 0.03125, 1024]
    cfg["scale"] = "u"
    m = ClassificationModel(cfg, nc=10)
    assert list(ck.state_dict) == list(m.state_dict())
    assert ck.epoch == 4 and ck.nc == 10
    y = YOLO(p)
    assert y.task == "classify" and isinstance(y.model, ClassificationModel)
    for k, v in y.model.state_dict().items():
        assert torch.equal(v.float(), ck.state_dict[k].float()), k
    for task in ("detect", "pose"):
        with pytest.raises(NotImplementedError):
            YOLO(p, task=task)


# ---------------------------------------------------------------------------------------------------- library
def test_library_exports_the_classify_symbols():
    from dedark_yolo_amd import _C
    names = ["dy_gap_fwd", "dy_gap_bwd", "dy_cls_xent_fwd", "dy_cls_xent_bwd", "dy_cls_softmax", "dy_cls_topk", "dy_cls_metrics_update"]
    assert all(n in _C.exported_symbols() for n in names)
    L = _C.lib()
    assert all(hasattr(L, n) for n in names)
    with open(os.path.join(os.path.dirname(GOLD), "..", "include", "dedark_yolo.h")) as f:
        header = f.read()
    assert all(f"int {n}(" in header for n in names)
