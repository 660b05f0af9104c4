"""Pose task on the CPU (no GPU needed): yolov8-pose.yaml / yolov8-pose-p6.yaml build with the reference's state_dict layout,
parameter counts, optimizer groups and strides (tests/golden/make_pose_golden.py), the Pose registry rule, task detection, the YOLO
facade, the pose / kobj gains, the checkpoint writer's classes for a pose model, PoseMetrics and the keypoint `correct` matrices."""
import numpy as np
import pytest
import torch

from util import gold, load_yaml


def _model(scale, yml="yolov8-pose.yaml", **kw):
    from dedark_yolo_amd.nn.tasks import PoseModel
    cfg = load_yaml(yml)
    cfg["scale"] = scale
    return PoseModel(cfg, **kw)


def _opt_groups(m):
    bn_types = tuple(v for k, v in torch.nn.__dict__.items() if "Norm" in k and isinstance(v, type))
    g = [0, 0, 0]
    for mname, mod in m.named_modules():
        for pname, _ in mod.named_parameters(recurse=False):
            full = f"{mname}.{pname}" if mname else pname
            g[2 if "bias" in full else 1 if isinstance(mod, bn_types) else 0] += 1
    return g


@pytest.mark.parametrize("yml,scale,tag", [("yolov8-pose.yaml", "n", "pose_n"), ("yolov8-pose.yaml", "l", "pose_l"),
                                           ("yolov8-pose-p6.yaml", "n", "p6_n")])
def test_pose_graph_matches_the_reference(yml, scale, tag):
    g = gold("g17_pose_keys")
    m = _model(scale, yml)
    sd = m.state_dict()
    p = tag + "_"
    assert list(sd.keys()) == [str(k) for k in g[p + "keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g[p + "shapes"]]
    assert sum(q.numel() for q in m.parameters()) == int(g[p + "n_params"])
    assert len(m.model) == int(g[p + "n_layers"])
    assert [sum(q.numel() for q in L.parameters()) for L in m.model] == g[p + "layer_np"].tolist()
    assert _opt_groups(m) == g[p + "opt_groups"].tolist()
    assert m.stride.tolist() == g[p + "stride"].tolist()


def test_pose_head_layout():
    from dedark_yolo_amd.nn.modules import Detect, Pose
    m = _model("n")
    head = m.model[-1]
    assert isinstance(head, Pose) and isinstance(head, Detect)
    assert list(head.kpt_shape) == [17, 3] and head.nk == 51 and head.nl == 3
    assert head.cv4[0][0].conv.out_channels == 51                # c4 = max(64 // 4, 51)
    assert _model("l").model[-1].cv4[0][0].conv.out_channels == 64
    assert [k.split(".")[0] for k in head.state_dict()][-1] == "cv4"
    assert head.detect is Detect.forward
    assert _model("n", "yolov8-pose-p6.yaml").model[-1].nl == 4


def test_pose_registry_rule_and_kpt_override():
    from dedark_yolo_amd.nn.tasks import PoseModel
    m = _model("n", data_kpt_shape=(5, 2))
    head = m.model[-1]
    assert tuple(head.kpt_shape) == (5, 2) and head.nk == 10
    assert head.cv4[0][2].out_channels == 10 and head.cv4[0][0].conv.out_channels == 16
    assert m.yaml["kpt_shape"] == (5, 2)
    with pytest.raises(ValueError):
        PoseModel(load_yaml("yolov8-seg.yaml"))


def test_task_detection():
    from dedark_yolo_amd.nn.tasks import guess_model_task, yaml_model_load
    assert guess_model_task(yaml_model_load("yolov8n-pose.yaml")) == "pose"
    assert guess_model_task(yaml_model_load("yolov8n-pose-p6.yaml")) == "pose"
    assert guess_model_task(yaml_model_load("yolov8n-seg.yaml")) == "segment"
    assert guess_model_task(yaml_model_load("yolov8n.yaml")) == "detect"
    assert guess_model_task(_model("n")) == "pose"


def test_yolo_facade_builds_the_pose_task():
    from dedark_yolo_amd.engine.model import YOLO
    from dedark_yolo_amd.nn.tasks import PoseModel
    y = YOLO("yolov8n-pose.yaml")
    assert y.task == "pose" and isinstance(y.model, PoseModel)
    assert YOLO("yolov8n-pose.yaml", task="pose").task == "pose"
    for task in ("detect", "segment", "classify"):
        with pytest.raises(NotImplementedError):
            YOLO("yolov8n-pose.yaml", task=task)
    for yml in ("yolov8n.yaml", "yolov8n-seg.yaml"):
        with pytest.raises(NotImplementedError):
            YOLO(yml, task="pose")
    with pytest.raises(RuntimeError, match="GPU"):          # val() dispatches to the pose validator, which runs on the device
        y.val(loader=[])


def test_default_cfg_has_the_pose_gains():
    from dedark_yolo_amd.engine.trainer import get_cfg
    a = get_cfg()
    assert a.pose == 12.0 and a.kobj == 1.0


def test_reference_checkpoint_of_a_pose_model(tmp_path):
    """save_reference_checkpoint names the reference's classes (PoseModel, Pose), carries kpt_shape / nk and `detect =
    Detect.forward` (pickled as getattr(Detect, 'forward')), and reads back through the restricted unpickler."""
    import pickletools
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint, reference_module_object, save_reference_checkpoint
    m = _model("n")
    obj = reference_module_object(m)
    assert type(obj).__module__ == "ultralytics.nn.tasks" and type(obj).__name__ == "PoseModel"
    head = obj._modules["model"]._modules["22"]
    assert type(head).__module__ == "ultralytics.nn.modules.head" and type(head).__name__ == "Pose"
    assert head.kpt_shape == [17, 3] and head.nk == 51 and head.nc == 1 and head.no == 65
    assert head.detect.name == "forward" and head.detect.obj.__name__ == "Detect"
    p = str(tmp_path / "last.pt")
    save_reference_checkpoint(p, m, ema_state=m.state_dict())
    import zipfile
    with zipfile.ZipFile(p) as z:
        data = z.read([n for n in z.namelist() if n.endswith("data.pkl")][0])
    globals_ = set()
    for op, arg, _ in pickletools.genops(data):
        if op.name in ("GLOBAL", "STACK_GLOBAL") and isinstance(arg, str):
            globals_.add(arg)
    assert "ultralytics.nn.tasks PoseModel" in globals_ and "ultralytics.nn.modules.head Pose" in globals_
    ck = load_checkpoint(p)
    assert ck.source == "reference-pickle" and list(ck.state_dict) == list(m.state_dict())
    assert ck.yaml["kpt_shape"] == [17, 3]
    from dedark_yolo_amd.engine.model import YOLO
    y = YOLO(p)
    assert y.task == "pose"
    for k, v in y.model.state_dict().items():
        assert torch.equal(v.float(), m.state_dict()[k].float().half().float()), k


def test_pose_metrics_vs_reference():
    from dedark_yolo_amd.utils.metrics import PoseMetrics
    g = gold("g17_pose_val")
    pm = PoseMetrics(names={i: str(i) for i in range(4)})
    pm.process(g["tp_b"].numpy(), g["tp_p"].numpy(), g["conf"].numpy(), g["pcls"].numpy(), g["tcls"].numpy())
    rd = pm.results_dict
    assert list(rd) == [str(k) for k in g["metric_keys"]]
    np.testing.assert_allclose(np.array(list(rd.values())), g["metric_values"].numpy(), rtol=1e-9, atol=1e-12)


def test_keypoint_correct_matrices_vs_reference():
    """match_from_iou on the reference's OKS matrix gives the reference PoseValidator._process_batch correct matrix (pose and
    box)."""
    from dedark_yolo_amd.engine.validator import match_from_iou, match_predictions
    g = gold("g17_pose_val")
    iouv = torch.linspace(0.5, 0.95, 10)
    got = match_from_iou(g["oks"].numpy(), g["labels"][:, 0], g["dets"][:, 5], iouv)
    assert torch.equal(got, g["correct_pose"])
    assert g["correct_pose"].any() and not g["correct_pose"].all()
    assert torch.equal(match_predictions(g["dets"], g["labels"], iouv), g["correct_box"])


def test_scale_coords_matches_the_reference_rule():
    from dedark_yolo_amd.utils.ops import scale_coords
    c = torch.tensor([[[10.0, 20.0, 0.5], [630.0, 5.0, 1.0], [320.0, 600.0, 0.0]]])
    out = scale_coords((640, 640), c.clone(), (480, 640))            # gain 1, pad (0, 80): not rounded, then clipped
    exp = torch.tensor([[[10.0, 0.0, 0.5], [630.0, 0.0, 1.0], [320.0, 480.0, 0.0]]])
    assert torch.equal(out, exp)
    out = scale_coords((640, 640), c.clone(), (300, 200), ratio_pad=((2.0, 2.0), (3.0, 7.0)))
    assert torch.allclose(out[0, 0, :2], torch.tensor([3.5, 6.5])) and out[0, 1, 0] == 200.0


def test_pose_loss_names_the_batch_error():
    from dedark_yolo_amd.utils.loss import _gt_keypoints
    batch = dict(batch_idx=torch.zeros(2))
    with pytest.raises(ValueError, match="keypoints"):
        _gt_keypoints(batch, 17, "cpu")
    batch["keypoints"] = torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match="K=17"):
        _gt_keypoints(batch, 17, "cpu")


def test_reference_checkpoint_writer_layout_matches_the_reference_for_pose():
    """What save_reference_checkpoint pickles for yolov8n-pose is, module by module, what the reference pickles for it
    (tests/golden/g17_pose_skeleton.json): class paths, plain attributes (kpt_shape, nk, ...), parameter / buffer names, shapes and
    dtypes, children.  Pose.detect is a function there (Detect.forward) and a getattr(Detect, 'forward') record here: both pickle the
    same way."""
    import json
    import os
    from test_host_cpu import _written_skeleton
    from util import GOLD
    from dedark_yolo_amd.utils.checkpoint import _RefMethod, reference_module_object
    with open(os.path.join(GOLD, "g17_pose_skeleton.json")) as f:
        want = json.load(f)["pose_n"]
    obj = reference_module_object(_model("n"), None, True, dict(box=7.5, cls=0.5, dfl=1.5, pose=12.0, kobj=1.0))
    head = obj._modules["model"]._modules["22"]
    assert isinstance(head.__dict__["detect"], _RefMethod) and head.__dict__["detect"].name == "forward"
    assert head.__dict__["detect"].obj.__module__ == "ultralytics.nn.modules.head" and head.__dict__["detect"].obj.__qualname__ == "Detect"
    got = _written_skeleton(obj)
    bad = []

    def walk(a, b, path):
        if a["cls"] != b["cls"]:
            bad.append((path, "class", a["cls"], b["cls"]))
        for k in set(a["attrs"]) | set(b["attrs"]):
            if k not in ("yaml", "detect") and a["attrs"].get(k, "<absent>") != b["attrs"].get(k, "<absent>"):
                bad.append((path, k, a["attrs"].get(k, "<absent>"), b["attrs"].get(k, "<absent>")))
        if ("detect" in a["attrs"]) != ("detect" in b["attrs"]):
            bad.append((path, "detect"))
        for f_ in ("params", "buffers"):
            if a[f_] != b[f_]:
                bad.append((path, f_, a[f_], b[f_]))
        if list(a["children"]) != list(b["children"]):
            bad.append((path, "children", list(a["children"]), list(b["children"])))
        for k, c in a["children"].items():
            if c is not None and b["children"].get(k) is not None:
                walk(c, b["children"][k], path + "." + k)
    assert want["children"]["model"]["children"]["22"]["cls"].endswith("Pose")
    walk(want, got, "pose_n")
    assert not bad, bad[:10]


def test_reads_a_pose_checkpoint_the_reference_wrote():
    """tests/golden/g17_ref_pose_last.pt: written by the reference's own classes (trainer.save_model layout, no EMA)."""
    import os
    from util import GOLD
    from dedark_yolo_amd.engine.model import YOLO
    from dedark_yolo_amd.nn.tasks import PoseModel
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint
    p = os.path.join(GOLD, "g17_ref_pose_last.pt")
    ck = load_checkpoint(p)
    assert ck.source == "reference-pickle" and ck.yaml["kpt_shape"] == [17, 3]
    cfg = load_yaml("yolov8-pose.yaml")
    cfg["scales"]["u"] = [0.33, 0.03125, 1024]
    cfg["scale"] = "u"
    m = PoseModel(cfg, nc=4)
    assert list(ck.state_dict) == list(m.state_dict())
    assert ck.epoch == 4 and ck.nc == 4
    y = YOLO(p)
    assert y.task == "pose" and isinstance(y.model, PoseModel) and list(y.model.model[-1].kpt_shape) == [17, 3]
    for k, v in y.model.state_dict().items():
        assert torch.equal(v.float(), ck.state_dict[k].float()), k
