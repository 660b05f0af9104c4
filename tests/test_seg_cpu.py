"""Segment task on the CPU (no GPU needed): yolov8-seg.yaml builds with the reference's state_dict layout, parameter counts,
optimizer groups and strides (tests/golden/make_seg_golden.py), the Segment registry rule, task detection, and the checkpoint
writer's classes for a segmentation model."""
import numpy as np
import pytest
import torch

from util import gold, load_yaml


def _model(scale, nc=20):
    from dedark_yolo_amd.nn.tasks import SegmentationModel
    cfg = load_yaml("yolov8-seg.yaml")
    cfg["scale"] = scale
    return SegmentationModel(cfg, nc=nc)


def _opt_groups(m):
    bn_types = tuple(v for k, v in torch.nn.__dict__.items() if "Norm" in k and isinstance(v, type))
    g = [0, 0, 0]
    for mname, mod in m.named_modules():
        for pname, _ in mod.named_parameters(recurse=False):
            full = f"{mname}.{pname}" if mname else pname
            g[2 if "bias" in full else 1 if isinstance(mod, bn_types) else 0] += 1
    return g


@pytest.mark.parametrize("scale", "nl")
def test_seg_graph_matches_the_reference(scale):
    g = gold("g16_seg_keys")
    m = _model(scale)
    sd = m.state_dict()
    p = f"seg_{scale}_"
    assert list(sd.keys()) == [str(k) for k in g[p + "keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g[p + "shapes"]]
    assert sum(q.numel() for q in m.parameters()) == int(g[p + "n_params"])
    assert len(m.model) == int(g[p + "n_layers"])
    assert [sum(q.numel() for q in L.parameters()) for L in m.model] == g[p + "layer_np"].tolist()
    assert _opt_groups(m) == g[p + "opt_groups"].tolist()
    assert m.stride.tolist() == g[p + "stride"].tolist()


def test_segment_head_layout():
    from dedark_yolo_amd.nn.modules import Proto, Segment
    m = _model("n")
    seg = m.model[-1]
    assert isinstance(seg, Segment) and isinstance(seg.proto, Proto)
    assert (seg.nm, seg.npr) == (32, 64)                  # npr = make_divisible(min(256, 1024) * 0.25, 8)
    assert _model("l").model[-1].npr == 256
    keys = [k for k in seg.state_dict() if k.startswith("proto.")]
    assert keys[:2] == ["proto.cv1.conv.weight", "proto.cv1.bn.weight"]
    assert "proto.upsample.weight" in keys and "proto.upsample.bias" in keys
    assert tuple(seg.proto.upsample.weight.shape) == (64, 64, 2, 2)
    assert [k.split(".")[0] for k in seg.state_dict()][-1] == "cv4"


def test_task_detection():
    from dedark_yolo_amd.nn.tasks import guess_model_task, yaml_model_load
    assert guess_model_task(yaml_model_load("yolov8n-seg.yaml")) == "segment"
    assert guess_model_task(yaml_model_load("yolov8n.yaml")) == "detect"
    assert guess_model_task(_model("n")) == "segment"


def test_yolo_facade_builds_the_segment_task():
    from dedark_yolo_amd.engine.model import YOLO
    from dedark_yolo_amd.nn.tasks import SegmentationModel
    y = YOLO("yolov8n-seg.yaml")
    assert y.task == "segment" and isinstance(y.model, SegmentationModel)
    assert YOLO("yolov8n-seg.yaml", task="segment").task == "segment"
    for task in ("pose", "classify"):
        with pytest.raises(NotImplementedError):
            YOLO("yolov8n-seg.yaml", task=task)
    with pytest.raises(RuntimeError, match="GPU"):          # val() dispatches to the segment validator, which runs on the device
        y.val(loader=[])


def test_default_cfg_has_the_mask_keys():
    from dedark_yolo_amd.engine.trainer import get_cfg
    a = get_cfg()
    assert a.overlap_mask is True and a.mask_ratio == 4


def test_reference_checkpoint_of_a_segmentation_model(tmp_path):
    """save_reference_checkpoint names the reference's classes (SegmentationModel, Segment, Proto, torch's ConvTranspose2d),
    carries Segment's nm / npr and `detect = Detect.forward` (pickled as getattr(Detect, 'forward')), and reads back."""
    import pickletools
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint, save_reference_checkpoint
    m = _model("n")
    p = str(tmp_path / "last.pt")
    save_reference_checkpoint(p, m, ema_state=m.state_dict(), epoch=1, train_args=dict(model="yolov8n-seg.yaml", box=7.5))
    import zipfile
    with zipfile.ZipFile(p) as z:
        data = z.read([n for n in z.namelist() if n.endswith("data.pkl")][0])
    ops = [(op.name, arg) for op, arg, _ in pickletools.genops(data)]
    globs = {a for n, a in ops if n == "GLOBAL"}
    for want in ("ultralytics.nn.tasks SegmentationModel", "ultralytics.nn.modules.head Segment", "ultralytics.nn.modules.block Proto",
                 "torch.nn.modules.conv ConvTranspose2d", "ultralytics.nn.modules.head Detect", "__builtin__ getattr"):
        assert want in globs, want
    ck = load_checkpoint(p)
    assert list(ck.state_dict) == list(m.state_dict())
    for k, v in m.state_dict().items():
        w = ck.state_dict[k]
        assert torch.equal(w.float(), v.half().float() if v.is_floating_point() else v.float()), k
    from dedark_yolo_amd.utils.checkpoint import load_raw
    seg = load_raw(p)["model"]._modules["model"]._modules["22"]
    assert type(seg).__name__ == "Segment" and (seg.nm, seg.npr) == (32, 64)
    assert np.isclose(float(seg.stride[-1]), 32.0)


def test_reference_checkpoint_writer_layout_matches_the_reference_for_seg():
    """What save_reference_checkpoint pickles for yolov8n-seg is, module by module, what the reference pickles for it
    (tests/golden/g16_seg_skeleton.json): class paths, plain attributes, parameter / buffer names, shapes and dtypes, children.
    Segment.detect is a function there (Detect.forward) and a getattr(Detect, 'forward') record here: both pickle the same way."""
    import json
    import os
    from test_host_cpu import _written_skeleton
    from util import GOLD
    from dedark_yolo_amd.utils.checkpoint import _RefMethod, reference_module_object
    with open(os.path.join(GOLD, "g16_seg_skeleton.json")) as f:
        want = json.load(f)["seg_n"]
    obj = reference_module_object(_model("n"), None, True, dict(box=7.5, cls=0.5, dfl=1.5, lrl=2.0))
    seg = obj._modules["model"]._modules["22"]
    assert isinstance(seg.__dict__["detect"], _RefMethod) and seg.__dict__["detect"].name == "forward"
    assert seg.__dict__["detect"].obj.__module__ == "ultralytics.nn.modules.head" and seg.__dict__["detect"].obj.__qualname__ == "Detect"
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
    walk(want, got, "seg_n")
    assert not bad, bad[:10]


def test_reads_a_seg_checkpoint_the_reference_wrote():
    """tests/golden/g16_ref_seg_last.pt: written by the reference's own classes (trainer.save_model layout, no EMA)."""
    import os
    from util import GOLD
    from dedark_yolo_amd.engine.model import YOLO
    from dedark_yolo_amd.nn.tasks import SegmentationModel
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint
    p = os.path.join(GOLD, "g16_ref_seg_last.pt")
    ck = load_checkpoint(p)
    cfg = load_yaml("yolov8-seg.yaml")
    cfg["scales"]["u"] = [0.33, 0.0625, 1024]
    cfg["scale"] = "u"
    m = SegmentationModel(cfg, nc=4)
    assert list(ck.state_dict) == list(m.state_dict())
    assert ck.epoch == 4 and ck.nc == 4
    y = YOLO(p)
    assert y.task == "segment" and isinstance(y.model, SegmentationModel)
    for k, v in y.model.state_dict().items():
        assert torch.equal(v.float(), ck.state_dict[k].float()), k


def test_segment_metrics_vs_reference():
    from dedark_yolo_amd.utils.metrics import SegmentMetrics
    g = gold("g16_val")
    sm = SegmentMetrics(names={i: str(i) for i in range(4)})
    sm.process(g["tp_b"].numpy(), g["tp_m"].numpy(), g["conf"].numpy(), g["pcls"].numpy(), g["tcls"].numpy())
    rd = sm.results_dict
    assert list(rd) == [str(k) for k in g["metric_keys"]]
    np.testing.assert_allclose(np.array(list(rd.values())), g["metric_values"].numpy(), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("which", ["overlap", "planes"])
def test_iou_matrix_matcher_vs_reference(which):
    """match_from_iou on the reference's mask IoU gives the reference's _process_batch(masks=True) correct matrix."""
    from dedark_yolo_amd.engine.validator import match_from_iou
    g = gold("g16_val")
    iou = g["iou"].numpy()
    got = match_from_iou(iou, g["labels"][:, 0], g["dets"][:, 5], torch.linspace(0.5, 0.95, 10))
    assert torch.equal(got, g["correct_overlap" if which == "overlap" else "correct_planes"])
