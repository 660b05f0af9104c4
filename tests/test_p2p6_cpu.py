"""Four-level graphs and the remaining detection graphs on the CPU (no GPU needed): yolov8-p2.yaml, yolov8-p6.yaml (C2 blocks),
yolov8-Faster4.0.yaml, yolov8-Faster3.0-ThreeHead.yaml and yolov8+RBF.yaml build; state_dict layout, optimizer groups, strides and
the p6 checkpoint skeleton match fixtures captured from the reference (tests/golden/make_p2p6_golden.py)."""
import json
import os

import numpy as np
import pytest

from util import GOLD, load_yaml

GRAPHS = {"p2": "yolov8-p2.yaml", "p6": "yolov8-p6.yaml", "f4": "yolov8-Faster4.0.yaml", "th": "yolov8-Faster3.0-ThreeHead.yaml",
          "rbf": "yolov8+RBF.yaml"}
# scales at which the reference's own constructor succeeds (MFRU / ASFF / RFBblock widths are fixed: l only)
SCALES = {"p2": "nsmlx", "p6": "nsmlx", "f4": "l", "th": "l", "rbf": "l"}


def _model(name, scale, nc=20):
    from dedark_yolo_amd.nn.tasks import DetectionModel
    cfg = load_yaml(name)
    cfg["scale"] = scale
    return DetectionModel(cfg, nc=nc)


@pytest.mark.parametrize("tag,scale", [(t, s) for t in GRAPHS for s in SCALES[t]])
def test_yamls_build_at_every_scale_the_reference_builds(tag, scale):
    from dedark_yolo_amd.nn.modules import C2, Detect
    m = _model(GRAPHS[tag], scale)
    det = m.model[-1]
    assert isinstance(det, Detect)
    assert det.nl == (4 if tag in ("p2", "p6") else 3)
    if tag == "p6":
        assert sum(isinstance(L, C2) for L in m.model) == 6


def test_strides_of_the_four_level_heads():
    assert _model(GRAPHS["p2"], "n").stride.tolist() == [4.0, 8.0, 16.0, 32.0]
    assert _model(GRAPHS["p6"], "n").stride.tolist() == [8.0, 16.0, 32.0, 64.0]
    assert _model(GRAPHS["rbf"], "l").stride.tolist() == [32.0, 16.0, 8.0]        # coarse-to-fine Detect order


def test_scale_prefixed_names_resolve():
    from dedark_yolo_amd.nn.tasks import yaml_model_load
    d = yaml_model_load("yolov8l-p2.yaml")
    assert d["scale"] == "l" and d["head"][-1][0] == [18, 21, 24, 27]
    d = yaml_model_load("yolov8n-p6.yaml")
    assert d["scale"] == "n" and d["head"][2][2] == "C2"
    for name in ("yolov8l-Faster4.0.yaml", "yolov8l-Faster3.0-ThreeHead.yaml", "yolov8l+RBF.yaml"):
        assert yaml_model_load(name)["scale"] == "l"


def test_c2_is_registered_with_the_c2f_rule():
    from dedark_yolo_amd.nn.modules import C2
    from dedark_yolo_amd.nn.tasks import _REGISTRY, _RULES, _rule_c2f
    assert _REGISTRY["C2"] is C2 and _RULES[C2] is _rule_c2f


def test_c2_keys_follow_the_reference():
    from dedark_yolo_amd.nn.modules import C2
    sd = C2(48, 32, 2, False).state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert shapes["cv1.conv.weight"] == (32, 48, 1, 1)
    assert shapes["cv2.conv.weight"] == (32, 32, 1, 1)
    assert shapes["m.0.cv1.conv.weight"] == (16, 16, 3, 3) and shapes["m.1.cv2.conv.weight"] == (16, 16, 3, 3)
    assert [k for k in sd if k.startswith("m.")][0] == "m.0.cv1.conv.weight"


@pytest.mark.parametrize("tag,scale", [("p2", "n"), ("p2", "l"), ("p6", "n"), ("p6", "l"), ("f4", "l"), ("th", "l"), ("rbf", "l")])
def test_state_dict_counts_and_optimizer_groups_match_the_reference(tag, scale):
    z = np.load(os.path.join(GOLD, "g15_p2p6_keys.npz"))
    p = f"{tag}_{scale}_"
    m = _model(GRAPHS[tag], scale)
    sd = m.state_dict()
    assert list(sd.keys()) == list(z[p + "keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(z[p + "shapes"])
    assert sum(q.numel() for q in m.parameters()) == int(z[p + "n_params"])
    assert len(m.model) == int(z[p + "n_layers"])
    assert [L.np for L in m.model] == [int(v) for v in z[p + "layer_np"]]
    assert m.stride.tolist() == z[p + "stride"].tolist()
    from types import SimpleNamespace
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, FlatState
    _, sizes = DetectionTrainer._param_order(SimpleNamespace(flat=FlatState(m, with_ema=False)))
    bias, decayed, bn_w = sizes
    frozen = [k for k, q in m.named_parameters() if not q.requires_grad]
    assert frozen == [k for k in sd if k.endswith(".dfl.conv.weight")]
    assert [decayed + len(frozen), bn_w, bias] == [int(v) for v in z[p + "opt_groups"]]


def test_reference_checkpoint_writer_layout_for_p6():
    """save_reference_checkpoint's object tree for yolov8n-p6 is, module by module, what the reference pickles
    (tests/golden/g15_p6_skeleton.json): class paths (C2 among them), plain attributes, parameters and children."""
    from test_host_cpu import _written_skeleton
    from dedark_yolo_amd.utils.checkpoint import reference_module_object
    with open(os.path.join(GOLD, "g15_p6_skeleton.json")) as f:
        want = json.load(f)["p6_n"]
    obj = reference_module_object(_model(GRAPHS["p6"], "n"), None, True, dict(box=7.5, cls=0.5, dfl=1.5, lrl=2.0))
    got = _written_skeleton(obj)
    bad, seen = [], set()

    def walk(a, b, path):
        seen.add(a["cls"])
        if a["cls"] != b["cls"]:
            bad.append((path, "class", a["cls"], b["cls"]))
        for k in set(a["attrs"]) | set(b["attrs"]):
            if k == "yaml":
                continue
            if a["attrs"].get(k, "<absent>") != b["attrs"].get(k, "<absent>"):
                bad.append((path, k, a["attrs"].get(k, "<absent>"), b["attrs"].get(k, "<absent>")))
        for f_ in ("params", "buffers"):
            if a[f_] != b[f_]:
                bad.append((path, f_, a[f_], b[f_]))
        if list(a["children"]) != list(b["children"]):
            bad.append((path, "children", list(a["children"]), list(b["children"])))
        for k, c in a["children"].items():
            if c is not None and b["children"].get(k) is not None:
                walk(c, b["children"][k], path + "." + k)
    walk(want, got, "p6_n")
    assert not bad, bad[:10]
    assert any(c.endswith("C2") for c in seen), sorted(seen)


def test_p6_rejects_an_image_size_that_is_not_a_multiple_of_64():
    import torch
    m = _model(GRAPHS["p6"], "n")
    with pytest.raises(ValueError, match="multiple of the model's largest stride 64"):
        m._check_imgsz(torch.empty(1, 3, 96, 128))
    m._check_imgsz(torch.empty(1, 3, 128, 192))
