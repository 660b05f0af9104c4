"""FasterNet variants on the CPU (no GPU needed): yaml graphs, state_dict layout, optimizer groups and the checkpoint skeleton of
yolov8-Faster-2.0.yaml / yolov8-Faster3.0-twohead.yaml against fixtures captured from the reference (tests/golden/make_faster_golden.py)."""
import json
import os

import numpy as np
import pytest
import torch

from util import GOLD, load_yaml

GRAPHS = {"f2": "yolov8-Faster-2.0.yaml", "f3": "yolov8-Faster3.0-twohead.yaml"}


def _model(name, scale, nc=20):
    from dedark_yolo_amd.nn.tasks import DetectionModel
    cfg = load_yaml(name)
    cfg["scale"] = scale
    return DetectionModel(cfg, nc=nc)


@pytest.mark.parametrize("name", sorted(GRAPHS.values()))
@pytest.mark.parametrize("scale", "nsmlx")
def test_faster_yamls_build_at_every_scale(name, scale):
    from dedark_yolo_amd.nn.modules import FasterC2f_N, PConv
    m = _model(name, scale)
    blocks = [L for L in m.model if isinstance(L, FasterC2f_N)]
    assert len(blocks) == (8 if "Faster-2.0" in name else 7)
    for b in blocks:
        for pc in (mod for mod in b.modules() if isinstance(mod, PConv)):
            assert pc.dim_conv3 == b.c // 4 and pc.dim_untouched == b.c - b.c // 4 and 1 <= pc.dim_conv3 <= 128


def test_scale_prefixed_names_resolve():
    from dedark_yolo_amd.nn.tasks import yaml_model_load
    d = yaml_model_load("yolov8l-Faster-2.0.yaml")
    assert d["scale"] == "l" and d["backbone"][2][2] == "FasterC2f_N"
    d = yaml_model_load("yolov8n-Faster3.0-twohead.yaml")
    assert d["scale"] == "n" and d["head"][-1][2] == "AsffDetect"


@pytest.mark.parametrize("tag,scale", [("f2", "n"), ("f2", "l"), ("f3", "l")])
def test_state_dict_counts_and_optimizer_groups_match_the_reference(tag, scale):
    z = np.load(os.path.join(GOLD, "g14_faster_keys.npz"))
    p = f"{tag}_{scale}_"
    m = _model(GRAPHS[tag], scale)
    sd = m.state_dict()
    assert list(sd.keys()) == list(z[p + "keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(z[p + "shapes"])
    assert sum(q.numel() for q in m.parameters()) == int(z[p + "n_params"])
    assert len(m.model) == int(z[p + "n_layers"])
    assert [L.np for L in m.model] == [int(v) for v in z[p + "layer_np"]]
    # the groups the trainer itself builds (FlatState + DetectionTrainer._param_order, the numbering of its optimizer state_dict)
    # against the reference's build_optimizer groups (decayed weights, BatchNorm weights, biases)
    from types import SimpleNamespace
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, FlatState
    _, sizes = DetectionTrainer._param_order(SimpleNamespace(flat=FlatState(m, with_ema=False)))
    bias, decayed, bn_w = sizes
    # the reference also hands the frozen DFL projection (requires_grad=False, never stepped) to its decayed group; the trainer's
    # flat state holds trainable parameters only
    frozen = [k for k, q in m.named_parameters() if not q.requires_grad]
    assert frozen == [k for k in sd if k.endswith(".dfl.conv.weight")]
    assert [decayed + len(frozen), bn_w, bias] == [int(v) for v in z[p + "opt_groups"]]


def test_block_keys_follow_the_reference_nesting():
    from dedark_yolo_amd.nn.modules import FasterC2f, FasterC2f_N
    k = set(FasterC2f_N(32, 32, 1, True).state_dict())
    assert {"m.0.fasterblock.0.patial_conv3.weight", "m.0.fasterblock.1.conv.weight", "m.0.fasterblock.1.bn.running_var",
            "m.0.fasterblock.2.weight"} <= k
    k = set(FasterC2f(32, 32, 1, True).state_dict())
    assert {"m.0.fasterblock.0.patial_conv3.weight", "m.0.fasterblock.1.conv.weight", "m.0.conv.weight"} <= k
    assert tuple(FasterC2f(32, 32, 1).state_dict()["m.0.fasterblock.1.conv.weight"].shape) == (16, 16, 3, 3)


def test_pconv_rejects_the_slicing_mode():
    from dedark_yolo_amd.nn.modules import PConv
    with pytest.raises(NotImplementedError):
        PConv(32, 4, forward="slicing")


@pytest.mark.parametrize("tag", ["f2_n", "f3_l"])
def test_reference_checkpoint_writer_layout_for_faster_graphs(tag):
    """save_reference_checkpoint's object tree for a Faster graph is, module by module, what the reference pickles
    (tests/golden/g14_faster_skeleton.json): class paths (PConv, PconvBottleneck_n, FasterC2f_N), plain attributes (dim_conv3,
    dim_untouched, add, c), parameters and children.  PConv's per-instance `forward` is a bound method there: the writer must store
    getattr(<the PConv object>, 'forward_split_cat')."""
    from test_host_cpu import _written_skeleton
    from dedark_yolo_amd.utils.checkpoint import _RefMethod, reference_module_object
    with open(os.path.join(GOLD, "g14_faster_skeleton.json")) as f:
        want = json.load(f)[tag]
    name, scale = GRAPHS[tag[:2]], tag[3:]
    obj = reference_module_object(_model(name, scale), None, True, dict(box=7.5, cls=0.5, dfl=1.5, lrl=2.0))
    got = _written_skeleton(obj)
    bad, n_pconv = [], [0]

    def check_method(o):
        if type(o).__qualname__ == "PConv":
            n_pconv[0] += 1
            fm = o.__dict__.get("forward")
            red = fm.__reduce__() if isinstance(fm, _RefMethod) else None
            if red is None or red[0] is not getattr or red[1][0] is not o or red[1][1] != "forward_split_cat":
                bad.append(("PConv.forward", red))
        for c in o.__dict__.get("_modules", {}).values():
            if c is not None:
                check_method(c)

    def walk(a, b, path):
        if a["cls"] != b["cls"]:
            bad.append((path, "class", a["cls"], b["cls"]))
        for k in set(a["attrs"]) | set(b["attrs"]):
            if k in ("yaml", "forward"):
                continue
            if a["attrs"].get(k, "<absent>") != b["attrs"].get(k, "<absent>"):
                bad.append((path, k, a["attrs"].get(k, "<absent>"), b["attrs"].get(k, "<absent>")))
        if ("forward" in a["attrs"]) != ("forward" in b["attrs"]):
            bad.append((path, "forward attribute"))
        for f_ in ("params", "buffers"):
            if a[f_] != b[f_]:
                bad.append((path, f_, a[f_], b[f_]))
        if list(a["children"]) != list(b["children"]):
            bad.append((path, "children", list(a["children"]), list(b["children"])))
        for k, c in a["children"].items():
            if c is not None and b["children"].get(k) is not None:
                walk(c, b["children"][k], path + "." + k)
    walk(want, got, tag)
    check_method(obj)
    assert not bad, bad[:10]
    assert n_pconv[0] > 0


def test_faster_checkpoint_names_reference_classes(tmp_path):
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint, save_reference_checkpoint
    cfg = load_yaml("yolov8-Faster-2.0.yaml")
    cfg["scales"]["t"] = [0.33, 0.125, 1024]
    cfg["scale"] = "t"
    from dedark_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(cfg, nc=20)
    path = save_reference_checkpoint(str(tmp_path / "last.pt"), m, epoch=0, train_args=dict(imgsz=64))
    import zipfile
    with zipfile.ZipFile(path) as zf:
        pkl = zf.read([n for n in zf.namelist() if n.endswith("data.pkl")][0])
    for needle in (b"ultralytics.nn.modules.conv\nPConv", b"ultralytics.nn.modules.block\nPconvBottleneck_n",
                   b"ultralytics.nn.modules.block\nFasterC2f_N", b"forward_split_cat"):
        assert needle in pkl, needle
    assert b"dedark_yolo_amd" not in pkl
    ck = load_checkpoint(path)
    sd = m.state_dict()
    assert list(ck.state_dict) == list(sd)
    for k, v in sd.items():
        assert torch.equal(ck.state_dict[k], v.half().float() if v.is_floating_point() else v), k
