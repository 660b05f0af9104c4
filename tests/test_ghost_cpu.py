"""Ghost variants on the CPU (no GPU needed): the yolov8-ghost.yaml graph, state_dict layout, optimizer groups and checkpoint skeleton
against fixtures captured from the reference (tests/golden/make_ghost_golden.py), and the block fixtures against the plain-torch
statements of tests/ghost_ref.py."""
import json
import os

import numpy as np
import pytest
import torch

import ghost_ref
from util import GOLD, gold, load_yaml, rnd

YAML = "yolov8-ghost.yaml"


def _model(scale, nc=20):
    from dedark_yolo_amd.nn.tasks import DetectionModel
    cfg = load_yaml(YAML)
    cfg["scale"] = scale
    return DetectionModel(cfg, nc=nc)


@pytest.mark.parametrize("scale", "nl")
def test_ghost_graph_matches_the_reference(scale):
    """parse_model of yolov8{n,l}-ghost.yaml: keys, shapes, counts and optimizer groups of the reference's model"""
    z = np.load(os.path.join(GOLD, "g25_ghost_keys.npz"))
    p = f"{scale}_"
    m = _model(scale)
    sd = m.state_dict()
    assert list(sd.keys()) == list(z[p + "keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(z[p + "shapes"])
    assert sum(q.numel() for q in m.parameters()) == int(z[p + "n_params"])
    assert len(m.model) == int(z[p + "n_layers"])
    assert [L.np for L in m.model] == [int(v) for v in z[p + "layer_np"]]
    assert [float(v) for v in m.stride] == [float(v) for v in z[p + "stride"]]
    from types import SimpleNamespace
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, FlatState
    _, sizes = DetectionTrainer._param_order(SimpleNamespace(flat=FlatState(m, with_ema=False)))
    bias, decayed, bn_w = sizes
    frozen = [k for k, q in m.named_parameters() if not q.requires_grad]      # the DFL projection: in the reference's decayed group
    assert frozen == [k for k in sd if k.endswith(".dfl.conv.weight")]
    assert [decayed + len(frozen), bn_w, bias] == [int(v) for v in z[p + "opt_groups"]]


@pytest.mark.parametrize("scale", "nsmlx")
def test_ghost_yaml_builds_at_every_scale(scale):
    from dedark_yolo_amd.nn.modules import C3Ghost, Conv, GhostConv
    m = _model(scale)
    assert sum(isinstance(L, C3Ghost) for L in m.model) == 8 and sum(isinstance(L, GhostConv) for L in m.model) == 6
    dw = [c for c in m.modules() if isinstance(c, Conv) and c.conv.groups > 1]
    assert dw and all(c.conv.groups == c.conv.in_channels == c.conv.out_channels and c.conv.kernel_size == (5, 5) for c in dw)


def test_scale_prefixed_name_resolves_and_task_is_detect():
    from dedark_yolo_amd import YOLO
    from dedark_yolo_amd.nn.tasks import yaml_model_load
    d = yaml_model_load("yolov8n-ghost.yaml")
    assert d["scale"] == "n" and d["backbone"][1][2] == "GhostConv" and d["backbone"][2][2] == "C3Ghost"
    assert YOLO("yolov8n-ghost.yaml").task == "detect"


def test_block_keys_follow_the_reference_nesting():
    from dedark_yolo_amd.nn.modules import C3, C3Ghost, GhostBottleneck
    k = list(GhostBottleneck(16, 32, 3, 2).state_dict())
    assert {"conv.0.cv1.conv.weight", "conv.0.cv2.bn.running_var", "conv.1.conv.weight", "conv.2.cv2.conv.weight",
            "shortcut.0.conv.weight", "shortcut.1.bn.weight"} <= set(k)
    k = set(GhostBottleneck(16, 16).state_dict())
    assert "conv.2.cv1.conv.weight" in k and not any(s.startswith(("conv.1.", "shortcut.")) for s in k)     # nn.Identity keeps conv.2
    assert tuple(C3Ghost(32, 32, 1).state_dict()["m.0.conv.0.cv2.conv.weight"].shape) == (4, 1, 5, 5)
    assert tuple(C3(32, 32, 1).state_dict()["m.0.cv1.conv.weight"].shape) == (16, 16, 1, 1)


def test_unsupported_groupings_raise():
    from dedark_yolo_amd.nn.modules import Conv, DWConv, PconvBottleneck
    with pytest.raises(NotImplementedError, match="grouped convolution is outside the Dedark-YOLO hot path"):
        DWConv(8, 12)                                  # g = 4: a channel multiplier
    with pytest.raises(NotImplementedError, match="grouped convolution is outside the Dedark-YOLO hot path"):
        Conv(8, 8, 3, 1, g=2)                          # c1 != g
    with pytest.raises(NotImplementedError, match="grouped convolution is outside the Dedark-YOLO hot path"):
        Conv(8, 8, 3, 1, g=8, d=2)                     # dilation
    with pytest.raises(NotImplementedError, match="grouped convolution is outside the Dedark-YOLO hot path"):
        PconvBottleneck(16, 16, g=2)
    assert DWConv(8, 8, 3, 2).conv.groups == 8 and Conv(8, 8, 5, 1, g=8).conv.padding == (2, 2)


@pytest.mark.parametrize("name", sorted(ghost_ref.BLOCKS))
def test_ghost_ref_reproduces_the_block_fixture(name):
    """the plain-torch statement, in f64 on the fixture's weights and input, gives the reference's output, input gradient and parameter
    gradients within 1e-5 of the largest value: of the output, of the input gradient, and of all parameter gradients of the block taken
    together (a bias in front of another BatchNorm has an analytically zero gradient; the fixture holds the reference's fp32 rounding
    noise there, ~1e-6 next to gradients of order 1, which is no scale to measure against)"""
    from oracle import model as om
    from dedark_yolo_amd.nn import modules
    g = gold("g25_ghost_" + name)
    cls, args, fn = ghost_ref.BLOCKS[name]
    shapes = {k: tuple(v.shape) for k, v in getattr(modules, cls)(*args).state_dict().items()}
    sd = {k: (v.double().requires_grad_(v.is_floating_point() and "running" not in k) if v.is_floating_point() else v)
          for k, v in om.rng_fill(shapes, int(g["seed"])).items()}
    x = g["x0"].double().requires_grad_(True)
    y = fn(sd, x)
    (y * rnd(900, *y.shape, lo=-1, hi=1).double()).sum().backward()

    def near(a, b, what, top=None):
        err, top = float((a.double() - b.double()).abs().max()), float(b.abs().max()) if top is None else top
        assert err <= 1e-5 * max(top, 1e-30), f"{name} {what}: {err:.3e} vs max {top:.3e}"
    near(y.detach(), g["y0"], "y")
    near(x.grad, g["dx0"], "dx")
    gtop = max(float(v.abs().max()) for k, v in g.items() if k.startswith("g:"))
    n = 0
    for k, v in g.items():
        if k.startswith("g:"):
            near(sd[k[2:]].grad, v, k, gtop)
            n += 1
    assert n >= 3
    if cls == "DWConv":
        rm, rv = ghost_ref.running_stats({k: v.detach() for k, v in sd.items()}, "", x.detach(), 2)
        near(rm, g["b:bn.running_mean"], "running_mean")
        near(rv, g["b:bn.running_var"], "running_var")


def test_reference_checkpoint_writer_layout_for_the_ghost_graph():
    """save_reference_checkpoint's object tree for yolov8n-ghost is, module by module, what the reference pickles
    (tests/golden/g25_ghost_skeleton.json): class paths (GhostConv, GhostBottleneck, C3Ghost, DWConv is not in this graph), plain
    attributes, parameters, buffers and children -- nn.Identity at conv.1 and shortcut included."""
    from test_host_cpu import _written_skeleton
    from dedark_yolo_amd.utils.checkpoint import reference_module_object
    with open(os.path.join(GOLD, "g25_ghost_skeleton.json")) as f:
        want = json.load(f)["n"]
    got = _written_skeleton(reference_module_object(_model("n"), None, True, dict(box=7.5, cls=0.5, dfl=1.5, lrl=2.0)))
    bad, seen = [], set()

    def walk(a, b, path):
        seen.add(a["cls"])
        if a["cls"] != b["cls"]:
            bad.append((path, "class", a["cls"], b["cls"]))
        for k in set(a["attrs"]) | set(b["attrs"]):
            if k != "yaml" and a["attrs"].get(k, "<absent>") != b["attrs"].get(k, "<absent>"):
                bad.append((path, k, a["attrs"].get(k, "<absent>"), b["attrs"].get(k, "<absent>")))
        for f_ in ("params", "buffers"):
            if a[f_] != b[f_]:
                bad.append((path, f_, a[f_], b[f_]))
        if list(a["children"]) != list(b["children"]):
            bad.append((path, "children", list(a["children"]), list(b["children"])))
        for k, c in a["children"].items():
            if c is not None and b["children"].get(k) is not None:
                walk(c, b["children"][k], path + "." + k)
    walk(want, got, "n")
    assert not bad, bad[:10]
    assert {"ultralytics.nn.modules.conv.GhostConv", "ultralytics.nn.modules.block.GhostBottleneck",
            "ultralytics.nn.modules.block.C3Ghost", "torch.nn.modules.linear.Identity"} <= seen


def test_ghost_checkpoint_names_reference_classes(tmp_path):
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint, save_reference_checkpoint
    m = _model("n")
    path = save_reference_checkpoint(str(tmp_path / "last.pt"), m, epoch=0, train_args=dict(imgsz=64))
    import zipfile
    with zipfile.ZipFile(path) as zf:
        pkl = zf.read([n for n in zf.namelist() if n.endswith("data.pkl")][0])
    for needle in (b"ultralytics.nn.modules.conv\nGhostConv", b"ultralytics.nn.modules.block\nGhostBottleneck",
                   b"ultralytics.nn.modules.block\nC3Ghost"):
        assert needle in pkl, needle
    assert b"dedark_yolo_amd" not in pkl
    ck = load_checkpoint(path)
    sd = m.state_dict()
    assert list(ck.state_dict) == list(sd)
    for k, v in sd.items():
        assert torch.equal(ck.state_dict[k], v.half().float() if v.is_floating_point() else v), k


def test_standalone_classes_have_checkpoint_homes():
    from dedark_yolo_amd.utils.checkpoint import _REF_HOME
    assert _REF_HOME["GhostConv"] == _REF_HOME["DWConv"] == "ultralytics.nn.modules.conv"
    assert _REF_HOME["GhostBottleneck"] == _REF_HOME["C3"] == _REF_HOME["C3Ghost"] == "ultralytics.nn.modules.block"
