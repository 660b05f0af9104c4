"""The SCConv C2f family on the CPU (no GPU needed): the yolov8-SCC2f.yaml graph, state_dict layout, optimizer groups and checkpoint
skeleton against fixtures captured from the reference (tests/golden/make_scc2f_golden.py), and the block fixtures against the
plain-torch float64 statements of tests/scc2f_ref.py, which pins the yardstick the GPU kernel tests measure against."""
import json
import os

import numpy as np
import pytest
import torch

import scc2f_ref as sc
import scconv_ref as sr
from util import GOLD, gold, load_yaml, rnd

YAML = "yolov8-SCC2f.yaml"


def _cfg(scale, block="SCC2f"):
    cfg = load_yaml(YAML)
    cfg["scale"] = scale
    for row in cfg["backbone"] + cfg["head"]:
        if row[2] == "SCC2f":
            row[2] = block
    return cfg


def _model(scale, block="SCC2f", nc=20):
    from dedark_yolo_amd.nn.tasks import DetectionModel
    return DetectionModel(_cfg(scale, block), nc=nc)


@pytest.mark.parametrize("scale", "nml")
def test_scc2f_graph_matches_the_reference(scale):
    """parse_model of yolov8{n,m,l}-SCC2f.yaml: keys, shapes, counts and the three optimizer groups of the reference's model"""
    z = np.load(os.path.join(GOLD, "g28_scc2f_keys.npz"))
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


@pytest.mark.parametrize("block", ["SC_PW_C2f", "SC_Conv3_C2f", "Conv3_SC_C2f"])
def test_yaml_variants_build_from_a_dict(block):
    z = np.load(os.path.join(GOLD, "g28_scc2f_keys.npz"))
    m = _model("n", block)
    assert list(m.state_dict().keys()) == list(z[f"n_{block}_keys"])
    assert sum(q.numel() for q in m.parameters()) == int(z[f"n_{block}_n_params"])


@pytest.mark.parametrize("scale", "nsmlx")
def test_scc2f_yaml_builds_at_every_scale(scale):
    from dedark_yolo_amd.nn.modules import SCC2f, SCConv
    m = _model(scale)
    assert sum(isinstance(L, SCC2f) for L in m.model) == 4
    widths = sorted({s.c for s in m.modules() if isinstance(s, SCConv)})
    assert widths == dict(n=[16, 32, 64, 128], s=[32, 64, 128, 256], m=[48, 96, 192, 288], l=[64, 128, 256], x=[80, 160, 320])[scale]
    # widths that are no multiple of 64 run the CRU on the dy_cru_conv_* kernels, the others keep MFRU's composed path
    assert all(s._cru == (s.c % 64 != 0) for s in m.modules() if isinstance(s, SCConv))


def test_scale_prefixed_name_resolves_and_task_is_detect():
    from dedark_yolo_amd import YOLO
    from dedark_yolo_amd.nn.tasks import yaml_model_load
    d = yaml_model_load("yolov8m-SCC2f.yaml")
    assert d["scale"] == "m" and [r[2] for r in d["backbone"]].count("SCC2f") == 4 and all(r[2] != "SCC2f" for r in d["head"])
    assert YOLO("yolov8n-SCC2f.yaml").task == "detect"


def test_registry_holds_the_family_and_keys_follow_the_reference_nesting():
    from dedark_yolo_amd.nn import modules
    from dedark_yolo_amd.nn.tasks import _REGISTRY
    for name in sc.BOTTLENECKS + tuple(sc.C2FS):
        assert _REGISTRY[name] is getattr(modules, name)
    assert "SC_PW_PW_C2f" not in _REGISTRY and "SC_PW_PW_Bottleneck" not in _REGISTRY
    k = set(modules.SCConvBottleneck(16, 16).state_dict())
    assert {"SandCRblock.0.SRU.gn.weight", "SandCRblock.0.SRU.gn.bias", "SandCRblock.0.CRU.GWC.bias", "SandCRblock.0.CRU.PWC1.weight",
            "SandCRblock.1.conv.weight", "SandCRblock.1.bn.running_var"} <= k
    k = modules.SC_PW_Bottleneck(48, 48).state_dict()
    assert tuple(k["SandCRblock.1.weight"].shape) == (48, 48, 1, 1) and tuple(k["SandCRblock.1.bias"].shape) == (48,)
    assert not any(".bn." in s for s in k)
    k = modules.Conv3_SC_Bottleneck(16, 16).state_dict()
    assert tuple(k["SandCRblock.0.conv.weight"].shape) == (16, 16, 3, 3) and tuple(k["SandCRblock.1.CRU.GWC.weight"].shape) == (16, 2, 3, 3)
    assert tuple(modules.SC_Conv3_C2f(32, 32, 2).state_dict()["m.1.SandCRblock.1.conv.weight"].shape) == (16, 16, 3, 3)


def test_what_stays_out_of_scope_raises():
    from dedark_yolo_amd.nn import modules
    from dedark_yolo_amd.nn.tasks import DetectionModel
    assert modules.SCConv(48)._cru and not modules.SCConv(64)._cru
    for c in (8, 24, 40, 2064):
        with pytest.raises(NotImplementedError, match="multiple of 16"):
            modules.SCConv(c)
    with pytest.raises(NotImplementedError, match="0.5 gate"):
        modules.SCConv(48, gate_treshold=0.4)
    with pytest.raises(NotImplementedError, match="default split"):
        modules.SCConv(48, alpha=1 / 4)
    with pytest.raises(NotImplementedError, match="grouped convolution"):
        modules.SCConvBottleneck(16, 16, g=2)
    with pytest.raises(NotImplementedError, match="SC_PW_PW_C2f"):
        DetectionModel(_cfg("n", "SC_PW_PW_C2f"), nc=20)


@pytest.mark.parametrize("cls,c,shortcut", sc.BLOCK_CASES, ids=[sc.block_name(*k)[10:] for k in sc.BLOCK_CASES])
def test_scc2f_ref_reproduces_the_block_fixture(cls, c, shortcut):
    """the plain-torch statement (conv2d(groups=2) + 1x1 + cat for the CRU), in f64 on the fixture's weights and input, gives the
    reference's output, input gradient and parameter gradients within 1e-5 of the largest value (of the output, of the input
    gradient, of all parameter gradients taken together: test_ghost_cpu's measure); the fixture's input has no ambiguous SRU element
    and the statement's gate margins are the generator's"""
    from oracle import model as om
    from dedark_yolo_amd.nn import modules
    name, args = sc.block_name(cls, c, shortcut), sc.block_args(cls, c, shortcut)
    g = gold(name)
    with open(os.path.join(GOLD, "g28_scc2f_blocks.json")) as f:
        law = json.load(f)[name]
    assert int(g["seed"]) == law["seed"] and law["n_ambiguous"] == 0 and law["flips"] == 0 and law["share"] <= sr.SHARE_CAP
    shapes = {k: tuple(v.shape) for k, v in getattr(modules, cls)(*args).state_dict().items()}
    sd = {k: (v.double().requires_grad_(v.is_floating_point() and "running" not in k) if v.is_floating_point() else v)
          for k, v in om.rng_fill(shapes, int(g["seed"])).items()}
    x = g["x0"].double().requires_grad_(True)
    assert float(g["x0"].abs().max()) <= 4.0
    gates = []
    y = sc.block(cls, args, sd, x, True, gates)
    (y * rnd(900, *y.shape, lo=-1, hi=1).double()).sum().backward()
    assert len(gates) == law["n_sru"]
    for gn, t in gates:
        assert int((gn.abs() < sr.AMBIG).sum()) == 0 and float(t.abs().min()) >= sr.MARGIN

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
        elif k.startswith("gn:"):
            near(sd[k[3:]].grad.norm(), v, k)              # (a norm of a large tensor: against itself)
    assert n >= 8


def test_cru_conv_statement_is_its_own_adjoint():
    """the data- and weight-gradient statements the kernel tests use are autograd's of the forward statement"""
    g = np.random.default_rng(5)
    for G, N, C3, C1 in ((2, 24, 6, 12), (1, 12, 0, 24)):
        x = torch.from_numpy(g.standard_normal((2, C1, 5, 7))).requires_grad_(True)
        w3 = torch.from_numpy(g.standard_normal((G * N, C3, 3, 3))).requires_grad_(True) if C3 else None
        b = torch.from_numpy(g.standard_normal(G * N)).requires_grad_(True) if C3 else None
        w1 = torch.from_numpy(g.standard_normal((G * N, C1, 1, 1))).requires_grad_(True)
        dy = torch.from_numpy(g.standard_normal((2, G * N, 5, 7)))
        (sc.cru_conv_ref(x, w3, b, w1, G) * dy).sum().backward()
        dx = sc.cru_conv_dgrad_ref(dy, None if w3 is None else w3.detach(), w1.detach(), G, x.shape)
        dw3, db, dw1 = sc.cru_conv_wgrad_ref(x.detach(), dy, None if w3 is None else w3.shape, w1.shape, G)
        assert torch.allclose(dx, x.grad, 1e-12, 1e-12) and torch.allclose(dw1, w1.grad, 1e-12, 1e-12)
        if C3:
            assert torch.allclose(dw3, w3.grad, 1e-12, 1e-12) and torch.allclose(db, b.grad, 1e-12, 1e-12)


def test_reference_checkpoint_writer_layout_for_the_scc2f_graph():
    """save_reference_checkpoint's object tree for yolov8n-SCC2f is, module by module, what the reference pickles
    (tests/golden/g28_scc2f_skeleton.json), and so is one block of each of the other three variants"""
    from test_host_cpu import _written_skeleton
    from dedark_yolo_amd.utils.checkpoint import reference_module_object
    with open(os.path.join(GOLD, "g28_scc2f_skeleton.json")) as f:
        skel = json.load(f)
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
    walk(skel["n"], _written_skeleton(reference_module_object(_model("n"), None, True, dict(box=7.5, cls=0.5, dfl=1.5, lrl=2.0))), "n")
    for blk in ("SC_PW_C2f", "SC_Conv3_C2f", "Conv3_SC_C2f"):
        whole = _written_skeleton(reference_module_object(_model("n", blk), None, True, dict(box=7.5, cls=0.5, dfl=1.5, lrl=2.0)))
        walk(skel[blk], whole["children"]["model"]["children"]["2"], blk)
    assert not bad, bad[:10]
    assert {"ultralytics.nn.modules.block.SCC2f", "ultralytics.nn.modules.block.SCConvBottleneck", "ultralytics.nn.modules.conv.SCConv",
            "ultralytics.nn.modules.block.SC_PW_C2f", "ultralytics.nn.modules.block.SC_PW_Bottleneck",
            "ultralytics.nn.modules.block.SC_Conv3_C2f", "ultralytics.nn.modules.block.SC_Conv3_Bottleneck",
            "ultralytics.nn.modules.block.Conv3_SC_C2f", "ultralytics.nn.modules.block.Conv3_SC_Bottleneck"} <= seen


def test_scc2f_checkpoint_round_trip(tmp_path):
    from dedark_yolo_amd.utils.checkpoint import _REF_HOME, load_checkpoint, save_reference_checkpoint
    for name in sc.BOTTLENECKS + tuple(sc.C2FS):
        assert _REF_HOME[name] == "ultralytics.nn.modules.block"
    m = _model("n")
    path = save_reference_checkpoint(str(tmp_path / "last.pt"), m, epoch=0, train_args=dict(imgsz=64))
    import zipfile
    with zipfile.ZipFile(path) as zf:
        pkl = zf.read([n for n in zf.namelist() if n.endswith("data.pkl")][0])
    for needle in (b"ultralytics.nn.modules.block\nSCC2f", b"ultralytics.nn.modules.block\nSCConvBottleneck", b"ultralytics.nn.modules.conv\nSCConv"):
        assert needle in pkl, needle
    assert b"dedark_yolo_amd" not in pkl
    ck = load_checkpoint(path)
    sd = m.state_dict()
    assert list(ck.state_dict) == list(sd)
    for k, v in sd.items():
        assert torch.equal(ck.state_dict[k], v.half().float() if v.is_floating_point() else v), k
