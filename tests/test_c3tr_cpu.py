"""The transformer variant on the CPU (no GPU needed): the yolov8-C3TR.yaml graph, state_dict layout, optimizer groups and checkpoint
skeleton against fixtures captured from the reference (tests/golden/make_c3tr_golden.py), and tests/attn_ref.py, the float64
yardstick of the GPU kernel tests, against torch.nn.functional.multi_head_attention_forward in float64 (forward and autograd)."""
import json
import os

import numpy as np
import pytest
import torch

import attn_ref as ar
from util import GOLD, load_yaml

YAML = "yolov8-C3TR.yaml"


def _cfg(scale):
    cfg = load_yaml(YAML)
    cfg["scale"] = scale
    return cfg


def _model(scale, nc=20):
    from dedark_yolo_amd.nn.tasks import DetectionModel
    return DetectionModel(_cfg(scale), nc=nc)


@pytest.mark.parametrize("scale", "nml")
def test_c3tr_graph_matches_the_reference(scale):
    """parse_model of yolov8{n,m,l}-C3TR.yaml: keys, shapes, counts and the three optimizer groups of the reference's model
    (ma.in_proj_bias is a `bias` name: the no-decay group)"""
    z = np.load(os.path.join(GOLD, "g29_c3tr_keys.npz"))
    p = f"{scale}_"
    m = _model(scale)
    sd = m.state_dict()
    assert list(sd.keys()) == list(z[p + "keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(z[p + "shapes"])
    assert sum(q.numel() for q in m.parameters()) == int(z[p + "n_params"])
    assert len(m.model) == int(z[p + "n_layers"])
    assert [L.np for L in m.model] == [int(v) for v in z[p + "layer_np"]]
    assert [float(v) for v in m.stride] == [float(v) for v in z[p + "stride"]]
    tr = m.model[8].m.tr
    assert [tr[0].ma.num_heads, tr[0].ma.head_dim, len(tr)] == [int(v) for v in z[p + "heads_dim"]]
    from types import SimpleNamespace
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, FlatState
    flat = FlatState(m, with_ema=False)
    _, sizes = DetectionTrainer._param_order(SimpleNamespace(flat=flat))
    bias, decayed, bn_w = sizes
    frozen = [k for k, q in m.named_parameters() if not q.requires_grad]
    assert [decayed + len(frozen), bn_w, bias] == [int(v) for v in z[p + "opt_groups"]]
    gid = {id(q): g for q, _, _, g in flat.slots}
    assert gid[id(tr[0].ma.in_proj_bias)] == 2 and gid[id(tr[0].ma.out_proj.bias)] == 2 and gid[id(m.model[8].m.linear.bias)] == 2
    assert gid[id(tr[0].ma.in_proj_weight)] == 0 and gid[id(tr[0].q.weight)] == 0


@pytest.mark.parametrize("scale", "nsmlx")
def test_c3tr_yaml_builds_at_every_scale(scale):
    from dedark_yolo_amd.nn.modules import C3TR, TransformerBlock, TransformerLayer
    m = _model(scale)
    assert [i for i, L in enumerate(m.model) if isinstance(L, C3TR)] == [8]
    blk = m.model[8].m
    assert isinstance(blk, TransformerBlock) and blk.conv is None and all(isinstance(t, TransformerLayer) for t in blk.tr)
    width, dim, layers = dict(n=(128, 32, 1), s=(256, 64, 1), m=(288, 72, 2), l=(256, 64, 3), x=(320, 80, 3))[scale]
    assert (blk.c2, blk.tr[0].ma.head_dim, len(blk.tr)) == (width, dim, layers) and blk.tr[0].ma.num_heads == 4


def test_scale_prefixed_name_resolves_and_registry():
    from dedark_yolo_amd import YOLO
    from dedark_yolo_amd.nn import modules
    from dedark_yolo_amd.nn.tasks import _REGISTRY, yaml_model_load
    d = yaml_model_load("yolov8m-C3TR.yaml")
    assert d["scale"] == "m" and d["backbone"][8] == [-1, 3, "C3TR", [1024]]
    assert YOLO("yolov8n-C3TR.yaml").task == "detect"
    assert _REGISTRY["C3TR"] is modules.C3TR
    keys = set(modules.C3TR(64, 64, 2).state_dict())
    assert {"m.linear.weight", "m.linear.bias", "m.tr.1.q.weight", "m.tr.1.k.weight", "m.tr.1.v.weight", "m.tr.0.ma.in_proj_weight",
            "m.tr.0.ma.in_proj_bias", "m.tr.0.ma.out_proj.weight", "m.tr.0.ma.out_proj.bias", "m.tr.0.fc1.weight", "m.tr.0.fc2.weight",
            "cv3.bn.running_var"} <= keys
    assert "conv.conv.weight" in modules.TransformerBlock(16, 32, 4, 1).state_dict()
    # torch's own load_state_dict takes the reference's tensors
    ref = torch.nn.MultiheadAttention(32, 4).state_dict()
    modules.TransformerLayer(32, 4).ma.load_state_dict(ref, strict=True)


def test_what_stays_out_of_scope_raises():
    from dedark_yolo_amd.nn import modules
    from dedark_yolo_amd.nn.tasks import DetectionModel
    for c2 in (16, 48, 80):                                   # c_ = 8, 24, 40
        with pytest.raises(NotImplementedError, match="multiple of 32"):
            modules.C3TR(c2, c2)
    with pytest.raises(NotImplementedError, match="D % 8 == 0"):
        modules.TransformerLayer(48, 4)                       # D = 12
    with pytest.raises(NotImplementedError, match="D % 8 == 0"):
        modules.TransformerLayer(544, 4)                      # D = 136
    cfg = _cfg("n")
    cfg["backbone"][8][2] = "AIFI"
    with pytest.raises(NotImplementedError, match="AIFI"):
        DetectionModel(cfg, nc=20)


def test_reference_checkpoint_writer_layout_for_the_c3tr_graph():
    """save_reference_checkpoint's object tree for yolov8n-C3TR is, module by module, what the reference pickles
    (tests/golden/g29_c3tr_skeleton.json); so is a TransformerBlock with its inner Conv"""
    from test_host_cpu import _written_skeleton
    from dedark_yolo_amd.nn import modules
    from dedark_yolo_amd.utils.checkpoint import _RefWriter, reference_module_object
    with open(os.path.join(GOLD, "g29_c3tr_skeleton.json")) as f:
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
    tb = modules.TransformerBlock(16, 32, 4, 1)
    walk(skel["tb_conv"], _written_skeleton(_RefWriter(tb.state_dict(), True).convert(tb, "")), "tb_conv")
    assert not bad, bad[:10]
    assert {"ultralytics.nn.modules.block.C3TR", "ultralytics.nn.modules.transformer.TransformerBlock",
            "ultralytics.nn.modules.transformer.TransformerLayer", "torch.nn.modules.activation.MultiheadAttention",
            "torch.nn.modules.linear.NonDynamicallyQuantizableLinear", "torch.nn.modules.linear.Linear"} <= seen


def test_c3tr_checkpoint_round_trip(tmp_path):
    from dedark_yolo_amd.utils.checkpoint import _REF_HOME, load_checkpoint, save_reference_checkpoint
    assert _REF_HOME["C3TR"] == "ultralytics.nn.modules.block" and _REF_HOME["TransformerBlock"] == "ultralytics.nn.modules.transformer"
    m = _model("n")
    path = save_reference_checkpoint(str(tmp_path / "last.pt"), m, epoch=0, train_args=dict(imgsz=64))
    import zipfile
    with zipfile.ZipFile(path) as zf:
        pkl = zf.read([n for n in zf.namelist() if n.endswith("data.pkl")][0])
    for needle in (b"ultralytics.nn.modules.block\nC3TR", b"ultralytics.nn.modules.transformer\nTransformerBlock",
                   b"ultralytics.nn.modules.transformer\nTransformerLayer", b"MultiheadAttention", b"NonDynamicallyQuantizableLinear"):
        assert needle in pkl, needle
    assert b"dedark_yolo_amd" not in pkl
    ck = load_checkpoint(path)                                # the restricted unpickler: torch's attention classes arrive as records
    sd = m.state_dict()
    assert list(ck.state_dict) == list(sd)
    for k, v in sd.items():
        assert torch.equal(ck.state_dict[k], v.half().float() if v.is_floating_point() else v), k
    m2 = _model("n")
    m2.load_state_dict(ck.state_dict, strict=True)


def test_reference_loaded_our_checkpoint():
    """the recorded result of the reference loading a last.pt written here (make_c3tr_golden.py interop): finite outputs of the
    expected shape, fused and unfused within the fuse tolerance"""
    z = np.load(os.path.join(GOLD, "g29_c3tr_interop.npz"))
    assert z["y"].shape == (2, 24, 84) and np.isfinite(z["y"]).all()
    assert float(np.abs(z["y"] - z["y_fused"]).max()) <= 1e-3 * max(1.0, float(np.abs(z["y"]).max()))


@pytest.mark.parametrize("B,L,H,D", [(2, 9, 4, 8), (1, 70, 2, 16), (3, 1, 4, 8)])
def test_attn_ref_is_torchs_multi_head_attention(B, L, H, D):
    """attn_ref.forward / backward on f64 tensors against F.multi_head_attention_forward with identity projections (what is left
    is exactly softmax(q k^T / sqrt(D)) v per head), forward and autograd; the flash-form backward gets O and LSE of the forward"""
    import torch.nn.functional as F
    g = np.random.default_rng(B * 100 + L)
    C = H * D
    q, k, v, do = (torch.from_numpy(g.standard_normal((B, L, C))) for _ in range(4))
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    eye3 = torch.eye(C, dtype=torch.float64).repeat(3, 1)
    out, _ = F.multi_head_attention_forward(q.transpose(0, 1), k.transpose(0, 1), v.transpose(0, 1), C, H, eye3, torch.zeros(3 * C, dtype=torch.float64),
                                            None, None, False, 0.0, torch.eye(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64),
                                            training=True, need_weights=False)
    out = out.transpose(0, 1)
    (out * do).sum().backward()
    qn, kn, vn = (t.detach().numpy() for t in (q, k, v))
    o, lse, p = ar.forward(qn, kn, vn, H)
    assert np.abs(o - out.detach().numpy()).max() <= 1e-13
    assert np.abs(p.sum(-1) - 1).max() <= 1e-13 and lse.shape == (B, H, L)
    dq, dk, dv, _ = ar.backward(qn, kn, vn, o, do.numpy(), lse, H)
    for got, ref in ((dq, q.grad), (dk, k.grad), (dv, v.grad)):
        assert np.abs(got - ref.numpy()).max() <= 1e-13 * max(1.0, float(ref.abs().max()))
    tq, tk, tv = ar.backward_terms(qn, kn, vn, o, do.numpy(), lse, H)
    assert (tq >= np.abs(dq) - 1e-12).all() and (tk >= np.abs(dk) - 1e-12).all() and (tv >= np.abs(dv) - 1e-12).all()
    assert (ar.forward_terms(p, vn, H) >= np.abs(o) - 1e-12).all()
