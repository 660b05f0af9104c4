"""The transformer encoder layer on the CPU (no GPU needed): tests/aifi_ref.py, the float64 yardstick of the GPU kernel tests,
against torch's autograd through nn.LayerNorm / nn.GELU / nn.MultiheadAttention in float64; the host position table against the
reference's; the yolov8-AIFI.yaml graph, state_dict layout, optimizer groups and checkpoint skeleton against fixtures captured from
the reference (tests/golden/make_aifi_golden.py); and the cases that stay out of scope."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import aifi_ref as ar
from util import GOLD, load_yaml

YAML = "yolov8-AIFI.yaml"


def _cfg(scale):
    cfg = load_yaml(YAML)
    cfg["scale"] = scale
    return cfg


def _model(scale, nc=20):
    from dedark_yolo_amd.nn.tasks import DetectionModel
    return DetectionModel(_cfg(scale), nc=nc)


# ---------------------------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("rows,C,with_b", [(5, 8, True), (3, 72, False), (2, 256, True)])
def test_ln_ref_is_torchs_layer_norm(rows, C, with_b):
    g = torch.Generator().manual_seed(rows * 1000 + C)
    a, b, dy, old = (torch.randn(rows, C, dtype=torch.float64, generator=g) for _ in range(4))
    gamma, beta = torch.randn(C, dtype=torch.float64, generator=g), torch.randn(C, dtype=torch.float64, generator=g)
    z = (a + b if with_b else a).clone().requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(z, (C,), gm, bt, 1e-5)
    y.backward(dy)
    bb = b if with_b else None
    y64, mean, rstd = ar.ln_forward(a, bb, gamma, beta, 1e-5)
    assert float((y64 - y.detach()).abs().max()) <= 1e-13
    dz, dg, db = ar.ln_backward(a, bb, mean, rstd, gamma, dy, old)
    for got, ref in ((dz - old, z.grad), (dg, gm.grad), (db, bt.grad)):
        assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    ty, tm, tr = ar.ln_forward_terms(a, bb, gamma, beta, 1e-5)
    assert bool((ty >= y64.abs() - 1e-12).all()) and bool((tm >= mean.abs() - 1e-12).all()) and bool((tr >= rstd).all())
    tdz, tdg, tdb = ar.ln_backward_terms(a, bb, mean, rstd, gamma, dy, old)
    assert bool((tdz >= dz.abs() - 1e-12).all()) and bool((tdg >= dg.abs() - 1e-12).all()) and bool((tdb >= db.abs() - 1e-12).all())


def test_gelu_ref_is_torchs_gelu():
    u = torch.linspace(-10, 10, 4001, dtype=torch.float64).requires_grad_(True)
    dy = torch.cos(torch.arange(4001, dtype=torch.float64))
    y = torch.nn.functional.gelu(u)
    y.backward(dy)
    ud = u.detach()
    assert float((ar.gelu_forward(ud) - y.detach()).abs().max()) <= 1e-15 * 10
    assert float((ar.gelu_backward(ud, dy) - u.grad).abs().max()) <= 1e-14
    assert bool((ar.gelu_forward_terms(ud) >= ar.gelu_forward(ud).abs() - 1e-15).all())
    assert bool((ar.gelu_backward_terms(ud, dy) >= ar.gelu_backward(ud, dy).abs() - 1e-15).all())
    assert float(ar.gelu_forward(torch.tensor([-10.0]))) < 0.0           # no cancellation in the far negative tail


@pytest.mark.parametrize("B,H,W,C,heads,cm,with_pos", [(2, 3, 5, 64, 8, 128, True), (1, 2, 2, 32, 4, 48, True), (2, 3, 3, 64, 4, 128, False)])
def test_layer_ref_is_torch_autograd(B, H, W, C, heads, cm, with_pos):
    """aifi_ref.layer_forward / layer_backward against nn.MultiheadAttention (batch_first) + nn.Linear + nn.GELU + nn.LayerNorm wired
    as the reference's forward_post, in float64, forward and every gradient"""
    torch.manual_seed(B * 100 + C)
    ma = nn.MultiheadAttention(C, heads, batch_first=True).double()
    fc1, fc2, n1, n2, act = nn.Linear(C, cm).double(), nn.Linear(cm, C).double(), nn.LayerNorm(C).double(), nn.LayerNorm(C).double(), nn.GELU()
    mods = dict(ma=ma, fc1=fc1, fc2=fc2, norm1=n1, norm2=n2)
    with torch.no_grad():
        for m in mods.values():
            for p in m.parameters():
                p.copy_(torch.randn_like(p) * 0.3 + (1.0 if p.dim() == 1 and isinstance(m, nn.LayerNorm) else 0.0))
    x = torch.randn(B, H * W, C, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, H * W, C, dtype=torch.float64)
    pos = ar.pos_table(W, H, C).double() if with_pos else None
    q = x if pos is None else x + pos
    src = n1(x + ma(q, q, value=x)[0])
    y = n2(src + fc2(act(fc1(src))))
    y.backward(dy)
    P = {f"{n}.{k}": v.detach() for n, m in mods.items() for k, v in m.state_dict().items()}
    y64, cache = ar.layer_forward(P, x.detach(), pos, heads)
    assert float((y64 - y.detach()).abs().max()) <= 1e-12
    dx, G = ar.layer_backward(cache, dy)
    assert float((dx - x.grad).abs().max()) <= 1e-11 * max(1.0, float(x.grad.abs().max()))
    named = {f"{n}.{k}": p for n, m in mods.items() for k, p in m.named_parameters()}
    assert set(G) == set(named)
    for k, p in named.items():
        assert float((G[k] - p.grad).abs().max()) <= 1e-11 * max(1.0, float(p.grad.abs().max())), k


# ---------------------------------------------------------------------------------------------------------------- position table
@pytest.mark.parametrize("w,h,c", [(3, 5, 64), (20, 20, 256)])
def test_position_table_is_the_references_bit_for_bit(w, h, c):
    from dedark_yolo_amd import ops
    from dedark_yolo_amd.nn.modules import AIFI
    want = torch.from_numpy(np.load(os.path.join(GOLD, "g30_aifi_pos.npz"))[f"pos_{w}_{h}_{c}"])
    got = ops.sincos_pos_table(w, h, c)
    assert got.dtype == torch.float32 and got.shape == (w * h, c)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(AIFI.build_2d_sincos_position_embedding(w, h, c)[0], want)
    assert torch.equal(ar.pos_table(w, h, c), want)
    # the quirk: row p = (iw, ih) = (p // h, p % h)
    p = w * h - 2
    om1 = 1.0 / (10000.0 ** (1.0 / (c // 4)))
    assert abs(float(got[p, 1]) - np.sin((p // h) * om1)) < 1e-6 and abs(float(got[p, c // 2 + 1]) - np.sin((p % h) * om1)) < 1e-6
    assert ops.pos_table(w, h, c, torch.bfloat16, "cpu") is ops.pos_table(w, h, c, torch.bfloat16, "cpu")           # cached
    assert torch.equal(ops.pos_table(w, h, c, torch.float16, "cpu"), want.to(torch.float16))


# ---------------------------------------------------------------------------------------------------------------- graph, registry
@pytest.mark.parametrize("scale", "nml")
def test_aifi_graph_matches_the_reference(scale):
    """parse_model of yolov8{n,m,l}-AIFI.yaml: keys, shapes, counts and the three optimizer groups of the reference's model;
    norm1 / norm2 weights are in the no-decay norm group, every bias in the bias group"""
    z = np.load(os.path.join(GOLD, "g30_aifi_keys.npz"))
    p = f"{scale}_"
    m = _model(scale)
    sd = m.state_dict()
    assert list(sd.keys()) == list(z[p + "keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(z[p + "shapes"])
    assert sum(q.numel() for q in m.parameters()) == int(z[p + "n_params"])
    assert len(m.model) == int(z[p + "n_layers"])
    assert [L.np for L in m.model] == [int(v) for v in z[p + "layer_np"]]
    assert [float(v) for v in m.stride] == [float(v) for v in z[p + "stride"]]
    a = m.model[9]
    assert [a.ma.num_heads, a.ma.head_dim, a.fc1.out_features] == [int(v) for v in z[p + "heads_dim"]]
    from types import SimpleNamespace
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, FlatState
    flat = FlatState(m, with_ema=False)
    _, sizes = DetectionTrainer._param_order(SimpleNamespace(flat=flat))
    bias, decayed, bn_w = sizes
    frozen = [k for k, q in m.named_parameters() if not q.requires_grad]
    assert [decayed + len(frozen), bn_w, bias] == [int(v) for v in z[p + "opt_groups"]]
    gid = {id(q): g for q, _, _, g in flat.slots}
    names = {id(q): k for k, q in m.named_parameters()}
    assert sorted(names[i] for i, g in gid.items() if g == 1 and names[i].startswith("model.9.")) == sorted(z[p + "norm_group_layer9"]) \
        == ["model.9.norm1.weight", "model.9.norm2.weight"]
    for q in (a.norm1.bias, a.norm2.bias, a.fc1.bias, a.fc2.bias, a.ma.in_proj_bias, a.ma.out_proj.bias):
        assert gid[id(q)] == 2
    for q in (a.ma.in_proj_weight, a.ma.out_proj.weight, a.fc1.weight, a.fc2.weight):
        assert gid[id(q)] == 0


@pytest.mark.parametrize("scale", "nsmlx")
def test_aifi_yaml_builds_at_every_scale(scale):
    from dedark_yolo_amd.nn.modules import AIFI, SPPF
    from dedark_yolo_amd.nn.tasks import GraphPlan
    m = _model(scale)
    assert [i for i, L in enumerate(m.model) if isinstance(L, AIFI)] == [9] and not any(isinstance(L, SPPF) for L in m.model)
    a = m.model[9]
    width, dim = dict(n=(256, 32), s=(512, 64), m=(576, 72), l=(512, 64), x=(640, 80))[scale]
    assert (a.c_out, a.ma.embed_dim, a.ma.head_dim, a.ma.num_heads, a.fc1.out_features) == (width, width, dim, 8, 1024)
    assert a.ma.batch_first and isinstance(a.act, nn.GELU) and [type(c).__name__ for c in (a.dropout, a.dropout1, a.dropout2)] == ["Dropout"] * 3
    assert GraphPlan(list(m.model)).place.get(9) is not None            # row 9 writes into the head's last Concat buffer


def test_scale_prefixed_name_resolves_and_registry():
    from dedark_yolo_amd import YOLO
    from dedark_yolo_amd.nn import modules
    from dedark_yolo_amd.nn.tasks import _REGISTRY, yaml_model_load
    d = yaml_model_load("yolov8m-AIFI.yaml")
    assert d["scale"] == "m" and d["backbone"][9] == [-1, 1, "AIFI", [1024, 8]]
    ori = yaml_model_load("yolov8m.yaml".replace("yolov8m", "yolov8mori"))
    assert [r for i, r in enumerate(d["backbone"]) if i != 9] == [r for i, r in enumerate(ori["backbone"]) if i != 9] and d["head"] == ori["head"]
    assert YOLO("yolov8n-AIFI.yaml").task == "detect"
    assert _REGISTRY["AIFI"] is modules.AIFI and _REGISTRY["TransformerEncoderLayer"] is modules.TransformerEncoderLayer
    want = ["ma.in_proj_weight", "ma.in_proj_bias", "ma.out_proj.weight", "ma.out_proj.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias",
            "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"]
    assert list(modules.AIFI(64, 128, 8).state_dict()) == want and list(modules.TransformerEncoderLayer(64, 128, 4).state_dict()) == want
    assert list(modules.AIFI(64, 128, 8)._modules) == ["ma", "fc1", "fc2", "norm1", "norm2", "dropout", "dropout1", "dropout2", "act"]


def test_what_stays_out_of_scope_raises():
    from dedark_yolo_amd.nn import modules
    from dedark_yolo_amd.nn.tasks import DetectionModel
    for cls in (modules.AIFI, modules.TransformerEncoderLayer):
        with pytest.raises(NotImplementedError, match="normalize_before"):
            cls(64, 128, 8, normalize_before=True)
        with pytest.raises(NotImplementedError, match="dropout"):
            cls(64, 128, 8, dropout=0.1)
        with pytest.raises(NotImplementedError, match="GELU"):
            cls(64, 128, 8, act=nn.GELU(approximate="tanh"))
        with pytest.raises(NotImplementedError, match="GELU"):
            cls(64, 128, 8, act=nn.ReLU())
        with pytest.raises(NotImplementedError, match="D % 8 == 0"):
            cls(96, 128, 8)                                   # D = 12
        with pytest.raises(NotImplementedError, match="D % 8 == 0"):
            cls(1088, 128, 8)                                 # D = 136
        m = cls(64, 128, 8)
        x = torch.zeros(1, 64, 2, 2)
        with pytest.raises(NotImplementedError, match="mask"):
            m(x, src_mask=torch.zeros(4, 4))
        with pytest.raises(NotImplementedError, match="mask"):
            m(x, src_key_padding_mask=torch.zeros(1, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="divisible by 4"):
        modules.AIFI(66, 128, 1)
    with pytest.raises(ValueError, match="divisible by 4"):
        modules.AIFI.build_2d_sincos_position_embedding(3, 3, 30)
    cfg = _cfg("l")
    cfg["backbone"][9][1] = 3                                 # a stack of encoder layers through the row's repeat count
    with pytest.raises(NotImplementedError, match="AIFI row 9: repeats = 3"):
        DetectionModel(cfg, nc=20)
    for kind in ("RTDETRDecoder", "MSDeformAttn", "DeformableTransformerDecoder", "HGStem", "HGBlock"):
        cfg = _cfg("n")
        cfg["backbone"][9][2] = kind
        with pytest.raises(NotImplementedError, match=kind):
            DetectionModel(cfg, nc=20)


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def test_reference_checkpoint_writer_layout_for_the_aifi_graph():
    """save_reference_checkpoint's object tree for yolov8n-AIFI is, module by module, what the reference pickles
    (tests/golden/g30_aifi_skeleton.json); so is a bare TransformerEncoderLayer"""
    from test_host_cpu import _written_skeleton
    from dedark_yolo_amd.nn import modules
    from dedark_yolo_amd.utils.checkpoint import _RefWriter, reference_module_object
    with open(os.path.join(GOLD, "g30_aifi_skeleton.json")) as f:
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
    tel = modules.TransformerEncoderLayer(64, 128, 4)
    walk(skel["tel"], _written_skeleton(_RefWriter(tel.state_dict(), True).convert(tel, "")), "tel")
    assert not bad, bad[:10]
    assert {"ultralytics.nn.modules.transformer.AIFI", "ultralytics.nn.modules.transformer.TransformerEncoderLayer",
            "torch.nn.modules.activation.MultiheadAttention", "torch.nn.modules.linear.NonDynamicallyQuantizableLinear",
            "torch.nn.modules.linear.Linear", "torch.nn.modules.normalization.LayerNorm", "torch.nn.modules.activation.GELU",
            "torch.nn.modules.dropout.Dropout"} <= seen


def test_aifi_checkpoint_round_trip(tmp_path):
    from dedark_yolo_amd.utils.checkpoint import _REF_HOME, load_checkpoint, save_reference_checkpoint
    assert _REF_HOME["AIFI"] == _REF_HOME["TransformerEncoderLayer"] == "ultralytics.nn.modules.transformer"
    m = _model("n")
    path = save_reference_checkpoint(str(tmp_path / "last.pt"), m, epoch=0, train_args=dict(imgsz=64))
    import zipfile
    with zipfile.ZipFile(path) as zf:
        pkl = zf.read([n for n in zf.namelist() if n.endswith("data.pkl")][0])
    for needle in (b"ultralytics.nn.modules.transformer\nAIFI", b"MultiheadAttention", b"NonDynamicallyQuantizableLinear",
                   b"torch.nn.modules.normalization\nLayerNorm", b"torch.nn.modules.activation\nGELU"):
        assert needle in pkl, needle
    assert b"dedark_yolo_amd" not in pkl
    ck = load_checkpoint(path)                                # the restricted unpickler: LayerNorm / GELU arrive as inert records
    sd = m.state_dict()
    assert list(ck.state_dict) == list(sd)
    for k, v in sd.items():
        assert torch.equal(ck.state_dict[k], v.half().float() if v.is_floating_point() else v), k
    m2 = _model("n")
    m2.load_state_dict(ck.state_dict, strict=True)


def test_reference_loaded_our_checkpoint():
    """the recorded result of the reference loading a last.pt written here (make_aifi_golden.py interop): finite outputs of the
    expected shape, fused and unfused within the fuse tolerance"""
    z = np.load(os.path.join(GOLD, "g30_aifi_interop.npz"))
    assert z["y"].shape == (2, 24, 84) and np.isfinite(z["y"]).all()
    assert float(np.abs(z["y"] - z["y_fused"]).max()) <= 1e-3 * max(1.0, float(np.abs(z["y"]).max()))
