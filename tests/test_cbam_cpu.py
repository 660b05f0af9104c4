"""CPU tests of the CBAM variants (ChannelAttention / SpatialAttention / CBAM, cfg/models/v8/yolov8-CBAM.yaml and
yolov8-lowlight-CBAM.yaml): the float64 statement tests/cbam_ref.py against every block fixture of the reference and against
torch's autograd (ties included), eight wrong variants of the arithmetic that the cases must tell from the right one, the parse
rules, keys and optimizer groups against the reference's fixtures, placement inside a yaml-level Concat, validation errors, the
checkpoint writer's layout and the exported symbols.

Bound of the statement against a fixture: the fixture is the reference's own f32 run; an output there sums at most n = C + 2 k^2 <=
354 products, so its error is below n 2^-24 ~ 2e-5 of the sum of its absolute terms, which for these inputs (|x|, |w|, |dy| <= 1)
is a small multiple of max|value|: BOUND = 2e-4 max|fixture value| per compared array.
"""
import json
import os

import numpy as np
import pytest
import torch

import cbam_ref as cr
from util import GOLD, gold, load_yaml, rnd

YAMLS = {"": "yolov8-CBAM.yaml", "ll_": "yolov8-lowlight-CBAM.yaml"}
BOUND = 2e-4
#         name         kind    class               args      C
BLOCKS = {"cbam16_k7": ("cbam", "CBAM", (16, 7)), "cbam64_k3": ("cbam", "CBAM", (64, 3)), "cbam256_k7": ("cbam", "CBAM", (256, 7)),
          "ca32": ("ca", "ChannelAttention", (32,)), "sa7_c24": ("sa", "SpatialAttention", (7,))}


def _cfg(prefix, scale):
    d = load_yaml(YAMLS[prefix])
    d["scale"] = scale
    return d


def _model(prefix, scale, nc=20):
    from dedark_yolo_amd.nn.tasks import DetectionModel
    return DetectionModel(_cfg(prefix, scale), nc=nc)


def _params(name, seed):
    """the fixture's rng_fill weights of our module as float64 numpy arrays (fc_w, fc_b, cv_w)"""
    from oracle import model as om
    from dedark_yolo_amd.nn import modules
    kind, cls, args = BLOCKS[name]
    m = getattr(modules, cls)(*args)
    sd = om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed)
    pick = lambda tail: next((v.double().numpy() for k, v in sd.items() if k.endswith(tail)), None)
    return m, sd, pick("fc.weight"), pick("fc.bias"), pick("cv1.weight")


def _errors(name, variant=None):
    """relative errors (max |statement - fixture| / max |fixture|) of every array of the block's train and eval fixtures"""
    tr, ev = gold(f"g33_cbam_{name}_train"), gold(f"g33_cbam_{name}_eval")
    kind = BLOCKS[name][0]
    _, _, fw, fb, cw = _params(name, int(tr["seed"]))
    x = cr.nhwc(tr["x0"].numpy())
    dy = cr.nhwc(rnd(900, *tr["y0"].shape, lo=-1, hi=1).numpy())
    out = cr.block(kind, x, dy, fw, fb, cw, variant)
    rel = lambda got, want: float(np.abs(got - want.double().numpy()).max() / np.abs(want.double().numpy()).max())
    errs = {"y": rel(cr.nchw(out["y"]), tr["y0"]), "dx": rel(cr.nchw(out["dx"]), tr["dx0"])}
    for k, v in tr.items():
        if k.startswith("g:"):
            key = "fc_w" if k.endswith("fc.weight") else "fc_b" if k.endswith("fc.bias") else "cv_w"
            errs[key] = rel(out[key], v)
    errs["y_eval"] = rel(cr.nchw(cr.block(kind, cr.nhwc(ev["x0"].numpy()), None, fw, fb, cw, variant)["y"]), ev["y0"])
    if "gap" in out:
        assert float(out["gap"].min()) >= 1e-4 * out["u_max"] * 0.99, "the fixture's seed walk guarantees the top-two gap"
    return errs


# ---------------------------------------------------------------------------------------------------------------- host statement
@pytest.mark.parametrize("name", list(BLOCKS))
def test_ref_matches_block_fixtures(name):
    errs = _errors(name)
    want = {"y", "dx", "y_eval"} | ({"fc_w", "fc_b"} if BLOCKS[name][0] != "sa" else set()) | ({"cv_w"} if BLOCKS[name][0] != "ca" else set())
    assert set(errs) == want
    print(name, errs)
    assert all(e <= BOUND for e in errs.values()), errs


def _tie_case(variant=None):
    """SpatialAttention on a map whose channels are pairwise equal (every pixel is a tie) against torch's CPU autograd in float64:
    torch.max sends the gradient of a tie to the lowest channel index"""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 4, 5, 6, generator=g, dtype=torch.float64).repeat(1, 2, 1, 1)
    w = torch.randn(1, 2, 7, 7, generator=g, dtype=torch.float64) * 0.3
    dy = torch.randn(2, 8, 5, 6, generator=g, dtype=torch.float64)
    xt = x.clone().requires_grad_(True)
    m = torch.cat([xt.mean(1, keepdim=True), xt.max(1, keepdim=True)[0]], 1)
    (xt * torch.sigmoid(torch.nn.functional.conv2d(m, w, padding=3))).backward(dy)
    out = cr.block("sa", cr.nhwc(x.numpy()), cr.nhwc(dy.numpy()), cv_w=w.numpy(), variant=variant)
    return float(np.abs(cr.nchw(out["dx"]) - xt.grad.numpy()).max() / xt.grad.abs().max())


def test_ref_tie_rule_is_torch_cpu():
    assert _tie_case() <= 1e-12


@pytest.mark.parametrize("variant", cr.VARIANTS)
def test_cases_tell_the_wrong_variants_apart(variant):
    """each of the eight wrong arithmetics exceeds, on at least one case, the bound the right one meets on all of them"""
    worst = max(max(_errors(name, variant).values()) for name in BLOCKS)
    tie = _tie_case(variant)
    print(variant, worst, tie)
    assert worst > BOUND or tie > BOUND, (variant, worst, tie)
    if variant == "last_tie":
        assert tie > BOUND              # only a tie shows it: the fixtures have none by construction
    if variant == "pad3_k3":
        assert max(_errors("cbam64_k3", variant).values()) > BOUND


def test_terms_bound_their_values():
    g = np.random.default_rng(3)
    x, dy, a = g.standard_normal((2, 4, 5, 16)), g.standard_normal((2, 4, 5, 16)), g.standard_normal((2, 16))
    w = g.standard_normal((1, 2, 3, 3))
    f = cr.forward(x, a, w)
    assert (f["y_terms"] >= np.abs(f["y"]) * (1 - 1e-12)).all() and (f["mean_terms"] >= np.abs(f["mean"]) * (1 - 1e-12)).all()
    dpre, t = cr.bwd_px(dy, x, a, f["s"])
    assert (t >= np.abs(dpre) * (1 - 1e-12)).all()
    dmean, dmx, dw, tm, tx, tw = cr.conv_bwd(dpre, f["mean"], f["mx"], w)
    assert (tm >= np.abs(dmean) * (1 - 1e-12)).all() and (tx >= np.abs(dmx) * (1 - 1e-12)).all() and (tw >= np.abs(dw) * (1 - 1e-12)).all()
    pl = dict(s=f["s"], dmean=dmean, dmx=dmx, arg=f["arg"])
    for got, terms in (cr.gate_reduce(dy, x, a, pl), cr.gate_apply(dy, a, pl, g.standard_normal((2, 16)))):
        assert (terms >= np.abs(got) * (1 - 1e-12)).all()


# ---------------------------------------------------------------------------------------------------------------- graph, registry
@pytest.mark.parametrize("prefix,scale", [(p, s) for p in YAMLS for s in "nml"])
def test_cbam_graphs_match_the_reference(prefix, scale):
    """parse_model of both yamls at n / m / l: keys, shapes, counts and the three optimizer groups of the reference's model; fc.bias
    is in the bias group, the two conv weights in the decayed group"""
    from types import SimpleNamespace
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, FlatState
    from dedark_yolo_amd.nn import modules
    z = np.load(os.path.join(GOLD, "g33_cbam_keys.npz"))
    p = f"{prefix}{scale}_"
    m = _model(prefix, scale)
    sd = m.state_dict()
    assert list(sd.keys()) == list(z[p + "keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(z[p + "shapes"])
    assert sum(q.numel() for q in m.parameters()) == int(z[p + "n_params"])
    assert len(m.model) == int(z[p + "n_layers"])
    assert [L.np for L in m.model] == [int(v) for v in z[p + "layer_np"]]
    assert [float(v) for v in m.stride] == [float(v) for v in z[p + "stride"]]
    off = 1 if prefix else 0
    rows = [i for i, L in enumerate(m.model) if isinstance(L, modules.CBAM)]
    assert rows == [5 + off, 8 + off, 12 + off]
    flat = FlatState(m, with_ema=False)
    _, sizes = DetectionTrainer._param_order(SimpleNamespace(flat=flat))
    bias, decayed, bn_w = sizes
    frozen = [k for k, q in m.named_parameters() if not q.requires_grad]
    assert [decayed + len(frozen), bn_w, bias] == [int(v) for v in z[p + "opt_groups"]]
    gid = {id(q): g for q, _, _, g in flat.slots}
    names = {id(q): k for k, q in m.named_parameters()}
    group = {names[i]: g for i, g in gid.items() if names[i].startswith(f"model.{rows[0]}.")}
    assert set(group) == {f"model.{rows[0]}.{k}" for k in ("channel_attention.fc.weight", "channel_attention.fc.bias", "spatial_attention.cv1.weight")}
    gw, gb, gc = (group[f"model.{rows[0]}.{k}"] for k in ("channel_attention.fc.weight", "channel_attention.fc.bias", "spatial_attention.cv1.weight"))
    assert gw == gc != gb and gb != 1 and gw != 1        # (group 1 is the no-decay BatchNorm group)


@pytest.mark.parametrize("scale", "nsmlx")
def test_cbam_yamls_build_at_every_scale_and_place(scale):
    from dedark_yolo_amd.nn import modules
    from dedark_yolo_amd.nn.tasks import GraphPlan
    for prefix, off in (("", 0), ("ll_", 1)):
        m = _model(prefix, scale)
        widths = [m.model[i + off].channel_attention.fc.in_channels for i in (5, 8, 12)]
        assert widths == [m.model[i + off].c_out for i in (4, 7, 11)]
        assert all(isinstance(m.model[i + off], modules.CBAM) and m.model[i + off].spatial_attention.cv1.kernel_size == (7, 7) for i in (5, 8, 12))
        plan = GraphPlan(list(m.model))
        # rows 8 and 5 feed the Concat rows 14 and 17 and write into their slices (behind the Upsample's), row 12 feeds row 23
        assert plan.place.get(8 + off) == (14 + off, widths[2]) and plan.place.get(5 + off) == (17 + off, m.model[15 + off].c_out)
        assert plan.place.get(12 + off) == (23 + off, m.model[22 + off].c_out)


def test_scale_prefixed_names_registry_and_rules():
    from dedark_yolo_amd import YOLO
    from dedark_yolo_amd.nn import modules
    from dedark_yolo_amd.nn.tasks import _PLACEABLE, _REGISTRY, parse_model, yaml_model_load
    d, ori = yaml_model_load("yolov8m-CBAM.yaml"), yaml_model_load("yolov8mori.yaml")
    assert d["scale"] == "m"
    rows = d["backbone"] + d["head"]
    assert [r for r in rows if r[2] != "CBAM"][:10] == ori["backbone"] and [r[3] for r in rows if r[2] == "CBAM"] == [[7]] * 3
    assert YOLO("yolov8n-CBAM.yaml").task == "detect" and YOLO("yolov8l-lowlight-CBAM.yaml").task == "detect"
    for n in ("CBAM", "ChannelAttention", "SpatialAttention"):
        assert _REGISTRY[n] is getattr(modules, n) and getattr(modules, n) in _PLACEABLE
    cfg = dict(nc=3, backbone=[[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "ChannelAttention", []], [-1, 1, "SpatialAttention", [3]], [-1, 1, "CBAM", [3]]],
               head=[[[1, 2, 3], 1, "Detect", ["nc"]]])
    layers, _ = parse_model(cfg, 3)
    assert layers[1].fc.in_channels == 16 and layers[2].cv1.kernel_size == (3, 3) and layers[3].spatial_attention.cv1.padding == (1, 1)
    assert [L.c_out for L in layers[:4]] == [16] * 4
    assert list(modules.CBAM(16).state_dict()) == ["channel_attention.fc.weight", "channel_attention.fc.bias", "spatial_attention.cv1.weight"]
    assert [k for k, _ in modules.ChannelAttention(8).named_children()] == ["pool", "fc", "act"]
    assert [k for k, _ in modules.SpatialAttention().named_children()] == ["cv1", "act"]


def test_construction_draws_torch_initialisation_in_the_reference_order():
    from dedark_yolo_amd.nn import modules
    torch.manual_seed(5)
    m = modules.CBAM(16, 3)
    torch.manual_seed(5)
    fc = torch.nn.Conv2d(16, 16, 1, 1, 0, bias=True)
    cv = torch.nn.Conv2d(2, 1, 3, padding=1, bias=False)
    assert torch.equal(m.channel_attention.fc.weight, fc.weight) and torch.equal(m.channel_attention.fc.bias, fc.bias)
    assert torch.equal(m.spatial_attention.cv1.weight, cv.weight)


def test_validation_errors():
    from dedark_yolo_amd.nn import modules
    with pytest.raises(AssertionError, match="kernel size must be 3 or 7"):
        modules.SpatialAttention(5)
    with pytest.raises(AssertionError, match="kernel size must be 3 or 7"):
        modules.CBAM(16, 1)
    for c in (12, 4, 2056):
        with pytest.raises(NotImplementedError, match=f"C={c}"):
            modules.CBAM(c)
        with pytest.raises(NotImplementedError, match=f"C={c}"):
            modules.ChannelAttention(c)
    with pytest.raises(NotImplementedError, match="outside the Dedark-YOLO hot path"):
        from dedark_yolo_amd.nn.tasks import parse_model
        parse_model(dict(nc=3, backbone=[[-1, 1, "ECA", []]], head=[]), 3)


def test_fuse_leaves_the_blocks_alone():
    m = _model("", "n")
    before = {k: v.clone() for k, v in m.state_dict().items() if "attention" in k}
    m.fuse()
    after = m.state_dict()
    assert before and all(torch.equal(after[k], v) for k, v in before.items())
    assert [k for k, _ in m.model[5].named_children()] == ["channel_attention", "spatial_attention"]


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def test_reference_checkpoint_writer_layout_for_the_cbam_graph():
    """save_reference_checkpoint's object tree for yolov8n-CBAM is, module by module, what the reference pickles
    (tests/golden/g33_cbam_skeleton.json)"""
    from test_host_cpu import _written_skeleton
    from dedark_yolo_amd.utils.checkpoint import reference_module_object
    with open(os.path.join(GOLD, "g33_cbam_skeleton.json")) as f:
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
    walk(skel["n"], _written_skeleton(reference_module_object(_model("", "n"), None, True, dict(box=7.5, cls=0.5, dfl=1.5, lrl=2.0))), "n")
    assert not bad, bad[:10]
    assert {"ultralytics.nn.modules.conv.CBAM", "ultralytics.nn.modules.conv.ChannelAttention", "ultralytics.nn.modules.conv.SpatialAttention",
            "torch.nn.modules.pooling.AdaptiveAvgPool2d", "torch.nn.modules.activation.Sigmoid"} <= seen


def test_cbam_checkpoint_round_trip(tmp_path):
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint, save_reference_checkpoint
    m = _model("", "n")
    path = str(tmp_path / "last.pt")
    save_reference_checkpoint(path, m, epoch=0, train_args=dict(imgsz=64))
    import zipfile
    with zipfile.ZipFile(path) as zf:
        pkl = zf.read([n for n in zf.namelist() if n.endswith("data.pkl")][0])
    for needle in (b"ultralytics.nn.modules.conv\nCBAM", b"ultralytics.nn.modules.conv\nChannelAttention",
                   b"ultralytics.nn.modules.conv\nSpatialAttention", b"torch.nn.modules.pooling\nAdaptiveAvgPool2d"):
        assert needle in pkl, needle
    assert b"dedark_yolo_amd" not in pkl
    ck = load_checkpoint(path)
    sd = m.state_dict()
    assert ck.source == "reference-pickle" and list(ck.state_dict) == list(sd)
    for k, v in sd.items():
        assert torch.equal(ck.state_dict[k], v.half().float() if v.is_floating_point() else v), k
    _model("", "n").load_state_dict(ck.state_dict, strict=True)


def test_reference_loaded_our_checkpoint():
    """the recorded result of the reference loading a last.pt written here (make_cbam_golden.py interop)"""
    z = np.load(os.path.join(GOLD, "g33_cbam_interop.npz"))
    assert z["y"].shape == (2, 24, 84) and np.isfinite(z["y"]).all()
    assert float(np.abs(z["y"] - z["y_fused"]).max()) <= 1e-3 * max(1.0, float(np.abs(z["y"]).max()))


def test_library_exports_the_new_symbols():
    import ctypes
    from dedark_yolo_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    names = ("dy_chan_pool_fwd", "dy_chan_gate_fwd", "dy_spatial_stats_fwd", "dy_spatial_gate_fwd", "dy_spatial_gate_bwd_px", "dy_spatial_conv_bwd",
             "dy_spatial_conv_bwd_workspace", "dy_spatial_gate_bwd_reduce", "dy_spatial_gate_bwd_apply", "dy_cbam_reduce_workspace")
    for name in names:
        assert name in _C._SIGS and hasattr(lib, name), name
    with open(os.path.join(os.path.dirname(GOLD), "..", "include", "dedark_yolo.h")) as f:
        header = f.read()
    assert all(f" {n}(" in header for n in names) and "conv.py:294-304" in header and "conv.py:307-320" in header
    L = _C.lib()
    assert L.dy_spatial_conv_bwd_workspace(2, 17, 33, 7) == 2 * 2 * 3 * 98 and L.dy_spatial_conv_bwd_workspace(2, 17, 33, 5) == 0
    for B, HW, C, dt in ((1, 1, 8, 1), (32, 6400, 64, 1), (2, 400, 2048, 0)):
        n = L.dy_cbam_reduce_workspace(B, HW, C, dt)
        assert B * C <= n <= B * C * 64 and n % (B * C) == 0
    assert L.dy_cbam_reduce_workspace(1, 16, 12, 1) == 0
