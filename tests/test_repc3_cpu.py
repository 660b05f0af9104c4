"""CPU tests of the RepC3 variant (RepConv / RepC3, cfg/models/v8/yolov8-RepC3.yaml): the parse rule, keys and optimizer groups
against the reference's fixtures, the host statement tests/repc3_ref.py against every block fixture (train, eval, fused) and
against torch's autograd, get_equivalent_kernel_bias / fuse_convs, the checkpoint writer's layout, what stays out of scope, and
the exported symbols."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import repc3_ref as rr
from util import GOLD, gold, load_yaml, rnd

YAML = "yolov8-RepC3.yaml"
F64 = torch.float64
#         name             class      args          kwargs            act
BLOCKS = {"repconv16": ("RepConv", (16, 16), {}, rr.ACT_SILU), "repconv64_id": ("RepConv", (64, 64), dict(act=False), rr.ACT_NONE),
          "repc3_32_64n1": ("RepC3", (32, 64, 1), {}, rr.ACT_SILU), "repc3_64n2": ("RepC3", (64, 64, 2), {}, rr.ACT_SILU)}


def _cfg(scale):
    d = load_yaml(YAML)
    d["scale"] = scale
    return d


def _model(scale, nc=20):
    from dedark_yolo_amd.nn.tasks import DetectionModel
    return DetectionModel(_cfg(scale), nc=nc)


def _block(name, seed):
    """our module with the fixture's rng_fill weights, and the same parameters as a float64 dict"""
    from oracle import model as om
    from parity_helpers import load_sd, set_bn
    from dedark_yolo_amd.nn import modules
    cls, args, kw, code = BLOCKS[name]
    m = set_bn(getattr(modules, cls)(*args, **kw))
    load_sd(m, om.rng_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed))
    return m, {k: v.to(F64) for k, v in m.state_dict().items() if v.is_floating_point()}, cls, code


def _fwd(cls, P, x, code, n, train, buffers=None, fused=False):
    if cls == "RepC3":
        return rr.repc3_forward(P, x, n, train, buffers, fused)
    if fused:
        return rr.repconv_fused_forward(P, "", x, code), None
    return rr.repconv_forward(P, "", x, code, train, buffers)


# ---------------------------------------------------------------------------------------------------------------- host statement
@pytest.mark.parametrize("code", [rr.ACT_SILU, rr.ACT_NONE, rr.ACT_LEAKY])
def test_bn2_ref_is_torch_autograd(code):
    """the stage and its adjoint against autograd through F.batch_norm twice + add + activation, float64"""
    g = torch.Generator().manual_seed(5 + code)
    M, C = 37, 12
    u, v, dy = (torch.randn(M, C, generator=g, dtype=F64) for _ in range(3))
    gu, bu, gv, bv = (torch.randn(C, generator=g, dtype=F64) for _ in range(4))
    ut, vt, p = u.clone().requires_grad_(True), v.clone().requires_grad_(True), [t.clone().requires_grad_(True) for t in (gu, bu, gv, bv)]
    z = F.batch_norm(ut, None, None, p[0], p[1], True, 0.0, rr.BN_EPS) + F.batch_norm(vt, None, None, p[2], p[3], True, 0.0, rr.BN_EPS)
    y = {rr.ACT_SILU: F.silu, rr.ACT_NONE: lambda t: t, rr.ACT_LEAKY: lambda t: F.leaky_relu(t, 0.1)}[code](z)
    y.backward(dy)
    su, hu, mu, iu = rr.bn_stats(u, gu, bu)
    sv, hv, mv, iv = rr.bn_stats(v, gv, bv)
    assert torch.allclose(rr.bn2_forward(u, v, su, hu, sv, hv, code), y.detach(), rtol=1e-12, atol=1e-12)
    du, dv, dgu, db, dgv = rr.bn2_backward(dy, u, v, (su, hu, mu, iu, gu), (sv, hv, mv, iv, gv), code)
    for got, want in ((du, ut.grad), (dv, vt.grad), (dgu, p[0].grad), (db, p[1].grad), (dgv, p[2].grad), (db, p[3].grad)):
        assert torch.allclose(got, want, rtol=1e-10, atol=1e-11)
    terms = rr.bn2_backward_terms(dy, u, v, (su, hu, mu, iu, gu), (sv, hv, mv, iv, gv), code)
    for got, t in zip((du, dv, dgu, db, dgv), terms):
        assert bool((t >= got.abs() * (1 - 1e-9)).all())           # the measure's denominator bounds the value it measures
    ty = rr.bn2_forward_terms(u, v, su, hu, sv, hv, code)
    assert bool((ty >= y.detach().abs()).all())


@pytest.mark.parametrize("name", list(BLOCKS))
def test_ref_matches_block_fixtures(name):
    """repc3_ref in float64 against the reference's train / eval / fused fixtures: outputs, input and parameter gradients, running
    buffers, fused kernel and bias"""
    tr, ev, fu = (gold(f"g31_repc3_{name}_{s}") for s in ("train", "eval", "fused"))
    _, P, cls, code = _block(name, int(tr["seed"]))
    n = BLOCKS[name][1][2] if cls == "RepC3" else 0
    x = tr["x0"].to(F64)
    buffers, grads = {}, {}
    y, c = _fwd(cls, P, x, code, n, True, buffers)
    assert torch.allclose(y.float(), tr["y0"], rtol=1e-4, atol=1e-5)
    g = rnd(900, *y.shape, lo=-1, hi=1).to(F64)
    dx = (rr.repc3_backward if cls == "RepC3" else rr.repconv_backward)(c, g, grads)
    assert torch.allclose(dx.float(), tr["dx0"], rtol=2e-3, atol=2e-4)
    seen = 0
    for k, v in tr.items():
        if k.startswith("g:"):
            assert torch.allclose(grads[k[2:]].float(), v, rtol=2e-3, atol=2e-3 * float(v.abs().max())), k
        elif k.startswith("gn:"):
            assert abs(float(grads[k[3:]].norm()) - float(v)) <= 2e-3 * float(v), k
        elif k.startswith("b:"):
            assert torch.allclose(buffers[k[2:]].float(), v, rtol=1e-5, atol=1e-6), k
        seen += k.startswith(("g:", "gn:"))
    assert seen == len(grads) == sum(1 for k in P if k.endswith("weight") or k.endswith("bias"))
    assert grads[[k for k in grads if k.endswith("conv1.bn.bias")][0]].equal(grads[[k for k in grads if k.endswith("conv2.bn.bias")][0]])
    ye, _ = _fwd(cls, P, ev["x0"].to(F64), code, n, False)
    assert torch.allclose(ye.float(), ev["y0"], rtol=1e-4, atol=1e-5)
    for k, v in ev.items():
        if k.startswith("b:"):
            assert torch.equal(P[k[2:]].float(), v), k                  # an eval forward leaves the buffers alone
    yf, _ = _fwd(cls, P, fu["x0"].to(F64), code, n, False, fused=True)
    assert torch.allclose(yf.float(), fu["y0"], rtol=1e-4, atol=1e-5)
    assert float((yf - ye).abs().max()) <= 1e-9 * float(ye.abs().max())


@pytest.mark.parametrize("name", list(BLOCKS))
def test_get_equivalent_kernel_bias_and_fuse_convs(name):
    """our modules' re-parameterisation against the reference's fused weights; afterwards the children are act, conv"""
    from dedark_yolo_amd.nn import modules
    fu = gold(f"g31_repc3_{name}_fused")
    m, P, cls, _ = _block(name, int(fu["seed"]))
    reps = [("", m)] if cls == "RepConv" else [(f"m.{i}.", r) for i, r in enumerate(m.m)]
    for pre, r in reps:
        w, b = r.get_equivalent_kernel_bias()
        assert w.dtype == b.dtype == torch.float32 and w.shape == (r.c2, r.c1, 3, 3)
        w64, b64 = rr.repconv_fused(P, pre)
        assert torch.allclose(w, w64.float(), rtol=1e-5, atol=1e-7) and torch.allclose(b, b64.float(), rtol=1e-5, atol=1e-7)
    before = [k for k, _ in reps[0][1].named_children()]
    assert before == ["act", "conv1", "conv2"] and reps[0][1].bn is None
    for _, r in reps:
        r.fuse_convs()
        r.fuse_convs()                                                   # a second call is a no-op
        assert [k for k, _ in r.named_children()] == ["act", "conv"] == [str(s) for s in fu["children"]]
        assert isinstance(r.conv, nn.Conv2d) and r.conv.bias is not None and r.conv.kernel_size == (3, 3) and r.conv.padding == (1, 1)
        assert not any(p.requires_grad for p in r.parameters())
    sd = m.state_dict()
    for k, v in fu.items():
        if k.startswith("w:"):
            assert torch.allclose(sd[k[2:]], v, rtol=1e-5, atol=1e-6), k
        elif k.startswith("wn:"):
            assert abs(float(sd[k[3:]].norm()) - float(v)) <= 1e-5 * float(v), k
        elif k.startswith("w4:"):
            assert torch.allclose(sd[k[3:]][:4], v, rtol=1e-5, atol=1e-6), k
    assert isinstance(modules.RepC3(32, 64, 1).cv3, nn.Identity)


# ---------------------------------------------------------------------------------------------------------------- graph, registry
@pytest.mark.parametrize("scale", "nml")
def test_repc3_graph_matches_the_reference(scale):
    """parse_model of yolov8{n,m,l}-RepC3.yaml: keys, shapes, counts and the three optimizer groups of the reference's model; the
    BatchNorm weights of both RepConv branches are in the no-decay group"""
    from dedark_yolo_amd.nn import modules
    z = np.load(os.path.join(GOLD, "g31_repc3_keys.npz"))
    p = f"{scale}_"
    m = _model(scale)
    sd = m.state_dict()
    assert list(sd.keys()) == list(z[p + "keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(z[p + "shapes"])
    assert sum(q.numel() for q in m.parameters()) == int(z[p + "n_params"])
    assert len(m.model) == int(z[p + "n_layers"])
    assert [L.np for L in m.model] == [int(v) for v in z[p + "layer_np"]]
    assert [float(v) for v in m.stride] == [float(v) for v in z[p + "stride"]]
    assert [i for i, L in enumerate(m.model) if isinstance(L, modules.RepC3)] == [12, 15, 18, 21]
    assert [len(m.model[i].m) for i in (12, 15, 18, 21)] == [int(v) for v in z[p + "n_repconv"]]
    from types import SimpleNamespace
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, FlatState
    flat = FlatState(m, with_ema=False)
    _, sizes = DetectionTrainer._param_order(SimpleNamespace(flat=flat))
    bias, decayed, bn_w = sizes
    frozen = [k for k, q in m.named_parameters() if not q.requires_grad]
    assert [decayed + len(frozen), bn_w, bias] == [int(v) for v in z[p + "opt_groups"]]
    gid = {id(q): g for q, _, _, g in flat.slots}
    names = {id(q): k for k, q in m.named_parameters()}
    ours = sorted(names[i] for i, g in gid.items() if g == 1 and names[i].startswith("model.12."))
    assert ours == sorted(z[p + "norm_group_layer12"])
    assert "model.12.m.0.conv1.bn.weight" in ours and "model.12.m.0.conv2.bn.weight" in ours


@pytest.mark.parametrize("scale", "nsmlx")
def test_repc3_yaml_builds_at_every_scale(scale):
    from dedark_yolo_amd.nn import modules
    from dedark_yolo_amd.nn.tasks import GraphPlan
    m = _model(scale)
    width = dict(n=128, s=256, m=384, l=512, x=640)[scale]
    r = m.model[12]
    assert r.cv1.conv.out_channels == width and all(isinstance(c, modules.RepConv) and c.c1 == c.c2 == width for c in r.m)
    assert isinstance(r.cv3, nn.Identity) and not any(isinstance(L, modules.C2f) for L in m.model[10:])
    assert GraphPlan(list(m.model)).place.get(12) is not None          # row 12 writes into the Concat buffer of row 17


def test_scale_prefixed_name_resolves_and_registry():
    from dedark_yolo_amd import YOLO
    from dedark_yolo_amd.nn import modules
    from dedark_yolo_amd.nn.tasks import _REGISTRY, _RULES, yaml_model_load
    d = yaml_model_load("yolov8m-RepC3.yaml")
    ori = yaml_model_load("yolov8mori.yaml")
    assert d["scale"] == "m" and d["backbone"] == ori["backbone"]
    assert d["head"] == [[f, n, "RepC3" if k == "C2f" else k, a] for f, n, k, a in ori["head"]]
    assert YOLO("yolov8n-RepC3.yaml").task == "detect"
    assert _REGISTRY["RepC3"] is modules.RepC3 and _RULES[modules.RepC3] is _RULES[modules.C2f]
    assert "RepConv" not in _REGISTRY                                  # no yaml rule in the reference's parse_model either
    want = [f"{c}.{k}" for c in ("conv1", "conv2") for k in ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var",
                                                               "bn.num_batches_tracked")]
    assert list(modules.RepConv(16, 16).state_dict()) == want


def test_what_stays_out_of_scope_raises():
    from dedark_yolo_amd.nn import modules
    with pytest.raises(NotImplementedError, match="e=0.5"):
        modules.RepC3(32, 64, 2, 0.5)
    with pytest.raises(NotImplementedError, match="bn=True"):
        modules.RepConv(16, 16, bn=True)
    with pytest.raises(NotImplementedError, match="s=2"):
        modules.RepConv(16, 16, s=2)
    with pytest.raises(NotImplementedError, match="g=2"):
        modules.RepConv(16, 16, g=2)
    with pytest.raises(NotImplementedError, match="d=2"):
        modules.RepConv(16, 16, d=2)
    with pytest.raises(NotImplementedError, match="c1=16 != c2=32"):
        modules.RepConv(16, 32)
    with pytest.raises(AssertionError):
        modules.RepConv(16, 16, k=1, p=0)


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def test_reference_checkpoint_writer_layout_for_the_repc3_graph():
    """save_reference_checkpoint's object tree for yolov8n-RepC3 is, module by module, what the reference pickles
    (tests/golden/g31_repc3_skeleton.json); the restricted unpickler needs no new entries: the two classes arrive as records"""
    from test_host_cpu import _written_skeleton
    from dedark_yolo_amd.utils.checkpoint import reference_module_object
    with open(os.path.join(GOLD, "g31_repc3_skeleton.json")) as f:
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
    assert not bad, bad[:10]
    assert {"ultralytics.nn.modules.block.RepC3", "ultralytics.nn.modules.conv.RepConv", "torch.nn.modules.linear.Identity"} <= seen


def test_repc3_checkpoint_round_trip(tmp_path):
    from dedark_yolo_amd.utils.checkpoint import load_checkpoint, save_reference_checkpoint
    m = _model("n")
    path = str(tmp_path / "last.pt")
    save_reference_checkpoint(path, m, epoch=0, train_args=dict(imgsz=64))
    import zipfile
    with zipfile.ZipFile(path) as zf:
        pkl = zf.read([n for n in zf.namelist() if n.endswith("data.pkl")][0])
    for needle in (b"ultralytics.nn.modules.block\nRepC3", b"ultralytics.nn.modules.conv\nRepConv", b"torch.nn.modules.linear\nIdentity"):
        assert needle in pkl, needle
    assert b"dedark_yolo_amd" not in pkl
    ck = load_checkpoint(path)
    sd = m.state_dict()
    assert ck.source == "reference-pickle" and list(ck.state_dict) == list(sd)
    for k, v in sd.items():
        assert torch.equal(ck.state_dict[k], v.half().float() if v.is_floating_point() else v), k
    _model("n").load_state_dict(ck.state_dict, strict=True)


def test_reference_loaded_our_checkpoint():
    """the recorded result of the reference loading a last.pt written here (make_repc3_golden.py interop): finite outputs of the
    expected shape, its own fuse() (RepConv re-parameterised) within the fuse tolerance of the unfused output"""
    z = np.load(os.path.join(GOLD, "g31_repc3_interop.npz"))
    assert z["y"].shape == (2, 24, 84) and np.isfinite(z["y"]).all()
    assert float(np.abs(z["y"] - z["y_fused"]).max()) <= 1e-3 * max(1.0, float(np.abs(z["y"]).max()))


def test_library_exports_the_new_symbols():
    import ctypes
    from dedark_yolo_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name in ("dy_bn2_act_fwd", "dy_bn2_act_bwd", "dy_bn2_act_bwd_workspace"):
        assert name in _C._SIGS and hasattr(lib, name), name
    # the documented bound of the workspace: 3 C (DY_BN2_MAX_PARTS + 1) floats
    lib.dy_bn2_act_bwd_workspace.restype = ctypes.c_int64
    lib.dy_bn2_act_bwd_workspace.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    for px, C, dt in ((1, 8, 1), (4100, 264, 1), (1 << 22, 64, 0), (51200, 512, 2)):
        n = lib.dy_bn2_act_bwd_workspace(px, C, dt)
        assert 6 * C <= n <= 3 * C * 1025 and n % (3 * C) == 0, (px, C, dt, n)
    assert lib.dy_bn2_act_bwd_workspace(64, 12, 1) == 0                # 12 channels are not whole vectors in bf16
