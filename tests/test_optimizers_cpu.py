"""The optimizer names of the reference's `optimizer:` key on the CPU (no GPU needed): name resolution (build_optimizer,
ultralytics/engine/trainer.py:611-665), the torch.optim-style state_dict of Adam / Adamax / NAdam / RAdam / RMSProp against torch's own
optimizers built the reference way, and the momentum warm-up (:326-327)."""
from types import SimpleNamespace

import pytest
import torch

from util import load_yaml

NAMES = ["Adam", "Adamax", "NAdam", "RAdam", "RMSProp"]
LR0, MOM, WD = 0.002, 0.9, 5e-4


def test_optimizer_names_resolve_like_the_reference():
    from dedark_yolo_amd.engine.trainer import DetectionTrainer
    res = DetectionTrainer.resolve_optimizer
    for name in ("SGD", "Adam", "Adamax", "AdamW", "NAdam", "RAdam", "RMSProp"):
        assert res(name, 0.01, 0.937) == (name, 0.01, 0.937)
    for bad in ("adam", "RMSprop", "Lion"):
        with pytest.raises(NotImplementedError) as e:
            res(bad, 0.01, 0.937)
        assert f"Optimizer '{bad}' not found in list of available optimizers" in str(e.value)
        assert all(n in str(e.value) for n in ("SGD", "Adam", "Adamax", "AdamW", "NAdam", "RAdam", "RMSProp", "auto"))
    assert res("auto", 0.01, 0.937, nc=20, total_iterations=10001) == ("SGD", 0.01, 0.9)
    assert res("auto", 0.01, 0.937, nc=20, total_iterations=10000) == ("AdamW", round(0.002 * 5 / 24, 6), 0.9)
    assert res("auto", 0.01, 0.937, nc=20) == ("SGD", 0.01, 0.9)             # unknown length: the long-run choice, as before


def _cpu_trainer(name):
    """A CPU FlatState of the tiny lowlight graph behind the few attributes the state_dict methods read."""
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, FlatState
    from dedark_yolo_amd.nn.tasks import DetectionModel
    cfgd = load_yaml("yolov8-lowlight.yaml")
    cfgd["scales"]["t"] = [0.33, 0.125, 1024]
    cfgd["scale"] = "t"
    torch.manual_seed(3)
    flat = FlatState(DetectionModel(cfgd, nc=20), with_ema=False)
    flat.alloc_optimizer(name)
    ns = SimpleNamespace(flat=flat, opt_name=name, lr0=LR0, momentum=MOM, weight_decay=WD, updates=0)
    ns._param_order = lambda: DetectionTrainer._param_order(ns)
    return ns


def _torch_optimizer(ns, name):
    """build_optimizer's three groups (biases, decayed weights, BatchNorm weights) over the trainable parameters in the trainer's
    numbering, and the LambdaLR of the reference's _setup_scheduler (it is what writes `initial_lr` into the groups)."""
    flat = ns.flat
    groups = {0: [], 1: [], 2: []}
    for p, o, n, g in flat.slots:
        groups[g].append(torch.nn.Parameter(flat.p[o:o + n].detach().clone().view(p.shape)))
    if name == "RMSProp":
        opt = torch.optim.RMSprop(groups[2], lr=LR0, momentum=MOM)
    else:
        opt = getattr(torch.optim, name)(groups[2], lr=LR0, betas=(MOM, 0.999), weight_decay=0.0)
    opt.add_param_group({"params": groups[0], "weight_decay": WD})
    opt.add_param_group({"params": groups[1], "weight_decay": 0.0})
    torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda x: 1.0)
    return opt, groups[2] + groups[0] + groups[1]


def _random_grads(params, seed):
    gen = torch.Generator().manual_seed(seed)
    for q in params:
        q.grad = torch.randn(q.shape, generator=gen) * 1e-2


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_loads_into_the_torch_optimizer(name):
    from dedark_yolo_amd.engine.trainer import DetectionTrainer
    ns = _cpu_trainer(name)
    gen = torch.Generator().manual_seed(1)
    ns.flat.m.copy_(torch.randn(ns.flat.n, generator=gen) * 1e-3)
    ns.flat.m2.copy_(torch.rand(ns.flat.n, generator=gen) * 1e-3 + 1e-6)
    ns.flat.opt_state[0], ns.flat.opt_state[1] = 3.0, 0.17
    ours = DetectionTrainer.optimizer_state_dict(ns)
    opt, params = _torch_optimizer(ns, name)
    own = opt.state_dict()
    for mine, theirs in zip(ours["param_groups"], own["param_groups"]):
        assert set(mine) == set(theirs), set(mine) ^ set(theirs)
        for k in set(mine) - {"params", "lr", "initial_lr", "weight_decay", "momentum", "betas"}:
            assert mine[k] == theirs[k] and type(mine[k]) is type(theirs[k]), (k, mine[k], theirs[k])
        assert mine["params"] == theirs["params"]
    opt.load_state_dict(ours)
    _random_grads(params, 2)
    opt.step()
    sd = opt.state_dict()["state"]
    assert len(sd) == len(params) and all(float(st["step"]) == 4.0 for st in sd.values())
    # torch's own state after one step has the key names and dtypes ours had
    fresh, fparams = _torch_optimizer(ns, name)
    _random_grads(fparams, 3)
    fresh.step()
    for i, st in fresh.state_dict()["state"].items():
        assert set(st) == set(ours["state"][i]), (set(st), set(ours["state"][i]))
        for k, v in st.items():
            assert ours["state"][i][k].dtype == v.dtype and ours["state"][i][k].shape == v.shape, k


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_round_trip(name):
    from dedark_yolo_amd.engine.trainer import DetectionTrainer
    ns = _cpu_trainer(name)
    opt, params = _torch_optimizer(ns, name)
    for seed in (4, 5):
        _random_grads(params, seed)
        opt.step()
    theirs = opt.state_dict()
    DetectionTrainer.load_optimizer_state_dict(ns, theirs)
    assert float(ns.flat.opt_state[0]) == 2.0
    ours = DetectionTrainer.optimizer_state_dict(ns)
    assert set(ours["state"]) == set(theirs["state"])
    for i, st in theirs["state"].items():
        assert set(st) == set(ours["state"][i])
        for k, v in st.items():
            got = ours["state"][i][k]
            assert got.dtype == v.dtype and torch.equal(got, v), (i, k)
    assert float(ours["state"][0]["step"]) == 2.0
    if name == "NAdam":
        assert float(theirs["state"][0]["mu_product"]) != 1.0
        assert torch.equal(ours["state"][0]["mu_product"], theirs["state"][0]["mu_product"])
    # a state that belongs to another optimizer is refused
    other = _cpu_trainer("RMSProp" if name != "RMSProp" else "Adam")
    with pytest.raises(RuntimeError):
        DetectionTrainer.load_optimizer_state_dict(other, theirs)
    sgd = _cpu_trainer("SGD")
    with pytest.raises(RuntimeError):
        DetectionTrainer.load_optimizer_state_dict(sgd, theirs)


def test_adam_family_is_told_apart():
    """Adam, RAdam and AdamW share their per-parameter keys: the writer's name decides when the checkpoint has it, the group keys
    otherwise."""
    from dedark_yolo_amd.engine.trainer import optimizer_of_state_dict
    w = [torch.nn.Parameter(torch.ones(3))]
    w[0].grad = torch.ones(3)
    for name in ("Adam", "RAdam", "AdamW", "NAdam", "Adamax", "RMSprop", "SGD"):
        kw = dict(momentum=0.9) if name in ("RMSprop", "SGD") else {}
        opt = getattr(torch.optim, name)(w, lr=1e-3, **kw)
        want = {"RMSprop": "RMSProp"}.get(name, name)
        assert optimizer_of_state_dict(opt.state_dict()) == {want}, name          # before the first step: by the group keys
        opt.step()
        assert optimizer_of_state_dict(opt.state_dict()) == {want}, name
    sd = torch.optim.Adam(w, lr=1e-3).state_dict()
    assert optimizer_of_state_dict(sd, "Adam") == {"Adam"}
    opt = torch.optim.AdamW(w, lr=1e-3)
    opt.step()
    sd = opt.state_dict()
    del sd["param_groups"][0]["decoupled_weight_decay"]                            # an older torch: Adam and AdamW look the same
    assert optimizer_of_state_dict(sd) == {"Adam", "AdamW"} and optimizer_of_state_dict(sd, "AdamW") == {"AdamW"}


def test_sgd_and_adamw_state_dicts_keep_their_layout():
    from dedark_yolo_amd.engine.trainer import DetectionTrainer
    for name, keys, gkeys in (("SGD", ["momentum_buffer"], ["lr", "initial_lr", "weight_decay", "maximize", "foreach", "differentiable", "params",
                                                           "momentum", "dampening", "nesterov", "fused"]),
                              ("AdamW", ["step", "exp_avg", "exp_avg_sq"], ["lr", "initial_lr", "weight_decay", "maximize", "foreach",
                                                                            "differentiable", "params", "betas", "eps", "amsgrad", "capturable",
                                                                            "fused"])):
        ns = _cpu_trainer(name)
        ns.updates = 5
        sd = DetectionTrainer.optimizer_state_dict(ns)
        assert list(sd["state"][0]) == keys and list(sd["param_groups"][1]) == gkeys
        assert ns.flat.opt_state is None and (ns.flat.m2 is None) == (name == "SGD")
        DetectionTrainer.load_optimizer_state_dict(ns, sd)


@pytest.mark.parametrize("name", ["Adam", "Adamax", "NAdam", "RAdam", "RMSProp", "SGD"])
def test_warmup_momentum(name):
    """trainer.py:326-327 interpolates `momentum` only in groups that have the key: SGD and RMSProp, not the `betas` groups."""
    from dedark_yolo_amd.engine.trainer import DetectionTrainer
    args = SimpleNamespace(lrf=0.01, cos_lr=False, warmup_bias_lr=0.1, warmup_momentum=0.8, momentum=0.937)
    ns = SimpleNamespace(args=args, lr0=0.01, momentum=args.momentum, opt_name=name)
    lr, mom = DetectionTrainer.lr_factors(ns, 25, 100, 0, 10)
    warmed = 0.8 + (0.937 - 0.8) * 0.25
    assert mom == pytest.approx(warmed if name in ("RMSProp", "SGD") else 0.937, abs=1e-12)
    assert lr[0] == pytest.approx(0.01 * 0.25) and lr[2] == pytest.approx(0.1 + (0.01 - 0.1) * 0.25)
    assert DetectionTrainer.lr_factors(ns, 101, 100, 0, 10)[1] == 0.937
