"""GPU tests of the fused Adam / Adamax / NAdam / RAdam / RMSProp steps (dy_optim_step, csrc/optim.hip) against torch.optim on the
same gradients -- the reference's optimizer_step is clip_grad_norm_(10.0) -> optimizer.step() -> ema.update()
(ultralytics/engine/trainer.py:459-467, build_optimizer :648-651, ModelEMA torch_utils.py:344-377).

Truth is torch.optim.<Name>(foreach=False) on f64 CPU copies.  The bound for parameters, both state buffers and the EMA, per step:
    |got - truth| <= max(2e-6 * max(1, max|truth|), 4 * E)
2e-6 * max(1, max|truth|) is the bound of the SGD / AdamW test (tests/test_gpu_trainer.py); E is the largest error of torch's OWN f32
run (foreach=False, CPU) of the same sequence against the f64 truth for that quantity and step, and the factor 4 covers a different
but equally valid order of the f32 operations.  Each test prints E and the achieved error."""
import math

import pytest
import torch

from util import load_yaml

pytestmark = pytest.mark.gpu

NAMES = ["Adam", "Adamax", "NAdam", "RAdam", "RMSProp"]
KEYS = dict(Adam=("exp_avg", "exp_avg_sq"), Adamax=("exp_avg", "exp_inf"), NAdam=("exp_avg", "exp_avg_sq"),
            RAdam=("exp_avg", "exp_avg_sq"), RMSProp=("square_avg", "momentum_buffer"))
BETA2 = dict(Adam=0.999, Adamax=0.999, NAdam=0.999, RAdam=0.999, RMSProp=0.99)      # RMSProp: alpha


def _torch_run(name, dtype, p0, gid, grads, lrs, wds, moms):
    """clip_grad_norm_(10) + torch.optim.<name>.step() + the EMA formula on CPU copies in `dtype`: one tensor per parameter group (the
    rules are element-wise, so the split into tensors does not matter).  gid = the flat state's group per element; lrs[t] / wds are
    indexed by it.  Returns per step (p, buf1, buf2, ema) as flat f64 tensors."""
    gid = gid.cpu().long()
    idx = [torch.nonzero(gid == k).reshape(-1) for k in range(3)]
    qs = [torch.nn.Parameter(p0.cpu().to(dtype)[i].clone()) for i in idx]
    pg = [dict(params=[q], lr=lrs[0][k], weight_decay=wds[k]) for k, q in enumerate(qs)]
    if name == "RMSProp":
        opt = torch.optim.RMSprop(pg, lr=1e-3, momentum=moms[0], foreach=False)
    else:
        opt = getattr(torch.optim, name)(pg, lr=1e-3, betas=(moms[0], 0.999), foreach=False)
    ema = p0.cpu().to(dtype).clone()
    out = []
    for t, g in enumerate(grads):
        g = g.cpu().to(dtype)
        for k, q in enumerate(qs):
            q.grad = g[idx[k]].clone()
        torch.nn.utils.clip_grad_norm_(qs, max_norm=10.0)
        for k, grp in enumerate(opt.param_groups):
            grp["lr"] = lrs[t][k]
            if name == "RMSProp":
                grp["momentum"] = moms[t]
            else:
                grp["betas"] = (moms[t], 0.999)
        opt.step()
        flat = [torch.zeros(gid.numel(), dtype=torch.float64) for _ in range(3)]
        for k, q in enumerate(qs):
            flat[0][idx[k]] = q.detach().double()
            for j, key in enumerate(KEYS[name]):
                flat[1 + j][idx[k]] = opt.state[q][key].double()
        d = 0.9999 * (1 - math.exp(-(t + 1) / 2000))
        ema = ema * d + (1 - d) * flat[0].to(dtype)
        out.append((flat[0], flat[1], flat[2], ema.double()))
    return out


def _check(name, step, got, truth, own, ratios):
    """got: our (p, buf1, buf2, ema) on the GPU, truth / own: torch's f64 / f32 runs.  Applies the bound of the module docstring."""
    for what, x, w, o in zip(("p", KEYS[name][0], KEYS[name][1], "ema"), got, truth, own):
        E = float((o - w).abs().max())
        err = float((x.detach().double().cpu() - w).abs().max())
        bound = max(2e-6 * max(1.0, float(w.abs().max())), 4 * E)
        print(f"{name} step {step} {what}: err {err:.3e}  E {E:.3e}  bound {bound:.3e}  err/bound {err / bound:.3f}")
        ratios.append(err / bound)
        assert err <= bound, (name, step, what, err, E, bound)


def _new_state():
    st = torch.zeros(8, dtype=torch.float64, device="cuda")
    st[1] = 1.0
    return st


def _optim_step(name, p, g, b1, b2, ema, gid, lr, wd, mom, d, ss, state, n, loss_scale=None):
    from dedark_yolo_amd._C import OPT_RULES, call
    from dedark_yolo_amd.ops import ptr, stream
    call("dy_optim_step", OPT_RULES[name], ptr(p), ptr(g), ptr(b1), ptr(b2), ptr(ema), ptr(gid), lr[0], lr[1], lr[2], wd[0], wd[1], wd[2],
         mom, BETA2[name], 1e-8, 0.004, d, ptr(ss), 10.0, 1.0, ptr(loss_scale), ptr(state), n, stream())


def _sumsq(g, n):
    from dedark_yolo_amd._C import call
    from dedark_yolo_amd.ops import ptr, stream
    ss = torch.zeros(1, dtype=torch.float64, device="cuda")
    call("dy_sumsq", ptr(g), n, ptr(ss), stream())
    return ss


def _run_cabi(name, n, norms, seed=11):
    """`len(norms)` steps of dy_optim_step on a synthetic flat state of n elements; norms = the gradient norm of each step (max_norm is
    10).  About 1 % of the elements have an exactly zero gradient in every step: with no weight decay in their group that is Adamax's
    |g| + eps, RMSProp's sqrt(0) + eps and a zero exp_avg_sq under RAdam."""
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    gid = torch.randint(0, 3, (n,), generator=gen).to(torch.uint8)
    zero = torch.rand(n, generator=gen) < 0.01
    lr, wd = (1e-3, 2.5e-3, 4e-4), (5e-4, 0.0, 1e-4)
    grads = []
    for s in norms:
        g = torch.randn(n, generator=gen) * (s / math.sqrt(n))
        g[zero] = 0.0
        grads.append(g)
    steps = len(norms)
    truth = _torch_run(name, torch.float64, p0, gid, grads, [lr] * steps, wd, [0.9] * steps)
    own = _torch_run(name, torch.float32, p0, gid, grads, [lr] * steps, wd, [0.9] * steps)
    p, ema, gd = p0.cuda(), p0.cuda(), gid.cuda()
    b1, b2, state = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), _new_state()
    ratios = []
    for t in range(steps):
        g = grads[t].cuda()
        d = 0.9999 * (1 - math.exp(-(t + 1) / 2000))
        _optim_step(name, p, g, b1, b2, ema, gd, lr, wd, 0.9, d, _sumsq(g, n), state, n)
        torch.cuda.synchronize()
        _check(name, t + 1, (p, b1, b2, ema), truth[t], own[t], ratios)
    assert float(state[0]) == steps
    print(f"{name}: largest err / bound {max(ratios):.3f}")
    return ratios


@pytest.mark.parametrize("name", NAMES)
def test_optim_step_vs_torch(name):
    """n = 2048 * 256 + 15: 16-byte vectors and a 3-element scalar tail, more elements than a grid of one-element threads covers in one
    pass.  Steps 2, 4 and 7 are clipped.  7 steps with beta2 = 0.999 cross RAdam's rho_t > 5 between steps 5 and 6."""
    norms = [0.5, 30.0, 3.0, 80.0, 1.0, 0.2, 15.0]
    assert sum(s > 10.0 for s in norms) >= 2
    rho_inf = 2 / (1 - 0.999) - 1
    rho = [rho_inf - 2 * t * 0.999 ** t / (1 - 0.999 ** t) for t in range(1, len(norms) + 1)]
    assert any(r <= 5.0 for r in rho) and any(r > 5.0 for r in rho) and rho[4] <= 5.0 < rho[5]
    _run_cabi(name, 2048 * 256 + 15, norms)


def test_optim_step_vector_grid_stride():
    """The element kernel's grid is 2048 blocks of 256 threads with four elements per thread: 2048 * 256 * 4 + 7 elements take the
    grid-stride loop of the vector body (one vector) and the scalar tail.  The loop is shared by the five rules."""
    _run_cabi("NAdam", 2048 * 256 * 4 + 7, [0.5, 30.0])


@pytest.mark.parametrize("name", NAMES)
def test_optim_step_unaligned_buffers_take_the_scalar_loop(name):
    """Any n and any pointer are legal for a C-ABI caller: buffers that start one element past a 16-byte boundary (every element in
    the scalar loop) give the same result as aligned ones (vector body + tail) -- the same arithmetic per element, compared at f32
    round-off because the compiler may contract the two loops differently -- and nothing outside [0, n) is written."""
    n = 1003
    gen = torch.Generator().manual_seed(2)
    p0, g = torch.randn(n, generator=gen).cuda(), (torch.randn(n, generator=gen) * 0.1).cuda()
    gid = torch.randint(0, 3, (n,), generator=gen).to(torch.uint8).cuda()
    lr, wd = (1e-3, 2.5e-3, 4e-4), (5e-4, 0.0, 1e-4)
    ss = _sumsq(g, n)

    def run(shift):
        bases = [torch.zeros(n + 8, dtype=x.dtype, device="cuda") for x in (p0, g, p0, p0, p0, gid)]
        views = [b[shift:shift + n] for b in bases]
        for v, x in zip(views, (p0, g, None, None, p0, gid)):
            if x is not None:
                v.copy_(x)
        p, gg, b1, b2, ema, gi = views
        state = _new_state()
        for _ in range(2):
            _optim_step(name, p, gg, b1, b2, ema, gi, lr, wd, 0.9, 0.5, ss, state, n)
        torch.cuda.synchronize()
        for b in bases:
            assert float(b[:shift].abs().sum()) == 0.0 and float(b[shift + n:].abs().sum()) == 0.0
        return [v.clone() for v in (p, b1, b2, ema)]

    for a, b in zip(run(0), run(1)):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-9)
        assert float(a.abs().max()) > 0.0


def _tiny_trainer(optimizer, dtype="fp32"):
    import dedark_yolo_amd as dy
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    from dedark_yolo_amd.nn.tasks import DetectionModel
    dy.set_compute_dtype(torch.float32)
    cfgd = load_yaml("yolov8-lowlight.yaml")
    cfgd["scales"]["t"] = [0.33, 0.125, 1024]
    cfgd["scale"] = "t"
    torch.manual_seed(3)
    tr = DetectionTrainer(get_cfg(dict(model="tiny", dtype=dtype, optimizer=optimizer, batch=64, lowlight_FLAG=True, dedark_FLAG=True)))
    tr.setup(DetectionModel(cfgd, nc=20))
    return tr


@pytest.mark.parametrize("name", NAMES)
def test_trainer_optimizer_step_vs_torch(name):
    """DetectionTrainer.optimizer_step: 4 steps, per-group lr, another beta1 / momentum on step 1, steps 2 and 4 clipped."""
    tr = _tiny_trainer(name)
    flat = tr.flat
    assert tr.opt_name == name and tr.accumulate == 1 and flat.m2 is not None and flat.opt_state is not None
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(flat.n, generator=gen) * s / math.sqrt(flat.n) * 10 for s in (0.02, 3.0, 0.5, 40.0)]
    lrs = [[tr.lr0 * 0.7, tr.lr0 * 0.9, tr.lr0 * 1.3] if t % 2 == 0 else [tr.lr0] * 3 for t in range(4)]
    moms = [0.85] + [tr.momentum] * 3
    wds = (tr.weight_decay, 0.0, 0.0)
    p0 = flat.p.detach().cpu().clone()
    truth = _torch_run(name, torch.float64, p0, flat.gid, grads, lrs, wds, moms)
    own = _torch_run(name, torch.float32, p0, flat.gid, grads, lrs, wds, moms)
    ratios = []
    for t in range(4):
        flat.g.copy_(grads[t])
        tr.optimizer_step(lrs[t], moms[t])
        torch.cuda.synchronize()
        _check(name, t + 1, (flat.p, flat.m, flat.m2, flat.ema), truth[t], own[t], ratios)
    assert float(tr.optimizer_state_dict()["state"][0]["step"]) == 4.0


@pytest.mark.parametrize("name", NAMES)
def test_fp16_overflow_skips_the_step(name):
    """GradScaler.step after an inf: optimizer.step() is not called, so parameters, both buffers, torch's `step` and NAdam's
    `mu_product` stay; the EMA still moves; the scale halves.  The next finite step is the optimizer's FIRST (bias correction at 1)."""
    import dedark_yolo_amd as dy
    tr = _tiny_trainer(name, dtype="fp16")
    try:
        f = tr.flat
        gen = torch.Generator(device="cuda").manual_seed(5)
        g_true = torch.randn(f.n, device="cuda", generator=gen) * 1e-3
        f.g.copy_(g_true * 65536.0)
        f.g[7] = float("inf")
        p0, m0, v0, e0, s0 = f.p.clone(), f.m.clone(), f.m2.clone(), f.ema.clone(), f.opt_state.clone()
        tr.optimizer_step([0.01] * 3, 0.9)
        torch.cuda.synchronize()
        assert torch.equal(f.p, p0) and torch.equal(f.m, m0) and torch.equal(f.m2, v0)
        assert torch.equal(f.opt_state[:2], s0[:2]) and [float(v) for v in f.opt_state[:2]] == [0.0, 1.0]
        d = 0.9999 * (1 - math.exp(-tr.updates / 2000))
        assert torch.allclose(f.ema, d * e0 + (1 - d) * p0, rtol=1e-6, atol=1e-7)
        assert [float(v) for v in tr.loss_scale] == [32768.0, 0.0, 1.0]
        # a finite step at scale 32768 == the first step of a twin state through the unscaled path
        f.g.copy_(g_true * 32768.0)
        twin = [f.p.clone(), torch.zeros_like(f.m), torch.zeros_like(f.m2)]
        _optim_step(name, twin[0], g_true, twin[1], twin[2], None, f.gid, [0.01] * 3, (tr.weight_decay, 0.0, 0.0), 0.9, 0.0, _sumsq(g_true, f.n),
                    _new_state(), f.n)
        tr.optimizer_step([0.01] * 3, 0.9)
        torch.cuda.synchronize()
        for got, want in zip((f.p, f.m, f.m2), twin):
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-8)
        assert not torch.equal(f.p, p0)
        assert [float(v) for v in tr.loss_scale] == [32768.0, 1.0, 1.0]
        assert float(f.opt_state[0]) == 1.0
        assert float(tr.optimizer_state_dict()["state"][0]["step"]) == 1.0
    finally:
        dy.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("name", ["Adam", "NAdam"])
def test_resume_continues_bit_for_bit(name, tmp_path):
    """Two steps, save_model, resume_training into a fresh trainer, one more step with the same gradient in both: parameters, both
    buffers and the EMA are equal byte for byte, i.e. the step count (bias correction) and NAdam's mu_product came back exactly.  The
    checkpoint format keeps the weights in half precision (as the reference's does), so the first trainer continues from the values
    the checkpoint holds; the optimizer state is f32 in the file."""
    tr = _tiny_trainer(name)
    f = tr.flat
    gen = torch.Generator(device="cuda").manual_seed(8)
    real = torch.zeros(f.n, device="cuda")                  # the slots are padded to 4 elements: a backward pass leaves the padding's
    for _, o, n, _ in f.slots:                              # gradient (and with it its parameter and state) at zero, a checkpoint has no
        real[o:o + n] = 1.0                                 # place for it
    for _ in range(2):
        f.g.copy_(torch.randn(f.n, device="cuda", generator=gen) * 1e-2 * real)
        tr.optimizer_step([0.01, 0.008, 0.012], 0.9)
    last = tr.save_model(str(tmp_path), epoch=0)
    f.p.copy_(f.p.half().float())
    f.ema.copy_(f.ema.half().float())
    tr2 = _tiny_trainer(name)
    tr2.resume_training(last)
    f2 = tr2.flat
    assert torch.equal(f2.opt_state[:2], f.opt_state[:2]) and float(f2.opt_state[0]) == 2.0
    assert torch.equal(f2.p, f.p) and torch.equal(f2.m, f.m) and torch.equal(f2.m2, f.m2) and torch.equal(f2.ema, f.ema)
    g = torch.randn(f.n, device="cuda", generator=gen) * 1e-2 * real
    for t in (tr, tr2):
        t.flat.g.copy_(g)
        t.optimizer_step([0.01, 0.008, 0.012], 0.9)
    torch.cuda.synchronize()
    for a, b in ((f.p, f2.p), (f.m, f2.m), (f.m2, f2.m2), (f.ema, f2.ema)):
        assert torch.equal(a, b)
    assert float(f2.opt_state[0]) == 3.0
    with pytest.raises(RuntimeError, match="does not belong to SGD"):
        _tiny_trainer("SGD").resume_training(last)
