"""tests/bnact_ref.py (the float64 yardstick of tests/test_gpu_bnact_kernels.py) against torch autograd in float64: the graph
F.batch_norm(training=True, eps 1e-3) -> activation -> + res, and the bias-only graph act(z + b) of a conv without BatchNorm.
y, dz, dgamma, dbeta and dres agree to 1e-12 of the largest reference value of each tensor.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import bnact_ref as br
from repc3_ref import ACT_LEAKY, ACT_NONE, ACT_SILU, BN_EPS

F64 = torch.float64
ACTS = {"silu": ACT_SILU, "none": ACT_NONE, "leaky": ACT_LEAKY}
TOL = 1e-12


def _act(u, code):
    return F.silu(u) if code == ACT_SILU else (F.leaky_relu(u, 0.1) if code == ACT_LEAKY else u)


def _close(what, got, want):
    err = float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)
    assert err <= TOL, (what, err)


def _data(px, C, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)          # noqa: E731
    return 1.5 * r(px, C) + 0.3, r(px, C), r(px, C), 1.0 + 0.3 * r(C), 0.3 * r(C)


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("px,C,Cv", [(2, 8, 8), (7, 24, 21), (64, 12, 12), (257, 8, 5)])
@pytest.mark.parametrize("use_res", [False, True], ids=["plain", "res"])
def test_bn_act_graph(px, C, Cv, act, use_res):
    """C_valid < C: the stage is the C_valid-channel graph, the pad channels see scale = shift = mean = invstd = 0 (what
    dy_bn_finalize_valid writes there) and get dz = 0"""
    code = ACTS[act]
    z, dy, res, gamma, beta = _data(px, C, px * 31 + C)
    gamma, beta = gamma[:Cv], beta[:Cv]
    res = res if use_res else None
    zz, gg, bb = (t.clone().requires_grad_(True) for t in (z[:, :Cv], gamma, beta))
    rr = res[:, :Cv].clone().requires_grad_(True) if use_res else None
    y = _act(F.batch_norm(zz.t()[None], None, None, gg, bb, training=True, eps=BN_EPS)[0].t(), code)
    y = y + rr if use_res else y
    y.backward(dy[:, :Cv])

    aff = [torch.zeros(C, dtype=F64) for _ in range(4)]
    for dst, src in zip(aff, br.bn_stats(z[:, :Cv], gamma, beta)):
        dst[:Cv] = src
    scale, shift, mean, invstd = aff
    got_y = br.forward(z, scale, shift, code, res)
    dz, dgamma, dbeta, s0, s1 = br.backward(dy, z, scale, shift, mean, invstd, gamma, code, 1, Cv)
    _close("y", got_y[:, :Cv], y.detach())
    pad = br.forward(z, scale, shift, code)[:, Cv:]
    assert bool((pad == 0).all())                                   # act(0) = 0 for all three activations
    _close("dz", dz[:, :Cv], zz.grad)
    assert bool((dz[:, Cv:] == 0).all())
    _close("dgamma", dgamma, gg.grad)
    _close("dbeta", dbeta, bb.grad)
    assert dgamma.shape == dbeta.shape == (Cv,) and s0.shape == s1.shape == (C,)
    assert torch.equal(dgamma, s1[:Cv]) and torch.equal(dbeta, s0[:Cv])
    if use_res:
        _close("dres", dy[:, :Cv], rr.grad)                         # the residual's gradient is dy itself
    for t, ref in zip(br.backward_terms(dy, z, scale, shift, mean, invstd, gamma, code, 1, Cv), (dz, dgamma, dbeta, s0, s1)):
        assert t.shape == ref.shape and bool((t >= ref.abs() * (1 - 1e-12)).all())       # a sum of magnitudes bounds its sum
    t = br.forward_terms(z, scale, shift, code, res)
    assert bool((t >= got_y.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("px,C,Cv", [(1, 8, 8), (7, 24, 21), (130, 4, 3)])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
def test_bias_only_graph(px, C, Cv, act, with_bias):
    """no BatchNorm: y = act(z + b), dz = dy act'(z + b) on every channel, dbias = column sums of dz (C_valid of them)"""
    code = ACTS[act]
    z, dy, _, _, b = _data(px, C, px * 17 + C)
    zz, bb = z.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = _act(zz + bb if with_bias else zz, code)
    y.backward(dy)
    shift = b if with_bias else None
    _close("y", br.forward(z, None, shift, code), y.detach())
    dz, dgamma, dbeta, s0, s1 = br.backward(dy, z, None, shift, None, None, None, code, 0, Cv)
    _close("dz", dz, zz.grad)
    assert dgamma is None and bool((s1 == 0).all())
    want_db = bb.grad if with_bias else zz.grad.sum(0)
    _close("dbeta", dbeta, want_db[:Cv])
    _close("S0", s0, want_db)
    tdz, tdg, tdb, ts0, ts1 = br.backward_terms(dy, z, None, shift, None, None, None, code, 0, Cv)
    assert tdg is None and bool((ts1 == 0).all()) and bool((tdz >= dz.abs() * (1 - 1e-12)).all())
    assert bool((ts0 >= s0.abs() * (1 - 1e-12)).all()) and torch.equal(tdb, ts0[:Cv])


def test_f32_run_is_the_same_formula():
    """dt = float32 evaluates the same statement in f32 (the tests' E): close to the float64 run, and float32 throughout"""
    z, dy, res, gamma, beta = _data(64, 8, 5)
    aff = [t.float() for t in br.bn_stats(z.float(), gamma.float(), beta.float())]
    args = (dy.float(), z.float(), *aff, gamma.float(), ACT_SILU, 1, 8)
    for a, b in zip(br.backward(*args, dt=torch.float32), br.backward(*args)):
        assert a.dtype == torch.float32 and b.dtype == F64
        assert float((a.double() - b).abs().max()) <= 1e-4 * float(b.abs().max())
    y32 = br.forward(z.float(), aff[0], aff[1], ACT_SILU, res.float(), dt=torch.float32)
    assert y32.dtype == torch.float32
    assert float((y32.double() - br.forward(z.float(), aff[0], aff[1], ACT_SILU, res.float())).abs().max()) <= 1e-5
