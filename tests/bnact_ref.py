"""Host statement of the single-branch BatchNorm + activation stage (csrc/bnact.hip: dy_bn_act_fwd, dy_bn_act_bwd_reduce,
dy_bn_act_bwd_apply[_valid], dy_bn_act_bwd[_valid]) written out by hand in torch: the yardstick of tests/test_gpu_bnact_kernels.py,
itself checked against float64 autograd in tests/test_bnact_ref_cpu.py.

Activations are [pixels, C].  scale / shift / mean / invstd / gamma are per-channel; scale = None stands for 1 and shift = None
for 0 (the kernels' NULL pointers).  Every function runs in the dtype `dt` it is given: float64 is the reference, float32 the run
whose own error E sets the tests' allowance.  The *_terms functions give, per output element, the sum of the magnitudes of the
terms that form it (the denominator of the tests' error measure), first order in the errors of the inputs of each step, the way
repc3_ref's bn2_*_terms do.
"""
import torch

from repc3_ref import F64, _d, act, bn_stats, d2act, dact  # noqa: F401  (bn_stats: re-exported for the tests)


def _u(z, scale, shift):
    u = z if scale is None else z * scale
    return u if shift is None else u + shift


def _tu(z, scale, shift):
    t = z.abs() if scale is None else (z * scale).abs()
    return t if shift is None else t + shift.abs()


def forward(z, scale, shift, code, res=None, dt=F64):
    """y = act(z scale + shift) (+ res)"""
    z, scale, shift, res = (_d(t, dt) for t in (z, scale, shift, res))
    y = act(code, _u(z, scale, shift))
    return y if res is None else y + res


def forward_terms(z, scale, shift, code, res=None):
    """|act'(u)| (|z scale| + |shift|) + |act(u)| (+ |res|)"""
    z, scale, shift, res = (_d(t) for t in (z, scale, shift, res))
    u = _u(z, scale, shift)
    t = dact(code, u).abs() * _tu(z, scale, shift) + act(code, u).abs()
    return t if res is None else t + res.abs()


def backward(dy, z, scale, shift, mean, invstd, gamma, code, has_bn, C_valid, dt=F64):
    """g = dy act'(u), u = z scale + shift; S0 = sum g, S1 = sum g zhat with zhat = (z - mean) invstd (0 without BatchNorm).
    With BatchNorm dz = gamma invstd (g - S0 / M - zhat S1 / M) on the C_valid real channels and 0 on the rest (gamma is C_valid
    long); without, dz = g on every channel.  Returns dz, dgamma (None without BatchNorm), dbeta, S0, S1; dgamma = S1[:C_valid],
    dbeta = S0[:C_valid]."""
    dy, z, scale, shift, mean, invstd, gamma = (_d(t, dt) for t in (dy, z, scale, shift, mean, invstd, gamma))
    M, C = z.shape
    g = dy * dact(code, _u(z, scale, shift))
    s0 = g.sum(0)
    if not has_bn:
        return g, None, s0[:C_valid], s0, torch.zeros_like(s0)
    zh = (z - mean) * invstd
    s1 = (g * zh).sum(0)
    k1 = torch.zeros(C, dtype=dt)
    k1[:C_valid] = (torch.ones(C_valid, dtype=dt) if gamma is None else gamma[:C_valid]) * invstd[:C_valid]
    dz = k1 * (g - s0 / M - zh * s1 / M)
    return dz, s1[:C_valid], s0[:C_valid], s0, s1


def backward_terms(dy, z, scale, shift, mean, invstd, gamma, code, has_bn, C_valid):
    """the sums of magnitudes behind dz, dgamma, dbeta, S0, S1, in backward's order"""
    dy, z, scale, shift, mean, invstd, gamma = (_d(t) for t in (dy, z, scale, shift, mean, invstd, gamma))
    M, C = z.shape
    u = _u(z, scale, shift)
    g = dy * dact(code, u)
    tg = dy.abs() * (dact(code, u).abs() + d2act(code, u) * _tu(z, scale, shift))
    ts0 = tg.sum(0)
    if not has_bn:
        return tg, None, ts0[:C_valid], ts0, torch.zeros_like(ts0)
    zh, tzh = (z - mean) * invstd, (z.abs() + mean.abs()) * invstd
    s1 = (g * zh).sum(0)
    ts1 = (tg * zh.abs() + g.abs() * tzh).sum(0)
    k1 = torch.zeros(C, dtype=F64)
    k1[:C_valid] = ((torch.ones(C_valid, dtype=F64) if gamma is None else gamma[:C_valid]) * invstd[:C_valid]).abs()
    tdz = k1 * (tg + ts0 / M + tzh * s1.abs() / M + zh.abs() * ts1 / M)
    return tdz, ts1[:C_valid], ts0[:C_valid], ts0, ts1
