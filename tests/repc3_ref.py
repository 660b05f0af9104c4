"""Host statement of the two-branch BatchNorm + activation stage (csrc/bn2act.hip: dy_bn2_act_fwd / dy_bn2_act_bwd) and its adjoint,
and of RepConv / RepC3 (nn/modules.py) forward and backward, written out by hand in torch: the yardstick of
tests/test_gpu_bn2act.py, itself checked against the reference's fixtures in tests/test_repc3_cpu.py.

Activations are [pixels, C] for the stage and [B, C, H, W] for the blocks.  Every function runs in the dtype `dt` it is given: float64
is the reference, float32 the run whose own error E sets the tests' allowance.  The *_terms functions give, per output element, the
sum of the magnitudes of the terms that form it (the denominator of the tests' error measure), first order in the errors of the
inputs of each step.
"""
import torch
import torch.nn.functional as F

F64 = torch.float64
ACT_NONE, ACT_SILU, ACT_LEAKY = 0, 1, 2
BN_EPS, BN_MOMENTUM = 1e-3, 0.03


def _d(t, dt=F64):
    return None if t is None else torch.as_tensor(t).to(dt)


def act(code, z):
    if code == ACT_SILU:
        return z * torch.sigmoid(z)
    if code == ACT_LEAKY:
        return torch.where(z > 0, z, 0.1 * z)
    return z


def dact(code, z):
    if code == ACT_SILU:
        s = torch.sigmoid(z)
        return s * (1.0 + z * (1.0 - s))
    if code == ACT_LEAKY:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.1))
    return torch.ones_like(z)


def d2act(code, z):
    """|act''| (SiLU only; LeakyReLU away from its kink and the identity have none)"""
    if code == ACT_SILU:
        s = torch.sigmoid(z)
        return (s * (1.0 - s) * (2.0 + z * (1.0 - 2.0 * s))).abs()
    return torch.zeros_like(z)


def bn_stats(z, gamma, beta, eps=BN_EPS):
    """what dy_bn_finalize_valid hands the stage for the raw map z [pixels, C]: scale, shift, mean, invstd (biased variance)"""
    z, gamma, beta = _d(z), _d(gamma), _d(beta)
    mean = z.mean(0)
    invstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(0) + eps)
    scale = gamma * invstd
    return scale, beta - mean * scale, mean, invstd


# ------------------------------------------------------------------------------------------------------- the two-branch stage
def bn2_forward(u, v, su, hu, sv, hv, code, dt=F64):
    """y = act(u su + hu + v sv + hv)"""
    u, v, su, hu, sv, hv = (_d(t, dt) for t in (u, v, su, hu, sv, hv))
    return act(code, u * su + hu + v * sv + hv)


def _tz(u, v, su, hu, sv, hv):
    return (u * su).abs() + hu.abs() + (v * sv).abs() + hv.abs()


def bn2_forward_terms(u, v, su, hu, sv, hv, code):
    u, v, su, hu, sv, hv = (_d(t) for t in (u, v, su, hu, sv, hv))
    z = u * su + hu + v * sv + hv
    return dact(code, z).abs() * _tz(u, v, su, hu, sv, hv) + act(code, z).abs()


def bn2_backward(dy, u, v, bu, bv, code, dt=F64):
    """bu / bv = (scale, shift, mean, invstd, gamma) of a branch.  Returns du, dv, dgamma_u, dbeta, dgamma_v (dbeta_u == dbeta_v)."""
    dy, u, v = _d(dy, dt), _d(u, dt), _d(v, dt)
    su, hu, mu, iu, gu = (_d(t, dt) for t in bu)
    sv, hv, mv, iv, gv = (_d(t, dt) for t in bv)
    M = u.shape[0]
    g = dy * dact(code, u * su + hu + v * sv + hv)
    uh, vh = (u - mu) * iu, (v - mv) * iv
    s0, s1, s2 = g.sum(0), (g * uh).sum(0), (g * vh).sum(0)
    du = gu * iu * (g - s0 / M - uh * s1 / M)
    dv = gv * iv * (g - s0 / M - vh * s2 / M)
    return du, dv, s1, s0, s2


def bn2_backward_terms(dy, u, v, bu, bv, code):
    dy, u, v = _d(dy), _d(u), _d(v)
    su, hu, mu, iu, gu = (_d(t) for t in bu)
    sv, hv, mv, iv, gv = (_d(t) for t in bv)
    M = u.shape[0]
    z = u * su + hu + v * sv + hv
    g = dy * dact(code, z)
    tg = dy.abs() * (dact(code, z).abs() + d2act(code, z) * _tz(u, v, su, hu, sv, hv))
    ts0 = tg.sum(0)
    out = []
    for x, m, i, gm in ((u, mu, iu, gu), (v, mv, iv, gv)):
        xh, txh = (x - m) * i, (x.abs() + m.abs()) * i
        s = (g * xh).sum(0)
        ts = (tg * xh.abs() + g.abs() * txh).sum(0)
        out.append(((gm * i).abs() * (tg + ts0 / M + txh * s.abs() / M + xh.abs() * ts / M), ts))
    (tdu, ts1), (tdv, ts2) = out
    return tdu, tdv, ts1, ts0, ts2


# ------------------------------------------------------------------------------------------------------- RepConv / RepC3
def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _map(r, like):
    B, _, H, W = like.shape
    return r.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _bn_eval(P, pre, eps=BN_EPS):
    sc = P[pre + "bn.weight"] / torch.sqrt(P[pre + "bn.running_var"] + eps)
    return sc, P[pre + "bn.bias"] - P[pre + "bn.running_mean"] * sc


def _running(P, pre, z, out, momentum=BN_MOMENTUM):
    """the running buffers after one training forward over the raw map z [pixels, C] (unbiased variance)"""
    n = z.shape[0]
    var = z.var(0, unbiased=False)
    out[pre + "bn.running_mean"] = (1 - momentum) * P[pre + "bn.running_mean"] + momentum * z.mean(0)
    out[pre + "bn.running_var"] = (1 - momentum) * P[pre + "bn.running_var"] + momentum * var * (n / (n - 1) if n > 1 else 1.0)


def conv_bn_act_forward(P, pre, x, code, train, k, buffers=None):
    """a Conv module (conv k x k 'same' + BatchNorm + act); returns y and what the backward needs"""
    w = P[pre + "conv.weight"]
    z = F.conv2d(x, w, None, 1, k // 2)
    zr = _rows(z)
    if train:
        sc, sh, mean, invstd = bn_stats(zr, P[pre + "bn.weight"], P[pre + "bn.bias"])
        buffers is not None and _running(P, pre, zr, buffers)
    else:
        (sc, sh), mean, invstd = _bn_eval(P, pre), None, None
    y = act(code, zr * sc + sh)
    return _map(y, z), dict(pre=pre, x=x, w=w, zr=zr, aff=(sc, sh, mean, invstd, P[pre + "bn.weight"]), code=code, k=k)


def conv_bn_act_backward(c, dy, grads):
    sc, sh, mean, invstd, gamma = c["aff"]
    zr, M = c["zr"], c["zr"].shape[0]
    g = _rows(dy) * dact(c["code"], zr * sc + sh)
    zh = (zr - mean) * invstd
    s0, s1 = g.sum(0), (g * zh).sum(0)
    grads[c["pre"] + "bn.weight"], grads[c["pre"] + "bn.bias"] = s1, s0
    return _conv_grads(c, _map(gamma * invstd * (g - s0 / M - zh * s1 / M), dy), grads)


def _conv_grads(c, dz, grads):
    grads[c["pre"] + "conv.weight"] = torch.nn.grad.conv2d_weight(c["x"], c["w"].shape, dz, 1, c["k"] // 2)
    return torch.nn.grad.conv2d_input(c["x"].shape, c["w"], dz, 1, c["k"] // 2)


def repconv_forward(P, pre, x, code, train, buffers=None):
    """act(bn1(conv3x3(x)) + bn2(conv1x1(x))) from the parameter dict P (keys pre + 'conv1.conv.weight', ...), all in P's dtype"""
    br = []
    for name, k in (("conv1.", 3), ("conv2.", 1)):
        p = pre + name
        w = P[p + "conv.weight"]
        zr = _rows(F.conv2d(x, w, None, 1, k // 2))
        if train:
            aff = (*bn_stats(zr, P[p + "bn.weight"], P[p + "bn.bias"]), P[p + "bn.weight"])
            buffers is not None and _running(P, p, zr, buffers)
        else:
            aff = (*_bn_eval(P, p), None, None, P[p + "bn.weight"])
        br.append(dict(pre=p, x=x, w=w, zr=zr, aff=aff, k=k))
    a, b = br
    y = bn2_forward(a["zr"], b["zr"], a["aff"][0], a["aff"][1], b["aff"][0], b["aff"][1], code, x.dtype)
    return _map(y, x), dict(a=a, b=b, code=code)


def repconv_backward(c, dy, grads):
    a, b = c["a"], c["b"]
    du, dv, dgu, db, dgv = bn2_backward(_rows(dy), a["zr"], b["zr"], a["aff"], b["aff"], c["code"], dy.dtype)
    grads[a["pre"] + "bn.weight"], grads[a["pre"] + "bn.bias"] = dgu, db
    grads[b["pre"] + "bn.weight"], grads[b["pre"] + "bn.bias"] = dgv, db
    return _conv_grads(a, _map(du, dy), grads) + _conv_grads(b, _map(dv, dy), grads)


def repconv_fused(P, pre, eps=BN_EPS):
    """get_equivalent_kernel_bias: W = W3 t3 + pad(W1 t1), b = b3 + b1"""
    s3, b3 = _bn_eval(P, pre + "conv1.", eps)
    s1, b1 = _bn_eval(P, pre + "conv2.", eps)
    return (P[pre + "conv1.conv.weight"] * s3.reshape(-1, 1, 1, 1) + F.pad(P[pre + "conv2.conv.weight"] * s1.reshape(-1, 1, 1, 1), [1, 1, 1, 1]),
            b3 + b1)


def repconv_fused_forward(P, pre, x, code):
    w, b = repconv_fused(P, pre)
    return act(code, F.conv2d(x, w, b, 1, 1))


def repc3_forward(P, x, n, train, buffers=None, fused=False):
    """m(cv1(x)) + cv2(x) (cv3 = Identity: e == 1.0)"""
    t, c1 = conv_bn_act_forward(P, "cv1.", x, ACT_SILU, train, 1, buffers)
    y2, c2 = conv_bn_act_forward(P, "cv2.", x, ACT_SILU, train, 1, buffers)
    ms = []
    for i in range(n):
        if fused:
            t = repconv_fused_forward(P, f"m.{i}.", t, ACT_SILU)
        else:
            t, c = repconv_forward(P, f"m.{i}.", t, ACT_SILU, train, buffers)
            ms.append(c)
    return t + y2, dict(c1=c1, c2=c2, ms=ms)


def repc3_backward(c, dy, grads):
    g = dy
    for cm in reversed(c["ms"]):
        g = repconv_backward(cm, g, grads)
    return conv_bn_act_backward(c["c1"], g, grads) + conv_bn_act_backward(c["c2"], dy, grads)
