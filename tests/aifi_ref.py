"""float64 torch statement of the transformer encoder layer's kernels (csrc/layernorm.hip: dy_add_layernorm_fwd / _bwd, dy_gelu_fwd /
_bwd, dy_add_pos) and of the whole post-norm layer (nn/modules.py: TransformerEncoderLayer / AIFI), forward and backward, written
out by hand: the yardstick of tests/test_gpu_layernorm.py, itself checked against torch's autograd through nn.LayerNorm / nn.GELU /
nn.MultiheadAttention in tests/test_aifi_cpu.py.

Tokens are rows: every activation is [rows, C] (or [B, L, C]) float64.  The *_terms functions give, per output element, the sum of
the magnitudes of the terms that form it (the denominator of the tests' error measure), first order in the errors of the inputs of
each step.
"""
import math

import torch

F64 = torch.float64


def _d(t):
    return None if t is None else torch.as_tensor(t).to(F64)


# ---------------------------------------------------------------------------------------------------------------- add + LayerNorm
def ln_forward(a, b, gamma, beta, eps):
    """y [rows, C], mean [rows], rstd [rows] of LayerNorm(a + b); biased variance of the centred values"""
    a, b, gamma, beta = _d(a), _d(b), _d(gamma), _d(beta)
    z = a if b is None else a + b
    mean = z.mean(-1)
    d = z - mean[..., None]
    rstd = 1.0 / torch.sqrt((d * d).mean(-1) + eps)
    return d * rstd[..., None] * gamma + beta, mean, rstd


def _tz(a, b, mean, rstd):
    """sum of the magnitudes behind z^ = (a + b - mean) rstd: (|a| + |b| + mean_j(|a_j| + |b_j|)) rstd >= |z^|"""
    za = a.abs() if b is None else a.abs() + b.abs()
    return (za + za.mean(-1, keepdim=True)) * rstd[..., None]


def ln_forward_terms(a, b, gamma, beta, eps):
    """terms of y, of mean and of rstd (rstd: its own magnitude plus what the errors of the centred values do to the variance)"""
    a, b, gamma, beta = _d(a), _d(b), _d(gamma), _d(beta)
    _, mean, rstd = ln_forward(a, b, gamma, beta, eps)
    za = a.abs() if b is None else a.abs() + b.abs()
    z = a if b is None else a + b
    d = z - mean[..., None]
    ty = _tz(a, b, mean, rstd) * gamma.abs() + beta.abs()
    tm = za.mean(-1)
    tr = rstd * (1.0 + (d.abs() * (za + tm[..., None])).mean(-1) * rstd * rstd)
    return ty, tm, tr


def ln_backward(a, b, mean, rstd, gamma, dy, dz_old=None):
    """dz (the gradient of a and of b; + dz_old), dgamma, dbeta from the inputs the kernel gets"""
    a, b, mean, rstd, gamma, dy = _d(a), _d(b), _d(mean), _d(rstd), _d(gamma), _d(dy)
    z = a if b is None else a + b
    zh = (z - mean[..., None]) * rstd[..., None]
    g = dy * gamma
    dz = rstd[..., None] * (g - g.mean(-1, keepdim=True) - zh * (g * zh).mean(-1, keepdim=True))
    if dz_old is not None:
        dz = dz + _d(dz_old)
    C = a.shape[-1]
    return dz, (dy * zh).reshape(-1, C).sum(0), dy.reshape(-1, C).sum(0)


def ln_backward_terms(a, b, mean, rstd, gamma, dy, dz_old=None):
    a, b, mean, rstd, gamma, dy = _d(a), _d(b), _d(mean), _d(rstd), _d(gamma), _d(dy)
    z = a if b is None else a + b
    zh = ((z - mean[..., None]) * rstd[..., None]).abs()
    tz = _tz(a, b, mean, rstd)
    g = (dy * gamma).abs()
    t = rstd[..., None] * (g + g.mean(-1, keepdim=True) + tz * (g * zh).mean(-1, keepdim=True) + zh * (g * tz).mean(-1, keepdim=True))
    if dz_old is not None:
        t = t + _d(dz_old).abs()
    C = a.shape[-1]
    return t, (dy.abs() * tz).reshape(-1, C).sum(0), dy.abs().reshape(-1, C).sum(0)


# ---------------------------------------------------------------------------------------------------------------- exact GELU
def gelu_forward(u):
    u = _d(u)
    return 0.5 * u * torch.erfc(-u / math.sqrt(2.0))           # = 0.5 u (1 + erf(u / sqrt 2)) without the cancellation at u << 0


def gelu_forward_terms(u):
    u = _d(u)
    return 0.5 * u.abs() * (1.0 + torch.erf(u / math.sqrt(2.0)).abs())


def gelu_backward(u, dy):
    u, dy = _d(u), _d(dy)
    cdf = 0.5 * torch.erfc(-u / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    return dy * (cdf + u * pdf)


def gelu_backward_terms(u, dy):
    u, dy = _d(u), _d(dy)
    pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    return dy.abs() * (0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)).abs()) + u.abs() * pdf)


# ---------------------------------------------------------------------------------------------------------------- position table
def pos_table(w, h, c, temperature=10000.0):
    """the 2D sine-cosine table in float32 arithmetic on the CPU, [w h, c]: row p = (iw, ih) = (p // h, p % h), columns
    sin(iw om) | cos(iw om) | sin(ih om) | cos(ih om), om_k = temperature^(-k / (c / 4))"""
    assert c % 4 == 0
    iw = torch.arange(int(w), dtype=torch.float32).repeat_interleave(int(h))
    ih = torch.arange(int(h), dtype=torch.float32).repeat(int(w))
    pd = c // 4
    om = 1.0 / (temperature ** (torch.arange(pd, dtype=torch.float32) / pd))
    ow, oh = iw[:, None] @ om[None], ih[:, None] @ om[None]
    return torch.cat([torch.sin(ow), torch.cos(ow), torch.sin(oh), torch.cos(oh)], 1)


# ---------------------------------------------------------------------------------------------------------------- the whole layer
def _heads(t, H):
    B, L, C = t.shape
    return t.reshape(B, L, H, C // H).permute(0, 2, 1, 3)


def _tokens(t):
    B, H, L, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, L, H * D)


def layer_forward(P, x, pos, heads, eps=1e-5):
    """P: dict of the layer's state_dict tensors (ma.in_proj_weight, ..., norm2.bias); x [B, L, C]; pos [L, C] or None.
    Returns y and the cache layer_backward needs."""
    P = {k: _d(v) for k, v in P.items()}
    x, pos = _d(x), _d(pos)
    C = x.shape[-1]
    wi, bi = P["ma.in_proj_weight"], P["ma.in_proj_bias"]
    p = x if pos is None else x + pos
    q, k, v = p @ wi[:C].T + bi[:C], p @ wi[C:2 * C].T + bi[C:2 * C], x @ wi[2 * C:].T + bi[2 * C:]
    qh, kh, vh = _heads(q, heads), _heads(k, heads), _heads(v, heads)
    scale = (C // heads) ** -0.5
    prob = torch.softmax(scale * (qh @ kh.transpose(2, 3)), -1)
    a = _tokens(prob @ vh)
    s2 = a @ P["ma.out_proj.weight"].T + P["ma.out_proj.bias"]
    x1, m1, r1 = ln_forward(x, s2, P["norm1.weight"], P["norm1.bias"], eps)
    u = x1 @ P["fc1.weight"].T + P["fc1.bias"]
    t = gelu_forward(u)
    s3 = t @ P["fc2.weight"].T + P["fc2.bias"]
    y, m2, r2 = ln_forward(x1, s3, P["norm2.weight"], P["norm2.bias"], eps)
    return y, dict(P=P, x=x, p=p, qh=qh, kh=kh, vh=vh, prob=prob, a=a, s2=s2, x1=x1, m1=m1, r1=r1, u=u, t=t, s3=s3, m2=m2, r2=r2,
                   heads=heads, scale=scale)


def layer_backward(c, dy):
    """dx and the dict of parameter gradients (state_dict names) for the upstream gradient dy"""
    P, dy = c["P"], _d(dy)
    C = dy.shape[-1]
    f2 = lambda t: t.reshape(-1, t.shape[-1])
    G = {}
    dz2, G["norm2.weight"], G["norm2.bias"] = ln_backward(c["x1"], c["s3"], c["m2"], c["r2"], P["norm2.weight"], dy)
    G["fc2.weight"], G["fc2.bias"] = f2(dz2).T @ f2(c["t"]), f2(dz2).sum(0)
    du = gelu_backward(c["u"], dz2 @ P["fc2.weight"])
    G["fc1.weight"], G["fc1.bias"] = f2(du).T @ f2(c["x1"]), f2(du).sum(0)
    dx1 = du @ P["fc1.weight"] + dz2
    dz1, G["norm1.weight"], G["norm1.bias"] = ln_backward(c["x"], c["s2"], c["m1"], c["r1"], P["norm1.weight"], dx1)
    G["ma.out_proj.weight"], G["ma.out_proj.bias"] = f2(dz1).T @ f2(c["a"]), f2(dz1).sum(0)
    dah = _heads(dz1 @ P["ma.out_proj.weight"], c["heads"])
    prob, qh, kh, vh = c["prob"], c["qh"], c["kh"], c["vh"]
    dv = prob.transpose(2, 3) @ dah
    dp = dah @ vh.transpose(2, 3)
    ds = prob * (dp - (dp * prob).sum(-1, keepdim=True))
    dq, dk, dv = _tokens(c["scale"] * (ds @ kh)), _tokens(c["scale"] * (ds.transpose(2, 3) @ qh)), _tokens(dv)
    wi = P["ma.in_proj_weight"]
    G["ma.in_proj_weight"] = torch.cat([f2(dq).T @ f2(c["p"]), f2(dk).T @ f2(c["p"]), f2(dv).T @ f2(c["x"])])
    G["ma.in_proj_bias"] = torch.cat([f2(dq).sum(0), f2(dk).sum(0), f2(dv).sum(0)])
    dx = dz1 + dq @ wi[:C] + dk @ wi[C:2 * C] + dv @ wi[2 * C:]
    return dx, G


# ---------------------------------------------------------------------------------------------------------------- fixture inputs
def rect_batch(seed, B, H, W, nbox, nc=20):
    """a training batch on H x W images (tests/util.make_batch for a map that need not be square): the inputs of the model fixtures
    of tests/golden/make_aifi_golden.py and of the tests that replay them"""
    import numpy as np
    g = np.random.default_rng(seed)
    img = torch.from_numpy(g.random((B, 3, H, W), dtype=np.float32))
    bi, cls, bb = [], [], []
    for b in range(B):
        for _ in range(nbox[b]):
            bi.append(b)
            cls.append(int(g.integers(0, nc)))
            cx, cy = g.uniform(0.25, 0.75, 2)
            w, h = g.uniform(0.15, 0.5, 2)
            bb.append([cx, cy, w, h])
    return dict(img=img, batch_idx=torch.tensor(bi, dtype=torch.float32), cls=torch.tensor(cls, dtype=torch.float32).view(-1, 1),
                bboxes=torch.tensor(bb, dtype=torch.float32).view(-1, 4))
