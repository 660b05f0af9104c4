"""Float64 statement of the channel / spatial attention blocks (reference ultralytics/nn/modules/conv.py:294-320, 449-459) in numpy,
forward and backward, split at the same places as the C-ABI entries of csrc/cbam.hip so that every entry can be checked alone.

Layout: maps are NHWC arrays [B, H, W, C]; a = the fc's logits [B, C] (None: no channel gate, SpatialAttention alone); planes are
[B, H, W]; w = cv1.weight [1, 2, k, k] (plane 0 = mean, plane 1 = max), zero padding k // 2.

    g = sigmoid(a), u = x g, m = (mean_c u, max_c u), s = sigmoid(conv(m)), y = u s

Ties of the channel max go to the FIRST (lowest) channel index, torch.max's rule on the CPU.  Every function also returns `terms`,
the sum of the absolute addends behind each output element (the error measure of tests/test_gpu_attn.py: |got - ref| / terms).

`variant` selects one of eight deliberately WRONG arithmetics (tests/test_cbam_cpu.py shows that the chosen cases tell each of them
from the right one): swap_planes, no_inv_c, unflipped, edge_clamp, last_tie, max_of_x, no_dsigmoid, pad3_k3.
"""
import numpy as np

VARIANTS = ("swap_planes", "no_inv_c", "unflipped", "edge_clamp", "last_tie", "max_of_x", "no_dsigmoid", "pad3_k3")


def sigmoid(z):
    z = np.asarray(z, dtype=np.float64)
    return 1.0 / (1.0 + np.exp(-z))


def gate(a, like):
    """g [B, 1, 1, C] (ones without a gate)"""
    B, C = like.shape[0], like.shape[-1]
    return np.ones((B, 1, 1, C)) if a is None else sigmoid(a).reshape(B, 1, 1, C)


def nhwc(t):
    """NCHW array -> NHWC float64"""
    return np.ascontiguousarray(np.transpose(np.asarray(t, dtype=np.float64), (0, 2, 3, 1)))


def nchw(t):
    return np.ascontiguousarray(np.transpose(t, (0, 3, 1, 2)))


# ------------------------------------------------------------------------------------------------ forward
def chan_gate(x, a):
    y = np.asarray(x, np.float64) * gate(a, x)
    return y, np.abs(y)


def stats(x, a, variant=None):
    """-> dict(mean, mx, arg, mean_terms, mx_terms, gap): gap = per pixel, largest minus second largest u_c"""
    x = np.asarray(x, np.float64)
    C = x.shape[-1]
    u = x * gate(a, x)
    src = x if variant == "max_of_x" else u
    mean = u.sum(-1) if variant == "no_inv_c" else u.sum(-1) / C
    arg = (C - 1 - np.argmax(src[..., ::-1], -1)) if variant == "last_tie" else np.argmax(src, -1)
    mx = np.take_along_axis(src, arg[..., None], -1)[..., 0]
    srt = np.sort(u, -1)
    return dict(mean=mean, mx=mx, arg=arg.astype(np.int32), mean_terms=np.abs(u).sum(-1) / C, mx_terms=np.abs(mx), gap=srt[..., -1] - srt[..., -2])


def _pad(p, r, variant=None):
    return np.pad(p, ((0, 0), (r, r), (r, r)), mode="edge" if variant == "edge_clamp" else "constant")


def conv_planes(mean, mx, w, variant=None):
    """pre[b, y, x] = sum_{plane, i, j} w[plane, i, j] m[plane][b, y + i - r, x + j - r] -> (pre, terms)"""
    w = np.asarray(w, np.float64).reshape(2, w.shape[-2], w.shape[-1])
    k = w.shape[-1]
    r = 3 if variant == "pad3_k3" else k // 2
    B, H, W = mean.shape
    planes = (mx, mean) if variant == "swap_planes" else (mean, mx)
    pre, terms = np.zeros((B, H, W)), np.zeros((B, H, W))
    for pl, m in enumerate(planes):
        mp = _pad(np.asarray(m, np.float64), r, variant)
        for i in range(k):
            for j in range(k):
                pre += w[pl, i, j] * mp[:, i:i + H, j:j + W]
                terms += abs(w[pl, i, j]) * np.abs(mp[:, i:i + H, j:j + W])
    return pre, terms


def spatial_gate(x, a, mean, mx, w, variant=None):
    """-> (y, s, y_terms): y = x g s from given planes"""
    pre, pt = conv_planes(mean, mx, w, variant)
    s = sigmoid(pre)
    u = np.asarray(x, np.float64) * gate(a, x)
    y = u * s[..., None]
    return y, s, np.abs(u) * (s + s * (1 - s) * pt)[..., None]


def forward(x, a, w, variant=None):
    st = stats(x, a, variant)
    y, s, yt = spatial_gate(x, a, st["mean"], st["mx"], w, variant)
    return dict(st, y=y, s=s, y_terms=yt)


# ------------------------------------------------------------------------------------------------ backward
def bwd_px(dy, x, a, s, variant=None):
    """dpre = s (1 - s) sum_c dy x g -> (dpre, terms)"""
    u = np.asarray(x, np.float64) * gate(a, x)
    dy = np.asarray(dy, np.float64)
    ds, t = (dy * u).sum(-1), np.abs(dy * u).sum(-1)
    k = np.ones_like(s) if variant == "no_dsigmoid" else s * (1 - s)
    return ds * k, t * k


def conv_bwd(dpre, mean, mx, w, variant=None):
    """-> (dmean, dmx, dw [1, 2, k, k], dmean_terms, dmx_terms, dw_terms): the transposed convolution of dpre (flipped taps, zero
    padding) and dw[plane, i, j] = sum_{b, q} dpre[q] m[plane][q + (i - r, j - r)]"""
    w = np.asarray(w, np.float64).reshape(2, w.shape[-2], w.shape[-1])
    k = w.shape[-1]
    r = 3 if variant == "pad3_k3" else k // 2
    B, H, W = dpre.shape
    dpp = _pad(np.asarray(dpre, np.float64), r)
    planes = (mx, mean) if variant == "swap_planes" else (mean, mx)
    dm, dmt = np.zeros((2, B, H, W)), np.zeros((2, B, H, W))
    dw, dwt = np.zeros((2, k, k)), np.zeros((2, k, k))
    for pl, m in enumerate(planes):
        mp = _pad(np.asarray(m, np.float64), r, variant)
        for i in range(k):
            for j in range(k):
                oi, oj = (i, j) if variant == "unflipped" else (2 * r - i, 2 * r - j)
                d = dpp[:, oi:oi + H, oj:oj + W]
                dm[pl] += w[pl, i, j] * d
                dmt[pl] += abs(w[pl, i, j]) * np.abs(d)
                dw[pl, i, j] = (dpre * mp[:, i:i + H, j:j + W]).sum()
                dwt[pl, i, j] = np.abs(dpre * mp[:, i:i + H, j:j + W]).sum()
    if variant == "swap_planes":
        dm, dmt = dm[::-1], dmt[::-1]
    return dm[0], dm[1], dw.reshape(1, 2, k, k), dmt[0], dmt[1], dwt.reshape(1, 2, k, k)


def du_of(dy, planes, variant=None):
    """du = dy s + dmean / C + (c == arg ? dmx : 0) -> (du, terms); planes = dict(s, dmean, dmx, arg) or None (du = dy)"""
    dy = np.asarray(dy, np.float64)
    if planes is None:
        return dy, np.abs(dy)
    C = dy.shape[-1]
    dmean_c = planes["dmean"] if variant == "no_inv_c" else planes["dmean"] / C
    hot = np.arange(C).reshape(1, 1, 1, C) == planes["arg"][..., None]
    parts = (dy * planes["s"][..., None], np.broadcast_to(dmean_c[..., None], dy.shape), hot * planes["dmx"][..., None])
    return sum(parts), sum(np.abs(p) for p in parts)


def gate_reduce(dy, x, a, planes=None, variant=None):
    """da [B, C] = g (1 - g) sum_p du x -> (da, terms)"""
    du, dut = du_of(dy, planes, variant)
    x = np.asarray(x, np.float64)
    k = sigmoid(a) * sigmoid(-np.asarray(a, np.float64))       # g (1 - g) without the cancellation at saturated logits
    return k * (du * x).sum((1, 2)), k * (dut * np.abs(x)).sum((1, 2))


def gate_apply(dy, a, planes=None, dpool=None, prior=None, variant=None):
    """dx = du g + dpool / (H W) (+ prior) -> (dx, terms)"""
    du, dut = du_of(dy, planes, variant)
    g = gate(a, dy)
    dx, t = du * g, dut * g
    if dpool is not None:
        B, H, W, C = dy.shape
        dx = dx + np.asarray(dpool, np.float64).reshape(B, 1, 1, C) / (H * W)
        t = t + np.abs(np.asarray(dpool, np.float64)).reshape(B, 1, 1, C) / (H * W)
    if prior is not None:
        dx, t = dx + prior, t + np.abs(prior)
    return dx, t


# ------------------------------------------------------------------------------------------------ whole blocks (NHWC in, NHWC out)
def block(kind, x, dy, fc_w=None, fc_b=None, cv_w=None, variant=None):
    """Forward and backward of ChannelAttention ('ca'), SpatialAttention ('sa') or CBAM ('cbam') -> dict(y, dx, fc_w, fc_b, cv_w
    gradients, gap): fc_w [C, C] (or [C, C, 1, 1]), fc_b [C], cv_w [1, 2, k, k]"""
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    out = {}
    a = pooled = None
    if kind != "sa":
        fw = np.asarray(fc_w, np.float64).reshape(C, C)
        pooled = x.mean((1, 2))
        a = pooled @ fw.T + np.asarray(fc_b, np.float64)
    if kind == "ca":
        out["y"], planes = chan_gate(x, a)[0], None
    else:
        f = forward(x, a, cv_w, variant)
        out.update(y=f["y"], gap=f["gap"], u_max=np.abs(x * gate(a, x)).max())
        if dy is None:
            return out
        dpre, _ = bwd_px(dy, x, a, f["s"], variant)
        dmean, dmx, dw = conv_bwd(dpre, f["mean"], f["mx"], cv_w, variant)[:3]
        out["cv_w"] = dw
        planes = dict(s=f["s"], dmean=dmean, dmx=dmx, arg=f["arg"])
    if dy is None:
        return out
    dp = None
    if kind != "sa":
        da = gate_reduce(dy, x, a, planes, variant)[0]
        out["fc_w"], out["fc_b"] = (da.T @ pooled).reshape(C, C, 1, 1), da.sum(0)
        dp = da @ fw
    out["dx"] = gate_apply(dy, a, planes, dp, None, variant)[0]
    return out
