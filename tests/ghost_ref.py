"""The five Ghost modules (Conv / DWConv, GhostConv, GhostBottleneck, C3, C3Ghost) stated in plain torch, float64 on the CPU, from their
formulas: functions of a state_dict (name -> tensor) and a key prefix, differentiable through torch.autograd.  The CPU test checks that
the fixtures captured from the reference (tests/golden/make_ghost_golden.py) agree with these statements; the GPU tests use them as
truth where no fixture applies.

    Conv(c1, c2, k, s, g)      act(BN(conv2d(x, W, stride s, pad k // 2, groups g)))          BN: eps 1e-3, batch or running statistics
    GhostConv(c1, c2, k, s)    y = Conv(c1, c2 / 2, k, s)(x);  cat(y, Conv(c2 / 2, c2 / 2, 5, 1, g = c2 / 2)(y))
    GhostBottleneck(c1, c2, k, s)   s = 1: G2(G1(x)) + x          s = 2: G2(DW(G1(x))) + Conv1x1(DW'(x))    (G2, DW, DW', Conv1x1 linear)
    C3(c1, c2, n)              cv3(cat(m(cv1(x)), cv2(x))),  m = n x Bottleneck: t + cv2_3x3(cv1_1x1(t))
    C3Ghost(c1, c2, n)         the same with m = n x GhostBottleneck(c_, c_)
"""
import torch
import torch.nn.functional as F

EPS = 1e-3


def conv_bn_act(sd, p, x, stride=1, act=True, train=True):
    """`p`conv.weight [c2, c1 / g, k, k] (g read off the shape), `p`bn.*; returns act(BN(conv(x)))"""
    w = sd[p + "conv.weight"]
    k = w.shape[2]
    groups = x.shape[1] // w.shape[1]
    z = F.conv2d(x, w, None, stride, k // 2, 1, groups)
    if train:
        mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
    else:
        mean, var = sd[p + "bn.running_mean"], sd[p + "bn.running_var"]
    u = (z - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + EPS) * sd[p + "bn.weight"].view(1, -1, 1, 1) + sd[p + "bn.bias"].view(1, -1, 1, 1)
    return u * torch.sigmoid(u) if act else u


def running_stats(sd, p, x, stride=1, momentum=0.03):
    """(running_mean, running_var) of `p`bn after one training forward of conv_bn_act on x (unbiased variance into the buffer)"""
    w = sd[p + "conv.weight"]
    z = F.conv2d(x, w, None, stride, w.shape[2] // 2, 1, x.shape[1] // w.shape[1])
    return ((1 - momentum) * sd[p + "bn.running_mean"] + momentum * z.mean((0, 2, 3)),
            (1 - momentum) * sd[p + "bn.running_var"] + momentum * z.var((0, 2, 3), unbiased=True))


def ghost_conv(sd, p, x, stride=1, act=True, train=True):
    y = conv_bn_act(sd, p + "cv1.", x, stride, act, train)
    return torch.cat([y, conv_bn_act(sd, p + "cv2.", y, 1, act, train)], 1)


def ghost_bottleneck(sd, p, x, stride=1, train=True):
    t = ghost_conv(sd, p + "conv.0.", x, 1, True, train)
    if stride == 2:
        t = conv_bn_act(sd, p + "conv.1.", t, 2, False, train)
    t = ghost_conv(sd, p + "conv.2.", t, 1, False, train)
    if stride == 1:
        return t + x
    return t + conv_bn_act(sd, p + "shortcut.1.", conv_bn_act(sd, p + "shortcut.0.", x, 2, False, train), 1, False, train)


def bottleneck(sd, p, x, train=True):
    return x + conv_bn_act(sd, p + "cv2.", conv_bn_act(sd, p + "cv1.", x, 1, True, train), 1, True, train)


def c3(sd, p, x, n, ghost=False, train=True):
    t = conv_bn_act(sd, p + "cv1.", x, 1, True, train)
    for i in range(n):
        t = ghost_bottleneck(sd, f"{p}m.{i}.", t, 1, train) if ghost else bottleneck(sd, f"{p}m.{i}.", t, train)
    return conv_bn_act(sd, p + "cv3.", torch.cat([t, conv_bn_act(sd, p + "cv2.", x, 1, True, train)], 1), 1, True, train)


# the blocks of tests/golden/make_ghost_golden.py: fixture -> (class, constructor arguments, statement)
BLOCKS = {
    "ghostconv_16_32": ("GhostConv", (16, 32, 1, 1), lambda sd, x, tr=True: ghost_conv(sd, "", x, 1, True, tr)),
    "ghostconv_s2_h12": ("GhostConv", (16, 24, 3, 2), lambda sd, x, tr=True: ghost_conv(sd, "", x, 2, True, tr)),
    "ghostconv_h4_noact": ("GhostConv", (8, 8, 1, 1, 1, False), lambda sd, x, tr=True: ghost_conv(sd, "", x, 1, False, tr)),
    "dwconv_12_s2": ("DWConv", (12, 12, 3, 2, 1, False), lambda sd, x, tr=True: conv_bn_act(sd, "", x, 2, False, tr)),
    "gbottleneck_16": ("GhostBottleneck", (16, 16), lambda sd, x, tr=True: ghost_bottleneck(sd, "", x, 1, tr)),
    "gbottleneck_s2": ("GhostBottleneck", (16, 32, 3, 2), lambda sd, x, tr=True: ghost_bottleneck(sd, "", x, 2, tr)),
    "c3_32": ("C3", (32, 32, 2), lambda sd, x, tr=True: c3(sd, "", x, 2, False, tr)),
    "c3ghost_32": ("C3Ghost", (32, 32, 2), lambda sd, x, tr=True: c3(sd, "", x, 2, True, tr)),
    "c3ghost_48_32": ("C3Ghost", (48, 32, 1), lambda sd, x, tr=True: c3(sd, "", x, 1, True, tr)),
}
