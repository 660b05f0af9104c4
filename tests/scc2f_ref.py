"""float64 statements of the SCConv C2f family, shared by tests/test_scc2f_cpu.py and tests/test_gpu_scc2f.py; nothing here needs a GPU.

The CRU convolutions (csrc/cru.hip) as plain torch: one "CRU conv" is
    conv2d(x, w3, bias, pad 1, groups G) + conv2d(x, w1)            (w3 None: the plain 1x1)
and the CRU's buffer is cat(GWC(up') + PWC1(up'), PWC2(low'), low') with up' = squeeze1(y[:, :C/2]), low' = squeeze2(y[:, C/2:]).
SRU and the CRU tail are scconv_ref's statements ([N, HW, C] layout); Conv is ghost_ref's.  The blocks are functions of a state_dict
(name -> tensor) and a key prefix, differentiable through torch.autograd:

    SCConv(c)                    cru_fuse(cru_buffer(sru(x)))
    SCConvBottleneck(c, c)       Conv1x1(SCConv(x)) [+ x]           SC_PW_Bottleneck: conv2d 1x1 with bias, no BatchNorm
    SC_Conv3_Bottleneck(c, c)    Conv3x3(SCConv(x)) [+ x]           Conv3_SC_Bottleneck: SCConv(Conv3x3(x)) [+ x]
    <X>C2f(c1, c2, n)            cv2(cat(a, b, m1(b), m2(m1(b)), ...)),  a, b = chunk(cv1(x)),  m = n x the variant's bottleneck

Error terms of a CRU conv: `*_terms` give, per output element, the sum of |products| of the sum that forms it (the denominator of
scconv_ref.sum_err); K is 9 C3 + C1 (+ bias) forward, 9 N + G N for the data gradient, the pixel count for the weight gradients.
"""
import torch
import torch.nn.functional as F

import ghost_ref
import scconv_ref as sr

F64 = torch.float64
GROUP_NUM, GN_EPS = 4, 1e-10              # SCConv's SRU: GroupBatchnorm2d(c, group_num=4), eps 1e-10

BOTTLENECKS = ("SCConvBottleneck", "SC_PW_Bottleneck", "SC_Conv3_Bottleneck", "Conv3_SC_Bottleneck")
C2FS = {"SCC2f": "SCConvBottleneck", "SC_PW_C2f": "SC_PW_Bottleneck", "SC_Conv3_C2f": "SC_Conv3_Bottleneck", "Conv3_SC_C2f": "Conv3_SC_Bottleneck"}
WIDTHS = (16, 48, 64)


def block_args(cls, c, shortcut):
    """the fixtures' constructor arguments (tests/golden/make_scc2f_golden.py): a bottleneck c -> c, a C2f 2c -> 2c with one block"""
    return (c, c, shortcut) if cls in BOTTLENECKS else (2 * c, 2 * c, 1, shortcut)


def block_name(cls, c, shortcut):
    return f"g28_scc2f_{cls}_c{c}_{'sc' if shortcut else 'nosc'}"


BLOCK_CASES = [(cls, c, sc) for cls in BOTTLENECKS + tuple(C2FS) for c in WIDTHS for sc in (True, False)]


# ------------------------------------------------------------------------------------------------------------ CRU convolutions
def cru_conv_ref(x, w3, bias, w1, G):
    """x [B, C1, H, W]; w3 [G N, C1 / G, 3, 3] or None; bias [G N] or None; w1 [G N, C1, 1, 1]"""
    y = F.conv2d(x, w1)
    if w3 is not None:
        y = y + F.conv2d(x, w3, bias, 1, 1, 1, G)
    elif bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    return y


def cru_conv_fwd_terms(x, w3, bias, w1, G):
    return cru_conv_ref(x.abs(), None if w3 is None else w3.abs(), None if bias is None else bias.abs(), w1.abs(), G)


def cru_conv_dgrad_ref(dy, w3, w1, G, shape):
    """dx of cru_conv_ref for the upstream gradient dy (gather form of the transposed convolutions)"""
    dx = torch.nn.grad.conv2d_input(shape, w1, dy)
    if w3 is not None:
        dx = dx + torch.nn.grad.conv2d_input(shape, w3, dy, 1, 1, 1, G)
    return dx


def cru_conv_dgrad_terms(dy, w3, w1, G, shape):
    return cru_conv_dgrad_ref(dy.abs(), None if w3 is None else w3.abs(), w1.abs(), G, shape)


def cru_conv_wgrad_ref(x, dy, w3_shape, w1_shape, G):
    """(dw3 or None, dbias, dw1)"""
    dw1 = torch.nn.grad.conv2d_weight(x, w1_shape, dy)
    dw3 = None if w3_shape is None else torch.nn.grad.conv2d_weight(x, w3_shape, dy, 1, 1, 1, G)
    return dw3, dy.sum((0, 2, 3)), dw1


def cru_conv_wgrad_terms(x, dy, w3_shape, w1_shape, G):
    return cru_conv_wgrad_ref(x.abs(), dy.abs(), w3_shape, w1_shape, G)


def cru_buffer(sd, p, y):
    """y [B, C, H, W] (the SRU's output) -> cat(Y1 [C], PWC2(low') [3C/4], low' [C/4]); `p` = the CRU's key prefix"""
    h = y.shape[1] // 2
    up = cru_conv_ref(y[:, :h], None, None, sd[p + "squeeze1.weight"], 1)
    low = cru_conv_ref(y[:, h:], None, None, sd[p + "squeeze2.weight"], 1)
    y1 = cru_conv_ref(up, sd[p + "GWC.weight"], sd[p + "GWC.bias"], sd[p + "PWC1.weight"], 2)
    return torch.cat([y1, cru_conv_ref(low, None, None, sd[p + "PWC2.weight"], 1), low], 1)


# ------------------------------------------------------------------------------------------------------------------ modules
def _rows(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B, H * W, C)


def _maps(r, H, W):
    B, _, C = r.shape
    return r.reshape(B, H, W, C).permute(0, 3, 1, 2)


def scconv(sd, p, x):
    """`p`SRU.gn.{weight, bias}, `p`CRU.*; returns (output, gn, t) with gn / t of the SRU input ([B, HW, C]: scconv_ref's layout)"""
    B, C, H, W = x.shape
    y, gn, t = sr.sru_ref(_rows(x), sd[p + "SRU.gn.weight"].reshape(C), sd[p + "SRU.gn.bias"].reshape(C), GROUP_NUM, GN_EPS, x.dtype)
    buf = cru_buffer(sd, p + "CRU.", _maps(y, H, W))
    res, _ = sr.cru_fuse_ref(_rows(buf), x.dtype)
    return _maps(res, H, W), gn, t


def bottleneck(cls, sd, p, x, add, train=True, gates=None):
    q = p + "SandCRblock."
    if cls == "Conv3_SC_Bottleneck":
        y, gn, t = scconv(sd, q + "1.", ghost_ref.conv_bn_act(sd, q + "0.", x, 1, True, train))
    else:
        s, gn, t = scconv(sd, q + "0.", x)
        if cls == "SC_PW_Bottleneck":
            y = F.conv2d(s, sd[q + "1.weight"], sd[q + "1.bias"])
        else:
            y = ghost_ref.conv_bn_act(sd, q + "1.", s, 1, True, train)
    if gates is not None:
        gates.append((gn.detach(), t.detach()))
    return x + y if add else y


def c2f(cls, sd, p, x, n, shortcut, train=True, gates=None):
    ys = list(ghost_ref.conv_bn_act(sd, p + "cv1.", x, 1, True, train).chunk(2, 1))
    for i in range(n):
        ys.append(bottleneck(C2FS[cls], sd, f"{p}m.{i}.", ys[-1], shortcut, train, gates))
    return ghost_ref.conv_bn_act(sd, p + "cv2.", torch.cat(ys, 1), 1, True, train)


def block(cls, args, sd, x, train=True, gates=None):
    """the statement of getattr(modules, cls)(*args) on x"""
    if cls in BOTTLENECKS:
        return bottleneck(cls, sd, "", x, bool(args[2]) and args[0] == args[1], train, gates)
    return c2f(cls, sd, "", x, args[2], bool(args[3]), train, gates)
