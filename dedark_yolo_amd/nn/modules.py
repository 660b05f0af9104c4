"""Module registry of the MI355X-native Dedark-YOLO path.

Same class names, constructor arguments, call signatures and state_dict key names as the reference modules (cited per
class), so `parse_model` / checkpoints / user scripts are drop-in.  Every module runs hand-written HIP kernels through
`ops` (C-ABI); nn.Conv2d / nn.BatchNorm2d / nn.Linear instances are used ONLY as parameter containers (their forward is
never called).  Each module implements `_fwd(tape, ...)` / `_bwd(tape, ...)`; a top-level call wraps the pair in one
autograd.Function so torch.autograd links modules while everything inside a module is explicit.
"""
import ctypes as C
import math
import os

import torch
import torch.nn as nn

from .. import ops
from .._C import ACT_LEAKY, ACT_NONE, ACT_SILU, call
from ..ops import as_nhwc, conv_backward, conv_forward, copy2d, empty_nhwc, ld_of, ptr, stream

__all__ = ("Conv", "DWConv", "GhostConv", "GhostBottleneck", "C3", "C3Ghost", "C3TR", "RepConv", "RepC3", "ChannelAttention", "SpatialAttention", "CBAM", "TransformerLayer", "TransformerBlock", "TransformerEncoderLayer", "AIFI", "Concat", "Bottleneck", "C2", "C2f", "PConv", "PconvBottleneck", "PconvBottleneck_n", "FasterC2f", "FasterC2f_N", "SPPF", "Upsample", "AsffTribeLevel", "AsffDoubLevel", "MFRU", "SCConv", "SCConvBottleneck", "SC_PW_Bottleneck", "SC_Conv3_Bottleneck", "Conv3_SC_Bottleneck", "SCC2f", "SC_PW_C2f",
           "SC_Conv3_C2f", "Conv3_SC_C2f", "RFBblock", "DFL", "Detect",
           "AsffDetect", "Proto", "Segment", "Pose", "Classify",
           "lowlight_recovery", "ExtractParameters2", "autopad")


def autopad(k, p=None, d=1):
    """Pad to 'same' (reference ultralytics/nn/modules/conv.py:15-21)."""
    if d > 1:
        k = d * (k - 1) + 1 if isinstance(k, int) else [d * (x - 1) + 1 for x in k]
    if p is None:
        p = k // 2 if isinstance(k, int) else [x // 2 for x in k]
    return p


class Tape:
    """LIFO of per-op contexts recorded by a module's _fwd and consumed in reverse by its _bwd."""

    def __init__(self):
        self.stack = []
        self.pgrads = {}

    def push(self, c):
        self.stack.append(c)

    def pop(self):
        return self.stack.pop()


class _ModuleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, n_in, out, *args):
        tape = Tape()
        outs = module._fwd(tape, *args[:n_in]) if out is None else module._fwd(tape, *args[:n_in], out=out)
        ctx.module, ctx.tape, ctx.n_in = module, tape, n_in
        ctx.multi = isinstance(outs, (list, tuple))
        if ctx.multi:
            ctx.out_meta = [(o.shape, o.dtype, o.device) for o in outs]
            return tuple(outs)
        ctx.out_meta = [(outs.shape, outs.dtype, outs.device)]
        return outs

    @staticmethod
    def backward(ctx, *gouts):
        gouts = [g if g is not None else torch.zeros(m[0], dtype=m[1], device=m[2]) for g, m in zip(gouts, ctx.out_meta)]
        module, tape = ctx.module, ctx.tape
        if getattr(module, "_planar_grad_ok", False) and all(g.is_contiguous() and g.dtype == m[1] for g, m in zip(gouts, ctx.out_meta)):
            pass             # the module's backward consumes planar [B,C,H,W] gradients as they are (front-end <- direct stem dgrad)
        else:
            gouts = [as_nhwc(g, m[1]) for g, m in zip(gouts, ctx.out_meta)]
        gins = module._bwd(tape, *gouts, needs=list(ctx.needs_input_grad[3:3 + ctx.n_in]))
        if not isinstance(gins, (list, tuple)):
            gins = (gins,)
        assert not tape.stack, f"{type(module).__name__}: unbalanced tape"
        cb = module.__dict__.get("_dy_after_backward")
        if cb is not None:
            cb()                 # data-parallel trainer: this layer's gradients are enqueued -> maybe launch its bucket
        pg = [tape.pgrads.get(p) for p in module._plist]
        return (None, None, None, *gins, *pg)


class DyModule(nn.Module):
    """Base: dispatches a call either through autograd (_ModuleFn) or straight to _fwd (no_grad / eval)."""
    in_dtype = None      # None -> compute dtype

    def _params(self):
        pl = self.__dict__.get("_plist")
        if pl is None:
            pl = [p for p in self.parameters() if p.requires_grad]
            self.__dict__["_plist"] = pl
        return pl

    def forward(self, x, *extra, out=None):
        """`out`: optional NHWC view the module's result is written into (GraphPlan: a producer's slice of a yaml-level Concat
        buffer); only modules whose _fwd takes `out` are called with it."""
        xs = list(x) if isinstance(x, (list, tuple)) else [x]
        xs = [self._adapt(t) for t in xs]
        pl = self._params()
        if torch.is_grad_enabled() and (any(t.requires_grad for t in xs) or any(p.requires_grad for p in pl)):
            return self._wrap(_ModuleFn.apply(self, len(xs), out, *xs, *pl))
        with torch.no_grad():
            return self._wrap(self._fwd(None, *xs) if out is None else self._fwd(None, *xs, out=out))

    def _adapt(self, t):
        return as_nhwc(t, self.in_dtype)

    def _wrap(self, out):
        return list(out) if isinstance(out, tuple) else out

    def train(self, mode=True):
        self.__dict__.pop("_plist", None)
        return super().train(mode)


def _act_code(act):
    if act is True or isinstance(act, nn.SiLU):
        return ACT_SILU
    if isinstance(act, nn.LeakyReLU):
        if abs(act.negative_slope - 0.1) > 1e-12:
            raise NotImplementedError("only LeakyReLU(0.1) is implemented in the HIP epilogue")
        return ACT_LEAKY
    if act is False or act is None or isinstance(act, nn.Identity):
        return ACT_NONE
    raise NotImplementedError(f"activation {act!r} has no HIP epilogue")


class Conv(DyModule):
    """Conv2d(bias=False) + BatchNorm2d + SiLU (reference ultralytics/nn/modules/conv.py:38-55).  g == 1 runs the MFMA convolutions;
    g == c1 == c2 (pure depthwise: odd k <= 7, stride 1 or 2, no dilation) runs the depthwise kernels (ops.dwconv_forward); every other
    grouping is refused."""
    default_act = nn.SiLU()
    _dw = False              # True on an instance: pure depthwise, runs ops.dwconv_forward / dwconv_backward

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, d=1, act=True):
        super().__init__()
        if g != 1:
            self._dw = True
        if self._dw and not (g == c1 == c2 and d == 1 and isinstance(k, int) and k % 2 == 1 and 3 <= k <= 7 and s in (1, 2) and p in (None, k // 2)):
            raise NotImplementedError("grouped convolution is outside the Dedark-YOLO hot path")
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p, d), groups=g, dilation=d, bias=False)
        self.bn = nn.BatchNorm2d(c2)
        self.act = self.default_act if act is True else act if isinstance(act, nn.Module) else nn.Identity()
        self._act = _act_code(self.act)

    def _fwd(self, tape, x, out=None, residual=None):
        c = self.conv
        if self._dw:
            if residual is not None:
                raise RuntimeError("Conv: the depthwise path takes no residual")
            return ops.dwconv_forward(tape, x, c.weight, None, self.bn, self._act, c.stride[0], self.training, out=out)
        return conv_forward(tape, x, c.weight, None, self.bn, self._act, c.stride[0], c.padding[0], c.dilation[0],
                            self.training, out=out, residual=residual)

    _takes_into = True       # GraphPlan.backward_train: `into[k]` = gradient another consumer of input k already left; add into it

    def _bwd(self, tape, dy, needs=(True,), dx_out=None, accumulate=False, add_src=None, into=None):
        bwd = ops.dwconv_backward if self._dw else conv_backward
        if into is not None and into[0] is not None:
            bwd(tape, dy, need_dx=True, dx_out=into[0], accumulate=True)
            return None
        return bwd(tape, dy, need_dx=needs[0], dx_out=dx_out, accumulate=accumulate, add_src=add_src)


class DWConv(Conv):
    """Depthwise Conv (reference conv.py:95-99): g = gcd(c1, c2); only the pure depthwise case c1 == c2 is implemented."""

    def __init__(self, c1, c2, k=1, s=1, d=1, act=True):
        g = math.gcd(c1, c2)
        if not (g == c1 == c2):
            raise NotImplementedError("grouped convolution is outside the Dedark-YOLO hot path")
        super().__init__(c1, c2, k, s, g=g, d=d, act=act)


class GhostConv(DyModule):
    """cat(y, cv2(y)), y = cv1(x), cv2 a 5x5 depthwise Conv over the c2 // 2 hidden channels (reference conv.py:142-154).  One
    buffer: cv1 writes its first half, the depthwise kernel reads that half and writes the second (exact channel bounds: the halves
    are live neighbours).  A half that is not made of whole 16-byte vectors (4 / 12 / 20 channels in a 16-bit dtype) cannot be the
    direct target of the MFMA conv or the BatchNorm pass: cv1 then runs into a temporary that ops.copy_exact moves over."""

    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        c_ = c2 // 2
        self.cv1 = Conv(c1, c_, k, s, None, g, act=act)
        self.cv2 = Conv(c_, c_, 5, 1, None, c_, act=act)
        self._c = c_

    def _fwd(self, tape, x, out=None, residual=None):
        """residual: optional view of the output's shape added to it (GhostBottleneck's identity shortcut).  The first half is the
        depthwise conv's input, which the tape keeps for the weight gradient: when a residual is going to be added on top of it
        (training), cv1 keeps its own buffer and the half is copied over."""
        c_ = self._c
        B, _, H, W = x.shape
        c = self.cv1.conv
        k, st, p = c.kernel_size[0], c.stride[0], c.padding[0]
        Ho, Wo = (H + 2 * p - k) // st + 1, (W + 2 * p - k) // st + 1
        Y = out if out is not None else ops._nhwc_like(B, 2 * c_, Ho, Wo, x.dtype, x.device)
        a, b = Y[:, :c_], Y[:, c_:]
        whole = ops.vec_ok(a)
        if whole and not (residual is not None and tape is not None):
            y1 = self.cv1._fwd(tape, x, out=a)
        else:
            y1 = self.cv1._fwd(tape, x)
            (copy2d if whole else ops.copy_exact)(y1, a)
        self.cv2._fwd(tape, y1, out=b)
        if residual is not None:
            (copy2d if ops.vec_ok(residual) and ops.vec_ok(Y) else ops.copy_exact)(residual, Y, accumulate=True)
            ops.emu_round(Y)
        return Y

    def _bwd(self, tape, dy, needs=(True,), dx_out=None, accumulate=False, add_src=None):
        """d cat(y, cv2(y)): the first half of dy joins cv2's data gradient as its add_src (one launch)."""
        c_ = self._c
        da, db = dy[:, :c_], dy[:, c_:]
        g = self.cv2._bwd(tape, db, add_src=da)
        return self.cv1._bwd(tape, g, needs=needs, dx_out=dx_out, accumulate=accumulate, add_src=add_src)


class GhostBottleneck(DyModule):
    """conv(x) + shortcut(x), conv = GhostConv -> [DWConv s2] -> GhostConv(act=False) (reference block.py:535-550).  s == 1: the
    identity shortcut is added into the last GhostConv's buffer by one dy_copy2d(accumulate) (GhostConv's `residual`) and its gradient
    rides on the first GhostConv's data gradient (add_src).  s == 2: the shortcut's 1x1 Conv adds conv(x) in its BatchNorm pass (residual) and the two
    input gradients meet in one buffer (dx_out, accumulate)."""

    def __init__(self, c1, c2, k=3, s=1):
        super().__init__()
        c_ = c2 // 2
        self.conv = nn.Sequential(GhostConv(c1, c_, 1, 1), DWConv(c_, c_, k, s, act=False) if s == 2 else nn.Identity(),
                                  GhostConv(c_, c2, 1, 1, act=False))
        self.shortcut = nn.Sequential(DWConv(c1, c1, k, s, act=False), Conv(c1, c2, 1, 1, act=False)) if s == 2 else nn.Identity()
        self._s2 = s == 2
        if not self._s2 and c1 != c2:
            raise ValueError("GhostBottleneck: the identity shortcut needs c1 == c2")

    def _fwd(self, tape, x, out=None):
        cv = self.conv
        t = cv[0]._fwd(tape, x)
        if not self._s2:
            return cv[2]._fwd(tape, t, out=out, residual=x)
        u = cv[2]._fwd(tape, cv[1]._fwd(tape, t))
        return self.shortcut[1]._fwd(tape, self.shortcut[0]._fwd(tape, x), out=out, residual=u)

    def _bwd(self, tape, dy, needs=(True,), dx_out=None, accumulate=False):
        cv = self.conv
        if not self._s2:
            dt = cv[2]._bwd(tape, dy)
            return cv[0]._bwd(tape, dt, needs=needs, dx_out=dx_out, accumulate=accumulate, add_src=dy)
        dx = self.shortcut[0]._bwd(tape, self.shortcut[1]._bwd(tape, dy), needs=needs, dx_out=dx_out, accumulate=accumulate)
        dt = cv[1]._bwd(tape, cv[2]._bwd(tape, dy))
        if not needs[0]:
            return cv[0]._bwd(tape, dt, needs=needs)
        return cv[0]._bwd(tape, dt, dx_out=dx, accumulate=True)


class AddConv(nn.Module):
    """Parameter container for add_conv (reference ultralytics/nn/modules/block.py:24-45): conv + batch_norm + LeakyReLU(0.1)."""

    def __init__(self, in_ch, out_ch, ksize, stride):
        super().__init__()
        self.conv = nn.Conv2d(in_ch, out_ch, ksize, stride, (ksize - 1) // 2, bias=False)
        self.batch_norm = nn.BatchNorm2d(out_ch)
        self.leaky = nn.LeakyReLU(0.1)

    def _fwd(self, tape, x, training, out=None):
        c = self.conv
        return conv_forward(tape, x, c.weight, None, self.batch_norm, ACT_LEAKY, c.stride[0], c.padding[0], 1, training, out=out)


def plain_conv_fwd(tape, m, x, act=ACT_NONE, out=None):
    """nn.Conv2d-with-bias container `m` run as a HIP conv (Detect 1x1 heads, ASFF weight_levels, RFB, extractor)."""
    return conv_forward(tape, x, m.weight, m.bias, None, act, m.stride[0], m.padding[0], m.dilation[0], False, out=out)


class Concat(DyModule):
    """torch.cat along channels (reference conv.py:462-473) as strided slab copies into one NHWC buffer."""

    def __init__(self, dimension=1):
        super().__init__()
        if dimension != 1:
            raise NotImplementedError("Concat: only channel concat is on the hot path")
        self.d = dimension

    @staticmethod
    def _in_place(xs, tot):
        """The inputs already ARE the channel slices, in order, of one [B, tot, H, W] NHWC buffer (GraphPlan placed their
        producers there): return that buffer as a view, else None."""
        t0 = xs[0]
        if ld_of(t0) != tot or t0.dim() != 4:
            return None
        es, base, o = t0.element_size(), t0.data_ptr(), 0
        for t in xs:
            if (t.dtype != t0.dtype or tuple(t.shape[2:]) != tuple(t0.shape[2:]) or t.shape[0] != t0.shape[0] or ld_of(t) != tot
                    or t.stride() != t0.stride() or t.data_ptr() != base + o * es
                    or t.untyped_storage().data_ptr() != t0.untyped_storage().data_ptr()):
                return None
            o += t.shape[1]
        return torch.as_strided(t0, (t0.shape[0], tot, t0.shape[2], t0.shape[3]), t0.stride(), t0.storage_offset())

    def _fwd(self, tape, *xs):
        B, _, H, W = xs[0].shape
        tot = sum(t.shape[1] for t in xs)
        whole = self._in_place(xs, tot)
        if whole is not None:
            if tape is not None:
                tape.push([t.shape[1] for t in xs])
            return whole
        out = empty_nhwc(B, tot, H, W, xs[0].dtype, xs[0].device)
        o = 0
        for t in xs:
            copy2d(t, out[:, o:o + t.shape[1]])
            o += t.shape[1]
        if tape is not None:
            tape.push([t.shape[1] for t in xs])
        return out

    def _bwd(self, tape, dy, needs=None):
        sizes = tape.pop()
        outs, o = [], 0
        for c in sizes:
            outs.append(dy[:, o:o + c])
            o += c
        return outs


class Upsample(DyModule):
    """nn.Upsample(size=None, scale_factor, 'nearest') of the yaml head (reference yolov8.yaml:32,36)."""

    def __init__(self, size=None, scale_factor=None, mode="nearest"):
        super().__init__()
        if size is not None or mode != "nearest" or int(scale_factor) != scale_factor:
            raise NotImplementedError("Upsample: integer nearest-neighbour scale only")
        self.scale_factor = int(scale_factor)
        self.mode = mode

    def _fwd(self, tape, x, out=None):
        return ops.upsample_fwd(x, self.scale_factor, out=out)

    _takes_into = True

    def _bwd(self, tape, dy, needs=None, into=None):
        if into is not None and into[0] is not None:
            ops.upsample_bwd(dy, self.scale_factor, dx_out=into[0], accumulate=True)
            return None
        return ops.upsample_bwd(dy, self.scale_factor)


class Bottleneck(DyModule):
    """x + cv2(cv1(x)) (reference ultralytics/nn/modules/block.py:553-565)."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, k[0], 1)
        self.cv2 = Conv(c_, c2, k[1], 1, g=g)
        self.add = shortcut and c1 == c2

    def _fwd(self, tape, x, out=None):
        t = self.cv1._fwd(tape, x)
        return self.cv2._fwd(tape, t, out=out, residual=x if self.add else None)

    def _bwd(self, tape, dy, needs=(True,), dx_out=None, accumulate=False):
        dt = self.cv2._bwd(tape, dy)
        # shortcut: dx = d cv1 + dy, added inside cv1's data gradient (dy_conv_desc.add_src) instead of by a copy pass
        return self.cv1._bwd(tape, dt, dx_out=dx_out, accumulate=accumulate, add_src=dy if self.add else None)


class C2(DyModule):
    """CSP bottleneck with two convolutions (reference block.py:355-370): a, b = chunk(cv1(x)); cv2(cat(m(a), b)), m a chain of
    n Bottlenecks.  cv1 writes [a | b] into one buffer and the last Bottleneck writes m(a) straight into the first half of
    cv2's input buffer; the reference order (m(a), b) is not a slice of cv1's output, so b is copied next to m(a) (one
    c-channel dy_copy2d forward, one for its gradient backward)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c2, 1)
        self.m = nn.Sequential(*(Bottleneck(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n)))

    def _fwd(self, tape, x, out=None):
        c, n = self.c, len(self.m)
        B, _, H, W = x.shape
        Y = empty_nhwc(B, 2 * c, H, W, x.dtype, x.device)              # cv1: [a | b]
        Z = empty_nhwc(B, 2 * c, H, W, x.dtype, x.device)              # cv2's input: [m(a) | b]
        self.cv1._fwd(tape, x, out=Y)
        t = Y[:, :c]
        for i, m in enumerate(self.m):
            t = m._fwd(tape, t, out=Z[:, :c] if i == n - 1 else None)
        copy2d(Y[:, c:], Z[:, c:])
        return self.cv2._fwd(tape, Z, out=out)

    def _bwd(self, tape, dy, needs=(True,)):
        c, n = self.c, len(self.m)
        dZ = self.cv2._bwd(tape, dy)                                   # [d m(a) | d b]
        B, _, H, W = dZ.shape
        dY = empty_nhwc(B, 2 * c, H, W, dZ.dtype, dZ.device)
        copy2d(dZ[:, c:], dY[:, c:])
        g = dZ[:, :c]
        for i in reversed(range(n)):
            g = self.m[i]._bwd(tape, g, dx_out=dY[:, :c] if i == 0 else None)
        return self.cv1._bwd(tape, dY, needs=needs)


class C2f(DyModule):
    """CSP block (reference block.py:373-393).  chunk / cat are free: cv1 and every Bottleneck write straight into
    channel slices of ONE NHWC buffer that cv2 then reads; backward mirrors it with one gradient buffer."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(Bottleneck(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n))

    def _fwd(self, tape, x, out=None):
        c, n = self.c, len(self.m)
        B, _, H, W = x.shape
        Y = empty_nhwc(B, (2 + n) * c, H, W, x.dtype, x.device)
        self.cv1._fwd(tape, x, out=Y[:, :2 * c])
        for i, m in enumerate(self.m):
            m._fwd(tape, Y[:, (1 + i) * c:(2 + i) * c], out=Y[:, (2 + i) * c:(3 + i) * c])
        return self.cv2._fwd(tape, Y, out=out)

    def _bwd(self, tape, dy, needs=(True,)):
        c, n = self.c, len(self.m)
        dY = self.cv2._bwd(tape, dy)
        for i in reversed(range(n)):
            self.m[i]._bwd(tape, dY[:, (2 + i) * c:(3 + i) * c], dx_out=dY[:, (1 + i) * c:(2 + i) * c], accumulate=True)
        return self.cv1._bwd(tape, dY[:, :2 * c], needs=needs)


class C3(DyModule):
    """CSP bottleneck with three convolutions (reference block.py:473-486): cv3(cat(m(cv1(x)), cv2(x))).  cv2 and the last block of
    m write the two halves of cv3's input buffer; backward: both input gradients meet in one buffer (cv2 adds into cv1's)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, k=((1, 1), (3, 3)), e=1.0) for _ in range(n)))
        self._c = c_
        if c_ % 8:
            raise NotImplementedError("C3: a hidden width that is not a multiple of 8 is outside the Dedark-YOLO hot path")

    def _fwd(self, tape, x, out=None):
        c_, n = self._c, len(self.m)
        B, _, H, W = x.shape
        Z = empty_nhwc(B, 2 * c_, H, W, x.dtype, x.device)             # cv3's input: [m(cv1(x)) | cv2(x)]
        self.cv2._fwd(tape, x, out=Z[:, c_:])
        t = self.cv1._fwd(tape, x, out=Z[:, :c_] if n == 0 else None)
        for i, m in enumerate(self.m):
            t = m._fwd(tape, t, out=Z[:, :c_] if i == n - 1 else None)
        return self.cv3._fwd(tape, Z, out=out)

    def _bwd(self, tape, dy, needs=(True,)):
        c_, n = self._c, len(self.m)
        dZ = self.cv3._bwd(tape, dy)
        g = dZ[:, :c_]
        for i in reversed(range(n)):
            g = self.m[i]._bwd(tape, g)
        dx = self.cv1._bwd(tape, g, needs=needs)
        if not needs[0]:
            return self.cv2._bwd(tape, dZ[:, c_:], needs=needs)
        return self.cv2._bwd(tape, dZ[:, c_:], dx_out=dx, accumulate=True)


class C3Ghost(C3):
    """C3 with GhostBottleneck blocks (reference block.py:525-532)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.Sequential(*(GhostBottleneck(self._c, self._c) for _ in range(n)))


class RepConv(DyModule):
    """act(conv1(x) + conv2(x)), conv1 = Conv 3x3 + BatchNorm, conv2 = Conv 1x1 + BatchNorm, both without activation (reference
    ultralytics/nn/modules/conv.py:193-291).  Training and unfused eval run the two raw convolutions and ONE two-branch
    BatchNorm + activation kernel (ops.repconv_forward); after fuse_convs() the block is one 3x3 convolution with a bias and the
    activation in its epilogue.  The BatchNorm identity branch (bn=True), stride, groups, dilation and c1 != c2 are refused."""
    default_act = nn.SiLU()

    def __init__(self, c1, c2, k=3, s=1, p=1, g=1, d=1, act=True, bn=False, deploy=False):
        super().__init__()
        assert k == 3 and p == 1
        for name, val, only in (("s", s, 1), ("g", g, 1), ("d", d, 1), ("bn", bool(bn), False)):
            if val != only:
                raise NotImplementedError(f"RepConv: {name}={val!r} is outside the Dedark-YOLO hot path (only {name}={only!r} is implemented)")
        if c1 != c2:
            raise NotImplementedError(f"RepConv: c1={c1} != c2={c2} is outside the Dedark-YOLO hot path")
        self.g, self.c1, self.c2 = g, c1, c2
        self.act = self.default_act if act is True else act if isinstance(act, nn.Module) else nn.Identity()
        self._act = _act_code(self.act)
        self.bn = None
        self.conv1 = Conv(c1, c2, k, s, p=p, g=g, act=False)
        self.conv2 = Conv(c1, c2, 1, s, p=(p - k // 2), g=g, act=False)

    def _fwd(self, tape, x, out=None):
        if "conv" in self._modules:          # fused (fuse_convs): one 3x3 conv, bias and activation in the epilogue
            c = self.conv
            return conv_forward(tape, x, c.weight, c.bias, None, self._act, 1, 1, 1, False, out=out)
        return ops.repconv_forward(tape, x, self.conv1, self.conv2, self._act, self.training, out=out)

    def _bwd(self, tape, dy, needs=(True,), dx_out=None, accumulate=False, add_src=None):
        bwd = conv_backward if "conv" in self._modules else ops.repconv_backward
        return bwd(tape, dy, need_dx=needs[0], dx_out=dx_out, accumulate=accumulate, add_src=add_src)

    def _fuse_bn_tensor(self, branch):
        """conv.py:241-266 for a Conv branch, in f32: (W gamma / std, beta - running_mean gamma / std)"""
        w, bn = branch.conv.weight.detach().float(), branch.bn
        std = (bn.running_var.detach().float() + bn.eps).sqrt()
        gamma, beta, mean = bn.weight.detach().float(), bn.bias.detach().float(), bn.running_mean.detach().float()
        return w * (gamma / std).reshape(-1, 1, 1, 1), beta - mean * gamma / std

    def get_equivalent_kernel_bias(self):
        """conv.py:220-224: the 3x3 kernel and bias of the one convolution that equals both eval-mode branches"""
        k3, b3 = self._fuse_bn_tensor(self.conv1)
        k1, b1 = self._fuse_bn_tensor(self.conv2)
        return k3 + torch.nn.functional.pad(k1, [1, 1, 1, 1]), b3 + b1

    def fuse_convs(self):
        """conv.py:268-291: replace conv1 / conv2 by `conv`, an nn.Conv2d(c, c, 3, 1, 1, bias=True) holding the equivalent kernel"""
        if "conv" in self._modules:
            return
        kernel, bias = self.get_equivalent_kernel_bias()
        c = self.conv1.conv
        self.conv = nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, c.dilation, c.groups, bias=True).requires_grad_(False)
        self.conv.weight.data = kernel
        self.conv.bias.data = bias
        for para in self.parameters():
            para.detach_()
        del self.conv1, self.conv2
        self.__dict__.pop("bn", None)
        self.__dict__.pop("_plist", None)
        ops.bump_weights_epoch()


class RepC3(DyModule):
    """cv3(m(cv1(x)) + cv2(x)), m a chain of n RepConv (reference block.py:499-512), the RT-DETR neck block.  Only e == 1.0
    works in the reference (its cv1 already has c2 channels while m expects int(c2 * e)), and then cv3 is nn.Identity.  The add is
    free: cv2's BatchNorm pass takes m(cv1(x)) as its residual; backward: both input gradients meet in one buffer (cv1 adds
    into cv2's)."""

    def __init__(self, c1, c2, n=3, e=1.0):
        super().__init__()
        c_ = int(c2 * e)
        if c_ != c2:
            raise NotImplementedError(f"RepC3: e={e} gives a hidden width {c_} != c2={c2}; the reference's cv1 feeds c2 channels into "
                                      f"RepConv({c_}, {c_}) and fails there, so only e == 1.0 exists")
        if c2 % 8:
            raise NotImplementedError("RepC3: a width that is not a multiple of 8 is outside the Dedark-YOLO hot path")
        self.cv1 = Conv(c1, c2, 1, 1)
        self.cv2 = Conv(c1, c2, 1, 1)
        self.m = nn.Sequential(*[RepConv(c_, c_) for _ in range(n)])
        self.cv3 = Conv(c_, c2, 1, 1) if c_ != c2 else nn.Identity()

    def _fwd(self, tape, x, out=None):
        t = self.cv1._fwd(tape, x)
        for m in self.m:
            t = m._fwd(tape, t)
        return self.cv2._fwd(tape, x, out=out, residual=t)

    def _bwd(self, tape, dy, needs=(True,)):
        dx = self.cv2._bwd(tape, dy, needs=needs)          # the residual's gradient is dy itself
        g = dy
        for m in reversed(self.m):
            g = m._bwd(tape, g)
        if not needs[0]:
            return self.cv1._bwd(tape, g, needs=needs)
        return self.cv1._bwd(tape, g, dx_out=dx, accumulate=True)


def _check_attn_channels(who, c):
    if c % 8 or not 8 <= c <= ops._C.CBAM_MAX_C:
        raise NotImplementedError(f"{who}: C={c} is outside the attention kernels' rule C % 8 == 0, 8 <= C <= {ops._C.CBAM_MAX_C}")


def _spatial_fwd(tape, weight, x, a, out):
    """y = u s, u = x sigmoid(a) (a None: u = x), s = sigmoid(cv1(mean_c u, max_c u)): one read of x for the planes, one read and one
    write for the scale; u is never stored.  With a tape the planes (and the argmax channel) stay for the backward."""
    train = tape is not None
    planes = ops.spatial_stats_fwd(x, a, want_arg=train)
    y = ops.spatial_gate_fwd(x, a, planes, weight, out=out, keep_s=train)
    if train:
        tape.push((x, a, planes, weight))
    return y


def _spatial_bwd(tape, dy):
    """the plane half of the backward: pops _spatial_fwd's context, files cv1's weight gradient; -> (x, a, planes with dmean / dmx)"""
    x, a, planes, weight = tape.pop()
    dpre = ops.spatial_gate_bwd_px(dy, x, a, planes)
    ops.spatial_conv_bwd(tape, dpre, planes, weight)
    return x, a, planes


def _chan_bwd(tape, dy, x, a, planes, needs, dx_out, accumulate):
    """the channel half: da from one reduce pass, the fc's backward (its context is next on the tape), then ONE apply pass that
    writes dx with the pooled branch's share dp / (H W) already in it"""
    da = ops.gate_bwd_reduce(dy, x, a, planes)
    dp = conv_backward(tape, da, need_dx=needs[0])
    if not needs[0]:
        return None
    return ops.gate_bwd_apply(dy, a, planes, dp, dx_out=dx_out, accumulate=accumulate)


class ChannelAttention(DyModule):
    """x * sigmoid(fc(avgpool(x))), fc = Conv2d(C, C, 1, bias=True) (reference ultralytics/nn/modules/conv.py:294-304).  The pool is
    dy_chan_pool_fwd, the fc a 1x1 conv with bias on the pooled [B, C, 1, 1] map (as Classify's Linear), the scale dy_chan_gate_fwd.
    `pool` and `act` are containers only (the checkpoint writer names them)."""

    def __init__(self, channels: int) -> None:
        super().__init__()
        _check_attn_channels(type(self).__name__, channels)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Conv2d(channels, channels, 1, 1, 0, bias=True)
        self.act = nn.Sigmoid()

    def _logits(self, tape, x):
        return plain_conv_fwd(tape, self.fc, ops.chan_pool_fwd(x))

    def _fwd(self, tape, x, out=None):
        a = self._logits(tape, x)
        y = ops.chan_gate_fwd(x, a, out=out)
        if tape is not None:
            tape.push((x, a))
        return y

    def _bwd(self, tape, dy, needs=(True,), dx_out=None, accumulate=False):
        x, a = tape.pop()
        return _chan_bwd(tape, dy, x, a, None, needs, dx_out, accumulate)


class SpatialAttention(DyModule):
    """x * sigmoid(cv1(cat(mean_c x, max_c x))), cv1 = Conv2d(2, 1, k, padding=k // 2, bias=False), k in (3, 7) (reference
    conv.py:307-320): dy_spatial_stats_fwd + dy_spatial_gate_fwd, no cat and no stored planes beyond [B, H, W] f32 ones."""

    def __init__(self, kernel_size=7):
        super().__init__()
        assert kernel_size in (3, 7), 'kernel size must be 3 or 7'
        padding = 3 if kernel_size == 7 else 1
        self.cv1 = nn.Conv2d(2, 1, kernel_size, padding=padding, bias=False)
        self.act = nn.Sigmoid()

    def _fwd(self, tape, x, out=None):
        return _spatial_fwd(tape, self.cv1.weight, x, None, out)

    def _bwd(self, tape, dy, needs=(True,), dx_out=None, accumulate=False):
        _, _, planes = _spatial_bwd(tape, dy)
        if not needs[0]:
            return None
        return ops.gate_bwd_apply(dy, None, planes, None, dx_out=dx_out, accumulate=accumulate)


class CBAM(DyModule):
    """spatial_attention(channel_attention(x)) (reference conv.py:449-459) without the intermediate map: the channel gate is folded
    into both spatial kernels (forward 3 reads + 1 write of the map with the pool; backward 5 reads + 1 write)."""

    def __init__(self, c1, kernel_size=7):
        super().__init__()
        self.channel_attention = ChannelAttention(c1)
        self.spatial_attention = SpatialAttention(kernel_size)

    def _fwd(self, tape, x, out=None):
        a = self.channel_attention._logits(tape, x)
        return _spatial_fwd(tape, self.spatial_attention.cv1.weight, x, a, out)

    def _bwd(self, tape, dy, needs=(True,), dx_out=None, accumulate=False):
        x, a, planes = _spatial_bwd(tape, dy)
        return _chan_bwd(tape, dy, x, a, planes, needs, dx_out, accumulate)


_ParamRows = ops._ParamRows


def _linear(tape, x, weight, bias=None, out=None, residual=None, rows=None):
    """x W^T [+ bias] [+ residual] over the pixels of an NHWC map, which already is the token matrix [B, L = H W, C]: an nn.Linear
    weight [out, in] run as a 1x1 conv through its persistent view (ops.weight_view).  rows = (r0, r1): only those rows of the
    weight and of the bias, which then own their part of the gradients (ops._ParamRows)."""
    if rows is None:
        w, owner = ops.weight_view(weight, (*weight.shape, 1, 1)), weight
    else:
        w = ops.weight_view(weight, (rows[1] - rows[0], weight.shape[1], 1, 1), *rows)
        owner, bias = _ParamRows(weight, *rows), _ParamRows(bias, *rows)
    return conv_forward(tape, x, w, bias, None, ACT_NONE, 1, 0, 1, False, out=out, residual=residual, owner=owner)


class _AttnCore(DyModule):
    """What the two transformer layers share: nn.MultiheadAttention `self.ma` of `self._heads` heads over `self._c` channels, run
    as three in-projections with bias (rows of ONE in_proj_weight / in_proj_bias) writing Q | K | V into the slices of one buffer,
    ops.attn_forward and out_proj with bias."""

    def _check_heads(self, c, heads):
        if c % heads or (c // heads) % 8 or not 8 <= c // heads <= 128:
            raise NotImplementedError(f"{type(self).__name__}: head dim {c}/{heads} is outside the attention kernels' rule D % 8 == 0, 8 <= D <= 128")

    def _attn_fwd(self, tape, q, k, v, residual=None):
        """out_proj(attention(in0(q), in1(k), in2(v))) [+ residual]"""
        ma, C_ = self.ma, self._c
        B, _, H, W = q.shape
        qkv = empty_nhwc(B, 3 * C_, H, W, q.dtype, q.device)
        for i, t in enumerate((q, k, v)):
            _linear(tape, t, ma.in_proj_weight, ma.in_proj_bias, out=qkv[:, i * C_:(i + 1) * C_], rows=(i * C_, (i + 1) * C_))
        a = ops.attn_forward(tape, qkv[:, :C_], qkv[:, C_:2 * C_], qkv[:, 2 * C_:], self._heads)
        return _linear(tape, a, ma.out_proj.weight, ma.out_proj.bias, residual=residual)

    def _attn_bwd(self, tape, dy):
        """out_proj and the attention backwards; returns dQ | dK | dV, which the caller takes through the in-projections (last
        first) before _join_in_proj"""
        return ops.attn_backward(tape, conv_backward(tape, dy))

    def _join_in_proj(self, tape):
        """no direct placement: the three row blocks of each in-projection parameter -> the parameter's gradient"""
        ops.join_param_rows(tape, self.ma.in_proj_weight)
        ops.join_param_rows(tape, self.ma.in_proj_bias)


class TransformerLayer(_AttnCore):
    """x = ma(q(x), k(x), v(x)) + x; x = fc2(fc1(x)) + x over the pixels of an NHWC map (reference
    ultralytics/nn/modules/transformer.py:100-117; no LayerNorm).  nn.Linear / nn.MultiheadAttention hold the parameters under the
    reference's names; every Linear runs as a 1x1 conv (nine per layer: q / k / v, the attention core's four, fc1, fc2).  Both
    residuals are added by the conv's own dy_copy2d(accumulate) pass; in backward the fan-outs of x and of the attention output add
    through add_src / accumulate."""

    def __init__(self, c, num_heads):
        super().__init__()
        self._check_heads(c, num_heads)
        self.q = nn.Linear(c, c, bias=False)
        self.k = nn.Linear(c, c, bias=False)
        self.v = nn.Linear(c, c, bias=False)
        self.ma = nn.MultiheadAttention(embed_dim=c, num_heads=num_heads)
        self.fc1 = nn.Linear(c, c, bias=False)
        self.fc2 = nn.Linear(c, c, bias=False)
        self._c, self._heads = c, num_heads

    def _fwd(self, tape, x, out=None):
        if self.ma.dropout:
            raise NotImplementedError("TransformerLayer: attention dropout > 0 is not implemented")
        x1 = self._attn_fwd(tape, *(_linear(tape, x, m.weight) for m in (self.q, self.k, self.v)), residual=x)
        return _linear(tape, _linear(tape, x1, self.fc1.weight), self.fc2.weight, out=out, residual=x1)

    def _bwd(self, tape, dy, needs=(True,)):
        C_ = self._c
        dt = conv_backward(tape, dy)                                       # fc2
        dx1 = conv_backward(tape, dt, add_src=dy)                          # fc1; + the second residual
        g = self._attn_bwd(tape, dx1)
        dqkv = [conv_backward(tape, g[:, i * C_:(i + 1) * C_]) for i in (2, 1, 0)]      # the in-projections of V, K, Q
        dx = conv_backward(tape, dqkv[0], add_src=dx1)                     # v; + the first residual
        for dt in dqkv[1:]:
            conv_backward(tape, dt, dx_out=dx, accumulate=True)            # k, q: x feeds all three
        self._join_in_proj(tape)
        return dx


class TransformerBlock(DyModule):
    """Optional Conv, p + linear(p) (the learnable position embedding) and num_layers TransformerLayers (reference
    transformer.py:120-139).  The reference's flatten / permute to [L, B, C] and back are the identity on an NHWC map."""

    def __init__(self, c1, c2, num_heads, num_layers):
        super().__init__()
        self.conv = None
        if c1 != c2:
            self.conv = Conv(c1, c2)
        self.linear = nn.Linear(c2, c2)
        self.tr = nn.Sequential(*(TransformerLayer(c2, num_heads) for _ in range(num_layers)))
        self.c2 = c2

    # C3._fwd / _bwd walk `m` as a sequence of blocks: as C3TR's m this module is a sequence of one
    def __len__(self):
        return 1

    def __iter__(self):
        return iter((self,))

    def __getitem__(self, i):
        return (self,)[i]

    def _fwd(self, tape, x, out=None):
        if self.conv is not None:
            x = self.conv._fwd(tape, x)
        n = len(self.tr)
        x = _linear(tape, x, self.linear.weight, self.linear.bias, out=out if n == 0 else None, residual=x)
        for i, m in enumerate(self.tr):
            x = m._fwd(tape, x, out=out if i == n - 1 else None)
        return x

    def _bwd(self, tape, dy, needs=(True,)):
        for m in reversed(self.tr):
            dy = m._bwd(tape, dy)
        dx = conv_backward(tape, dy, add_src=dy)                           # p + linear(p)
        if self.conv is not None:
            return self.conv._bwd(tape, dx, needs=needs)
        return dx


class C3TR(C3):
    """C3 whose m is a TransformerBlock of n layers and 4 heads (reference block.py:515-522)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        c_ = int(c2 * e)
        if c_ % 32:
            raise NotImplementedError(f"C3TR: the hidden width int(c2 * e) = {c_} must be a multiple of 32 (4 heads of a head dim D % 8 == 0)")
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = TransformerBlock(c_, c_, 4, n)


class TransformerEncoderLayer(_AttnCore):
    """The post-norm encoder layer over the pixels of an NHWC map = the token matrix [B, L = H W, C] (reference
    ultralytics/nn/modules/transformer.py:20-67, forward_post):
        q = k = src + pos; src = norm1(src + ma(q, k, src)); src = norm2(src + fc2(gelu(fc1(src))))
    Real nn.MultiheadAttention / nn.Linear / nn.LayerNorm objects hold the parameters under the reference's names.  Six 1x1 convs
    with bias (the attention core's four, fc1, fc2), ops.add_pos, ops.gelu_forward and two ops.add_layernorm_forward: each
    residual add is fused into its LayerNorm, the position table is a constant.  Called on a map this class adds no position term
    (the reference's pos=None)."""

    def __init__(self, c1, cm=2048, num_heads=8, dropout=0.0, act=nn.GELU(), normalize_before=False):
        super().__init__()
        self._check(normalize_before, dropout, act)
        self._check_heads(c1, num_heads)
        if cm % 4 or not 4 <= c1 <= 2048:
            raise NotImplementedError(f"{type(self).__name__}: c1 = {c1} must be at most 2048 (the LayerNorm kernels) and cm = {cm} a multiple of 4")
        self.ma = nn.MultiheadAttention(c1, num_heads, dropout=dropout, batch_first=True)
        self.fc1 = nn.Linear(c1, cm)
        self.fc2 = nn.Linear(cm, c1)
        self.norm1 = nn.LayerNorm(c1)
        self.norm2 = nn.LayerNorm(c1)
        self.dropout = nn.Dropout(dropout)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.act = act
        self.normalize_before = normalize_before
        self._c, self._heads = c1, num_heads

    def _pos(self, x):
        return None

    def _check(self, normalize_before, dropout, act):
        """what has no kernel: the constructor's arguments, and again what the attributes hold when the layer runs"""
        who = type(self).__name__
        if normalize_before:
            raise NotImplementedError(f"{who}: normalize_before=True (forward_pre) is not implemented")
        if dropout:
            raise NotImplementedError(f"{who}: dropout > 0 is not implemented")
        if not isinstance(act, nn.GELU) or getattr(act, "approximate", "none") != "none":
            raise NotImplementedError(f"{who}: only the exact nn.GELU() activation is implemented, got {act!r}")

    def forward(self, x, src_mask=None, src_key_padding_mask=None, pos=None, out=None):
        if src_mask is not None or src_key_padding_mask is not None:
            raise NotImplementedError(f"{type(self).__name__}: attention masks and key-padding masks are not implemented")
        if pos is not None:
            raise NotImplementedError(f"{type(self).__name__}: an explicit position tensor is not implemented (AIFI builds its own table)")
        return super().forward(x, out=out)

    def _fwd(self, tape, x, out=None):
        self._check(self.normalize_before, self.ma.dropout or self.dropout.p or self.dropout1.p or self.dropout2.p, self.act)
        pos = self._pos(x)
        p = x if pos is None else ops.add_pos(x, pos)
        s2 = self._attn_fwd(tape, p, p, x)
        x1 = ops.add_layernorm_forward(tape, x, s2, self.norm1)
        u = _linear(tape, x1, self.fc1.weight, self.fc1.bias)
        t = ops.gelu_forward(tape, u)
        s3 = _linear(tape, t, self.fc2.weight, self.fc2.bias)
        return ops.add_layernorm_forward(tape, x1, s3, self.norm2, out=out)

    def _bwd(self, tape, dy, needs=(True,)):
        C_ = self._c
        dz2 = ops.add_layernorm_backward(tape, dy)                         # norm2: the gradient of x1 (residual) and of fc2's output
        dt = conv_backward(tape, dz2)                                      # fc2
        du = ops.gelu_backward(tape, dt)
        dx1 = conv_backward(tape, du, add_src=dz2)                         # fc1; + the second residual
        dz1 = ops.add_layernorm_backward(tape, dx1)                        # norm1: the gradient of src (residual) and of out_proj's output
        g = self._attn_bwd(tape, dz1)
        dx = conv_backward(tape, g[:, 2 * C_:], add_src=dz1)               # V's in-projection reads src; + the first residual
        for i in (1, 0):                                                   # K, Q read src + pos: the table gets no gradient
            conv_backward(tape, g[:, i * C_:(i + 1) * C_], dx_out=dx, accumulate=True)
        self._join_in_proj(tape)
        return dx


class AIFI(TransformerEncoderLayer):
    """TransformerEncoderLayer on a [B, C, H, W] map with the fixed 2D sine-cosine position table added to the queries and keys
    (reference transformer.py:70-97).  The table is the reference's build_2d_sincos_position_embedding(w, h, C), built on the host
    and cached per (w, h, C, dtype, device) (ops.pos_table): its row p holds (iw, ih) = (p // H, p % H) while token p is the pixel
    (p // W, p % W) -- on a non-square map the two disagree, and the reference trains that way."""

    def __init__(self, c1, cm=2048, num_heads=8, dropout=0, act=nn.GELU(), normalize_before=False):
        if c1 % 4:
            raise ValueError("Embed dimension must be divisible by 4 for 2D sin-cos position embedding")
        super().__init__(c1, cm, num_heads, dropout, act, normalize_before)

    def _pos(self, x):
        return ops.pos_table(x.shape[3], x.shape[2], self._c, x.dtype, x.device)

    @staticmethod
    def build_2d_sincos_position_embedding(w, h, embed_dim=256, temperature=10000.0):
        return ops.sincos_pos_table(w, h, embed_dim, temperature)[None]


class PConv(DyModule):
    """FasterNet partial convolution, split_cat mode (reference conv.py:157-190): 3x3 conv on the first dim // n_div channels, the
    rest passed through -- one HIP kernel per direction (ops.pconv_forward / pconv_backward).  The inference-only 'slicing' mode
    is not provided."""

    def __init__(self, dim, n_div, forward="split_cat"):
        super().__init__()
        if forward != "split_cat":
            raise NotImplementedError("PConv: only the split_cat forward is implemented")
        self.dim_conv3 = dim // n_div
        self.dim_untouched = dim - self.dim_conv3
        self.patial_conv3 = nn.Conv2d(self.dim_conv3, self.dim_conv3, 3, 1, 1, bias=False)

    def _fwd(self, tape, x, out=None):
        return ops.pconv_forward(tape, x, self.patial_conv3.weight, out=out)

    def _bwd(self, tape, dy, needs=(True,), dx_out=None, accumulate=False, add_src=None):
        return ops.pconv_backward(tape, dy, dx_out=dx_out, accumulate=accumulate, add_src=add_src)


class _PconvBottleneckBase(DyModule):
    """fasterblock (PConv -> Conv [-> bias-free 1x1]) -> bias-free 1x1 [+ x].  The last 1x1 conv writes straight into `out`; the
    shortcut is then added in place (one pass; conv_forward's residual route without BatchNorm would stage the conv output in a
    temporary).  Backward routes the shortcut and C2f's gradient-buffer accumulate through PConv's data gradient."""

    def _last(self):
        raise NotImplementedError

    def _fwd(self, tape, x, out=None):
        fb = self.fasterblock
        t = fb[1]._fwd(tape, fb[0]._fwd(tape, x))
        y = conv_forward(tape, t, self._last().weight, None, None, ACT_NONE, 1, 0, 1, False, out=out)
        if self.add:
            copy2d(x, y, accumulate=True)
            ops.emu_round(y)
        return y

    def _bwd(self, tape, dy, needs=(True,), dx_out=None, accumulate=False):
        fb = self.fasterblock
        du = conv_backward(tape, dy)
        dt = fb[1]._bwd(tape, du)
        return fb[0]._bwd(tape, dt, dx_out=dx_out, accumulate=accumulate, add_src=dy if self.add else None)


class PconvBottleneck(_PconvBottleneckBase):
    """PConv -> Conv 3x3 -> 1x1 [+ x] (reference block.py:568-587)."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        if g != 1:
            raise NotImplementedError("grouped convolution is outside the Dedark-YOLO hot path")
        c_ = int(c2 * e)
        self.fasterblock = nn.Sequential(PConv(dim=c1, n_div=4), Conv(c1=c1, c2=c_, k=3, s=1, p=1))
        self.conv = nn.Conv2d(c_, c2, 1, 1, autopad(1, None, 1), groups=g, bias=False)
        self.add = shortcut and c1 == c2

    def _last(self):
        return self.conv


class PconvBottleneck_n(_PconvBottleneckBase):
    """PConv -> Conv 1x1 (2c_) -> 1x1 [+ x], all inside `fasterblock` (reference block.py:590-607)."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        if g != 1:
            raise NotImplementedError("grouped convolution is outside the Dedark-YOLO hot path")
        c_ = int(c2 * e)
        self.fasterblock = nn.Sequential(PConv(dim=c1, n_div=4), Conv(c1=c1, c2=2 * c_, k=1, s=1),
                                         nn.Conv2d(2 * c_, c2, 1, 1, autopad(1, None, 1), groups=g, bias=False))
        self.add = shortcut and c1 == c2

    def _last(self):
        return self.fasterblock[2]


class FasterC2f_N(C2f):
    """C2f with PconvBottleneck_n blocks (reference block.py:396-405); same single-buffer dataflow as C2f."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(PconvBottleneck_n(self.c, self.c, shortcut, g=g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n))


class FasterC2f(C2f):
    """C2f with PconvBottleneck blocks (reference block.py:408-415)."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(PconvBottleneck(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n))


class SPPF(DyModule):
    """cv1 -> 3 chained MaxPool2d(5,1,2) -> cat -> cv2 (reference block.py:323-338); pools write into slices."""

    def __init__(self, c1, c2, k=5):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * 4, c2, 1, 1)
        self.k = k
        self.c_ = c_

    def _fwd(self, tape, x, out=None):
        c_, k = self.c_, self.k
        B, _, H, W = x.shape
        Y = empty_nhwc(B, 4 * c_, H, W, x.dtype, x.device)
        self.cv1._fwd(tape, x, out=Y[:, :c_])
        args = []
        for i in range(3):
            _, a = ops.maxpool_fwd(Y[:, i * c_:(i + 1) * c_], k, 1, k // 2, out=Y[:, (i + 1) * c_:(i + 2) * c_],
                                   want_arg=tape is not None)
            args.append(a)
        if tape is not None:
            tape.push(args)
        return self.cv2._fwd(tape, Y, out=out)

    def _bwd(self, tape, dy, needs=(True,)):
        c_, k = self.c_, self.k
        dY = self.cv2._bwd(tape, dy)
        args = tape.pop()
        B, _, H, W = dY.shape
        for i in reversed(range(3)):
            ops.maxpool_bwd(dY[:, (i + 1) * c_:(i + 2) * c_], args[i], (B, c_, H, W), k, 1, k // 2,
                            dx_out=dY[:, i * c_:(i + 1) * c_], accumulate=True)
        return self.cv1._bwd(tape, dY[:, :c_], needs=needs)


def _asff_blend_fwd(tape, rs, levels, weight_levels, level_conv, logits_conv):
    """The blend stage of the ASFF blocks: levels[k] (through level_conv(tape, m, x, out=)) compresses source rs[k] into its slice
    of one weight-vector buffer, weight_levels (through logits_conv(tape, m, x)) turns that into one logit per source and pixel,
    and ops.asff_fuse_forward blends the sources under their soft-max.  Returns the fused map."""
    n, c = len(rs), weight_levels.in_channels // len(rs)
    B, _, H, W = rs[0].shape
    wv = empty_nhwc(B, n * c, H, W, rs[0].dtype, rs[0].device)
    for k in range(n):
        level_conv(tape, levels[k], rs[k], out=wv[:, k * c:(k + 1) * c])
    logits = logits_conv(tape, weight_levels, wv)                             # [B,n,H,W] view of a channel-padded buffer
    fused = ops.asff_fuse_forward(rs, logits)
    if tape is not None:
        tape.push((rs, logits))
    return fused


def _asff_blend_bwd(tape, dfused, into=None):
    """Mirror of _asff_blend_fwd: the gradients of the sources, each the blend's part plus its level conv's.  into[k]: a gradient
    another consumer of source k already left, which both add into."""
    rs, logits = tape.pop()
    dr, dlog = ops.asff_fuse_backward(dfused, rs, logits, into)
    dwv = conv_backward(tape, dlog)                                           # weight_levels -> the weight-vector buffer
    c = dwv.shape[1] // len(rs)
    for k in reversed(range(len(rs))):
        conv_backward(tape, dwv[:, k * c:(k + 1) * c], dx_out=dr[k], accumulate=True)
    return dr


def _add_conv_fwd(training):
    return lambda tape, m, x, out=None: m._fwd(tape, x, training, out=out)


class AsffTribeLevel(DyModule):
    """3-level adaptive spatial feature fusion (reference block.py:48-115). Inputs (P5, P4, P3)."""

    def __init__(self, level):
        super().__init__()
        self.level = level
        self.dim = [512, 512, 256]
        self.inter_dim = self.dim[level]
        if level == 0:
            self.stride_level_1 = nn.MaxPool2d(kernel_size=2, stride=2)
            self.stride_level_2 = AddConv(256, self.inter_dim, 3, 2)
            self.expand = AddConv(self.inter_dim, 512, 3, 1)
        elif level == 1:
            self.stride_level_2 = AddConv(256, self.inter_dim, 3, 2)
            self.expand = AddConv(self.inter_dim, 512, 3, 1)
        elif level == 2:
            self.compress_level_0 = AddConv(512, self.inter_dim, 1, 1)
            self.compress_level_1 = AddConv(512, self.inter_dim, 1, 1)
            self.expand = AddConv(self.inter_dim, 256, 3, 1)
        compress_c = 8
        self.weight_level_0 = AddConv(self.inter_dim, compress_c, 1, 1)
        self.weight_level_1 = AddConv(self.inter_dim, compress_c, 1, 1)
        self.weight_level_2 = AddConv(self.inter_dim, compress_c, 1, 1)
        self.weight_levels = nn.Conv2d(compress_c * 3, 3, kernel_size=1, stride=1, padding=0)

    def _fwd(self, tape, x0, x1, x2):
        tr = self.training
        saved = {}
        if self.level == 0:
            r0 = x0
            r1, saved["a1"] = ops.maxpool_fwd(x1, 2, 2, 0, want_arg=tape is not None)
            p2, saved["a2"] = ops.maxpool_fwd(x2, 3, 2, 1, want_arg=tape is not None)
            r2 = self.stride_level_2._fwd(tape, p2, tr)
        elif self.level == 1:
            r0 = ops.upsample_fwd(x0, 2)
            r1 = x1
            r2 = self.stride_level_2._fwd(tape, x2, tr)
        else:
            r0 = ops.upsample_fwd(self.compress_level_0._fwd(tape, x0, tr), 4)
            r1 = ops.upsample_fwd(self.compress_level_1._fwd(tape, x1, tr), 2)
            r2 = x2
        fused = _asff_blend_fwd(tape, (r0, r1, r2), (self.weight_level_0, self.weight_level_1, self.weight_level_2), self.weight_levels,
                                _add_conv_fwd(tr), plain_conv_fwd)
        if tape is not None:
            saved.update(shapes=(x0.shape, x1.shape, x2.shape))
            tape.push(saved)
        return self.expand._fwd(tape, fused, tr)

    _takes_into = True

    def _bwd(self, tape, dy, needs=(True, True, True), into=None):
        dfused = conv_backward(tape, dy)
        s = tape.pop()
        into = list(into) if into is not None else [None, None, None]
        # the input this level takes as it is (r_k = x_k): the blend's gradient adds straight into what another consumer left
        dr = _asff_blend_bwd(tape, dfused, [t if k == self.level else None for k, t in enumerate(into)])
        (s0, s1, s2) = s["shapes"]
        A = [dict(dx_out=t, accumulate=True) if t is not None else {} for t in into]      # add into an existing gradient
        if self.level == 0:
            dp2 = conv_backward(tape, dr[2])                                  # stride_level_2
            dx2 = ops.maxpool_bwd(dp2, s["a2"], tuple(s2), 3, 2, 1, **A[2])
            dx1 = ops.maxpool_bwd(dr[1], s["a1"], tuple(s1), 2, 2, 0, **A[1])
            dx0 = dr[0]
        elif self.level == 1:
            dx2 = conv_backward(tape, dr[2], **A[2])
            dx1 = dr[1]
            dx0 = ops.upsample_bwd(dr[0], 2, **A[0])
        else:
            dx2 = dr[2]
            dx1 = conv_backward(tape, ops.upsample_bwd(dr[1], 2), **A[1])     # compress_level_1
            dx0 = conv_backward(tape, ops.upsample_bwd(dr[0], 4), **A[0])     # compress_level_0
        return tuple(None if into[k] is not None else d for k, d in enumerate((dx0, dx1, dx2)))


class GroupBatchnorm2d(nn.Module):
    """Parameter container (reference ultralytics/nn/modules/conv.py:323-343): weight ~ randn(c, 1, 1), bias = 0, eps 1e-10."""

    def __init__(self, c_num, group_num=16, eps=1e-10):
        super().__init__()
        assert c_num >= group_num
        self.group_num = group_num
        self.weight = nn.Parameter(torch.randn(c_num, 1, 1))
        self.bias = nn.Parameter(torch.zeros(c_num, 1, 1))
        self.eps = eps


class SRU(nn.Module):
    """Spatial reconstruction unit (conv.py:346-376): container; the arithmetic is dy_chan_moments + dy_sru_fwd / dy_sru_bwd."""

    def __init__(self, oup_channels, group_num=16, gate_treshold=0.5, torch_gn=False):
        super().__init__()
        if torch_gn or gate_treshold != 0.5:
            raise NotImplementedError("SRU: only the GroupBatchnorm2d variant with the 0.5 gate (what SCConv builds) is implemented")
        self.gn = GroupBatchnorm2d(oup_channels, group_num=group_num)
        self.gate_treshold = gate_treshold


class CRU(nn.Module):
    """Channel reconstruction unit (conv.py:379-417): container of its six convolutions (alpha 1/2, squeeze 2, 2 groups, 3x3)."""

    def __init__(self, op_channel, alpha=1 / 2, squeeze_radio=2, group_size=2, group_kernel_size=3):
        super().__init__()
        if (alpha, squeeze_radio, group_size, group_kernel_size) != (1 / 2, 2, 2, 3):
            raise NotImplementedError("CRU: only the default split (what SCConv / MFRU build) is implemented")
        self.up_channel = up = int(alpha * op_channel)
        self.low_channel = low = op_channel - up
        self.squeeze1 = nn.Conv2d(up, up // squeeze_radio, kernel_size=1, bias=False)
        self.squeeze2 = nn.Conv2d(low, low // squeeze_radio, kernel_size=1, bias=False)
        self.GWC = nn.Conv2d(up // squeeze_radio, op_channel, kernel_size=group_kernel_size, stride=1, padding=group_kernel_size // 2,
                             groups=group_size)
        self.PWC1 = nn.Conv2d(up // squeeze_radio, op_channel, kernel_size=1, bias=False)
        self.PWC2 = nn.Conv2d(low // squeeze_radio, op_channel - low // squeeze_radio, kernel_size=1, bias=False)


class SCConv(DyModule):
    """Spatial and channel reconstruction convolution (reference conv.py:420-440): SRU then CRU, channels preserved.
    Every parameter may be used more than once per step (MFRU applies one SCConv to two inputs), so all gradients are collected
    on the tape (which adds them up) instead of being written in place."""

    def __init__(self, op_channel, group_num=4, gate_treshold=0.5, alpha=1 / 2, squeeze_radio=2, group_size=2, group_kernel_size=3):
        super().__init__()
        if op_channel % 16 != 0 or not 16 <= op_channel <= 2048:
            raise NotImplementedError("SCConv: channel count must be a multiple of 16 in 16..2048 (C/8 input channels per GWC group, whole "
                                      "16-byte vectors of the SRU halves)")
        # C % 64 == 0 (MFRU's widths): the CRU is composed of the generic conv routes on 16-byte channel slices.  Any other width has
        # slices of 2 / 6 / 10 ... channels: the CRU convolutions run on the dy_cru_conv_* kernels (ops.cru_conv_forward).
        self._cru = op_channel % 64 != 0
        self.SRU = SRU(op_channel, group_num=group_num, gate_treshold=gate_treshold)
        self.CRU = CRU(op_channel, alpha=alpha, squeeze_radio=squeeze_radio, group_size=group_size, group_kernel_size=group_kernel_size)
        self.c = op_channel

    def _gwc_views(self):
        g = self.CRU.GWC
        key = (g.weight.data_ptr(), g.bias.data_ptr())
        c = self.__dict__.get("_gwc_cache")
        if c is None or c[0] != key:
            h = self.c // 2
            # slices of the parameters as gradient-taking leaves of their own: conv_backward files their gradients under these
            # objects, _bwd copies them into the halves of the full GWC gradient
            c = (key, [g.weight.detach()[j * h:(j + 1) * h].requires_grad_(True) for j in range(2)],
                 [g.bias.detach()[j * h:(j + 1) * h].requires_grad_(True) for j in range(2)])
            self.__dict__["_gwc_cache"] = c
            for w in c[1]:
                ops.register_pack_view(w)
        return c[1], c[2]

    def _fwd(self, tape, x, out=None):
        """out: optional NHWC view the result is written into (Conv3_SC_Bottleneck inside a C2f buffer)"""
        B, C_, H, W = x.shape
        if C_ != self.c:
            raise RuntimeError(f"SCConv: expected {self.c} channels, got {C_}")
        dt, dev, did, st = x.dtype, x.device, ops.dt_id(x.dtype), stream()
        gn, cru = self.SRU.gn, self.CRU
        mom = torch.zeros((B, C_, 2), dtype=torch.float64, device=dev)
        call("dy_chan_moments", ptr(x), ld_of(x), B, H * W, C_, ptr(mom), did, st)
        y = empty_nhwc(B, C_, H, W, dt, dev)
        call("dy_sru_fwd", ptr(x), ld_of(x), ptr(y), ld_of(y), B, H * W, C_, gn.group_num, ptr(mom), ptr(gn.weight), ptr(gn.bias),
             float(gn.eps), did, st)
        h, q, e = C_ // 2, C_ // 4, C_ // 8
        buf = empty_nhwc(B, 2 * C_, H, W, dt, dev)                       # cat(Y1 [C], PWC2(low) [3C/4], low [C/4])
        if self._cru:
            wv = bv = None
            sq1 = ops.cru_conv_forward(tape, y[:, :h], None, None, cru.squeeze1.weight)
            low = ops.cru_conv_forward(tape, y[:, h:], None, None, cru.squeeze2.weight, out=buf[:, 2 * C_ - q:])
            ops.cru_conv_forward(tape, sq1, cru.GWC.weight, cru.GWC.bias, cru.PWC1.weight, G=2, out=buf[:, :C_])      # Y1, one accumulator
            ops.cru_conv_forward(tape, low, None, None, cru.PWC2.weight, out=buf[:, C_:2 * C_ - q])
        else:
            wv, bv = self._composed_cru_fwd(tape, y, buf)
        mom2 = torch.zeros((B, 2 * C_, 2), dtype=torch.float64, device=dev)
        call("dy_chan_moments", ptr(buf), ld_of(buf), B, H * W, 2 * C_, ptr(mom2), did, st)
        res = out if out is not None else empty_nhwc(B, C_, H, W, dt, dev)
        call("dy_cru_fuse_fwd", ptr(buf), ld_of(buf), ptr(res), ld_of(res), B, H * W, C_, ptr(mom2), did, st)
        if tape is not None:
            tape.push(dict(x=x, mom=mom, buf=buf, mom2=mom2, views=(wv, bv)))
        return res

    def _composed_cru_fwd(self, tape, y, buf):
        cru = self.CRU
        C_ = self.c
        h, q, e = C_ // 2, C_ // 4, C_ // 8
        kw = dict(shared=True)
        sq1 = conv_forward(tape, y[:, :h], cru.squeeze1.weight, None, None, ACT_NONE, 1, 0, 1, False, **kw)
        sq2 = conv_forward(tape, y[:, h:], cru.squeeze2.weight, None, None, ACT_NONE, 1, 0, 1, False, out=buf[:, 2 * C_ - q:], **kw)
        wv, bv = self._gwc_views()
        for j in range(2):                                               # grouped 3x3: group j maps channels [j e, (j+1) e) to [j h, (j+1) h)
            conv_forward(tape, sq1[:, j * e:(j + 1) * e], wv[j], bv[j], None, ACT_NONE, 1, 1, 1, False, out=buf[:, j * h:(j + 1) * h], **kw)
        pw1 = conv_forward(tape, sq1, cru.PWC1.weight, None, None, ACT_NONE, 1, 0, 1, False, **kw)
        copy2d(pw1, buf[:, :C_], accumulate=True)                        # Y1 = GWC(up) + PWC1(up)
        conv_forward(tape, sq2, cru.PWC2.weight, None, None, ACT_NONE, 1, 0, 1, False, out=buf[:, C_:2 * C_ - q], **kw)
        return wv, bv

    def _bwd(self, tape, dres, needs=(True,)):
        s = tape.pop()
        x, mom, buf, mom2, (wv, bv) = s["x"], s["mom"], s["buf"], s["mom2"], s["views"]
        B, C_, H, W = x.shape
        dt, dev, did, st = x.dtype, x.device, ops.dt_id(x.dtype), stream()
        gn, cru = self.SRU.gn, self.CRU
        h, q, e = C_ // 2, C_ // 4, C_ // 8
        dbuf = empty_nhwc(B, 2 * C_, H, W, dt, dev)
        ds = torch.zeros((B, 2 * C_, 2), dtype=torch.float64, device=dev)
        call("dy_cru_fuse_bwd", ptr(buf), ld_of(buf), ptr(dres), ld_of(dres), ptr(dbuf), ld_of(dbuf), B, H * W, C_, ptr(mom2), ptr(ds), did, st)
        dy = empty_nhwc(B, C_, H, W, dt, dev)
        if self._cru:
            ops.cru_conv_backward(tape, dbuf[:, C_:2 * C_ - q], dx_out=dbuf[:, 2 * C_ - q:], accumulate=True)     # PWC2: d low' += ...
            dsq1 = ops.cru_conv_backward(tape, dbuf[:, :C_])                                           # GWC^T + PWC1^T, one accumulator
            ops.cru_conv_backward(tape, dbuf[:, 2 * C_ - q:], dx_out=dy[:, h:])                        # squeeze2
            ops.cru_conv_backward(tape, dsq1, dx_out=dy[:, :h])                                        # squeeze1
        else:
            self._composed_cru_bwd(tape, dbuf, dy, wv, bv)
        dx = empty_nhwc(B, C_, H, W, dt, dev)
        red = torch.zeros((B, C_, 2), dtype=torch.float64, device=dev)
        call("dy_sru_bwd", ptr(x), ld_of(x), ptr(dy), ld_of(dy), ptr(dx), ld_of(dx), B, H * W, C_, gn.group_num, ptr(mom), ptr(gn.weight),
             ptr(gn.bias), float(gn.eps), ptr(red), did, st)
        tot = red.sum(0).float()
        ops._add_pgrad(tape, gn.weight, tot[:, 1].reshape(C_, 1, 1))
        ops._add_pgrad(tape, gn.bias, tot[:, 0].reshape(C_, 1, 1))
        return dx

    def _composed_cru_bwd(self, tape, dbuf, dy, wv, bv):
        cru = self.CRU
        C_ = self.c
        h, q, e = C_ // 2, C_ // 4, C_ // 8
        conv_backward(tape, dbuf[:, C_:2 * C_ - q], dx_out=dbuf[:, 2 * C_ - q:], accumulate=True)       # PWC2: d low' += ...
        dsq1 = conv_backward(tape, dbuf[:, :C_])                                                       # PWC1
        gw = torch.empty_like(cru.GWC.weight)
        gb = torch.empty_like(cru.GWC.bias)
        for j in (1, 0):                                                                               # GWC groups, reverse order
            conv_backward(tape, dbuf[:, j * h:(j + 1) * h], dx_out=dsq1[:, j * e:(j + 1) * e], accumulate=True)
            gw[j * h:(j + 1) * h].copy_(tape.pgrads.pop(wv[j]).view(h, e, 3, 3))
            gb[j * h:(j + 1) * h].copy_(tape.pgrads.pop(bv[j]).view(h))
        ops._add_pgrad(tape, cru.GWC.weight, gw)
        ops._add_pgrad(tape, cru.GWC.bias, gb)
        conv_backward(tape, dbuf[:, 2 * C_ - q:], dx_out=dy[:, h:])                                    # squeeze2
        conv_backward(tape, dsq1, dx_out=dy[:, :h])                                                    # squeeze1


def _flush_shared_grads(tape):
    """Gradients collected on the tape for parameters that a module uses more than once: under the trainer's direct placement they
    are copied into the parameter's slot of the flat gradient buffer (and leave the tape), otherwise autograd gets them."""
    for p in list(tape.pgrads):
        gd = ops._grad_dst(p)
        if gd is not None:
            gd.copy_(tape.pgrads.pop(p).view_as(gd))


class _SCBottleneckBase(DyModule):
    """SandCRblock(x) [+ x] with SandCRblock = (SCConv, conv) or (conv, SCConv): the bottlenecks of the SCConv C2f family (reference
    block.py:610-700).  The conv is a Conv (BatchNorm + SiLU; the shortcut rides on its BatchNorm pass as in Bottleneck) or a plain
    nn.Conv2d with bias.  SCConv's gradients are collected on the tape and flushed to their slots like MFRU's."""
    _sc_first = True

    def _make(self, c1, c2, shortcut, g, conv):
        if g != 1:
            raise NotImplementedError("grouped convolution is outside the Dedark-YOLO hot path")
        self.SandCRblock = nn.Sequential(SCConv(c1), conv) if self._sc_first else nn.Sequential(conv, SCConv(c2))
        self.add = shortcut and c1 == c2

    def _fwd(self, tape, x, out=None):
        a, b = self.SandCRblock
        res = x if self.add else None
        if not self._sc_first:                                    # Conv -> SCConv: the CRU tail writes into `out`, the shortcut is added in place
            y = b._fwd(tape, a._fwd(tape, x), out=out)
            if res is not None:
                copy2d(res, y, accumulate=True)
                ops.emu_round(y)
            return y
        t = a._fwd(tape, x)
        if isinstance(b, Conv):
            return b._fwd(tape, t, out=out, residual=res)
        y = plain_conv_fwd(tape, b, t, out=out)
        if res is not None:
            copy2d(res, y, accumulate=True)
            ops.emu_round(y)
        return y

    def _bwd(self, tape, dy, needs=(True,), dx_out=None, accumulate=False):
        a, b = self.SandCRblock
        if not self._sc_first:
            dt = b._bwd(tape, dy)
            _flush_shared_grads(tape)
            return a._bwd(tape, dt, dx_out=dx_out, accumulate=accumulate, add_src=dy if self.add else None)
        dt = b._bwd(tape, dy) if isinstance(b, Conv) else conv_backward(tape, dy)
        dx = a._bwd(tape, dt)                                     # SRU backward writes a buffer of its own
        _flush_shared_grads(tape)
        if self.add:
            copy2d(dy, dx, accumulate=True)
            ops.emu_round(dx)
        if dx_out is None:
            return dx
        copy2d(dx, dx_out, accumulate=accumulate)
        if accumulate:
            ops.emu_round(dx_out)
        return dx_out

class SCConvBottleneck(_SCBottleneckBase):
    """SCConv -> Conv 1x1 [+ x] (reference block.py:610-627)."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        self._make(c1, c2, shortcut, g, Conv(c1=c1, c2=c2, k=1, s=1))


class SC_PW_Bottleneck(_SCBottleneckBase):
    """SCConv -> nn.Conv2d 1x1 with bias, no BatchNorm [+ x] (reference block.py:630-645)."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        self._make(c1, c2, shortcut, g, nn.Conv2d(c1, c2, 1, 1, autopad(1, None, 1), groups=g, bias=True))


class SC_Conv3_Bottleneck(_SCBottleneckBase):
    """SCConv -> Conv 3x3 [+ x] (reference block.py:648-662)."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        self._make(c1, c2, shortcut, g, Conv(c1=c1, c2=c2, k=3, s=1, p=autopad(3, d=1), g=g))


class Conv3_SC_Bottleneck(_SCBottleneckBase):
    """Conv 3x3 -> SCConv [+ x] (reference block.py:684-700)."""
    _sc_first = False

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        self._make(c1, c2, shortcut, g, Conv(c1=c1, c2=c2, k=3, s=1, p=autopad(3, d=1), g=g))


class _SCC2fBase(C2f):
    """C2f whose blocks are one of the SCConv bottlenecks (reference block.py:418-459): C2f's buffer-slice forward and backward as
    they are."""
    _block = None

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(self._block(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n))


class SCC2f(_SCC2fBase):
    """C2f of SCConvBottleneck (reference block.py:418-426)."""
    _block = SCConvBottleneck


class SC_PW_C2f(_SCC2fBase):
    """C2f of SC_PW_Bottleneck (reference block.py:429-437)."""
    _block = SC_PW_Bottleneck


class SC_Conv3_C2f(_SCC2fBase):
    """C2f of SC_Conv3_Bottleneck (reference block.py:440-448)."""
    _block = SC_Conv3_Bottleneck


class Conv3_SC_C2f(_SCC2fBase):
    """C2f of Conv3_SC_Bottleneck (reference block.py:451-459)."""
    _block = Conv3_SC_Bottleneck


class MFRU(DyModule):
    """Multi-scale feature reconstruction unit (reference block.py:164-217, yolov8-3.yaml).  Inputs (P5 512 ch, P4 512 ch, P3 256 ch);
    ONE SCConv(512) + 1x1 conv serve both coarse levels and ONE SCConv(256) serves the fine level and the fused map; output 256
    channels at the P3 size."""

    def __init__(self, level=None):
        super().__init__()
        compress_c = 16
        self.scconv512 = SCConv(512)
        self.scconv256 = SCConv(256)
        self.pwconv = nn.Conv2d(512, 256, 1, 1, 0)
        self.weight_level_0 = nn.Conv2d(256, compress_c, 1, 1, 0)
        self.weight_level_1 = nn.Conv2d(256, compress_c, 1, 1, 0)
        self.weight_level_2 = nn.Conv2d(256, compress_c, 1, 1, 0)
        self.weight_levels = nn.Conv2d(compress_c * 3, 3, 1, 1, 0)

    def _pw(self, tape, m, x, out=None):
        return conv_forward(tape, x, m.weight, m.bias, None, ACT_NONE, 1, 0, 1, False, out=out, shared=True)

    def _fwd(self, tape, x0, x1, x2):
        r0 = ops.upsample_fwd(self._pw(tape, self.pwconv, self.scconv512._fwd(tape, x0)), 4)
        r1 = ops.upsample_fwd(self._pw(tape, self.pwconv, self.scconv512._fwd(tape, x1)), 2)
        r2 = self.scconv256._fwd(tape, x2)
        if tuple(r0.shape) != tuple(r2.shape) or tuple(r1.shape) != tuple(r2.shape):
            raise RuntimeError("MFRU: inputs must be at strides 4 : 2 : 1")
        fused = _asff_blend_fwd(tape, (r0, r1, r2), (self.weight_level_0, self.weight_level_1, self.weight_level_2), self.weight_levels,
                                self._pw, self._pw)
        return self.scconv256._fwd(tape, fused)

    def _bwd(self, tape, dy, needs=(True, True, True)):
        dr = _asff_blend_bwd(tape, self.scconv256._bwd(tape, dy))
        dx2 = self.scconv256._bwd(tape, dr[2])
        dx1 = self.scconv512._bwd(tape, conv_backward(tape, ops.upsample_bwd(dr[1], 2)))
        dx0 = self.scconv512._bwd(tape, conv_backward(tape, ops.upsample_bwd(dr[0], 4)))
        _flush_shared_grads(tape)
        return dx0, dx1, dx2


class AsffDoubLevel(DyModule):
    """2-level adaptive spatial feature fusion (reference block.py:118-162).  Inputs (P4-like 512 ch, P3-like 256 ch at twice the
    resolution); level 0 fuses at the coarse size (512 ch out), level 1 at the fine size (256 ch out)."""

    def __init__(self, level):
        super().__init__()
        self.level = level
        self.dim = [512, 256]
        self.inter_dim = self.dim[level]
        if level == 0:
            self.stride_level_1 = AddConv(256, self.inter_dim, 3, 2)
            self.expand = AddConv(self.inter_dim, 512, 3, 1)
        elif level == 1:
            self.compress_level_0 = AddConv(512, self.inter_dim, 1, 1)
            self.expand = AddConv(self.inter_dim, 256, 3, 1)
        compress_c = 16
        self.weight_level_0 = AddConv(self.inter_dim, compress_c, 1, 1)
        self.weight_level_1 = AddConv(self.inter_dim, compress_c, 1, 1)
        self.weight_levels = nn.Conv2d(compress_c * 2, 2, kernel_size=1, stride=1, padding=0)

    def _fwd(self, tape, x0, x1):
        tr = self.training
        if self.level == 0:
            r0 = x0
            r1 = self.stride_level_1._fwd(tape, x1, tr)
        else:
            r0 = ops.upsample_fwd(self.compress_level_0._fwd(tape, x0, tr), 2)
            r1 = x1
        fused = _asff_blend_fwd(tape, (r0, r1), (self.weight_level_0, self.weight_level_1), self.weight_levels, _add_conv_fwd(tr), plain_conv_fwd)
        return self.expand._fwd(tape, fused, tr)

    def _bwd(self, tape, dy, needs=(True, True)):
        dr = _asff_blend_bwd(tape, conv_backward(tape, dy))
        if self.level == 0:
            dx1 = conv_backward(tape, dr[1])                                  # stride_level_1
            dx0 = dr[0]
        else:
            dx1 = dr[1]
            dx0 = conv_backward(tape, ops.upsample_bwd(dr[0], 2))             # compress_level_0
        return dx0, dx1


class RFBblock(DyModule):
    """Receptive-field block: four branches of biased convs with dilations 1/1/2/3, concatenated
    (reference block.py:703-734).  Branch outputs are written into slices of the output buffer."""

    def __init__(self, in_ch):
        super().__init__()
        q = in_ch // 4
        self.branch_0 = nn.Sequential(nn.Conv2d(in_ch, q, 1, 1, 0))
        self.branch_1 = nn.Sequential(nn.Conv2d(in_ch, q, 1, 1, 0), nn.Conv2d(q, q, 3, 1, 1))
        self.branch_2 = nn.Sequential(nn.Conv2d(in_ch, q, 1, 1, 0), nn.Conv2d(q, q, 3, 1, 1), nn.Conv2d(q, q, 3, 1, dilation=2, padding=2))
        self.branch_3 = nn.Sequential(nn.Conv2d(in_ch, q, 1, 1, 0), nn.Conv2d(q, q, 5, 1, 2), nn.Conv2d(q, q, 3, 1, dilation=3, padding=3))
        self.q = q

    def _branches(self):
        return (self.branch_0, self.branch_1, self.branch_2, self.branch_3)

    def _fwd(self, tape, x):
        B, _, H, W = x.shape
        q = self.q
        out = empty_nhwc(B, 4 * q, H, W, x.dtype, x.device)
        for i, br in enumerate(self._branches()):
            t = x
            for j, m in enumerate(br):
                t = plain_conv_fwd(tape, m, t, out=out[:, i * q:(i + 1) * q] if j == len(br) - 1 else None)
        return out

    def _bwd(self, tape, dy, needs=(True,)):
        q = self.q
        dx = None
        for i in reversed(range(4)):
            g = dy[:, i * q:(i + 1) * q]
            br = self._branches()[i]
            for j in reversed(range(len(br))):
                if j == 0:
                    dx = conv_backward(tape, g, dx_out=dx, accumulate=dx is not None)
                else:
                    g = conv_backward(tape, g)
        return dx


class DFL(nn.Module):
    """Integral of the distribution focal loss bins (reference block.py:220-238). The frozen 1x1 conv (weights = arange)
    is kept for state_dict compatibility; the softmax-expectation itself runs inside the decode kernels."""

    def __init__(self, c1=16):
        super().__init__()
        self.conv = nn.Conv2d(c1, 1, 1, bias=False).requires_grad_(False)
        self.conv.weight.data[:] = torch.arange(c1, dtype=torch.float).view(1, c1, 1, 1)
        self.c1 = c1


class Detect(DyModule):
    """YOLOv8 detect head (reference ultralytics/nn/modules/head.py:19-102). Train: list of raw maps [B, 64+nc, h, w];
    eval: (y [B, 4+nc, A], maps)."""
    dynamic = False
    export = False
    shape = None
    anchors = torch.empty(0)
    strides = torch.empty(0)

    def __init__(self, nc=80, ch=()):
        super().__init__()
        self.nc = nc
        self.nl = len(ch)
        self.reg_max = 16
        self.no = nc + self.reg_max * 4
        self.stride = torch.zeros(self.nl)
        self._make_branches(ch)
        self.dfl = DFL(self.reg_max)

    def _make_branches(self, ch):
        c2, c3 = max((16, ch[0] // 4, self.reg_max * 4)), max(ch[0], min(self.nc, 100))
        self.cv2 = self._chains(ch, c2, 4 * self.reg_max)
        self.cv3 = self._chains(ch, c3, self.nc)

    @staticmethod
    def _chains(ch, c, c_out):
        """One Conv3x3, Conv3x3, Conv2d(c -> c_out, 1) chain per level: cv2, cv3 and the cv4 of Segment and Pose."""
        return nn.ModuleList(nn.Sequential(Conv(x, c, 3), Conv(c, c, 3), nn.Conv2d(c, c_out, 1)) for x in ch)

    @staticmethod
    def _chain_fwd(tape, chain, x, out=None):
        a, b, c = chain
        return plain_conv_fwd(tape, c, b._fwd(tape, a._fwd(tape, x)), out=out)

    @staticmethod
    def _chain_bwd(tape, chain, g, dx=None):
        """Gradient wrt the chain's input; added to `dx` when one is given."""
        gt = chain[1]._bwd(tape, conv_backward(tape, g))
        return chain[0]._bwd(tape, gt, dx_out=dx, accumulate=dx is not None)

    def _level_fwd(self, tape, i, x):
        B, _, H, W = x.shape
        ve = ops.vec_elems(x.dtype)
        nc_pad = ops.round_up(self.nc, ve)
        buf = empty_nhwc(B, 4 * self.reg_max + nc_pad, H, W, x.dtype, x.device)
        self._chain_fwd(tape, self.cv2[i], x, out=buf[:, :4 * self.reg_max])
        self._chain_fwd(tape, self.cv3[i], x, out=buf[:, 4 * self.reg_max:4 * self.reg_max + nc_pad])
        return buf[:, :self.no]

    def _level_bwd(self, tape, i, g):
        r = 4 * self.reg_max
        nc_pad = ops.round_up(self.nc, ops.vec_elems(g.dtype))
        if ld_of(g) < r + nc_pad:
            raise RuntimeError("Detect: gradient map lacks channel padding")
        dx = self._chain_bwd(tape, self.cv3[i], g[:, r:r + self.nc])
        return self._chain_bwd(tape, self.cv2[i], g[:, :r], dx)

    def _run_levels(self, fn, tapes, args):
        """fn(tapes[i], i, args[i]) for every pyramid level.  The levels are independent chains of small kernels (three convs
        + BatchNorm each way), so when the trainer enabled branch streams the coarser levels run on side streams next to
        level 0 on the compute stream: fork before, join after (everything later on the compute stream is ordered behind
        them).  The operand of a side level was allocated on the compute stream: it is marked as used by the side stream
        (record_stream), because the host drops its last reference (tape pop in the backward pass) while the side stream's
        kernels that read it are still queued -- without the mark the caching allocator hands the block to the next
        compute-stream allocation (level 0's weight gradient) at once and that kernel overwrites it first."""
        n = len(args)
        side = ops.branch_streams(n - 1, args[0].device) if (self.training and tapes[0] is not None) else None
        out = [None] * n
        if side is None:
            for i in range(n):
                out[i] = fn(tapes[i], i, args[i])
            return out
        main_raw = stream()
        for i in range(1, n):                       # issue the side levels first: they run while level 0 is being issued
            s = side[i - 1]
            call("dy_stream_fork", main_raw, s.cuda_stream)
            args[i].record_stream(s)
            with torch.cuda.stream(s):
                out[i] = fn(tapes[i], i, args[i])
        out[0] = fn(tapes[0], 0, args[0])
        for s in side:
            call("dy_stream_fork", s.cuda_stream, main_raw)
        return out

    def _fwd(self, tape, *xs):
        subs = [Tape() if tape is not None else None for _ in xs]          # one tape per level: the levels are independent
        maps = self._run_levels(self._level_fwd, subs, list(xs))
        if tape is not None:
            tape.push(subs)
        if self.training:
            return maps
        win = self.__dict__.get("_tta_window")
        if win is not None:                              # a pass of DetectionModel._predict_augment: no plain decode as well
            return (self._decode_into(maps, **win), *maps)
        return (self._decode(maps), *maps)

    def _decode_into(self, maps, y, col0, a_lo, a_hi, scale, flip, img_h, img_w):
        """The eval decode of one augmented pass written into columns [col0, col0 + a_hi - a_lo) of the merged y [B, 4 + nc, A_total]
        f32, de-scaled, de-flipped and clipped (dy_detect_decode_tta; reference tasks.py:320-340)."""
        if not (y.dtype == torch.float32 and y.is_contiguous() and y.dim() == 3 and y.shape[0] == maps[0].shape[0]
                and y.shape[1] == 4 + self.nc and y.device == maps[0].device):
            raise ValueError(f"Detect._decode_into: y {tuple(y.shape)} {y.dtype} is not the merged [B, {4 + self.nc}, A] f32 buffer")
        m = ops.det_maps(maps, self.strides_as_floats(), self.nc)
        call("dy_detect_decode_tta", C.byref(m), ptr(y), y.shape[2], col0, a_lo, a_hi, float(scale), int(flip or 0), float(img_h),
             float(img_w), stream())
        return y

    def _decode(self, maps):
        """The eval output y [B, 4 + nc, A] f32 of the level maps (dy_detect_decode)."""
        m = ops.det_maps(maps, self.strides_as_floats(), self.nc)
        A = sum(t.shape[2] * t.shape[3] for t in maps)
        y = torch.empty((maps[0].shape[0], 4 + self.nc, A), dtype=torch.float32, device=maps[0].device)
        call("dy_detect_decode", C.byref(m), ptr(y), stream())
        return y

    def strides_as_floats(self):
        """self.stride as host floats, read back once (float(tensor) per call is a device synchronisation)."""
        key = (id(self.stride), self.stride._version)
        if self.__dict__.get("_stride_key") != key:
            self.__dict__["_stride_host"] = [float(v) for v in self.stride.detach().cpu()]
            self.__dict__["_stride_key"] = key
        return self.__dict__["_stride_host"]

    def _wrap(self, out):
        if self.training:
            return list(out)
        return out[0], list(out[1:])

    def _require_training(self):
        if not self.training:
            raise RuntimeError(f"{type(self).__name__}: backward through the eval decode is not supported")

    @staticmethod
    def _fold_tapes(tape, subs):
        """The head's own tapes (one per level, Segment's Proto) must be used up; their parameter gradients go to `tape`."""
        for t in subs:
            assert not t.stack, "Detect head: unbalanced tape"
            for p, g in t.pgrads.items():
                ops._add_pgrad(tape, p, g)

    def _bwd(self, tape, *dmaps, needs=None):
        self._require_training()
        subs = tape.pop()
        dxs = self._run_levels(self._level_bwd, subs, list(dmaps))
        self._fold_tapes(tape, subs)
        return dxs

    def bias_init(self):
        """reference head.py:95-102."""
        for a, b, s in zip(self.cv2, self.cv3, self.stride):
            a[-1].bias.data[:] = 1.0
            b[-1].bias.data[:self.nc] = math.log(5 / self.nc / (640 / s) ** 2)


class AsffDetect(Detect):
    """Detect head with one 1x1 conv per branch and level (reference head.py:105-174): cv2[i] = Conv2d(ch_i, 64, 1),
    cv3[i] = Conv2d(ch_i, nc, 1); decode, anchors and bias_init as Detect."""

    def _make_branches(self, ch):
        self.cv2 = nn.ModuleList(nn.Sequential(nn.Conv2d(x, 4 * self.reg_max, 1)) for x in ch)
        self.cv3 = nn.ModuleList(nn.Sequential(nn.Conv2d(x, self.nc, 1)) for x in ch)

    def _level_fwd(self, tape, i, x):
        B, _, H, W = x.shape
        nc_pad = ops.round_up(self.nc, ops.vec_elems(x.dtype))
        r = 4 * self.reg_max
        buf = empty_nhwc(B, r + nc_pad, H, W, x.dtype, x.device)
        plain_conv_fwd(tape, self.cv2[i][0], x, out=buf[:, :r])
        plain_conv_fwd(tape, self.cv3[i][0], x, out=buf[:, r:r + nc_pad])
        return buf[:, :self.no]

    def _level_bwd(self, tape, i, g):
        r = 4 * self.reg_max
        nc_pad = ops.round_up(self.nc, ops.vec_elems(g.dtype))
        if ld_of(g) < r + nc_pad:
            raise RuntimeError("AsffDetect: gradient map lacks channel padding")
        dx = conv_backward(tape, g[:, r:r + self.nc])                      # cv3[i][0]
        return conv_backward(tape, g[:, :r], dx_out=dx, accumulate=True)   # cv2[i][0]


class Proto(DyModule):
    """YOLOv8 mask prototypes (reference block.py:242-254): Conv3x3 -> ConvTranspose2d(c_, c_, 2, 2) -> Conv3x3 -> Conv1x1.  The
    transposed conv runs on the conv kernels (ops.conv_transpose2x2_forward)."""

    def __init__(self, c1, c_=256, c2=32):
        super().__init__()
        self.cv1 = Conv(c1, c_, k=3)
        self.upsample = nn.ConvTranspose2d(c_, c_, 2, 2, 0, bias=True)
        self.cv2 = Conv(c_, c_, k=3)
        self.cv3 = Conv(c_, c2)

    def _fwd(self, tape, x):
        t = self.cv1._fwd(tape, x)
        t = ops.conv_transpose2x2_forward(tape, t, self.upsample.weight, self.upsample.bias)
        return self.cv3._fwd(tape, self.cv2._fwd(tape, t))

    def _bwd(self, tape, dy, needs=(True,), dx_out=None, accumulate=False):
        g = self.cv2._bwd(tape, self.cv3._bwd(tape, dy))
        g = ops.conv_transpose2x2_backward(tape, g)
        return self.cv1._bwd(tape, g, needs=needs, dx_out=dx_out, accumulate=accumulate)


class Segment(Detect):
    """YOLOv8 segment head (reference head.py:177-200): Detect plus per-level mask-coefficient chains cv4[i] = Conv3x3, Conv3x3,
    Conv2d(c4 -> nm, 1) and a Proto on the finest level.  Train: (maps, mc [B, nm, A], p [B, nm, mh, mw]); eval:
    (cat([y, mc], 1) [B, 4+nc+nm, A] f32, (maps, mc, p)).

    mc lives in one [B, A, nm] buffer (one NHWC row per anchor): each level's final 1x1 conv result is copied into its anchor
    range, and the loss writes its gradient in the same layout.  The cv4 chains run inside the level chains that
    Detect._run_levels forks onto the branch streams; the Proto runs on the compute stream."""

    def __init__(self, nc=80, nm=32, npr=256, ch=()):
        super().__init__(nc, ch)
        self.nm = nm
        self.npr = npr
        self.proto = Proto(ch[0], self.npr, self.nm)
        self.detect = Detect.forward
        self.cv4 = self._chains(ch, max(ch[0] // 4, self.nm), self.nm)

    @staticmethod
    def _offsets(ts):
        offs, o = [], 0
        for t in ts:
            offs.append(o)
            o += t.shape[2] * t.shape[3]
        return offs, o

    def _seg_level_fwd(self, tape, i, x, mc, off):
        y = self._chain_fwd(tape, self.cv4[i], x)
        B, _, H, W = y.shape
        mc[:, off:off + H * W].view(B, H, W, self.nm).copy_(y.permute(0, 2, 3, 1))
        return self._level_fwd(tape, i, x)            # Detect's branches: their contexts sit on top of the tape

    def _seg_level_bwd(self, tape, i, g, dmc, off):
        dx = self._level_bwd(tape, i, g)
        B, _, H, W = g.shape
        gl = empty_nhwc(B, self.nm, H, W, g.dtype, g.device)
        gl.permute(0, 2, 3, 1).view(B, H * W, self.nm).copy_(dmc[:, off:off + H * W])   # .view: raises if gl were not dense
        return self._chain_bwd(tape, self.cv4[i], gl, dx)

    def _fwd(self, tape, *xs):
        if self.nm % ops.vec_elems(xs[0].dtype):
            raise NotImplementedError("Segment: nm must be a multiple of the vector width")
        B, dev, dt = xs[0].shape[0], xs[0].device, xs[0].dtype
        offs, A = self._offsets(xs)
        mc = torch.empty((B, A, self.nm), dtype=dt, device=dev)
        ptape = Tape() if tape is not None else None
        p = self.proto._fwd(ptape, xs[0])
        subs = [Tape() if tape is not None else None for _ in xs]
        maps = self._run_levels(lambda t, i, x: self._seg_level_fwd(t, i, x, mc, offs[i]), subs, list(xs))
        if tape is not None:
            tape.push((subs, ptape))
        mc4 = mc.permute(0, 2, 1).unsqueeze(2)         # [B, nm, 1, A]: a 4-d NHWC view (pixel stride nm) for the graph plumbing
        if self.training:
            return [*maps, mc4, p]
        return (self._decode(maps), *maps, mc4, p)

    def _wrap(self, out):
        n = self.nl
        if self.training:
            return list(out[:n]), out[n].squeeze(2), out[n + 1]
        mc = out[1 + n].squeeze(2)
        return torch.cat([out[0], mc.float()], 1), (list(out[1:1 + n]), mc, out[2 + n])

    def _bwd(self, tape, *gs, needs=None):
        self._require_training()
        n = self.nl
        subs, ptape = tape.pop()
        dmc = gs[n].squeeze(2).permute(0, 2, 1)        # [B, A, nm]
        offs, _ = self._offsets(gs[:n])
        dxs = self._run_levels(lambda t, i, g: self._seg_level_bwd(t, i, g, dmc, offs[i]), subs, list(gs[:n]))
        self.proto._bwd(ptape, gs[n + 1], dx_out=dxs[0], accumulate=True)
        self._fold_tapes(tape, subs + [ptape])
        return dxs


class Pose(Detect):
    """YOLOv8 pose head (reference head.py:203-241): Detect plus per-level keypoint chains cv4[i] = Conv3x3, Conv3x3,
    Conv2d(c4 -> nk, 1) with nk = K * ndim and c4 = max(ch[0] // 4, nk).  Train: (maps, kpt); eval: (y [B, 4+nc+nk, A] f32 with
    the keypoint rows decoded, (maps, kpt)).

    kpt is the list of the per-level cv4 outputs, NHWC [B, nk, h, w] with the pixel stride rounded up to the vector width
    (pad lanes zero): the loss and decode kernels (csrc/pose.hip) read them in place, anchors numbered level by level, and the
    loss writes each level's gradient map in the same layout -- no [B, nk, A] concatenation either way.  The cv4 chains run
    inside the level chains that Detect._run_levels forks onto the branch streams."""

    def __init__(self, nc=80, kpt_shape=(17, 3), ch=()):
        super().__init__(nc, ch)
        self.kpt_shape = kpt_shape
        self.nk = kpt_shape[0] * kpt_shape[1]
        self.detect = Detect.forward
        self.cv4 = self._chains(ch, max(ch[0] // 4, self.nk), self.nk)

    def _pose_level_fwd(self, tape, i, x):
        k = self._chain_fwd(tape, self.cv4[i], x)
        return self._level_fwd(tape, i, x), k          # Detect's branches: their contexts sit on top of the tape

    def _pose_level_bwd(self, tape, i, g, gk):
        gk.record_stream(torch.cuda.current_stream(gk.device))   # may be a branch stream: as Detect._run_levels does for g
        dx = self._level_bwd(tape, i, g)
        return self._chain_bwd(tape, self.cv4[i], gk, dx)

    def _fwd(self, tape, *xs):
        subs = [Tape() if tape is not None else None for _ in xs]
        outs = self._run_levels(self._pose_level_fwd, subs, list(xs))
        if tape is not None:
            tape.push(subs)
        maps, kpts = [o[0] for o in outs], [o[1] for o in outs]
        if self.training:
            return [*maps, *kpts]
        B, dev = maps[0].shape[0], maps[0].device
        strides = self.strides_as_floats()
        A = sum(t.shape[2] * t.shape[3] for t in maps)
        rows = 4 + self.nc + self.nk
        y = torch.empty((B, rows, A), dtype=torch.float32, device=dev)
        m = ops.det_maps(maps, strides, self.nc)
        call("dy_detect_decode_rows", C.byref(m), ptr(y), rows, stream())
        d = ops.pose_desc(kpts, strides, self.kpt_shape)
        call("dy_pose_kpt_decode", C.byref(d), self.nc, ptr(y), stream())
        return (y, *maps, *kpts)

    def _wrap(self, out):
        n = self.nl
        if self.training:
            return list(out[:n]), list(out[n:2 * n])
        return out[0], (list(out[1:1 + n]), list(out[1 + n:1 + 2 * n]))

    def _bwd(self, tape, *gs, needs=None):
        self._require_training()
        n = self.nl
        subs = tape.pop()
        gk = gs[n:2 * n]
        dxs = self._run_levels(lambda t, i, g: self._pose_level_bwd(t, i, g, gk[i]), subs, list(gs[:n]))
        self._fold_tapes(tape, subs)
        return dxs


class _RowsFn(torch.autograd.Function):
    """NHWC logits [B, n, 1, 1] -> the [B, n] view the caller sees, and the [B, n] gradient (rows of the padded buffer
    dy_cls_xent_bwd wrote) back to an NHWC view: both directions are views, nothing is compacted or copied."""

    @staticmethod
    def forward(ctx, z):
        ctx.ve = ops.vec_elems(z.dtype)
        return ops.rows_2d(z)

    @staticmethod
    def backward(ctx, g):
        g4 = ops.rows_4d(g, ctx.ve)
        if g4 is None:                          # a gradient that did not come from the criterion: pad it on the way in
            B, n = g.shape
            buf = torch.zeros((B, ops.round_up(n, ctx.ve)), dtype=g.dtype, device=g.device)
            buf[:, :n] = g
            g4 = ops.rows_4d(buf[:, :n], ctx.ve)
        return g4


class Classify(DyModule):
    """YOLOv8 classification head (reference head.py:244-260): Conv(c1, 1280, k, s) -> AdaptiveAvgPool2d(1) -> Dropout(0.0) ->
    Linear(1280, c2).  Train: logits [B, c2] in the compute dtype (rows of a buffer padded to the vector width); eval: softmax(1),
    f32 [B, c2].  The pool is dy_gap_fwd / dy_gap_bwd, the Linear runs as a 1x1 conv with bias on the pooled [B, 1280, 1, 1] map
    and the soft-max is dy_cls_softmax.  `pool` and `drop` are containers only (the checkpoint writer names them); p > 0 has no
    kernel (torch's Philox stream cannot be matched) and raises."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1):
        super().__init__()
        c_ = 1280
        self.conv = Conv(c1, c_, k, s, p, g)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.drop = nn.Dropout(p=0.0, inplace=True)
        self.linear = nn.Linear(c_, c2)

    def _fwd(self, tape, x, *more):
        if more:
            raise NotImplementedError("Classify: a list of input layers (torch.cat in the reference) is outside the hot path")
        if self.drop.p:
            raise NotImplementedError("Classify: dropout > 0 is not implemented (torch's Philox order cannot be matched)")
        y = self.conv._fwd(tape, x)
        pooled = ops.gap_fwd(y)
        if tape is not None:
            tape.push((y.shape[2], y.shape[3]))
        z = _linear(tape, pooled, self.linear.weight, self.linear.bias)
        return z if self.training else ops.cls_softmax(z)

    def _wrap(self, out):
        if out.dim() != 4:
            return out
        return _RowsFn.apply(out) if out.requires_grad else ops.rows_2d(out)

    def _bwd(self, tape, dz, needs=(True,)):
        if not self.training:
            raise RuntimeError("Classify: backward through the eval soft-max is not supported")
        dp = conv_backward(tape, dz)
        H, W = tape.pop()
        return self.conv._bwd(tape, ops.gap_bwd(dp, H, W), needs=needs)

# ------------------------------------------------------------------------------------------------ low-light front-end
class ConvBlock(nn.Module):
    """Parameter container of the extractor's conv + LeakyReLU(0.1) block (reference ultralytics/nn/modules/common.py:9-23)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, downsample=False, bn=False, activate=True):
        super().__init__()
        if bn:
            raise NotImplementedError("the front-end extractor uses bn=False")
        layers = [nn.Conv2d(in_channels, out_channels, kernel_size, 2 if downsample else 1, (kernel_size - 1) // 2)]
        if activate:
            layers.append(nn.LeakyReLU(0.1, inplace=False))
        self.conv_block = nn.Sequential(*layers)


_EXTRACTOR_F32 = os.environ.get("DY_EXTRACTOR_F32") is not None


class ExtractParameters2(nn.Module):
    """CNN parameter regressor (reference common.py:52-78): 5 x (conv3x3 s2 + LeakyReLU) 256^2 -> 8^2, fc 2048-64-15."""

    def __init__(self, cfg=None):
        super().__init__()
        self.output_dim = 15
        self.channels = 16
        c = self.channels
        self.conv_layers = nn.Sequential(ConvBlock(3, c, downsample=True), ConvBlock(c, 2 * c, downsample=True),
                                         ConvBlock(2 * c, 2 * c, downsample=True), ConvBlock(2 * c, 2 * c, downsample=True),
                                         ConvBlock(2 * c, 2 * c, downsample=True))
        self.fc1 = nn.Linear(2048, 64)
        self.fc2 = nn.Linear(64, self.output_dim)


# the reference filters' short names (filtersB.py: DeDarkFilter, ImprovedWhiteBalanceFilter, GammaFilter, ToneFilter, ContrastFilter,
# UsmFilter) and the chain filter_cfg.py:75 builds
FILTER_NAMES = ("DF", "W", "G", "T", "Ct", "UF")
DEFAULT_FILTERS = ("DF", "W", "G", "Ct", "UF")
_FILTER_CODES = dict(DF=1, W=2, G=3, T=4, Ct=5)           # DY_FILTER_* of include/dedark_yolo.h


def check_filters(filters):
    """A chain as the tuple of short names lowlight_recovery runs: None -> DEFAULT_FILTERS; an empty chain, an unknown or a repeated
    name raise ValueError; UF anywhere but last raises NotImplementedError (the blur needs the finished image)."""
    if filters is None:
        return DEFAULT_FILTERS
    if isinstance(filters, str) or not isinstance(filters, (list, tuple)):
        raise ValueError(f"filters: expected a list of filter names out of {list(FILTER_NAMES)}, got {filters!r}")
    names = tuple(filters)
    if not names:
        raise ValueError("filters: the chain is empty")
    for k, n in enumerate(names):
        if n not in FILTER_NAMES:
            raise ValueError(f"filters: unknown filter {n!r} at position {k} (known: {list(FILTER_NAMES)})")
        if n in names[:k]:
            raise ValueError(f"filters: {n!r} is repeated at position {k}")
    if "UF" in names and names.index("UF") != len(names) - 1:
        raise NotImplementedError(f"filters: 'UF' at position {names.index('UF')} of {list(names)}: UsmFilter is only implemented as the last filter")
    return names


def chain_word(names):
    """the pointwise filters of a chain as dy_filter_chain_fwd/bwd take them: one code per 4 bits, first stage lowest"""
    w = 0
    for k, n in enumerate(names):
        w |= _FILTER_CODES[n] << (4 * k)
    return w


class lowlight_recovery(DyModule):
    """Image-adaptive enhancement front-end (reference ultralytics/nn/modules/llie.py:11-54).

    forward(x [B,3,H,W] fp32, dedark_A [B,3] | None, IcA [B,1,H,W] | None) -> enhanced image [B,3,H,W] (a 3-channel view of an
    NHWC8 buffer in the compute dtype, consumed in place by the stem conv).  All filter math is fp32.

    `filters`: the chain as an ordered list of the reference filters' short names (the list `cfg.filters` of filter_cfg.py:65-75;
    a model yaml's top-level `filters:` key), None = DEFAULT_FILTERS.  The default chain runs the fused pair
    dy_filters_pointwise_fwd/bwd + dy_usm_*; any other chain runs dy_filter_chain_fwd/bwd (csrc/filterchain.hip) for its pointwise
    part, dy_tone_params_* when it has a ToneFilter and dy_usm_* when it ends in UF.  The filters hold no parameters: the
    state_dict does not depend on the chain.
    """
    in_dtype = torch.float32

    _planar_grad_ok = True          # _bwd takes the planar gradient written by the direct stem dgrad kernel

    def __init__(self, in_channels=3, out_channels=3, filters=None):
        super().__init__()
        self.extractor = ExtractParameters2()
        self.filter_names = check_filters(filters)

    def _adapt(self, t):
        ops.require_gpu(t)
        return t.float().contiguous()          # NCHW fp32 image

    def forward(self, x, dedark_A=None, IcA=None):
        self._A = None if dedark_A is None else dedark_A.detach().float().contiguous()
        self._I = None if IcA is None else IcA.detach().float().contiguous()
        return super().forward(x)

    def _fwd(self, tape, x):
        B, _, H, W = x.shape
        dev = x.device
        f32 = torch.float32
        A, I = getattr(self, "_A", None), getattr(self, "_I", None)
        st = stream()
        # the five stride-2 convs of the regressor run in the compute dtype (the reference's autocast covers them as well); the two
        # fully connected layers and all filter math stay fp32.  DY_EXTRACTOR_F32=1 keeps the whole regressor in fp32.
        xd = f32 if _EXTRACTOR_F32 else ops.get_compute_dtype()
        r8 = torch.empty((B, 256, 256, 8), dtype=xd, device=dev).permute(0, 3, 1, 2)
        call("dy_image_to_nhwc8", ptr(x), B, H, W, ptr(r8), 256, 256, ops.dt_id(xd), st)
        t = r8[:, :3]
        ex = self.extractor
        for blk in ex.conv_layers:
            t = plain_conv_fwd(tape, blk.conv_block[0], t, act=ACT_LEAKY)
        if xd != f32:
            t = as_nhwc(t, f32)                          # [B,32,8,8]: 64 K values
        w1 = ops.weight_view(ex.fc1.weight, (64, 32, 8, 8))             # fc1 as a conv whose window is the whole [32, 8, 8] input
        t = conv_forward(tape, t, w1, ex.fc1.bias, None, ACT_LEAKY, 1, 0, 1, False, owner=ex.fc1.weight)
        feat = _linear(tape, t, ex.fc2.weight, ex.fc2.bias)              # [B,15,1,1], ld 16
        params = torch.empty((B, 8), dtype=f32, device=dev)
        call("dy_filter_params_fwd", ptr(feat), ld_of(feat), ptr(params), B, st)
        if self.filter_names != DEFAULT_FILTERS:
            return self._chain_fwd(tape, x, feat, params, A, I)
        s4 = torch.empty((B, 3, H, W), dtype=f32, device=dev)
        call("dy_filters_pointwise_fwd", ptr(x), ptr(params), ptr(A), ptr(I), ptr(s4), B, H, W, int(ops.get_compute_dtype() != torch.float32), st)
        cd = ops.get_compute_dtype()
        out8 = torch.empty((B, H, W, 8), dtype=cd, device=dev).permute(0, 3, 1, 2)
        hp = torch.empty((B, 3, H, W), dtype=f32, device=dev) if tape is not None else None
        call("dy_usm_fwd", ptr(s4), ptr(params), None, ptr(out8), ptr(hp), B, H, W, ops.dt_id(cd), st)
        ops.emu_round(out8)
        if tape is not None:
            tape.push(dict(x=x, feat=feat, params=params, hp=hp, A=A, I=I))
        return out8[:, :3]

    def _chain_fwd(self, tape, x, feat, params, A, I):
        """any chain but the default: [dy_tone_params_fwd] -> dy_filter_chain_fwd (the filters before UF, one pass) ->
        dy_usm_fwd, or dy_image_to_nhwc8 when the chain has no UF"""
        B, _, H, W = x.shape
        dev, f32, st, cd = x.device, torch.float32, stream(), ops.get_compute_dtype()
        names = self.filter_names
        pw = tuple(n for n in names if n != "UF")
        tone = None
        if "T" in pw:
            tone = torch.empty((B, 8), dtype=f32, device=dev)
            call("dy_tone_params_fwd", ptr(feat), ld_of(feat), ptr(tone), B, st)
        s = x
        if pw:
            s = torch.empty((B, 3, H, W), dtype=f32, device=dev)
            call("dy_filter_chain_fwd", ptr(x), ptr(params), ptr(tone), ptr(A), ptr(I), chain_word(pw), ptr(s), B, H, W, int(cd != f32), st)
        out8 = torch.empty((B, H, W, 8), dtype=cd, device=dev).permute(0, 3, 1, 2)
        hp = None
        if names[-1] == "UF":
            hp = torch.empty((B, 3, H, W), dtype=f32, device=dev) if tape is not None else None
            call("dy_usm_fwd", ptr(s), ptr(params), None, ptr(out8), ptr(hp), B, H, W, ops.dt_id(cd), st)
        else:
            call("dy_image_to_nhwc8", ptr(s), B, H, W, ptr(out8), H, W, ops.dt_id(cd), st)
        ops.emu_round(out8)
        if tape is not None:
            tape.push(dict(x=x, feat=feat, params=params, hp=hp, A=A, I=I, tone=tone))
        return out8[:, :3]

    def _bwd(self, tape, dout, needs=(False,)):
        s = tape.pop()
        x, feat, params, hp = s["x"], s["feat"], s["params"], s["hp"]
        B, _, H, W = x.shape
        dev, f32, st = x.device, torch.float32, stream()
        need_dx = bool(needs[0])
        dparams = torch.zeros((B, 8), dtype=torch.float64, device=dev)      # f64 atomics: order-free sums (frontend.hip)
        if dout.is_contiguous() and dout.shape[1] == 3:       # planar gradient from the direct stem dgrad kernel
            dld = 0
        else:
            ops.padded_channels(dout)           # raises unless dout is a zero-padded NHWC view
            dld = ld_of(dout)
        fl = ld_of(feat)
        dfeat = torch.empty((B, 1, 1, fl), dtype=f32, device=dev).permute(0, 3, 1, 2)
        if self.filter_names != DEFAULT_FILTERS:
            dx = self._chain_bwd(s, dout, dld, dparams, dfeat, need_dx)
        else:
            ds4 = torch.empty((B, 3, H, W), dtype=f32, device=dev)
            call("dy_usm_bwd", None, ptr(dout), dld, ptr(hp), ptr(params), ptr(ds4), ptr(dparams), B, H, W,
                 ops.dt_id(dout.dtype), st)
            dx = torch.empty((B, 3, H, W), dtype=f32, device=dev) if need_dx else None
            call("dy_filters_pointwise_bwd", ptr(x), ptr(params), ptr(s["A"]), ptr(s["I"]), ptr(ds4), ptr(dx), ptr(dparams), B, H, W, 0,
                 int(ops.get_compute_dtype() != torch.float32), st)
            call("dy_filter_params_bwd", ptr(feat), fl, ptr(dparams), ptr(dfeat), B, st)
        g = conv_backward(tape, dfeat[:, :15])            # fc2
        g = conv_backward(tape, g)                        # fc1
        if not _EXTRACTOR_F32 and ops.get_compute_dtype() != f32:
            g = as_nhwc(g, ops.get_compute_dtype())
        for k in reversed(range(5)):
            g = conv_backward(tape, g, need_dx=(k > 0 or need_dx))
        if need_dx:
            if g.dtype != f32:
                g = as_nhwc(g, f32)
            call("dy_resize_bwd", ptr(g), ld_of(g), B, H, W, 256, 256, ptr(dx), st)
        return dx

    def _chain_bwd(self, s, dout, dld, dparams, dfeat, need_dx):
        """adjoint of _chain_fwd up to the regressed features: dy_usm_bwd (chains ending in UF; its f32 planar result feeds
        dy_filter_chain_bwd) or dy_filter_chain_bwd straight on the stem's gradient in either of its layouts; then
        dy_filter_params_bwd and, after it, dy_tone_params_bwd into columns 5..12 of the same rows.  Returns dx (None unless needed)."""
        x, feat, params, tone = s["x"], s["feat"], s["params"], s["tone"]
        B, _, H, W = x.shape
        dev, f32, st = x.device, torch.float32, stream()
        names = self.filter_names
        pw = tuple(n for n in names if n != "UF")
        fast = int(ops.get_compute_dtype() != f32)
        dtone = torch.zeros((B, 8), dtype=torch.float64, device=dev) if tone is not None else None
        dx = torch.empty((B, 3, H, W), dtype=f32, device=dev) if need_dx else None
        if names[-1] == "UF":
            ds = dx if (not pw and need_dx) else torch.empty((B, 3, H, W), dtype=f32, device=dev)
            call("dy_usm_bwd", None, ptr(dout), dld, ptr(s["hp"]), ptr(params), ptr(ds), ptr(dparams), B, H, W, ops.dt_id(dout.dtype), st)
            if pw:
                call("dy_filter_chain_bwd", ptr(x), ptr(params), ptr(tone), ptr(s["A"]), ptr(s["I"]), chain_word(pw), ptr(ds), None, 0, 0,
                     ptr(dx), ptr(dparams), ptr(dtone), B, H, W, 0, fast, st)
        else:
            call("dy_filter_chain_bwd", ptr(x), ptr(params), ptr(tone), ptr(s["A"]), ptr(s["I"]), chain_word(pw), None, ptr(dout), dld,
                 ops.dt_id(dout.dtype), ptr(dx), ptr(dparams), ptr(dtone), B, H, W, 0, fast, st)
        fl = ld_of(feat)
        call("dy_filter_params_bwd", ptr(feat), fl, ptr(dparams), ptr(dfeat), B, st)
        if tone is not None:
            call("dy_tone_params_bwd", ptr(feat), fl, ptr(dtone), ptr(dfeat), B, st)
        return dx
