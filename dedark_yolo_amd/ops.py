"""Host-side operator layer: tensors -> C-ABI calls (libdedark_yolo.so).  PyTorch is plumbing only (device memory, streams).

Tensor convention between modules: logical shape [B, C, H, W] (the reference's module interface), physical layout NHWC
(`channels_last`), dtype = compute dtype (fp32 parity path or bf16 throughput path).  A channel slice of a wider buffer is a
legal input/output ("view" = pointer + pixel stride), which is how C2f / SPPF / Detect concats cost nothing.
"""
import ctypes as C
import math
import os
import weakref

import torch

from . import _C
from ._C import ACT_LEAKY, ACT_NONE, ACT_SILU, ConvDesc, DetMaps, DetMaps4, call

_compute_dtype = torch.float32
_pack_generation = 0        # bumped whenever _pack() allocates a new packed copy
_weights_epoch = 0          # bumped by the fused optimizer (it writes parameters through raw pointers)


def set_compute_dtype(dt):
    """fp32 = the parity path (exact-f32 MFMA), bf16 = the throughput path, fp16 = the reference's AMP dtype (BASELINE configs[4];
    the trainer adds dynamic loss scaling)."""
    global _compute_dtype
    if dt not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(f"dedark_yolo_amd: unsupported compute dtype {dt}")
    _compute_dtype = dt


def get_compute_dtype():
    return _compute_dtype


_emulate_storage = None     # TEST HOOK: fp32 path with every stored activation / gradient tensor rounded to this 16-bit dtype


def set_storage_emulation(dt):
    """Test hook (tests/test_gpu_lowprec.py): with the fp32 compute dtype, round what the 16-bit paths STORE -- pre-BatchNorm conv
    outputs, activations, data gradients -- to `dt` right after the kernel that produced it, while all arithmetic stays on the
    golden-pinned fp32 kernels.  That is an ideal 16-bit-storage implementation running on the same GPU: the yardstick that
    separates kernel error from the rounding error any implementation of that storage format has.  None switches it off."""
    global _emulate_storage
    if dt not in (None, torch.bfloat16, torch.float16):
        raise ValueError("storage emulation: bf16 / fp16 / None")
    _emulate_storage = dt


def emu_round(*tensors):
    if _emulate_storage is not None:
        for t in tensors:
            if t is not None and t.dtype == torch.float32:
                t.copy_(t.to(_emulate_storage))


def bump_weights_epoch():
    global _weights_epoch
    _weights_epoch += 1


def dt_id(dtype):
    if dtype == torch.float32:
        return _C.DY_F32
    if dtype == torch.bfloat16:
        return _C.DY_BF16
    if dtype == torch.float16:
        return _C.DY_F16
    raise RuntimeError(f"dedark_yolo_amd: unsupported dtype {dtype}")


def vec_elems(dtype):
    return 4 if dtype == torch.float32 else 8


def round_up(c, m):
    return (c + m - 1) // m * m


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """hipStream_t of torch's current stream (the raw accessor: torch.cuda.current_stream() costs ~8 us per call)."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def require_gpu(t):
    if not t.is_cuda:
        raise RuntimeError("dedark_yolo_amd: the HIP path needs tensors on the GPU (there is no CPU fallback)")


def empty_nhwc(B, C_, H, W, dtype, device):
    return torch.empty((B, C_, H, W), dtype=dtype, device=device, memory_format=torch.channels_last)


def zeros_nhwc(B, C_, H, W, dtype, device):
    return torch.zeros((B, H, W, C_), dtype=dtype, device=device).permute(0, 3, 1, 2)


def ld_of(t):
    """Pixel stride (elements) of an NHWC view [B,C,H,W]; raises if `t` is not such a view."""
    B, Cc, H, W = t.shape
    sb, sc, sh, sw = t.stride()              # one call: this runs ~400 times per training step
    if Cc > 1 and sc != 1:
        raise RuntimeError(f"dedark_yolo_amd: expected an NHWC (channels_last) view, got strides {t.stride()} for {tuple(t.shape)}")
    if W > 1:
        ld = sw
    elif H > 1:
        ld = sh
    elif B > 1:
        ld = sb
    else:
        ld = Cc
    if not (ld >= Cc and (W == 1 or sw == ld) and (H == 1 or sh == W * ld) and (B == 1 or sb == H * W * ld)):
        raise RuntimeError(f"dedark_yolo_amd: not a dense NHWC view: shape {tuple(t.shape)} strides {t.stride()}")
    return ld


def is_nhwc_view(t):
    try:
        ld_of(t)
        return True
    except RuntimeError:
        return False


def as_nhwc(t, dtype=None):
    """Boundary adapter: any [B,C,H,W] tensor -> NHWC view in `dtype` (torch relayout only when the caller hands NCHW)."""
    dtype = dtype or _compute_dtype
    require_gpu(t)
    if t.dtype != dtype:
        t = t.to(dtype)
    ve = vec_elems(dtype)
    if is_nhwc_view(t) and (ld_of(t) >= round_up(t.shape[1], ve)) and (ld_of(t) * t.element_size()) % 16 == 0 \
            and t.data_ptr() % 16 == 0:
        return t          # (a narrower-than-ld view is one of our own zero-padded buffers)
    Cc = t.shape[1]
    Cp = round_up(Cc, ve)
    if Cp == Cc:
        return t.contiguous(memory_format=torch.channels_last)
    buf = torch.zeros((t.shape[0], t.shape[2], t.shape[3], Cp), dtype=dtype, device=t.device)
    buf[..., :Cc] = t.permute(0, 2, 3, 1)
    return buf.permute(0, 3, 1, 2)[:, :Cc]


def padded_channels(t):
    """Channels physically readable behind view `t` when C is not a vector multiple (pad lanes must be zero)."""
    ve = vec_elems(t.dtype)
    Cp = round_up(t.shape[1], ve)
    if Cp != t.shape[1] and ld_of(t) < Cp:
        raise RuntimeError("dedark_yolo_amd: channel count needs zero padding to a 16-byte multiple")
    return Cp


def vec_ok(t):
    """may the vectorised entries (dy_bn_act_*, dy_copy2d, the tiled convs) take view `t` as it is?  Whole 16-byte vectors: C a
    vector multiple, 16-byte aligned pointer and pixel stride.  A half of GhostConv's buffer whose width is 4 / 12 / 20 channels in a
    16-bit dtype is not; the depthwise kernels and copy_exact take it anyway."""
    return t.shape[1] % vec_elems(t.dtype) == 0 and t.data_ptr() % 16 == 0 and (ld_of(t) * t.element_size()) % 16 == 0


def copy_exact(src, dst, accumulate=False):
    """dst[:, :C] (+)= src[:, :C] touching exactly C lanes per pixel (dy_copy2d_exact), for views that are not vec_ok"""
    B, Cc, H, W = src.shape
    if tuple(dst.shape) != (B, Cc, H, W) or dst.dtype != src.dtype:
        raise RuntimeError("copy_exact: views differ in shape or dtype")
    call("dy_copy2d_exact", ptr(src), ld_of(src), ptr(dst), ld_of(dst), B * H * W, Cc, 1 if accumulate else 0, dt_id(src.dtype), stream())


# ------------------------------------------------------------------------------------------------ scratch arena
class _Arena:
    """Zero-initialised double scratch for per-channel statistics; one fill per step instead of one per conv.

    Streams: reset() runs on the compute stream at the start of a forward pass and remembers it.  A chunk that has to be added in
    the middle of a pass (the first pass, before the right size is known) may be requested from a branch stream (Detect levels,
    weight gradients): it is then allocated AND zeroed on the compute stream, every side stream is made to wait for that fill
    (dy_stream_fork), and the chunk it replaces stays alive until the next reset(), so that no kernel of another stream can see
    memory that is being filled or has gone back to the allocator."""

    def __init__(self):
        self.buf = None
        self.off = 0
        self.used = 0          # doubles handed out since the last reset
        self.chunks = 0        # buffers created since the last reset
        self.retired = []      # chunks replaced since the last reset (kept alive: other streams may still use their slices)
        self.main_raw = None   # hipStream_t of the compute stream (set by reset)

    def _new_chunk(self, cap, device):
        cur = stream()
        main_raw = self.main_raw if self.main_raw is not None else cur
        if cur == main_raw:
            buf = torch.zeros(cap, dtype=torch.float64, device=device)
        else:
            with torch.cuda.stream(torch.cuda.ExternalStream(main_raw, device=device)):
                buf = torch.zeros(cap, dtype=torch.float64, device=device)
        # every side stream that may take a slice of this chunk waits for the fill
        others = [s.cuda_stream for s in _branch["streams"]]
        if _wg_side.raw is not None:
            others.append(_wg_side.raw)
        if cur != main_raw and cur not in others:
            others.append(cur)
        for raw in others:
            call("dy_stream_fork", main_raw, raw)
        return buf

    def alloc(self, n, device):
        n = round_up(n, 2)
        self.used += n
        if self.buf is None or self.buf.device != device or self.off + n > self.buf.numel():
            cap = max(1 << 18, 4 * n)                # overflow chunk; reset() replaces the chunks by one buffer of the right size
            if self.buf is not None:
                self.retired.append(self.buf)
            self.buf = self._new_chunk(cap, device)
            self.off = 0
            self.chunks += 1
        out = self.buf[self.off:self.off + n]
        self.off += n
        return out

    def reset(self):
        self.main_raw = stream() if torch.cuda.is_available() else None
        self.retired.clear()
        if self.chunks > 1 and self.buf is not None:
            self.buf = torch.zeros(int(self.used * 1.25) + 1024, dtype=torch.float64, device=self.buf.device)
        elif self.buf is not None and self.off:
            self.buf[:self.off].zero_()
        self.off = 0
        self.used = 0
        self.chunks = 1 if self.buf is not None else 0


arena = _Arena()


# ------------------------------------------------------------------------------------------------ weights
def _w32(weight):
    w = weight.detach()
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    return w


def _pack(weight, cout_pad, cin_pad, transposed, dtype):
    key = (cout_pad, cin_pad, transposed, dtype)
    cache = weight.__dict__.setdefault("_dy_pack", {})
    hit = cache.get(key)
    tag = (_weights_epoch, weight._version)
    if hit is not None and hit[0] == tag:
        return hit[1]
    Co, Ci, KH, KW = weight.shape
    if hit is None:
        global _pack_generation
        _pack_generation += 1                  # a new packed copy exists: PackPlan must re-collect
    out = hit[1] if hit is not None else torch.empty(cout_pad * KH * KW * cin_pad, dtype=dtype, device=weight.device)
    w32 = _w32(weight)
    call("dy_pack_weight", ptr(w32), ptr(out), Co, cout_pad, Ci, cin_pad, KH, KW, 1 if transposed else 0, dt_id(dtype), stream())
    cache[key] = (tag, out)
    return out


def _packed_image(owner, slot, key, tag, numel, dtype, fill, *args):
    """The packed operand image `key` that the parameter `owner` keeps under owner.__dict__[slot]: built by fill(out, *args) at its
    first use and re-packed into the same storage whenever `tag` is not the one it was packed for (optimizer step,
    load_state_dict, an in-place update).  The hit is the per-call path of small layers: no closure, one dict lookup each."""
    cache = owner.__dict__.get(slot)
    hit = None if cache is None else cache.get(key)
    if hit is not None and hit[0] == tag:
        return hit[1]
    out = hit[1] if hit is not None else torch.empty(numel, dtype=dtype, device=owner.device)
    fill(out, *args)
    owner.__dict__.setdefault(slot, {})[key] = (tag, out)
    return out


_extra_pack_views = []      # weakrefs of persistent weight VIEWS (fully connected layers run as convs) that PackPlan re-packs too


def register_pack_view(t):
    _extra_pack_views.append(weakref.ref(t))


def weight_view(p, shape, r0=None, r1=None):
    """Parameter `p` (rows [r0, r1) of it when given) as a conv weight of the 4-D `shape`: how an nn.Linear weight reaches the conv
    kernels.  The view OBJECT is kept on the parameter, next to _dy_pack, and comes back on every call: the packed-weight cache
    lives on it, and a fresh view per step meant a re-pack launch per use and step.  It is rebuilt, and announced to PackPlan once,
    when the parameter's storage moved (model.to(), the trainer's flat state)."""
    cache = p.__dict__.setdefault("_dy_views", {})
    key = (tuple(shape), r0, r1)
    hit = cache.get(key)
    at = p.data_ptr()
    if hit is None or hit[0] != at:
        w = p.detach()
        hit = cache[key] = (at, (w if r0 is None else w[r0:r1]).view(shape))
        register_pack_view(hit[1])
    return hit[1]


class PackPlan:
    """Re-packs every cached packed weight of a model with one launch (dy_pack_weights_multi) right after the optimizer
    step wrote the f32 masters; the per-conv lazy path of _pack() then only ever hits its cache."""

    def __init__(self):
        self.sig = None
        self.table = None
        self.n_blocks = 0
        self._ent_key = None       # (id(model), _pack_generation) that _ent / _ent_sig were collected for
        self._ent = []
        self._ent_sig = ()

    def _collect(self, model):
        ent = []
        _extra_pack_views[:] = [r for r in _extra_pack_views if r() is not None]
        for w in list(model.parameters()) + [r() for r in _extra_pack_views]:
            cache = w.__dict__.get("_dy_pack")
            if not cache or w.dtype != torch.float32 or not w.is_contiguous() or w.dim() != 4:
                continue
            for key, (tag, out) in cache.items():
                ent.append((w, key, out))
        return ent

    def repack(self, model):
        # the entry list only changes when _pack() creates a new packed copy (first use of a layout) or the parameters move:
        # walking model.parameters() and rebuilding the signature cost ~1 ms of host time per step
        key = (id(model), _pack_generation)
        if key != self._ent_key:
            self._ent = self._collect(model)
            self._ent_sig = tuple((w.data_ptr(), out.data_ptr(), k) for w, k, out in self._ent)
            self._ent_key = key
        ent = self._ent
        if not ent:
            return
        sig = self._ent_sig
        if any(w.data_ptr() != sg[0] for (w, _, _), sg in zip(ent[:4], sig[:4])):      # parameters re-bound (model.to(), new flat state)
            self._ent_key = None
            return self.repack(model)
        if sig != self.sig:
            items = (_C.PackItem * len(ent))()
            blk = 0
            lib = _C.lib()
            for it, (w, (cout_pad, cin_pad, transposed, dtype), out) in zip(items, ent):
                Co, Ci, KH, KW = w.shape
                it.w, it.packed = w.data_ptr(), out.data_ptr()
                it.Cout, it.Cout_pad, it.Cin, it.Cin_pad, it.KH, it.KW = Co, cout_pad, Ci, cin_pad, KH, KW
                it.transposed, it.dtype, it.first_block = int(transposed), dt_id(dtype), blk
                blk += lib.dy_pack_item_blocks(cout_pad, cin_pad, KH, KW)
            raw = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8)
            self.table = raw.to(ent[0][0].device)
            self.n_blocks, self.sig = blk, sig
        call("dy_pack_weights_multi", ptr(self.table), len(ent), self.n_blocks, stream())
        for w, key, out in ent:
            w.__dict__["_dy_pack"][key] = ((_weights_epoch, w._version), out)


def _padded_vec(v, n):
    """f32 per-channel vector zero-padded to n (bias for padded output channels)."""
    if v is None:
        return None
    v = v.detach()
    if v.numel() == n and v.dtype == torch.float32:
        return v
    out = torch.zeros(n, dtype=torch.float32, device=v.device)
    out[:v.numel()] = v
    return out


# ------------------------------------------------------------------------------------------------ conv + bn + act
def bn_fold(bn, cout_pad):
    """scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale as a cached [2, cout_pad] f32 tensor on the
    BatchNorm module (0 / 0 on the pad channels past bn.num_features).  The fold is recomputed only when a weight or buffer changed (optimizer step, load_state_dict, a training
    forward): `BaseModel.fuse()` fills every cache up front, afterwards an eval forward launches no fold kernel at all."""
    tag = (_weights_epoch, bn.weight._version, bn.bias._version, bn.running_mean._version, bn.running_var._version,
           bn.weight.data_ptr(), bn.running_mean.data_ptr(), cout_pad)
    hit = bn.__dict__.get("_dy_fold")
    if hit is not None and hit[0] == tag:
        return hit[1]
    aff = hit[1] if (hit is not None and hit[1].shape[1] == cout_pad and hit[1].device == bn.weight.device) else \
        torch.empty((2, cout_pad), dtype=torch.float32, device=bn.weight.device)
    call("dy_bn_fold_eval_valid", ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var), float(bn.eps),
         ptr(aff[0]), ptr(aff[1]), cout_pad, bn.weight.numel(), stream())
    bn.__dict__["_dy_fold"] = (tag, aff)
    return aff


def bn_fold_is_current(bn):
    hit = bn.__dict__.get("_dy_fold")
    return hit is not None and hit[0][:7] == (_weights_epoch, bn.weight._version, bn.bias._version, bn.running_mean._version,
                                               bn.running_var._version, bn.weight.data_ptr(), bn.running_mean.data_ptr())


class ConvCtx:
    __slots__ = ("x", "z", "aff", "weight", "bias", "bn", "act", "k", "stride", "pad", "dil", "cout", "cout_pad", "cin_pad",
                 "has_bn", "y", "owner", "shared")


def _conv_desc(src, w, dst, N, Hs, Ws, Cs, Hd, Wd, Cd, KH, KW, stride, pad, dil, scale, shift, act, stats, accumulate, dtype):
    # positional construction (field order of _C.ConvDesc): ~4x cheaper than 25 attribute stores, and this runs twice per conv
    if dst is not None:
        dptr, dld = dst.data_ptr(), ld_of(dst)
    else:                                   # dgrad into a planar tensor (dst_planar is set by the caller)
        dptr, dld = None, Cd
    return ConvDesc(src.data_ptr(), ld_of(src), N, Hs, Ws, Cs, w.data_ptr(), dptr, dld, Hd, Wd, Cd, KH, KW, stride, pad, dil,
                    None if scale is None else scale.data_ptr(), None if shift is None else shift.data_ptr(), act,
                    None if stats is None else stats.data_ptr(), 1 if accumulate else 0, dt_id(dtype))


_bn_pending = {}


def flush_bn_counters():
    """num_batches_tracked is bumped lazily (one tiny kernel per BN per step would be pure launch overhead)."""
    for bn, n in _bn_pending.items():
        bn.num_batches_tracked += n
    _bn_pending.clear()


def _conv_meta(Cin, Cout, KH, KW, stride, B, H, W, pixels, note=""):
    """shape string and flops of a conv as keywords of _C.set_meta.  Formatting costs: only behind the `_C._prof is not None` guard."""
    return dict(shape=f"{Cin}->{Cout} k{KH} s{stride} in {B}x{H}x{W}{note}", flops=2.0 * pixels * Cout * KH * KW * Cin)


def _bn_train_begin(bn, C, dev):
    """Bookkeeping of one training-mode BatchNorm forward; returns the [4, C] f32 buffer `aff` (rows scale, shift, mean, invstd)
    that the finalize kernel fills and the backward pass reads."""
    _bn_pending[bn] = _bn_pending.get(bn, 0) + 1
    bn.__dict__.pop("_dy_fold", None)          # the kernels rewrite the running statistics through raw pointers
    return torch.empty((4, C), dtype=torch.float32, device=dev)


def _bn_train_tail(z, stats, bn, act, residual, y, pixels, C, C_valid, did, st):
    """y = act(bn(z)) [+ residual] from the raw conv output z and its batch sums `stats`: dy_bn_finalize_valid (batch statistics ->
    aff, running buffers) + dy_bn_act_fwd.  z / y: whole-vector NHWC views of C channels, C_valid of them real.  Returns aff."""
    aff = _bn_train_begin(bn, C, z.device)
    pa, sa = aff.data_ptr(), 4 * C
    call("dy_bn_finalize_valid", ptr(stats), pixels, ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var),
         float(bn.momentum), float(bn.eps), pa, pa + sa, pa + 2 * sa, pa + 3 * sa, C, C_valid, st)
    rp, rld = (residual.data_ptr(), ld_of(residual)) if residual is not None else (None, 0)
    _C._prof is not None and _C.set_meta(kind="bn_act_fwd", shape=f"{C}ch {y.shape[0]}x{y.shape[2]}x{y.shape[3]}", dtype=str(z.dtype), flops=0.0,
                                         bytes=float(pixels * C * z.element_size() * (3 if residual is not None else 2)))
    call("dy_bn_act_fwd", ptr(z), ld_of(z), pa, pa + sa, act, rp, rld, ptr(y), ld_of(y), pixels, C, did, st)
    emu_round(y)
    return aff


def conv_forward(tape, x, weight, bias=None, bn=None, act=ACT_NONE, stride=1, pad=0, dil=1, training=False, out=None,
                 residual=None, owner=None, shared=False):
    """y = act(bn(conv(x) [+ bias])) [+ residual].  x: NHWC view; returns an NHWC view (into `out` when given).

    Training + bn: conv kernel (raw z + batch statistics) -> finalize -> fused affine/activation/residual pass.
    Otherwise one kernel with the affine (+bias / folded BN) and activation in the epilogue.
    A context is pushed on `tape` when it is not None.
    """
    dtype = x.dtype
    B, Cin, H, W = x.shape
    Cout, Cw, KH, KW = weight.shape
    if Cw != Cin:
        raise RuntimeError(f"conv: weight expects {Cw} input channels, got {Cin}")
    ve = vec_elems(dtype)
    cin_pad = padded_channels(x)
    cout_pad = round_up(Cout, ve)
    Ho = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    wp = _pack(weight, cout_pad, cin_pad, False, dtype)
    dev = x.device
    has_bn = bn is not None
    batch_stats = has_bn and training
    ctx = None
    if tape is not None:
        ctx = ConvCtx()
        ctx.x, ctx.weight, ctx.bias, ctx.bn, ctx.act = x, weight, bias, bn, act
        ctx.owner = owner if owner is not None else weight
        ctx.shared = shared        # parameters used more than once per step (MFRU): gradients go through tape.pgrads, which adds them up
        ctx.k, ctx.stride, ctx.pad, ctx.dil = (KH, KW), stride, pad, dil
        ctx.cout, ctx.cout_pad, ctx.cin_pad, ctx.has_bn = Cout, cout_pad, cin_pad, has_bn
    if batch_stats:
        z = empty_nhwc(B, cout_pad, Ho, Wo, dtype, dev)
        stats = arena.alloc(2 * cout_pad * _C.STATS_REPLICAS, dev)
        d = _conv_desc(x, wp, z, B, H, W, cin_pad, Ho, Wo, cout_pad, KH, KW, stride, pad, dil, None, None, ACT_NONE, stats,
                       False, dtype)
        pixels = B * Ho * Wo
        y = out if out is not None else empty_nhwc(B, cout_pad, Ho, Wo, dtype, dev)
        st = stream()
        if _C._prof is None and _emulate_storage is None:
            # conv (raw z + statistics) -> finalize -> affine/activation/residual: three launches, ONE foreign call
            aff = _bn_train_begin(bn, cout_pad, dev)
            rp, rld = (residual.data_ptr(), ld_of(residual)) if residual is not None else (None, 0)
            bp = bn._parameters
            call("dy_conv2d_bn_act_fwd_valid", C.byref(d), pixels, ptr(bp["weight"]), ptr(bp["bias"]), ptr(bn.running_mean), ptr(bn.running_var),
                 float(bn.momentum), float(bn.eps), aff.data_ptr(), act, rp, rld, y.data_ptr(), ld_of(y), Cout, st)
        else:                               # per-entry timing (bench.py roofline leg, tools/layer_profile.py)
            _C._prof is not None and _C.set_meta(kind="conv_fwd", dtype=str(dtype), **_conv_meta(Cin, Cout, KH, KW, stride, B, H, W, pixels),
                                                 bytes=float((B * H * W * Cin + pixels * Cout + Cout * KH * KW * Cin) * x.element_size()))
            call("dy_conv2d_fwd", C.byref(d), st)
            emu_round(z)                    # (the statistics come from the f32 accumulators in every dtype)
            aff = _bn_train_tail(z, stats, bn, act, residual, y, pixels, cout_pad, Cout, dt_id(dtype), st)
        if ctx is not None:
            ctx.z, ctx.aff, ctx.y = z, aff, None
    else:
        if has_bn:                      # eval: running statistics folded into the conv epilogue (fuse_conv_and_bn, torch_utils.py:123-144)
            aff = bn_fold(bn, cout_pad)
            scale, shift = aff[0], aff[1]
        else:
            scale, shift = None, _padded_vec(bias, cout_pad)
        direct = residual is None
        y = out if (out is not None and direct) else empty_nhwc(B, cout_pad, Ho, Wo, dtype, dev)
        # The backward pass needs act'(conv + bias).  y gives that for no activation and for LeakyReLU (same sign), not for SiLU:
        # with a tape the conv then leaves the pre-activation in z and y = SiLU(z) is a second pass.  Every other case, and every
        # call without a tape (predict, val), stays one launch with the activation in the conv's epilogue.
        keep_z = ctx is not None and not has_bn and act == ACT_SILU
        z = empty_nhwc(B, cout_pad, Ho, Wo, dtype, dev) if keep_z else None
        d = _conv_desc(x, wp, z if keep_z else y, B, H, W, cin_pad, Ho, Wo, cout_pad, KH, KW, stride, pad, dil, scale, shift,
                       ACT_NONE if keep_z else act, None, False, dtype)
        _C._prof is not None and _C.set_meta(kind="conv_fwd", dtype=str(dtype), **_conv_meta(Cin, Cout, KH, KW, stride, B, H, W, B * Ho * Wo),
                                             bytes=float((B * H * W * Cin + B * Ho * Wo * Cout + Cout * KH * KW * Cin) * x.element_size()))
        call("dy_conv2d_fwd", C.byref(d), stream())
        if keep_z:
            emu_round(z)
            call("dy_bn_act_fwd", ptr(z), ld_of(z), None, None, act, None, 0, ptr(y), ld_of(y), B * Ho * Wo, cout_pad, dt_id(dtype), stream())
        if not direct:                  # eval-time residual: y_out = y + residual
            tgt = out if out is not None else y
            if tgt is not y:
                call("dy_copy2d", ptr(y), ld_of(y), ptr(tgt), ld_of(tgt), B * Ho * Wo, cout_pad, 0, dt_id(dtype), stream())
            call("dy_copy2d", ptr(residual), ld_of(residual), ptr(tgt), ld_of(tgt), B * Ho * Wo, cout_pad, 1, dt_id(dtype),
                 stream())
            y = tgt
        emu_round(y)
        if ctx is not None:
            if has_bn:
                raise RuntimeError("conv: gradients through an eval-mode BatchNorm are not supported")
            ctx.z, ctx.aff, ctx.y = (z, None, None) if keep_z else (None, None, y)
    if tape is not None:
        tape.push(ctx)
    return y if cout_pad == Cout else y[:, :Cout]


def _add_pgrad(tape, p, g):
    if p is None or not p.requires_grad:
        return
    if p in tape.pgrads:
        tape.pgrads[p] = tape.pgrads[p] + g
    else:
        tape.pgrads[p] = g


_wg_scratch = {}


def wgrad_scratch(device, elems=32 << 20, tag=0):
    """Reusable f32 workspace for the split-pixel partial tiles of dy_conv2d_wgrad (128 MiB; stream-ordered reuse, one per
    launch stream: `tag` = the raw stream handle.  A shared workspace was a race once the Detect levels ran on branch streams
    with gradients handed back to autograd -- their weight gradients then run on three streams at once)."""
    t = _wg_scratch.get((device, tag))
    if t is None or t.numel() < elems:
        t = torch.empty(elems, dtype=torch.float32, device=device)
        _wg_scratch[(device, tag)] = t
    return t


# ---- weight gradients on a second HIP stream.  dgrad and wgrad of a conv both depend only on dz; the next layer's backward
# depends only on the dgrad.  At the batch sizes of BASELINE configs[1] most kernels are launch-/latency-bound (20-50 us, a few
# hundred blocks), so the wgrad + its split reduction are issued on a side stream where they fill the gaps of the
# dz -> dgrad -> BN-backward chain.  Only used with direct gradient placement (the trainer's flat gradient buffer): gradients
# handed back to autograd are accumulated on the compute stream and stay there.  The operands are kept alive until the join.
class _WgradSide:
    GROUP = 8                      # operands are released in groups of this many weight gradients (one event per group)

    def __init__(self):
        self.on = False
        self.stream = None
        self.raw = None            # hipStream_t of the side stream
        self.cur = []              # operands of the group being filled
        self.groups = []           # [(event recorded on the side stream after the group's last wgrad, operands)], issue order
        self.free_events = []
        self.cb_queued = False


_wg_side = _WgradSide()


def enable_wgrad_stream(on=True):
    """Trainer switch (DY_WGRAD_STREAM=0 keeps everything on the compute stream)."""
    _wg_side.on = bool(on) and os.environ.get("DY_WGRAD_STREAM", "1") != "0"


def wgrad_stream_enabled():
    return bool(_wg_side.on)


def wgrad_side_stream(device=None):
    s = _wg_side
    if not s.on:
        return None
    if s.stream is None:
        prio = int(os.environ.get("DY_WGRAD_PRIO", "0"))       # experiments: 1 = below the compute stream where HIP offers it
        s.stream = torch.cuda.Stream(device=device, priority=prio)
        s.raw = s.stream.cuda_stream
    return s.stream


def _side_wait_main():
    """side stream waits for everything issued so far on the current (compute) stream."""
    call("dy_stream_fork", stream(), _wg_side.raw)


def _wg_track(x, dz):
    """Keeps the operands of a side-stream wgrad alive; finished groups (oldest first) are released so that their memory
    returns to the allocator during the backward pass instead of at the join."""
    s = _wg_side
    s.cur.append((x, dz))
    if len(s.cur) < s.GROUP or torch.cuda.is_current_stream_capturing():
        return
    ev = s.free_events.pop() if s.free_events else torch.cuda.Event()
    ev.record(s.stream)
    s.groups.append((ev, s.cur))
    s.cur = []
    while s.groups and s.groups[0][0].query():
        s.free_events.append(s.groups.pop(0)[0])


def wgrad_pending():
    return bool(_wg_side.cur or _wg_side.groups)


def wgrad_join():
    """The compute stream waits for the weight gradients issued so far; their operands may be freed afterwards."""
    s = _wg_side
    if s.cur or s.groups:
        call("dy_stream_fork", s.raw, stream())
        s.free_events.extend(g[0] for g in s.groups)
        s.groups.clear()
        s.cur = []
    s.cb_queued = False


# ---- independent branches on their own streams (the three pyramid levels of the Detect head, forward and backward)
_branch = {"on": False, "streams": [], "by_device": {}}      # "streams": every side stream ever made (arena fills fork to all)


def enable_branch_streams(on=True):
    """Trainer switch (DY_BRANCH_STREAMS=0 keeps the branches on the compute stream)."""
    _branch["on"] = bool(on) and os.environ.get("DY_BRANCH_STREAMS", "1") != "0"


def branch_streams(n, device):
    """n side streams for independent branches, or None when the switch is off."""
    if not _branch["on"] or n <= 0:
        return None
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    mine = _branch["by_device"].setdefault(key, [])            # a stream belongs to ONE device: one list per ordinal
    while len(mine) < n:
        s = torch.cuda.Stream(device=device)
        mine.append(s)
        _branch["streams"].append(s)
    return mine[:n]


def _grad_dst(p):
    """p.grad storage when the trainer enabled direct gradient placement (kernels write there; autograd gets None)."""
    if p is not None and p.requires_grad and getattr(p, "_dy_direct", False) and p.grad is not None:
        return p.grad
    return None


def _grad_sink(p, shape, dev, shared=False):
    """(f32 tensor a kernel writes p's gradient into, whether that is p's own .grad slot).  Direct placement needs a trainable p
    that the trainer marked (_grad_dst) and is not `shared`: a parameter used more than once per step (MFRU) goes through
    tape.pgrads, which adds the uses up.  A result that is not direct is handed over with _add_pgrad."""
    gd = None if shared else _grad_dst(p)
    if gd is not None:
        return gd, True
    return torch.empty(shape, dtype=torch.float32, device=dev), False


class _ParamRows:
    """Rows [r0, r1) of a parameter as the gradient owner (and bias) of one conv: nn.MultiheadAttention keeps its three in-projections
    in ONE in_proj_weight [3C, C] / in_proj_bias [3C], each of which runs as a 1x1 conv of its own.  The gradient sinks see an object
    with the parameter's flags and, under the trainer's direct gradient placement, the rows of its .grad: the weight / bias gradient
    kernels write them in place.  Without direct placement the results are filed under these objects on the tape and
    join_param_rows puts them together."""

    def __init__(self, p, r0, r1):
        self.p, self.r0, self.r1 = p, r0, r1
        self.shape = torch.Size((r1 - r0, *p.shape[1:]))

    requires_grad = property(lambda self: self.p.requires_grad)
    _dy_direct = property(lambda self: getattr(self.p, "_dy_direct", False))
    grad = property(lambda self: None if self.p.grad is None else self.p.grad[self.r0:self.r1])

    def detach(self):
        return self.p.detach()[self.r0:self.r1]


def join_param_rows(tape, p):
    """The row blocks filed on the tape under _ParamRows of `p` leave it and become p's gradient, concatenated in row order (they
    cover p).  Under direct placement nothing was filed and nothing happens."""
    rows = sorted((k for k in tape.pgrads if isinstance(k, _ParamRows) and k.p is p), key=lambda k: k.r0)
    if rows:
        _add_pgrad(tape, p, torch.cat([tape.pgrads.pop(k).reshape(k.shape[0], -1) for k in rows]).reshape(p.shape))


def _bn_backward(tape, dy, z, aff, bn, act, dz, pixels, C, C_valid, did, st, dev, shared):
    """dz = gradient wrt the raw conv output z of y = act(bn(z)), from dy, plus dgamma / dbeta (C_valid entries each).  dy / z /
    dz: whole-vector NHWC views of C channels.  One merged foreign call; the split reduce + apply entries while profiling."""
    sums = arena.alloc(2 * C * _C.BN_BWD_REPLICAS, dev)
    pa = aff.data_ptr()                                                     # rows of aff: scale, shift, mean, invstd
    # dgamma / dbeta go direct only when both can; otherwise both through one [2, C_valid] temporary
    gb_ = None if shared else _grad_dst(bn.bias)
    gw_, direct = _grad_sink(bn.weight, (2, C_valid), dev, gb_ is None)
    if not direct:
        gw_, gb_ = gw_[0], gw_[1]
    if _C._prof is None or _emulate_storage is not None:
        call("dy_bn_act_bwd_valid", dy.data_ptr(), ld_of(dy), z.data_ptr(), ld_of(z), pa, ptr(bn._parameters["weight"]), act,
             sums.data_ptr(), dz.data_ptr(), ld_of(dz), gw_.data_ptr(), gb_.data_ptr(), pixels, C, C_valid, did, st)
    else:
        sa, nb = 4 * C, float(pixels * C * dy.element_size())
        _C.set_meta(kind="bn_act_bwd_reduce", shape=f"{C}ch {pixels}px", dtype=str(dy.dtype), flops=0.0, bytes=nb * 2)
        call("dy_bn_act_bwd_reduce", ptr(dy), ld_of(dy), ptr(z), ld_of(z), pa, pa + sa, pa + 2 * sa, pa + 3 * sa,
             act, 1, ptr(sums), pixels, C, did, st)
        _C.set_meta(kind="bn_act_bwd_apply", shape=f"{C}ch {pixels}px", dtype=str(dy.dtype), flops=0.0, bytes=nb * 3)
        call("dy_bn_act_bwd_apply_valid", ptr(dy), ld_of(dy), ptr(z), ld_of(z), pa, pa + sa, pa + 2 * sa, pa + 3 * sa,
             ptr(bn.weight), act, 1, ptr(sums), ptr(dz), ld_of(dz), ptr(gw_), ptr(gb_), pixels, C, C_valid, did, st)
    emu_round(dz)
    if not direct:
        _add_pgrad(tape, bn.weight, gw_)
        _add_pgrad(tape, bn.bias, gb_)


def _act_backward(tape, dy, z, bias, act, dz, pixels, C, C_valid, did, st, dev, shared):
    """Backward of y = act(u), u = conv + bias, without BatchNorm: dz = dy act'(u) (the caller passes dz = dy for ACT_NONE, where
    only the bias gradient is left to compute: 0 pixels), and dbias.  z must be the pre-activation u, which the forward keeps for
    SiLU; for the sign-preserving activations (none, LeakyReLU) the stored output y gives the same act' and is passed instead.
    dy / z / dz: whole-vector NHWC views of C channels."""
    need_bias = bias is not None and bias.requires_grad
    if dz is dy and not need_bias:
        return
    sums = arena.alloc(2 * C * _C.BN_BWD_REPLICAS, dev)
    pdy, ldy, py, ly = dy.data_ptr(), ld_of(dy), z.data_ptr(), ld_of(z)
    call("dy_bn_act_bwd_reduce", pdy, ldy, py, ly, None, None, None, None, act, 0, ptr(sums), pixels, C, did, st)
    db, direct = _grad_sink(bias, C, dev, shared or C != C_valid)         # (a padded dbias never goes straight into bias.grad)
    pdz, ldz, n = (pdy, ldy, 0) if dz is dy else (dz.data_ptr(), ld_of(dz), pixels)                  # 0 pixels: only dbias
    call("dy_bn_act_bwd_apply_valid", pdy, ldy, py, ly, None, None, None, None, None, act, 0, ptr(sums), pdz, ldz, None, ptr(db),
         n, C, C_valid, did, st)
    if dz is not dy:
        emu_round(dz)
    if need_bias and not direct:
        gd = None if shared else _grad_dst(bias)
        if gd is not None:
            gd.copy_(db[:C_valid])
        else:
            _add_pgrad(tape, bias, db[:C_valid])


def conv_backward(tape, dy, need_dx=True, dx_out=None, accumulate=False, add_src=None):
    """Backward of the matching conv_forward (pops its context). dy: NHWC view of the gradient wrt the conv's output
    (for a residual conv the caller routes dy to the residual branch itself). Returns dx (NHWC view) or None.
    add_src: optional NHWC view of dx's shape added to the data gradient in the same call (dx = [dx_out +] dgrad + add_src): the
    shortcut gradient of a Bottleneck."""
    ctx = tape.pop()
    x = ctx.x
    dtype = x.dtype
    dev = x.device
    B, Cin, H, W = x.shape
    KH, KW = ctx.k
    Cout, cout_pad, cin_pad = ctx.cout, ctx.cout_pad, ctx.cin_pad
    Ho, Wo = dy.shape[2], dy.shape[3]
    if cout_pad != Cout:
        if padded_channels(dy) != cout_pad:
            raise RuntimeError("conv_backward: gradient view lacks zero padding")
    pixels = B * Ho * Wo
    did = dt_id(dtype)
    st = stream()
    if ctx.has_bn:
        dz = empty_nhwc(B, cout_pad, Ho, Wo, dtype, dev)
        _bn_backward(tape, dy, ctx.z, ctx.aff, ctx.bn, ctx.act, dz, pixels, cout_pad, Cout, did, st, dev, ctx.shared)
    else:
        dz = empty_nhwc(B, cout_pad, Ho, Wo, dtype, dev) if ctx.act != ACT_NONE else dy
        _act_backward(tape, dy, ctx.y if ctx.z is None else ctx.z, ctx.bias, ctx.act, dz, pixels, cout_pad, Cout, did, st, dev, ctx.shared)
    return _conv_grads(tape, ctx, dz, need_dx, dx_out, accumulate, add_src)


def _conv_grads(tape, ctx, dz, need_dx=True, dx_out=None, accumulate=False, add_src=None):
    """Weight gradient (side stream when the trainer enabled it) and data gradient of the convolution recorded in `ctx`, from
    dz, the gradient wrt its raw output.  The tail of conv_backward; repconv_backward runs it once per branch."""
    x = ctx.x
    dtype = x.dtype
    dev = x.device
    B, Cin, H, W = x.shape
    KH, KW = ctx.k
    Cout, cout_pad, cin_pad = ctx.cout, ctx.cout_pad, ctx.cin_pad
    Ho, Wo = dz.shape[2], dz.shape[3]
    pixels = B * Ho * Wo
    did = dt_id(dtype)
    st = stream()
    # weight gradient
    if ctx.owner.requires_grad:
        gw, direct = _grad_sink(ctx.owner, ctx.weight.shape, dev, ctx.shared)
        side = wgrad_side_stream(dev) if direct else None
        st_w = st
        if side is not None:
            if _C._prof is not None:
                _side_wait_main()                      # dz (and, for a first step, x) are ready
            if not _wg_side.cb_queued:                 # join at the end of this backward pass even without a trainer
                try:
                    torch.autograd.Variable._execution_engine.queue_callback(wgrad_join)
                    _wg_side.cb_queued = True
                except RuntimeError:
                    pass
            st_w = side.cuda_stream
        scratch = wgrad_scratch(dev, tag=st_w)         # one workspace per launch stream: Detect's levels may run their wgrads side by side
        _C._prof is not None and _C.set_meta(kind="conv_wgrad", dtype=str(dtype), **_conv_meta(Cin, Cout, KH, KW, ctx.stride, B, H, W, pixels),
                    bytes=float((B * H * W * Cin + pixels * Cout) * x.element_size() + Cout * KH * KW * Cin * 4))
        wargs = (ptr(x), ld_of(x), B, H, W, cin_pad, ptr(dz), ld_of(dz), Ho, Wo, cout_pad, KH, KW, ctx.stride, ctx.pad, ctx.dil, Cout, Cin,
                 ptr(scratch), scratch.numel(), ptr(gw), did)
        if side is not None and _C._prof is not None:
            with torch.cuda.stream(side):              # per-call timing: the events must sit on the launch stream
                call("dy_conv2d_wgrad", *wargs, st_w)
        elif side is not None:
            call("dy_conv2d_wgrad_forked", st, *wargs, st_w)        # fork from the compute stream + wgrad: one foreign call
        else:
            call("dy_conv2d_wgrad", *wargs, st_w)
        if side is not None:
            _wg_track(x, dz)
        if not direct:
            _add_pgrad(tape, ctx.owner, gw.view(ctx.owner.shape))
    if not need_dx:
        return None
    wt = _pack(ctx.weight, cout_pad, cin_pad, True, dtype)
    # network stem (3 -> c, 3x3 stride 2): the direct kernel writes dx planar [B,Cin,H,W], the layout the front-end's
    # backward consumes (6 B/pixel instead of a 16 B NHWC8 vector that is 5/8 padding)
    planar = (dx_out is None and add_src is None and dtype in (torch.bfloat16, torch.float16) and cin_pad == 8 and Cin <= 4 and (KH, KW) == (3, 3) and ctx.stride == 2
              and ctx.pad == 1 and ctx.dil == 1 and cout_pad in (16, 32, 64) and os.environ.get("DY_NO_CONV_SMALL") is None)
    if planar:
        dxp = torch.empty((B, Cin, H, W), dtype=dtype, device=dev)
        d = _conv_desc(dz, wt, None, B, Ho, Wo, cout_pad, H, W, cin_pad, KH, KW, ctx.stride, ctx.pad, ctx.dil, None, None, ACT_NONE,
                       None, False, dtype)
        d.dst_valid_channels = Cin
        d.dst_planar = dxp.data_ptr()
        _C._prof is not None and _C.set_meta(kind="conv_dgrad", dtype=str(dtype), **_conv_meta(Cin, Cout, KH, KW, ctx.stride, B, H, W, pixels, " (planar)"),
                    bytes=float((B * H * W * Cin + pixels * Cout) * x.element_size()))
        call("dy_conv2d_dgrad", C.byref(d), st)
        return dxp
    if dx_out is None:
        dxb = empty_nhwc(B, cin_pad, H, W, dtype, dev)
        accumulate = False
    else:
        dxb = dx_out
        if padded_channels(dxb) != cin_pad:
            raise RuntimeError("conv_backward: dx_out view too narrow")
    d = _conv_desc(dz, wt, dxb, B, Ho, Wo, cout_pad, H, W, cin_pad, KH, KW, ctx.stride, ctx.pad, ctx.dil, None, None, ACT_NONE,
                   None, accumulate, dtype)
    d.dst_valid_channels = Cin
    if add_src is not None:
        if tuple(add_src.shape) != (B, Cin, H, W) or add_src.dtype != dtype or padded_channels(add_src) != cin_pad:
            raise RuntimeError("conv_backward: add_src must be an NHWC view of dx's shape and dtype")
        d.add_src, d.add_src_ld = add_src.data_ptr(), ld_of(add_src)
    _C._prof is not None and _C.set_meta(kind="conv_dgrad", dtype=str(dtype), **_conv_meta(Cin, Cout, KH, KW, ctx.stride, B, H, W, pixels),
                bytes=float((B * H * W * Cin * (2 if accumulate else 1) + pixels * Cout + Cout * KH * KW * Cin) * x.element_size()))
    call("dy_conv2d_dgrad", C.byref(d), st)
    emu_round(dxb)
    if dx_out is not None:
        return dx_out
    return dxb if cin_pad == Cin else dxb[:, :Cin]


# ------------------------------------------------------------------------------------------------ RepConv
def conv_bn_stats_forward(x, weight, bn, stride=1, pad=0, dil=1, owner=None):
    """A training-mode convolution up to and including dy_bn_finalize_valid: the raw output z, its batch sums from the conv
    kernel's f32 accumulators, the running-buffer update, num_batches_tracked and the saved mean / invstd, but NOT the normalise
    pass.  Returns (z, aff, ctx): aff = [4, C] f32 rows scale, shift, mean, invstd; ctx = the ConvCtx _conv_grads takes (it is
    not pushed on a tape)."""
    dtype = x.dtype
    B, Cin, H, W = x.shape
    Cout, Cw, KH, KW = weight.shape
    if Cw != Cin:
        raise RuntimeError(f"conv: weight expects {Cw} input channels, got {Cin}")
    ve = vec_elems(dtype)
    cin_pad = padded_channels(x)
    cout_pad = round_up(Cout, ve)
    Ho = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    dev = x.device
    wp = _pack(weight, cout_pad, cin_pad, False, dtype)
    z = empty_nhwc(B, cout_pad, Ho, Wo, dtype, dev)
    stats = arena.alloc(2 * cout_pad * _C.STATS_REPLICAS, dev)
    d = _conv_desc(x, wp, z, B, H, W, cin_pad, Ho, Wo, cout_pad, KH, KW, stride, pad, dil, None, None, ACT_NONE, stats, False, dtype)
    pixels = B * Ho * Wo
    st = stream()
    _C._prof is not None and _C.set_meta(kind="conv_fwd", dtype=str(dtype), **_conv_meta(Cin, Cout, KH, KW, stride, B, H, W, pixels),
                                         bytes=float((B * H * W * Cin + pixels * Cout + Cout * KH * KW * Cin) * x.element_size()))
    call("dy_conv2d_fwd", C.byref(d), st)
    emu_round(z)
    aff = _bn_train_begin(bn, cout_pad, dev)
    pa, sa = aff.data_ptr(), 4 * cout_pad
    call("dy_bn_finalize_valid", ptr(stats), pixels, ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var),
         float(bn.momentum), float(bn.eps), pa, pa + sa, pa + 2 * sa, pa + 3 * sa, cout_pad, Cout, st)
    ctx = ConvCtx()
    ctx.x, ctx.weight, ctx.bias, ctx.bn, ctx.act = x, weight, None, bn, ACT_NONE
    ctx.owner, ctx.shared = owner if owner is not None else weight, False
    ctx.k, ctx.stride, ctx.pad, ctx.dil = (KH, KW), stride, pad, dil
    ctx.cout, ctx.cout_pad, ctx.cin_pad, ctx.has_bn = Cout, cout_pad, cin_pad, True
    ctx.z, ctx.aff, ctx.y = z, aff, None
    return z, aff, ctx


def bn2_act_bwd_workspace(pixels, C_, dtype):
    """floats of workspace dy_bn2_act_bwd needs for this shape"""
    return int(_C.lib().dy_bn2_act_bwd_workspace(pixels, C_, dt_id(dtype)))


def repconv_forward(tape, x, conv1, conv2, act, training, out=None):
    """y = act(bn1(conv1(x)) + bn2(conv2(x))) of RepConv (reference conv.py:215-218); conv1 / conv2: the two Conv modules (3x3 and
    1x1, act=False).  Training: the two raw convolutions on the usual routes with their batch statistics, then ONE
    dy_bn2_act_fwd.  Eval: the same kernel with the two eval folds.  A context is pushed on `tape` when it is not None."""
    dtype = x.dtype
    B, Cin, H, W = x.shape
    Cout = conv1.conv.weight.shape[0]
    if Cout % vec_elems(dtype) or Cin % vec_elems(dtype):
        raise NotImplementedError(f"RepConv: {Cin} -> {Cout} channels are not whole 16-byte vectors in {dtype}")
    uv = []
    for m in (conv1, conv2):
        c = m.conv
        if training:
            uv.append(conv_bn_stats_forward(x, c.weight, m.bn, c.stride[0], c.padding[0], c.dilation[0]))
        else:
            if tape is not None:
                raise RuntimeError("repconv: gradients through an eval-mode BatchNorm are not supported")
            z = conv_forward(None, x, c.weight, None, None, ACT_NONE, c.stride[0], c.padding[0], c.dilation[0])
            uv.append((z, bn_fold(m.bn, Cout), None))
    (u, au, cu), (v, av, cv) = uv
    if u.shape != v.shape:
        raise RuntimeError(f"repconv: the branches disagree in shape, {tuple(u.shape)} and {tuple(v.shape)}")
    y = out if out is not None else empty_nhwc(B, Cout, u.shape[2], u.shape[3], dtype, x.device)
    pixels = B * u.shape[2] * u.shape[3]
    _C._prof is not None and _C.set_meta(kind="bn2_act_fwd", shape=f"{Cout}ch {pixels}px", dtype=str(dtype), flops=0.0,
                                         bytes=float(3 * pixels * Cout * x.element_size()))
    call("dy_bn2_act_fwd", ptr(u), ld_of(u), ptr(v), ld_of(v), ptr(au[0]), ptr(au[1]), ptr(av[0]), ptr(av[1]), act, ptr(y), ld_of(y),
         pixels, Cout, dt_id(dtype), stream())
    emu_round(y)
    if tape is not None:
        tape.push((cu, cv, act))
    return y


def repconv_backward(tape, dy, need_dx=True, dx_out=None, accumulate=False, add_src=None):
    """Backward of the matching repconv_forward (pops its context): dy_bn2_act_bwd (du, dv and the four BatchNorm parameter
    gradients), the two weight gradients, and the two data gradients into ONE buffer: the 3x3 branch honours accumulate /
    add_src / dx_out like conv_backward, the 1x1 branch adds into the same buffer.  Returns dx or None."""
    cu, cv, act = tape.pop()
    u, v = cu.z, cv.z
    B, Cc, Ho, Wo = u.shape
    dtype, dev = u.dtype, u.device
    pixels = B * Ho * Wo
    du, dv = empty_nhwc(B, Cc, Ho, Wo, dtype, dev), empty_nhwc(B, Cc, Ho, Wo, dtype, dev)
    ws = torch.empty(bn2_act_bwd_workspace(pixels, Cc, dtype), dtype=torch.float32, device=dev)
    sinks = []
    for c in (cu, cv):                      # dgamma / dbeta go direct only when both can; otherwise through one [2, C] temporary
        gb_ = _grad_dst(c.bn.bias)
        gw_, direct = _grad_sink(c.bn.weight, (2, Cc), dev, gb_ is None)
        if not direct:
            gw_, gb_ = gw_[0], gw_[1]
        sinks.append((gw_, gb_, direct))
    pu, pv, s = cu.aff.data_ptr(), cv.aff.data_ptr(), 4 * Cc
    _C._prof is not None and _C.set_meta(kind="bn2_act_bwd", shape=f"{Cc}ch {pixels}px", dtype=str(dtype), flops=0.0,
                                         bytes=float(8 * pixels * Cc * u.element_size()))
    call("dy_bn2_act_bwd", ptr(dy), ld_of(dy), ptr(u), ld_of(u), ptr(v), ld_of(v), pu, pu + s, pu + 2 * s, pu + 3 * s, ptr(cu.bn.weight),
         pv, pv + s, pv + 2 * s, pv + 3 * s, ptr(cv.bn.weight), act, ptr(du), ld_of(du), ptr(dv), ld_of(dv), ptr(sinks[0][0]),
         ptr(sinks[0][1]), ptr(sinks[1][0]), ptr(sinks[1][1]), ptr(ws), ws.numel(), pixels, Cc, dt_id(dtype), stream())
    emu_round(du, dv)
    for c, (gw_, gb_, direct) in zip((cu, cv), sinks):
        if not direct:
            _add_pgrad(tape, c.bn.weight, gw_)
            _add_pgrad(tape, c.bn.bias, gb_)
    dx = _conv_grads(tape, cu, du, need_dx, dx_out, accumulate, add_src)
    _conv_grads(tape, cv, dv, need_dx, dx, True)
    return dx


# ------------------------------------------------------------------------------------------------ PConv
def _nhwc_like(B, Cc, H, W, dtype, device):
    """[B, Cc, H, W] NHWC tensor whose vector-padding lanes (if any) are zero, so a conv may read it (padded_channels)."""
    Cp = round_up(Cc, vec_elems(dtype))
    if Cp == Cc:
        return empty_nhwc(B, Cc, H, W, dtype, device)
    return zeros_nhwc(B, Cp, H, W, dtype, device)[:, :Cc]


def _dx_dest(op, dx_out, accumulate, add_src, shape, dtype, alloc):
    """Where the data gradient of `op` goes: (dx, accumulate).  Without dx_out a fresh alloc(), which there is nothing to accumulate
    onto; dx_out and add_src are NHWC views of the input's shape and dtype."""
    for name, t in (("dx_out", dx_out), ("add_src", add_src)):
        if t is not None and (tuple(t.shape) != tuple(shape) or t.dtype != dtype):
            raise RuntimeError(f"{op}: {name} must be an NHWC view of the input's shape and dtype")
    return (alloc(), False) if dx_out is None else (dx_out, accumulate)


def _pconv_packed(weight, w32, transposed, dtype):
    """MFMA operand image of a PConv weight for the 16-bit route (dy_pconv_pack; None where the VALU route runs), cached on the
    parameter and re-packed when the weights changed (optimizer step, load_state_dict)."""
    c3 = weight.shape[0]
    if dtype == torch.float32 or c3 < 16:
        return None
    return _packed_image(weight, "_dy_pconv_pack", (bool(transposed), dtype), (_weights_epoch, weight._version, weight.data_ptr()),
                         9 * ((c3 + 31) // 32) * ((c3 + 15) // 16) * 512, dtype, _pconv_pack, w32, c3, transposed)


def _pconv_pack(out, w32, c3, transposed):
    call("dy_pconv_pack", ptr(w32), ptr(out), c3, 1 if transposed else 0, dt_id(out.dtype), stream())


def pconv_forward(tape, x, weight, out=None):
    """PConv split_cat (reference conv.py:157-190): y[:, :c3] = conv3x3(x[:, :c3]), y[:, c3:] = x[:, c3:] in one kernel.
    x / out: NHWC views of C channels (channel slices of wider buffers are fine: exactly the lanes [0, C) are touched)."""
    B, Cc, H, W = x.shape
    c3 = weight.shape[0]
    if tuple(weight.shape) != (c3, c3, 3, 3) or c3 > Cc:
        raise RuntimeError(f"pconv: weight {tuple(weight.shape)} does not fit {Cc} channels")
    y = out if out is not None else _nhwc_like(B, Cc, H, W, x.dtype, x.device)
    w32 = _w32(weight)
    es = x.element_size()
    _C._prof is not None and _C.set_meta(kind="pconv_fwd", shape=f"{c3}/{Cc} k3 in {B}x{H}x{W}", dtype=str(x.dtype),
                                         flops=2.0 * B * H * W * c3 * 9 * c3, bytes=float(2 * B * H * W * Cc * es + 9 * c3 * c3 * 4))
    wp = _pconv_packed(weight, w32, False, x.dtype)
    call("dy_pconv_fwd", ptr(x), ld_of(x), ptr(y), ld_of(y), ptr(w32), ptr(wp), B, H, W, Cc, c3, dt_id(x.dtype), stream())
    emu_round(y)
    if tape is not None:
        tape.push((x, weight))
    return y


def pconv_backward(tape, dy, dx_out=None, accumulate=False, add_src=None):
    """Backward of the matching pconv_forward (pops its context): weight gradient (deterministic, f32) and
    dx = [dx_out +] split/cat adjoint of dy [+ add_src], one launch each.  Returns dx."""
    x, weight = tape.pop()
    B, Cc, H, W = x.shape
    c3 = weight.shape[0]
    dtype, dev, st = x.dtype, x.device, stream()
    es = x.element_size()
    if tuple(dy.shape) != (B, Cc, H, W) or dy.dtype != dtype:
        raise RuntimeError("pconv_backward: gradient does not match the forward's output")
    if weight.requires_grad:
        gw, direct = _grad_sink(weight, weight.shape, dev)
        scratch = wgrad_scratch(dev, tag=st)
        _C._prof is not None and _C.set_meta(kind="pconv_wgrad", shape=f"{c3}/{Cc} k3 in {B}x{H}x{W}", dtype=str(dtype),
                                             flops=2.0 * B * H * W * c3 * 9 * c3, bytes=float(2 * B * H * W * c3 * es + 9 * c3 * c3 * 4))
        call("dy_pconv_wgrad", ptr(x), ld_of(x), ptr(dy), ld_of(dy), ptr(gw), B, H, W, c3, ptr(scratch), scratch.numel(), dt_id(dtype), st)
        if not direct:
            _add_pgrad(tape, weight, gw)
    dx, accumulate = _dx_dest("pconv_backward", dx_out, accumulate, add_src, (B, Cc, H, W), dtype,
                              lambda: _nhwc_like(B, Cc, H, W, dtype, dev))
    w32 = _w32(weight)
    n_rw = 2 + (1 if accumulate else 0) + (1 if add_src is not None else 0)
    _C._prof is not None and _C.set_meta(kind="pconv_dgrad", shape=f"{c3}/{Cc} k3 in {B}x{H}x{W}", dtype=str(dtype),
                                         flops=2.0 * B * H * W * c3 * 9 * c3, bytes=float(n_rw * B * H * W * Cc * es + 9 * c3 * c3 * 4))
    wp = _pconv_packed(weight, w32, True, dtype)
    call("dy_pconv_dgrad", ptr(dy), ld_of(dy), ptr(dx), ld_of(dx), ptr(w32), ptr(wp), B, H, W, Cc, c3, 1 if accumulate else 0,
         ptr(add_src), 0 if add_src is None else ld_of(add_src), dt_id(dtype), st)
    emu_round(dx)
    return dx


# ------------------------------------------------------------------------------------------------ CRU convolutions
def _cru_packed(w3, w1, G, transposed, dtype):
    """MFMA operand image of a CRU conv's weights (dy_cru_conv_pack), cached on the 1x1 weight and re-packed when either weight
    changed (optimizer step, load_state_dict)."""
    GN, C1 = w1.shape[0], w1.shape[1]
    C3 = 0 if w3 is None else w3.shape[1]
    tag = (_weights_epoch, w1._version, w1.data_ptr(), None if w3 is None else (w3._version, w3.data_ptr()))
    return _packed_image(w1, "_dy_cru_pack", (bool(transposed), dtype), tag, GN * (9 * C3 + C1), dtype, _cru_pack, w3, w1, G, transposed)


def _cru_pack(out, w3, w1, G, transposed):
    GN, C1 = w1.shape[0], w1.shape[1]
    call("dy_cru_conv_pack", None if w3 is None else ptr(_w32(w3)), ptr(_w32(w1)), ptr(out), G, GN // G, 0 if w3 is None else w3.shape[1], C1,
         1 if transposed else 0, dt_id(out.dtype), stream())


def _cru_dims(x, w3, bias, w1, G):
    GN, C1 = w1.shape[0], w1.shape[1]
    C3 = 0 if w3 is None else w3.shape[1]
    if (tuple(w1.shape[2:]) != (1, 1) or GN % G or x.shape[1] != C1 or (bias is not None and tuple(bias.shape) != (GN,))
            or (w3 is not None and (tuple(w3.shape) != (GN, C3, 3, 3) or G * C3 != C1)) or (w3 is None and G != 1)):
        raise RuntimeError(f"cru_conv: weights {None if w3 is None else tuple(w3.shape)} / {tuple(w1.shape)} in {G} groups do not fit "
                           f"{x.shape[1]} channels")
    return GN // G, C3, C1


def cru_conv_forward(tape, x, w3, bias, w1, G=1, out=None):
    """One CRU convolution (dy_cru_conv_fwd): out = conv3x3(x, w3, groups=G, pad 1) + bias + conv1x1(x, w1) in one accumulator, or
    the plain 1x1 when w3 is None.  x / out: NHWC views of exactly w1.shape[1] / w1.shape[0] channels, any channel offset inside a
    wider buffer (only those lanes are touched)."""
    B, _, H, W = x.shape
    N, C3, C1 = _cru_dims(x, w3, bias, w1, G)
    y = out if out is not None else empty_nhwc(B, G * N, H, W, x.dtype, x.device)
    if tuple(y.shape) != (B, G * N, H, W) or y.dtype != x.dtype:
        raise RuntimeError("cru_conv_forward: out must be an NHWC view of the result's shape and dtype")
    wp = _cru_packed(w3, w1, G, False, x.dtype)
    es = x.element_size()
    _C._prof is not None and _C.set_meta(kind="cru_fwd", shape=f"{G}x{N} <- 9x{C3}+{C1} in {B}x{H}x{W}", dtype=str(x.dtype),
                                         flops=2.0 * B * H * W * G * N * (9 * C3 + C1), bytes=float(B * H * W * (C1 + G * N) * es))
    call("dy_cru_conv_fwd", ptr(x), ld_of(x), ptr(wp), None if bias is None else ptr(_w32(bias)), ptr(y), ld_of(y), B, H, W, G, N, C3, C1,
         dt_id(x.dtype), stream())
    emu_round(y)
    if tape is not None:
        tape.push((x, w3, bias, w1, G))
    return y


def cru_conv_backward(tape, dy, need_dx=True, dx_out=None, accumulate=False):
    """Backward of the matching cru_conv_forward (pops its context): the weight / bias gradients (deterministic, f32) are filed on
    the tape (_add_pgrad: a parameter used twice per step adds up) and dx = [dx_out +] the gather-form data gradient."""
    x, w3, bias, w1, G = tape.pop()
    B, _, H, W = x.shape
    N, C3, C1 = _cru_dims(x, w3, bias, w1, G)
    dtype, dev, st = x.dtype, x.device, stream()
    es = x.element_size()
    if tuple(dy.shape) != (B, G * N, H, W) or dy.dtype != dtype:
        raise RuntimeError("cru_conv_backward: gradient does not match the forward's output")
    want = [p is not None and p.requires_grad for p in (w3, bias, w1)]
    if any(want):
        g3 = torch.empty(w3.shape, dtype=torch.float32, device=dev) if want[0] else None
        gb = torch.empty(bias.shape, dtype=torch.float32, device=dev) if want[1] else None
        g1 = torch.empty(w1.shape, dtype=torch.float32, device=dev) if want[2] else None
        scratch = wgrad_scratch(dev, tag=st)
        _C._prof is not None and _C.set_meta(kind="cru_wgrad", shape=f"{G}x{N} <- 9x{C3}+{C1} in {B}x{H}x{W}", dtype=str(dtype),
                                             flops=2.0 * B * H * W * G * N * (9 * C3 + C1), bytes=float(B * H * W * (C1 + G * N) * es))
        call("dy_cru_conv_wgrad", ptr(x), ld_of(x), ptr(dy), ld_of(dy), ptr(g3), ptr(gb), ptr(g1), B, H, W, G, N, C3, C1, ptr(scratch),
             scratch.numel(), dt_id(dtype), st)
        for p, g in ((w3, g3), (bias, gb), (w1, g1)):
            if g is not None:
                _add_pgrad(tape, p, g)
    if not need_dx:
        return None
    dx, accumulate = _dx_dest("cru_conv_backward", dx_out, accumulate, None, (B, C1, H, W), dtype,
                              lambda: empty_nhwc(B, C1, H, W, dtype, dev))
    wp = _cru_packed(w3, w1, G, True, dtype)
    _C._prof is not None and _C.set_meta(kind="cru_dgrad", shape=f"{G}x{N} <- 9x{C3}+{C1} in {B}x{H}x{W}", dtype=str(dtype),
                                         flops=2.0 * B * H * W * G * N * (9 * C3 + C1),
                                         bytes=float(B * H * W * ((2 if accumulate else 1) * C1 + G * N) * es))
    call("dy_cru_conv_dgrad", ptr(dy), ld_of(dy), ptr(wp), ptr(dx), ld_of(dx), B, H, W, G, N, C3, C1, 1 if accumulate else 0, dt_id(dtype), st)
    emu_round(dx)
    return dx


# ------------------------------------------------------------------------------------------------ fused attention
def _attn_dims(who, q, k, v, heads):
    B, Cc, H, W = q.shape
    if tuple(k.shape) != tuple(q.shape) or tuple(v.shape) != tuple(q.shape) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise RuntimeError(f"{who}: q, k and v must be NHWC views of one shape and dtype")
    if heads < 1 or Cc % heads:
        raise RuntimeError(f"{who}: {Cc} channels do not split into {heads} heads")
    return B, Cc, H, W, H * W, Cc // heads


def attn_forward(tape, q, k, v, heads, out=None):
    """softmax(Q K^T / sqrt(D)) V over the pixels of a map (dy_attn_fwd; reference transformer.py:115, torch's
    multi_head_attention_forward between in-projection and out_proj).  q / k / v / out: NHWC views [B, C, H, W] = token matrices
    [B, L = H W, C], normally the three channel slices of one [B, 3C, H, W] buffer; head h = channels [h D, (h + 1) D).  With a
    tape the log-sum-exp is kept for attn_backward."""
    B, Cc, H, W, L, D = _attn_dims("attn_forward", q, k, v, heads)
    o = out if out is not None else empty_nhwc(B, Cc, H, W, q.dtype, q.device)
    if tuple(o.shape) != (B, Cc, H, W) or o.dtype != q.dtype:
        raise RuntimeError("attn_forward: out must be an NHWC view of q's shape and dtype")
    lse = torch.empty(B * heads * L, dtype=torch.float32, device=q.device) if tape is not None else None
    _C._prof is not None and _C.set_meta(kind="attn_fwd", shape=f"{heads}x{D} L={L} B={B}", dtype=str(q.dtype), flops=4.0 * B * heads * L * L * D,
                                         bytes=float(4 * B * L * Cc * q.element_size()))
    call("dy_attn_fwd", ptr(q), ld_of(q), ptr(k), ld_of(k), ptr(v), ld_of(v), ptr(o), ld_of(o), ptr(lse), B, L, heads, D, D ** -0.5,
         dt_id(q.dtype), stream())
    emu_round(o)
    if tape is not None:
        tape.push((q, k, v, o, lse, heads))
    return o


def attn_backward(tape, dy, out=None):
    """Backward of the matching attn_forward (pops its context; dy_attn_bwd, deterministic).  Returns the [B, 3C, H, W] NHWC buffer
    dQ | dK | dV (`out` when given): the in-projections' data gradients read its three slices in place."""
    q, k, v, o, lse, heads = tape.pop()
    B, Cc, H, W, L, D = _attn_dims("attn_backward", q, k, v, heads)
    if tuple(dy.shape) != (B, Cc, H, W) or dy.dtype != q.dtype:
        raise RuntimeError("attn_backward: gradient does not match the forward's output")
    g = out if out is not None else empty_nhwc(B, 3 * Cc, H, W, q.dtype, q.device)
    if tuple(g.shape) != (B, 3 * Cc, H, W) or g.dtype != q.dtype:
        raise RuntimeError("attn_backward: out must be an NHWC view of [B, 3C, H, W] in q's dtype")
    dq, dk, dv = g[:, :Cc], g[:, Cc:2 * Cc], g[:, 2 * Cc:]
    _C._prof is not None and _C.set_meta(kind="attn_bwd", shape=f"{heads}x{D} L={L} B={B}", dtype=str(q.dtype), flops=14.0 * B * heads * L * L * D,
                                         bytes=float(8 * B * L * Cc * q.element_size()))
    call("dy_attn_bwd", ptr(q), ld_of(q), ptr(k), ld_of(k), ptr(v), ld_of(v), ptr(o), ld_of(o), ptr(dy), ld_of(dy), ptr(lse), ptr(dq), ld_of(dq),
         ptr(dk), ld_of(dk), ptr(dv), ld_of(dv), B, L, heads, D, D ** -0.5, dt_id(q.dtype), stream())
    emu_round(g)
    return g


# ------------------------------------------------------------------------------------------------ transformer encoder layer
def _same_view(who, ref, *others):
    for t in others:
        if t is not None and (tuple(t.shape) != tuple(ref.shape) or t.dtype != ref.dtype):
            raise RuntimeError(f"{who}: every operand must be an NHWC view of one shape and dtype")


def ln_parts(rows, C_):
    """workgroups (= dgamma / dbeta partials) of dy_add_layernorm_bwd, the launcher's own rule (include/dedark_yolo.h)"""
    per = 1 if C_ > 1024 else 4
    return max(1, min(_C.LN_MAX_PARTS, (rows + per - 1) // per))


def add_layernorm_forward(tape, a, b, norm, out=None):
    """y = LayerNorm(a + b) over the channels of every pixel (dy_add_layernorm_fwd; reference transformer.py:46-47, 49-50: the
    residual add and nn.LayerNorm in one pass, a + b never stored).  a / b / out: NHWC views [B, C, H, W]; b may be None.  norm: the
    nn.LayerNorm that owns weight, bias and eps.  With a tape the rows' (mean, rstd) are kept for add_layernorm_backward."""
    B, Cc, H, W = a.shape
    _same_view("add_layernorm_forward", a, b, out)
    if tuple(norm.normalized_shape) != (Cc,) or norm.weight is None or norm.bias is None:
        raise RuntimeError(f"add_layernorm_forward: the LayerNorm must be affine over the {Cc} channels")
    y = out if out is not None else empty_nhwc(B, Cc, H, W, a.dtype, a.device)
    rows = B * H * W
    stats = torch.empty(rows * 2, dtype=torch.float32, device=a.device) if tape is not None else None
    _C._prof is not None and _C.set_meta(kind="add_layernorm_fwd", shape=f"{Cc}ch {rows}px", dtype=str(a.dtype), flops=0.0,
                                         bytes=float((3 if b is not None else 2) * rows * Cc * a.element_size()))
    call("dy_add_layernorm_fwd", ptr(a), ld_of(a), ptr(b), ld_of(b) if b is not None else 0, ptr(norm.weight), ptr(norm.bias), ptr(y), ld_of(y),
         ptr(stats), rows, Cc, norm.eps, dt_id(a.dtype), stream())
    emu_round(y)
    if tape is not None:
        tape.push((a, b, stats, norm))
    return y


def add_layernorm_backward(tape, dy, dz_out=None, accumulate=False):
    """Backward of the matching add_layernorm_forward (pops its context; dy_add_layernorm_bwd, deterministic).  Returns dz, the
    gradient of a and of b alike (`dz_out` when given; accumulate: added into it); norm.weight / norm.bias get their gradients."""
    a, b, stats, norm = tape.pop()
    B, Cc, H, W = a.shape
    _same_view("add_layernorm_backward", a, dy, dz_out)
    dz = dz_out if dz_out is not None else empty_nhwc(B, Cc, H, W, a.dtype, a.device)
    rows, dev = B * H * W, a.device
    need = norm.weight.requires_grad or norm.bias.requires_grad
    gw = gb = scratch = None
    direct = False
    if need:
        gb_ = _grad_dst(norm.bias)
        gw, direct = _grad_sink(norm.weight, (2, Cc), dev, gb_ is None)       # direct only when both can (as _bn_backward)
        gw, gb = (gw, gb_) if direct else (gw[0], gw[1])
        scratch = torch.empty(ln_parts(rows, Cc) * 2 * Cc, dtype=torch.float32, device=dev)
    _C._prof is not None and _C.set_meta(kind="add_layernorm_bwd", shape=f"{Cc}ch {rows}px", dtype=str(a.dtype), flops=0.0,
                                         bytes=float((4 if b is not None else 3) * rows * Cc * a.element_size()))
    call("dy_add_layernorm_bwd", ptr(a), ld_of(a), ptr(b), ld_of(b) if b is not None else 0, ptr(stats), ptr(norm.weight), ptr(dy), ld_of(dy),
         ptr(dz), ld_of(dz), 1 if (accumulate and dz_out is not None) else 0, ptr(gw), ptr(gb), ptr(scratch),
         0 if scratch is None else scratch.numel(), rows, Cc, dt_id(a.dtype), stream())
    emu_round(dz)
    if need and not direct:
        _add_pgrad(tape, norm.weight, gw)
        _add_pgrad(tape, norm.bias, gb)
    return dz


def gelu_forward(tape, u, out=None):
    """y = 0.5 u (1 + erf(u / sqrt 2)), nn.GELU()'s default (dy_gelu_fwd; reference transformer.py:48).  With a tape the
    pre-activation u is kept for gelu_backward."""
    B, Cc, H, W = u.shape
    _same_view("gelu_forward", u, out)
    y = out if out is not None else empty_nhwc(B, Cc, H, W, u.dtype, u.device)
    _C._prof is not None and _C.set_meta(kind="gelu_fwd", shape=f"{Cc}ch {B * H * W}px", dtype=str(u.dtype), flops=0.0,
                                         bytes=float(2 * B * H * W * Cc * u.element_size()))
    call("dy_gelu_fwd", ptr(u), ld_of(u), ptr(y), ld_of(y), B * H * W, Cc, dt_id(u.dtype), stream())
    emu_round(y)
    if tape is not None:
        tape.push(u)
    return y


def gelu_backward(tape, dy, out=None):
    """du = dy (Phi(u) + u phi(u)) of the matching gelu_forward (pops its context; dy_gelu_bwd)"""
    u = tape.pop()
    B, Cc, H, W = u.shape
    _same_view("gelu_backward", u, dy, out)
    du = out if out is not None else empty_nhwc(B, Cc, H, W, u.dtype, u.device)
    _C._prof is not None and _C.set_meta(kind="gelu_bwd", shape=f"{Cc}ch {B * H * W}px", dtype=str(u.dtype), flops=0.0,
                                         bytes=float(3 * B * H * W * Cc * u.element_size()))
    call("dy_gelu_bwd", ptr(u), ld_of(u), ptr(dy), ld_of(dy), ptr(du), ld_of(du), B * H * W, Cc, dt_id(u.dtype), stream())
    emu_round(du)
    return du


def sincos_pos_table(w, h, c, temperature=10000.0):
    """The reference's AIFI.build_2d_sincos_position_embedding(w, h, c) (transformer.py:83-97) restated: f32 [w h, c] on the CPU.
    Its meshgrid is indexing='ij' over (grid_w, grid_h), so row p holds (iw, ih) = (p // h, p % h)."""
    if c % 4:
        raise ValueError("Embed dimension must be divisible by 4 for 2D sin-cos position embedding")
    gw, gh = torch.meshgrid(torch.arange(int(w), dtype=torch.float32), torch.arange(int(h), dtype=torch.float32), indexing="ij")
    pos_dim = c // 4
    omega = torch.arange(pos_dim, dtype=torch.float32) / pos_dim
    omega = 1.0 / (temperature ** omega)
    ow = gw.flatten()[..., None] @ omega[None]
    oh = gh.flatten()[..., None] @ omega[None]
    return torch.cat([torch.sin(ow), torch.cos(ow), torch.sin(oh), torch.cos(oh)], dim=1)


_pos_tables = {}


def pos_table(w, h, c, dtype, device):
    """sincos_pos_table in `dtype` on `device`, built once per (w, h, c, dtype, device)"""
    key = (int(w), int(h), int(c), dtype, str(device))
    t = _pos_tables.get(key)
    if t is None:
        t = _pos_tables[key] = sincos_pos_table(w, h, c).to(dtype).to(device).contiguous()
    return t


def add_pos(x, pos, out=None):
    """y[b, :, p] = x[b, :, p] + pos[p, :] over the pixels p of an NHWC map (dy_add_pos; reference transformer.py:41); pos: dense
    [H W, C] table of x's dtype.  The table is a constant: there is no backward."""
    B, Cc, H, W = x.shape
    _same_view("add_pos", x, out)
    if tuple(pos.shape) != (H * W, Cc) or pos.dtype != x.dtype or not pos.is_contiguous():
        raise RuntimeError("add_pos: pos must be a dense [H W, C] table of x's dtype")
    y = out if out is not None else empty_nhwc(B, Cc, H, W, x.dtype, x.device)
    _C._prof is not None and _C.set_meta(kind="add_pos", shape=f"{Cc}ch {B * H * W}px", dtype=str(x.dtype), flops=0.0,
                                         bytes=float(2 * B * H * W * Cc * x.element_size()))
    call("dy_add_pos", ptr(x), ld_of(x), ptr(pos), ptr(y), ld_of(y), B, H * W, Cc, dt_id(x.dtype), stream())
    emu_round(y)
    return y


# ------------------------------------------------------------------------------------------------ channel / spatial attention (csrc/cbam.hip)
class SpatialPlanes:
    """The per-pixel planes of one spatial-attention stage, dense f32 [B, H, W] (arg: int32): mean_c / max_c of u = x g, the argmax
    channel and s = sigmoid(cv1(mean, max)) from the forward; dmean / dmax from spatial_conv_bwd."""
    __slots__ = ("mean", "mx", "arg", "s", "dmean", "dmx")

    def __init__(self, mean, mx, arg=None, s=None):
        self.mean, self.mx, self.arg, self.s, self.dmean, self.dmx = mean, mx, arg, s, None, None


def _cbam_dims(who, x, a, *like):
    """(B, H, W, C) of the NHWC view x after the kernels' rule; `a`: the fc's logits [B, C, 1, 1] or None; `like`: views of x's shape"""
    B, Cc, H, W = x.shape
    if Cc % 8 or not 8 <= Cc <= _C.CBAM_MAX_C:
        raise NotImplementedError(f"{who}: C={Cc} is outside the attention kernels' rule C % 8 == 0, 8 <= C <= {_C.CBAM_MAX_C}")
    if a is not None and (tuple(a.shape) != (B, Cc, 1, 1) or a.dtype != x.dtype):
        raise RuntimeError(f"{who}: gate logits {tuple(a.shape)} {a.dtype} do not belong to a {tuple(x.shape)} {x.dtype} map")
    for t in like:
        if t is not None and (tuple(t.shape) != tuple(x.shape) or t.dtype != x.dtype):
            raise RuntimeError(f"{who}: views differ in shape or dtype ({tuple(t.shape)} {t.dtype} vs {tuple(x.shape)} {x.dtype})")
    return B, H, W, Cc


def _gate_args(a):
    return (None, 0) if a is None else (ptr(a), ld_of(a))


def _cbam_meta(kind, x, passes):
    B, Cc, H, W = x.shape
    _C._prof is not None and _C.set_meta(kind=kind, shape=f"{Cc}ch {B * H * W}px", dtype=str(x.dtype), flops=0.0,
                                         bytes=float(passes * B * H * W * Cc * x.element_size()))


def chan_pool_fwd(x):
    """AdaptiveAvgPool2d(1) of an NHWC view [B, C, H, W] -> NHWC [B, C, 1, 1] (dy_chan_pool_fwd; reference conv.py:299, 304): the
    pixels of an image are spread over up to 64 workgroups, partial sums added in a fixed order"""
    B, H, W, Cc = _cbam_dims("chan_pool_fwd", x, None)
    y = empty_nhwc(B, Cc, 1, 1, x.dtype, x.device)
    need = int(_C.lib().dy_cbam_reduce_workspace(B, H * W, Cc, dt_id(x.dtype)))
    ws = torch.empty(need, dtype=torch.float32, device=x.device)
    _cbam_meta("chan_pool_fwd", x, 1)
    call("dy_chan_pool_fwd", ptr(x), ld_of(x), ptr(y), ld_of(y), ptr(ws), need, B, H * W, Cc, dt_id(x.dtype), stream())
    emu_round(y)
    return y


def chan_gate_fwd(x, a, out=None):
    """y = x sigmoid(a[b]) (dy_chan_gate_fwd; reference conv.py:302-304): ChannelAttention alone"""
    B, H, W, Cc = _cbam_dims("chan_gate_fwd", x, a, out)
    y = out if out is not None else empty_nhwc(B, Cc, H, W, x.dtype, x.device)
    _cbam_meta("chan_gate_fwd", x, 2)
    call("dy_chan_gate_fwd", ptr(x), ld_of(x), ptr(a), ld_of(a), ptr(y), ld_of(y), B, H * W, Cc, dt_id(x.dtype), stream())
    emu_round(y)
    return y


def spatial_stats_fwd(x, a=None, want_arg=False):
    """mean_c / max_c (and the argmax channel, lowest index on ties) of u = x sigmoid(a[b]) in one read of x, u not stored
    (dy_spatial_stats_fwd; reference conv.py:320).  a = None: u = x."""
    B, H, W, Cc = _cbam_dims("spatial_stats_fwd", x, a)
    mean = torch.empty((2, B, H, W), dtype=torch.float32, device=x.device)
    arg = torch.empty((B, H, W), dtype=torch.int32, device=x.device) if want_arg else None
    _cbam_meta("spatial_stats_fwd", x, 1)
    call("dy_spatial_stats_fwd", ptr(x), ld_of(x), *_gate_args(a), ptr(mean[0]), ptr(mean[1]), ptr(arg), B, H * W, Cc, dt_id(x.dtype), stream())
    return SpatialPlanes(mean[0], mean[1], arg)


def spatial_gate_fwd(x, a, planes, weight, out=None, keep_s=False):
    """y = x g s, s = sigmoid(cv1(mean, max)) with zero padding k // 2 (dy_spatial_gate_fwd; reference conv.py:320, 458).  weight:
    cv1.weight [1, 2, k, k]; keep_s: s is stored in `planes` for the backward."""
    B, H, W, Cc = _cbam_dims("spatial_gate_fwd", x, a, out)
    k = weight.shape[-1]
    if tuple(weight.shape) != (1, 2, k, k):
        raise RuntimeError(f"spatial_gate_fwd: weight {tuple(weight.shape)} is not [1, 2, k, k]")
    y = out if out is not None else empty_nhwc(B, Cc, H, W, x.dtype, x.device)
    if keep_s:
        planes.s = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    _cbam_meta("spatial_gate_fwd", x, 2)
    call("dy_spatial_gate_fwd", ptr(x), ld_of(x), *_gate_args(a), ptr(planes.mean), ptr(planes.mx), ptr(_w32(weight)), k, ptr(y), ld_of(y),
         ptr(planes.s) if keep_s else None, B, H, W, Cc, dt_id(x.dtype), stream())
    emu_round(y)
    return y


def spatial_gate_bwd_px(dy, x, a, planes):
    """dpre [B, H, W] f32 = s (1 - s) sum_c dy x g (dy_spatial_gate_bwd_px)"""
    B, H, W, Cc = _cbam_dims("spatial_gate_bwd_px", x, a, dy)
    dpre = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    _cbam_meta("spatial_gate_bwd_px", x, 2)
    call("dy_spatial_gate_bwd_px", ptr(dy), ld_of(dy), ptr(x), ld_of(x), *_gate_args(a), ptr(planes.s), ptr(dpre), B, H * W, Cc,
         dt_id(x.dtype), stream())
    return dpre


def spatial_conv_bwd(tape, dpre, planes, weight):
    """Backward of cv1 on the planes (dy_spatial_conv_bwd): planes.dmean / planes.dmx = the transposed convolution of dpre, and the
    weight's gradient (deterministic) goes into its sink."""
    B, H, W = dpre.shape
    k, dev = weight.shape[-1], dpre.device
    dm = torch.empty((2, B, H, W), dtype=torch.float32, device=dev)
    planes.dmean, planes.dmx = dm[0], dm[1]
    dw, direct = _grad_sink(weight, tuple(weight.shape), dev)
    need = int(_C.lib().dy_spatial_conv_bwd_workspace(B, H, W, k))
    ws = torch.empty(need, dtype=torch.float32, device=dev)
    call("dy_spatial_conv_bwd", ptr(dpre), ptr(planes.mean), ptr(planes.mx), ptr(_w32(weight)), k, ptr(planes.dmean), ptr(planes.dmx), ptr(dw),
         ptr(ws), need, B, H, W, stream())
    if not direct:
        _add_pgrad(tape, weight, dw)


def gate_bwd_reduce(dy, x, a, planes=None):
    """da [B, C, 1, 1] = g (1 - g) sum_p du x in the compute dtype (dy_spatial_gate_bwd_reduce, deterministic); du = dy s + dmean / C +
    (c == argmax ? dmax : 0), or dy without `planes` (ChannelAttention alone)"""
    B, H, W, Cc = _cbam_dims("gate_bwd_reduce", x, a, dy)
    da = empty_nhwc(B, Cc, 1, 1, x.dtype, x.device)
    need = int(_C.lib().dy_cbam_reduce_workspace(B, H * W, Cc, dt_id(x.dtype)))
    ws = torch.empty(need, dtype=torch.float32, device=x.device)
    p = planes
    _cbam_meta("gate_bwd_reduce", x, 2)
    call("dy_spatial_gate_bwd_reduce", ptr(dy), ld_of(dy), ptr(x), ld_of(x), ptr(a), ld_of(a), *(_plane_args(p)), ptr(da), ld_of(da), ptr(ws),
         need, B, H * W, Cc, dt_id(x.dtype), stream())
    emu_round(da)
    return da


def _plane_args(p):
    return (None, None, None, None) if p is None else (ptr(p.s), ptr(p.dmean), ptr(p.dmx), ptr(p.arg))


def gate_bwd_apply(dy, a, planes=None, dpool=None, dx_out=None, accumulate=False):
    """dx = du g + dpool[b] / (H W) (+ dx_out when accumulate) (dy_spatial_gate_bwd_apply); dpool [B, C, 1, 1]: the fc's data gradient,
    i.e. the pooled branch's share; a = None: g = 1 (SpatialAttention alone)"""
    B, H, W, Cc = _cbam_dims("gate_bwd_apply", dy, a, dx_out)
    if dpool is not None and (tuple(dpool.shape) != (B, Cc, 1, 1) or dpool.dtype != dy.dtype):
        raise RuntimeError("gate_bwd_apply: dpool does not belong to the map")
    dx = dx_out if dx_out is not None else empty_nhwc(B, Cc, H, W, dy.dtype, dy.device)
    _cbam_meta("gate_bwd_apply", dy, 3 if (accumulate and dx_out is not None) else 2)
    call("dy_spatial_gate_bwd_apply", ptr(dy), ld_of(dy), *_gate_args(a), *_plane_args(planes), *_gate_args(dpool), ptr(dx), ld_of(dx),
         1 if (accumulate and dx_out is not None) else 0, B, H * W, Cc, dt_id(dy.dtype), stream())
    emu_round(dx)
    return dx


# ------------------------------------------------------------------------------------------------ depthwise conv
def dwconv_forward(tape, x, weight, bias=None, bn=None, act=ACT_NONE, stride=1, training=False, out=None):
    """y = act(bn(dwconv(x) [+ bias])) for a depthwise conv (weight [C, 1, k, k], pad k // 2), the contract of conv_forward.
    x / out: NHWC views of C channels that need not be vector multiples or aligned (exact lanes).

    Training + bn: dy_dwconv_fwd in statistics mode (raw z + batch sums) -> dy_bn_finalize_valid -> dy_bn_act_fwd.  The
    BatchNorm pass wants whole vectors: z is a vector-padded temporary (kept for the backward pass anyway), and y goes straight
    into `out` where that view is vec_ok (no extra copy), else through a padded temporary and copy_exact.
    Otherwise one launch with the affine (folded BN / bias) and the activation in the epilogue, written straight into `out`."""
    dtype, dev = x.dtype, x.device
    B, Cc, H, W = x.shape
    k = weight.shape[2]
    if tuple(weight.shape) != (Cc, 1, k, k):
        raise RuntimeError(f"dwconv: weight {tuple(weight.shape)} is not depthwise over {Cc} channels")
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if out is not None and (tuple(out.shape) != (B, Cc, Ho, Wo) or out.dtype != dtype):
        raise RuntimeError("dwconv: `out` does not match the output")
    cpad = round_up(Cc, vec_elems(dtype))
    pixels, es, did, st = B * Ho * Wo, x.element_size(), dt_id(dtype), stream()
    w32 = _w32(weight)
    has_bn = bn is not None
    ctx = None
    if tape is not None:
        ctx = ConvCtx()
        ctx.x, ctx.weight, ctx.bias, ctx.bn, ctx.act, ctx.k, ctx.stride = x, weight, bias, bn, act, k, stride
    flops, nbytes = 2.0 * pixels * Cc * k * k, float((B * H * W + pixels) * Cc * es + Cc * k * k * 4)
    shape = f"dw {Cc} k{k} s{stride} in {B}x{H}x{W}"
    if has_bn and training:
        z = _nhwc_like(B, Cc, Ho, Wo, dtype, dev)
        stats = arena.alloc(2 * cpad * _C.STATS_REPLICAS, dev)
        _C._prof is not None and _C.set_meta(kind="dwconv_fwd", shape=shape, dtype=str(dtype), flops=flops, bytes=nbytes)
        call("dy_dwconv_fwd", ptr(x), ld_of(x), ptr(z), ld_of(z), ptr(w32), B, H, W, Cc, k, stride, None, None, ACT_NONE, ptr(stats), cpad,
             did, st)
        emu_round(z)
        direct = out is not None and vec_ok(out)
        y = out if direct else _nhwc_like(B, Cc, Ho, Wo, dtype, dev)
        aff = _bn_train_tail(z, stats, bn, act, None, y, pixels, cpad, Cc, did, st)
        if out is not None and not direct:
            copy_exact(y, out)
            y = out
        if ctx is not None:
            ctx.z, ctx.aff, ctx.y = z, aff, None
    else:
        if has_bn:
            aff = bn_fold(bn, cpad)
            scale, shift = aff[0], aff[1]
        else:
            scale, shift = None, (None if bias is None else bias.detach().float())
        keep_z = ctx is not None and not has_bn and act == ACT_SILU         # conv_forward: SiLU's backward needs the pre-activation
        _C._prof is not None and _C.set_meta(kind="dwconv_fwd", shape=shape, dtype=str(dtype), flops=flops, bytes=nbytes)
        if keep_z:
            z = _nhwc_like(B, Cc, Ho, Wo, dtype, dev)
            call("dy_dwconv_fwd", ptr(x), ld_of(x), ptr(z), ld_of(z), ptr(w32), B, H, W, Cc, k, stride, ptr(scale), ptr(shift), ACT_NONE,
                 None, 0, did, st)
            emu_round(z)
            direct = out is not None and vec_ok(out)
            y = out if direct else _nhwc_like(B, Cc, Ho, Wo, dtype, dev)
            call("dy_bn_act_fwd", ptr(z), ld_of(z), None, None, act, None, 0, ptr(y), ld_of(y), pixels, cpad, did, st)
            emu_round(y)
            if out is not None and not direct:
                copy_exact(y, out)
                y = out
        else:
            z = None
            y = out if out is not None else _nhwc_like(B, Cc, Ho, Wo, dtype, dev)
            call("dy_dwconv_fwd", ptr(x), ld_of(x), ptr(y), ld_of(y), ptr(w32), B, H, W, Cc, k, stride, ptr(scale), ptr(shift), act, None, 0,
                 did, st)
            emu_round(y)
        if ctx is not None:
            if has_bn:
                raise RuntimeError("dwconv: gradients through an eval-mode BatchNorm are not supported")
            ctx.z, ctx.aff, ctx.y = (z, None, None) if keep_z else (None, None, y)
    if tape is not None:
        tape.push(ctx)
    return y


def dwconv_backward(tape, dy, need_dx=True, dx_out=None, accumulate=False, add_src=None):
    """Backward of the matching dwconv_forward (pops its context), the contract of conv_backward: BatchNorm / activation backward
    (dy_bn_act_bwd*, on a vector-padded copy of dy when the view is not vec_ok), the deterministic f32 weight gradient on the
    compute stream, and dx = [dx_out +] dgrad [+ add_src] in one launch with exact channel bounds."""
    ctx = tape.pop()
    x = ctx.x
    dtype, dev = x.dtype, x.device
    B, Cc, H, W = x.shape
    k, stride = ctx.k, ctx.stride
    Ho, Wo = dy.shape[2], dy.shape[3]
    cpad = round_up(Cc, vec_elems(dtype))
    pixels, es, did, st = B * Ho * Wo, x.element_size(), dt_id(dtype), stream()
    if tuple(dy.shape) != (B, Cc, Ho, Wo) or dy.dtype != dtype:
        raise RuntimeError("dwconv_backward: gradient does not match the forward's output")
    need_bias = ctx.bias is not None and ctx.bias.requires_grad
    if (ctx.bn is not None or ctx.act != ACT_NONE or need_bias) and not vec_ok(dy):
        t = _nhwc_like(B, Cc, Ho, Wo, dtype, dev)           # the BatchNorm passes read whole vectors: stage the slice
        copy_exact(dy, t)
        dy = t
    if ctx.bn is not None:
        dz = _nhwc_like(B, Cc, Ho, Wo, dtype, dev)
        _bn_backward(tape, dy, ctx.z, ctx.aff, ctx.bn, ctx.act, dz, pixels, cpad, Cc, did, st, dev, False)
    elif ctx.act == ACT_NONE and not need_bias:
        dz = dy
    else:
        src = ctx.z                                         # SiLU: the pre-activation, a vector-padded buffer of the forward's
        if src is None:
            src = ctx.y
            if not vec_ok(src):
                t = _nhwc_like(B, Cc, Ho, Wo, dtype, dev)
                copy_exact(src, t)
                src = t
        dz = _nhwc_like(B, Cc, Ho, Wo, dtype, dev) if ctx.act != ACT_NONE else dy
        _act_backward(tape, dy, src, ctx.bias, ctx.act, dz, pixels, cpad, Cc, did, st, dev, False)
    w32 = _w32(ctx.weight)
    shape = f"dw {Cc} k{k} s{stride} in {B}x{H}x{W}"
    flops = 2.0 * pixels * Cc * k * k
    if ctx.weight.requires_grad:
        gw, direct = _grad_sink(ctx.weight, ctx.weight.shape, dev)
        scratch = wgrad_scratch(dev, tag=st)
        _C._prof is not None and _C.set_meta(kind="dwconv_wgrad", shape=shape, dtype=str(dtype), flops=flops,
                                             bytes=float((B * H * W + pixels) * Cc * es + Cc * k * k * 4))
        call("dy_dwconv_wgrad", ptr(x), ld_of(x), ptr(dz), ld_of(dz), ptr(gw), B, H, W, Cc, k, stride, ptr(scratch), scratch.numel(), did, st)
        if not direct:
            _add_pgrad(tape, ctx.weight, gw)
    if not need_dx:
        return None
    dx, accumulate = _dx_dest("dwconv_backward", dx_out, accumulate, add_src, (B, Cc, H, W), dtype,
                              lambda: _nhwc_like(B, Cc, H, W, dtype, dev))
    n_rw = 1 + (1 if accumulate else 0) + (1 if add_src is not None else 0)
    _C._prof is not None and _C.set_meta(kind="dwconv_dgrad", shape=shape, dtype=str(dtype), flops=flops,
                                         bytes=float((n_rw * B * H * W + pixels) * Cc * es + Cc * k * k * 4))
    call("dy_dwconv_dgrad", ptr(dz), ld_of(dz), ptr(dx), ld_of(dx), ptr(w32), B, H, W, Cc, k, stride, 1 if accumulate else 0,
         ptr(add_src), 0 if add_src is None else ld_of(add_src), did, st)
    emu_round(dx)
    return dx


# ------------------------------------------------------------------------------------------------ small ops
def copy2d(src, dst, accumulate=False):
    B, Cc, H, W = src.shape
    Cp = padded_channels(src)
    call("dy_copy2d", ptr(src), ld_of(src), ptr(dst), ld_of(dst), B * H * W, Cp, 1 if accumulate else 0, dt_id(src.dtype), stream())


def maxpool_fwd(x, k, stride, pad, out=None, want_arg=True):
    B, Cc, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = out if out is not None else empty_nhwc(B, Cc, Ho, Wo, x.dtype, x.device)
    arg = torch.empty((B, Ho, Wo, Cc), dtype=torch.uint8, device=x.device) if want_arg else None
    call("dy_maxpool_fwd", ptr(x), ld_of(x), ptr(y), ld_of(y), ptr(arg), B, H, W, Cc, k, stride, pad, Ho, Wo, dt_id(x.dtype),
         stream())
    return y, arg


def maxpool_bwd(dy, arg, in_shape, k, stride, pad, dx_out=None, accumulate=False):
    B, Cc, H, W = in_shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    dx = dx_out if dx_out is not None else empty_nhwc(B, Cc, H, W, dy.dtype, dy.device)
    call("dy_maxpool_bwd", ptr(dy), ld_of(dy), ptr(arg), ptr(dx), ld_of(dx), B, H, W, Cc, k, stride, pad, Ho, Wo,
         1 if (accumulate and dx_out is not None) else 0, dt_id(dy.dtype), stream())
    emu_round(dx)
    return dx


def upsample_fwd(x, scale, out=None):
    B, Cc, H, W = x.shape
    y = out if out is not None else empty_nhwc(B, Cc, H * scale, W * scale, x.dtype, x.device)
    call("dy_upsample_nearest_fwd", ptr(x), ld_of(x), ptr(y), ld_of(y), B, H, W, Cc, scale, dt_id(x.dtype), stream())
    return y


def upsample_bwd(dy, scale, dx_out=None, accumulate=False):
    B, Cc, Ho, Wo = dy.shape
    H, W = Ho // scale, Wo // scale
    dx = dx_out if dx_out is not None else empty_nhwc(B, Cc, H, W, dy.dtype, dy.device)
    call("dy_upsample_nearest_bwd", ptr(dy), ld_of(dy), ptr(dx), ld_of(dx), B, H, W, Cc, scale,
         1 if (accumulate and dx_out is not None) else 0, dt_id(dy.dtype), stream())
    emu_round(dx)
    return dx


def _asff_dims(who, sources, logits, *like):
    n = len(sources)
    B, Cc, H, W = sources[0].shape
    if n not in (2, 3) or any(tuple(t.shape) != (B, Cc, H, W) or t.dtype != logits.dtype for t in (*sources, *like) if t is not None):
        raise RuntimeError(f"{who}: two or three sources, all NHWC views of one shape and of the logits' dtype")
    if tuple(logits.shape) != (B, n, H, W):
        raise RuntimeError(f"{who}: {n} sources need logits [B, {n}, H, W], got {tuple(logits.shape)}")
    return n, B, Cc, H, W


def _ptr_ld(t):
    return (None, 0) if t is None else (t.data_ptr(), ld_of(t))


def asff_fuse_forward(sources, logits, out=None):
    """sum_k softmax_k(logits) * sources[k] per pixel (dy_asff_fuse_fwd): the ASFF blend of 2 or 3 same-shape NHWC maps under the
    per-pixel logits [B, n, H, W].  Returns the fused map (`out` when given)."""
    n, B, Cc, H, W = _asff_dims("asff_fuse_forward", sources, logits, out)
    o = out if out is not None else empty_nhwc(B, Cc, H, W, logits.dtype, logits.device)
    r = (*sources, None)[:3]
    call("dy_asff_fuse_fwd", *_ptr_ld(r[0]), *_ptr_ld(r[1]), *_ptr_ld(r[2]), *_ptr_ld(logits), *_ptr_ld(o), B * H * W, Cc, dt_id(o.dtype),
         stream())
    emu_round(o)
    return o


def asff_fuse_backward(dfused, sources, logits, into=None):
    """Backward of asff_fuse_forward (dy_asff_fuse_bwd).  Returns ([gradient of each source], gradient of the logits [B, n, H, W], a
    view of a buffer as wide as the logits' own).  into[k]: a gradient another consumer of source k already left; the blend's adds
    into it (the kernel's acc flag) and it is what comes back for k."""
    n, B, Cc, H, W = _asff_dims("asff_fuse_backward", sources, logits, dfused, *(into or ()))
    dt, dev = logits.dtype, logits.device
    into = (*(into or (None,) * n), None)[:3]
    r = (*sources, None)[:3]
    d = [t if t is not None else empty_nhwc(B, Cc, H, W, dt, dev) for t in into[:n]] + [None] * (3 - n)
    lw = ld_of(logits)
    dlog = empty_nhwc(B, lw, H, W, dt, dev)
    call("dy_asff_fuse_bwd", *_ptr_ld(dfused), *_ptr_ld(r[0]), *_ptr_ld(r[1]), *_ptr_ld(r[2]), ptr(logits), lw, *_ptr_ld(d[0]), *_ptr_ld(d[1]),
         *_ptr_ld(d[2]), ptr(dlog), lw, B * H * W, Cc, *(int(t is not None) for t in into), dt_id(dt), stream())
    emu_round(*d, dlog)
    return d[:n], dlog[:, :n]


DET_MAX_LEVELS = 4          # DY_DET_MAX_LEVELS


def det_maps(maps, strides, nc):
    """Build the descriptor for 1-4 NHWC Detect maps [B, 64+nc, h, w]: a dy_det_maps for up to three levels, a
    dy_det_maps4 (a DetMaps subclass, passed the same way) for four."""
    if not 1 <= len(maps) <= DET_MAX_LEVELS:
        raise ValueError(f"det_maps: {len(maps)} maps; the loss and decode kernels take 1-{DET_MAX_LEVELS}")
    m = DetMaps4() if len(maps) == 4 else DetMaps()
    m.B, m.nc, m.n_levels = maps[0].shape[0], nc, len(maps)
    m.dtype = dt_id(maps[0].dtype)
    for i, t in enumerate(maps[:3]):
        m.map[i] = t.data_ptr()
        m.map_ld[i] = ld_of(t)
        m.h[i], m.w[i] = t.shape[2], t.shape[3]
        m.stride[i] = float(strides[i])
    if len(maps) == 4:
        t = maps[3]
        m.map3, m.map_ld3, m.h3, m.w3, m.stride3 = t.data_ptr(), ld_of(t), t.shape[2], t.shape[3], float(strides[3])
    return m


def scale_img_sizes(H, W, ratio, gs):
    """(hs, ws, Hp, Wp) of scale_img (reference torch_utils.py:270-279): the resized size int(H * ratio), int(W * ratio) and the
    padded one ceil(H * ratio / gs) * gs, ceil(W * ratio / gs) * gs, in Python doubles as the reference computes them; ratio 1.0 keeps
    the image."""
    if ratio == 1.0:
        return H, W, H, W
    return (int(H * ratio), int(W * ratio), *(math.ceil(v * ratio / gs) * gs for v in (H, W)))


def tta_scale_img(x, ratio, gs, flip=None):
    """scale_img(x.flip(flip), ratio, gs=gs) of one augmented pass in one kernel (dy_tta_scale_img) for x f32 NCHW on the GPU: flip
    None / 0, 2 (up-down) or 3 (left-right); bilinear resize by `ratio`, right / bottom padding with 0.447 to the multiple of gs."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise ValueError("tta_scale_img: expected a contiguous f32 NCHW tensor on the GPU")
    B, Cc, H, W = x.shape
    hs, ws, Hp, Wp = scale_img_sizes(H, W, ratio, gs)
    out = torch.empty((B, Cc, Hp, Wp), dtype=torch.float32, device=x.device)
    call("dy_tta_scale_img", ptr(x), B, Cc, H, W, hs, ws, Hp, Wp, int(flip or 0), ptr(out), stream())
    return out


def pose_desc(kpts, strides, kpt_shape):
    """dy_pose_desc of the Pose head's per-level keypoint maps (NHWC [B, K*ndim, h, w], anchors level by level); the loss fields
    are left null for the caller to fill."""
    if not 1 <= len(kpts) <= _C.POSE_MAX_LEVELS:
        raise ValueError(f"pose_desc: {len(kpts)} levels; the pose kernels take 1-{_C.POSE_MAX_LEVELS}")
    d = _C.PoseDesc()
    d.n_levels, d.B, d.K, d.ndim = len(kpts), kpts[0].shape[0], int(kpt_shape[0]), int(kpt_shape[1])
    d.dtype = dt_id(kpts[0].dtype)
    A = 0
    for i, t in enumerate(kpts):
        if t.dtype != kpts[0].dtype or t.shape[1] != d.K * d.ndim:
            raise ValueError(f"pose_desc: level {i} is {tuple(t.shape)} {t.dtype}, expected {d.K * d.ndim} channels")
        d.kpt[i], d.kpt_ld[i], d.h[i], d.w[i], d.stride[i] = t.data_ptr(), ld_of(t), t.shape[2], t.shape[3], float(strides[i])
        A += t.shape[2] * t.shape[3]
    d.A = A
    return d


# ------------------------------------------------------------------------------------------------ classify task (csrc/classify.hip)
def gap_fwd(x):
    """AdaptiveAvgPool2d(1) of an NHWC view [N, C, H, W] -> NHWC [N, C, 1, 1] (pad lanes, if any, zero)."""
    N, Cc, H, W = x.shape
    Cp = round_up(Cc, vec_elems(x.dtype))
    y = (empty_nhwc if Cp == Cc else zeros_nhwc)(N, Cp, 1, 1, x.dtype, x.device)
    call("dy_gap_fwd", ptr(x), ld_of(x), N, H * W, Cc, dt_id(x.dtype), ptr(y), Cp, stream())
    emu_round(y)
    return y if Cp == Cc else y[:, :Cc]


def gap_bwd(dy, H, W):
    """Adjoint of gap_fwd: dy NHWC [N, C, 1, 1] -> dx NHWC [N, C, H, W] = dy / (H W) at every pixel."""
    N, Cc = dy.shape[0], dy.shape[1]
    Cp = round_up(Cc, vec_elems(dy.dtype))
    dx = (empty_nhwc if Cp == Cc else zeros_nhwc)(N, Cp, H, W, dy.dtype, dy.device)
    call("dy_gap_bwd", ptr(dy), ld_of(dy), N, H * W, Cc, dt_id(dy.dtype), ptr(dx), Cp, stream())
    emu_round(dx)
    return dx if Cp == Cc else dx[:, :Cc]


def row_matrix(t):
    """(B, n, leading dimension) of a device row matrix: [B, n] with unit column stride (a slice of a padded buffer included) or an
    NHWC [B, n, 1, 1] view -- how logits travel, never compacted."""
    require_gpu(t)
    if t.dim() == 4 and t.shape[2] == 1 and t.shape[3] == 1:
        return t.shape[0], t.shape[1], ld_of(t)
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError(f"dedark_yolo_amd: expected rows [B, n] with unit column stride, got {tuple(t.shape)} strides {t.stride()}")
    B, n = t.shape
    ld = t.stride(0) if B > 1 else n
    if ld < n:
        raise RuntimeError(f"dedark_yolo_amd: rows overlap: shape {tuple(t.shape)} strides {t.stride()}")
    return B, n, ld


def rows_2d(t):
    """The [B, n] view (strides (ld, 1)) of an NHWC [B, n, 1, 1] view."""
    return t[:, :, 0, 0] if t.dim() == 4 else t


def rows_4d(t, ve):
    """The NHWC [B, n, 1, 1] view of rows [B, n] whose leading dimension covers n rounded up to `ve` (a gradient written by
    dy_cls_xent_bwd, pad columns zero); None when `t` is not such a view."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        return None
    B, n = t.shape
    ld = t.stride(0)
    if ld < round_up(n, ve) or t.storage_offset() + (B - 1) * ld + round_up(n, ve) > t.untyped_storage().nbytes() // t.element_size():
        return None
    return torch.as_strided(t, (B, n, 1, 1), (ld, 1, ld, ld), t.storage_offset())


def cls_xent_fwd(logits, cls):
    """(loss f32 [1], row_lse f32 [B]) of cross_entropy(logits, cls, reduction='sum') / 64; cls int64 [B] on the device."""
    B, nc, ld = row_matrix(logits)
    if cls.dtype != torch.int64 or not cls.is_cuda or cls.numel() != B or not cls.is_contiguous():
        raise RuntimeError(f"cls_xent_fwd: cls must be a contiguous int64 [{B}] device tensor")
    lse = torch.empty(B, dtype=torch.float32, device=logits.device)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    call("dy_cls_xent_fwd", ptr(logits), ld, dt_id(logits.dtype), ptr(cls), B, nc, ptr(lse), ptr(loss), stream())
    return loss, lse


def cls_xent_bwd(logits, cls, lse, grad_out):
    """d loss / d logits * grad_out (f32 device scalar): rows [B, nc] of a [B, round_up(nc, vector)] buffer whose pad columns are 0."""
    B, nc, ld = row_matrix(logits)
    dld = round_up(nc, vec_elems(logits.dtype))
    d = torch.empty((B, dld), dtype=logits.dtype, device=logits.device)
    call("dy_cls_xent_bwd", ptr(logits), ld, dt_id(logits.dtype), ptr(cls), ptr(lse), ptr(grad_out), B, nc, ptr(d), dld, stream())
    emu_round(d)
    return d[:, :nc]


def cls_softmax(logits):
    B, nc, ld = row_matrix(logits)
    probs = torch.empty((B, nc), dtype=torch.float32, device=logits.device)
    call("dy_cls_softmax", ptr(logits), ld, dt_id(logits.dtype), B, nc, ptr(probs), stream())
    return probs


def cls_topk(scores, k=None):
    """int32 [B, k] indices of the k (default min(nc, 5)) largest scores per row, descending; ties by ascending index, NaN last."""
    B, nc, ld = row_matrix(scores)
    k = min(nc, 5) if k is None else int(k)
    idx = torch.empty((B, k), dtype=torch.int32, device=scores.device)
    call("dy_cls_topk", ptr(scores), ld, dt_id(scores.dtype), B, nc, k, ptr(idx), stream())
    return idx


def cls_metrics_update(idx, cls, nc, counts, confusion=None):
    """counts int64 [3] += (rows, top-1 hits, top-k hits), confusion int32 [nc, nc] [pred][target] += 1 for one batch (device)."""
    B, k = idx.shape
    if idx.dtype != torch.int32 or cls.dtype != torch.int64 or cls.numel() != B or counts.dtype != torch.int64 or counts.numel() != 3:
        raise RuntimeError("cls_metrics_update: idx int32 [B, k], cls int64 [B], counts int64 [3]")
    if confusion is not None and (confusion.dtype != torch.int32 or tuple(confusion.shape) != (nc, nc) or not confusion.is_contiguous()):
        raise RuntimeError(f"cls_metrics_update: confusion must be a contiguous int32 [{nc}, {nc}]")
    for t in (idx, cls, counts):
        require_gpu(t)
    call("dy_cls_metrics_update", ptr(idx.contiguous()), k, ptr(cls.contiguous()), B, nc, ptr(counts), ptr(confusion), stream())

# ------------------------------------------------------------------------------------------------ validation matching
VAL_MATCH_SLOTS, VAL_MATCH_LDS = 5, 40 * 1024       # csrc/valmatch.hip: ints of state per detection, bytes of it that LDS holds


def _val_match_ws(B, max_det, device):
    """The global workspace of the per-detection state when it does not fit in LDS (include/dedark_yolo.h), else None."""
    if max_det * VAL_MATCH_SLOTS * 4 <= VAL_MATCH_LDS:
        return None
    return torch.empty(B * max_det * VAL_MATCH_SLOTS, dtype=torch.int32, device=device)


def _val_match_args(det, ocnt, lcls, loff, iouv):
    if det.dim() != 3 or det.dtype != torch.float32 or not det.is_contiguous() or det.shape[1] < 1 or det.shape[2] < 6:
        raise RuntimeError("val match: det must be a contiguous f32 [B, max_det >= 1, >= 6] tensor (nms_batched's rows)")
    B = det.shape[0]
    if ocnt.dtype != torch.int32 or ocnt.numel() != B or loff.dtype != torch.int32 or loff.numel() != B + 1:
        raise RuntimeError("val match: ocnt int32 [B], loff int32 [B + 1]")
    if lcls.dtype != torch.float32 or lcls.dim() != 1 or iouv.dtype != torch.float32 or not 1 <= iouv.numel() <= 16:
        raise RuntimeError("val match: lcls f32 [L], iouv f32 [T <= 16]")
    for t in (det, ocnt, lcls, loff, iouv):
        require_gpu(t)
    return B, det.shape[1], det.shape[2]


def val_box_match(det, ocnt, lcls, lxywh, loff, shape, rec, iouv, single_cls=False, confusion=None, conf=0.25, iou_thres=0.45):
    """dy_val_box_match on one batch (all device tensors): det [B, max_det, >= 6] f32 + ocnt [B] int32 from nms_batched, the labels
    sorted by image (lcls [L] f32, lxywh [L, 4] f32 normalised, loff [B + 1] int32), shape = the network input (H, W), rec [B, 5] f32
    = (gain, pad_x, pad_y, h0, w0), iouv [T] f32 -> (correct uint8 [B, max_det, T], predn f32 [B, max_det, 4], tboxn f32 [L, 4]).
    confusion: int32 [nc + 1, nc + 1] accumulator [predicted][true], updated in place (None: not filled)."""
    B, max_det, ld = _val_match_args(det, ocnt, lcls, loff, iouv)
    L, T, dev = lcls.numel(), iouv.numel(), det.device
    if lxywh.dtype != torch.float32 or tuple(lxywh.shape) != (L, 4) or rec.dtype != torch.float32 or tuple(rec.shape) != (B, 5):
        raise RuntimeError("val_box_match: lxywh f32 [L, 4], rec f32 [B, 5]")
    nc = 1
    if confusion is not None:
        nc = confusion.shape[0] - 1
        if confusion.dtype != torch.int32 or tuple(confusion.shape) != (nc + 1, nc + 1) or not confusion.is_contiguous() or nc < 1:
            raise RuntimeError("val_box_match: confusion must be a contiguous int32 [nc + 1, nc + 1]")
        require_gpu(confusion)
    correct = torch.empty((B, max_det, T), dtype=torch.uint8, device=dev)
    predn = torch.empty((B, max_det, 4), dtype=torch.float32, device=dev)
    tboxn = torch.empty((L, 4), dtype=torch.float32, device=dev)
    ws = _val_match_ws(B, max_det, dev)
    call("dy_val_box_match", ptr(det), ld, ptr(ocnt), B, max_det, ptr(lcls.contiguous()), ptr(lxywh.contiguous()), ptr(loff.contiguous()),
         L, int(shape[0]), int(shape[1]), ptr(rec.contiguous()), ptr(iouv.contiguous()), T, int(bool(single_cls)), float(conf),
         float(iou_thres), nc, ptr(correct), ptr(predn), ptr(tboxn), ptr(confusion), ptr(ws), stream())
    return correct, predn, tboxn


def val_iou_match(iou, moff, det, ocnt, lcls, loff, iouv, single_cls=False):
    """dy_val_iou_match: iou = the batch's [M_b, N_b] f32 matrices packed one after another (f32 [sum M_b * N_b]), moff int64 [B] their
    offsets; the other arguments as val_box_match -> correct uint8 [B, max_det, T]."""
    B, max_det, ld = _val_match_args(det, ocnt, lcls, loff, iouv)
    if iou.dtype != torch.float32 or not iou.is_contiguous() or moff.dtype != torch.int64 or moff.numel() != B:
        raise RuntimeError("val_iou_match: iou contiguous f32, moff int64 [B]")
    require_gpu(moff)
    T, dev = iouv.numel(), det.device
    correct = torch.empty((B, max_det, T), dtype=torch.uint8, device=dev)
    ws = _val_match_ws(B, max_det, dev)
    call("dy_val_iou_match", ptr(iou), iou.numel(), ptr(moff.contiguous()), ptr(det), ld, ptr(ocnt), B, max_det, ptr(lcls.contiguous()),
         ptr(loff.contiguous()), lcls.numel(), ptr(iouv.contiguous()), T, int(bool(single_cls)), ptr(correct), ptr(ws), stream())
    return correct

# ------------------------------------------------------------------------------------------------ ConvTranspose2d(k=2, s=2)
class ConvTCtx:
    __slots__ = ("x", "weight", "bias")


def conv_transpose2x2_forward(tape, x, weight, bias=None):
    """nn.ConvTranspose2d(c1, c2, 2, 2, 0) (the Proto's upsample, reference block.py:242-254) on the conv kernels.  The weight
    [c1, c2, 2, 2] is the OIHW weight of a 2x2 / stride-2 / pad-0 conv that maps c2 -> c1, so the transposed conv's forward is that
    conv's data gradient (dy_conv2d_dgrad: four one-tap parity classes writing strided destinations) and its bias is added by
    dy_bias_add.  x: NHWC view [B, c1, H, W] -> NHWC [B, c2, 2H, 2W] with zero channel padding."""
    dtype = x.dtype
    B, c1, H, W = x.shape
    if weight.shape[0] != c1 or tuple(weight.shape[2:]) != (2, 2):
        raise RuntimeError(f"conv_transpose2x2: weight {tuple(weight.shape)} does not fit {c1} input channels")
    c2 = weight.shape[1]
    ve = vec_elems(dtype)
    c1_pad, c2_pad = padded_channels(x), round_up(c2, ve)
    wt = _pack(weight, c1_pad, c2_pad, True, dtype)
    y = empty_nhwc(B, c2_pad, 2 * H, 2 * W, dtype, x.device)
    d = _conv_desc(x, wt, y, B, H, W, c1_pad, 2 * H, 2 * W, c2_pad, 2, 2, 2, 0, 1, None, None, ACT_NONE, None, False, dtype)
    d.dst_valid_channels = c2
    _C._prof is not None and _C.set_meta(kind="convT_fwd", dtype=str(dtype), **_conv_meta(c1, c2, 2, 2, 2, B, H, W, B * H * W),
                                         bytes=float((B * H * W * c1 + 4 * B * H * W * c2) * x.element_size()))
    call("dy_conv2d_dgrad", C.byref(d), stream())
    if bias is not None:
        call("dy_bias_add", ptr(y), ld_of(y), ptr(bias.detach()), B * 4 * H * W, c2, dt_id(dtype), stream())
    emu_round(y)
    if tape is not None:
        ctx = ConvTCtx()
        ctx.x, ctx.weight, ctx.bias = x, weight, bias
        tape.push(ctx)
    return y if c2_pad == c2 else y[:, :c2]


def conv_transpose2x2_backward(tape, dy, need_dx=True):
    """Backward of conv_transpose2x2_forward (pops its context).  Weight gradient = the 2x2 / stride-2 conv's weight gradient with
    x = dy and dz = the forward's input (dy_conv2d_wgrad writes [c1][c2][2][2], exactly ConvTranspose2d.weight.grad); bias gradient =
    per-channel sum of dy (dy_bias_grad, fixed order); data gradient = that conv's forward of dy (dy_conv2d_fwd)."""
    ctx = tape.pop()
    x, weight, bias = ctx.x, ctx.weight, ctx.bias
    dtype, dev, st = x.dtype, x.device, stream()
    B, c1, H, W = x.shape
    c2 = weight.shape[1]
    c1_pad = padded_channels(x)
    c2_pad = round_up(c2, vec_elems(dtype))
    if tuple(dy.shape) != (B, c2, 2 * H, 2 * W) or dy.dtype != dtype:
        raise RuntimeError("conv_transpose2x2_backward: gradient does not match the forward's output")
    if padded_channels(dy) != c2_pad:
        raise RuntimeError("conv_transpose2x2_backward: gradient view lacks zero padding")
    did = dt_id(dtype)
    pixels = B * 4 * H * W
    if bias is not None and bias.requires_grad:
        db, direct = _grad_sink(bias, c2, dev)
        scratch = wgrad_scratch(dev, tag=st)
        call("dy_bias_grad", ptr(dy), ld_of(dy), pixels, c2, did, ptr(scratch), scratch.numel(), ptr(db), st)
        if not direct:
            _add_pgrad(tape, bias, db)
    if weight.requires_grad:
        gw, direct = _grad_sink(weight, weight.shape, dev)
        scratch = wgrad_scratch(dev, tag=st)
        _C._prof is not None and _C.set_meta(kind="convT_wgrad", dtype=str(dtype), **_conv_meta(c1, c2, 2, 2, 2, B, H, W, B * H * W),
                                             bytes=float((B * H * W * c1 + pixels * c2) * x.element_size()))
        call("dy_conv2d_wgrad", ptr(dy), ld_of(dy), B, 2 * H, 2 * W, c2_pad, ptr(x), ld_of(x), H, W, c1_pad, 2, 2, 2, 0, 1, c1, c2,
             ptr(scratch), scratch.numel(), ptr(gw), did, st)
        if not direct:
            _add_pgrad(tape, weight, gw)
    if not need_dx:
        return None
    wp = _pack(weight, c1_pad, c2_pad, False, dtype)
    dx = empty_nhwc(B, c1_pad, H, W, dtype, dev)
    d = _conv_desc(dy, wp, dx, B, 2 * H, 2 * W, c2_pad, H, W, c1_pad, 2, 2, 2, 0, 1, None, None, ACT_NONE, None, False, dtype)
    _C._prof is not None and _C.set_meta(kind="convT_dgrad", dtype=str(dtype), **_conv_meta(c1, c2, 2, 2, 2, B, H, W, B * H * W),
                                         bytes=float((B * H * W * c1 + pixels * c2) * x.element_size()))
    call("dy_conv2d_fwd", C.byref(d), st)
    emu_round(dx)
    return dx if c1_pad == c1 else dx[:, :c1]
