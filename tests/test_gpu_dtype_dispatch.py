"""GPU: the dtype dispatch of the C-ABI launchers (csrc/dy_host.h), through the entries of csrc/pool.hip called directly.

Exact operations (max pool, nearest upsample, copy / accumulate, cast) in f32, bf16 and f16, compared BIT FOR BIT with torch on the
same GPU: every value is a small integer, so every sum is exact in all three dtypes and there is no tolerance.  Sources and
destinations are channel slices [8, 24) (C = 16, ld = 32) of NHWC parents of 32 channels filled with a sentinel; the sentinel
lanes outside the slice must survive every call.

Unknown dtype: every entry returns "<entry>: bad dtype 7" and launches nothing.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
N, LD, H, W = 2, 32, 9, 7
C0, C = 8, 16                   # the view: channels [C0, C0 + C) of the LD-wide parent
SENTINEL = 99.0                 # exact in all three dtypes, outside every value range used below


def _api():
    from dedark_yolo_amd._C import call
    from dedark_yolo_amd.ops import dt_id, ptr, stream
    return call, ptr, stream, dt_id


def _parent(h, w, dt, fill=SENTINEL):
    return torch.full((N, h, w, LD), fill, device="cuda", dtype=dt)


def _view_ptr(parent):
    return parent.data_ptr() + C0 * parent.element_size()


def _put(parent, nchw):
    """write an [N, C, h, w] tensor into the view of an NHWC parent"""
    parent[..., C0:C0 + C] = nchw.permute(0, 2, 3, 1).to(parent.dtype)


def _get(parent):
    return parent[..., C0:C0 + C].permute(0, 3, 1, 2).contiguous()


def _same_bits(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    assert torch.equal(got.contiguous().view(BITS[got.dtype]), ref.contiguous().view(BITS[ref.dtype])), what


def _outside_intact(parent, what):
    assert bool((parent[..., :C0] == SENTINEL).all()) and bool((parent[..., C0 + C:] == SENTINEL).all()), f"{what}: wrote outside the view"


@functools.lru_cache(maxsize=None)
def _planes():
    """[N, C, H, W] f32 on the GPU: every (image, channel) plane is a permutation of the 63 integers -31 .. 31 (no ties)"""
    g = torch.Generator().manual_seed(20)
    p = torch.stack([torch.randperm(H * W, generator=g) for _ in range(N * C)]).view(N, C, H, W)
    return (p - 31).float().cuda()


def _ints(lo, hi, *shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float().cuda()


@functools.lru_cache(maxsize=None)
def _maxpool_ref(k, s, p):
    """(forward, dy, gradient of the forward with respect to x for that dy), all f32 NCHW, from torch"""
    x = _planes().clone().requires_grad_(True)
    y = F.max_pool2d(x, k, s, p)
    dy = _ints(-3, 3, *y.shape, seed=21)
    y.backward(dy)
    return y.detach(), dy, x.grad.detach()


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("k,s,p", [(5, 1, 2), (3, 2, 1)])
def test_maxpool_fwd_bwd_exact(k, s, p, dt):
    call, ptr, stream, dt_id = _api()
    dtype = DT[dt]
    y_ref, dy, dx_ref = _maxpool_ref(k, s, p)
    Ho, Wo = y_ref.shape[2:]
    x = _parent(H, W, dtype)
    _put(x, _planes())
    y = _parent(Ho, Wo, dtype)
    arg = torch.full((N * Ho * Wo * C,), 255, device="cuda", dtype=torch.uint8)
    call("dy_maxpool_fwd", _view_ptr(x), LD, _view_ptr(y), LD, ptr(arg), N, H, W, C, k, s, p, Ho, Wo, dt_id(dtype), stream())
    _same_bits(_get(y), y_ref.to(dtype), "max pool forward")
    _outside_intact(y, "max pool forward")
    assert int(arg.max()) < k * k

    g = _parent(Ho, Wo, dtype)
    _put(g, dy)
    base = _ints(-5, 5, N, C, H, W, seed=22)
    for accumulate in (0, 1):
        dx = _parent(H, W, dtype)
        if accumulate:
            _put(dx, base)
        call("dy_maxpool_bwd", _view_ptr(g), LD, ptr(arg), _view_ptr(dx), LD, N, H, W, C, k, s, p, Ho, Wo, accumulate, dt_id(dtype),
             stream())
        ref = dx_ref + base if accumulate else dx_ref          # |.| <= 25 * 3 + 5: exact in bf16 (8 bits) and f16 (11 bits)
        _same_bits(_get(dx), ref.to(dtype), f"max pool backward, accumulate={accumulate}")
        _outside_intact(dx, f"max pool backward, accumulate={accumulate}")
    _outside_intact(g, "max pool backward (dy)")
    _outside_intact(x, "max pool forward (x)")


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_upsample_nearest_fwd_bwd_exact(dt):
    call, ptr, stream, dt_id = _api()
    dtype = DT[dt]
    x = _parent(H, W, dtype)
    _put(x, _planes())
    y = _parent(2 * H, 2 * W, dtype)
    call("dy_upsample_nearest_fwd", _view_ptr(x), LD, _view_ptr(y), LD, N, H, W, C, 2, dt_id(dtype), stream())
    _same_bits(_get(y), F.interpolate(_planes(), scale_factor=2, mode="nearest").to(dtype), "upsample forward")
    _outside_intact(y, "upsample forward")

    dy = _ints(-3, 3, N, C, 2 * H, 2 * W, seed=23)
    dx_ref = dy.view(N, C, H, 2, W, 2).sum((3, 5))
    g = _parent(2 * H, 2 * W, dtype)
    _put(g, dy)
    base = _ints(-5, 5, N, C, H, W, seed=24)
    for accumulate in (0, 1):
        dx = _parent(H, W, dtype)
        if accumulate:
            _put(dx, base)
        call("dy_upsample_nearest_bwd", _view_ptr(g), LD, _view_ptr(dx), LD, N, H, W, C, 2, accumulate, dt_id(dtype), stream())
        ref = dx_ref + base if accumulate else dx_ref
        _same_bits(_get(dx), ref.to(dtype), f"upsample backward, accumulate={accumulate}")
        _outside_intact(dx, f"upsample backward, accumulate={accumulate}")


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_copy2d_exact(dt):
    call, ptr, stream, dt_id = _api()
    dtype = DT[dt]
    src = _parent(H, W, dtype)
    _put(src, _planes())
    base = _ints(-5, 5, N, C, H, W, seed=25)
    for accumulate in (0, 1):
        dst = _parent(H, W, dtype)
        if accumulate:
            _put(dst, base)
        call("dy_copy2d", _view_ptr(src), LD, _view_ptr(dst), LD, N * H * W, C, accumulate, dt_id(dtype), stream())
        ref = _planes() + base if accumulate else _planes()
        _same_bits(_get(dst), ref.to(dtype), f"copy2d, accumulate={accumulate}")
        _outside_intact(dst, f"copy2d, accumulate={accumulate}")
    _outside_intact(src, "copy2d (src)")


@functools.lru_cache(maxsize=None)
def _cast_source():
    g = torch.Generator().manual_seed(26)
    v = torch.cat([torch.randn(998, generator=g) * 100, torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1e-6])])
    assert v.numel() == 1003 and not bool(v.isnan().any())
    return v.cuda()


@pytest.mark.parametrize("src,dst", [("f32", "bf16"), ("bf16", "f32"), ("f32", "f16"), ("f16", "f32"), ("f32", "f32"), ("bf16", "bf16")])
def test_cast_matches_torch_bits(src, dst):
    call, ptr, stream, dt_id = _api()
    s = _cast_source().to(DT[src])
    n, tail = s.numel(), 13
    d = torch.full((n + tail,), SENTINEL, device="cuda", dtype=DT[dst])
    call("dy_cast", ptr(s), dt_id(DT[src]), ptr(d), dt_id(DT[dst]), n, stream())
    _same_bits(d[:n], s.to(DT[dst]), f"cast {src} -> {dst}")
    assert bool((d[n:] == SENTINEL).all()), "cast wrote past n"


# ============================================================================================================ unknown dtype
def _bad_dtype_calls():
    """name -> (entry, arguments).  Every tensor is legal and sized for f32, so even a check that failed to fire would stay in
    bounds; all of them hold the value 7."""
    call, ptr, stream, _ = _api()
    z = lambda *s: torch.full(s, 7.0, device="cuda")
    zd = lambda *s: torch.full(s, 7.0, device="cuda", dtype=torch.float64)
    t = dict(a=z(N, H, W, LD), b=z(N, H, W, LD), c=z(N, H, W, LD), d=z(N, H, W, LD), e=z(N, H, W, LD), f=z(N, H, W, LD), g=z(N, H, W, LD),
             up=z(N, 2 * H, 2 * W, LD), arg=torch.full((N * H * W * C,), 7, device="cuda", dtype=torch.uint8),
             lg=z(N * H * W, 4), dlg=z(N * H * W, 4), v1=z(LD), v2=z(LD), v3=z(LD), v4=z(LD), v5=z(LD), v6=z(LD), v7=z(LD),
             sums=zd(8 * 2 * C), mom=zd(N * C * 2), pooled=z(N, LD),
             img=z(1, 3, 16, 16), i2=z(1, 3, 16, 16), i3=z(1, 3, 16, 16), o8=z(1, 16, 16, 8), prm=z(1, 8), dprm=zd(1, 8))
    v = lambda k: t[k].data_ptr() + C0 * 4
    p, st, px, BAD = (lambda k: ptr(t[k])), stream(), N * H * W, 7
    calls = {
        "maxpool_fwd": ("dy_maxpool_fwd", (v("a"), LD, v("b"), LD, p("arg"), N, H, W, C, 5, 1, 2, H, W, BAD, st)),
        "maxpool_bwd": ("dy_maxpool_bwd", (v("a"), LD, p("arg"), v("b"), LD, N, H, W, C, 5, 1, 2, H, W, 0, BAD, st)),
        "upsample_fwd": ("dy_upsample_nearest_fwd", (v("a"), LD, v("up"), LD, N, H, W, C, 2, BAD, st)),
        "upsample_bwd": ("dy_upsample_nearest_bwd", (v("up"), LD, v("a"), LD, N, H, W, C, 2, 0, BAD, st)),
        "copy2d": ("dy_copy2d", (v("a"), LD, v("b"), LD, px, C, 0, BAD, st)),
        "asff_fwd": ("dy_asff_fuse_fwd", (v("a"), LD, v("b"), LD, v("c"), LD, p("lg"), 4, v("d"), LD, px, C, BAD, st)),
        "asff_bwd": ("dy_asff_fuse_bwd", (v("a"), LD, v("b"), LD, v("c"), LD, v("d"), LD, p("lg"), 4, v("e"), LD, v("f"), LD, v("g"), LD,
                                          p("dlg"), 4, px, C, 0, 0, 0, BAD, st)),
        "cast_src": ("dy_cast", (p("a"), BAD, p("b"), 0, px * LD, st)),
        "cast_dst": ("dy_cast", (p("a"), 0, p("b"), BAD, px * LD, st)),
        "bn_act_fwd": ("dy_bn_act_fwd", (v("a"), LD, p("v1"), p("v2"), 1, None, 0, v("b"), LD, px, C, BAD, st)),
        "bn_act_bwd_reduce": ("dy_bn_act_bwd_reduce", (v("a"), LD, v("b"), LD, p("v1"), p("v2"), p("v3"), p("v4"), 1, 1, p("sums"), px, C,
                                                       BAD, st)),
        "bn_act_bwd_apply_valid": ("dy_bn_act_bwd_apply_valid", (v("a"), LD, v("b"), LD, p("v1"), p("v2"), p("v3"), p("v4"), p("v5"), 1, 1,
                                                                 p("sums"), v("c"), LD, p("v6"), p("v7"), px, C, C, BAD, st)),
        "usm_fwd": ("dy_usm_fwd", (p("img"), p("prm"), p("i2"), p("o8"), p("i3"), 1, 16, 16, BAD, st)),
        "usm_bwd": ("dy_usm_bwd", (p("img"), None, 0, p("i3"), p("prm"), p("i2"), p("dprm"), 1, 16, 16, BAD, st)),
        "image_to_nhwc8": ("dy_image_to_nhwc8", (p("img"), 1, 16, 16, p("o8"), 16, 16, BAD, st)),
        "chan_moments": ("dy_chan_moments", (v("a"), LD, N, H * W, C, p("mom"), BAD, st)),
        "gap_fwd": ("dy_gap_fwd", (v("a"), LD, N, H * W, C, BAD, p("pooled"), LD, st)),
        "bias_add": ("dy_bias_add", (v("a"), LD, p("v1"), px, C, BAD, st)),
    }
    return call, t, calls


@pytest.mark.parametrize("name", ["maxpool_fwd", "maxpool_bwd", "upsample_fwd", "upsample_bwd", "copy2d", "asff_fwd", "asff_bwd",
                                  "cast_src", "cast_dst", "bn_act_fwd", "bn_act_bwd_reduce", "bn_act_bwd_apply_valid", "usm_fwd",
                                  "usm_bwd", "image_to_nhwc8", "chan_moments", "gap_fwd", "bias_add"])
def test_unknown_dtype_raises_and_launches_nothing(name):
    call, t, calls = _bad_dtype_calls()
    entry, args = calls[name]
    with pytest.raises(RuntimeError, match=entry + ".*bad dtype"):
        call(entry, *args)
    torch.cuda.synchronize()
    for k, v in t.items():
        assert bool((v == 7).all()), f"{name}: {k} was written"
