"""Where a parameter's gradient lands must not change its value.

Every conv flavour of ops (conv, depthwise, PConv, ConvTranspose2x2) hands a parameter gradient either to `tape.pgrads` or, under
the trainer's direct placement (`p.grad` pre-allocated as f32, `p._dy_direct = True`), writes it into `p.grad`.  Both ways run
the same deterministic kernels and differ in the destination pointer only, so each case runs forward + backward twice from
identical inputs, once per way, and asserts torch.equal on dx and on every parameter gradient, and that the direct run left
nothing in `tape.pgrads`.  A `shared` conv (a weight used more than once per step) must deliver through `tape.pgrads` in both
runs, and its two uses must add up.  The attention in-projections own row blocks of one parameter (ops._ParamRows): the same two
ways, through the two transformer layers.  The weight-gradient side stream is off, so both runs are on one stream."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])


class _Tape:
    def __init__(self):
        self.stack, self.pgrads = [], {}

    def push(self, c):
        self.stack.append(c)

    def pop(self):
        return self.stack.pop()


@pytest.fixture(autouse=True)
def _one_stream():
    from dedark_yolo_amd import ops
    was = ops.wgrad_stream_enabled()
    ops.enable_wgrad_stream(False)
    yield
    ops.enable_wgrad_stream(was)
    ops.set_compute_dtype(torch.float32)


def _randn(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).cuda()


def _param(gen, *shape, scale=0.1):
    return _randn(gen, *shape, scale=scale).requires_grad_(True)


def _bn(gen, C):
    bn = nn.BatchNorm2d(C, eps=1e-3, momentum=0.03).cuda()
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.2 * _randn(gen, C))
        bn.bias.copy_(0.2 * _randn(gen, C))
    return bn


def _half(t, C, second):
    """A C-channel half of a fresh 2C-channel NHWC buffer holding `t` (the other half holds 7)."""
    from dedark_yolo_amd import ops
    B, _, H, W = t.shape
    buf = ops.empty_nhwc(B, 2 * C, H, W, t.dtype, t.device)
    buf.fill_(7.0)
    v = buf[:, C:] if second else buf[:, :C]
    v.copy_(t)
    return v


def _run(build, direct, expect_direct=True):
    """One forward + backward of `build()` = (parameters by name, step(tape) -> dx).  Returns dx and the gradients by name."""
    params, step = build()
    if direct:
        for p in params.values():
            p.grad = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
            p._dy_direct = True
    tape = _Tape()
    dx = step(tape)
    torch.cuda.synchronize()
    assert not tape.stack
    if direct and expect_direct:
        held = [n for n, p in params.items() if p in tape.pgrads]
        assert not held, f"direct placement, yet tape.pgrads holds {held}"
        return dx, {n: p.grad for n, p in params.items()}
    return dx, {n: tape.pgrads[p] for n, p in params.items()}


def _check_both_ways(build, expect_direct=True):
    dx0, g0 = _run(build, False)
    dx1, g1 = _run(build, True, expect_direct)
    assert dx0.shape == dx1.shape and torch.equal(dx0, dx1), "dx differs between the two gradient destinations"
    for n in g0:
        assert g0[n].dtype == torch.float32 and bool(g0[n].abs().max() > 0), n
        assert torch.equal(g0[n].reshape(-1), g1[n].reshape(-1)), f"gradient of {n} differs between tape.pgrads and p.grad"
    return g0


@DTYPES
def test_conv_bn_silu(dtype):
    """16 -> 20 channels (24 with padding in bf16: C_valid < C), 3x3, 9x7 map: weight, dgamma and dbeta."""
    from dedark_yolo_amd import ops
    ops.set_compute_dtype(dtype)

    def build():
        g = torch.Generator().manual_seed(11)
        w, bn = _param(g, 20, 16, 3, 3), _bn(g, 20)
        x, dy = ops.as_nhwc(_randn(g, 2, 16, 9, 7), dtype), ops.as_nhwc(_randn(g, 2, 20, 9, 7), dtype)

        def step(tape):
            ops.conv_forward(tape, x, w, None, bn, ops.ACT_SILU, 1, 1, 1, True)
            return ops.conv_backward(tape, dy)
        return dict(w=w, gamma=bn.weight, beta=bn.bias), step
    _check_both_ways(build)


def _bias_conv(dtype, act, shared, uses=(0, 1)):
    """Conv with bias and no BN, 16 -> 20, 1x1, 4x4 map, applied to the inputs `uses` with ONE weight."""
    from dedark_yolo_amd import ops

    def build():
        g = torch.Generator().manual_seed(12)
        w, b = _param(g, 20, 16, 1, 1), _param(g, 20)
        xs = [ops.as_nhwc(_randn(g, 2, 16, 4, 4), dtype) for _ in range(2)]
        dys = [ops.as_nhwc(_randn(g, 2, 20, 4, 4), dtype) for _ in range(2)]

        def step(tape):
            for i in uses:
                ops.conv_forward(tape, xs[i], w, b, None, act, 1, 0, 1, True, shared=shared)
            return torch.stack([ops.conv_backward(tape, dys[i]) for i in reversed(uses)])
        return dict(w=w, b=b), step
    return build


@DTYPES
@pytest.mark.parametrize("act", [0, 1], ids=["none", "silu"])
def test_conv_bias(dtype, act):
    """ACT_NONE takes the 0-pixel bias-only call, SiLU the full reduce + apply."""
    from dedark_yolo_amd import ops
    ops.set_compute_dtype(dtype)
    assert (ops.ACT_NONE, ops.ACT_SILU) == (0, 1)
    _check_both_ways(_bias_conv(dtype, act, False, uses=(0,)))


@DTYPES
@pytest.mark.parametrize("act", [0, 1], ids=["none", "silu"])
def test_shared_conv_bias_goes_through_pgrads_and_sums(dtype, act):
    from dedark_yolo_amd import ops
    ops.set_compute_dtype(dtype)
    both = _check_both_ways(_bias_conv(dtype, act, True), expect_direct=False)
    one = [_run(_bias_conv(dtype, act, True, uses=(i,)), False)[1] for i in (0, 1)]
    for n in both:
        assert torch.equal(both[n], one[0][n] + one[1][n]), f"two uses of {n} do not sum"


@DTYPES
@pytest.mark.parametrize("k,stride,C,halves", [(5, 1, 12, True), (3, 2, 16, False)], ids=["k5-c12-halves", "k3-s2-c16"])
def test_dwconv_bn_silu(dtype, k, stride, C, halves):
    """k5: x, out and dy are 12-channel halves of 24-channel buffers (not whole vectors in bf16: y and dy are staged)."""
    from dedark_yolo_amd import ops
    ops.set_compute_dtype(dtype)
    Ho = (8 + 2 * (k // 2) - k) // stride + 1

    def build():
        g = torch.Generator().manual_seed(13)
        w, bn = _param(g, C, 1, k, k), _bn(g, C)
        x, dy = _randn(g, 2, C, 8, 8).to(dtype), _randn(g, 2, C, Ho, Ho).to(dtype)
        if halves:
            x, dy, out = _half(x, C, False), _half(dy, C, True), _half(torch.zeros_like(dy), C, True)
            assert dtype != BF or not (ops.vec_ok(out) or ops.vec_ok(dy))
        else:
            x, dy, out = ops.as_nhwc(x, dtype), ops.as_nhwc(dy, dtype), None

        def step(tape):
            ops.dwconv_forward(tape, x, w, None, bn, ops.ACT_SILU, stride, True, out)
            return ops.dwconv_backward(tape, dy)
        return dict(w=w, gamma=bn.weight, beta=bn.bias), step
    _check_both_ways(build)


@DTYPES
@pytest.mark.parametrize("c3", [8, 16], ids=["c3_8-valu", "c3_16-packed"])
def test_pconv(dtype, c3):
    from dedark_yolo_amd import ops
    ops.set_compute_dtype(dtype)

    def build():
        g = torch.Generator().manual_seed(14)
        w = _param(g, c3, c3, 3, 3)
        x, dy = ops.as_nhwc(_randn(g, 2, 32, 8, 8), dtype), ops.as_nhwc(_randn(g, 2, 32, 8, 8), dtype)

        def step(tape):
            ops.pconv_forward(tape, x, w)
            return ops.pconv_backward(tape, dy)
        return dict(w=w), step
    _check_both_ways(build)


@DTYPES
def test_conv_transpose2x2(dtype):
    """16 -> 12 channels with bias, 4x4 map; dy is a 12-channel view whose pad lanes (to 16 in bf16) are zero."""
    from dedark_yolo_amd import ops
    ops.set_compute_dtype(dtype)

    def build():
        g = torch.Generator().manual_seed(15)
        w, b = _param(g, 16, 12, 2, 2), _param(g, 12)
        x, dy = ops.as_nhwc(_randn(g, 2, 16, 4, 4), dtype), ops.as_nhwc(_randn(g, 2, 12, 8, 8), dtype)
        assert ops.padded_channels(dy) == ops.round_up(12, ops.vec_elems(dtype))

        def step(tape):
            ops.conv_transpose2x2_forward(tape, x, w, b)
            return ops.conv_transpose2x2_backward(tape, dy)
        return dict(w=w, b=b), step
    _check_both_ways(build)


@DTYPES
@pytest.mark.parametrize("block", ["TransformerLayer", "TransformerEncoderLayer"])
def test_attention_in_projection_rows(dtype, block):
    """The three in-projections of nn.MultiheadAttention own ROWS of one in_proj_weight / in_proj_bias (ops._ParamRows): direct
    placement writes the rows of p.grad in place, the tape path files three blocks and joins them.  Head dim 8 (the kernels'
    minimum), a 3x5 map: every parameter of the block, the in-projection pair included, the same bytes both ways, and no row proxy
    left on either tape."""
    from dedark_yolo_amd import ops
    from dedark_yolo_amd.nn import modules
    ops.set_compute_dtype(dtype)
    tapes = []

    def build():
        torch.manual_seed(16)
        m = (modules.TransformerLayer(32, 4) if block == "TransformerLayer" else modules.TransformerEncoderLayer(32, 64, 4)).cuda().train()
        g = torch.Generator().manual_seed(16)
        x, dy = ops.as_nhwc(_randn(g, 2, 32, 3, 5), dtype), ops.as_nhwc(_randn(g, 2, 32, 3, 5), dtype)

        def step(tape):
            tapes.append(tape)
            m._fwd(tape, x)
            return m._bwd(tape, dy)
        return dict(m.named_parameters()), step
    g = _check_both_ways(build)
    assert g["ma.in_proj_weight"].shape == (96, 32) and g["ma.in_proj_bias"].shape == (96,)
    for i in range(3):                                        # each of the three row blocks received a gradient of its own
        assert bool(g["ma.in_proj_weight"][32 * i:32 * i + 32].abs().max() > 0)
        assert i == 1 or bool(g["ma.in_proj_bias"][32 * i:32 * i + 32].abs().max() > 0)      # (K's bias cancels in the soft-max)
    assert len(tapes) == 2 and not tapes[1].pgrads, "direct placement, yet tape.pgrads is not empty"
    assert not any(isinstance(k, ops._ParamRows) for t in tapes for k in t.pgrads)
