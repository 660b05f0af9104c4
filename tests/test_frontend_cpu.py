"""CPU: the yardsticks of the front-end kernel tests (tests/test_gpu_frontend_kernels.py) checked on their own.

  * the oracle's lowlight_recovery in f32 against the reference fixture of the TRAINING configuration (A / IcA supplied);
  * the input law of every pointwise case meets the conditions that keep f32 and f64 comparable (tests/frontend_ref.py);
  * the f64 separable USM equals the dense 625-tap definition;
  * the adjoint border rule csrc/usm.hip's backward kernel is built on.
"""
import numpy as np
import pytest
import torch

import frontend_ref as fr
from oracle import frontend as ofe
from oracle import model as om
from util import close, gold


def test_frontend_aica_golden_forward_backward():
    """oracle.frontend.lowlight_recovery with A / IcA given, train-mode gradients included, at the tolerances of g1_frontend."""
    g = gold("g19_frontend_aica")
    shapes = {k[len("model.0."):]: v for k, v in om.param_shapes([dict(i=0, kind="lowlight_recovery")]).items()}
    sd = om.rng_fill(shapes, int(g["seed"]))
    for v in sd.values():
        v.requires_grad_(v.is_floating_point())
    x = g["x"].clone().requires_grad_(True)
    out, feat, st, _ = ofe.lowlight_recovery(sd, "", x, g["A"], g["IcA"], stages=True)
    close(feat, g["feat"], 1e-4, 1e-5, "feat")
    for i, s in enumerate(st):
        close(s[..., ::3, ::3], g[f"s{i + 1}"], 1e-4, 1e-4, f"stage {i + 1}")
    close(out, g["out"], 1e-4, 1e-4, "out")
    (out * g["wgt"]).sum().backward()
    close(x.grad, g["dx"], 1e-3, 1e-3, "dx")
    close(sd["extractor.fc2.weight"].grad, g["d_fc2_w"], 1e-3, 1e-2, "d fc2.w")
    close(sd["extractor.fc2.bias"].grad, g["d_fc2_b"], 1e-3, 1e-2, "d fc2.b")
    close(sd["extractor.fc1.bias"].grad, g["d_fc1_b"], 1e-3, 1e-2, "d fc1.b")
    close(sd["extractor.conv_layers.0.conv_block.0.weight"].grad, g["d_c0_w"], 2e-3, 2e-2, "d conv0.w")
    close(sd["extractor.conv_layers.4.conv_block.0.bias"].grad, g["d_c4_b"], 2e-3, 2e-2, "d conv4.b")


@pytest.mark.parametrize("aica", [True, False], ids=["aica", "defaults"])
@pytest.mark.parametrize("shape", fr.POINTWISE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pointwise_input_law(shape, aica):
    """Every pointwise case of the GPU file: no pixel near a gradient kink, every branch populated, and -- what the law is for --
    torch's own f32 chain then agrees with f64 far inside the kernels' bounds (so a kernel that misses them is wrong)."""
    c = fr.pointwise_case(*shape, aica=aica)
    pop = fr.check_input_law(c, aica)
    ref = fr.pointwise_fwd_bwd(c["x"], c["params"], c["A"], c["IcA"], c["g4"])
    f32 = fr.pointwise_fwd_bwd(c["x"], c["params"], c["A"], c["IcA"], c["g4"], torch.float32)
    errs = [fr.rel_err(a, b) for a, b in zip(f32, ref)]
    print(shape, aica, pop, "torch f32 vs f64: s4 %.1e dx %.1e dparams %.1e" % tuple(errs))
    # Inside the project's f32 ceilings (forward 1e-4, gradients 2e-3) with room to spare.  What is left is not a kink: a row
    # whose three luminance pixels are all clamped has lum ~ 3e-5, where f32 evaluates 0.5 - 0.5 cos(pi lum) as exactly 0
    # (f64: 3e-9), which moves K = (1 - alpha) + alpha cl / (lum + 1e-6) by ~ alpha * 8e-5.  Any f32 evaluation of the reference's
    # formula shares that, the kernels included.
    assert errs[0] <= 1e-4 and max(errs[1:]) <= 2e-3 / 4, errs


def test_pointwise_null_defaults_are_08_05():
    """A / IcA None in the reference helper is the kernels' nullptr default: A = 0.8, IcA = 0.5."""
    c = fr.pointwise_case(2, 13, 13, aica=False)
    A, I = fr.default_aica(2, 13, 13, torch.float32)
    a = fr.pointwise_fwd_bwd(c["x"], c["params"], None, None, c["g4"])
    b = fr.pointwise_fwd_bwd(c["x"], c["params"], A, I, c["g4"])
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("H,W", [(13, 13), (24, 25), (41, 65)])
def test_separable_usm_equals_dense(H, W):
    g = np.random.default_rng(H * 100 + W)
    img = torch.from_numpy(g.random((2, 3, H, W))) * 1.5 - 0.2
    lam = torch.tensor([[0.0], [5.0]], dtype=torch.float64)
    dense, sep = ofe.f_usm(img, lam), fr.usm_separable(img, lam)
    assert float((dense - sep).abs().max()) <= 1e-13 * float(dense.abs().max())


@pytest.mark.parametrize("n", range(13, 61))
def test_usm_adjoint_border_rule(n):
    """With A = (reflect-pad 12, symmetric 25-tap blur) along one axis of n >= 13 samples, the adjoint differs from A only at the
    13 samples next to each edge:
        (A^T g)[m] = (A g)[m] + k[m] g[0]  for 1 <= m <= 12,     (A^T g)[0] = (A g)[0] - sum_{i=1..12} k[i] g[i],
    mirrored at n - 1 (both corrections add where the two borders overlap, n < 26).  usm_bwd_kernel evaluates A^T as the
    forward blur plus exactly these terms (adj_edge in csrc/usm.hip); this restates the rule against the explicit matrix so
    that a rewrite of the kernel has the derivation to lean on."""
    R = ofe.USM_RADIUS
    k = ofe.gaussian_taps(torch.float64).numpy()[R:]          # k[|d|]
    M = fr.blur_matrix(n)
    g = np.random.default_rng(n).standard_normal(n)
    want = M.T @ g
    got = M @ g
    for m in range(n):
        if m == 0:
            got[m] -= sum(k[i] * g[i] for i in range(1, R + 1))
        elif m <= R:
            got[m] += k[m] * g[0]
        if m == n - 1:
            got[m] -= sum(k[i] * g[n - 1 - i] for i in range(1, R + 1))
        elif n - 1 - R <= m <= n - 2:
            got[m] += k[n - 1 - m] * g[n - 1]
    assert np.abs(got - want).max() <= 1e-14 * max(1.0, np.abs(want).max())


def test_resize_reference_is_identity_without_resize():
    x = torch.from_numpy(np.random.default_rng(5).random((1, 3, 9, 7), dtype=np.float32))
    gy = torch.ones(1, 3, 9, 7)
    y, dx = fr.resize_fwd_bwd(x, 9, 7, gy)
    assert torch.equal(y, x.double()) and torch.equal(dx, gy.double())
