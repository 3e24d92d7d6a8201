"""Pins tests/pointwise_fp64.py -- the float64 yardstick of tests/test_hip_losses.py and tests/test_hip_pointwise.py --
without a GPU: against the reference-generated tests/golden/losses.npz, against the torch oracle (values and autograd
gradients, which are fp32: the bar is fp32 rounding of the ORACLE, a few 1e-6 relative) and against torch's own float64
autograd of batch_norm (bar: float64 rounding)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_fp64 as R
from oracle import gdn_oracle as O

F32_SUM = 2e-6        # an fp32 mean of ~1e3..1e6 terms accumulated pairwise by torch: a few 2^-24, with headroom


def _u(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _grad_close(ref64, got32, keep, what):
    scale = np.abs(ref64).max()
    err = np.abs(ref64 - R.f64(got32))[keep]
    assert err.max() <= 8 * R.EPS32 * scale, "%s: max err %.3e (scale %.3e)" % (what, err.max(), scale)


def test_golden_losses(golden):
    gl = golden["losses"]
    pred, gt, img = gl["pred"], gl["gt"], gl["img"]
    loss, grad = R.sobel_l1(pred, gt, 1.0)
    assert loss == pytest.approx(float(gl["imgrad_loss"]), rel=F32_SUM)
    amb = R.sobel_ambiguous(pred, gt)
    assert amb.mean() <= 5e-4
    _grad_close(grad, gl["imgrad_loss.dpred"], ~amb, "imgrad dpred")
    loss, grad, _ = R.smoothness(pred, img)
    assert loss == pytest.approx(float(gl["smooth_loss"]), rel=F32_SUM)
    amb = R.smooth_ambiguous(pred)
    assert amb.mean() <= 5e-4
    _grad_close(grad, gl["smooth_loss.dpred"], ~amb, "smooth dpred")


@pytest.mark.parametrize("B,H,W", [(2, 32, 48), (3, 5, 7), (1, 1, 9), (1, 9, 1)])
def test_oracle_losses(B, H, W):
    depth, rgb, sparse = O.synthetic_batch(B, H, W, seed=3)
    out = (depth + 0.4 * _u(depth.shape, 4)).requires_grad_(True)
    for sp, box in ((None, None), (sparse, None), (sparse, (1, max(2, H - 1), 0, max(1, W // 2)))):
        out.grad = None
        lo = O.berhu_masked(out, depth, sp, box)
        lo.backward()
        loss, grad, _ = R.berhu(out, depth, sp, box)
        assert loss == pytest.approx(lo.item(), rel=F32_SUM)
        _grad_close(grad, out.grad, np.ones(grad.shape, bool), "berhu grad")
    out.grad = None
    lo = O.imgrad_loss(out, depth)
    lo.backward()
    loss, grad = R.sobel_l1(out, depth, 1.0)
    assert loss == pytest.approx(lo.item(), rel=F32_SUM)
    _grad_close(grad, out.grad, ~R.sobel_ambiguous(out, depth), "sobel grad")
    out.grad = None
    lo = O.smoothness_loss(out, rgb)
    lo.backward()
    loss, grad, _ = R.smoothness(out, rgb)
    assert loss == pytest.approx(lo.item(), rel=F32_SUM)
    _grad_close(grad, out.grad, ~R.smooth_ambiguous(out), "smooth grad")


def test_oracle_losses_float64_exact():
    """The same formulas in torch float64: agreement to float64 rounding, signs at exact zeros included (dyadic inputs)."""
    g = torch.Generator().manual_seed(5)
    q = lambda shape, den: (torch.randint(-4, 5, shape, generator=g).double() / den)
    out, gt, img = q((2, 1, 12, 17), 4).requires_grad_(True), q((2, 1, 12, 17), 4), q((2, 3, 12, 17), 16)
    sparse = q((2, 2, 12, 17), 1)
    sob_x, sob_y = O._SOBEL_X, O._SOBEL_Y
    O._SOBEL_X, O._SOBEL_Y = sob_x.double(), sob_y.double()
    try:
        # (the oracle builds the 0.3 / 0.1 BerHu weights as fp32 constants also when the tensors are float64: 4e-8 relative)
        for fn, ref, rt in ((lambda: O.berhu_masked(out, gt, None), lambda: R.berhu(out, gt, None)[:2], 1e-13),
                            (lambda: O.berhu_masked(out, gt, sparse), lambda: R.berhu(out, gt, sparse)[:2], 5e-8),
                            (lambda: O.imgrad_loss(out, gt), lambda: R.sobel_l1(out, gt), 1e-13),
                            (lambda: O.smoothness_loss(out, img), lambda: R.smoothness(out, img)[:2], 1e-13)):
            out.grad = None
            lo = fn()
            lo.backward()
            loss, grad = ref()
            assert loss == pytest.approx(lo.item(), rel=rt)
            np.testing.assert_allclose(grad, out.grad.numpy(), rtol=10 * rt, atol=1e-15)      # (atol: cancellation in the stencil sums)
    finally:
        O._SOBEL_X, O._SOBEL_Y = sob_x, sob_y


def test_oracle_latent_loss():
    f = [_u((2, c, 6, 10), 10 + i) for i, c in enumerate((8, 16, 32, 32))]
    t = [_u((2, c, 6, 10), 20 + i) for i, c in enumerate((8, 16, 32, 32))]
    for a in f:
        a.requires_grad_(True)
    lo = O.latent_loss(f, t)
    lo.backward(torch.tensor(0.7))
    ref = sum(R.mse(a, b, 1.5 * w / 4.0) for w, a, b in zip(O.LATENT_W, f, t))
    assert ref == pytest.approx(lo.item(), rel=F32_SUM)
    for w, a, b in zip(O.LATENT_W, f, t):
        _grad_close(R.mse_grad(a, b, 1.5 * w / 4.0, 0.7), a.grad, np.ones(a.shape, bool), "latent grad")


@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)])
def test_batchnorm_vs_torch_float64(relu, res):
    g = torch.Generator().manual_seed(6)
    B, C, H, W = 3, 12, 7, 5
    y = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 2 + 0.7).requires_grad_(True)
    r = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    gam = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    bet = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
    z = F.batch_norm(y, None, None, gam, bet, True, 0.1, 1e-5)
    out = F.relu(z) if relu else z
    if res:
        out = out + r
    go = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(go)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    scale, shift, mean, invstd = R.bn_stats(nhwc(y), gam, bet)
    np.testing.assert_allclose(R.bn_apply(nhwc(y), scale, shift, relu, nhwc(r) if res else None), nhwc(out).numpy(),
                               rtol=1e-12, atol=1e-13)
    b = R.bn_train_bwd(nhwc(go), nhwc(y), scale, shift, mean, invstd, relu)
    np.testing.assert_allclose(b["dy"], nhwc(y.grad).numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(b["dgamma"], gam.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(b["dbeta"], bet.grad.numpy(), rtol=1e-10, atol=1e-12)
    # eval mode: fixed coefficients, the three relu modes
    y2 = y.detach().clone().requires_grad_(True)
    sc, sh = torch.from_numpy(scale).view(1, C, 1, 1), torch.from_numpy(shift).view(1, C, 1, 1)
    for mode in (0, 1, 2):
        y2.grad = None
        pre = y2 * sc + sh
        act = F.relu(pre) if mode else pre
        act.backward(go)
        seen = nhwc(act) if mode == 2 else nhwc(y2)
        np.testing.assert_allclose(R.bn_eval_bwd(nhwc(go), seen, scale, shift if mode != 2 else shift, mode),
                                   nhwc(y2.grad).numpy(), rtol=1e-12, atol=1e-13)


def test_rounding_helpers():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(20000, generator=g, dtype=torch.float64) * torch.exp(torch.randn(20000, generator=g, dtype=torch.float64) * 20)
    x32 = x.float()
    # from an fp32 value the hand rounding and torch's agree (one rounding either way)
    assert np.array_equal(R.round_bf16(x32.double().numpy()), x32.bfloat16().double().numpy())
    # double rounding differs from single rounding exactly where fp32 rounding lands on a bf16 tie
    v = np.array([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.4028234663852886e38, 2.0 ** -133 * 1.5,
                  -(1.0 + 2.0 ** -8 + 2.0 ** -40)])
    np.testing.assert_array_equal(R.round_bf16(v), [1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -6, np.inf, 2.0 ** -132, -(1.0 + 2.0 ** -7)])
    assert torch.tensor(v[0]).float().bfloat16().item() == 1.0          # (the two-step route gets the first one wrong)
    assert R.ulp(1.0, R.F32) == 2.0 ** -23 and R.ulp(1.5, R.BF16) == 2.0 ** -7 and R.ulp(0.0, R.F32) == 2.0 ** -149
    assert R.near_bf16_boundary(1.0 + 2.0 ** -8) and not R.near_bf16_boundary(1.0 + 2.0 ** -9)
    assert R.ulps_off(np.float32(1.0), 1.0 + 2.0 ** -23, R.F32) == 1.0
