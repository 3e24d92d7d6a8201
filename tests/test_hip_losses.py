"""Every entry point of csrc/losses.hip, called through gdn_amd.ops, against the float64 restatement in
tests/pointwise_fp64.py (pinned without a GPU by tests/test_pointwise_fp64_cpu.py) at the training shapes: the capped grid of
LOSS_MAXBLK = 1024 blocks, its grid-stride loop and the ragged last pass.

    entry point          test
    -------------------  ---------------------------------------------------------------------------
    gdn_absdiff_max      test_absdiff_max, test_berhu_all_equal
    gdn_berhu_masked     test_berhu (sparse None / Cs 1 / Cs 2, default / explicit box, own / external maximum,
                         dout None / zero / pre-filled), test_berhu_all_equal
    gdn_sobel_l1         test_sobel (weight 1 / 3, plus + total, dpred None)
    gdn_smoothness       test_smoothness (Ci 1 / 3, the four plus / plus2 combinations, ddepth None)
    gdn_mse              test_mse (sizes, the four dtype masks), test_mse_accumulate_chain
    gdn_mse_grad         test_mse_grad (sizes, the eight dtype masks, gscale None / device scalar)

Inputs come in two kinds.  DYADIC: out / gt / depth are k/4, |k| <= 4, img is k/16: every Sobel sum, depth difference and
out - gt is exact in fp32, so every sgn() and every tie is decided as float64 decides it and gradients are compared at
EVERY pixel.  CONTINUOUS: seeded uniform (-1, 1); pixels whose L1 argument lies within the fp32 error band of zero
(pointwise_fp64.sobel_ambiguous / smooth_ambiguous) are left out of the gradient comparison, and their share is asserted
to be <= 5e-4 before anything is compared.

Bars, in units of EPS = 2^-24 (the relative error bound of one fp32 rounding); r counts roundings along the longest path:
  BerHu loss      r = 12 + 1: d 1; c = 0.2f * max 2.25 (0.2f itself 0.25, the fp32 maximum 1, the product 1); c*c 5.5; d*d 3;
                  their sum 6.5; / (2c) 9.75; w * rho with w = 0.3f 11.4; the sums are float64, + 1 for the store.
  BerHu gradient  continuous r = 8 (d / c 4.25, 3.0f / n 1, * w 1.67, * g 1), plus EPS * |dout| for the += when dout was
                  not zero.  Dyadic: 2 ulp where the linear branch is taken, 4 ulp in the quadratic branch.
  Sobel           dyadic: 2 ulp on loss and gradient (the stencil sums are exact, the gradient is weight / n times an
                  integer: 2 roundings).  Continuous loss: each |dy|, |dx| is off by at most the band ->
                  weight * 2 * band + EPS * loss, absolute; gradient 2 ulp outside the excluded pixels.
  smoothness      loss r = 6 + 2 * (Ci + 2) + 1: difference 1, product 1, expf 2 ulp = 4 EPS, its argument
                  -(sum_c |dI|) / Ci with Ci + 2 roundings times |argument| <= 2; gradient: (14 + 3 + 2.25 -> 20) EPS times
                  0.1 / n * sum |w| over the up to four weights that meet in a pixel.
  MSE             loss r = 4 + 1 (d 1, d*d 3, pair sum 4); an accumulate chain adds one rounding per call.
                  gradient r = 4 (coefficient, * gscale, a - b, product) + half a bf16 ulp when it is stored as bf16.
No bar is looser than tests/test_hip_kernels.py applies to the same quantity (1e-4 relative on losses, 1e-3 of the
largest element on gradients); `_no_looser` asserts that next to each derived bar.

Worst errors observed on an MI355X (also in DESIGN.md 4.1): BerHu loss 1.1 EPS (all-linear dyadic: 0 ulp), gradient 1 ulp
dyadic, 2.8 EPS continuous, the += increment 0.67 of its bar; Sobel loss 0 ulp dyadic, 0.73 EPS continuous, gradient 1 ulp,
excluded share <= 1.2e-4 (smoothness: 0); smoothness loss 1.3 EPS, gradient 0.21 of its bar; MSE loss 0.97 EPS, accumulate
chain 0.03 EPS, gradient 1.4 EPS (bf16: within the half ulp); absdiff_max and every `total` exactly equal.
"""
import numpy as np
import pytest
import torch

import pointwise_fp64 as R

pytestmark = pytest.mark.gpu

EPS = R.EPS32
CAP = 256 * 1024                                             # pixels one pass of the capped grid covers
SHAPES = [(20, 128, 416), (4, 228, 304), (3, 5, 7), (1, 1, 9), (1, 9, 1), (1, 1, 1),
          (1, 512, 512), (1, 511, 513), (1, 1, CAP + 1)]    # the last three: == cap, cap - 1 blocks' worth + ragged, cap + 1
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
KINDS = ["dyadic", "continuous"]
MAX_EXCLUDED = 5e-4
LATENT_WEIGHTS = (1.0, 2.5, 14.0, 12.0)
MSE_SIZES = [1, 3, 4, 5, 6, 7, 4 * CAP + 4 * 300 + 3]        # the last: more than one pass of the capped grid, n % 4 == 3


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dyadic(shape, seed, den=4):
    return torch.randint(-4, 5, shape, generator=_gen(seed)).float() / den


def _uniform(shape, seed):
    return torch.rand(shape, generator=_gen(seed)) * 2 - 1


def _draw(kind, shape, seed, den=4):
    return _dyadic(shape, seed, den) if kind == "dyadic" else _uniform(shape, seed)


def _report(what, value):
    print("FIGURE %-58s %.4g" % (what, value))


def _no_looser(bar, old):
    assert bar <= old, "derived bar %.3e is looser than the existing one %.3e" % (bar, old)


def _scalar(dev, v=float("nan")):
    return torch.full((), v, dtype=torch.float32, device=dev)


def _check_loss(got, ref, r, what, extra_abs=0.0):
    """|got - ref| <= r * EPS * |ref| + extra_abs (a loss built from non-negative fp32 terms summed in float64)."""
    bar = r * EPS * abs(ref) + extra_abs
    if ref:
        _no_looser(bar, 1e-4 * abs(ref))
    err = abs(float(got) - ref)
    _report(what + " |err|/EPS/|ref|", err / (EPS * abs(ref)) if ref else err)
    assert err <= bar, "%s: got %.9g, float64 %.9g, err %.3e > bar %.3e" % (what, float(got), ref, err, bar)


def _check_ulps(got, ref, bar, what, keep=None):
    """Element-wise distance to the once-rounded float64 result, in fp32 ulps; `bar` may be an array."""
    u = R.ulps_off(got, ref, R.F32)
    bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), u.shape)
    if keep is not None:
        u, bar = u[keep], bar[keep]
    _no_looser(float((bar * R.ulp(ref, R.F32).max()).max()) if u.size else 0.0, 1e-3 * float(np.abs(ref).max()) + 1e-30)
    worst = float(u.max()) if u.size else 0.0
    _report(what + " worst ulps", worst)
    bad = u > bar
    assert not bad.any(), "%s: %d of %d elements over the bar, worst %.2f ulp" % (what, int(bad.sum()), u.size, worst)


def _check_abs(got, ref, bar, what, keep=None, fp32=True):
    """fp32: the result is stored as fp32, the dtype the existing gradient bar (1e-3 of the largest element) was set for."""
    err = np.abs(R.f64(got) - ref)
    bar = np.broadcast_to(bar, err.shape)
    if keep is not None:
        err, bar = err[keep], bar[keep]
    if fp32:
        _no_looser(float(bar.max()) if err.size else 0.0, 1e-3 * float(np.abs(ref).max()) + 1e-30)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    _report(what + " worst err/bar", float(ratio.max()) if err.size else 0.0)
    bad = err > bar
    assert not bad.any(), "%s: %d of %d elements over the bar, worst err/bar %.3g" % (what, int(bad.sum()), err.size, float(ratio.max()))


def _excluded_ok(amb, what):
    share = float(amb.mean())
    _report(what + " excluded share", share)
    assert share <= MAX_EXCLUDED, "%s: %.3e of the pixels are ambiguous (cap %.1e): pick another seed" % (what, share, MAX_EXCLUDED)
    return ~amb


# ------------------------------------------------------------------------------------------------------ absdiff max
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_absdiff_max(gpu, shape, kind):
    """The maximum rounds nothing beyond the subtraction IEEE defines: exact equality with the float32 maximum."""
    from gdn_amd import ops
    B, H, W = shape
    a, b = _draw(kind, (B, 1, H, W), 101), _draw(kind, (B, 1, H, W), 102)
    # plant the maximum in the last pixel (the ragged tail of the last grid-stride pass) for one of the two kinds
    if kind == "dyadic":
        a.view(-1)[-1], b.view(-1)[-1] = 1.25, -1.25
    m = ops.absdiff_max(a.to(gpu), b.to(gpu))
    want = (a - b).abs().max()                                  # IEEE float32 on the CPU
    assert m.cpu().item() == want.item()
    if kind == "dyadic":
        assert want.item() == np.abs(R.f64(a) - R.f64(b)).max()      # ... which is the exact maximum here


# ------------------------------------------------------------------------------------------------------------ BerHu
def _sparse(kind, B, H, W, Cs, seed):
    """Channel 0: -1 (no measurement) on about half the pixels, a depth in (-1, 1] elsewhere.  Channel 1 (Cs == 2): a
    value that would flip EVERY weight if the kernel read it in place of channel 0."""
    hole = torch.rand((B, 1, H, W), generator=_gen(seed)) < 0.5
    v = _dyadic((B, 1, H, W), seed + 1).clamp(min=-0.75) if kind == "dyadic" else _uniform((B, 1, H, W), seed + 1) * 0.999
    s0 = torch.where(hole, torch.tensor(-1.0), v)
    if Cs == 1:
        return s0
    return torch.cat((s0, torch.where(s0 > -1, torch.tensor(-1.0), torch.tensor(0.5))), 1).contiguous()


def _off_centre_box(H, W):
    return (H // 5, H - H // 4, W // 3, W - W // 7)


# (name, Cs, box: None = the kernel's default (whole image) / "kitti" / "off" (off-centre), external maximum factor,
#  dout: None / "zero" / "filled")
BERHU_VARIANTS = [("plain", 0, None, None, "zero"), ("cs1-defaultbox", 1, None, None, "zero"),
                  ("cs2-offbox-filled", 2, "off", None, "filled"), ("cs1-kitti-extmax", 1, "kitti", 1.5, "zero"),
                  ("cs2-value-only", 2, "off", None, None), ("all-linear", 0, None, 5.0, "zero")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_berhu(gpu, shape, kind):
    from gdn_amd import ops
    B, H, W = shape
    n = B * H * W
    out, gt = _draw(kind, (B, 1, H, W), 11), _draw(kind, (B, 1, H, W), 12)
    if n > 1:
        out.view(-1)[-1], gt.view(-1)[-1] = 1.0, -1.0          # the maximum sits in the ragged tail of the last pass
    else:
        out.view(-1)[0], gt.view(-1)[0] = 0.75, -0.5           # (one pixel: keep it off out == gt, see test_berhu_all_equal)
    max32 = (out - gt).abs().max()
    od, gd = out.to(gpu), gt.to(gpu)
    for name, Cs, boxed, ext, fill in BERHU_VARIANTS:
        what = "berhu %s %s %s" % (SHAPE_IDS[SHAPES.index(shape)], kind, name)
        sparse = _sparse(kind, B, H, W, Cs, 13) if Cs else None
        box = {None: None, "kitti": R.crop_box_kitti(H, W), "off": _off_centre_box(H, W)}[boxed]
        ref_box = (0, H, 0, W) if box is None else box           # a NULL box means the whole image to the kernel
        extv = None if ext is None else (max32 * ext).float()
        before = None
        if fill == "zero":
            before = torch.zeros(B, 1, H, W)
        elif fill == "filled":
            before = _uniform((B, 1, H, W), 14) * (4.0 / n)    # the size of the gradient itself: the += must keep both
        dd = None if before is None else before.clone().to(gpu)
        loss = _scalar(gpu)
        ops.berhu_masked(od, gd, None if sparse is None else sparse.to(gpu), box, dd, loss,
                         ext_max=None if extv is None else extv.to(gpu))
        ref_loss, ref_grad, c = R.berhu(out, gt, sparse, ref_box, None if extv is None else extv)
        if name == "all-linear" and kind == "dyadic":
            # c >= max|d|: loss = 3 * mean|d| with every term exact: 2 ulp (the float64 sum times 3/n, one store)
            assert not (np.abs(R.f64(out) - R.f64(gt)) > c).any()
            _check_ulps(loss.cpu(), np.asarray(ref_loss), 2, what + " loss")
        else:
            _check_loss(loss.cpu(), ref_loss, 12 + 1, what + " loss")
        if dd is None:
            continue
        after = dd.cpu()
        if fill == "filled":
            # contract: dout += gradient.  after = fl(before + t) with t the kernel's term: the increment is the gradient
            # up to t's own error (r = 8) and the one rounding of the addition, EPS * |after|
            want = R.f64(before) + ref_grad
            _check_abs(R.f64(after) - R.f64(before), ref_grad, 8.01 * EPS * np.abs(ref_grad) + EPS * np.abs(want),
                       what + " dout_after - dout_before")
        elif kind == "dyadic":
            quad = np.abs(R.f64(out) - R.f64(gt)) > c
            _check_ulps(after, ref_grad, np.where(quad, 4.0, 2.0), what + " grad")       # nothing excluded
        else:
            _check_abs(after, ref_grad, 8 * EPS * np.abs(ref_grad), what + " grad")      # r = 8, nothing excluded


def test_berhu_all_equal(gpu):
    """out == gt everywhere: c = 0, and the quadratic branch -- unused, |d| > c is false at every pixel -- divides 0 by 0.
    The float64 reference evaluates that branch to NaN by construction and then SELECTS the linear one (np.where), so its
    value and gradient are 0; torch.where's autograd multiplies the NaN by a zero mask instead, so the oracle's gradient is
    NaN here and is not consulted.  The kernel takes the linear branch: loss 0, gradient 0, and a maximum of +0.0."""
    from gdn_amd import ops
    x = _uniform((3, 1, 5, 7), 21)
    xd = x.to(gpu)
    ref_loss, ref_grad, c = R.berhu(x, x.clone())
    assert c == 0.0 and ref_loss == 0.0 and not ref_grad.any()
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.zeros(1) / (2.0 * c))                  # the unused branch
    m = ops.absdiff_max(xd, xd.clone())
    assert m.cpu().item() == 0.0 and not np.signbit(m.cpu().numpy())
    loss, dout = _scalar(gpu), torch.zeros_like(xd)
    ops.berhu_masked(xd, xd.clone(), None, None, dout, loss)
    assert loss.cpu().item() == 0.0
    assert torch.equal(dout.cpu(), torch.zeros(3, 1, 5, 7))


# ------------------------------------------------------------------------------------------------------------ Sobel
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_sobel(gpu, shape, kind):
    from gdn_amd import ops
    B, H, W = shape
    n = B * H * W
    pred, gt = _draw(kind, (B, 1, H, W), 31), _draw(kind, (B, 1, H, W), 32)
    pd, gd = pred.to(gpu), gt.to(gpu)
    keep = None
    if kind == "continuous":
        keep = _excluded_ok(R.sobel_ambiguous(pred, gt), "sobel %s" % SHAPE_IDS[SHAPES.index(shape)])      # asserted FIRST
    for weight, with_total, with_grad in ((1.0, False, True), (3.0, True, True), (3.0, True, False), (1.0, False, False)):
        what = "sobel %s %s w%g%s%s" % (SHAPE_IDS[SHAPES.index(shape)], kind, weight, " total" if with_total else "",
                                       "" if with_grad else " value-only")
        loss, total, plus = _scalar(gpu), _scalar(gpu), _scalar(gpu, 0.8125 if kind == "dyadic" else 0.7310486)
        dp = torch.zeros(B, 1, H, W, device=gpu) if with_grad else None
        ops.sobel_l1(pd, gd, weight, dp, loss, plus=plus if with_total else None, total=total if with_total else None)
        ref_loss, ref_grad = R.sobel_l1(pred, gt, weight)
        if kind == "dyadic":
            _check_ulps(loss.cpu(), np.asarray(ref_loss), 2, what + " loss")
        else:
            # each of the 2n terms |dy|, |dx| is off by at most its band (<= SOBEL_BAND): the mean over n pixels by at most
            # mean(by + bx) <= 2 * band; + the store
            by, bx, _, _ = R.sobel_bands(pred, gt)
            _check_loss(loss.cpu(), ref_loss, 1, what + " loss", extra_abs=weight * float((by + bx).mean()))
        if with_total:
            assert total.cpu().numpy() == np.float32(loss.cpu().numpy() + plus.cpu().numpy()), what + ": total != float32(loss + plus)"
        if with_grad:
            _check_ulps(dp.cpu(), ref_grad, 2, what + " grad", keep=keep)      # dyadic: keep is None, every pixel compared


# ------------------------------------------------------------------------------------------------------- smoothness
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_smoothness(gpu, shape, kind):
    from gdn_amd import ops
    B, H, W = shape
    depth = _draw(kind, (B, 1, H, W), 41)
    dd = depth.to(gpu)
    keep = None
    if kind == "continuous":
        keep = _excluded_ok(R.smooth_ambiguous(depth), "smooth %s" % SHAPE_IDS[SHAPES.index(shape)])       # asserted FIRST
    combos = [(3, False, False, True), (3, True, False, True), (1, False, True, True), (1, True, True, True), (3, True, True, False)]
    for Ci, with_plus, with_plus2, with_grad in combos:
        what = "smooth %s %s Ci%d%s%s%s" % (SHAPE_IDS[SHAPES.index(shape)], kind, Ci, " plus" if with_plus else "",
                                           " plus2" if with_plus2 else "", "" if with_grad else " value-only")
        img = _draw(kind, (B, Ci, H, W), 42 + Ci, den=16)
        loss, total = _scalar(gpu), _scalar(gpu)
        plus, plus2 = _scalar(gpu, 1.5390625 if kind == "dyadic" else 1.2345678), _scalar(gpu, 0.3330001)
        g = torch.zeros(B, 1, H, W, device=gpu) if with_grad else None
        ops.smoothness(dd, img.to(gpu), g, loss, plus=plus if with_plus else None, plus2=plus2 if with_plus2 else None, total=total)
        ref_loss, ref_grad, ref_mag = R.smoothness(depth, img)
        # r = difference 1 + product 1 + expf 4 (2 ulp: the bound assumed for the device expf) + 2 * (Ci + 2) + store 1
        _check_loss(loss.cpu(), ref_loss, 6 + 2 * (Ci + 2) + 1, what + " loss")
        lo = loss.cpu().numpy()
        t = (np.float32(lo + plus.cpu().numpy()) if with_plus else lo) + (plus2.cpu().numpy() if with_plus2 else np.float32(0))
        assert total.cpu().numpy() == np.float32(t), what + ": total != (loss + plus) + plus2 in float32"
        if with_grad:
            _check_abs(g.cpu(), ref_grad, 20 * EPS * ref_mag, what + " grad", keep=keep)


# -------------------------------------------------------------------------------------------------------------- MSE
def _operand(x, bf16):
    return x.bfloat16() if bf16 else x


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
def test_mse(gpu, mask):
    """Includes n = 3 < 4: no vector iteration, the scalar tail starts at element 0 and must add each element once."""
    from gdn_amd import ops
    for n in MSE_SIZES:
        a, b = _operand(_uniform((n,), 51), mask & 1), _operand(_uniform((n,), 52), mask & 2)
        loss = _scalar(gpu)
        ops.mse_accum(a.to(gpu), b.to(gpu), 0.9375, loss, accumulate=False)
        # r = 4 + 1: d 1, d*d 3, the sum of a pair 4 (the rest of the sum is float64), store 1
        _check_loss(loss.cpu(), R.mse(a, b, 0.9375), 5, "mse n=%d mask=%d" % (n, mask))
    # dyadic, n = 3 and n = 7: every term exact, the result is the rounded float64 value
    for n in (3, 7):
        a, b = _operand(_dyadic((n,), 53), mask & 1), _operand(_dyadic((n,), 54), mask & 2)
        loss = _scalar(gpu)
        ops.mse_accum(a.to(gpu), b.to(gpu), 1.0, loss, accumulate=False)
        assert loss.cpu().numpy() == np.float32(R.mse(a, b, 1.0)), "mse dyadic n=%d: tail elements not summed once each" % n


@pytest.mark.parametrize("bf16", [False, True])
def test_mse_accumulate_chain(gpu, bf16):
    """The four calls latent_loss issues: weights 1.5 * w / 4 for w in LATENT_WEIGHTS, accumulate from the second on."""
    from gdn_amd import ops
    loss = _scalar(gpu)
    ref = 0.0
    for i, (w, c) in enumerate(zip(LATENT_WEIGHTS, (8, 16, 32, 33))):
        a, b = _operand(_uniform((2, c, 6, 11), 61 + i), bf16), _operand(_uniform((2, c, 6, 11), 71 + i), bf16)
        ops.mse_accum(a.to(gpu), b.to(gpu), 1.5 * w / 4.0, loss, accumulate=i > 0)
        ref += R.mse(a, b, 1.5 * w / 4.0)
    _check_loss(loss.cpu(), ref, 5 + 3, "mse accumulate chain bf16=%s" % bf16)      # + one rounding per accumulating call


@pytest.mark.parametrize("gscale", [None, 0.7], ids=["noscale", "gscale"])
@pytest.mark.parametrize("mask", list(range(8)))
def test_mse_grad(gpu, mask, gscale):
    from gdn_amd import ops
    out_dt = torch.bfloat16 if mask & 4 else torch.float32
    gs = None if gscale is None else torch.tensor(gscale, dtype=torch.float32, device=gpu)
    for n in MSE_SIZES:
        a, b = _operand(_uniform((n,), 81), mask & 1), _operand(_uniform((n,), 82), mask & 2)
        da = ops.mse_grad(a.to(gpu), b.to(gpu), 2.5, gs, out_dtype=out_dt)
        assert da.dtype == out_dt and da.shape == a.shape
        ref = R.mse_grad(a, b, 2.5, 1.0 if gs is None else float(gs.cpu()))
        # r = 4: the coefficient 2w/n, its product with gscale, a - b, the product; a bf16 store adds half a bf16 ulp
        bar = 4 * EPS * np.abs(ref) + (0.5 * R.ulp(ref, R.BF16) if mask & 4 else 0.0)
        _check_abs(da.cpu(), ref, bar, "mse_grad n=%d mask=%d %s" % (n, mask, "gscale" if gs is not None else "noscale"),
                   fp32=not mask & 4)
