"""gdn_silog_masked, called through gdn_amd.ops, against the float64 restatement in tests/silog_fp64.py (pinned without a GPU by
tests/test_silog_cpu.py) at the shapes of tests/test_hip_losses.py: the training shape, the capped grid of 1024 blocks, its
grid-stride loop and the ragged last pass.

Inputs come in two kinds.  GRID: x = k/64 - 1 with integer k in [0, 128]: x + 1 is exact and no t(x) = (x + 1) / 2 sits on
the floor 0.0125 (1/128 < 0.0125 < 2/128), so every validity and clamp decision is the same in float32 and float64 and every
pixel is compared.  CONTINUOUS: seeded uniform (-1, 1); the pixels whose t(out) or t(gt) lies within silog_fp64.BAND of the
floor are left out of the gradient comparison, and their share is asserted to be <= 5e-4 before anything is compared.

Bars (the kernel's per-pixel arithmetic and its sums are float64; EPS = 2^-24):
  loss                  1 ulp of float32 against the float64 value (one rounding, + the float64 noise at a rounding boundary)
  stats (n, m1, m2, D)  n exact, the others 1e-12 relative
  gradient, dout zero   1 ulp
  gradient, dout filled |after - (before + g)| <= ulp(g) / 2 + ulp(sum) / 2: the term's rounding and the addition's (the
                        comparison allows 2^-26 of the bar for the float64 arithmetic of the test itself: `want` and the
                        error are each rounded once at 2^-53 of the sum, 2^-27 of a bar that is 2^-25 of it or more)
lambda runs over 0, 0.5 and 0.85; weight over 0.5, 0.85 and 10 -- a weight of 0 is refused as a bad argument with the other
out-of-range values (test_bad_arguments).

Worst errors observed on an MI355X (also in DESIGN.md 4.1; every figure is printed as a FIGURE line): loss 0 ulp in all 73
comparisons, stats 1.5e-15 relative, gradient 0 ulp into a zeroed dout in all 36, 1.00 of the bar into a filled one (the
addition's own half ulp, reached where the term is far below the ulp of the sum), excluded share <= 9.4e-7 (grid: 0).
"""
import numpy as np
import pytest
import torch

import pointwise_fp64 as P
import silog_fp64 as R
from test_hip_losses import SHAPE_IDS, SHAPES

pytestmark = pytest.mark.gpu

KINDS = ["grid", "continuous"]
MAX_EXCLUDED = 5e-4
FLOOR = 0.0125
# (name, Cs, box: None / "kitti" / "off", dout: None / "zero" / "filled", lambda, weight)
VARIANTS = [("dense", 0, None, "zero", 0.85, 10.0), ("cs1-kitti-filled", 1, "kitti", "filled", 0.5, 0.5),
            ("cs3-offbox", 3, "off", "zero", 0.0, 0.85), ("cs3-value-only", 3, "off", None, 0.85, 10.0)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _draw(kind, shape, seed):
    if kind == "grid":
        return torch.randint(0, 129, shape, generator=_gen(seed)).float() / 64 - 1
    return torch.rand(shape, generator=_gen(seed)) * 2 - 1


def _sparse(kind, B, H, W, Cs, seed):
    """Channel 0: -1 (no return) on about half the pixels, a value above -1 elsewhere.  Channels 1.. (Cs == 3): values that
    would flip EVERY decision if the kernel read them in place of channel 0."""
    hole = torch.rand((B, 1, H, W), generator=_gen(seed)) < 0.5
    v = _draw(kind, (B, 1, H, W), seed + 1).clamp(min=-0.75)
    s0 = torch.where(hole, torch.tensor(-1.0), v)
    if Cs == 1:
        return s0
    flip = torch.where(s0 > -1, torch.tensor(-1.0), torch.tensor(0.5))
    return torch.cat([s0] + [flip] * (Cs - 1), 1).contiguous()


def _off_centre_box(H, W):
    return (H // 5, H - H // 4, W // 3, W - W // 7)


def _report(what, value):
    print("FIGURE %-64s %.4g" % (what, value))


def _scalar(dev, v=float("nan")):
    return torch.full((), v, dtype=torch.float32, device=dev)


def _check_loss(got, ref, what):
    u = float(P.ulps_off(got, np.asarray(ref), P.F32))
    _report(what + " loss ulps", u)
    assert u <= 1.0, "%s: loss %.9g, float64 %.17g, %.2f ulp" % (what, float(got), ref, u)


def _check_stats(got, ref, what):
    got = [float(v) for v in got]
    assert got[0] == ref[0], "%s: n %r != %r" % (what, got[0], ref[0])
    worst = 0.0
    for name, g, r in zip(("m1", "m2", "D"), got[1:], ref[1:]):
        rel = 0.0 if g == r else abs(g - r) / abs(r) if r else float("inf")
        worst = max(worst, rel)
        assert rel <= 1e-12, "%s: %s %.17g, float64 %.17g, relative %.3e" % (what, name, g, r, rel)
    _report(what + " stats worst relative", worst)


def _check_grad_ulps(got, ref, what, keep):
    u = P.ulps_off(got, ref, P.F32)[keep]
    worst = float(u.max()) if u.size else 0.0
    _report(what + " grad worst ulps", worst)
    assert worst <= 1.0, "%s: %d of %d gradient elements over 1 ulp, worst %.2f" % (what, int((u > 1).sum()), u.size, worst)


def _check_increment(after, before, ref, what, keep):
    want = P.f64(before) + ref
    a = P.f64(after)
    err = np.abs(a - want)
    bar = 0.5 * P.ulp(ref, P.F32) + 0.5 * np.maximum(P.ulp(want, P.F32), P.ulp(a, P.F32))
    ratio = (err / bar)[keep]
    worst = float(ratio.max()) if ratio.size else 0.0
    _report(what + " dout_after - (dout_before + g) worst err/bar", worst)
    assert worst <= 1.0 + 2.0 ** -26, "%s: %d elements over the bar, worst %.6f" % (what, int((ratio > 1 + 2.0 ** -26).sum()), worst)
    untouched = ref == 0.0
    assert np.array_equal(a[untouched], P.f64(before)[untouched]), what + ": a pixel without gradient was written"


def _case(gpu, kind, shape, variant, out, gt, od, gd):
    from gdn_amd import ops
    name, Cs, boxed, fill, lam, weight = variant
    B, H, W = shape
    n = B * H * W
    sparse = _sparse(kind, B, H, W, Cs, 13) if Cs else None
    box = {None: None, "kitti": P.crop_box_kitti(H, W), "off": _off_centre_box(H, W)}[boxed]
    if sparse is not None and box is None:
        box = (0, H, 0, W)
    before = None
    if fill == "zero":
        before = torch.zeros(B, 1, H, W)
    elif fill == "filled":
        before = (torch.rand((B, 1, H, W), generator=_gen(14)) * 2 - 1) * (weight * 4.0 / n)     # the size of the gradient itself
    dd = None if before is None else before.clone().to(gpu)
    loss, stats = _scalar(gpu), torch.full((4,), float("nan"), dtype=torch.float64, device=gpu)
    ops.silog_masked(od, gd, None if sparse is None else sparse.to(gpu), box, dd, loss, lam, weight, FLOOR, stats=stats)
    return name, fill, before, dd, loss, stats, R.silog(out, gt, sparse, box, lam, weight, FLOOR)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_silog(gpu, shape, kind):
    B, H, W = shape
    out, gt = _draw(kind, (B, 1, H, W), 11), _draw(kind, (B, 1, H, W), 12)
    amb = R.ambiguous(out, FLOOR) | R.ambiguous(gt, FLOOR)
    share = float(amb.mean())
    _report("silog %s %s excluded share" % (SHAPE_IDS[SHAPES.index(shape)], kind), share)
    assert share <= MAX_EXCLUDED                                  # asserted FIRST
    assert kind != "grid" or not amb.any()                        # grid inputs: every pixel is compared
    keep = ~amb
    od, gd = out.to(gpu), gt.to(gpu)
    for variant in VARIANTS:
        name, fill, before, dd, loss, stats, (ref_loss, ref_grad, ref_stats) = _case(gpu, kind, shape, variant, out, gt, od, gd)
        what = "silog %s %s %s" % (SHAPE_IDS[SHAPES.index(shape)], kind, name)
        _check_loss(loss.cpu(), ref_loss, what)
        _check_stats(stats.cpu().tolist(), ref_stats, what)
        if dd is None:
            continue
        if fill == "zero":
            _check_grad_ulps(dd.cpu(), ref_grad, what, keep)
            if kind == "grid":
                assert not dd.cpu().numpy()[ref_grad == 0.0].any()
        else:
            _check_increment(dd.cpu(), before, ref_grad, what, keep)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_degenerate_cases_leave_dout_alone(gpu):
    """No valid pixel (ground truth at the floor everywhere; a sparse map without a return) and out == gt: loss exactly 0 and
    dout -- pre-filled, a -0.0 and a NaN among its values -- keeps its bits.  Every prediction clamped: a loss, no gradient."""
    from gdn_amd import ops
    B, H, W = 3, 5, 7
    out, gt = _draw("continuous", (B, 1, H, W), 21), _draw("continuous", (B, 1, H, W), 22).clamp(min=-0.9)
    before = _draw("continuous", (B, 1, H, W), 23)
    before.view(-1)[0], before.view(-1)[1] = -0.0, float("nan")
    cases = [("gt at the floor", out, torch.full((B, 1, H, W), -1.0), None, None),
             ("no return", out, gt, torch.full((B, 1, H, W), -1.0), (0, H, 0, W)),
             ("empty box", out, gt, torch.zeros(B, 1, H, W), (2, 2, 0, W)),
             ("out == gt", gt.clone(), gt, None, None)]
    for what, o, g, sparse, box in cases:
        dd, loss = before.clone().to(gpu), _scalar(gpu)
        stats = torch.full((4,), float("nan"), dtype=torch.float64, device=gpu)
        ops.silog_masked(o.to(gpu), g.to(gpu), None if sparse is None else sparse.to(gpu), box, dd, loss, 0.85, 10.0, FLOOR, stats=stats)
        assert loss.cpu().item() == 0.0 and not np.signbit(loss.cpu().numpy()), what
        assert torch.equal(_bits(dd), _bits(before)), what
        ref = R.silog(o, g, sparse, box, 0.85, 10.0, FLOOR)
        assert ref[0] == 0.0 and stats.cpu().tolist() == list(ref[2]), what
    clamped = torch.full((B, 1, H, W), -0.99)
    dd, loss = before.clone().to(gpu), _scalar(gpu)
    ops.silog_masked(clamped.to(gpu), gt.to(gpu), None, None, dd, loss, 0.85, 10.0, FLOOR)
    ref_loss, ref_grad, _ = R.silog(clamped, gt, None, None, 0.85, 10.0, FLOOR)
    assert ref_loss > 0 and not ref_grad.any()
    _check_loss(loss.cpu(), ref_loss, "every prediction clamped")
    assert torch.equal(_bits(dd), _bits(before))


def test_nonfinite_prediction(gpu):
    """A NaN (or +Inf) prediction at a valid pixel: the loss and the gradient of every valid pixel are non-finite -- what
    --skip_nonfinite has to see.  The same value at an invalid pixel changes nothing, bit for bit."""
    from gdn_amd import ops
    B, H, W = 2, 6, 9
    out, gt = _draw("continuous", (B, 1, H, W), 31), _draw("continuous", (B, 1, H, W), 32).clamp(min=-0.9)
    gt.view(-1)[5] = -1.0                                           # the invalid pixel
    od, gd = out.to(gpu), gt.to(gpu)
    d0, l0 = torch.zeros(B, 1, H, W, device=gpu), _scalar(gpu)
    ops.silog_masked(od, gd, None, None, d0, l0, 0.85, 10.0, FLOOR)
    assert np.isfinite(l0.cpu().item()) and l0.cpu().item() > 0 and d0.cpu()[0, 0, 0, 5] == 0
    valid = torch.from_numpy(R.valid_mask(gt, None, None, FLOOR))
    for bad in (float("nan"), float("inf")):
        o = out.clone()
        o.view(-1)[5] = bad
        d1, l1 = torch.zeros(B, 1, H, W, device=gpu), _scalar(gpu)
        ops.silog_masked(o.to(gpu), gd, None, None, d1, l1, 0.85, 10.0, FLOOR)
        assert torch.equal(_bits(l1), _bits(l0)) and torch.equal(_bits(d1), _bits(d0)), "an invalid pixel's prediction was read"
        o = out.clone()
        o.view(-1)[7] = bad
        assert valid.view(-1)[7]
        d2, l2 = torch.zeros(B, 1, H, W, device=gpu), _scalar(gpu)
        ops.silog_masked(o.to(gpu), gd, None, None, d2, l2, 0.85, 10.0, FLOOR)
        assert not np.isfinite(l2.cpu().item())
        live = valid & ((o.double() + 1) / 2 > float(np.float32(FLOOR))).logical_or(torch.isnan(o))
        assert not torch.isfinite(d2.cpu()[live]).any() and live.sum() > 50
        assert not d2.cpu()[~valid].any()
        ref_loss, ref_grad, _ = R.silog(o, gt, None, None, 0.85, 10.0, FLOOR)
        assert ref_loss != ref_loss and np.isnan(ref_grad[live.numpy()]).all()


@pytest.mark.parametrize("shape", [(20, 128, 416), (1, 511, 513)], ids=["20x128x416", "1x511x513"])
def test_two_calls_give_identical_bits(gpu, shape):
    from gdn_amd import ops
    B, H, W = shape
    od, gd = _draw("continuous", (B, 1, H, W), 41).to(gpu), _draw("continuous", (B, 1, H, W), 42).to(gpu)
    sparse = _sparse("continuous", B, H, W, 1, 43).to(gpu)
    runs = []
    for _ in range(2):
        dd, loss = torch.zeros(B, 1, H, W, device=gpu), _scalar(gpu)
        stats = torch.zeros(4, dtype=torch.float64, device=gpu)
        ops.silog_masked(od, gd, sparse, P.crop_box_kitti(H, W), dd, loss, 0.85, 10.0, FLOOR, stats=stats)
        runs.append((_bits(dd), _bits(loss), stats.cpu().view(torch.int64)))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert runs[0][0].any()


def test_bad_arguments(gpu):
    from gdn_amd import ops
    from gdn_amd._lib import GdnError
    x = torch.zeros(1, 1, 4, 6, device=gpu)
    dd, loss = torch.zeros_like(x), _scalar(gpu, 7.0)
    for lam, weight, floor in ((1.0, 10.0, FLOOR), (-0.1, 10.0, FLOOR), (float("nan"), 10.0, FLOOR), (0.85, 0.0, FLOOR),
                               (0.85, -1.0, FLOOR), (0.85, 10.0, 0.0), (0.85, 10.0, 1.0)):
        with pytest.raises(GdnError, match="gdn_silog_masked failed"):
            ops.silog_masked(x, x, None, None, dd, loss, lam, weight, floor)
    with pytest.raises(GdnError, match="gdn_silog_masked failed"):
        ops.silog_masked(x, x, x, None, dd, loss, 0.85, 10.0, FLOOR)              # a sparse map without its box
    with pytest.raises(GdnError, match="stats"):
        ops.silog_masked(x, x, None, None, dd, loss, 0.85, 10.0, FLOOR, stats=torch.zeros(4, device=gpu))
    assert loss.cpu().item() == 7.0 and not dd.cpu().any()                         # nothing was launched


@pytest.mark.parametrize("kind", KINDS)
def test_total_chain(gpu, kind):
    """dtod_loss(pixel=spec): parts[0] is the SILog value (the bits of a call of its own), the returned loss is
    float32(silog + 3 * sobel) exactly, and the gradient buffer holds both terms; rtod_pixel_loss likewise with plus."""
    from gdn_amd import ops
    from gdn_amd import utils as U
    B, H, W = 2, 16, 32
    out, gt = _draw(kind, (B, 1, H, W), 51).to(gpu), _draw(kind, (B, 1, H, W), 52).to(gpu)
    sparse, rgb = _sparse(kind, B, H, W, 1, 53).to(gpu), _draw("continuous", (B, 3, H, W), 54).to(gpu)
    for use_sparse in (False, True):
        spec = U.silog_spec(0.5, 0.85, FLOOR, use_sparse)
        alone, d_alone = _scalar(gpu), torch.zeros(B, 1, H, W, device=gpu)
        ops.silog_masked(out, gt, sparse if use_sparse else None, U.crop_box_kitti(H, W) if use_sparse else None, d_alone, alone,
                         0.5, 0.85, FLOOR)
        pred = out.clone().requires_grad_(True)
        total, p0, p1 = U.dtod_loss(pred, gt, sparse, pixel=spec)
        assert torch.equal(_bits(p0), _bits(alone))
        sob, d_sob = _scalar(gpu), torch.zeros(B, 1, H, W, device=gpu)
        ops.sobel_l1(out, gt, 3.0, d_sob, sob)
        assert torch.equal(_bits(p1), _bits(sob))
        assert total.detach().cpu().numpy() == np.float32(p0.cpu().numpy() + p1.cpu().numpy())
        total.backward()
        both = d_alone.clone()
        ops.sobel_l1(out, gt, 3.0, both, _scalar(gpu))
        assert torch.equal(_bits(pred.grad), _bits(both))
        # the stand-alone loss kind
        pred2 = out.clone().requires_grad_(True)
        one = U.silog_loss(pred2, gt, sparse if use_sparse else None, lam=0.5, weight=0.85, floor=FLOOR)
        assert torch.equal(_bits(one), _bits(alone))
        one.backward()
        assert torch.equal(_bits(pred2.grad), _bits(d_alone))
        plus = _scalar(gpu, 0.7310486)
        t2, q0, q1 = U.rtod_pixel_loss(out, gt, rgb, sparse, plus=plus, pixel=spec)
        assert torch.equal(_bits(q0), _bits(alone))
        assert t2.cpu().numpy() == np.float32(np.float32(q0.cpu().numpy() + q1.cpu().numpy()) + plus.cpu().numpy())
