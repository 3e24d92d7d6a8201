"""Float64 restatement of the scale-invariant log loss (gdn_silog_masked), written from the formula:

    t(x) = (x + 1) / 2,  u(x) = max(t(x), floor)
    a pixel is valid iff t(gt) > floor and, with a sparse map, it lies inside box = (y1, y2, x1, x2) with sparse[:, 0] > -1
    d_i = log u(out_i) - log u(gt_i) over the n valid pixels,  m1 = sum d / n,  m2 = sum d^2 / n,  D = m2 - lambda * m1^2
    loss = weight * sqrt(D)
    dloss/dout_i = weight / (sqrt(D) * n) * (d_i - lambda * m1) / (out_i + 1)   where pixel i is valid and t(out_i) > floor
    n == 0 or D <= 0: loss 0, gradient 0.

No GPU code and nothing from gdn_amd: this is the yardstick tests/test_hip_silog.py holds the kernel to, and
tests/test_silog_cpu.py pins it against torch's float64 autograd and a case worked by hand.

Conventions
  * out / gt / sparse are taken as they are stored: float32 tensors (torch or numpy), upcast to float64, which is exact; both
    comparisons are evaluated on (float64(x) + 1) / 2;
  * lambda, weight and floor are taken as the C ABI carries them, float32 scalars, upcast likewise (`scalars`);
  * the three sums are exact (math.fsum), so the reference's own error is the handful of float64 roundings per pixel;
  * a NaN prediction at a valid pixel stays a NaN (max() written as a selection that lets it through), an invalid pixel's
    prediction is never looked at.
"""
import math

import numpy as np

EPS32 = 2.0 ** -24          # relative error bound of ONE round-to-nearest fp32 operation
BAND = EPS32                # |t(x) - floor| <= BAND: a float32 evaluation of t(x) > floor may decide otherwise (t is off by
#                             at most EPS32 * |x + 1| / 2 <= EPS32, the float32 floor by less)


def f64(x):
    if x is None:
        return None
    if hasattr(x, "detach"):
        import torch
        return x.detach().to("cpu").to(torch.float64).numpy()
    return np.asarray(x, dtype=np.float64)


def scalars(lam, weight, floor):
    """(lambda, weight, floor) as float64 values of the float32 scalars the entry point is handed."""
    return tuple(float(np.float32(v)) for v in (lam, weight, floor))


def valid_mask(gt, sparse=None, box=None, floor=0.0125):
    g = f64(gt)
    fl = scalars(0.0, 1.0, floor)[2]
    valid = (g + 1.0) * 0.5 > fl
    if sparse is not None:
        y1, y2, x1, x2 = box
        crop = np.zeros(g.shape, dtype=bool)
        crop[:, :, y1:y2, x1:x2] = True
        valid &= crop & (f64(sparse)[:, 0:1] > -1.0)
    return valid


def ambiguous(x, floor=0.0125, band=BAND):
    """True where t(x) lies within `band` of the floor."""
    return np.abs((f64(x) + 1.0) * 0.5 - scalars(0.0, 1.0, floor)[2]) <= band


def _fsum(v):
    try:
        return math.fsum(v.tolist())
    except (ValueError, OverflowError):          # +inf and -inf among the terms
        return float("nan")


def silog(out, gt, sparse=None, box=None, lam=0.85, weight=10.0, floor=0.0125):
    """(loss, dloss/dout [B,1,H,W], (n, m1, m2, D)) in float64.  sparse given: box is required."""
    lam, weight, fl = scalars(lam, weight, floor)
    o, g = f64(out), f64(gt)
    valid = valid_mask(gt, sparse, box, floor)
    grad = np.zeros(o.shape)
    n = int(valid.sum())
    if n == 0:
        return 0.0, grad, (0.0, 0.0, 0.0, 0.0)
    ov, gv = o[valid], g[valid]
    to, tg = (ov + 1.0) * 0.5, (gv + 1.0) * 0.5
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.log(np.where(to < fl, fl, to)) - np.log(tg)
        m1, m2 = _fsum(d) / n, _fsum(d * d) / n
        D = m2 - lam * m1 * m1
        if D <= 0.0:
            return 0.0, grad, (float(n), m1, m2, D)
        r = math.sqrt(D) if D == D and D != float("inf") else float("nan") if D != D else float("inf")
        a, b = weight / (r * n), lam * m1
        live = ~(to <= fl)                           # (a NaN prediction is live: the gradient must show it)
        gv_ = np.where(live, a * (d - b) / (ov + 1.0), 0.0)
    grad[valid] = gv_
    return weight * r, grad, (float(n), m1, m2, D)
