"""Float64 restatement of the per-pixel losses (csrc/losses.hip) and of the BatchNorm / elementwise kernels
(csrc/pointwise.hip), written from the formulas in the kernels' header comments and in oracle/gdn_oracle.py.

No GPU code and nothing from gdn_amd: this is the yardstick tests/test_hip_losses.py and tests/test_hip_pointwise.py
hold the kernels to, and tests/test_pointwise_fp64_cpu.py pins it against the reference-generated goldens, the torch
oracle and torch's float64 autograd.

Conventions
  * inputs are taken as they are stored: fp32 / bf16 tensors (torch or numpy) are upcast to float64, which is exact;
  * every function returns float64 numpy arrays (or Python floats); a test rounds them ONCE to the dtype the kernel
    stores (round_to) and measures the distance in units in the last place of that dtype (ulps_off);
  * loss tensors are NCHW [B,C,H,W], BatchNorm tensors NHWC [..., C] with per-channel vectors [C].
"""
import numpy as np

F32, BF16 = "f32", "bf16"
EPS32 = 2.0 ** -24          # relative error bound of ONE round-to-nearest fp32 operation


def f64(x):
    """torch tensor (any device / float dtype) or array -> float64 numpy array (exact for fp32 and bf16)."""
    if x is None:
        return None
    if hasattr(x, "detach"):
        import torch
        return x.detach().to("cpu").to(torch.float64).numpy()
    return np.asarray(x, dtype=np.float64)


# ---------------------------------------------------------------------------------------------- rounding and ulps
def round_bf16(x):
    """float64 -> nearest bfloat16 (ties to even), returned as float64 holding bf16 values.  One rounding, done by hand:
    going through fp32 first would round twice.  8 significant bits, exponent range of fp32, subnormals kept."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(np.abs(x))                       # |x| = m * 2^e, m in [0.5, 1)
    e = np.maximum(e, -125)                          # below 2^-126 the spacing stays that of the subnormals
    q = np.ldexp(1.0, e - 8)                         # spacing of bf16 around |x|
    r = np.rint(np.abs(x) / q) * q                   # np.rint rounds halves to even; the quotient is exact
    r = np.where(r >= 2.0 ** 128, np.inf, r)
    r = np.where(np.isfinite(x), r, np.abs(x))
    return np.copysign(r, x)


def round_to(x, dtype):
    if dtype == BF16:
        return round_bf16(x)
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def ulp(x, dtype):
    """Spacing of `dtype` at |x| (that of the smallest normal for anything below it)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(x)
    e = np.where(x == 0.0, -1000, e)                 # (frexp gives exponent 0 for zero)
    return np.ldexp(1.0, np.maximum(e - 1, -126) - (7 if dtype == BF16 else 23))


def near_bf16_boundary(x):
    """True where x lies within 2^-24 (relative) of the midpoint of two neighbouring bf16 values: an fp32 intermediate
    that is off by one fp32 rounding may then fall to the other side and store the neighbour."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    u = ulp(x, BF16)
    t = x / u
    return np.abs((t - np.floor(t)) - 0.5) * u <= EPS32 * x


def ulps_off(got, ref, dtype):
    """|got - round(ref)| in ulps of `dtype`, element-wise; ref is the unrounded float64 result."""
    r = round_to(ref, dtype)
    g = f64(got)
    with np.errstate(invalid="ignore"):
        d = np.abs(g - r) / ulp(r, dtype)
    return np.where(g == r, 0.0, d)                  # (inf == inf)


def ulp_bar(ref, dtype, bar):
    """The per-element bar in ulps: `bar`, plus ONE where a bf16 result sits on a rounding boundary (near_bf16_boundary).
    This is the only place that rule lives."""
    if dtype == BF16:
        return bar + near_bf16_boundary(ref).astype(np.float64)
    return np.full(np.shape(ref), float(bar))


# ---------------------------------------------------------------------------------------------------------- losses
def crop_box_kitti(H, W):
    """The Garg crop of the training loss mask (oracle.crop_box_kitti)."""
    return (int(0.40810811 * H), int(0.99189189 * H), int(0.03594771 * W), int(0.96405229 * W))


def berhu_weights(shape, sparse, box):
    """1 inside the box where sparse[:, 0] > -1, 0.3 inside elsewhere, 0.1 outside; all 1 without a sparse tensor.
    The kernel holds 0.3 and 0.1 as fp32 constants, which is part of ITS rounding budget, not of this formula."""
    B, _, H, W = shape
    w = np.ones(shape)
    if sparse is not None:
        y1, y2, x1, x2 = crop_box_kitti(H, W) if box is None else box
        crop = np.zeros(shape, dtype=bool)
        crop[:, :, y1:y2, x1:x2] = True
        valid = f64(sparse)[:, 0:1] > -1.0
        w = np.where(crop, np.where(valid, 1.0, 0.3), 0.1)
    return w


def berhu(out, gt, sparse=None, box=None, ext_max=None):
    """(loss, dloss/dout, c): d = out - gt, c = 0.2 * max|d| (or 0.2 * ext_max), rho = |d| where |d| <= c else
    (d^2 + c^2) / (2c), loss = 3 * mean(w * rho).  c carries no gradient.  With out == gt everywhere c is 0 and the quadratic
    branch is 0 / 0 = NaN by construction, but it is unused (|d| > c is false) and np.where selects: loss 0, gradient 0."""
    o, g = f64(out), f64(gt)
    d = o - g
    a = np.abs(d)
    c = 0.2 * (float(a.max()) if ext_max is None else float(f64(ext_max)))
    with np.errstate(divide="ignore", invalid="ignore"):
        quad, gquad = (d * d + c * c) / (2.0 * c), d / c
    big = a > c
    rho = np.where(big, quad, a)
    grad = np.where(big, gquad, np.sign(d))
    w = berhu_weights(d.shape, sparse, box)
    n = d.size
    return float(3.0 * (w * rho).sum() / n), 3.0 * w * grad / n, c


_SOBEL_Y = np.array([[1., 2., 1.], [0., 0., 0.], [-1., -2., -1.]])
_SOBEL_X = np.array([[1., 0., -1.], [2., 0., -2.], [1., 0., -1.]])


def _corr3(x, f):
    """3x3 cross-correlation with zero padding 1 over the last two axes."""
    H, W = x.shape[-2:]
    p = np.zeros(x.shape[:-2] + (H + 2, W + 2))
    p[..., 1:-1, 1:-1] = x
    o = np.zeros_like(x)
    for i in range(3):
        for j in range(3):
            if f[i][j]:
                o += f[i][j] * p[..., i:i + H, j:j + W]
    return o


def _corr3_adjoint(s, f):
    """Adjoint of _corr3: in[y, x] receives f[i][j] * s[y - i + 1, x - j + 1]."""
    H, W = s.shape[-2:]
    p = np.zeros(s.shape[:-2] + (H + 2, W + 2))
    p[..., 1:-1, 1:-1] = s
    o = np.zeros_like(s)
    for i in range(3):
        for j in range(3):
            if f[i][j]:
                o += f[i][j] * p[..., 2 - i:2 - i + H, 2 - j:2 - j + W]
    return o


def sobel_args(pred, gt):
    """(dy, dx): Sobel response of pred minus that of gt, the two arguments of the L1 norm."""
    p, g = f64(pred), f64(gt)
    return _corr3(p, _SOBEL_Y) - _corr3(g, _SOBEL_Y), _corr3(p, _SOBEL_X) - _corr3(g, _SOBEL_X)


def sobel_l1(pred, gt, weight=1.0):
    """(loss, dloss/dpred): weight * (mean|dy| + mean|dx|), sgn(0) = 0 as torch's abs."""
    dy, dx = sobel_args(pred, gt)
    n = dy.size
    loss = weight * (np.abs(dy).sum() + np.abs(dx).sum()) / n
    grad = (weight / n) * (_corr3_adjoint(np.sign(dy), _SOBEL_Y) + _corr3_adjoint(np.sign(dx), _SOBEL_X))
    return float(loss), grad


def _dilate(mask, up, down, left, right):
    """mask OR its shifts: result[y, x] = any mask[y + a, x + b], a in [-up, down], b in [-left, right]."""
    H, W = mask.shape[-2:]
    o = np.zeros_like(mask)
    for a in range(-up, down + 1):
        for b in range(-left, right + 1):
            ys, yd = (slice(a, H), slice(0, H - a)) if a >= 0 else (slice(0, H + a), slice(-a, H))
            xs, xd = (slice(b, W), slice(0, W - b)) if b >= 0 else (slice(0, W + b), slice(-b, W))
            if 0 <= abs(a) < H and 0 <= abs(b) < W:
                o[..., yd, xd] |= mask[..., ys, xs]
    return o


SOBEL_BAND = 32 * EPS32 * 16        # worst-case sum |tap| * |input| over both images is 16; 32 roundings of headroom
SMOOTH_BAND = 4 * EPS32 * 2         # one subtraction of values in (-1, 1), the same headroom per operation


def sobel_bands(pred, gt, band=SOBEL_BAND):
    """Per-pixel fp32 error band of the two Sobel arguments (by, bx) and the tap-weighted input magnitudes (sy, sx).
    `band` is the worst case over inputs in (-1, 1); where the taps meet smaller values the same count of roundings
    gives a smaller band, 32 * 2^-24 * sum |tap| * |input|, and the smaller one is used -- in particular an argument all
    of whose taps fall on the zero padding (the vertical response of a one-row image) is exactly zero in any arithmetic."""
    p, g = np.abs(f64(pred)), np.abs(f64(gt))
    sy = _corr3(p, np.abs(_SOBEL_Y)) + _corr3(g, np.abs(_SOBEL_Y))
    sx = _corr3(p, np.abs(_SOBEL_X)) + _corr3(g, np.abs(_SOBEL_X))
    return np.minimum(band, 32 * EPS32 * sy), np.minimum(band, 32 * EPS32 * sx), sy, sx


def sobel_ambiguous(pred, gt, band=SOBEL_BAND):
    """Pixels whose gradient may legitimately differ between fp32 and float64: a Sobel argument within its band of zero
    decides its sign by rounding; that sign reaches the 3x3 neighbourhood through the adjoint stencil."""
    dy, dx = sobel_args(pred, gt)
    by, bx, sy, sx = sobel_bands(pred, gt, band)
    return _dilate(((np.abs(dy) <= by) & (sy > 0)) | ((np.abs(dx) <= bx) & (sx > 0)), 1, 1, 1, 1)


def _gx(x):
    o = np.zeros_like(x)
    o[..., :, :-1] = x[..., :, :-1] - x[..., :, 1:]
    return o


def _gy(x):
    o = np.zeros_like(x)
    o[..., :-1, :] = x[..., :-1, :] - x[..., 1:, :]
    return o


def smoothness(depth, img):
    """(loss, dloss/ddepth): 0.1 * mean(|gx(D) * wx| + |gy(D) * wy|), gx(X)[x] = X[x] - X[x+1] with the last column
    replicated (difference 0), w = exp(-mean_c |g(I)|).  The image carries no gradient."""
    D, I = f64(depth), f64(img)
    wx = np.exp(-np.abs(_gx(I)).mean(1, keepdims=True))
    wy = np.exp(-np.abs(_gy(I)).mean(1, keepdims=True))
    gx, gy = _gx(D), _gy(D)
    n = D.size
    loss = 0.1 * (np.abs(gx * wx) + np.abs(gy * wy)).sum() / n
    tx, ty = np.sign(gx) * wx, np.sign(gy) * wy
    grad = tx + ty
    grad[..., :, 1:] -= tx[..., :, :-1]
    grad[..., 1:, :] -= ty[..., :-1, :]
    # sum of the |weights| that enter each pixel's gradient: the scale of its rounding error
    mag = np.abs(tx) + np.abs(ty)
    mag[..., :, 1:] += np.abs(tx[..., :, :-1])
    mag[..., 1:, :] += np.abs(ty[..., :-1, :])
    return float(loss), 0.1 * grad / n, 0.1 * mag / n


def smooth_ambiguous(depth, band=SMOOTH_BAND):
    """Pixels whose gradient may legitimately differ between fp32 and float64: a depth difference within `band` of zero,
    carried to the two pixels of its stencil."""
    D = f64(depth)
    ax, ay = np.abs(_gx(D)) <= band, np.abs(_gy(D)) <= band
    ax[..., :, -1] = False           # the replicated border: the difference is 0 by definition, not by rounding
    ay[..., -1, :] = False
    return _dilate(ax, 0, 0, 1, 0) | _dilate(ay, 1, 0, 0, 0)


def mse(a, b, weight=1.0):
    """weight * mean((a - b)^2)."""
    d = f64(a) - f64(b)
    return float(weight * (d * d).sum() / d.size)


def mse_grad(a, b, weight=1.0, gscale=1.0):
    """d/da of weight * mean((a - b)^2), times the upstream scalar."""
    d = f64(a) - f64(b)
    return float(gscale) * 2.0 * weight / d.size * d


# ------------------------------------------------------------------------------------------------------- BatchNorm
def bn_preact(y, scale, shift):
    return f64(y) * f64(scale) + f64(shift)


def bn_apply(y, scale, shift, relu=False, residual=None):
    """[relu](y * scale + shift) (+ residual), per channel (last axis)."""
    z = bn_preact(y, scale, shift)
    if relu:
        z = np.maximum(z, 0.0)
    if residual is not None:
        z = z + f64(residual)
    return z


def bn_relu_ambiguous(y, scale, shift):
    """Pre-activations within 4 * 2^-24 * (|y * scale| + |shift|) of zero: fp32 may put them on the other side of the ReLU."""
    ys = f64(y) * f64(scale)
    return np.abs(ys + f64(shift)) <= 4 * EPS32 * (np.abs(ys) + np.abs(f64(shift)))


def bn_train_bwd(dout, y, scale, shift, mean, invstd, relu=False):
    """Backward of out = [relu](BN_train(y)) given the stored coefficients: dz = dout * [y*scale + shift > 0],
    xhat = (y - mean) * invstd, dbeta = sum dz, dgamma = sum dz * xhat, k1 = dbeta / N, k2 = dgamma / N,
    dy = scale * (dz - k1 - xhat * k2)   (scale = gamma * invstd).
    Returns a dict with those and abs1 = sum |dz|, abs2 = sum |dz * xhat| (the scale of the sums' rounding error)."""
    dz = f64(dout).copy()
    yy = f64(y)
    C = yy.shape[-1]
    if relu:
        dz[~(bn_preact(yy, scale, shift) > 0.0)] = 0.0
    xh = (yy - f64(mean)) * f64(invstd)
    t2 = dz * xh
    n = yy.size // C
    dbeta, dgamma = dz.reshape(-1, C).sum(0), t2.reshape(-1, C).sum(0)
    r = {"dz": dz, "xhat": xh, "dbeta": dbeta, "dgamma": dgamma, "k1": dbeta / n, "k2": dgamma / n, "n": n,
         "abs1": np.abs(dz).reshape(-1, C).sum(0), "abs2": np.abs(t2).reshape(-1, C).sum(0)}
    r["dy"] = bn_train_dy(r, scale, r["k1"], r["k2"])
    return r


def bn_train_dy(r, scale, k1, k2):
    return f64(scale) * (r["dz"] - f64(k1) - r["xhat"] * f64(k2))


def bn_eval_bwd(dout, y, scale, shift, relu=0):
    """dy = scale * dout * mask; relu 0: no mask, 1: y is the raw conv output (mask y*scale + shift > 0),
    2: y is the activated output (mask y > 0)."""
    o = f64(dout) * f64(scale)
    if relu == 1:
        o[~(bn_preact(y, scale, shift) > 0.0)] = 0.0
    elif relu == 2:
        o[~(f64(y) > 0.0)] = 0.0
    return o


def bn_stats(y, gamma, beta, eps=1e-5):
    """Train-mode coefficients in float64 (biased variance): scale, shift, mean, invstd."""
    yy = f64(y)
    C = yy.shape[-1]
    flat = yy.reshape(-1, C)
    mean = flat.mean(0)
    var = (flat * flat).mean(0) - mean * mean
    invstd = 1.0 / np.sqrt(np.maximum(var, 0.0) + eps)
    scale = f64(gamma) * invstd
    return scale, f64(beta) - mean * scale, mean, invstd


# ----------------------------------------------------------------------------------------------------- elementwise
def add(a, b):
    return f64(a) + f64(b)


def scale(x, s):
    return f64(x) * float(f64(s))


def tanh_bwd(dout, out):
    """d/dpre of out = tanh(pre): dout * (1 - out^2)."""
    o = f64(out)
    return f64(dout) * (1.0 - o * o)


def cast(x, dtype):
    return round_to(f64(x), dtype)
