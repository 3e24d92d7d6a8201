"""numpy restatement of the reference's evaluation arithmetic (calculate_error.py, the NYU validation transform,
scipy's bytescale), the yardstick the evaluation tests compare the HIP kernels and the CLI against.

The per-pixel chain is float32, operation by operation as torch evaluates it, so every mask decision and median equals
torch's; the reductions are float64.  test_eval_cpu.py pins it to the reference's own results (metrics_eval.npz, and
metrics_edges.npz for the edge inputs below)."""
import hashlib

import numpy as np

F = np.float32

# Inputs of tests/golden/metrics_eval.npz: (name, B, H, W, levels), levels 0 = (near) continuous values.  The npz stores the
# reference's results and a digest of these inputs, not the inputs: golden_inputs() rebuilds them from integer draws of a
# seeded RandomState and exact integer -> float32 conversions, which give the same bits on every platform.
GOLDEN_CASES = [("kitti", 3, 128, 416, 0), ("nyu", 2, 320, 420, 0), ("kitti_tie", 3, 128, 416, 5),
                ("nyu_tie", 2, 320, 420, 7), ("small", 7, 32, 104, 0)]


def golden_inputs(case):
    """(gt_np, gt, pred) float32 [B,1,H,W] of one GOLDEN_CASES entry."""
    k, (name, B, H, W, levels) = [(i, c) for i, c in enumerate(GOLDEN_CASES) if c[0] == case][0]
    r = np.random.RandomState(100 + k)
    shape = (B, 1, H, W)
    if levels:      # a few levels only: the medians sit on long runs of equal values
        return tuple(r.randint(0, levels, shape).astype(F) for _ in range(3))
    sparse = r.randint(0, 10, shape) < 3                       # sparse LiDAR-like: 70 % "no return" (-1)
    gt_np = np.where(sparse, r.randint(-2 ** 15, 2 ** 15, shape), -2 ** 15).astype(F) * F(2.0 ** -15)
    ramp = (np.arange(W) * 97) % 1280                          # some structure along x
    gt = (r.randint(128, 20480, shape) + ramp).astype(F) * F(2.0 ** -8)
    pred = r.randint(-2 ** 20, 2 ** 20, shape).astype(F) * F(2.0 ** -20)
    return gt_np, gt, pred


def inputs_digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=F).tobytes())
    return h.hexdigest()[:16]


def _median(v):
    """torch.median: the lower of the two middle values, NaN as soon as one value is NaN."""
    if np.isnan(v).any():
        return F("nan")
    return np.sort(v)[(v.size - 1) // 2]


def _godard(n, lo, hi):
    return int(lo * n), int(hi * n)


class Rules:
    """The primitives of the reference's arithmetic that a kernel can get subtly wrong.  The restatement runs on the
    defaults; test_eval_cpu.py swaps one at a time for a wrong one to show that the edge cases notice."""
    median = staticmethod(_median)
    less = staticmethod(np.less)                  # thresh < 1.25 ** k: strict
    clip = staticmethod(np.clip)                  # torch.clamp: NaN stays NaN
    amin = staticmethod(np.min)                   # torch.min / max: NaN as soon as one pixel is NaN
    amax = staticmethod(np.max)
    box = staticmethod(lambda H, W, fy, fx: _godard(H, *fy) + _godard(W, *fx))      # (y1, y2, x1, x2)


KITTI_BOX = ((0.3324324, 0.91351351), (0.0359477, 0.96405229))
NYU_BOX = ((0.0359477, 0.96405229), (0.0359477, 0.96405229))


def _norm(x, scale, R=Rules):
    x = x.astype(F)
    with np.errstate(all="ignore"):
        mn, mx = R.amin(x), R.amax(x)
        return ((x - mn) / (mx - mn)) * F(scale)


def _box_mask(shape, fracs, R):
    m = np.zeros(shape, bool)
    y1, y2, x1, x2 = R.box(shape[0], shape[1], *fracs)
    m[max(y1, 0):max(y2, 0), max(x1, 0):max(x2, 0)] = True
    return m


def nyu_masked(g, p, crop, R=Rules):
    """(vg, vp) of one image [H,W]: the normalised values under the NYU mask, before the median scaling."""
    g, p = _norm(g, 10, R), _norm(p, 10, R)
    valid = (g < F(10)) & (g > F(0))
    if crop:
        valid &= _box_mask(g.shape, NYU_BOX, R)
    return g[valid], p[valid]


def kitti_masked(s, g, p, crop, R=Rules):
    """(vg, vp) of one image [H,W]: the normalised values under the KITTI mask, before the median scaling."""
    p, g = _norm(p, 80, R), _norm(g, 80, R)
    s = ((s.astype(F) + F(1.0)) / F(2.0)) * F(80)
    with np.errstate(invalid="ignore"):
        valid = (s < F(80)) & (g < F(80)) & (s > F(1)) & (g > F(1))
    if crop:
        valid &= _box_mask(g.shape, KITTI_BOX, R)
    return g[valid], p[valid]


def scaled_thresh(vg, vp, lo, hi, R=Rules):
    """(vp after median scaling and clamp, thresh), float32 as the reference computes them."""
    with np.errstate(all="ignore"):
        vp = R.clip(vp * R.median(vg) / R.median(vp), F(lo), F(hi))
        return vp, np.maximum(vg / vp, vp / vg)


def _frac(th, bound, R):
    with np.errstate(invalid="ignore"):
        return R.less(th, bound).mean()


@np.errstate(all="ignore")
def _per_image_nyu(g, p, crop, R=Rules):
    vg, vp = nyu_masked(g, p, crop, R)
    if vg.size == 0:
        return [float("nan")] * 8
    vp, th = scaled_thresh(vg, vp, 1e-3, 10, R)
    d = (vg - vp).astype(np.float64)
    lg = (np.log(vg) - np.log(vp)).astype(np.float64)
    return [np.abs(d).mean(), (np.abs(vg - vp) / vg).astype(np.float64).mean(),
            np.abs(np.log10(vg) - np.log10(vp)).astype(np.float64).mean(),
            _frac(th, 1.25, R), _frac(th, 1.25 ** 2, R), _frac(th, 1.25 ** 3, R),
            np.sqrt((d * d).mean()), np.sqrt((lg * lg).mean())]


@np.errstate(all="ignore")
def _per_image_make3d(s, g, p, R=Rules):
    s, g, p = _norm(s, 1, R), _norm(g, 1, R), _norm(p, 1, R)
    valid = (s > F(1e-2)) & (g > F(1e-2))
    s, g, p = s * F(80), g * F(80), p * F(80)
    valid &= (s < F(80)) & (g < F(80))
    vg, vp = R.clip(g[valid], F(1e-2), F(80)), R.clip(p[valid], F(1e-2), F(80))
    if vg.size == 0:
        return [float("nan")] * 4
    vp = vp * R.median(vg) / R.median(vp)
    d = (vg - vp).astype(np.float64)
    return [np.abs(d).mean(), (np.abs(vg - vp) / vg).astype(np.float64).mean(),
            np.abs(np.log10(vg) - np.log10(vp)).astype(np.float64).mean(), np.sqrt((d * d).mean())]


@np.errstate(all="ignore")
def _per_image_kitti(s, g, p, crop, R=Rules):
    vg, vp = kitti_masked(s, g, p, crop, R)
    if vg.size == 0:
        return [float("nan")] * 8
    vp, th = scaled_thresh(vg, vp, 1, 80, R)
    d = (vg - vp).astype(np.float64)
    lg = (np.log(vg) - np.log(vp)).astype(np.float64)
    return [np.abs(d).mean(), (np.abs(vg - vp) / vg).astype(np.float64).mean(), ((vg - vp) ** 2 / vg).astype(np.float64).mean(),
            _frac(th, 1.25, R), _frac(th, 1.25 ** 2, R), _frac(th, 1.25 ** 3, R),
            np.sqrt((d * d).mean()), np.sqrt((lg * lg).mean())]


def nyu_per_image(gt, pred, crop=True, R=Rules):
    """[B,n] per-image metrics; gt, pred [B,1,H,W]."""
    return np.array([_per_image_nyu(gt[b, 0], pred[b, 0], crop, R) for b in range(gt.shape[0])], np.float64)


def make3d_per_image(gt_np, gt, pred, R=Rules):
    return np.array([_per_image_make3d(gt_np[b, 0], gt[b, 0], pred[b, 0], R) for b in range(gt.shape[0])], np.float64)


def kitti_per_image(gt_np, gt, pred, crop=True, R=Rules):
    return np.array([_per_image_kitti(gt_np[b, 0], gt[b, 0], pred[b, 0], crop, R) for b in range(gt.shape[0])], np.float64)


def compute_errors_NYU(gt, pred, crop=True):
    return nyu_per_image(gt, pred, crop).mean(0)


def compute_errors_Make3D(gt_np, gt, pred):
    return make3d_per_image(gt_np, gt, pred).mean(0)


def compute_errors(gt_np, gt, pred, crop=True):
    return kitti_per_image(gt_np, gt, pred, crop).mean(0)


# ---------------------------------------------------------------------------------------------------------------------
# Edge inputs of tests/golden/metrics_edges.npz: (name, kind, B, H, W, seed).  As above the npz stores the reference's
# results and a digest; edge_inputs() rebuilds the inputs from integer draws and exact conversions.  Kinds:
#   cont     continuous values, 60 % of the sparse map has a return (the Godard crop of 4 x 6 leaves ONE valid pixel)
#   two      exactly two valid pixels under every mask
#   tie<L>   L levels only: the medians sit on long runs of equal values
#   bucket_g / bucket_p   an even number of KITTI-valid pixels, half of them below and half above 8.0 (gt) / 2.0 (pred): the
#            two middle values differ in the top byte of their bit pattern, the first digit of the radix select
#   thresh   levels k / 256 chosen so that thresh is 1.25, 1.5625 and 1.953125 exactly on many pixels
#   the non-finite kinds start from `cont` and change one thing; `mixed` holds a constant prediction (image 1), a constant
#   ground truth (image 3) and a sparse map without a return (image 4)
NAN_AT = (7, 11)        # inside every crop box of a 16 x 24 image
EDGE_CASES = [("s4x6", "cont", 1, 4, 6, 267), ("s16x24", "cont", 1, 16, 24, 1), ("s33x31", "cont", 1, 33, 31, 2),
              ("s32x32", "cont", 1, 32, 32, 3), ("s25x41", "cont", 1, 25, 41, 4), ("s32x104", "cont", 2, 32, 104, 5),
              ("two", "two", 1, 16, 24, 6),
              ("tie5_16x24", "tie5", 1, 16, 24, 7), ("tie7_16x24", "tie7", 1, 16, 24, 8),
              ("tie5_33x31", "tie5", 1, 33, 31, 9), ("tie7_33x31", "tie7", 1, 33, 31, 10),
              ("bucket_g", "bucket_g", 1, 16, 24, 11), ("bucket_p", "bucket_p", 1, 16, 24, 12),
              ("thresh", "thresh", 1, 33, 31, 13),
              ("pred_nan", "pred_nan", 1, 16, 24, 14), ("pred_inf", "pred_inf", 1, 16, 24, 14),
              ("pred_all_nan", "pred_all_nan", 1, 16, 24, 14), ("pred_const", "pred_const", 1, 16, 24, 14),
              ("gt_nan", "gt_nan", 1, 16, 24, 14), ("gt_const", "gt_const", 1, 16, 24, 14),
              ("sparse_nan", "sparse_nan", 1, 16, 24, 14),
              ("mixed", "mixed", 5, 16, 24, 15)]
# (gt level, pred level) pairs of `thresh`: the ratios 1, 1.25, 1.5625, 1.953125 both ways round, and some far off
THRESH_PAIRS = [(64, 64), (80, 64), (64, 80), (100, 64), (64, 100), (125, 64), (64, 125), (125, 64), (64, 125),
                (40, 32), (32, 40), (50, 32), (32, 50), (128, 32), (32, 128)]


def _cont(r, shape):
    W = shape[-1]
    sparse = r.randint(0, 10, shape) < 6
    gt_np = np.where(sparse, r.randint(-2 ** 15, 2 ** 15, shape), -2 ** 15).astype(F) * F(2.0 ** -15)
    ramp = (np.arange(W) * 97) % 1280
    gt = (r.randint(128, 20480, shape) + ramp).astype(F) * F(2.0 ** -8)
    pred = r.randint(-2 ** 20, 2 ** 20, shape).astype(F) * F(2.0 ** -20)
    return gt_np, gt, pred


def _bucket(r, shape, which):
    """gt and pred in 1/256 steps of [0, 80] with 0 and 80 in the first row (outside the crop box), so the normalised
    value is the value itself up to rounding; returns only inside the Godard box, so crop on and off see the same pixels."""
    H, W = shape[-2:]
    y1, y2, x1, x2 = Rules.box(H, W, *KITTI_BOX)
    ret = np.zeros((H, W), bool)
    ret[y1:y2, x1:x2] = r.randint(0, 10, (y2 - y1, x2 - x1)) < 6
    idx = r.permutation(np.flatnonzero(ret))
    idx = idx[:idx.size // 2 * 2]
    ret[:] = False
    ret.flat[idx] = True
    gt_np = np.where(ret, r.randint(-2 ** 14, 2 ** 14, (H, W)), -2 ** 15).astype(F) * F(2.0 ** -15)
    gt = r.randint(3 * 256, 70 * 256, (H, W))
    pred = r.randint(3 * 256, 70 * 256, (H, W))
    lo, hi = idx[:idx.size // 2], idx[idx.size // 2:]
    if which == "g":
        gt.flat[lo] = r.randint(2 * 256 + 64, 7 * 256 + 128, lo.size)
        gt.flat[hi] = r.randint(8 * 256 + 128, 70 * 256, hi.size)
    else:
        pred.flat[lo] = r.randint(128, 256 + 230, lo.size)
        pred.flat[hi] = r.randint(2 * 256 + 26, 60 * 256, hi.size)
    for a in (gt, pred):
        a[0, 0], a[0, 1] = 0, 80 * 256
    return tuple(a.astype(F).reshape(shape) for a in (gt_np, gt * F(2.0 ** -8), pred * F(2.0 ** -8)))


def edge_inputs(case):
    """(gt_np, gt, pred) float32 [B,1,H,W] of one EDGE_CASES entry."""
    name, kind, B, H, W, seed = [c for c in EDGE_CASES if c[0] == case][0]
    r = np.random.RandomState(1000 + seed)
    shape = (B, 1, H, W)
    if kind.startswith("tie"):
        return tuple(r.randint(0, int(kind[3:]), shape).astype(F) for _ in range(3))
    if kind.startswith("bucket"):
        return _bucket(r, shape, kind[-1])
    if kind == "thresh":
        pairs = np.array(THRESH_PAIRS)[r.randint(0, len(THRESH_PAIRS), shape)]
        gt, pred = pairs[..., 0].copy(), pairs[..., 1].copy()
        for a in (gt, pred):            # min and max outside every crop box: normalised value = level / 256 * scale, exact
            a[0, 0, 0, 0], a[0, 0, 0, 1] = 0, 256
        gt_np = np.where(r.randint(0, 10, shape) < 6, r.randint(-2 ** 14, 2 ** 14, shape), -2 ** 15)
        return gt_np.astype(F) * F(2.0 ** -15), gt.astype(F), pred.astype(F)
    gt_np, gt, pred = _cont(r, shape)
    y, x = NAN_AT
    if kind == "two":                   # gt: 0 everywhere but one maximum and two values in between
        gt[:] = 0
        gt[0, 0, 0, 0], gt[0, 0, y, x], gt[0, 0, y + 1, x + 2] = 1024, 300, 700
        gt_np[0, 0, 0, 0], gt_np[0, 0, y, x], gt_np[0, 0, y + 1, x + 2] = 0.75, 0.25, -0.5
    elif kind == "pred_nan":
        pred[0, 0, y, x] = np.nan
    elif kind == "pred_inf":
        pred[0, 0, y, x] = np.inf
    elif kind == "pred_all_nan":
        pred[:] = np.nan
    elif kind == "pred_const":
        pred[:] = 0.5
    elif kind == "gt_nan":
        gt[0, 0, y, x] = np.nan
    elif kind == "gt_const":
        gt[:] = 3.0
    elif kind == "sparse_nan":
        gt_np[0, 0, y, x] = np.nan
    elif kind == "mixed":
        pred[1], gt[3], gt_np[4] = 0.5, 3.0, -1.0
    return gt_np, gt, pred


# Which columns of a metric row are what: `count` a1..a3, `arith` sums of float32 terms, `log` rest on log / log10
COLUMNS = {"kitti": {"arith": (0, 1, 2, 6), "count": (3, 4, 5), "log": (7,)},
           "nyu": {"arith": (0, 1, 6), "count": (3, 4, 5), "log": (2, 7)},
           "make3d": {"arith": (0, 1, 3), "count": (), "log": (2,)}}


def ulps32(a, b):
    """Distance in float32 steps between two finite float32 values."""
    def key(v):
        i = np.asarray(v, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def row_mismatch(got, want, kind, log_bar, count_ulps=0):
    """What of a float32 metric row `got` misses the float64 row `want`: NaN positions must be identical, the counts equal
    float32(want) bit for bit (within one step for a batch mean), the sums of float32 terms lie within one float32 step of
    it, and the log metrics within `log_bar`, relative.  Returns a list of messages, empty when the row holds."""
    got, want = np.asarray(got, F), np.asarray(want, np.float64)
    bad = []
    for cls, cols in COLUMNS[kind].items():
        for c in cols:
            g, w = got[c], want[c]
            if np.isnan(g) or np.isnan(w):
                ok = bool(np.isnan(g) and np.isnan(w))
            elif not (np.isfinite(g) and np.isfinite(w)):
                ok = bool(g == w)
            elif cls == "log":
                ok = bool(abs(float(g) - w) <= log_bar * abs(w))
            else:
                ok = bool(ulps32(g, F(w)) <= (count_ulps if cls == "count" else 1))
            if not ok:
                bad.append("column %d (%s): got %r, want %r" % (c, cls, float(g), float(w)))
    return bad


def center_crop_offsets(h0, w0, h, w):
    return int(round((h0 - h) / 2.)), int(round((w0 - w) / 2.))


def crop_normalize(a, i, j, H, W):
    """a [H0,W0,C] uint8/float32 -> [C,H,W] float32: ArrayToTensor (/255) + Normalize ((t - 0.5) / 0.5) of the window."""
    w = a[i:i + H, j:j + W].astype(F)
    return ((w / F(255) - F(0.5)) / F(0.5)).transpose(2, 0, 1)


def bytescale(x):
    """[C,H,W] float32 -> [H,W,C] uint8 as scipy.misc.bytescale treats the float64 copy GDN_main.py:298-306 makes."""
    d = x.astype(np.float64).transpose(1, 2, 0)
    cmin, cmax = d.min(), d.max()
    cscale = cmax - cmin
    if cscale == 0:
        cscale = 1
    scale = float(255 - 0) / cscale
    b = (d - cmin) * scale + 0
    return (b.clip(0, 255) + 0.5).astype(np.uint8)
