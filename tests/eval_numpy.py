"""numpy restatement of the reference's evaluation arithmetic (calculate_error.py, the NYU validation transform,
scipy's bytescale), the yardstick the evaluation tests compare the HIP kernels and the CLI against.

The per-pixel chain is float32, operation by operation as torch evaluates it, so every mask decision and median equals
torch's; the reductions are float64.  test_eval_cpu.py pins it to the reference's own results (metrics_eval.npz)."""
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


def _norm(x, scale):
    x = x.astype(F)
    return ((x - x.min()) / (x.max() - x.min())) * F(scale)


def _median(v):
    return np.sort(v)[(v.size - 1) // 2]          # torch.median: the lower of the two middle values


def _godard(n, lo, hi):
    return int(lo * n), int(hi * n)


def _per_image_nyu(g, p, crop):
    H, W = g.shape
    g, p = _norm(g, 10), _norm(p, 10)
    valid = (g < F(10)) & (g > F(0))
    if crop:
        m = np.zeros_like(valid)
        y1, y2 = _godard(H, 0.0359477, 0.96405229)
        x1, x2 = _godard(W, 0.0359477, 0.96405229)
        m[y1:y2, x1:x2] = True
        valid &= m
    vg, vp = g[valid], p[valid]
    if vg.size == 0:
        return [float("nan")] * 8
    vp = np.clip(vp * _median(vg) / _median(vp), F(1e-3), F(10))
    th = np.maximum(vg / vp, vp / vg)
    d = (vg - vp).astype(np.float64)
    lg = (np.log(vg) - np.log(vp)).astype(np.float64)
    return [np.abs(d).mean(), (np.abs(vg - vp) / vg).astype(np.float64).mean(),
            np.abs(np.log10(vg) - np.log10(vp)).astype(np.float64).mean(),
            (th < 1.25).mean(), (th < 1.25 ** 2).mean(), (th < 1.25 ** 3).mean(),
            np.sqrt((d * d).mean()), np.sqrt((lg * lg).mean())]


def _per_image_make3d(s, g, p):
    s, g, p = _norm(s, 1), _norm(g, 1), _norm(p, 1)
    valid = (s > F(1e-2)) & (g > F(1e-2))
    s, g, p = s * F(80), g * F(80), p * F(80)
    valid &= (s < F(80)) & (g < F(80))
    vg, vp = np.clip(g[valid], F(1e-2), F(80)), np.clip(p[valid], F(1e-2), F(80))
    if vg.size == 0:
        return [float("nan")] * 4
    vp = vp * _median(vg) / _median(vp)
    d = (vg - vp).astype(np.float64)
    return [np.abs(d).mean(), (np.abs(vg - vp) / vg).astype(np.float64).mean(),
            np.abs(np.log10(vg) - np.log10(vp)).astype(np.float64).mean(), np.sqrt((d * d).mean())]


def _per_image_kitti(s, g, p, crop):
    H, W = g.shape
    p, g = _norm(p, 80), _norm(g, 80)
    s = ((s.astype(F) + F(1.0)) / F(2.0)) * F(80)
    valid = (s < F(80)) & (g < F(80)) & (s > F(1)) & (g > F(1))
    if crop:
        m = np.zeros_like(valid)
        y1, y2 = _godard(H, 0.3324324, 0.91351351)
        x1, x2 = _godard(W, 0.0359477, 0.96405229)
        m[y1:y2, x1:x2] = True
        valid &= m
    vg, vp = g[valid], p[valid]
    if vg.size == 0:
        return [float("nan")] * 8
    vp = np.clip(vp * _median(vg) / _median(vp), F(1), F(80))
    th = np.maximum(vg / vp, vp / vg)
    d = (vg - vp).astype(np.float64)
    lg = (np.log(vg) - np.log(vp)).astype(np.float64)
    return [np.abs(d).mean(), (np.abs(vg - vp) / vg).astype(np.float64).mean(), ((vg - vp) ** 2 / vg).astype(np.float64).mean(),
            (th < 1.25).mean(), (th < 1.25 ** 2).mean(), (th < 1.25 ** 3).mean(),
            np.sqrt((d * d).mean()), np.sqrt((lg * lg).mean())]


def nyu_per_image(gt, pred, crop=True):
    """[B,n] per-image metrics; gt, pred [B,1,H,W]."""
    return np.array([_per_image_nyu(gt[b, 0], pred[b, 0], crop) for b in range(gt.shape[0])], np.float64)


def make3d_per_image(gt_np, gt, pred):
    return np.array([_per_image_make3d(gt_np[b, 0], gt[b, 0], pred[b, 0]) for b in range(gt.shape[0])], np.float64)


def kitti_per_image(gt_np, gt, pred, crop=True):
    return np.array([_per_image_kitti(gt_np[b, 0], gt[b, 0], pred[b, 0], crop) for b in range(gt.shape[0])], np.float64)


def compute_errors_NYU(gt, pred, crop=True):
    return nyu_per_image(gt, pred, crop).mean(0)


def compute_errors_Make3D(gt_np, gt, pred):
    return make3d_per_image(gt_np, gt, pred).mean(0)


def compute_errors(gt_np, gt, pred, crop=True):
    return kitti_per_image(gt_np, gt, pred, crop).mean(0)


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
