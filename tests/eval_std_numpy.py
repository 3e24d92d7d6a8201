"""Float64 numpy restatement of the Eigen-split evaluation (gdn_depth_metrics_std), written from the
formulas: the yardstick of tests/test_hip_eval_std.py, pinned without a GPU by tests/test_eval_std_cpu.py against an
independent formulation (torch's float64 bilinear interpolation, np.median, boolean masks).

The operation order of the interpolation and of every per-pixel expression is the kernel's, so that the float32-rounded
depths -- and with them every count -- come out bit for bit; only the order of the sums differs (numpy sums pairwise)."""
import numpy as np

ERROR_NAMES_STD = ['abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'a1', 'a2', 'a3', 'log10', 'silog']
CROPS = {'garg': (0.40810811, 0.99189189, 0.03594771, 0.96405229), 'eigen': (0.3324324, 0.91351351, 0.0359477, 0.96405229)}


def eval_box(h, w, crop):
    """(h0, w0, y1, y2, x1, x2) of one image."""
    if crop == 'none':
        return [h, w, 0, h, 0, w]
    a, b, c, d = CROPS[crop]
    return [h, w, int(a * h), int(b * h), int(c * w), int(d * w)]


def gt_metres(raw, kind, depth_scale):
    """The ground truth in metres as float32.  kind 0: float32 metres; 1: uint16 / 256; 2: float32 in [-1, 1]."""
    if kind == 0:
        return np.asarray(raw, np.float32)
    if kind == 1:
        assert raw.dtype == np.uint16
        return raw.astype(np.float32) / np.float32(256)
    scale = np.float64(np.float32(depth_scale))
    return ((np.asarray(raw, np.float32).astype(np.float64) + 1.0) / 2.0 * scale).astype(np.float32)


def _axis(n_in, n_out):
    i = np.arange(n_out, dtype=np.float64)
    s = np.maximum((i + 0.5) * (np.float64(n_in) / np.float64(n_out)) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0.astype(np.float64)


def resample(pred, h0, w0, depth_scale):
    """pred [H,W] float32 in [-1, 1] -> the float32 depth at h0 x w0: bilinear, half-pixel centres, edge-clamped, float64."""
    u = (np.asarray(pred, np.float32).astype(np.float64) + 1.0) / 2.0
    y0, y1, wy = _axis(u.shape[0], h0)
    x0, x1, wx = _axis(u.shape[1], w0)
    wy, wx = wy[:, None], wx[None, :]
    top = u[y0][:, x0] * (1.0 - wx) + u[y0][:, x1] * wx
    bot = u[y1][:, x0] * (1.0 - wx) + u[y1][:, x1] * wx
    t = top * (1.0 - wy) + bot * wy
    with np.errstate(invalid='ignore', over='ignore'):
        p = (t * np.float64(np.float32(depth_scale))).astype(np.float32)
    return np.maximum(p, np.float32(0)) + np.float32(0)           # NaN propagates; -0 becomes +0


def median(v):
    """numpy's median of a float32 vector, in float64: the mean of the two middle values of an even count."""
    if np.isnan(v).any():
        return np.float64('nan')
    s = np.sort(np.asarray(v, np.float32)).astype(np.float64)
    n = s.size
    return (s[(n - 1) // 2] + s[n // 2]) / 2.0


def valid_mask(g, box, min_depth, max_depth):
    h0, w0, y1, y2, x1, x2 = box
    m = (g > np.float32(min_depth)) & (g < np.float32(max_depth))
    inside = np.zeros((h0, w0), bool)
    inside[y1:y2, x1:x2] = True
    return m & inside


def std_row(raw, kind, box, pred, depth_scale=80.0, min_depth=1e-3, max_depth=80.0, median_scaling=False):
    """One image: raw ground truth (at least h0 x w0; the rest is ignored), its box, pred [H,W] -> the 12 float64 of a row."""
    h0, w0 = int(box[0]), int(box[1])
    g32 = gt_metres(np.asarray(raw)[:h0, :w0], kind, depth_scale)
    m = valid_mask(g32, [int(v) for v in box], min_depth, max_depth)
    n = int(m.sum())
    row = np.full(12, np.nan)
    row[0], row[11] = n, 0.0
    if n == 0:
        return row
    p32 = resample(pred, h0, w0, depth_scale)[m]
    g = g32[m].astype(np.float64)
    ratio = np.float64(1.0)
    with np.errstate(all='ignore'):
        if median_scaling:
            ratio = median(g32[m]) / median(p32)
        p = p32.astype(np.float64) * ratio
        lo, hi = np.float64(np.float32(min_depth)), np.float64(np.float32(max_depth))
        p = np.where(np.isnan(p), p, np.minimum(np.maximum(p, lo), hi))
        d = g - p
        e = np.log(p) - np.log(g)
        th = np.maximum(g / p, p / g)
        m1, m2 = np.mean(e), np.mean(e * e)
        var = m2 - m1 * m1
        row[1] = ratio
        row[2] = np.mean(np.abs(d) / g)
        row[3] = np.mean((d * d) / g)
        row[4] = np.sqrt(np.mean(d * d))
        row[5] = np.sqrt(m2)
        row[6] = np.float64(int((th < 1.25).sum())) / np.float64(n)
        row[7] = np.float64(int((th < 1.5625).sum())) / np.float64(n)
        row[8] = np.float64(int((th < 1.953125).sum())) / np.float64(n)
        row[9] = np.mean(np.abs(np.log10(g) - np.log10(p)))
        row[10] = var if np.isnan(var) else 100.0 * np.sqrt(max(var, 0.0))
    return row


def std_rows(gt, kind, boxes, pred, **kw):
    """gt [B,Hmax,Wmax], boxes [B][6], pred [B,1,H,W] or [B,H,W] -> [B,12] float64."""
    pred = np.asarray(pred)
    pred = pred[:, 0] if pred.ndim == 4 else pred
    return np.stack([std_row(gt[b], kind, boxes[b], pred[b], **kw) for b in range(len(boxes))])


def log_error_stats(raw, kind, box, pred, depth_scale=80.0, min_depth=1e-3, max_depth=80.0, median_scaling=False):
    """(mean, std) of e = ln p - ln g over the valid pixels of one image: how much silog's subtraction cancels."""
    h0, w0 = int(box[0]), int(box[1])
    g32 = gt_metres(np.asarray(raw)[:h0, :w0], kind, depth_scale)
    m = valid_mask(g32, [int(v) for v in box], min_depth, max_depth)
    p32 = resample(pred, h0, w0, depth_scale)[m]
    ratio = median(g32[m]) / median(p32) if median_scaling else 1.0
    p = np.clip(p32.astype(np.float64) * ratio, np.float64(np.float32(min_depth)), np.float64(np.float32(max_depth)))
    e = np.log(p) - np.log(g32[m].astype(np.float64))
    return float(e.mean()), float(e.std())


def mean_rows(rows):
    """(float64 mean of the nine metrics over the rows with n > 0, number of rows left out)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 12)
    keep = rows[:, 0] > 0
    if not keep.any():
        return np.full(9, np.nan), int((~keep).sum())
    return rows[keep][:, 2:11].mean(0), int((~keep).sum())
