"""Depth metrics on the HIP path (drop-in for the reference's calculate_error.py: compute_errors :10-103,
compute_errors_NYU :105-150, compute_errors_Make3D :152-182).

Where the reference raises (an image with no valid pixel: torch.median of an empty tensor) these return NaN for that
image, so the batch mean is NaN.

Non-finite inputs give what the reference gives, since torch's min / max / median propagate NaN and clamp keeps it: a NaN
or +-inf pixel in pred, or a constant pred (0 / 0 in the min-max normalisation), makes every sum NaN and a1 = a2 = a3 = 0
-- a diverged network does not get finite numbers -- and a NaN pixel in gt, or a constant gt, leaves no valid pixel (NaN
throughout).  A NaN in compute_errors' gt_np only drops that pixel; compute_errors_Make3D normalises gt_np as well, so
there it leaves none."""

from . import ops
from ._lib import GdnError

ERROR_NAMES = ['abs_diff', 'abs_rel', 'sq_rel', 'a1', 'a2', 'a3', 'rmse', 'rmse_log']
ERROR_NAMES_NYU = ['abs_diff', 'abs_rel', 'log10', 'a1', 'a2', 'a3', 'rmse', 'rmse_log']
ERROR_NAMES_MAKE3D = ['abs_diff', 'abs_rel', 'ave_log10', 'rmse']


def _plane(t, name):
    if t.dim() != 4:
        raise GdnError("%s must be [B,C,H,W]" % name)
    if not t.is_cuda:
        raise GdnError("%s must live on the GPU: the HIP path has no CPU fallback" % name)
    t = t.detach().float()
    return t[:, 0:1].contiguous()


def compute_errors_device(gt_np, gt, pred, crop=True):
    """Eight KITTI metrics as a device tensor [8] (no host sync)."""
    g, s, p = _plane(gt, "gt"), _plane(gt_np, "gt_np"), _plane(pred, "pred")
    if not (g.shape == s.shape == p.shape):
        raise GdnError("gt_np, gt and pred must have the same batch and spatial size")
    return ops.depth_metrics(s, g, p, crop)


def compute_errors(gt_np, gt, pred, crop=True):
    """[abs_diff, abs_rel, sq_rel, a1, a2, a3, rmse, rmse_log] batch means as Python floats.

    gt_np: sparse LiDAR ground truth in [-1,1]; gt: dense ground truth; pred: prediction
    (same call signature and meaning as the reference)."""
    return [float(v) for v in compute_errors_device(gt_np, gt, pred, crop).tolist()]


# ---------------------------------------------------------------------------------------------------------------------
# The Eigen-split protocol (--eval_protocol standard): metric depth, a min / max depth cap, the Garg or
# Eigen crop at the ground truth's own resolution, optional median scaling, nine metrics averaged PER IMAGE.  It differs
# from compute_errors above on purpose and shares nothing with it.
ERROR_NAMES_STD = ['abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'a1', 'a2', 'a3', 'log10', 'silog']
STD_ROW = 12            # per image: n, ratio, the nine metrics, 0
EVAL_CROPS = {'garg': (0.40810811, 0.99189189, 0.03594771, 0.96405229),
              'eigen': (0.3324324, 0.91351351, 0.0359477, 0.96405229)}


def eval_boxes(sizes, crop='garg'):
    """[(h, w), ...] -> int32 [B,6] host tensor of (h0, w0, y1, y2, x1, x2): the crop box of each image at its own size.
    garg: rows int(0.40810811 h) .. int(0.99189189 h), columns int(0.03594771 w) .. int(0.96405229 w); eigen: rows
    0.3324324 / 0.91351351, columns 0.0359477 / 0.96405229; none: the whole image.  Python float arithmetic."""
    import torch
    if crop not in EVAL_CROPS and crop != 'none':
        raise GdnError("unknown crop %r (garg, eigen, none)" % (crop,))
    rows = []
    for h, w in sizes:
        h, w = int(h), int(w)
        if h <= 0 or w <= 0:
            raise GdnError("eval_boxes: an image of %d x %d" % (h, w))
        if crop == 'none':
            rows.append([h, w, 0, h, 0, w])
        else:
            fy1, fy2, fx1, fx2 = EVAL_CROPS[crop]
            rows.append([h, w, int(fy1 * h), int(fy2 * h), int(fx1 * w), int(fx2 * w)])
    return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 6)


def compute_errors_std_device(gt, sizes, pred, crop='garg', min_depth=1e-3, max_depth=80.0, depth_scale=80.0,
                              median_scaling=False, gt_kind=None):
    """The per-image rows [B,12] (float64, on the device, no sync) of gdn_depth_metrics_std.

    gt: [B,Hmax,Wmax] or [B,1,Hmax,Wmax] on the GPU -- uint16 (metres x 256, the official KITTI depth PNG), or float32 in
    [-1, 1] as the loaders yield it (gt_kind=ops.GT_METRES: float32 metres).  sizes: [(h, w), ...] of the images inside
    the pool, None = all of it.  pred: [B,1,H,W] in [-1, 1]; it is resampled to each image's own size."""
    import torch
    if gt.dim() == 4:
        gt = gt[:, 0]
    if gt.dim() != 3 or not gt.is_cuda:
        raise GdnError("gt must be [B,Hmax,Wmax] or [B,1,Hmax,Wmax] on the GPU: the HIP path has no CPU fallback")
    if gt_kind is None:
        gt_kind = ops.GT_U16 if gt.dtype == torch.uint16 else ops.GT_UNIT
    gt = gt.detach().contiguous() if gt_kind == ops.GT_U16 else gt.detach().float().contiguous()
    p = _plane(pred, "pred")
    B, Hmax, Wmax = gt.shape
    if sizes is None:
        sizes = [(Hmax, Wmax)] * B
    if len(sizes) != B or p.shape[0] != B:
        raise GdnError("gt holds %d images, sizes %d, pred %d" % (B, len(sizes), p.shape[0]))
    if any(h > Hmax or w > Wmax for h, w in sizes):
        raise GdnError("an image of %s does not fit the %d x %d pool" % (max(sizes), Hmax, Wmax))
    boxes = eval_boxes(sizes, crop)
    boxes = boxes.pin_memory().to(gt.device, non_blocking=True)
    return ops.depth_metrics_std(gt, gt_kind, boxes, p, depth_scale, min_depth, max_depth, median_scaling)


def mean_errors_std(rows):
    """rows: [N,12] float64 host tensor -> (the nine metrics as the float64 mean over the images with n > 0, the number of
    images left out); NaN where no image is left."""
    import torch
    rows = torch.as_tensor(rows, dtype=torch.float64).reshape(-1, STD_ROW)
    keep = rows[:, 0] > 0
    left_out = int((~keep).sum())
    if not bool(keep.any()):
        return [float('nan')] * len(ERROR_NAMES_STD), left_out
    return [float(v) for v in rows[keep][:, 2:11].mean(0).tolist()], left_out


def compute_errors_std(gt, sizes, pred, **kw):
    """[abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, log10, silog] as Python floats: the mean over the images of the batch
    that have a valid pixel (arguments as for compute_errors_std_device)."""
    return mean_errors_std(compute_errors_std_device(gt, sizes, pred, **kw).cpu())[0]


def compute_errors_NYU_device(gt, pred, crop=True):
    """Eight NYU Depth v2 metrics as a device tensor [8] (no host sync)."""
    g, p = _plane(gt, "gt"), _plane(pred, "pred")
    if g.shape != p.shape:
        raise GdnError("gt and pred must have the same batch and spatial size")
    return ops.depth_metrics_nyu(g, p, crop)


def compute_errors_NYU(gt, pred, crop=True):
    """[abs_diff, abs_rel, log10, a1, a2, a3, rmse, rmse_log] batch means as Python floats (reference signature)."""
    return [float(v) for v in compute_errors_NYU_device(gt, pred, crop).tolist()]


def compute_errors_Make3D_device(gt_np, gt, pred):
    """Four Make3D metrics as a device tensor [4] (no host sync)."""
    g, s, p = _plane(gt, "gt"), _plane(gt_np, "gt_np"), _plane(pred, "pred")
    if not (g.shape == s.shape == p.shape):
        raise GdnError("gt_np, gt and pred must have the same batch and spatial size")
    return ops.depth_metrics_make3d(s, g, p)


def compute_errors_Make3D(gt_np, gt, pred):
    """[abs_diff, abs_rel, ave_log10, rmse] batch means as Python floats (reference signature)."""
    return [float(v) for v in compute_errors_Make3D_device(gt_np, gt, pred).tolist()]
