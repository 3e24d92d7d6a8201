"""Float64 numpy yardsticks of the Velodyne projection (gdn_velo_project).

restate     the specification, elementwise: the kernel's operation order, the minimum taken by np.minimum.at on the
            order-preserving keys.  tests/test_hip_velo.py compares the device pools with it bit for bit.
published   a literal transcription of the host routine in circulation (np.dot, last writer, then the minimum over the
            pixels hit more than once in a Python loop, then depth[depth < 0] = 0).  tests/test_velo_cpu.py pins the
            restatement to it, away from rounding boundaries."""
from collections import Counter

import numpy as np

EMPTY = np.uint32(0xFFFFFFFF)


def key_of(d):
    """float32 -> uint32 whose unsigned order is the float order: bits | 0x80000000 for a clear sign bit, ~bits for a set one."""
    bits = np.asarray(d, np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def float_of(key):
    """The inverse of key_of (EMPTY gives the NaN 0x7fffffff)."""
    key = np.asarray(key, np.uint32)
    return np.where(key & np.uint32(0x80000000), key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32).view(np.float32)


def restate(points, P, size, depth_kind=0, pool=None):
    """One image: points [N,4] float32, P [3,4] float64, size (h0, w0) -> float32 [h0,w0] (or the pool's shape, image in the
    top-left corner), and the number of pixels > 0."""
    h0, w0 = int(size[0]), int(size[1])
    P = np.asarray(P, np.float64).reshape(3, 4)
    pts = np.asarray(points, np.float32).reshape(-1, 4).astype(np.float64)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all='ignore'):
        r = [((P[i, 0] * x + P[i, 1] * y) + P[i, 2] * z) + P[i, 3] for i in range(3)]
        u = np.rint(r[0] / r[2]) - 1.0
        v = np.rint(r[1] / r[2]) - 1.0
        keep = (x >= 0.0) & (u >= 0.0) & (v >= 0.0) & (u < np.float64(w0)) & (v < np.float64(h0))
        d = (x if depth_kind else r[2]).astype(np.float32)
    H, W = (h0, w0) if pool is None else (int(pool[0]), int(pool[1]))
    keys = np.full(H * W, EMPTY, np.uint32)
    np.minimum.at(keys, v[keep].astype(np.int64) * W + u[keep].astype(np.int64), key_of(d[keep]))
    m = float_of(keys)
    with np.errstate(invalid='ignore'):
        out = np.where(m > 0, m, np.float32(0)).astype(np.float32).reshape(H, W)
    return out, int((out > 0).sum())


def restate_batch(clouds, Ps, sizes, Hmax, Wmax, depth_kind=0):
    """-> (float32 [B,Hmax,Wmax], int32 [B])."""
    got = [restate(c, P, s, depth_kind, pool=(Hmax, Wmax)) for c, P, s in zip(clouds, Ps, sizes)]
    return np.stack([g[0] for g in got]), np.array([g[1] for g in got], np.int32)


def sub2ind(shape, rows, cols):
    return rows * (shape[1] - 1) + cols - 1


def published(points, P, size, vel_depth=False):
    """The published routine on one scan, from the line that drops the points behind the scanner onwards -> float64 [h0,w0]."""
    im_shape = (int(size[0]), int(size[1]))
    velo = np.array(points, np.float32).reshape(-1, 4)
    velo[:, 3] = 1.0
    P_velo2im = np.asarray(P, np.float64).reshape(3, 4)
    velo = velo[velo[:, 0] >= 0, :]
    velo_pts_im = np.dot(P_velo2im, velo.T).T
    velo_pts_im[:, :2] = velo_pts_im[:, :2] / velo_pts_im[:, 2][..., np.newaxis]
    if vel_depth:
        velo_pts_im[:, 2] = velo[:, 0]
    velo_pts_im[:, 0] = np.round(velo_pts_im[:, 0]) - 1
    velo_pts_im[:, 1] = np.round(velo_pts_im[:, 1]) - 1
    val_inds = (velo_pts_im[:, 0] >= 0) & (velo_pts_im[:, 1] >= 0)
    val_inds = val_inds & (velo_pts_im[:, 0] < im_shape[1]) & (velo_pts_im[:, 1] < im_shape[0])
    velo_pts_im = velo_pts_im[val_inds, :]
    depth = np.zeros(im_shape[:2])
    depth[velo_pts_im[:, 1].astype(int), velo_pts_im[:, 0].astype(int)] = velo_pts_im[:, 2]
    inds = sub2ind(depth.shape, velo_pts_im[:, 1], velo_pts_im[:, 0])
    dupe_inds = [item for item, count in Counter(inds).items() if count > 1]
    for dd in dupe_inds:
        pts = np.where(inds == dd)[0]
        x_loc = int(velo_pts_im[pts[0], 0])
        y_loc = int(velo_pts_im[pts[0], 1])
        depth[y_loc, x_loc] = velo_pts_im[pts, 2].min()
    depth[depth < 0] = 0
    return depth
