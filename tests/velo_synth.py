"""Synthetic raw-KITTI material for the Velodyne tests: a calibration pair with KITTI's magnitudes, clouds whose projected
coordinates are placed on purpose, and a raw tree on disk."""
import pathlib

import numpy as np


def calib_arrays(seed=0, w0=1242, h0=375):
    """{key: array} of the two files: a velo-to-cam rotation near KITTI's axis swap, a rectifying rotation near identity."""
    r = np.random.RandomState(seed)

    def near(R, eps):
        q, _ = np.linalg.qr(R + r.uniform(-eps, eps, (3, 3)))        # orthonormal; QR leaves each column's sign open
        return q @ np.diag(np.sign(np.diag(q.T @ R)))
    R = near(np.array([[0., -1, 0], [0, 0, -1], [1, 0, 0]]), 0.02)
    f = 721.5377 * w0 / 1242.0
    cam = {}
    for c, bx in ((2, 44.85728), (3, -339.5242)):
        cam["S_rect_0%d" % c] = np.array([float(w0), float(h0)])
        cam["P_rect_0%d" % c] = np.array([f, 0, 0.49 * w0 + c, bx * w0 / 1242.0, 0, f, 0.46 * h0 + c, 0.2163791, 0, 0, 1, 0.002745884])
    cam["R_rect_00"] = near(np.eye(3), 0.01).reshape(9)
    velo = {"R": R.reshape(9), "T": np.array([-0.004069766, -0.07631618, -0.2717806]) + r.uniform(-0.01, 0.01, 3)}
    return cam, velo


def write_calib(date_dir, seed=0, w0=1242, h0=375):
    date_dir = pathlib.Path(date_dir)
    date_dir.mkdir(parents=True, exist_ok=True)
    cam, velo = calib_arrays(seed, w0, h0)
    fmt = lambda d: "".join("%s: %s\n" % (k, " ".join(repr(float(x)) for x in v)) for k, v in d.items())
    (date_dir / "calib_cam_to_cam.txt").write_text("calib_time: 09-Jan-2012 13:57:47\ncorner_dist: 9.950000e-02\n" + fmt(cam))
    (date_dir / "calib_velo_to_cam.txt").write_text("calib_time: 15-Mar-2012 11:37:16\n" + fmt(velo) +
                                                    "delta_f: 0.000000e+00 0.000000e+00\n")
    return cam, velo


def compose(cam, velo, c=2, size=None):
    """The specification's P, written out independently of gdn_amd.kitti_raw."""
    P_rect = cam["P_rect_0%d" % c].reshape(3, 4).copy()
    w0, h0 = (int(v) for v in cam["S_rect_0%d" % c])
    if size is not None:
        P_rect[0] *= size[1] / w0
        P_rect[1] *= size[0] / h0
        h0, w0 = size
    R4 = np.eye(4)
    R4[:3, :3] = cam["R_rect_00"].reshape(3, 3)
    T4 = np.vstack([np.hstack([velo["R"].reshape(3, 3), velo["T"].reshape(3, 1)]), [[0, 0, 0, 1.0]]])
    return np.dot(np.dot(P_rect, R4), T4), (int(h0), int(w0))


def cloud_at(P, pix_u, pix_v, depth, r, margin=0.05):
    """Points whose projected 1-based coordinates are pix + 1 + offset with |offset| <= 0.5 - margin, at camera depth `depth`:
    back-projected through P in float64, stored as float32 (which moves the projection by ~1e-4 px at most)."""
    n = len(pix_u)
    a = np.asarray(pix_u, np.float64) + 1.0 + r.uniform(-(0.5 - margin), 0.5 - margin, n)
    b = np.asarray(pix_v, np.float64) + 1.0 + r.uniform(-(0.5 - margin), 0.5 - margin, n)
    Z = np.asarray(depth, np.float64)
    rhs = np.stack([a * Z, b * Z, Z]) - P[:, 3:4]
    X = np.linalg.solve(P[:, :3], rhs).T
    return np.concatenate([X, r.uniform(0, 1, (n, 1))], axis=1).astype(np.float32)


def seeded_cloud(P, size, n, seed, first_col=0, behind=0.1):
    """n points spread over (and a little beyond) an image of `size`, several per pixel, plus `behind` x n points behind the
    scanner.  first_col: the lowest pixel column that is used."""
    r = np.random.RandomState(seed)
    h0, w0 = size
    u = r.randint(first_col, w0 + 2, n)
    v = r.randint(-1, h0 + 2, n)
    pts = cloud_at(P, u, v, r.uniform(4.0, 80.0, n), r)
    back = pts[: int(behind * n)].copy()
    back[:, 0] = -np.abs(back[:, 0]) - 0.5
    out = np.concatenate([pts, back])
    return out[r.permutation(len(out))]


def write_scan(raw_root, date, drive, frame, points):
    d = pathlib.Path(raw_root) / date / drive / "velodyne_points" / "data"
    d.mkdir(parents=True, exist_ok=True)
    np.asarray(points, np.float32).tofile(d / ("%010d.bin" % frame))
    return d / ("%010d.bin" % frame)
