"""Raw KITTI on the host: the calibration files of a recording date and the lists that name Velodyne scans (--eval_velodyne,
DESIGN.md 3.15).  numpy only; the projection itself runs on the device (ops.velo_project).

A raw KITTI tree is ``ROOT/DATE/calib_cam_to_cam.txt``, ``ROOT/DATE/calib_velo_to_cam.txt``,
``ROOT/DATE/DRIVE/velodyne_points/data/%010d.bin`` (float32 x, y, z, reflectance per point) and, for the training-set
preparation (gdn_amd.prepare_kitti), the colour frames ``ROOT/DATE/DRIVE/image_0C/data/%010d.png``."""
import os
import pathlib

import numpy as np

from ._lib import GdnError

CALIB_FILES = ("calib_cam_to_cam.txt", "calib_velo_to_cam.txt")


def read_calib(path):
    """A KITTI calibration file -> {key: float64 array}.  Every line is ``key: v v v ...``; a line whose values are not all
    numbers (calib_time) is skipped."""
    data = {}
    try:
        with open(path) as f:
            lines = f.readlines()
    except OSError as e:
        raise GdnError("cannot read the calibration file %s: %s" % (path, e)) from e
    for line in lines:
        key, sep, value = line.partition(":")
        if not sep or not value.split():
            continue
        try:
            data[key.strip()] = np.array([float(v) for v in value.split()], dtype=np.float64)
        except ValueError:
            continue
    return data


def _field(calib, key, n, path):
    if key not in calib or calib[key].size != n:
        raise GdnError("%s: no %s of %d numbers" % (path, key, n))
    return calib[key]


def projection(date_dir, cam=2, size=None):
    """(P [3,4] float64, (h0, w0)) of camera `cam` of the recording date in date_dir: P = P_rect_0cam . R4 . T4, R4 the 4 x 4
    identity with R_rect_00 in its top-left corner, T4 = [[R | T], [0 0 0 1]] of the velo-to-cam file, composed with np.dot
    in that order.  (h0, w0) is S_rect_0cam, which stores the width first; no image is opened.  size=(H, W): rows 0 and 1
    of P_rect are scaled by W / w0 and H / h0 first, and (H, W) is returned -- sparse maps at another resolution."""
    date_dir = pathlib.Path(date_dir)
    c2c_path, v2c_path = (date_dir / n for n in CALIB_FILES)
    c2c, v2c = read_calib(c2c_path), read_calib(v2c_path)
    T4 = np.eye(4, dtype=np.float64)
    T4[:3, :3] = _field(v2c, "R", 9, v2c_path).reshape(3, 3)
    T4[:3, 3] = _field(v2c, "T", 3, v2c_path)
    R4 = np.eye(4, dtype=np.float64)
    R4[:3, :3] = _field(c2c, "R_rect_00", 9, c2c_path).reshape(3, 3)
    P_rect = _field(c2c, "P_rect_0%d" % cam, 12, c2c_path).reshape(3, 4).copy()
    s = _field(c2c, "S_rect_0%d" % cam, 2, c2c_path)
    w0, h0 = int(s[0]), int(s[1])
    if h0 < 1 or w0 < 1:
        raise GdnError("%s: S_rect_0%d is %g x %g" % (c2c_path, cam, s[0], s[1]))
    if size is not None:
        H, W = int(size[0]), int(size[1])
        if H < 1 or W < 1:
            raise GdnError("projection: size %r" % (size,))
        P_rect[0] *= W / w0
        P_rect[1] *= H / h0
        h0, w0 = H, W
    return np.dot(np.dot(P_rect, R4), T4), (h0, w0)


def _parse_line(text):
    """One list line -> (date, drive, frame, cam), or None when it is in neither format."""
    toks = text.split()
    parts = toks[0].split("/")
    if len(parts) >= 5 and parts[-2] == "data" and parts[-3] in ("image_02", "image_03"):
        stem = parts[-1].rsplit(".", 1)[0]
        if stem.isdigit():                                      # DATE/DRIVE/image_0C/data/FRAME.png ...
            return parts[-5], parts[-4], int(stem), int(parts[-3][-1])
        return None
    if len(parts) == 2 and len(toks) >= 3 and toks[1].isdigit() and toks[2] in ("l", "r"):
        return parts[0], parts[1], int(toks[1]), 2 if toks[2] == "l" else 3     # DATE/DRIVE FRAME l|r
    return None


def parse_velo_list(list_file, raw_root):
    """One sample per non-empty line of list_file, in order -> [(scan file, date directory, cam), ...].  Two formats:
    ``DATE/DRIVE/image_0C/data/FRAME.png ...`` (camera C = 2 or 3) and ``DATE/DRIVE FRAME l|r`` (l: camera 2, r: camera 3).
    The scan is raw_root/DATE/DRIVE/velodyne_points/data/%010d.bin.  A line in neither format, a missing scan or a missing
    calibration file is a GdnError naming the file and the line."""
    return [(f["scan"], f["date_dir"], f["cam"]) for f in parse_frame_list(list_file, raw_root, images=False)]


def parse_frame_list(list_file, raw_root, images=True):
    """parse_velo_list with everything a line names -> [{date, drive, frame, cam, scan, date_dir, image}, ...]: image is the
    colour frame raw_root/DATE/DRIVE/image_0C/data/%010d.png, and with images=True a missing one is a GdnError like a missing
    scan (gdn_amd.prepare_kitti)."""
    raw_root = pathlib.Path(raw_root)
    out = []
    with open(list_file) as f:
        for no, line in enumerate(f, 1):
            text = line.strip()
            if not text:
                continue
            where = "%s line %d (%r)" % (list_file, no, text)
            parsed = _parse_line(text)
            if parsed is None:
                raise GdnError("%s: neither DATE/DRIVE/image_0C/data/FRAME.png nor DATE/DRIVE FRAME l|r" % where)
            date, drive, frame, cam = parsed
            scan = raw_root / date / drive / "velodyne_points" / "data" / ("%010d.bin" % frame)
            image = raw_root / date / drive / ("image_0%d" % cam) / "data" / ("%010d.png" % frame)
            for need in (scan, *(raw_root / date / n for n in CALIB_FILES), *((image,) if images else ())):
                if not os.path.isfile(need):
                    raise GdnError("%s not found, named by %s" % (need, where))
            out.append({"date": date, "drive": drive, "frame": frame, "cam": cam, "scan": scan, "date_dir": raw_root / date,
                        "image": image})
    return out
