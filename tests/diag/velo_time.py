#!/usr/bin/env python3
"""GPU box: what the Velodyne ground truth of one evaluation batch costs (gdn_velo_project).  B = 8 synthetic
scans of 120 000 points (64 rings x 1875 azimuths over a ground plane and a far wall, KITTI's calibration magnitudes), images
375 x 1242.

Forms, microseconds per call, alternated over `rounds` rounds, median / min / max:
  project      gdn_velo_project alone, points and table already on the device (window of 100 calls on one stream, device events)
  h2d          the pinned host-to-device copy of the batch's points alone (15.4 MB; window of 20)
  numpy        the float64 numpy restatement of the same batch on the host (tests/velo_numpy.py), which is what the kernel
               replaces (wall clock, one call per round)
  metrics      gdn_depth_metrics_std on the projected pool (kind 0, Garg crop, no median scaling; window of 100)
and the bytes gdn_velo_project moves per second: the points once, the pool three times (memset, finalise read and write), 4
bytes per kept point.  What bounds the kernel is not profiled here.

usage: velo_time.py [rounds = 3] [--out FILE]"""
import json
import pathlib
import statistics
import sys
import time

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(HERE.parent)); sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "gdn-pytorch_amd"))

import numpy as np
import torch
import velo_numpy as V
import velo_synth as Y
from gdn_amd import ops
from gdn_amd.calculate_error import eval_boxes
from gdn_amd.datasets import assemble_scans

out = None
if "--out" in sys.argv:
    i = sys.argv.index("--out")
    out = sys.argv[i + 1]
    del sys.argv[i:i + 2]
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B, RINGS, AZ, H0, W0 = 8, 64, 1875, 375, 1242
dev = torch.device("cuda:0")


def scan(seed):
    """One revolution: each ray meets the ground plane 1.73 m below the scanner or a wall 60 m away, whichever is nearer."""
    r = np.random.RandomState(seed)
    el = np.deg2rad(np.linspace(2.0, -24.8, RINGS))[:, None]
    az = np.linspace(-np.pi, np.pi, AZ, endpoint=False)[None, :] + r.uniform(0, 1e-3)
    with np.errstate(divide="ignore"):
        rng = np.minimum(np.where(el < 0, 1.73 / np.maximum(-np.sin(el), 1e-9), np.inf), 60.0 / np.cos(el))
    rng = rng * (1 + r.normal(0, 0.002, (RINGS, AZ)))
    x, y, z = rng * np.cos(el) * np.cos(az), rng * np.cos(el) * np.sin(az), rng * np.sin(el)
    return np.stack([x, y, z, r.uniform(0, 1, x.shape)], -1).reshape(-1, 4).astype(np.float32)


def window(step, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def spread(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


cam, velo = Y.calib_arrays(seed=0, w0=W0, h0=H0)
P, size = Y.compose(cam, velo, 2)
clouds = [scan(s) for s in range(B)]
assert all(len(c) == RINGS * AZ == 120000 for c in clouds)
points, offsets, proj, sizes, Hmax, Wmax, size_list = assemble_scans([(c, P, size) for c in clouds], dev)
pred = torch.from_numpy(np.clip(0.7 - 1.5 * np.linspace(0, 1, 128)[:, None] + np.zeros((B, 1, 128, 416)), -1, 1).astype(np.float32)).to(dev)
boxes = eval_boxes(size_list, "garg").to(dev)
stage = torch.from_numpy(np.concatenate(clouds)).pin_memory()
landing = torch.empty_like(points)
pool, hits = ops.velo_project(points, offsets, proj, sizes, Hmax, Wmax, hits=True, max_points=120000)
torch.cuda.synchronize()


def host():
    t = time.perf_counter()
    V.restate_batch(clouds, [P] * B, [size] * B, Hmax, Wmax, 0)
    return (time.perf_counter() - t) * 1e6


forms = {
    "project": lambda: window(lambda: ops.velo_project(points, offsets, proj, sizes, Hmax, Wmax, hits=True, max_points=120000), 100),
    "h2d": lambda: window(lambda: landing.copy_(stage, non_blocking=True), 20),
    "numpy": host,
    "metrics": lambda: window(lambda: ops.depth_metrics_std(pool, ops.GT_METRES, boxes, pred), 100),
}
for k, f in forms.items():
    if k != "numpy":
        f()
us = {k: [] for k in forms}
for _ in range(rounds):
    for k, f in forms.items():
        us[k].append(f())
want, want_hits = V.restate_batch(clouds, [P] * B, [size] * B, Hmax, Wmax, 0)
same = bool(np.array_equal(pool.cpu().numpy().view(np.uint32), want.view(np.uint32)) and hits.cpu().tolist() == want_hits.tolist())
def kept_points(c):
    """The points of one scan that reach the atomic: in front of the scanner and inside the image."""
    x, y, z = (c[:, i].astype(np.float64) for i in range(3))
    r = [((P[i, 0] * x + P[i, 1] * y) + P[i, 2] * z) + P[i, 3] for i in range(3)]
    with np.errstate(all="ignore"):
        u, v = np.rint(r[0] / r[2]) - 1, np.rint(r[1] / r[2]) - 1
    return int(((x >= 0) & (u >= 0) & (v >= 0) & (u < W0) & (v < H0)).sum())


kept = sum(kept_points(c) for c in clouds)
moved = points.numel() * 4 + 3 * pool.numel() * 4 + 4 * kept
res = {"batch": B, "points_per_scan": RINGS * AZ, "image": [H0, W0], "rounds": rounds,
       "us_per_call": {k: spread(v) for k, v in us.items()}, "rounds_us": {k: [round(x, 2) for x in v] for k, v in us.items()},
       "hits_per_image": hits.cpu().tolist(), "points_kept": kept, "bitwise_equal_to_restatement": same,
       "bytes_moved": moved, "gb_per_s": round(moved / statistics.median(us["project"]) / 1e3, 1)}
for k, v in res["us_per_call"].items():
    print("%-8s %s us per call" % (k, v))
print("project: %d bytes per call, %.1f GB/s; hits per image %s; equal to the restatement: %s"
      % (moved, res["gb_per_s"], res["hits_per_image"], same))
line = json.dumps(res)
print(line)
if out:
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text(line + "\n")
