#!/usr/bin/env python3
"""GPU box: what the dense depth of one preparation batch costs (gdn_depth_densify, gdn_depth_encode_u8).
B = 8 synthetic scans of 120 000 points (64 rings x 1875 azimuths over a ground plane and a far wall, KITTI's calibration
magnitudes), projected at 128 x 416 and at 375 x 1242.

Forms per size, microseconds per call, alternated over `rounds` rounds, median / min / max:
  densify      gdn_depth_densify alone on the projected pool (window of 100 calls on one stream, device events): 4 launches
  chain        gdn_velo_project + gdn_depth_densify + gdn_depth_encode_u8 twice (sparse with keep_valid, dense): the device
               work of one gdn_amd.prepare_kitti batch, 2 memset nodes and 8 launches (window of 100)
  h2d          the pinned host-to-device copy of the batch's points alone (15.4 MB; window of 20)
  numpy        the numpy restatement of the fill on the same batch on the host (tests/densify_numpy.py; wall clock, one call
               per round)
and the bytes gdn_depth_densify moves at the least: the input pool once, `out` three times (written, extended in place,
rewritten), the workspace twice -- 7 pool passes with the halo re-reads of the tiled launches left out.  What bounds the
kernels is NOT profiled here.

usage: densify_time.py [rounds = 3] [--out FILE] [--only HxW]"""
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
import densify_numpy as Z
import velo_synth as Y
from gdn_amd import ops
from gdn_amd.datasets import assemble_scans

out = None
if "--out" in sys.argv:
    i = sys.argv.index("--out")
    out = sys.argv[i + 1]
    del sys.argv[i:i + 2]
only = None
if "--only" in sys.argv:                 # one size alone, e.g. under a kernel trace: --only 128x416
    i = sys.argv.index("--only")
    only = tuple(int(v) for v in sys.argv[i + 1].split("x"))
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
clouds = [scan(s) for s in range(B)]
stage = torch.from_numpy(np.concatenate(clouds)).pin_memory()
results = {}
for H, W in ((128, 416), (H0, W0)):
    if only not in (None, (H, W)):
        continue
    P, size = Y.compose(cam, velo, 2, size=(H, W))
    points, offsets, proj, sizes, Hmax, Wmax, _ = assemble_scans([(c, P, size) for c in clouds], dev)
    landing = torch.empty_like(points)
    sparse = ops.velo_project(points, offsets, proj, sizes, Hmax, Wmax, max_points=120000)
    dense = torch.empty_like(sparse)
    ops.depth_densify(sparse, sizes, out=dense)
    torch.cuda.synchronize()
    sparse_np = sparse.cpu().numpy()

    def chain():
        s = ops.velo_project(points, offsets, proj, sizes, Hmax, Wmax, max_points=120000)
        d = ops.depth_densify(s, sizes, out=dense)
        ops.depth_encode_u8(s, 80.0, keep_valid=True)
        ops.depth_encode_u8(d, 80.0)

    def host():
        t = time.perf_counter()
        Z.densify_pool(sparse_np, [size] * B)
        return (time.perf_counter() - t) * 1e6

    forms = {
        "densify": lambda: window(lambda: ops.depth_densify(sparse, sizes, out=dense), 100),
        "chain": lambda: window(chain, 100),
        "h2d": lambda: window(lambda: landing.copy_(stage, non_blocking=True), 20),
        "numpy": host,
    }
    for k, f in forms.items():
        if k != "numpy":
            f()
    us = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            us[k].append(f())
    ops.depth_densify(sparse, sizes, out=dense)
    got = dense.cpu().numpy()
    want = Z.densify_pool(sparse_np, [size] * B)
    same = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
    moved = 7 * sparse.numel() * 4
    res = {"image": [H, W], "us_per_call": {k: spread(v) for k, v in us.items()},
           "rounds_us": {k: [round(x, 2) for x in v] for k, v in us.items()}, "launches": {"densify": 4, "chain": 8},
           "sparse_filled": round(float((sparse_np > 0).mean()), 4), "dense_filled": round(float((got > 0).mean()), 4),
           "bitwise_equal_to_restatement": same, "bytes_moved_densify": moved, "h2d_bytes": stage.numel() * 4,
           "gb_per_s_densify": round(moved / statistics.median(us["densify"]) / 1e3, 1)}
    results["%dx%d" % (H, W)] = res
    for k, v in res["us_per_call"].items():
        print("%4d x %4d  %-8s %s us per call" % (H, W, k, v))
    print("%4d x %4d  densify: 4 launches, %d bytes per call at the least, %.1f GB/s; sparse %.1f %% -> dense %.1f %% filled; equal "
          "to the restatement: %s" % (H, W, moved, res["gb_per_s_densify"], 100 * res["sparse_filled"], 100 * res["dense_filled"], same))
line = json.dumps({"batch": B, "points_per_scan": RINGS * AZ, "rounds": rounds, "sizes": results})
print(line)
if out:
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text(line + "\n")
