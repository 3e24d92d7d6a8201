#!/usr/bin/env python3
"""GPU box: time the device-side NYU training transform (gdn_nyu_augment, one B=20 batch of 320x420 sources -> 224x320,
DtoD and RtoD) and the host chain it replaces (the reference's Pillow / SciPy calls, one sample at a time on one core)."""
import pathlib
import random
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
for p in (ROOT, ROOT / "gdn-pytorch_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))
import numpy as np
import torch
from gdn_amd import ops
from gdn_amd.datasets import draw_params_nyu
from test_nyu_augment_cpu import _reference_chain, synthetic_nyu

dev = torch.device("cuda:0")
B, H0, W0, H, W = 20, 320, 420, 224, 320
r = np.random.RandomState(0)
srcs = [synthetic_nyu(r, H0, W0) for _ in range(B)]
depth = torch.from_numpy(np.stack([s[0] for s in srcs])).to(dev)
rgb = torch.from_numpy(np.stack([s[1] for s in srcs])).to(dev)
for mode in ("DtoD", "RtoD"):
    py, npr = random.Random(0), np.random.RandomState(0)
    draws = [draw_params_nyu(H0, W0, mode, py, npr) for _ in range(B)]
    for _ in range(3):
        ops.nyu_augment(depth, rgb, draws, H, W, mode)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 50
    e0.record()
    for _ in range(n):
        ops.nyu_augment(depth, rgb, draws, H, W, mode)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    packed = torch.from_numpy(ops.nyu_params(draws, H, W, mode).view(np.uint8)).to(dev)
    e0.record()
    for _ in range(n):
        ops.nyu_augment(depth, rgb, packed, H, W, mode)
    e1.record()
    torch.cuda.synchronize()
    ms_dev = e0.elapsed_time(e1) / n
    print("GPU %s: %.3f ms per batch of %d (%dx%d -> %dx%d) = %.0f img/s; %.3f ms with the host packing of the draws"
          % (mode, ms_dev, B, H0, W0, H, W, B / ms_dev * 1e3, ms))
    t0 = time.perf_counter()
    k = 4
    for b in range(k):
        _reference_chain(srcs[b][0], srcs[b][1], draws[b], mode, H, W)
    host = (time.perf_counter() - t0) / k * 1e3
    print("host %s (1 core, Pillow + scipy.ndimage chain): %.1f ms per sample = %.1f img/s; a batch of %d = %.0f ms"
          % (mode, host, 1e3 / host, B, host * B))
