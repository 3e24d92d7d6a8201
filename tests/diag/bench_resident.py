#!/usr/bin/env python3
"""GPU box: what a training run from FILES gets, next to the benchmark's no-input-work ceiling.

Writes a seeded KITTI-layout set (JPEG colour, PNG dense depth, PNG sparse depth with ~5 % valid pixels; default 2,000
samples at 128x416) to a temporary directory and times four loaders in one process, alternating them:
  (a) GpuAugmentLoader, workers=0      decode 3 x B files per batch on the calling thread (the default)
  (b) GpuAugmentLoader, workers=16     the same through a thread pool
  (c) GpuResidentLoader                decoded once, batches assembled on the device
  (d) SyntheticLoader                  ready-made device tensors: no input work at all
For each: the loader-only rate (one epoch at B=20, a device synchronise before the clock stops) and the DtoD training
rate at B=20 in fp32 and bf16 (>= 200 timed steps after a warm-up that has seen every shape; every configuration twice,
interleaved, so the spread is visible).  Also the preload's seconds and bytes.  Prints one JSON line at the end.

    python tests/diag/bench_resident.py [--samples 2000] [--steps 200] [--batch 20] [--trace-steps N]

--trace-steps N: only N resident training steps after a short warm-up (for `rocprofv3 --kernel-trace --stats -- python ...`:
batch assembly must show as ONE kernel and one small host-to-device copy per batch)."""
import argparse
import contextlib
import json
import pathlib
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "gdn-pytorch_amd"))
import numpy as np
import torch


def write_set(root, n, H, W, seed=0, per_scene=100):
    from PIL import Image
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    scenes = []
    for s in range((n + per_scene - 1) // per_scene):
        scene = "scene_%03d" % s
        scenes.append(scene)
        (root / scene / "color_gt2").mkdir(parents=True)
        (root / scene / "gt").mkdir()
        for i in range(min(per_scene, n - s * per_scene)):
            dense = np.clip(40 + 150 * yy / H + 30 * np.sin(xx / (11.0 + i % 17 + s)) + r.randint(0, 12, (H, W)), 0, 255).astype(np.uint8)
            sparse = np.where(r.rand(H, W) < 0.05, np.maximum(dense, 1), 0).astype(np.uint8)
            rgb = np.clip(np.stack([dense, dense[::-1], 255 - dense], 2).astype(np.int16) + r.randint(-25, 25, (H, W, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(rgb).save(root / scene / ("%07d.jpg" % i))
            Image.fromarray(dense).save(root / scene / "color_gt2" / ("%07d.png" % i))
            Image.fromarray(sparse).save(root / scene / "gt" / ("%07d.png" % i))
    (root / "train.txt").write_text("".join(s + "\n" for s in scenes))
    (root / "val.txt").write_text(scenes[-1] + "\n")


def make_trainer(dtype, dev, H, W):
    import gdn_amd.AE_model_unet as M
    from gdn_amd import utils as U
    from gdn_amd.optim import Adam
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        model = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W).to(dev)
    model.train().compute_dtype(dtype)
    opt = Adam(model.parameters(), 2e-5, [0.9, 0.999], eps=1e-08, weight_decay=5e-4)

    def step(batch):
        gt, _, sparse = batch
        out = model(gt, istrain=False)
        loss, _, _ = U.dtod_loss(out, gt, sparse)
        opt.zero_grad()
        U.backward(loss)
        opt.step()
        return loss
    return step


def endless(loader):
    while True:
        for b in loader:
            yield b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--trace-steps", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resident.py measures on the GPU; none is visible")
    from gdn_amd.datasets import GpuAugmentLoader, GpuResidentLoader, SequenceFolder
    from gdn_amd.synthetic import SyntheticLoader
    dev = torch.device("cuda:0")
    B, H, W = a.batch, a.height, a.width
    rec = {"samples": a.samples, "batch": B, "size": [H, W], "timed_steps": a.steps, "date": time.strftime("%Y-%m-%d")}
    with tempfile.TemporaryDirectory() as tmp:
        root = pathlib.Path(tmp)
        t0 = time.time()
        write_set(root, a.samples, H, W)
        rec["write_set_s"] = round(time.time() - t0, 1)
        ds = SequenceFolder(root, argparse.Namespace(img_test=False), seed=1, train=True)
        kw = dict(train=True, seed=3, drop_last=True)
        resident = GpuResidentLoader(ds, B, dev, **kw)
        rec["preload_s"], rec["preload_threads"] = round(resident.pools.seconds, 2), resident.pools.threads
        rec["resident_bytes"] = resident.pools.nbytes
        if a.trace_steps:
            step = make_trainer("fp32", dev, H, W)
            it = endless(resident)
            for _ in range(3 + a.trace_steps):
                step(next(it))
            torch.cuda.synchronize()
            print(json.dumps({"traced_resident_steps": a.trace_steps, "warmup": 3}))
            return
        loaders = {
            "a_files_workers0": GpuAugmentLoader(ds, B, dev, workers=0, **kw),
            "b_files_workers16": GpuAugmentLoader(ds, B, dev, workers=16, **kw),
            "c_resident": resident,
            "d_synthetic": SyntheticLoader(B, len(resident), H, W, seed=0, device=dev, distinct=4),
        }
        # loader-only rate: one epoch each, alternating, a synchronise before the clock stops
        rec["loader_only_img_s"] = {k: [] for k in loaders}
        for k, ld in loaders.items():                       # warm-up: code objects, pinned-memory pools, thread pools
            for i, _ in zip(range(3), ld):
                pass
        torch.cuda.synchronize()
        for rep in range(a.repeats):
            for k, ld in loaders.items():
                torch.cuda.synchronize()
                t0, n = time.perf_counter(), 0
                for batch in ld:
                    n += batch[0].shape[0]
                torch.cuda.synchronize()
                rec["loader_only_img_s"][k].append(round(n / (time.perf_counter() - t0), 1))
        # training rate
        rec["train_img_s"], rec["train_ms_per_step"] = {}, {}
        for dtype in ("fp32", "bf16"):
            step = make_trainer(dtype, dev, H, W)
            its = {k: endless(ld) for k, ld in loaders.items()}
            for k in its:                                   # every loader's shapes through the step before any timing
                for _ in range(a.warmup):
                    step(next(its[k]))
            torch.cuda.synchronize()
            rates = {k: [] for k in loaders}
            ms = {k: [] for k in loaders}
            for rep in range(a.repeats):
                for k in loaders:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        loss = step(next(its[k]))
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    rates[k].append(round(a.steps * B / dt, 1))
                    ms[k].append(round(dt / a.steps * 1e3, 2))
                    assert bool(torch.isfinite(loss)), (dtype, k)
            rec["train_img_s"][dtype], rec["train_ms_per_step"][dtype] = rates, ms
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
