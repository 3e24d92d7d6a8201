#!/usr/bin/env python3
"""What the training loops themselves cost on the host per batch, against another trainer.py.  A diagnostic,
not a test; needs no GPU.

Runs trainer.train_AE_DtoD / train_AE_RtoD for one epoch of `--batches` batches with everything heavy replaced by a
function that returns at once (the model returns its input, the losses three zeros, backward / all-reduce / optimizer / checkpoint /
state file nothing), so the time per batch is the loop's own: taking the batch, the stepper, the counters, the cadence tests, the state-file
bookkeeping and the two prints every 50 / 100 batches (into a buffer).  With --parent-trainer FILE the same for that file's
loops (the parent commit's trainer.py), the two alternated over `--reps` rounds, the order swapped every round.

usage: loop_host_time.py [--batches 20000] [--reps 7] [--parent-trainer FILE]"""
import argparse
import contextlib
import importlib.util
import io
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "gdn-pytorch_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=20000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--parent-trainer", default=None)
opt = ap.parse_args()

import torch
from gdn_amd import distributed as D
from gdn_amd import trainer as T
from gdn_amd import utils as U

mods = {"this": T}
if opt.parent_trainer:
    spec = importlib.util.spec_from_file_location("gdn_amd.trainer_parent", opt.parent_trainer)
    parent = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = parent
    spec.loader.exec_module(parent)
    mods["parent"] = parent
zero = torch.zeros(())
U.dtod_loss = U.rtod_pixel_loss = lambda *a, **k: (zero, zero, zero)
U.backward = lambda loss: None
D.sync_gradients = lambda model, optimizer: None
for mod in mods.values():
    mod._save_checkpoint = mod.save_training_state = lambda *a, **k: None


class Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x, istrain=False):
        return x


class Optimizer:
    param_groups, micro_batches = [{"lr": 1e-5}], 1

    def zero_grad(self):
        pass

    def step(self):
        pass


class Loader:
    batch = (torch.zeros(2, 1, 1, 2), torch.zeros(2, 3, 1, 2), torch.zeros(2, 1, 1, 2))

    def __len__(self):
        return opt.batches

    def __iter__(self):
        for _ in range(opt.batches):
            yield self.batch


def us_per_batch(mod, mode, flags):
    args = argparse.Namespace(dataset="KITTI", mode="DtoD" if mode == "DtoD" else "RtoD_single", **flags)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        if mode == "DtoD":
            mod.train_AE_DtoD(args, Model(), None, None, Optimizer(), Loader(), None, 2, 1, 2e-5, None, None)
        else:
            mod.train_AE_RtoD(args, Model(), None, None, None, Optimizer(), Loader(), None, 2, 1, 2e-5, None, None)
    return (time.perf_counter() - t0) / opt.batches * 1e6


for mode, flags in (("DtoD", {}), ("RtoD_single", {}), ("DtoD", {"accum_steps": 2}), ("DtoD", {"save_state_every": 1000})):
    got = {name: [] for name in mods}
    for r in range(opt.reps):
        for name in (list(mods) if r % 2 == 0 else list(mods)[::-1]):
            got[name].append(us_per_batch(mods[name], mode, flags))
    print("%-12s %-28s" % (mode, flags or "") + "   ".join(
        "%s %6.2f us/batch (min %.2f, max %.2f)" % (name, statistics.median(v), min(v), max(v)) for name, v in got.items()))
