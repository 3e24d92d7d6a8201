#!/usr/bin/env python3
"""Host time of optimizer.step(): the Python around the launches, this tree's gdn_amd/optim.py against another revision's.

The work the GPU receives is pinned elsewhere (tests/test_optim_launch_order_cpu.py); what a change to optim.py can still
cost is host time, so the launches are stubbed out (as in that test) and no queue back-pressure from 72 M-element kernels
enters.  Needs no GPU: AutoEncoder_DtoD's parameters (one arena) live on the CPU, loose parameters do not occur.
    forms      host path / capturable / guard + EMA (max_grad_norm, skip_nonfinite, ema_decay) / schedule (cosine) /
               segmented / seg + all (segmented with the guard, the average and the schedule)
    coverage   full: one launch per step;  frozen: res512_3 has no gradient -- the per-tensor path, one launch (and one
               gathered record, one EMA launch) per remaining parameter, where the host cost is largest; a segmented
               optimizer stays on one launch there (res512_3 is requires_grad False: its chunks are skipped)
A window is a fresh optimizer, 20 warm-up steps and time.perf_counter around `steps` calls of step().  With --parent-optim
FILE that file is loaded as a second module and the two alternate, `rounds` windows each per form.
Bar, per form: this tree's median <= the parent's median + (the parent's max - min over its rounds).  Exit status 1 if a
form misses it.  On a host without a GPU the parent's capturable path cannot ask whether its stream is capturing (its
refusals did not ask torch.cuda.is_available() first), so that one query is answered False for both modules.
--stub-intact: ParamArena.intact() answers True without looking.  step() asks it once per parameter and it compares every
item's pointer, 124 x 124 comparisons per step that are the same code on both sides and most of the time measured; without
them the numbers are those of the code that differs, and the parent's spread -- the bar -- is narrower.

usage: optim_host_time.py [--steps 200] [--rounds 5] [--parent-optim FILE] [--stub-intact] [--out FILE]"""
import argparse
import importlib.util
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "gdn-pytorch_amd"))
import torch
import gdn_amd.AE_model_unet as M
from gdn_amd import engine as E
from gdn_amd import ops
from gdn_amd import optim as new_optim

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--parent-optim", default=None)
ap.add_argument("--stub-intact", action="store_true")
ap.add_argument("--out", default=None)
opt = ap.parse_args()
rounds = max(5, opt.rounds) if opt.parent_optim else opt.rounds

modules = {"this tree": new_optim}
if opt.parent_optim:
    spec = importlib.util.spec_from_file_location("gdn_amd.optim_parent", opt.parent_optim)
    parent = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = parent
    spec.loader.exec_module(parent)
    modules["parent"] = parent
if not torch.cuda.is_available():
    torch.cuda.is_current_stream_capturing = lambda: False

for name in ("adam_step", "adam_step_dev", "adam_step_dev_guarded", "grad_sumsq", "grad_guard_finalize", "ema_update", "swap_",
             "adam_step_seg", "grad_sumsq_seg", "ema_update_seg", "lr_schedule"):
    setattr(ops, name, lambda *a, **k: None)
ops.zeros = lambda shape, device: torch.zeros(shape, dtype=torch.float32, device=device)

torch.manual_seed(0)
model = M.AutoEncoder_DtoD(input_dim=1, height=128, width=416)
ar = E.ParamArena(model, torch.device("cpu"))
model._gdn_param_arena = ar
if opt.stub_intact:
    ar.intact = lambda: True
frozen = {id(p) for p in model.res512_3.parameters()}
GUARD_EMA = {"max_grad_norm": 1.0, "skip_nonfinite": True, "ema_decay": 0.999}
SCHED = {"kind": "cosine", "warmup": 100, "total": 100000, "floor": 0.1}
FORMS = [("host path", {}), ("capturable", {"capturable": True}), ("guard + EMA", GUARD_EMA),
         ("schedule", {"schedule": SCHED}), ("segmented", {"segmented": True}),
         ("seg + all", dict(GUARD_EMA, segmented=True, schedule=SCHED))]
KW = dict(lr=2e-5, betas=[0.9, 0.999], eps=1e-8, weight_decay=5e-4)


def window(mod, kw, freeze):
    for p in model.parameters():
        p.requires_grad_(not (freeze and id(p) in frozen))
        p.grad = ar.grad_view(p) if p.requires_grad else None
    o = mod.Adam(model.parameters(), **KW, **kw)
    for _ in range(20):
        o.step()
    t0 = time.perf_counter()
    for _ in range(opt.steps):
        o.step()
    return (time.perf_counter() - t0) / opt.steps * 1e6          # us per step


cases = [(form, kw, cov) for form, kw in FORMS for cov in ("full", "frozen")]
times = {(form, cov, who): [] for form, _, cov in cases for who in modules}
for r in range(rounds):
    for form, kw, cov in cases:
        for who, mod in modules.items():
            times[(form, cov, who)].append(window(mod, kw, cov == "frozen"))

n_launch = sum(1 for p in model.parameters() if id(p) not in frozen)
lines = ["optimizer.step() host time, launches stubbed: AutoEncoder_DtoD, %d parameters in one arena (frozen: %d per-tensor "
         "updates), %d steps per window, %d alternated rounds%s; us per step" %
         (len(ar.items), n_launch, opt.steps, rounds, ", ParamArena.intact() stubbed" if opt.stub_intact else ""),
         "%-12s %-7s %-10s %9s %9s %9s" % ("form", "cover", "module", "median", "min", "max")]
missed = []
for form, _, cov in cases:
    for who in modules:
        t = times[(form, cov, who)]
        lines.append("%-12s %-7s %-10s %9.2f %9.2f %9.2f" % (form, cov, who, statistics.median(t), min(t), max(t)))
    if "parent" in modules:
        mine, theirs = times[(form, cov, "this tree")], times[(form, cov, "parent")]
        bar = statistics.median(theirs) + (max(theirs) - min(theirs))
        ok = statistics.median(mine) <= bar
        lines.append("%-12s %-7s %-10s %9.2f  %s" % ("", "", "bar", bar, "met" if ok else "MISSED"))
        if not ok:
            missed.append("%s, %s" % (form, cov))
text = "\n".join(lines)
print(text)
if opt.out:
    with open(opt.out, "a") as f:
        f.write(text + "\n")
sys.exit(1 if missed else 0)
