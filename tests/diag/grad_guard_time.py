#!/usr/bin/env python3
"""GPU box: what the gradient guard costs per optimizer.step() at the parameter arena of AutoEncoder_DtoD 128x416.

Three optimizers over the same arena, alternated in one process, each window timed with device events after a warm-up:
    capturable           Adam(capturable=True)                         prep + update                 (2 launches)
    guarded, idle        Adam(max_grad_norm=1e30, skip_nonfinite=True) + partial sums, final sum, decision (5 launches)
    guarded, clipping    Adam(max_grad_norm=1e-6, skip_nonfinite=True) the same launches, coef < 1
and, on its own, gdn_grad_sumsq over the arena (its two launches): bytes read per second as a share of the measured float4
copy rate of this chip (6.29 TB/s).  The kernel reads 4 bytes per parameter once and does two double operations per
element, so the bound that applies is memory bandwidth; below a few MB the two launches are what is measured instead.
Prints the best and the median window of each form, the shader clock held during the last window, and one JSON line.

usage: grad_guard_time.py [steps per window = 200] [rounds = 5] [--out FILE]"""
import contextlib
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "gdn-pytorch_amd"))
import torch
import gdn_amd.AE_model_unet as M
from gdn_amd import engine as E
from gdn_amd import ops
from gdn_amd.optim import Adam

COPY_RATE = 6.29e12          # bytes/s, measured float4 copy on this chip
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if out in argv:
    argv.remove(out)
steps = max(200, int(argv[0])) if argv else 200
rounds = int(argv[1]) if len(argv) > 1 else 5
dev = torch.device("cuda:0")

torch.manual_seed(0)
model = M.AutoEncoder_DtoD(input_dim=1, height=128, width=416).to(dev).train()
ar = E.ParamArena(model, dev)
for p, o, n, tr in ar.items:                      # a gradient in every parameter's slice; the alignment padding stays zero
    ar.grad[o:o + n].normal_(0.0, 1e-3)
    p.grad = ar.grad_view(p)
nbytes = 4 * ar.numel
kw = dict(lr=2e-5, betas=[0.9, 0.999], eps=1e-8, weight_decay=5e-4)
forms = [("capturable", Adam(model.parameters(), capturable=True, **kw)),
         ("guarded, idle", Adam(model.parameters(), max_grad_norm=1e30, skip_nonfinite=True, **kw)),
         ("guarded, clipping", Adam(model.parameters(), max_grad_norm=1e-6, skip_nonfinite=True, **kw))]
rec = torch.zeros(32, dtype=torch.uint8, device=dev)
calls = [(name, opt.step) for name, opt in forms] + [("gdn_grad_sumsq alone", lambda: ops.grad_sumsq(ar.grad, rec))]


def window(fn, clock=False):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    clk = ops.ShaderClock(dev) if clock else None
    with clk if clk is not None else contextlib.nullcontext():
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
    torch.cuda.synchronize()
    ghz = clk.ghz() if clk is not None else None
    return e0.elapsed_time(e1) / steps * 1e3, ghz          # us per call


times = {name: [] for name, _ in calls}
ghz = {}
for r in range(rounds):
    for name, fn in calls:
        t, g = window(fn, clock=r == rounds - 1)
        times[name].append(t)
        if g is not None:
            ghz[name] = g
gs = {name: opt.guard_stats() for name, opt in forms[1:]}
assert gs["guarded, idle"]["clipped"] == 0 and gs["guarded, clipping"]["clipped"] == gs["guarded, clipping"]["steps"]
assert gs["guarded, idle"]["skipped"] == 0 and gs["guarded, clipping"]["skipped"] == 0

print("arena: %d floats (%.1f MB), %d steps per window, %d alternated rounds" % (ar.numel, nbytes / 1e6, steps, rounds))
res = {"arena_floats": ar.numel, "steps_per_window": steps, "rounds": rounds, "forms": {}}
for name, _ in calls:
    best, med = min(times[name]), statistics.median(times[name])
    res["forms"][name] = {"best_us": round(best, 2), "median_us": round(med, 2), "max_us": round(max(times[name]), 2),
                          "clock_ghz": None if name not in ghz else round(ghz[name], 3)}
    print("%-22s best %8.2f us  median %8.2f us  max %8.2f us  clock %s GHz" %
          (name, best, med, max(times[name]), "n/a" if name not in ghz else "%.3f" % ghz[name]))
base = res["forms"]["capturable"]["median_us"]
for name in ("guarded, idle", "guarded, clipping"):
    print("%-22s +%.2f us per step over the capturable update (medians)" % (name, res["forms"][name]["median_us"] - base))
t = res["forms"]["gdn_grad_sumsq alone"]["median_us"] * 1e-6
rate = nbytes / t
res["sumsq_bytes_per_s"] = rate
res["sumsq_share_of_copy_rate"] = rate / COPY_RATE
print("gdn_grad_sumsq: %.1f MB in %.2f us = %.2f TB/s = %.1f %% of the %.2f TB/s float4 copy rate (bound: memory bandwidth; "
      "both launches and the gap between them are in the time)" % (nbytes / 1e6, t * 1e6, rate / 1e12, 100 * rate / COPY_RATE,
                                                                  COPY_RATE / 1e12))
line = json.dumps(res)
print(line)
if out:
    pathlib.Path(out).write_text(line + "\n")
