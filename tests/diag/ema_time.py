#!/usr/bin/env python3
"""GPU box: what the weight average costs per optimizer.step() at the parameter arena of AutoEncoder_DtoD 128x416, and what
the two exchanges around a validation cost.

Two optimizers over the same arena, alternated in one process, each window timed with device events after a warm-up:
    capturable       Adam(capturable=True)       prep + update                    (2 launches; the step as it was)
    ema              Adam(ema_decay=0.999)       the same two + gdn_ema_update    (3 launches)
and, on its own, optimizer.swap_averaged() (gdn_swap_f32 over the arena, one launch), timed in pairs so the weights end
where they began.  Expectation from bytes moved: the update reads p, g, m, v and writes p, m, v (28 bytes per parameter), the
average reads p and ema and writes ema (12 more), so about 12/28 of the update KERNEL's time on top if both ran at the same
rate; an exchange moves 16 bytes per parameter.  An expectation, not a gate.
Prints the best and the median window of each form, bytes per second of the two new kernels, and one JSON line.

usage: ema_time.py [steps per window = 200] [rounds = 5] [--out FILE]"""
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

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if out in argv:
    argv.remove(out)
steps = max(50, int(argv[0])) if argv else 200
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
plain, ema = Adam(model.parameters(), capturable=True, **kw), Adam(model.parameters(), ema_decay=0.999, **kw)
ema.step()                                        # (makes the average)
st = ema.store_of(ar)


def two_swaps():
    ema.swap_averaged()
    ema.swap_averaged()


calls = [("capturable", plain.step), ("ema", ema.step),
         ("gdn_ema_update alone", lambda: ops.ema_update(st.ema, ar.data, 0.999, st.state)),
         ("two exchanges", two_swaps)]


def window(fn):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3          # us per call


times = {name: [] for name, _ in calls}
for r in range(rounds):
    for name, fn in calls:
        times[name].append(window(fn))
assert ema._swapped is False and bool(torch.isfinite(ar.data).all())

print("arena: %d floats (%.1f MB), %d steps per window, %d alternated rounds" % (ar.numel, nbytes / 1e6, steps, rounds))
res = {"arena_floats": ar.numel, "steps_per_window": steps, "rounds": rounds, "forms": {}}
for name, _ in calls:
    best, med = min(times[name]), statistics.median(times[name])
    res["forms"][name] = {"best_us": round(best, 2), "median_us": round(med, 2), "max_us": round(max(times[name]), 2)}
    print("%-22s best %8.2f us  median %8.2f us  max %8.2f us" % (name, best, med, max(times[name])))
base, with_ema = res["forms"]["capturable"]["median_us"], res["forms"]["ema"]["median_us"]
res["ema_extra_us"] = round(with_ema - base, 2)
res["expected_extra_us_from_bytes"] = round(base * 12.0 / 28.0, 2)
print("ema: +%.2f us per step over the capturable update (medians), %.1f %% of it; 12/28 of the update would be %.2f us" %
      (with_ema - base, 100.0 * (with_ema - base) / base, base * 12.0 / 28.0))
t = res["forms"]["gdn_ema_update alone"]["median_us"] * 1e-6
res["ema_update_bytes_per_s"] = 3 * nbytes / t
print("gdn_ema_update: %.1f MB moved in %.2f us = %.2f TB/s" % (3 * nbytes / 1e6, t * 1e6, 3 * nbytes / t / 1e12))
t = res["forms"]["two exchanges"]["median_us"] * 1e-6 / 2
res["swap_bytes_per_s"] = 4 * nbytes / t
print("gdn_swap_f32: %.1f MB moved in %.2f us per exchange = %.2f TB/s (host work of swap_averaged() included)" %
      (4 * nbytes / 1e6, t * 1e6, 4 * nbytes / t / 1e12))
line = json.dumps(res)
print(line)
if out:
    pathlib.Path(out).write_text(line + "\n")
