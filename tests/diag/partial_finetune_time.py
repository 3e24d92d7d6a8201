#!/usr/bin/env python3
"""GPU box: what --freeze encoder costs and saves.  AutoEncoder_DtoD, 128 x 416, fp32 and bf16.

(a) kernel time: gdn_adam_step_seg with one group and no skipped chunk against gdn_adam_step_dev_guarded over the DtoD
    arena (both stream 28 bytes per element; the map adds 1/64 byte), alternated over `rounds` rounds.
(b) step time at batch B: three forms of the same model, alternated in one process over `rounds` rounds, each window timed
    with device events after a warm-up:
        unfrozen        everything trains, Adam(model.parameters())                         the flag-off step
        frozen-parent   encoder frozen, Adam(..., segmented=False), engine._PRUNE_FROZEN off  what the parent commit does
        frozen          encoder frozen, Adam(..., segmented=True), pruning on                --freeze encoder
    with the calls into the C ABI one step makes and those of optimizer.step() alone.
(c) the flag-off step against another build: run bench.py in both trees and compare within the rounds' spread.
Multi-rank behaviour cannot be measured on one GPU.

usage: partial_finetune_time.py [steps per window = 30] [rounds = 3] [--dtype fp32|bf16|both] [--batch 20] [--out FILE]"""
import collections
import json
import pathlib
import statistics
import struct
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "gdn-pytorch_amd"))
import torch
import gdn_amd.AE_model_unet as M
from gdn_amd import _lib, ops
from gdn_amd import engine as E
from gdn_amd import utils as U
from gdn_amd.optim import Adam
from gdn_amd.synthetic import SyntheticLoader


def opt_arg(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


out = opt_arg("--out", None)
dtypes = opt_arg("--dtype", "both")
B = int(opt_arg("--batch", "20"))
argv = sys.argv[1:]
steps = max(5, int(argv[0])) if argv else 30
rounds = int(argv[1]) if len(argv) > 1 else 3
H, W = 128, 416
dev = torch.device("cuda:0")
FORMS = ("unfrozen", "frozen-parent", "frozen")
OPT_CALLS = ("gdn_adam_step", "gdn_adam_step_dev", "gdn_adam_step_dev_guarded", "gdn_grad_sumsq", "gdn_grad_guard_finalize",
             "gdn_ema_update", "gdn_adam_step_seg", "gdn_grad_sumsq_seg", "gdn_ema_update_seg")


def count_library_calls(fn):
    """Calls into the C ABI (status-returning entry points: the ones that launch) while fn() runs, by name."""
    n = collections.Counter()
    saved = {}
    for name in _lib._STATUS_FUNCS - {"gdn_conv_out_dims", "gdn_fftconv_cgemm_shape"}:      # (these two launch nothing)
        f = getattr(_lib.lib, name)
        saved[name] = f

        def counted(*a, _f=f, _n=name):
            n[_n] += 1
            return _f(*a)
        setattr(_lib.lib, name, counted)
    try:
        fn()
    finally:
        for name, f in saved.items():
            setattr(_lib.lib, name, f)
    return n


def window(step, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


res = {"batch": B, "height": H, "width": W, "steps_per_window": steps, "rounds": rounds, "dtypes": {}}

# ---- (a) the update kernel alone ------------------------------------------------------------------------------------------
torch.manual_seed(0)
base = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
n = sum((p.numel() + 63) // 64 * 64 for p in base.parameters())
p, g, m, v = (torch.randn(n, device=dev) * s for s in (1.0, 1e-2, 1e-3, 1e-3))
v.abs_()
hyper = torch.tensor([[2e-5, 0.9, 0.999, 1e-8, 5e-4, 1.0]], dtype=torch.float32, device=dev)


def state():
    return torch.frombuffer(bytearray(struct.pack("<ddiff", 1.0, 1.0, 0, 0.0, 0.0) + b"\0" * 4), dtype=torch.uint8).to(dev)


guard = torch.frombuffer(bytearray(struct.pack("<dffiiii", 0.0, 1.0, 1.0, 0, 1, 0, 0)), dtype=torch.uint8).to(dev)
cmap = torch.zeros(n // 64, dtype=torch.uint8, device=dev)
s_seg, s_dev = state(), state()
kern = {"adam_step_seg": lambda: ops.adam_step_seg(p, g, m, v, cmap, hyper, s_seg, guard),
        "adam_step_dev_guarded": lambda: ops.adam_step_dev_guarded(p, g, m, v, hyper[0], s_dev, guard)}
for f in kern.values():
    window(f, 20)
kt = {k: [] for k in kern}
for r in range(rounds):
    for k, f in kern.items():
        kt[k].append(window(f, 200) * 1e3)           # microseconds per call (prep launch + update launch)
res["kernel_us"] = {k: spread(x) for k, x in kt.items()}
res["kernel_us"]["elements"] = n
d = res["kernel_us"]["adam_step_seg"]["median"] / res["kernel_us"]["adam_step_dev_guarded"]["median"] - 1.0
res["kernel_us"]["seg_over_dev_guarded_percent"] = round(100.0 * d, 2)
print("kernel: %d floats, adam_step_seg %s us, adam_step_dev_guarded %s us: %+.2f %%" % (
    n, res["kernel_us"]["adam_step_seg"], res["kernel_us"]["adam_step_dev_guarded"], 100.0 * d))
del p, g, m, v

# ---- (b) the training step ------------------------------------------------------------------------------------------------
for dtype in (("fp32", "bf16") if dtypes == "both" else (dtypes,)):
    loader = SyntheticLoader(B, 4, H, W, seed=0, device=dev)
    batches = [b for b in loader]
    runs, opts = {}, {}
    for form in FORMS:
        model = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
        model.load_state_dict(base.state_dict())
        model = model.to(dev).compute_dtype(dtype).train()
        if form != "unfrozen":
            model.freeze("encoder")
        opt = Adam(model.parameters(), 2e-5, [0.9, 0.999], eps=1e-08, weight_decay=5e-4, segmented=form == "frozen")
        it = [0]

        def step(model=model, opt=opt, it=it, prune=form != "frozen-parent"):
            E._PRUNE_FROZEN = prune
            depth, _, sparse = batches[it[0] % len(batches)][:3]
            it[0] += 1
            opt.zero_grad()
            o = model(depth, istrain=False)
            loss, _, _ = U.dtod_loss(o, depth, sparse)
            loss.backward()
            opt.step()
            E._PRUNE_FROZEN = True
        runs[form], opts[form] = step, opt
        window(step, 5)                                   # warm-up: workspaces, plans
    times = {f: [] for f in FORMS}
    for r in range(rounds):
        for f in FORMS:
            times[f].append(window(runs[f], steps))
    rec = {}
    for f in FORMS:
        calls = count_library_calls(runs[f])
        torch.cuda.synchronize()
        rec[f] = {"ms": spread(times[f]), "library_calls_per_step": sum(calls.values()),
                  "optimizer_calls_per_step": sum(calls[k] for k in OPT_CALLS)}
        print("%-5s %-14s median %8.3f ms  (%.3f .. %.3f over %d rounds)  %d library calls per step, %d of them the optimizer's" % (
            dtype, f, rec[f]["ms"]["median"], rec[f]["ms"]["min"], rec[f]["ms"]["max"], rounds, rec[f]["library_calls_per_step"],
            rec[f]["optimizer_calls_per_step"]))
    res["dtypes"][dtype] = rec
line = json.dumps(res)
print(line)
if out:
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text(line + "\n")
