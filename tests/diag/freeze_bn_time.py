#!/usr/bin/env python3
"""GPU box: what --freeze_bn does to a training step.  AutoEncoder_DtoD, B = 20, 128 x 416, fp32 and bf16.

Two models with the same weights and calibrated running statistics, alternated in one process over `rounds` rounds, each
window timed with device events after a warm-up:
    batch-stat   model.train()                   statistics in the conv epilogue + finalize, three-pass BatchNorm backward
    frozen       model.freeze_bn().train()       no statistics, one-pass gdn_bn_frozen_bwd + finalize
A step is forward, DtoD loss, backward and the fused Adam update.  Also printed: the calls into the C ABI one step makes
(each is one or more kernel launches; torch's own kernels are not in it), by entry point for the BatchNorm family.

The flag-off loop against another build (the parent commit): run this script in both trees with --only batch-stat and compare
the medians with the rounds' spread.  The BatchNorm share of a step from a kernel breakdown:
    rocprofv3 --kernel-trace --stats -d OUT -- python tests/diag/freeze_bn_time.py 20 1 --dtype fp32 --only frozen
and sum the bn_* kernels of OUT's kernel statistics (bn_bwd_sums_kernel<NH, true>, bn_bwd_finalize_kernel, bn_apply*; for the
other form bn_bwd_sums_kernel<1, false>, bn_bwd_apply_kernel<NH>, bn_finalize_train).

usage: freeze_bn_time.py [steps per window = 30] [rounds = 3] [--dtype fp32|bf16|both] [--only batch-stat|frozen] [--batch 20]
                         [--out FILE]"""
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "gdn-pytorch_amd")); sys.path.insert(0, str(ROOT / "tests"))
import torch
import gdn_amd.AE_model_unet as M
from libcalls import count_library_calls
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
only = opt_arg("--only", None)
B = int(opt_arg("--batch", "20"))
argv = sys.argv[1:]
steps = max(5, int(argv[0])) if argv else 30
rounds = int(argv[1]) if len(argv) > 1 else 3
H, W = 128, 416
dev = torch.device("cuda:0")
FORMS = [f for f in ("batch-stat", "frozen") if only in (None, f)]
BN_CALLS = ("gdn_bn_finalize_train", "gdn_bn_apply", "gdn_bn_apply_up2x", "gdn_bn_bwd", "gdn_bn_bwd_coeffs", "gdn_bn_eval_coeffs",
            "gdn_bn_eval_bwd", "gdn_bn_frozen_coeffs", "gdn_bn_frozen_bwd")


def build(dtype, frozen, sd):
    m = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
    m.load_state_dict(sd)
    m = m.to(dev).compute_dtype(dtype)
    if frozen:
        m.freeze_bn()               # (a tree without the feature has no such method: run it with --only batch-stat)
    return m.train()


def window(step, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


res = {"batch": B, "height": H, "width": W, "steps_per_window": steps, "rounds": rounds, "dtypes": {}}
for dtype in (("fp32", "bf16") if dtypes == "both" else (dtypes,)):
    torch.manual_seed(0)
    base = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
    loader = SyntheticLoader(B, 4, H, W, seed=0, device=dev)
    batches = [b for b in loader]
    # calibrate: a few train-mode steps' worth of statistics at momentum 1 on the first batch, so that the frozen form
    # normalises by sensible numbers (a fresh network's are mean 0 / variance 1)
    cal = build(dtype, False, base.state_dict())
    for n in cal.modules():
        if isinstance(n, torch.nn.BatchNorm2d):
            n.momentum = 1.0
    with torch.no_grad():
        cal(batches[0][0], istrain=False)
    sd = {k: v.detach().cpu().clone() for k, v in cal.state_dict().items()}
    del cal
    runs = {}
    for form in FORMS:
        model = build(dtype, form == "frozen", sd)
        opt = Adam(model.parameters(), 2e-5, [0.9, 0.999], eps=1e-08, weight_decay=5e-4)
        it = [0]

        def step(model=model, opt=opt, it=it):
            depth, _, sparse = batches[it[0] % len(batches)][:3]
            it[0] += 1
            opt.zero_grad()
            o = model(depth, istrain=False)
            loss, _, _ = U.dtod_loss(o, depth, sparse)
            loss.backward()
            opt.step()
        runs[form] = step
        window(step, 5)                                   # warm-up: workspaces, plans
    times = {f: [] for f in FORMS}
    for r in range(rounds):
        for f in FORMS:
            times[f].append(window(runs[f], steps))
    rec = {}
    for f in FORMS:
        calls, _ = count_library_calls(runs[f])
        torch.cuda.synchronize()
        rec[f] = {"median_ms": round(statistics.median(times[f]), 3), "min_ms": round(min(times[f]), 3),
                  "max_ms": round(max(times[f]), 3), "library_calls_per_step": sum(calls.values()),
                  "bn_calls": {k: calls[k] for k in BN_CALLS if calls[k]}}
        print("%-5s %-10s median %8.3f ms  (%.3f .. %.3f over %d rounds)  %d library calls per step, BatchNorm family: %s" % (
            dtype, f, rec[f]["median_ms"], rec[f]["min_ms"], rec[f]["max_ms"], rounds, rec[f]["library_calls_per_step"],
            rec[f]["bn_calls"]))
    if len(FORMS) == 2:
        d = rec["frozen"]["median_ms"] - rec["batch-stat"]["median_ms"]
        rec["frozen_minus_batch_stat_ms"] = round(d, 3)
        print("%-5s frozen - batch-stat: %+.3f ms per step (%.1f %%)" % (dtype, d, 100.0 * d / rec["batch-stat"]["median_ms"]))
    res["dtypes"][dtype] = rec
line = json.dumps(res)
print(line)
if out:
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text(line + "\n")
