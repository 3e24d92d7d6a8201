#!/usr/bin/env python3
"""GPU box: what the device-side learning-rate schedule costs.  AutoEncoder_DtoD, 128 x 416, fp32 and bf16.

(a) launch time: gdn_lr_schedule alone, G = 1 and G = 254, microseconds per call in a window of 200.
(b) step time at batch B: forms of the same model, alternated in one process over `rounds` rounds, each window timed with
    device events after a warm-up:
        off          Adam(model.parameters())                                     the flag-off step (host path)
        capturable   Adam(..., capturable=True)                                   the device tables, no schedule
        schedule     Adam(..., schedule=cosine, W = 100)                          --lr_schedule cosine --warmup_steps 100
        host-push    Adam(..., capturable=True), every step group['lr'] = lr * s(u); refresh_hyper()
                                                                                  the same schedule from the host: a blocking
                                                                                  copy from pageable memory per step
    with the calls into the C ABI one step makes.
(c) the flag-off step against another build: `--tree DIR --forms off` times form `off` with DIR's package and library (a
    checkout of the parent commit, built); run the two trees alternately, and bench.py in both, and compare within the
    rounds' spread.
Multi-rank behaviour cannot be measured on one GPU.

usage: lr_schedule_time.py [steps per window = 30] [rounds = 3] [--dtype fp32|bf16|both] [--batch 20] [--forms a,b,...]
                           [--tree DIR] [--out FILE]"""
import collections
import json
import pathlib
import statistics
import sys

HERE = pathlib.Path(__file__).resolve().parent


def opt_arg(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


ROOT = pathlib.Path(opt_arg("--tree", str(HERE.parent.parent))).resolve()
sys.path.insert(0, str(HERE.parent)); sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "gdn-pytorch_amd"))
import torch
import gdn_amd.AE_model_unet as M
import lr_schedule_fp64 as R
from gdn_amd import _lib, ops
from gdn_amd import utils as U
from gdn_amd.optim import Adam
from gdn_amd.synthetic import SyntheticLoader

out = opt_arg("--out", None)
dtypes = opt_arg("--dtype", "both")
B = int(opt_arg("--batch", "20"))
FORMS = tuple(opt_arg("--forms", "off,capturable,schedule,host-push").split(","))
argv = sys.argv[1:]
steps = max(5, int(argv[0])) if argv else 30
rounds = int(argv[1]) if len(argv) > 1 else 3
H, W = 128, 416
LR = 2e-5
SCHED = {"kind": "cosine", "warmup": 100, "total": 100000, "floor": 0.1}
dev = torch.device("cuda:0")


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


res = {"tree": str(ROOT), "batch": B, "height": H, "width": W, "steps_per_window": steps, "rounds": rounds, "forms": list(FORMS),
       "dtypes": {}}

# ---- (a) the launch alone -------------------------------------------------------------------------------------------------
if "schedule" in FORMS:
    res["launch_us"] = {}
    for G in (1, 254):
        hyper = torch.zeros(G, 6, device=dev)
        base = torch.full((G,), LR, dtype=torch.float64, device=dev)
        states = torch.frombuffer(bytearray(R.state_bytes(150) * G), dtype=torch.uint8).to(dev)
        call = lambda: ops.lr_schedule(hyper, base, states, "cosine", 100, 100000, 0.1)      # noqa: E731
        window(call, 20)
        res["launch_us"]["G=%d" % G] = spread([window(call, 200) * 1e3 for _ in range(rounds)])
        print("gdn_lr_schedule G = %3d: %s us per call (back to back on one stream)" % (G, res["launch_us"]["G=%d" % G]))

# ---- (b) the training step ------------------------------------------------------------------------------------------------
torch.manual_seed(0)
base_model = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
for dtype in (("fp32", "bf16") if dtypes == "both" else (dtypes,)):
    loader = SyntheticLoader(B, 4, H, W, seed=0, device=dev)
    batches = [b for b in loader]
    runs = {}
    for form in FORMS:
        model = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
        model.load_state_dict(base_model.state_dict())
        model = model.to(dev).compute_dtype(dtype).train()
        kw = {"off": {}, "capturable": {"capturable": True}, "schedule": {"schedule": SCHED}, "host-push": {"capturable": True}}[form]
        opt = Adam(model.parameters(), LR, [0.9, 0.999], eps=1e-08, weight_decay=5e-4, **kw)
        it = [0]

        def step(model=model, opt=opt, it=it, push=form == "host-push"):
            depth, _, sparse = batches[it[0] % len(batches)][:3]
            opt.zero_grad()
            o = model(depth, istrain=False)
            loss, _, _ = U.dtod_loss(o, depth, sparse)
            loss.backward()
            if push:
                for g in opt.param_groups:
                    g["lr"] = LR * R.s(it[0], SCHED["kind"], SCHED["warmup"], SCHED["total"], SCHED["floor"])
                opt.refresh_hyper()
            opt.step()
            it[0] += 1
        runs[form] = step
        window(step, 5)                                   # warm-up: workspaces, plans
    times = {f: [] for f in FORMS}
    for r in range(rounds):
        for f in FORMS:
            times[f].append(window(runs[f], steps))
    rec = {}
    for f in FORMS:
        calls = count_library_calls(runs[f])
        torch.cuda.synchronize()
        rec[f] = {"ms": spread(times[f]), "rounds_ms": [round(t, 4) for t in times[f]], "library_calls_per_step": sum(calls.values()),
                  "lr_schedule_calls_per_step": calls["gdn_lr_schedule"]}
        print("%-5s %-11s median %8.3f ms  (%.3f .. %.3f over %d rounds)  %d library calls per step, %d of them gdn_lr_schedule" % (
            dtype, f, rec[f]["ms"]["median"], rec[f]["ms"]["min"], rec[f]["ms"]["max"], rounds, rec[f]["library_calls_per_step"],
            rec[f]["lr_schedule_calls_per_step"]))
    res["dtypes"][dtype] = rec
line = json.dumps(res)
print(line)
if out:
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text(line + "\n")
