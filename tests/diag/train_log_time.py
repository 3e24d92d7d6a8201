#!/usr/bin/env python3
"""GPU box: what the training log costs.  AutoEncoder_DtoD, 128 x 416, fp32 and bf16.

(a) launch time: gdn_step_record back to back beside gdn_lr_schedule back to back, in the same run, microseconds per call in
    a window of 200 -- the yardstick for "one small launch".
(b) gdn_tensor_sumsq alone over the model's arena (weights and gradient: two arrays) beside gdn_grad_sumsq over the same arena
    (one array), both in GB/s of the bytes they read.
(c) step time at batch B: forms of the same model, alternated in one process over `rounds` rounds, each window timed with
    device events after a warm-up:
        off      Adam(model.parameters())                                  the flag-off step
        log      + TrainLog.record / note per step, the ring at 256 rows   --train_log
        norms    + TrainLog.tensor_norms every step                        --train_log --tensor_norms_every 1 (the worst case)
        item     off, then [t.item() for t in terms] every step            the host-side logger the ring replaces
    with the calls into the C ABI one step makes.
(d) the flag-off step against another build: `--tree DIR --forms off` times form `off` with DIR's package and library (a
    checkout of the parent commit, built); run the two trees alternately, and bench.py in both, and compare within the
    rounds' spread.
Multi-rank behaviour (rank 0's graph carrying one node more than the others') cannot be measured on one GPU.

usage: train_log_time.py [steps per window = 30] [rounds = 3] [--dtype fp32|bf16|both] [--batch 20] [--forms a,b,...]
                         [--tree DIR] [--out FILE]"""
import collections
import json
import pathlib
import statistics
import sys
import tempfile

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
FORMS = tuple(opt_arg("--forms", "off,log,norms,item").split(","))
argv = sys.argv[1:]
steps = max(5, int(argv[0])) if argv else 30
rounds = int(argv[1]) if len(argv) > 1 else 3
H, W = 128, 416
LR = 2e-5
dev = torch.device("cuda:0")
NEW = any(f != "off" for f in FORMS)            # (a tree without the training log times form `off` only)


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
tmp = pathlib.Path(tempfile.mkdtemp(prefix="train_log_time_"))

# ---- (a) the two small launches, alternated -----------------------------------------------------------------------------------
if NEW:
    hyper = torch.zeros(1, 6, device=dev)
    base = torch.full((1,), LR, dtype=torch.float64, device=dev)
    states = torch.frombuffer(bytearray(R.state_bytes(150)), dtype=torch.uint8).to(dev)
    guard = torch.zeros(32, dtype=torch.uint8, device=dev)
    ring = torch.zeros(64 * 257, dtype=torch.uint8, device=dev)
    terms = [t for t in torch.ones(3, device=dev)]
    calls = {"gdn_lr_schedule": lambda: ops.lr_schedule(hyper, base, states, "cosine", 100, 100000, 0.1),
             "gdn_step_record": lambda: ops.step_record(ring, 256, terms, hyper[0], states, guard)}
    times = {k: [] for k in calls}
    for c in calls.values():
        window(c, 20)
    for _ in range(rounds):
        for k, c in calls.items():
            times[k].append(window(c, 200) * 1e3)
    res["launch_us"] = {k: spread(v) for k, v in times.items()}
    for k, v in res["launch_us"].items():
        print("%-16s %s us per call (back to back on one stream)" % (k, v))

# ---- (b), (c): the model ------------------------------------------------------------------------------------------------------
torch.manual_seed(0)
base_model = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
for dtype in (("fp32", "bf16") if dtypes == "both" else (dtypes,)):
    loader = SyntheticLoader(B, 4, H, W, seed=0, device=dev)
    batches = [b for b in loader]
    runs, logs = {}, {}
    for form in FORMS:
        model = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
        model.load_state_dict(base_model.state_dict())
        model = model.to(dev).compute_dtype(dtype).train()
        opt = Adam(model.parameters(), LR, [0.9, 0.999], eps=1e-08, weight_decay=5e-4)
        log = None
        if form in ("log", "norms"):
            from gdn_amd.trainlog import TrainLog
            log = logs[form] = TrainLog(tmp / ("%s_%s.jsonl" % (dtype, form)), ["total_loss", "output_loss", "gradient_loss"], 256,
                                        dev, header={"form": form}, model=model)
        it = [0]

        def step(model=model, opt=opt, it=it, log=log, form=form):
            depth, _, sparse = batches[it[0] % len(batches)][:3]
            opt.zero_grad()
            o = model(depth, istrain=False)
            terms = U.dtod_loss(o, depth, sparse)
            terms[0].backward()
            opt.step()
            it[0] += 1
            if log is not None:
                log.record(terms, opt)
                log.note(0, it[0] - 1, it[0])
                if form == "norms":
                    log.tensor_norms(it[0], model._gdn_param_arena, 1.0)
            elif form == "item":
                [t.item() for t in terms]
        runs[form] = step
        window(step, 5)                                   # warm-up: workspaces, plans
    if NEW and "tensor_sumsq_gbs" not in res:
        # (b) the norms pass alone over this model's arena, beside the guard's norm pass over the same arena
        ar = model._gdn_param_arena
        seg = torch.tensor([[o, n] for _, o, n, _ in ar.items], dtype=torch.int64).to(dev)
        sums = torch.empty((seg.shape[0], 2), dtype=torch.float64, device=dev)
        live = sum(n for _, _, n, _ in ar.items)
        passes = {"gdn_tensor_sumsq": (lambda: ops.tensor_sumsq(ar.data, ar.grad, seg, sums), 8 * live),
                  "gdn_grad_sumsq": (lambda: ops.grad_sumsq(ar.grad, guard), 4 * ar.numel)}
        times = {k: [] for k in passes}
        for c, _ in passes.values():
            window(c, 10)
        for _ in range(rounds):
            for k, (c, _) in passes.items():
                times[k].append(window(c, 100))
        res["arena_floats"], res["arena_tensors"], res["tensor_sumsq_gbs"] = ar.numel, int(seg.shape[0]), {}
        for k, (_, nbytes) in passes.items():
            ms = spread(times[k])
            res["tensor_sumsq_gbs"][k] = {"ms": ms, "bytes": nbytes, "GB_per_s": round(nbytes / ms["median"] / 1e6, 1)}
            print("%-16s over %.1f M floats in %d tensors: %s ms, %.1f GB/s of the %d bytes it reads" % (
                k, ar.numel / 1e6, seg.shape[0], ms, res["tensor_sumsq_gbs"][k]["GB_per_s"], nbytes))
    times = {f: [] for f in FORMS}
    for r in range(rounds):
        for f in FORMS:
            times[f].append(window(runs[f], steps))
    rec = {}
    for f in FORMS:
        calls = count_library_calls(runs[f])
        torch.cuda.synchronize()
        rec[f] = {"ms": spread(times[f]), "rounds_ms": [round(t, 4) for t in times[f]], "library_calls_per_step": sum(calls.values()),
                  "step_record_calls_per_step": calls["gdn_step_record"], "tensor_sumsq_calls_per_step": calls["gdn_tensor_sumsq"]}
        print("%-5s %-6s median %8.3f ms  (%.3f .. %.3f over %d rounds)  %d library calls per step, %d gdn_step_record, %d "
              "gdn_tensor_sumsq" % (dtype, f, rec[f]["ms"]["median"], rec[f]["ms"]["min"], rec[f]["ms"]["max"], rounds,
                                    rec[f]["library_calls_per_step"], calls["gdn_step_record"], calls["gdn_tensor_sumsq"]))
    for log in logs.values():
        log.close()
    res["dtypes"][dtype] = rec
line = json.dumps(res)
print(line)
if out:
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text(line + "\n")
