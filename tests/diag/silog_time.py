#!/usr/bin/env python3
"""GPU box: what the scale-invariant log loss costs against the masked BerHu.  AutoEncoder_DtoD, 128 x 416, fp32 and bf16.

(a) the loss alone at [B,1,128,416]: gdn_silog_masked (three launches; float64 log per pixel in two of them) dense and with
    the LiDAR mask, against gdn_berhu_masked (four launches, float32), microseconds per call in a window of 200, back to back
    on one stream, forms alternated over `rounds` rounds.
(b) step time at batch B: the same model stepped with pixel = None (BerHu), the dense SILog spec and the LiDAR one,
    alternated in one process over `rounds` rounds, each window timed with device events after a warm-up, with the calls
    into the C ABI one step makes.
(c) the flag-off step against another build: `--tree DIR --forms berhu` times form `berhu` with DIR's package and library (a
    checkout of the parent commit, built); run the two trees alternately, and bench.py in both, and compare within the
    rounds' spread.
Multi-rank behaviour cannot be measured on one GPU.

usage: silog_time.py [steps per window = 30] [rounds = 3] [--dtype fp32|bf16|both] [--batch 20] [--forms a,b,...]
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
from gdn_amd import _lib, ops
from gdn_amd import utils as U
from gdn_amd.optim import Adam
from gdn_amd.synthetic import SyntheticLoader

out = opt_arg("--out", None)
dtypes = opt_arg("--dtype", "both")
B = int(opt_arg("--batch", "20"))
FORMS = tuple(opt_arg("--forms", "berhu,silog,silog-lidar").split(","))
argv = sys.argv[1:]
steps = max(5, int(argv[0])) if argv else 30
rounds = int(argv[1]) if len(argv) > 1 else 3
H, W = 128, 416
LR = 2e-5
dev = torch.device("cuda:0")
HAVE_SILOG = hasattr(U, "silog_spec")            # (a parent-commit tree has only the BerHu form)


def spec_of(form):
    return {"berhu": None, "silog": U.silog_spec() if HAVE_SILOG else None,
            "silog-lidar": U.silog_spec(use_sparse=True) if HAVE_SILOG else None}[form]


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
loader = SyntheticLoader(B, 4, H, W, seed=0, device=dev)
batches = [b for b in loader]

# ---- (a) the loss alone ---------------------------------------------------------------------------------------------------
if HAVE_SILOG and "silog" in FORMS:
    depth, _, sparse = batches[0][:3]
    pred = batches[1 % len(batches)][0].roll(1, 0).contiguous()
    dout, loss = torch.zeros_like(pred), torch.zeros((), device=dev)
    box = U.crop_box_kitti(H, W)
    calls = {"berhu": lambda: ops.berhu_masked(pred, depth, sparse, box, dout, loss),
             "berhu-dense": lambda: ops.berhu_masked(pred, depth, None, None, dout, loss),
             "silog": lambda: ops.silog_masked(pred, depth, None, None, dout, loss, 0.85, 10.0, 0.0125),
             "silog-lidar": lambda: ops.silog_masked(pred, depth, sparse, box, dout, loss, 0.85, 10.0, 0.0125),
             "silog-value-only": lambda: ops.silog_masked(pred, depth, None, None, None, loss, 0.85, 10.0, 0.0125)}
    for c in calls.values():
        window(c, 20)
    us = {k: [] for k in calls}
    for r in range(rounds):
        for k, c in calls.items():
            us[k].append(window(c, 200) * 1e3)
    res["loss_alone_us"] = {k: spread(v) for k, v in us.items()}
    for k, v in res["loss_alone_us"].items():
        print("loss alone %-17s %s us per call (back to back on one stream)" % (k, v))

# ---- (b) the training step ------------------------------------------------------------------------------------------------
torch.manual_seed(0)
base_model = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
for dtype in (("fp32", "bf16") if dtypes == "both" else (dtypes,)):
    runs = {}
    for form in FORMS:
        model = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
        model.load_state_dict(base_model.state_dict())
        model = model.to(dev).compute_dtype(dtype).train()
        opt = Adam(model.parameters(), LR, [0.9, 0.999], eps=1e-08, weight_decay=5e-4)
        it = [0]
        kw = {"pixel": spec_of(form)} if HAVE_SILOG else {}

        def step(model=model, opt=opt, it=it, kw=kw):
            depth, _, sparse = batches[it[0] % len(batches)][:3]
            opt.zero_grad()
            o = model(depth, istrain=False)
            loss, _, _ = U.dtod_loss(o, depth, sparse, **kw)
            U.backward(loss)
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
                  "silog_calls_per_step": calls["gdn_silog_masked"], "berhu_calls_per_step": calls["gdn_berhu_masked"]}
        print("%-5s %-12s median %8.3f ms  (%.3f .. %.3f over %d rounds)  %d library calls per step (silog %d, berhu %d)" % (
            dtype, f, rec[f]["ms"]["median"], rec[f]["ms"]["min"], rec[f]["ms"]["max"], rounds, rec[f]["library_calls_per_step"],
            rec[f]["silog_calls_per_step"], rec[f]["berhu_calls_per_step"]))
    res["dtypes"][dtype] = rec
line = json.dumps(res)
print(line)
if out:
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text(line + "\n")
