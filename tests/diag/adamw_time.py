#!/usr/bin/env python3
"""GPU box: what decoupled weight decay costs.  AutoEncoder_DtoD, 128 x 416, fp32 and bf16.

(a) the update alone on an arena of the full model's size (72.2 M floats; p, g, m, v: 1.16 GB read, 0.87 GB written): the
    decoupled entry point against its coupled sibling, gdn_adam[w]_step_dev_guarded and gdn_adam[w]_step_seg (three groups and a
    skipped tail, the map of a fine-tuning run), forms alternated over `rounds` rounds, each window timed with device events
    after a warm-up.  The kernels move the same bytes: the decoupled one should land inside the spread of the coupled one's
    own rounds.
(b) step time at batch B: the same model under Adam(weight_decay=5e-4) and Adam(weight_decay=1e-2, decoupled=True), alternated
    in one process over `rounds` rounds, with the calls into the C ABI one step makes (which must be equal).
Multi-rank behaviour cannot be measured on one GPU.

usage: adamw_time.py [steps per window = 30] [rounds = 3] [--dtype fp32|bf16|both|none] [--batch 20] [--floats 72200000]
                     [--out FILE]"""
import collections
import json
import pathlib
import statistics
import struct
import sys

HERE = pathlib.Path(__file__).resolve().parent


def opt_arg(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


ROOT = HERE.parent.parent
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
N = int(opt_arg("--floats", "72200000")) // 64 * 64
argv = sys.argv[1:]
steps = max(5, int(argv[0])) if argv else 30
rounds = int(argv[1]) if len(argv) > 1 else 3
H, W = 128, 416
LR = 2e-5
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


res = {"batch": B, "height": H, "width": W, "steps_per_window": steps, "rounds": rounds, "arena_floats": N, "update_ms": {},
       "dtypes": {}}

# ---- (a) the update alone -------------------------------------------------------------------------------------------------
gen = torch.Generator(device=dev).manual_seed(0)
p = torch.randn(N, device=dev, generator=gen)
g = torch.randn(N, device=dev, generator=gen) * 1e-2
m = torch.zeros(N, device=dev)
v = torch.zeros(N, device=dev)
rows = [(LR, 0.9, 0.999, 1e-8, 1e-2, 1.0), (LR * 0.1, 0.9, 0.999, 1e-8, 1e-2, 1.0), (LR, 0.9, 0.999, 1e-8, 0.0, 1.0)]
hyper = torch.tensor(rows, dtype=torch.float32, device=dev)
state = lambda: torch.frombuffer(bytearray(struct.pack("<ddiff", 1.0, 1.0, 0, 0.0, 0.0) + b"\0" * 4), dtype=torch.uint8)      # noqa: E731
guard = torch.frombuffer(bytearray(struct.pack("<dffiiii", 0.0, 1.0, 1.0, 0, 1, 0, 0)), dtype=torch.uint8).to(dev)
chunks = N // 64
cmap = torch.full((chunks,), 0xFF, dtype=torch.uint8)
cmap[:chunks // 2] = 0
cmap[chunks // 2:chunks * 9 // 10] = 1
cmap[chunks * 9 // 10:chunks * 99 // 100] = 2                                  # (the last hundredth is skipped)
cmap = cmap.to(dev)
forms = {}
for name, fn in (("adam_step_dev_guarded", ops.adam_step_dev_guarded), ("adamw_step_dev_guarded", ops.adamw_step_dev_guarded)):
    st = state().to(dev)
    forms[name] = lambda fn=fn, st=st: fn(p, g, m, v, hyper[0], st, guard)
for name, fn in (("adam_step_seg", ops.adam_step_seg), ("adamw_step_seg", ops.adamw_step_seg)):
    st = torch.cat([state() for _ in rows]).to(dev)
    forms[name] = lambda fn=fn, st=st: fn(p, g, m, v, cmap, hyper, st, guard)
for f in forms.values():
    window(f, 3)
times = {f: [] for f in forms}
for r in range(rounds):
    for f in forms:
        times[f].append(window(forms[f], steps))
for f in forms:
    res["update_ms"][f] = dict(spread(times[f]), rounds_ms=[round(t, 4) for t in times[f]])
    gb = N * 4 * (7 if "dev" in f else 7 * 0.99) / 1e9
    print("%-24s median %7.4f ms  (%.4f .. %.4f over %d rounds)  %.0f GB/s" % (
        f, res["update_ms"][f]["median"], res["update_ms"][f]["min"], res["update_ms"][f]["max"], rounds,
        gb / (res["update_ms"][f]["median"] * 1e-3)))
del p, g, m, v

# ---- (b) the training step ------------------------------------------------------------------------------------------------
torch.manual_seed(0)
base_model = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
FORMS = {"adam": dict(weight_decay=5e-4), "adamw": dict(weight_decay=1e-2, decoupled=True)}
for dtype in {"both": ("fp32", "bf16"), "none": ()}.get(dtypes, (dtypes,)):
    loader = SyntheticLoader(B, 4, H, W, seed=0, device=dev)
    batches = [b for b in loader]
    runs = {}
    for form, kw in FORMS.items():
        model = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
        model.load_state_dict(base_model.state_dict())
        model = model.to(dev).compute_dtype(dtype).train()
        opt = Adam(model.parameters(), LR, [0.9, 0.999], eps=1e-08, **kw)
        it = [0]

        def step(model=model, opt=opt, it=it):
            depth, _, sparse = batches[it[0] % len(batches)][:3]
            opt.zero_grad()
            o = model(depth, istrain=False)
            loss, _, _ = U.dtod_loss(o, depth, sparse)
            loss.backward()
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
                  "update_calls_per_step": {k: n for k, n in calls.items() if "adam" in k}}
        print("%-5s %-6s median %8.3f ms  (%.3f .. %.3f over %d rounds)  %d library calls per step, the update: %s" % (
            dtype, f, rec[f]["ms"]["median"], rec[f]["ms"]["min"], rec[f]["ms"]["max"], rounds, rec[f]["library_calls_per_step"],
            rec[f]["update_calls_per_step"]))
    res["dtypes"][dtype] = rec
line = json.dumps(res)
print(line)
if out:
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text(line + "\n")
