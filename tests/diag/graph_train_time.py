#!/usr/bin/env python3
"""GPU box: what --graph does to a training run's throughput and to the host time of a step.  A diagnostic,
not a test; run it under a `timeout` of its own.

Drives the training loops themselves (trainer.train_AE_DtoD / train_AE_RtoD) on a SyntheticLoader at the benchmark workload,
B = 20 at 128x416, for DtoD fp32, DtoD bf16 and RtoD bf16 (random frozen guide), each as
    eager     the loop without the flag                        (capturable Adam, like the graph run)
    graph     the loop with --graph, graph_warmup 3
    parent    the eager loop of another trainer.py (--parent-trainer FILE: the parent commit's), same optimizer
The variants of one configuration are alternated, `--reps` rounds each.  One call of the loop is one window: the first `skip`
batches (warm-up, capture) are not timed; the loader synchronises when the loop asks for batch `skip` and again when it
asks for batch `skip + timed`, and the time between the two is the window.
Reported per variant: images/s (median, min, max over the rounds), the host time per step -- wall time from the moment the
loop takes a batch to the moment it asks for the next one, i.e. the step call plus the loop's own counters, no sync in
between -- and the calls into the HIP library one step makes (counted at the C ABI: each is one or more kernel launches;
torch's own kernels are not in it), against the graph launches and input copies of a replayed step.
Clock state: the shader clock held under load (ops.ShaderClock around eager forwards) before and after every
configuration; a window is not bracketed by the clock probe itself, whose sleeping wave would share a hardware queue with
the branches of a replayed graph.

--world2: the same for DtoD bf16 with two ranks on ONE GPU under gloo (fresh child processes).  That exercises the host
path of graph.GraphedDataParallelStep -- two graphs around an eager all-reduce that travels through host memory -- and is
NOT a scaling number: both ranks share the GPU and gloo is not the deployment's transport.

usage: graph_train_time.py [--timed 36] [--skip 8] [--reps 3] [--parent-trainer FILE] [--world2] [--out FILE]"""
import argparse
import importlib.util
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "gdn-pytorch_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--timed", type=int, default=36)
ap.add_argument("--skip", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--batch", type=int, default=20)
ap.add_argument("--height", type=int, default=128)
ap.add_argument("--width", type=int, default=416)
ap.add_argument("--parent-trainer", default=None)
ap.add_argument("--world2", action="store_true")
ap.add_argument("--child", action="store_true", help="(internal) one rank of --world2")
ap.add_argument("--out", default=None)
opt = ap.parse_args()
assert opt.skip >= 5 and opt.skip + opt.timed + 1 < 50, "the loops print (and sync) every 50 steps: keep a call below that"

if opt.world2 and not opt.child:
    # the parent never touches the GPU: one fresh child per rank, both on device 0, gloo
    from gdn_amd import distributed as D
    argv = [a for a in sys.argv[1:]] + ["--child"]
    rc, text = D.launch_ranks(argv, [None, None], script=str(pathlib.Path(__file__).resolve()), timeout=900, capture_rank0=True,
                              extra_env={"GDN_DIST_BACKEND": "gloo", "GDN_SINGLE_DEVICE": "1", "LOCAL_RANK": "0"})
    sys.stdout.write(text)
    sys.exit(rc)

import torch
import gdn_amd.AE_model_unet as M
from gdn_amd import _lib
from gdn_amd import distributed as D
from gdn_amd import ops
from gdn_amd import trainer as T
from gdn_amd.optim import Adam
from gdn_amd.synthetic import synthetic_batch

rank, _, world = D.init() if opt.child else (0, 0, 1)
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
B, H, W = opt.batch, opt.height, opt.width
TOTAL = opt.skip + opt.timed + 1

trainers = {"eager": T, "graph": T}
if opt.parent_trainer and not opt.child:
    spec = importlib.util.spec_from_file_location("gdn_amd.trainer_parent", opt.parent_trainer)
    parent = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = parent
    spec.loader.exec_module(parent)
    trainers["parent"] = parent
for mod in set(trainers.values()):
    mod._save_checkpoint = lambda *a, **k: None          # the windows end before it; no 100 MB files per call


class TimedLoader:
    """TOTAL identical-shape resident batches; times the window described above."""

    def __init__(self):
        self.batches = [synthetic_batch(B, H, W, 5 + i + 100 * rank, dev) for i in range(4)]
        self.window_s = self.host_s = None

    def __len__(self):
        return TOTAL

    def __iter__(self):
        host, t_out = 0.0, None
        for i in range(TOTAL):
            now = time.perf_counter()
            if t_out is not None and i > opt.skip:
                host += now - t_out                       # the loop body that followed batch i - 1
            if i == opt.skip:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            if i == opt.skip + opt.timed:
                torch.cuda.synchronize()
                self.window_s, self.host_s = time.perf_counter() - t0, host
            t_out = time.perf_counter()
            yield self.batches[i % len(self.batches)]


def count_library_calls(fn):
    """Calls into the C ABI (status-returning entry points: the ones that launch) while fn() runs."""
    n = [0]
    saved = {}
    for name in _lib._STATUS_FUNCS - {"gdn_conv_out_dims", "gdn_fftconv_cgemm_shape"}:      # (these two launch nothing)
        f = getattr(_lib.lib, name)
        saved[name] = f

        def counted(*a, _f=f):
            n[0] += 1
            return _f(*a)
        setattr(_lib.lib, name, counted)
    try:
        fn()
    finally:
        for name, f in saved.items():
            setattr(_lib.lib, name, f)
    return n[0]


def clock_ghz(model, x):
    clk = ops.ShaderClock(dev, max_s=5.0)
    with torch.no_grad():
        for _ in range(3):
            model(x, istrain=False)
        torch.cuda.synchronize()
        with clk:
            for _ in range(10):
                model(x, istrain=False)
    torch.cuda.synchronize()
    g = clk.ghz()
    return None if g is None else round(g, 3)


class Variant:
    def __init__(self, name, mode, dtype):
        self.name, self.mode, self.mod = name, mode, trainers[name]
        torch.manual_seed(0)
        if mode == "DtoD":
            self.net, self.guide = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W).to(dev).compute_dtype(dtype), None
        else:
            self.net = M.AutoEncoder_2(input_dim=3, height=H, width=W).to(dev).compute_dtype(dtype)
            self.guide = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W).to(dev).compute_dtype(dtype).eval()
        D.broadcast_parameters(self.net)
        self.opt = Adam(self.net.parameters(), 2e-5, [0.9, 0.999], eps=1e-08, weight_decay=5e-4, capturable=True)
        self.args = argparse.Namespace(dataset="KITTI", epoch_size=0, batch_size=B, mode=mode, print_freq=10,
                                       graph=name == "graph", graph_warmup=3)
        self.loader = TimedLoader()
        self.ips, self.host_ms, self.report = [], [], None

    def window(self):
        if self.mode == "DtoD":
            self.mod.train_AE_DtoD(self.args, self.net, None, None, self.opt, self.loader, None, B, 1, 2e-5, None, None)
        else:
            self.mod.train_AE_RtoD(self.args, self.net, self.guide, None, None, self.opt, self.loader, None, B, 1, 2e-5, None, None)
        torch.cuda.synchronize()
        self.ips.append(B * world * opt.timed / self.loader.window_s)
        self.host_ms.append(self.loader.host_s / opt.timed * 1e3)
        if self.name == "graph":
            self.report = dict(T.last_graph_report)

    def calls_per_eager_step(self):
        gt, rgb, sp = self.loader.batches[0]
        loader = [(gt, rgb, sp)]
        args = argparse.Namespace(**dict(vars(self.args), graph=False))

        def one():
            if self.mode == "DtoD":
                T.train_AE_DtoD(args, self.net, None, None, self.opt, loader, None, B, 1, 2e-5, None, None)
            else:
                T.train_AE_RtoD(args, self.net, self.guide, None, None, self.opt, loader, None, B, 1, 2e-5, None, None)
        return count_library_calls(one)


configs = [("DtoD", "bf16")] if opt.child else [("DtoD", "fp32"), ("DtoD", "bf16"), ("RtoD", "bf16")]
res = {"batch": B, "height": H, "width": W, "world": world, "backend": str(torch.distributed.get_backend()) if opt.child else None,
       "timed_steps": opt.timed, "skipped_steps": opt.skip, "reps": opt.reps, "device": torch.cuda.get_device_name(0),
       "configs": []}
for mode, dtype in configs:
    names = [n for n in ("eager", "graph", "parent") if n in trainers]
    vs = [Variant(n, mode, dtype) for n in names]
    x = vs[0].loader.batches[0][1 if mode == "RtoD" else 0]
    clocks = [clock_ghz(vs[0].net, x)]
    for r in range(opt.reps):
        for v in (vs if r % 2 == 0 else vs[::-1]):          # alternated, order swapped every round
            v.window()
    clocks.append(clock_ghz(vs[0].net, x))
    calls = vs[0].calls_per_eager_step()
    rec = {"mode": mode, "dtype": dtype, "shader_clock_ghz_before_after": clocks, "library_calls_per_eager_step": calls,
           "variants": {}}
    for v in vs:
        rec["variants"][v.name] = {
            "images_per_s": {"median": round(statistics.median(v.ips), 1), "min": round(min(v.ips), 1), "max": round(max(v.ips), 1)},
            "host_ms_per_step": {"median": round(statistics.median(v.host_ms), 3), "min": round(min(v.host_ms), 3),
                                 "max": round(max(v.host_ms), 3)},
            "ms_per_step_median": round(B * world / statistics.median(v.ips) * 1e3, 2)}
        if v.report is not None:
            rec["variants"][v.name]["last_window"] = v.report
            rec["variants"][v.name]["launches_per_replayed_step"] = \
                "%d graph launch(es) + %d input copies" % (2 if world > 1 else 1, 3 if mode == "RtoD" else 2)
    res["configs"].append(rec)
    if rank == 0:
        print("%s %s, world %d: shader clock %s GHz before / after; %d library calls per eager step" %
              (mode, dtype, world, clocks, calls))
        for n, d in rec["variants"].items():
            print("  %-7s %8.1f img/s (min %.1f, max %.1f)   host %7.3f ms/step (min %.3f, max %.3f)   %.2f ms/step" %
                  (n, d["images_per_s"]["median"], d["images_per_s"]["min"], d["images_per_s"]["max"],
                   d["host_ms_per_step"]["median"], d["host_ms_per_step"]["min"], d["host_ms_per_step"]["max"],
                   d["ms_per_step_median"]))
        sys.stdout.flush()
    del vs
    torch.cuda.empty_cache()
if rank == 0:
    line = json.dumps(res)
    print(line)
    if opt.out:
        pathlib.Path(opt.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(opt.out).write_text(line + "\n")
if opt.child:
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
