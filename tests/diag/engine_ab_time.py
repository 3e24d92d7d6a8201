#!/usr/bin/env python3
"""GPU box: eager training with this tree's gdn_amd/engine.py against another engine.py (--parent-engine FILE: the parent
commit's), same library build.  A diagnostic, not a test; run it under a `timeout` of its own.  A sibling of
graph_train_time.py, which compares trainers inside one process; an engine cannot be swapped there, every module holds it.

The training loops themselves (trainer.train_AE_DtoD / train_AE_RtoD) on resident synthetic batches at the benchmark workload,
B = 20 at 128x416, for DtoD fp32 and RtoD bf16 (random frozen guide).  Every variant and round is a FRESH CHILD PROCESS -- this
process never touches the GPU -- and the rounds alternate `new` and `parent`, the order swapped every round.  The parent child
registers FILE as gdn_amd.engine before anything else imports it.  One call of the loop is one window: the first `skip`
batches are not timed; the loader synchronises when the loop asks for batch `skip` and for batch `skip + timed`.
Reported per variant: images/s and the host time per step (wall time from the moment the loop takes a batch to the moment it
asks for the next one, no sync in between), as median, min and max over the rounds; then, per configuration, whether the new
medians are within the parent's own min-to-max spread of the parent's medians -- the noise this comparison cannot resolve.

--layer-timer: one more child per variant with a host-only timer around every engine.conv_bn_act call and around Ctx.backward
(the tape replay), as us per call / ms per step.  The timers cost time themselves: those children's throughput is not reported.

usage: engine_ab_time.py --parent-engine FILE [--rounds 3] [--timed 36] [--skip 8] [--layer-timer] [--out FILE]"""
import argparse
import importlib.util
import json
import pathlib
import statistics
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "gdn-pytorch_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--parent-engine", required=True)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--timed", type=int, default=36)
ap.add_argument("--skip", type=int, default=8)
ap.add_argument("--batch", type=int, default=20)
ap.add_argument("--layer-timer", action="store_true")
ap.add_argument("--child", default=None, help="(internal) new | parent: measure one round in this process")
ap.add_argument("--out", default=None)
opt = ap.parse_args()
assert opt.skip >= 5 and opt.skip + opt.timed + 1 < 50, "the loops print (and sync) every 50 steps: keep a call below that"
CONFIGS = [("DtoD", "fp32"), ("RtoD", "bf16")]
B, H, W = opt.batch, 128, 416
TOTAL = opt.skip + opt.timed + 1


def child():
    if opt.child == "parent":
        import gdn_amd
        spec = importlib.util.spec_from_file_location("gdn_amd.engine", opt.parent_engine)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        gdn_amd.engine = mod
    import torch
    import gdn_amd.AE_model_unet as M
    from gdn_amd import engine as E
    from gdn_amd import trainer as T
    from gdn_amd.optim import Adam
    from gdn_amd.synthetic import synthetic_batch
    assert (pathlib.Path(E.__file__).resolve() == pathlib.Path(opt.parent_engine).resolve()) == (opt.child == "parent")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    T._save_checkpoint = lambda *a, **k: None
    timers = {"fwd_calls": 0, "fwd_s": 0.0, "bwd_s": 0.0}
    if opt.layer_timer:
        real_cba, real_bwd = E.conv_bn_act, E.Ctx.backward

        def cba(*a, **k):
            t = time.perf_counter()
            try:
                return real_cba(*a, **k)
            finally:
                timers["fwd_s"] += time.perf_counter() - t
                timers["fwd_calls"] += 1

        def bwd(self):
            t = time.perf_counter()
            real_bwd(self)
            timers["bwd_s"] += time.perf_counter() - t
        E.conv_bn_act, E.Ctx.backward = cba, bwd

    class TimedLoader:
        def __init__(self):
            self.batches = [synthetic_batch(B, H, W, 5 + i, dev) for i in range(4)]

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
                    timers.update(fwd_calls=0, fwd_s=0.0, bwd_s=0.0)
                if i == opt.skip + opt.timed:
                    torch.cuda.synchronize()
                    self.window_s, self.host_s, self.timers = time.perf_counter() - t0, host, dict(timers)
                t_out = time.perf_counter()
                yield self.batches[i % len(self.batches)]

    res = {}
    for mode, dtype in CONFIGS:
        torch.manual_seed(0)
        guide = None
        if mode == "DtoD":
            net = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W).to(dev).compute_dtype(dtype)
        else:
            net = M.AutoEncoder_2(input_dim=3, height=H, width=W).to(dev).compute_dtype(dtype)
            guide = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W).to(dev).compute_dtype(dtype).eval()
        adam = Adam(net.parameters(), 2e-5, [0.9, 0.999], eps=1e-08, weight_decay=5e-4, capturable=True)
        args = argparse.Namespace(dataset="KITTI", epoch_size=0, batch_size=B, mode=mode, print_freq=10, graph=False, graph_warmup=3)
        loader = TimedLoader()
        if mode == "DtoD":
            T.train_AE_DtoD(args, net, None, None, adam, loader, None, B, 1, 2e-5, None, None)
        else:
            T.train_AE_RtoD(args, net, guide, None, None, adam, loader, None, B, 1, 2e-5, None, None)
        torch.cuda.synchronize()
        rec = {"images_per_s": B * opt.timed / loader.window_s, "host_ms_per_step": loader.host_s / opt.timed * 1e3}
        if opt.layer_timer:
            t = loader.timers
            rec = {"conv_bn_act_calls_per_step": t["fwd_calls"] / opt.timed, "conv_bn_act_us_per_call": t["fwd_s"] / max(t["fwd_calls"], 1) * 1e6,
                   "conv_bn_act_ms_per_step": t["fwd_s"] / opt.timed * 1e3, "tape_replay_ms_per_step": t["bwd_s"] / opt.timed * 1e3}
        res["%s %s" % (mode, dtype)] = rec
        del net, guide, adam, loader
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res))


def run_child(variant, extra=()):
    cmd = [sys.executable, str(pathlib.Path(__file__).resolve()), "--child", variant, "--parent-engine", opt.parent_engine,
           "--timed", str(opt.timed), "--skip", str(opt.skip), "--batch", str(opt.batch)] + list(extra)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.stdout.write(p.stdout)
        raise SystemExit("child %s failed (exit status %d): nothing more is started" % (variant, p.returncode))
    return json.loads(lines[-1][len("RESULT "):])


def main():
    rounds = {"new": [], "parent": []}
    for r in range(opt.rounds):
        for v in (("new", "parent") if r % 2 == 0 else ("parent", "new")):
            rounds[v].append(run_child(v))
            print("round %d %-6s %s" % (r, v, json.dumps(rounds[v][-1])))
            sys.stdout.flush()
    out = {"batch": B, "height": H, "width": W, "timed_steps": opt.timed, "skipped_steps": opt.skip, "rounds": opt.rounds, "configs": {}}
    for mode, dtype in CONFIGS:
        cfg = "%s %s" % (mode, dtype)
        rec = {}
        for v in ("new", "parent"):
            for k in ("images_per_s", "host_ms_per_step"):
                xs = [r[cfg][k] for r in rounds[v]]
                rec.setdefault(v, {})[k] = {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}
        p, n = rec["parent"], rec["new"]
        spread_ips = p["images_per_s"]["max"] - p["images_per_s"]["min"]
        spread_host = p["host_ms_per_step"]["max"] - p["host_ms_per_step"]["min"]
        rec["parent_spread"] = {"images_per_s": round(spread_ips, 3), "host_ms_per_step": round(spread_host, 3)}
        rec["within_parent_spread"] = {
            "images_per_s": n["images_per_s"]["median"] >= p["images_per_s"]["median"] - spread_ips,
            "host_ms_per_step": n["host_ms_per_step"]["median"] <= p["host_ms_per_step"]["median"] + spread_host}
        out["configs"][cfg] = rec
        print(cfg)
        for v in ("new", "parent"):
            print("  %-7s %8.1f img/s (min %.1f, max %.1f)   host %7.3f ms/step (min %.3f, max %.3f)" % (
                v, rec[v]["images_per_s"]["median"], rec[v]["images_per_s"]["min"], rec[v]["images_per_s"]["max"],
                rec[v]["host_ms_per_step"]["median"], rec[v]["host_ms_per_step"]["min"], rec[v]["host_ms_per_step"]["max"]))
        print("  parent's spread: %.1f img/s, %.3f ms host; new median within it: img/s %s, host %s" % (
            spread_ips, spread_host, rec["within_parent_spread"]["images_per_s"], rec["within_parent_spread"]["host_ms_per_step"]))
    if opt.layer_timer:
        out["layer_timer"] = {v: run_child(v, ["--layer-timer"]) for v in ("new", "parent")}
        for v, r in out["layer_timer"].items():
            for cfg, t in r.items():
                print("layer timer %-6s %-9s conv_bn_act %.1f calls/step, %.1f us/call, %.3f ms/step; tape replay %.3f ms/step" % (
                    v, cfg, t["conv_bn_act_calls_per_step"], t["conv_bn_act_us_per_call"], t["conv_bn_act_ms_per_step"],
                    t["tape_replay_ms_per_step"]))
    line = json.dumps(out)
    print(line)
    if opt.out:
        pathlib.Path(opt.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(opt.out).write_text(line + "\n")


if __name__ == "__main__":
    child() if opt.child else main()
