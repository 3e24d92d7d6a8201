#!/usr/bin/env python3
"""GPU box: the bf16 LDS-DMA ring kernels (conv_ring_bf16 / conv_ring2_bf16) of this tree's libgdn_hip.so against another build
of the library (--parent-lib PATH: the parent commit's), selected with GDN_HIP_LIB.  A diagnostic, not a test; run it under a
`timeout` of its own.  A sibling of engine_ab_time.py, which swaps the engine instead of the library.

Every variant and round is a FRESH CHILD PROCESS under its own `timeout` -- this process never touches the GPU -- and the rounds
alternate `new` and `parent`, the order swapped every round; the first child that fails stops the run.  Timed per round:
  * the per-layer shapes of ring2_check.py at B = 20, on tile ids 10 / 11 / 12 where the layer is eligible: forward with the
    BatchNorm partials, data gradient with a residual, and (ids 10 and 12) the data gradient with the BatchNorm-backward partials;
    ms per launch over `--reps` launches between two events;
  * one RtoD bf16 training throughput figure: bench.py --mode RtoD --dtype bf16 (images/s).
Reported per item: median, min and max over the rounds of either variant, and whether the new median lies within the parent's
own min-to-max spread -- or, where that spread is under 0.5 % of the parent's median, no more than 0.5 % on the slow side of it.

usage: ring_ab_time.py --parent-lib PATH [--rounds 3] [--reps 20] [--steps 20] [--warmup 5] [--out FILE]"""
import argparse
import json
import os
import pathlib
import statistics
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "gdn-pytorch_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=20)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--child", default=None, help="(internal) new | parent: time the layers once in this process")
ap.add_argument("--out", default=None)
opt = ap.parse_args()
assert opt.rounds >= 3, "a median and a spread need three rounds"
NEW_LIB = ROOT / "gdn-pytorch_amd" / "lib" / "libgdn_hip.so"
L = [(128, 416), (64, 208), (32, 104), (16, 52)]
SHAPES = [("res64 k9", 64, 64, 9, 4, False, *L[0]), ("res128 k7", 128, 128, 7, 3, False, *L[1]), ("res256 k5", 256, 256, 5, 2, False, *L[2]),
          ("res512 k3 l3", 512, 512, 3, 1, False, *L[3]), ("R up3 k7 refl", 128, 64, 7, 3, True, *L[0]), ("R up2 k5 refl", 256, 128, 5, 2, True, *L[1])]


def child():
    import torch
    from gdn_amd import _lib, ops
    want = pathlib.Path(opt.parent_lib) if opt.child == "parent" else NEW_LIB
    assert pathlib.Path(_lib.LIB_PATH).resolve() == want.resolve(), "child %s loaded %s" % (opt.child, _lib.LIB_PATH)
    dev = torch.device("cuda:0")
    B = opt.batch

    def timeit(fn):
        fn(); fn(); fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(opt.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / opt.reps

    a = torch.randn(4096, 4096, device=dev)
    for _ in range(40):
        a @ a                                                 # (clocks up before the first timed launch)
    torch.cuda.synchronize()
    g = torch.Generator(device=dev).manual_seed(0)
    res = {}
    for name, ci, co, k, p, refl, H, W in SHAPES:
        op = ops.Conv(ci, co, k, 1, p, reflect=refl)
        x = torch.randn(B, H, W, ci, device=dev, generator=g).bfloat16()
        w = (torch.randn(k * k, co, ci, device=dev, generator=g) * 0.02).bfloat16()
        wt = ops.transpose_taps(w)
        gy = torch.randn(B, H, W, co, device=dev, generator=g).bfloat16()
        add = torch.randn(B, H, W, ci, device=dev, generator=g).bfloat16()
        y = torch.randn(B, H, W, ci, device=dev, generator=g).bfloat16()
        coef = torch.stack([torch.rand(ci, device=dev, generator=g) + 0.5, torch.randn(ci, device=dev, generator=g) * 0.3,
                            torch.randn(ci, device=dev, generator=g) * 0.1, torch.rand(ci, device=dev, generator=g) + 0.5])
        for c in (10, 11, 12):
            if c == 11 and co % 128:
                continue
            res["%s | id %d fwd+stats" % (name, c)] = timeit(lambda: op.fwd(x, w, stats=True, tile_cfg=c))
            if refl:
                continue
            res["%s | id %d dgrad+res" % (name, c)] = timeit(lambda: op.dgrad(gy, wt, (H, W), addsrc=add, tile_cfg=c))
            slots = op.dgrad_bnb_slots(B, H, W, torch.bfloat16, tile_cfg=c) if c != 11 else 0
            if slots > 0:
                part = torch.empty(slots, 2, ci, device=dev)
                res["%s | id %d dgrad+res+bnb" % (name, c)] = timeit(
                    lambda: op.dgrad(gy, wt, (H, W), addsrc=add, bnb=(y, coef, True, part), tile_cfg=c))
    print("RESULT " + json.dumps(res))


def run(variant, cmd, limit, pick):
    env = dict(os.environ)
    if variant == "parent":
        env["GDN_HIP_LIB"] = str(pathlib.Path(opt.parent_lib).resolve())
    else:
        env.pop("GDN_HIP_LIB", None)
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, cwd=str(ROOT))
    lines = [l for l in p.stdout.splitlines() if pick(l)]
    if p.returncode != 0 or not lines:
        sys.stdout.write(p.stdout)
        raise SystemExit("child %s failed (exit status %d): nothing more is started" % (variant, p.returncode))
    return lines[-1]


def one_round(variant):
    me = [sys.executable, str(pathlib.Path(__file__).resolve()), "--child", variant, "--parent-lib", opt.parent_lib,
          "--reps", str(opt.reps), "--batch", str(opt.batch)]
    rec = json.loads(run(variant, me, 300, lambda l: l.startswith("RESULT "))[len("RESULT "):])
    bench = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(opt.steps), "--warmup", str(opt.warmup),
             "--mode", "RtoD", "--dtype", "bf16", "--batch", str(opt.batch)]
    rec["RtoD bf16 training images/s"] = json.loads(run(variant, bench, 600, lambda l: l.startswith("{") and '"value"' in l))["value"]
    return rec


def main():
    assert pathlib.Path(opt.parent_lib).exists() and NEW_LIB.exists()
    rounds = {"new": [], "parent": []}
    for r in range(opt.rounds):
        for v in (("new", "parent") if r % 2 == 0 else ("parent", "new")):
            rounds[v].append(one_round(v))
            print("round %d %-6s %s" % (r, v, json.dumps(rounds[v][-1])))
            sys.stdout.flush()
    out = {"batch": opt.batch, "rounds": opt.rounds, "reps": opt.reps, "bench_steps": opt.steps, "items": {}}
    bad = 0
    print("%-42s %28s %28s  %s" % ("item (ms per launch; last: images/s)", "new median (min, max)", "parent median (min, max)", "new within parent's spread / 0.5 %"))
    for item in rounds["parent"][0]:
        st = {}
        for v in ("new", "parent"):
            xs = [r[item] for r in rounds[v]]
            st[v] = {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}
        n, p = st["new"], st["parent"]
        rate = item.endswith("images/s")                      # (higher is better; the times: lower)
        ok = n["median"] >= p["min"] if rate else n["median"] <= p["max"]
        if p["max"] - p["min"] < 0.005 * p["median"]:
            ok = ok or (n["median"] >= 0.995 * p["median"] if rate else n["median"] <= 1.005 * p["median"])
        bad += not ok
        out["items"][item] = {"new": n, "parent": p, "ok": ok}
        print("%-42s %9.4f (%8.4f, %8.4f) %9.4f (%8.4f, %8.4f)  %s  %+.2f %%" % (
            item, n["median"], n["min"], n["max"], p["median"], p["min"], p["max"], "ok" if ok else "OUTSIDE", (n["median"] / p["median"] - 1) * 100))
    print("items outside: %d of %d" % (bad, len(out["items"])))
    line = json.dumps(out)
    print(line)
    if opt.out:
        pathlib.Path(opt.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(opt.out).write_text(line + "\n")


if __name__ == "__main__":
    child() if opt.child else main()
