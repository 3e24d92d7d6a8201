"""The legacy AutoEncoder's three stride-1 ConvTranspose2d decoder layers at B = 20 and their training shapes: forward + data
gradient + weight gradient of one layer alone, through the transform-domain form (ops.Conv(flip_taps=True): frequency domain
for 5x5 / 7x7, Winograd for 3x3; GDN_HINT_TRAIN, saved state, as a trained layer runs it) and through the direct kernels
(op.fwd / op.dgrad / op.wgrad on the transposed=True op -- the baseline).  HIP events, the two forms interleaved, best of 3
rounds; every window is sized to about 0.4 s from a first estimate of the call time.  The spread (max / min - 1 over the rounds)
is printed beside each time, and the shader clock held during the last round (ops.ShaderClock; n/a with the reason if the
probe has no stream that runs beside the measured one, or its watcher did not see the stop).  --step also times one RtoD_single
training step of the whole network (B = 20, fp32, fused Adam).

    python tests/diag/legacy_layer_time.py [--step] [--json OUT.json]
"""
import argparse
import json
import pathlib
import sys

import torch

R = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(R / "gdn-pytorch_amd"))
sys.path.insert(0, str(R))
from gdn_amd import ops  # noqa: E402

B = 20
LAYERS = [("upconv0", 512, 256, 3, 32, 104), ("upconv1", 256, 128, 5, 64, 208), ("upconv2", 128, 64, 7, 128, 416)]


WINDOW_S = 0.4        # length of one timed window (the clock probe's watcher gives up after 2 s)


def window(fn, reps, clk=None):
    """ms per call over `reps` calls (HIP events); with `clk` the launches run inside the probe's bracket -- the synchronise
    comes AFTER the bracket closes (its stop marker is issued on exit), then the clock is read."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if clk is None:
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
    else:
        with clk:
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def clock_of(clk):
    """GHz, or the reason there is none."""
    if clk.side is None:
        return None, "no stream runs beside the measured one"
    g = clk.ghz()
    return g, None if g is not None else "the watcher did not see the stop"


def interleaved(fns, rounds=3, dev=None):
    """ms per call of each fn: warm-up, then `rounds` rounds in which the candidates take turns;
    (best, spread, GHz, why no GHz, reps)."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    reps = [max(5, int(WINDOW_S * 1e3 / window(fn, 3))) for fn in fns]
    t = [[] for _ in fns]
    ghz = [(None, "not probed")] * len(fns)
    for r in range(rounds):
        for i, fn in enumerate(fns):
            if r == rounds - 1:
                clk = ops.ShaderClock(dev)
                t[i].append(window(fn, reps[i], clk))
                ghz[i] = clock_of(clk)
            else:
                t[i].append(window(fn, reps[i]))
    return [(min(v), max(v) / min(v) - 1.0, g[0], g[1], n) for v, g, n in zip(t, ghz, reps)]


def layer(dev, name, ci, co, k, H, W):
    x = torch.randn(B, H, W, ci, device=dev)
    w = torch.randn(k * k, co, ci, device=dev) / (ci * k * k) ** 0.5
    g = torch.randn(B, H, W, co, device=dev)
    dw_t, dw_d = torch.empty_like(w), torch.empty_like(w)
    flip = ops.Conv(ci, co, k, 1, k // 2, flip_taps=True)
    direct = ops.Conv(ci, co, k, 1, k // 2, transposed=True)

    if k >= 5:
        def transform():
            y, st, xf = flip.fft_fwd(x, w, stats=True, spectrum=True, train=True)
            return y, flip.fft_bwd(g, w, (H, W), xf=xf, dw_tap=dw_t, train=True)
    else:
        def transform():
            y, st, sv = flip.wino_fwd(x, w, stats=True, state=True)
            return y, flip.wino_bwd(g, w, (H, W), state=sv, dw_tap=dw_t)

    def baseline():
        y, st = direct.fwd(x, w, stats=True)
        dx = direct.dgrad(g, ops.transpose_taps(w), (H, W))
        direct.wgrad(x, g, dw_d)
        return y, dx

    yt, dxt = transform()
    yd, dxd = baseline()
    err = max(float((a - b).abs().max() / b.abs().max()) for a, b in ((yt, yd), (dxt, dxd), (dw_t, dw_d)))
    (tt, st_, gt, wt_, nt), (td, sd_, gd, wd_, nd) = interleaved([transform, baseline], dev=dev)
    macs = 3.0 * B * H * W * ci * co * k * k
    return {"layer": name, "cin": ci, "cout": co, "k": k, "H": H, "W": W, "transform_ms": tt, "transform_spread": st_,
            "direct_ms": td, "direct_spread": sd_, "ratio_direct_over_transform": td / tt, "transform_ghz": gt, "direct_ghz": gd,
            "no_clock_reason": wt_ or wd_, "reps_per_window": [nt, nd],
            "direct_tflops": 2 * macs / td * 1e-9, "max_rel_diff_transform_vs_direct": err}


def step_time(dev, rounds=3):
    import gdn_amd.AE_model_unet as M
    from gdn_amd import utils as U
    from gdn_amd.optim import Adam
    from oracle import gdn_oracle as O
    depth, rgb, sparse = [t.to(dev) for t in O.synthetic_batch(B, 128, 416, seed=0)]
    torch.manual_seed(0)
    net = M.AutoEncoder().to(dev).train()
    opt = Adam(net.parameters(), 2e-5, [0.9, 0.999], eps=1e-08, weight_decay=5e-4)

    def step():
        out = net(rgb, istrain=False)
        loss = U.rtod_pixel_loss(out, depth, rgb, sparse)[0]
        opt.zero_grad()
        loss.backward()
        opt.step()

    (t, spread, ghz, why, n), = interleaved([step], rounds=rounds, dev=dev)
    return {"workload": "legacy AutoEncoder RtoD_single step, B=20, 128x416, fp32", "step_ms": t, "spread": spread, "ghz": ghz,
            "no_clock_reason": why, "reps_per_window": n, "images_per_s": B / t * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "layers": [layer(dev, *l) for l in LAYERS]}
    fmt = lambda g: "n/a" if g is None else "%.2f" % g
    print("%-8s %4s %4s %2s | %10s %7s %5s | %10s %7s %5s | %6s  (fwd + dgrad + wgrad, ms; spread = max/min - 1 of 3 rounds)"
          % ("layer", "Cin", "Cout", "k", "transform", "spread", "GHz", "direct", "spread", "GHz", "ratio"))
    for r in res["layers"]:
        if r["no_clock_reason"]:
            print("%s: no shader clock: %s" % (r["layer"], r["no_clock_reason"]))
        print("%-8s %4d %4d %2d | %10.3f %6.1f%% %5s | %10.3f %6.1f%% %5s | %5.2fx   direct %.1f TFLOP/s, max rel diff %.1e"
              % (r["layer"], r["cin"], r["cout"], r["k"], r["transform_ms"], 100 * r["transform_spread"], fmt(r["transform_ghz"]),
                 r["direct_ms"], 100 * r["direct_spread"], fmt(r["direct_ghz"]), r["ratio_direct_over_transform"],
                 r["direct_tflops"], r["max_rel_diff_transform_vs_direct"]))
    if a.step:
        res["step"] = step_time(dev)
        s = res["step"]
        print("%s: %.2f ms (spread %.1f%%, %s GHz) = %.1f images/s" % (s["workload"], s["step_ms"], 100 * s["spread"], fmt(s["ghz"]),
                                                                      s["images_per_s"]))
    if a.json:
        pathlib.Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
