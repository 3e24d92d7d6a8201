#!/usr/bin/env python3
"""Headline benchmark: training images/s of the GDN hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Without a launcher environment (RANK unset) ``--gpus N`` with N > 1 starts N fresh rank processes itself (one per GPU,
`distributed.launch_ranks`: the parent never touches the GPU, forwards rank 0's JSON line as the last line of its own
stdout and exits with the first non-zero child code) -- the reference trains on N GPUs from ONE command
(GDN_main.py:24,150-173, `--gpu_num 0,1,2,3` + nn.DataParallel).  Under torch.distributed.run the ranks are the launcher's;
``--gpus`` must then equal WORLD_SIZE (anything else is an error, rc 2).

A "step" is one full training step of BASELINE.json's configs[1]: DtoD mode
(AutoEncoder_DtoD forward, BerHu + 3*Sobel loss, backward, fused Adam), batch 20
per GPU, 128x416, fp32, synthetic KITTI-shaped inputs resident in HBM.  With N>1
each rank trains its own batch-20 shard and the gradient arena is all-reduced
with RCCL (weak scaling).  Rank 0 prints ONE JSON line.

A plain run does only what that line's headline figure needs: set up, warm up, time the --steps steps, print `value` (images/s),
`ms_per_step` and the workload's description.  --dump-outputs DIR also writes what the last timed step computed (loss, depth
map, a seeded sample of the model's state after Adam) as DIR/<name>.npy.  With --full the same line also carries
  step_kernel_breakdown -- device time per kernel symbol over two steps after the timed region (torch.profiler): decides which
                  kernel `roofline` describes;
  roofline     -- the dominant kernel of the step by that measurement: the per-bin complex GEMMs of the frequency-domain layers
                  (`cgemm_bins_kernel`, fp32 MFMA, on the MFMA / HBM ridge; the other family is under `roofline_gemm_x3`) or
                  `gemm_x3_nt_kernel`, the 36 per-bin GEMMs of the level-3 Winograd F(4x4,3x3) 512->512 layer as bf16 x 3 split
                  products (algorithmic fp32 FLOP / time against the bf16 MFMA peak / 6); timed with HIP events on the launch
                  stream; `traffic` from the committed PMC pass;
  roofline_direct3x3, roofline_fftconv -- the direct fused 3x3 kernel (fp32 MFMA peak 157.3 TFLOP/s) and a 9x9
                  frequency-domain layer (HBM-bound, 8 TB/s) measured the same way;
  mfma_util    -- whole-step MFMA utilisation replayed from profiles/ (with the commit it was collected at);
  other_configs -- RtoD fp32 / bf16 (BASELINE configs[2]), DtoD bf16, inference B = 64 256x832 under a hipGraph;
  cpu_baseline -- the CPU oracle (same step, reference semantics, torch CPU) on a
                  bounded sample, N=1 rank 0 only.
"""
import argparse
import contextlib
import json
import os
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent
for p in (str(ROOT), str(ROOT / "gdn-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md, v_mfma_f32_32x32x2_f32
PEAK_BF16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md, dense bf16 (v_mfma_f32_32x32x16_bf16); never the 2:1-sparse figure
DTOD_TRAIN_GFLOP_PER_IMG = 1017.5


NOMINAL_GHZ = 2.4                 # the engine clock both MFMA peaks above are quoted at (MI355X_MICROARCH.md)


def timed_with_clock(fn, reps, dev, warm=3):
    """(ms per launch, shader clock in GHz held during the window or None): `reps` launches of fn timed with HIP events on the
    launch stream while one sleeping wave on a second stream reads the cycle counter against the 100 MHz counter (ops.ShaderClock)."""
    from gdn_amd import ops
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    clk = ops.ShaderClock(dev)
    with clk:
        e0.record()                      # torch's current stream == the stream the C ABI launches on
        for _ in range(reps):
            fn()
        e1.record()
    torch.cuda.synchronize()
    try:
        ghz = clk.ghz()
    except Exception:  # noqa: BLE001
        ghz = None
    return e0.elapsed_time(e1) / reps, ghz


def at_clock(rec, ghz):
    """Adds `clock_ghz` (measured during the timed window) and `frac_at_clock` = achieved / (peak scaled to that clock) to an
    MFMA-bound roofline record: the part of a box-to-box difference in `frac` that is the clock the chip held under this
    kernel's power draw, not the kernel."""
    rec["clock_ghz"] = None if ghz is None else round(ghz, 3)
    if ghz and rec.get("bound") == "mfma" and rec.get("peak"):
        rec["frac_at_clock"] = round(rec["achieved"] / (rec["peak"] * ghz / NOMINAL_GHZ), 4)
        rec["peak_at_clock"] = round(rec["peak"] * ghz / NOMINAL_GHZ, 1)
    else:
        rec["frac_at_clock"] = None
    return rec


def gpu_state():
    """Power cap / average power / current engine-clock level of GPU 0 as sysfs shows them to an ordinary user (no rocm-smi):
    whatever is readable, None otherwise."""
    import glob
    out = {}

    def rd(pat):
        for f in sorted(glob.glob(pat)):
            try:
                return open(f).read().strip()
            except OSError:
                continue
        return None
    base = "/sys/class/drm/card*/device/"
    cap, avg = rd(base + "hwmon/hwmon*/power1_cap"), rd(base + "hwmon/hwmon*/power1_average") or rd(base + "hwmon/hwmon*/power1_input")
    out["power_cap_w"] = round(int(cap) / 1e6, 1) if cap and cap.isdigit() else None
    out["power_now_w"] = round(int(avg) / 1e6, 1) if avg and avg.isdigit() else None
    sclk = rd(base + "pp_dpm_sclk")
    out["sclk_levels"] = None if not sclk else [ln.strip() for ln in sclk.splitlines()][:8]
    out["perf_level"] = rd(base + "power_dpm_force_performance_level")
    return out


def conv3x3_roofline(dev, B, level, reps=20):
    """Fused 3x3 s1 512->512 conv + BN-stats epilogue at level 3 (16x52) or 4 (8x26)."""
    from gdn_amd import ops
    H, W = (16, 52) if level == 3 else (8, 26)
    op = ops.Conv(512, 512, 3, 1, 1)
    x = torch.randn(B, H, W, 512, device=dev)
    w = torch.randn(9, 512, 512, device=dev) * 0.02
    y, st = op.fwd(x, w, stats=True)          # outputs allocated once: the timed loop is launches only
    ms, ghz = timed_with_clock(lambda: op.fwd(x, w, stats=True, out=y, stats_out=st), reps, dev)
    flop = 2.0 * B * H * W * 4608 * 512
    return ms, flop, ghz


def wino_roofline(dev, B, reps=20):
    """The 512->512 3x3 layer at level 3 (16x52) as it now runs: Winograd F(4x4,3x3) with bf16 x 3 GEMMs.  Times the dominant
    kernel (the 36 per-bin GEMMs) alone, round 2's fp32 MFMA GEMMs of the F(2x2,3x3) plan beside it, and the whole forward
    (input / weight transforms + GEMMs + output transform with the BatchNorm partials)."""
    from gdn_amd import ops
    H, W, C = 16, 52, 512
    op = ops.Conv(C, C, 3, 1, 1)
    tiles = B * (H // 2) * (W // 2)
    V = torch.randn(16, tiles, C, device=dev)
    U = torch.randn(16, C, C, device=dev) * 0.02
    Mo = torch.empty(16, tiles, C, device=dev)
    x = torch.randn(B, H, W, C, device=dev)
    w = torch.randn(9, C, C, device=dev) * 0.02

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    ms_g = timed(lambda: op.wino_gemm_only(V, U, Mo, B, H, W))           # the fp32 MFMA per-bin GEMM (GDN_X3=0 path), F(2x2,3x3) shape
    del V, U, Mo
    # what the layer runs since round 4: F(4x4,3x3), 36 bins x [B * 4 * 13 tiles x 512] x [512 x 512] as bf16 x 3 split products
    tiles4 = B * (H // 4) * (W // 4)
    V4 = torch.randn(36, tiles4, C, device=dev)
    Up4 = ops.gemm_x3_pack(torch.randn(36, C, C, device=dev) * 0.02)
    Mo4 = torch.empty(36, tiles4, C, device=dev)
    ms_x, ghz_x = timed_with_clock(lambda: ops.gemm_x3_nt(V4, Up4, C, out=Mo4), reps, dev)
    ms_l = timed(lambda: op.wino_fwd(x, w, stats=True, state=True))
    return ms_g, 2.0 * 16 * tiles * C * C, ms_l, 2.0 * B * H * W * 9 * C * C, ms_x, 2.0 * 36 * tiles4 * C * C, ghz_x


def fftconv_roofline(dev, B, reps=10):
    """Frequency-domain 9x9 64->64 layer at level 0 (128x416): forward (+BN partials, spectra kept) and backward
    (dgrad + wgrad) against the bytes the decomposition has to move (spectra written once and read once)."""
    from gdn_amd import ops
    H, W, C, k = 128, 416, 64, 9
    op = ops.Conv(C, C, k, 1, k // 2)
    x = torch.randn(B, H, W, C, device=dev)
    w = torch.randn(k * k, C, C, device=dev) * 0.02
    gy = torch.randn(B, H, W, C, device=dev)
    dw = torch.empty_like(w)

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def plan(train, NP):
        y, st, xf = op.fft_fwd(x, w, stats=True, spectrum=True, train=train)
        ms_f = timed(lambda: op.fft_fwd(x, w, stats=True, spectrum=True, train=train))
        ms_b = timed(lambda: op.fft_bwd(gy, w, (H, W), xf=xf, dw_tap=dw, train=train))
        T = NP + 1 - k
        tiles = B * (-(-H // T)) * (-(-W // T))
        spec = tiles * NP * (NP // 2 + 1) * C * 8          # one spectrum, bytes
        act = B * H * W * C * 4
        by_f = act + 4 * spec + act                        # x -> Xf -> GEMM -> Yf -> y
        by_b = 2 * act + 8 * spec                          # dy -> Df | Df -> Ef | Ef -> S | S -> dx | wgrad reads Df + Xf
        return ms_f, ms_b, by_f, by_b

    ms_f, ms_b, by_f, by_b = plan(False, 32)               # the forward-optimal plan (eval-mode layers; round 1's line)
    tf, tb, tby_f, tby_b = plan(True, 40)                  # GDN_HINT_TRAIN: what a trained 9x9 layer runs in the timed step
    return {"layer": "9x9 s1 64->64, B=%d 128x416 (level 0), 32x32 tiles" % B, "bound": "hbm", "peak": 8000.0, "unit": "GB/s",
            "fwd_ms": round(ms_f, 4), "fwd_bytes": by_f, "fwd_achieved": round(by_f / ms_f / 1e6, 1),
            "bwd_ms": round(ms_b, 4), "bwd_bytes": by_b, "bwd_achieved": round(by_b / ms_b / 1e6, 1),
            "achieved": round(by_f / ms_f / 1e6, 1), "frac": round(by_f / ms_f / 1e6 / 8000.0, 4),
            "traffic": 2924000000,      # forward kernels' L2->fabric bytes, PMC (profiles/r01_fft_pmc.txt: 874 + 27 + 1173 + 849 MB)
            "direct_equiv_tflops_fwd": round(2.0 * B * H * W * k * k * C * C / ms_f / 1e9, 1),
            "train_plan_40x40_tiles": {
                "note": "the same layer as the training step runs it (GDN_HINT_TRAIN: 4 x 13 tiles of 32 valid outputs, 26 % fewer "
                        "spectrum bytes and GEMM rows): fewer bytes in less time -- the byte rate falls, the layer gets faster",
                "fwd_ms": round(tf, 4), "fwd_bytes": tby_f, "fwd_achieved": round(tby_f / tf / 1e6, 1),
                "bwd_ms": round(tb, 4), "bwd_bytes": tby_b, "bwd_achieved": round(tby_b / tb / 1e6, 1),
                "fwd_traffic": fft_train_fwd_traffic()}}


def cgemm_roofline(dev, B, reps=20):
    """The per-bin complex GEMMs of the frequency-domain layers (cgemm_bins_kernel<false|true>, cgemm_tn_bins_kernel: the largest
    symbol family of the headline step) on the 9x9 64->64 layer's TRAINING plan at level 0: 40-point tiles, 840 bins x
    [1040 x 64] x [64 x 64] complex = three real fp32-MFMA products each (Gauss).  Timed alone, and the backward's pair
    (data gradient + weight-gradient reduction) on two streams as the step runs them.  The GEMM sits on the ridge of the fp32
    matrix pipe and HBM (23 FLOP/B): both fractions are reported."""
    from gdn_amd import ops
    H, W, C, k = 128, 416, 64, 9
    op = ops.Conv(C, C, k, 1, k // 2)
    ws, bins, M, npnt = op.fft_cgemm_only(B, H, W, 0, train=True)
    s2 = torch.cuda.Stream()

    def timed(fn, sync_side=False):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        if sync_side:
            torch.cuda.current_stream().wait_stream(s2)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def pair():
        s2.wait_stream(torch.cuda.current_stream())
        op.fft_cgemm_only(B, H, W, 1, ws=ws, train=True)
        op.fft_cgemm_only(B, H, W, 2, ws=ws, train=True, st=s2.cuda_stream)
        torch.cuda.current_stream().wait_stream(s2)

    ms = [1e9, 1e9, 1e9]
    ms_pair = 1e9
    ghz = None
    for _ in range(3):                                     # interleaved rounds, best of three (cdna_hip_programming.md rule 24)
        for which in range(3):
            if which == 0:                                 # the record's kernel: with the clock it ran at
                t, g = timed_with_clock(lambda: op.fft_cgemm_only(B, H, W, 0, ws=ws, train=True), reps, dev)
                if t < ms[0]:
                    ms[0], ghz = t, g
            else:
                ms[which] = min(ms[which], timed(lambda w=which: op.fft_cgemm_only(B, H, W, w, ws=ws, train=True)))
        ms_pair = min(ms_pair, timed(pair, sync_side=True))
    flop = 3 * 2.0 * bins * M * C * C                      # three real products per complex product
    by = 2 * M * bins * C * 8 + bins * 3 * C * C * 4       # one spectrum in, one out, the weight planes
    by_tn = 2 * M * bins * C * 8 + bins * 2 * C * C * 4
    a = flop / (ms[0] * 1e-3) / 1e12

    def one(t, b):
        return {"ms_per_launch": round(t, 4), "achieved": round(flop / (t * 1e-3) / 1e12, 2),
                "frac": round(flop / (t * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4), "hbm_gbps": round(b / t / 1e6, 1),
                "hbm_frac": round(b / t / 1e6 / 8000.0, 4)}
    return at_clock({"kernel": "cgemm_bins_kernel<false>: the %d per-bin complex GEMMs [%d x 64] x [64 x 64] of the 9x9 s1 64->64 layer's training plan "
                      "(%d-point tiles), B=%d 128x416 (level 0), 3 real fp32 products per complex product on v_mfma_f32_32x32x2_f32"
                      % (bins, M, npnt, B),
            "bound": "mfma", "unit": "TFLOP/s", "achieved": round(a, 2), "peak": PEAK_F32_MFMA_TFLOPS,
            "frac": round(a / PEAK_F32_MFMA_TFLOPS, 4), "gflop_per_launch": round(flop / 1e9, 2), "ms_per_launch": round(ms[0], 4),
            "bytes_per_launch": by, "hbm_gbps": round(by / ms[0] / 1e6, 1), "hbm_frac": round(by / ms[0] / 1e6 / 8000.0, 4),
            "traffic": pmc_traffic("r05_cgemm_pmc.json"),
            "note": "arithmetic intensity %.1f FLOP/B: on the ridge between the fp32 matrix pipe (157.3 TFLOP/s) and HBM (8 TB/s); frac is "
                    "against the pipe, hbm_frac against the memory" % (flop / by),
            "dgrad_cgemm_bins_true": one(ms[1], by), "wgrad_cgemm_tn_bins": one(ms[2], by_tn),
            "backward_pair_two_streams": {"ms": round(ms_pair, 4), "sum_alone_ms": round(ms[1] + ms[2], 4),
                                          "achieved": round(2 * flop / (ms_pair * 1e-3) / 1e12, 2),
                                          "frac": round(2 * flop / (ms_pair * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)}}, ghz)


def wgrad_ring_roofline(dev, B, reps=20):
    """wgrad_ring_bf16<9> (round 5, csrc/wgrad_ring.h): the 9x9 64->64 weight gradient at level 0 on the bf16 matrix pipe, with the
    fixed-order slab reduce, against the round-1 kernel."""
    from gdn_amd import ops
    H, W, C, k = 128, 416, 64, 9
    op = ops.Conv(C, C, k, 1, k // 2)
    x = torch.randn(B, H, W, C, device=dev).bfloat16()
    gy = torch.randn(B, H, W, C, device=dev).bfloat16()
    dw = torch.empty(k * k, C, C, device=dev)

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    ms_new = ms_old = 1e9
    ghz = None
    for _ in range(3):
        ms_old = min(ms_old, timed(lambda: op.wgrad(x, gy, dw, cfg=2)))
        t, g = timed_with_clock(lambda: op.wgrad(x, gy, dw, cfg=4), reps, dev)
        if t < ms_new:
            ms_new, ghz = t, g
    flop = 2.0 * B * H * W * k * k * C * C
    a = flop / (ms_new * 1e-3) / 1e12
    return at_clock({"kernel": "wgrad_ring_bf16<9, true> + wgrad_bf16_reduce: 9x9 s1 64->64 weight gradient, B=%d 128x416 (level 0), bf16 in / fp32 "
                      "accumulate, fp32 dW (DESIGN.md 2.12)" % B,
            "bound": "mfma", "unit": "TFLOP/s", "achieved": round(a, 1), "peak": PEAK_BF16_MFMA_TFLOPS,
            "frac": round(a / PEAK_BF16_MFMA_TFLOPS, 4), "gflop_per_launch": round(flop / 1e9, 1), "ms_per_launch": round(ms_new, 4),
            "traffic": pmc_traffic("r05_wgrad_ring_pmc.json"),
            "round1_kernel": {"kernel": "conv_wgrad_bf16<9, 8, 7> (cfg 2)", "ms_per_launch": round(ms_old, 4),
                              "achieved": round(flop / (ms_old * 1e-3) / 1e12, 1)}}, ghz)


def step_kernel_breakdown(step, nsteps=2, top=8):
    """Device time per kernel SYMBOL (template arguments and namespaces stripped) over `nsteps` steps run after the timed region,
    from torch.profiler (roctracer): which kernel the step spends most of its time in is measured, not asserted.  `families` sums
    EVERY symbol of the step by family prefix (not only the `top` rows shown), `top_symbol` is the single largest symbol.
    Only ever called when this process is the whole job (world size 1): `step` contains the gradient all-reduce, and a
    collective issued by one rank after the others have left the group never returns under RCCL."""
    import re
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(nsteps):
                step()
            torch.cuda.synchronize()
        agg, total = {}, 0.0
        for e in prof.key_averages():
            t = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
            if t <= 0.0:
                continue
            name = e.key.replace("(anonymous namespace)::", "").replace("void ", "")
            name = re.sub(r"[<(].*", "", name).split("::")[-1].strip()
            a = agg.setdefault(name, [0.0, 0])
            a[0] += t
            a[1] += int(e.count)
            total += t
        if total <= 0.0:
            return {"error": "the profiler returned no device time"}
        allrows = sorted(agg.items(), key=lambda kv: -kv[1][0])
        fam = {}
        for k, v in allrows:
            f = kernel_family(k)
            fam[f] = fam.get(f, 0.0) + v[0] / total
        return {"steps": nsteps, "kernel_ms_per_step": round(total / nsteps / 1e3, 3), "symbols": len(allrows),
                "top_symbol": allrows[0][0],
                "families": {k: round(v, 4) for k, v in sorted(fam.items(), key=lambda kv: -kv[1])},
                "top": [{"symbol": k, "ms_per_step": round(v[0] / nsteps / 1e3, 3), "share": round(v[0] / total, 4),
                         "launches_per_step": round(v[1] / nsteps, 1)} for k, v in allrows[:top]]}
    except Exception as e:  # noqa: BLE001
        return {"error": "%s: %s" % (type(e).__name__, e)}


FAMILIES = (("cgemm", "cgemm"), ("gemm_x3", "gemm_x3"), ("fft", "fft_transforms"), ("ifft", "fft_transforms"),
            ("wino_gemm", "wino_gemm_f32"), ("wino", "winograd_transforms"), ("w2_", "winograd_transforms"), ("bn_", "batchnorm"),
            ("conv_ring", "bf16_ring"), ("wgrad_ring", "bf16_ring"), ("conv_igemm", "direct_conv"), ("conv_wgrad", "direct_conv"),
            ("conv_rowpatch", "direct_conv"), ("conv_c1", "direct_conv"), ("conv_head", "direct_conv"), ("adam", "adam"))


def kernel_family(symbol):
    """Family of a kernel symbol for step_kernel_breakdown (prefix table; everything else is 'other')."""
    for pre, fam in FAMILIES:
        if symbol.startswith(pre):
            return fam
    return "other"


def ring_roofline(dev, B, reps=20):
    """BASELINE configs[2]'s dominant kernel: the LDS-DMA ring kernel on the 9x9 64->64 stride-1 layer at level 0 (128x416) on the
    bf16 matrix pipe -- conv_ring2_bf16<64, 9> (round 5: 512 x 64 tiles on 32-channel slabs, the automatic choice), round 4's
    conv_ring_bf16<64, 9> (256 x 64, tile id 10) beside it -- forward with the BatchNorm partials, and the data gradient with a
    residual."""
    from gdn_amd import ops
    H, W, C, k = 128, 416, 64, 9
    op = ops.Conv(C, C, k, 1, k // 2)
    x = torch.randn(B, H, W, C, device=dev).bfloat16()
    w = (torch.randn(k * k, C, C, device=dev) * 0.02).bfloat16()
    wt = ops.transpose_taps(w)
    add = torch.randn(B, H, W, C, device=dev).bfloat16()
    y, st = op.fwd(x, w, stats=True)

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()                      # torch's current stream == the stream the C ABI launches on
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    # interleaved rounds in one process, best of three each: the clock the chip holds depends on what ran just before
    # (cdna_hip_programming.md rule 24), so a single A-then-B pass ranks whichever ran second higher
    ms_f = ms_d = ms_old = ms_r4 = 1e9
    ghz = None
    st10 = op.fwd(x, w, stats=True, tile_cfg=10)[1]            # (one partial-statistics slot per tile: the count follows the tile)
    st9 = op.fwd(x, w, stats=True, tile_cfg=9)[1]
    for _ in range(3):
        ms_old = min(ms_old, timed(lambda: op.fwd(x, w, stats=True, out=y, stats_out=st9, tile_cfg=9)))
        ms_r4 = min(ms_r4, timed(lambda: op.fwd(x, w, stats=True, out=y, stats_out=st10, tile_cfg=10)))
        t, g = timed_with_clock(lambda: op.fwd(x, w, stats=True, out=y, stats_out=st), reps, dev)
        if t < ms_f:
            ms_f, ghz = t, g
        ms_d = min(ms_d, timed(lambda: op.dgrad(x, wt, (H, W), addsrc=add)))
    flop = 2.0 * B * H * W * k * k * C * C
    a = flop / (ms_f * 1e-3) / 1e12
    return at_clock({"kernel": "conv_ring2_bf16<64, 9>: 9x9 s1 64->64 + BN-stats epilogue, B=%d 128x416 (level 0), bf16 in / fp32 accumulate -- the "
                      "dominant kernel of the RtoD bf16 step (configs[2]); LDS-DMA ring, persistent workgroups, 512 x 64 tiles "
                      "(DESIGN.md 2.11)" % B,
            "bound": "mfma", "unit": "TFLOP/s", "achieved": round(a, 1), "peak": PEAK_BF16_MFMA_TFLOPS,
            "frac": round(a / PEAK_BF16_MFMA_TFLOPS, 4), "gflop_per_launch": round(flop / 1e9, 1), "ms_per_launch": round(ms_f, 4),
            "traffic": pmc_traffic("r05_conv_ring_pmc.json"),
            "round4_kernel": {"kernel": "conv_ring_bf16<64, 9> (tile_cfg 10: 256 x 64 tiles)", "ms_per_launch": round(ms_r4, 4),
                              "achieved": round(flop / (ms_r4 * 1e-3) / 1e12, 1)},
            "dgrad_with_residual": {"ms_per_launch": round(ms_d, 4), "achieved": round(flop / (ms_d * 1e-3) / 1e12, 1)},
            "round1_kernel": {"kernel": "conv_rowpatch_bf16<64,4,1> (tile_cfg 9)", "ms_per_launch": round(ms_old, 4),
                              "achieved": round(flop / (ms_old * 1e-3) / 1e12, 1)}}, ghz)


def pmc_traffic(name="r01_conv3x3_pmc.json"):
    """L2->fabric bytes per launch of the roofline kernel from the committed rocprofv3 PMC passes
    (FETCH_SIZE doubled per the gfx950 correction + WRITE_SIZE); None if the summary is absent."""
    f = ROOT / "profiles" / name
    try:
        return json.loads(f.read_text())["traffic_bytes_per_launch"]
    except Exception:  # noqa: BLE001
        return None


def node_cores():
    """(logical CPUs of the node, physical cores if /proc/cpuinfo tells, CPUs this process may run on)."""
    logical = os.cpu_count() or 1
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = logical
    physical = None
    try:
        seen, phys, core = set(), None, None
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("physical id"):
                phys = ln.split(":")[1].strip()
            elif ln.startswith("core id"):
                core = ln.split(":")[1].strip()
            elif not ln.strip():
                if phys is not None and core is not None:
                    seen.add((phys, core))
                phys = core = None
        physical = len(seen) or None
    except OSError:
        pass
    return logical, physical, usable


def fft_train_fwd_traffic():
    """L2 -> fabric bytes of the three forward kernels of the 9x9 64->64 layer on its training plan (fft2d_fwd<40>, cgemm_bins<false>,
    ifft2d_valid<40>; B = 20) from the committed PMC passes (profiles/r06_fft_pmc.json; FETCH_SIZE doubled per the gfx950
    correction + WRITE_SIZE); None if absent."""
    try:
        d = json.loads((ROOT / "profiles" / "r06_fft_pmc.json").read_text())["kernels"]
        tot = 0.0
        for k, v in d.items():
            if k.startswith(("fft2d_fwd_kernel<40>", "ifft2d_valid_kernel<40>", "cgemm_bins_kernel<false>")):
                tot += v["fetch_bytes"] + v["write_bytes"]
        return int(tot) or None
    except Exception:  # noqa: BLE001
        return None


def cpu_baseline(batch=20):
    """The oracle's DtoD training step on the host cores at the benchmarked batch (B = 20, the node's core count
    stated).  Which thread count the step is timed at is MEASURED, cheaply: a batch-4 train-mode forward of the oracle at 32, 64,
    the physical core count and every usable CPU (each bounded; torch's CPU convolutions stop scaling well before a whole
    128-core node -- r06a: 201.7 s per step at 256 threads against 11.3 s at 32), then one untimed warm-up step and one timed step
    at the fastest count.  About 40 s of host time."""
    from oracle import gdn_oracle as O
    logical, physical, usable = node_cores()
    sd = O.init_state_dict("AutoEncoder_DtoD", seed=0)
    probe_x = O.synthetic_batch(4, 128, 416, seed=1)[0]
    cands = sorted({max(1, min(usable, n)) for n in (32, 64, physical or usable, usable)})
    probe = []
    best_n, best_t = cands[0], None
    for n in cands:
        torch.set_num_threads(n)
        ts = []
        with torch.no_grad():
            for _ in range(2):                       # the first pass builds the thread pool / primitive caches at this width
                t0 = time.time()
                O.forward_dtod({k: v.clone() for k, v in sd.items()}, probe_x, istrain=False, training=True)
                ts.append(time.time() - t0)
                if ts[-1] > 6.0:                     # already far slower than any useful setting: do not repeat it
                    break
        probe.append({"threads": n, "batch4_forward_s": round(min(ts), 3)})
        if best_t is None or min(ts) < best_t:
            best_n, best_t = n, min(ts)
        if min(ts) > 3.0 * best_t:                   # larger counts only get worse from here
            break
    torch.set_num_threads(best_n)
    data = O.synthetic_batch(batch, 128, 416, seed=0)
    st = {}
    t0 = time.time()
    O.train_step("DtoD", sd, data, st)               # warm-up (thread pools, oneDNN primitive caches), untimed
    t1 = time.time()
    O.train_step("DtoD", sd, data, st)
    dt = time.time() - t1
    return {"value": round(batch / dt, 4), "unit": "images/s", "cores": best_n, "kind": "port",
            "node_cores": {"logical": logical, "physical": physical, "usable_by_this_process": usable},
            "thread_probe": probe,
            "sample": "1 timed DtoD train step (fwd+loss+bwd+Adam, %.1f s) of the CPU oracle at batch %d, 128x416 fp32, after one "
                      "untimed warm-up step (%.1f s), at the thread count a batch-4 forward probe found fastest on this node "
                      "(thread_probe); the same workload as the GPU step" % (dt, batch, t1 - t0)}


def step_mfma_util():
    """Whole-step MFMA utilisation from the committed rocprofv3 PMC pass over training steps of this workload
    (tools/pmc_step.sh -> profiles/rNN_step_mfma_util.json, newest round): sum SQ_VALU_MFMA_BUSY_CYCLES / (4 SIMDs x CUs x
    GRBM_GUI_ACTIVE).  Counters cannot be read from inside the timed process, so the bench line carries the committed figure
    together with the commit it was collected at (`collected_at`: a replay of a file, not a live measurement); None if absent."""
    files = sorted((ROOT / "profiles").glob("r[0-9][0-9]_step_mfma_util.json"))
    if not files:
        return None
    f = files[-1]
    try:
        d = json.loads(f.read_text())
        return {"mfma_util_pct": d["mfma_util_pct"], "source": "profiles/" + f.name, "collected_at": d.get("collected_at"),
                "live": False, "steps": d.get("steps"), "note": d.get("note")}
    except Exception:  # noqa: BLE001
        return None


def infer_main(args):
    """BASELINE configs[4]: legacy AutoEncoder (the depth_extract.py network) eval forward, 256x832,
    batch 64 per GPU, one hipGraph replay per step.  fp32; images/s."""
    import gdn_amd.AE_model_unet as M
    from gdn_amd import distributed as D
    rank, local_rank, world = D.init()
    if world != args.gpus:
        print("bench.py: --gpus %d but the launcher environment has WORLD_SIZE %d" % (args.gpus, world), file=sys.stderr)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()
        return 2
    dev = torch.device("cuda", 0 if os.environ.get("GDN_SINGLE_DEVICE") == "1" else local_rank)   # (test hook: all ranks on one GPU)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    B = args.batch if args.batch != 20 else 64
    H, W = 256, 832
    with contextlib.redirect_stdout(sys.stderr):          # the ctor prints '- norm : Batch' like the reference's
        model = M.AutoEncoder(height=H, width=W).to(dev).eval().compute_dtype(args.dtype)
    x = (torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(rank)) * 2 - 1).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            out = model(x, istrain=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = None
    if not args.no_graph:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(x, istrain=False)

    def step():
        if graph is not None:
            graph.replay()
            return out
        return model(x, istrain=False)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        o = step()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    flush_c_stdio()
    if world > 1:
        torch.distributed.barrier()
    if rank == 0:
        dumped = dump_outputs(args.dump_outputs, {"depth": o}) if args.dump_outputs else None
        ms = dt / args.steps * 1e3
        rec = {"metric": "inference images/sec at 256x832 batch=64 (legacy AutoEncoder forward)",
               "value": round(B * world * args.steps / dt, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "f32" if args.dtype == "fp32" else "bf16", "data": "synthetic",
               "rccl_ranks": dist_info()[0], "dist_backend": dist_info()[1],
               "config": {"workload": "legacy AutoEncoder eval forward, batch %d per GPU, 256x832, %s, %s, "
                                      "BASELINE configs[4]" % (B, args.dtype, "hipGraph replay" if graph is not None else "eager"),
                          "global_batch": B * world, "parallelism": "dp%d" % world,
                          "direct_conv_equiv_tflops_per_gpu": round(2733.39 * B * args.steps / dt / 1e3, 2),
                          "direct_conv_equiv_note": "throughput label: direct-convolution FLOPs / time (fp32 k>=5 layers run in "
                                                    "the frequency domain, 3x3 as Winograd); not a utilisation",
                          "out_checksum": round(float(o.double().abs().mean().item()), 6)}}
        if dumped is not None:
            rec["outputs_dumped"] = dumped
        flush_c_stdio()
        print(json.dumps(rec), flush=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def make_train_step(mode, dtype, dev, batch, fast_guide=False, latent_grad=False, use_graph=False, keep=None):
    """One full training step of `mode` (DtoD / RtoD) as a closure over a resident batch: forward, fused losses,
    backward (tape), gradient all-reduce when data-parallel, fused Adam.  Returns (step, graphed-or-None).  A dict passed as
    `keep` receives the model ("model") and, at every step, the model's output ("out"; no copy: the step allocates a new one)."""
    import gdn_amd.AE_model_unet as M
    from gdn_amd import distributed as D
    from gdn_amd import trainer as T
    from gdn_amd import utils as U
    from gdn_amd.optim import Adam
    depth, rgb, sparse = batch
    G = None
    with contextlib.redirect_stdout(sys.stderr):          # the ctors print '- norm : Batch' like the reference's: keep stdout
        if mode == "DtoD":                                # to the one JSON line
            model = M.AutoEncoder_DtoD(input_dim=1).to(dev)
        else:
            model = M.AutoEncoder_2(input_dim=3).to(dev)
            torch.manual_seed(1)
            G = M.AutoEncoder_DtoD(input_dim=1).to(dev).eval()
    model.train().compute_dtype(dtype)
    if G is not None:
        G.compute_dtype(dtype)
        if latent_grad:
            G.requires_grad_(False)
    opt = Adam(model.parameters(), 2e-5, [0.9, 0.999], eps=1e-08, weight_decay=5e-4, capturable=use_graph)
    if keep is not None:
        keep["model"] = model

    from gdn_amd import tracing

    def step_fn(depth, rgb, sparse):
        tracing.push("gdn.forward")
        out = model(depth if mode == "DtoD" else rgb, istrain=False)
        if keep is not None:
            keep["out"] = out
        tracing.pop()
        tracing.push("gdn.losses")
        if mode == "DtoD":
            loss, _, _ = U.dtod_loss(out, depth, sparse)
        else:
            lat = T.guide_latent_loss(G, depth, out, faithful=not fast_guide, latent_grad=latent_grad)
            if lat.requires_grad:
                pix, _, _ = U.rtod_pixel_loss(out, depth, rgb, sparse)
                loss = pix + lat
            else:
                loss, _, _ = U.rtod_pixel_loss(out, depth, rgb, sparse, plus=lat)
        tracing.pop()
        opt.zero_grad()
        with tracing.span("gdn.backward"):
            U.backward(loss)
        with tracing.span("gdn.allreduce"):
            D.sync_gradients(model, opt)
        with tracing.span("gdn.adam"):
            opt.step()
        return loss.detach()

    graphed = None
    if use_graph:
        from gdn_amd.graph import GraphedTrainStep
        graphed = GraphedTrainStep(step_fn, (depth, rgb, sparse), opt, warmup=2)     # (its warm-up steps are untimed extras)

    def step():
        if graphed is not None:
            return graphed(depth, rgb, sparse)
        return step_fn(depth, rgb, sparse)

    return step, graphed


def roofline_records(rec, dev, B, step, world):
    """The roofline objects of the record (rank 0).  Everything here is local to this rank's GPU: single kernels timed with HIP
    events on the launch stream, and -- at world size 1 only -- the profiler pass over two more training steps.  At world > 1 only
    the dominant kernel is probed (a few seconds): the other ranks are already leaving the process group."""
    if world > 1:
        cg_rec = cgemm_roofline(dev, B)
        cg_rec["share_of_step_kernel_time"] = None
        cg_rec["chosen_by"] = ("cgemm* is the largest family of step_kernel_breakdown in the N = 1 record; the breakdown is not repeated at "
                               "world size %d (the step holds a collective, and no rank may run one alone after the closing barrier)" % world)
        rec["step_kernel_breakdown"] = {"skipped": "world size %d: a property of one rank's step, measured by the N = 1 run" % world}
        rec["roofline"] = cg_rec
        rec["n1_only"] = ["step_kernel_breakdown", "roofline_gemm_x3", "roofline_direct3x3", "roofline_fftconv", "other_configs", "cpu_baseline"]
        return
    ms3, fl3, ghz3 = conv3x3_roofline(dev, B, 3)
    ms4, fl4, _ = conv3x3_roofline(dev, B, 4)
    a3 = fl3 / (ms3 * 1e-3) / 1e12
    direct = {
        "kernel": "conv_igemm_f32 3x3 s1 512->512 + BN-stats epilogue, B=%d 16x52 (level 3): the direct fused kernel "
                  "(GDN_WINOGRAD=0, stride-2 / reflection layers, bf16 twin)" % B,
        "bound": "mfma", "achieved": round(a3, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
        "frac": round(a3 / PEAK_F32_MFMA_TFLOPS, 4), "traffic": pmc_traffic(),
        "gflop_per_launch": round(fl3 / 1e9, 2), "ms_per_launch": round(ms3, 4),
        "level4_8x26": {"achieved": round(fl4 / (ms4 * 1e-3) / 1e12, 2),
                        "frac": round(fl4 / (ms4 * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4),
                        "gflop_per_launch": round(fl4 / 1e9, 2), "ms_per_launch": round(ms4, 4)},
    }
    at_clock(direct, ghz3)
    # dominant kernel of the step: the per-bin GEMMs of the Winograd layers, since round 3 executed as bf16 x 3 split
    # products on the bf16 matrix pipe (csrc/gemm_x3.hip: six bf16 MFMA products per fp32 product)
    ms_g, fl_g, ms_l, fl_l, ms_x, fl_x, ghz_x = wino_roofline(dev, B)
    ax = fl_x / (ms_x * 1e-3) / 1e12                   # algorithmic (fp32) TFLOP/s
    ag = fl_g / (ms_g * 1e-3) / 1e12
    x3_rec = {
        "kernel": "gemm_x3_nt_kernel: the 36 per-bin fp32 GEMMs [%d x 512] x [512 x 512] of the Winograd F(4x4,3x3) 3x3 s1 "
                  "512->512 layer, B=%d 16x52 (level 3), as bf16 x 3 split products (6 bf16 MFMA products per fp32 "
                  "product, fp32 accumulate)" % (B * 4 * 13, B),
        "bound": "mfma", "unit": "TFLOP/s",
        "achieved": round(ax, 2), "peak": round(PEAK_BF16_MFMA_TFLOPS / 6.0, 1), "frac": round(6.0 * ax / PEAK_BF16_MFMA_TFLOPS, 4),
        "note": "achieved = ALGORITHMIC fp32 FLOPs (2 M N K per bin) / time; peak = what the pipe the kernel runs on can "
                "deliver of them: the dense bf16 MFMA peak (2500) / 6 products.  frac is therefore also executed bf16 "
                "FLOPs / bf16 peak.  Against the fp32 MFMA instruction this kernel replaces (157.3 TFLOP/s peak) the "
                "same figure is frac_of_fp32_mfma_peak",
        "executed_bf16_tflops": round(6.0 * ax, 1), "bf16_peak": PEAK_BF16_MFMA_TFLOPS,
        "frac_of_fp32_mfma_peak": round(ax / PEAK_F32_MFMA_TFLOPS, 4),
        "traffic": pmc_traffic("r04_gemm_x3_pmc.json"),
        "gflop_per_launch": round(fl_x / 1e9, 2), "ms_per_launch": round(ms_x, 4),
        "sustained_pipe_note": "with operands that are not constant the matrix pipe at full issue rate runs at 1.90-1.97 GHz "
                               "on this chip (tests/diag/mfma_rate.hip, profiles/r04d_mfma_rate.txt: 1914-1965 TFLOP/s for a "
                               "loop of nothing but v_mfma_f32_32x32x16_bf16): 0.78 of the 2.5 PF this record prices against",
        "fp32_mfma_kernel": {"kernel": "wino_gemm_kernel<64,64> on the F(2x2,3x3) shape, 16 x [4160 x 512] x [512 x 512] (round 2's dominant kernel; GDN_X3=0)", "ms_per_launch": round(ms_g, 4),
                             "achieved": round(ag, 2), "peak": PEAK_F32_MFMA_TFLOPS, "frac": round(ag / PEAK_F32_MFMA_TFLOPS, 4),
                             "traffic": pmc_traffic("r02_wino_gemm_pmc.json")},
        "layer_forward": {"ms": round(ms_l, 4), "direct_conv_gflop": round(fl_l / 1e9, 2),
                          "direct_equiv_tflops": round(fl_l / (ms_l * 1e-3) / 1e12, 2),
                          "note": "whole layer forward (transforms + GEMMs + BN-stats epilogue) counted in the direct "
                                  "convolution's FLOPs (SURVEY 8d unit, 78.5 GFLOP): 2.25x fewer multiplies are executed"},
    }
    at_clock(x3_rec, ghz_x)
    cg_rec = cgemm_roofline(dev, B)
    # which of the two is THE roofline record is decided by the measured step: the larger of the two GEMM families by share
    # of the step's kernel time over ALL symbols (torch.profiler over two steps after the timed region); the other one
    # keeps its own key, and the record says which single symbol is the step's largest.
    brk = step_kernel_breakdown(step)
    rec["step_kernel_breakdown"] = brk
    fams = brk.get("families", {})
    share = {"cgemm": float(fams.get("cgemm", 0.0)), "gemm_x3": float(fams.get("gemm_x3", 0.0))}
    measured = bool(fams)
    dominant = "cgemm" if share["cgemm"] >= share["gemm_x3"] else "gemm_x3"
    for fam, rr in (("cgemm", cg_rec), ("gemm_x3", x3_rec)):
        rr["share_of_step_kernel_time"] = round(share[fam], 4) if measured else None
    rec["roofline"] = cg_rec if dominant == "cgemm" else x3_rec
    if measured:
        top_fam = next(iter(fams))
        rec["roofline"]["chosen_by"] = ("the larger of the two GEMM families of step_kernel_breakdown over all %d symbols (cgemm* %.3f vs "
                                        "gemm_x3* %.3f of the kernel time); largest single symbol of the step: %s; largest family: "
                                        "%s (%.3f)" % (brk.get("symbols", 0), share["cgemm"], share["gemm_x3"], brk.get("top_symbol"),
                                                       top_fam, fams[top_fam]))
    else:
        rec["roofline"]["chosen_by"] = ("not measured in this run (%s): cgemm* is the largest family of the N = 1 records"
                                        % (brk.get("skipped") or brk.get("error")))
    rec["roofline_gemm_x3" if dominant == "cgemm" else "roofline_cgemm"] = x3_rec if dominant == "cgemm" else cg_rec
    rec["roofline_direct3x3"] = direct
    # second-largest share of the step: the frequency-domain layers, HBM-bound
    rec["roofline_fftconv"] = fftconv_roofline(dev, B)


def flush_c_stdio():
    """RCCL prints its version banner to C stdout, which is block-buffered when stdout is a pipe or a file and would
    otherwise be flushed at exit -- AFTER the JSON line.  Flushing it here keeps the JSON line the last line of stdout."""
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except OSError:
        pass
    sys.stdout.flush()


DUMP_BYTES = 60 * 2 ** 20         # --dump-outputs: all arrays together stay under 64 MB (npy headers included)


def dump_outputs(dirname, arrays, cap=DUMP_BYTES, seed=0):
    """--dump-outputs: each tensor of `arrays` (name -> tensor) as DIR/<name>.npy, float64 kept, everything else as float32.
    The arrays are taken smallest first and each gets an equal share of what is left of `cap`; one larger than its share is
    written as a fixed sample instead (flattened, `share` elements at sorted indices drawn from a generator seeded with
    `seed`: the same indices in every run for the same size).  Returns {name: [elements written, elements of the array]}."""
    import numpy as np
    d = pathlib.Path(dirname)
    d.mkdir(parents=True, exist_ok=True)
    items = sorted(((name, t.detach()) for name, t in arrays.items()), key=lambda kv: kv[1].numel())
    left, done = cap, {}
    for i, (name, t) in enumerate(items):
        t = t.double() if t.dtype == torch.float64 else t.float()
        share = left // (len(items) - i) // t.element_size()
        n = t.numel()
        if n > share:
            idx = torch.randint(0, n, (share,), generator=torch.Generator().manual_seed(seed)).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        a = t.contiguous().cpu().numpy()
        np.save(d / (name + ".npy"), a)
        left -= a.nbytes
        done[name] = [int(a.size), int(n)]
    return done


def train_outputs(keep, loss):
    """What a caller of the training step has after its last step: the loss, the model's output (the depth map), and the
    model's state (parameters after Adam, BatchNorm running statistics; every floating tensor of state_dict() in its order,
    flattened into one vector)."""
    state = [v.detach().reshape(-1).float() for v in keep["model"].state_dict().values() if v.is_floating_point()]
    return {"loss": loss.detach().reshape(1), "depth": keep["out"], "state": torch.cat(state)}


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        r = step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, r


def other_configs(dev, B, depth, rgb, sparse):
    """BASELINE configs[2] and [4] (and RtoD in fp32) measured in the SAME process right after the headline workload, a few
    steps each, so every number of DESIGN.md 5 is driver-run rather than a builder's claim.  N = 1, rank 0 only."""
    import gc
    out = {}
    for key, mode, dtype, fast in (("rtod_fp32", "RtoD", "fp32", False), ("rtod_bf16", "RtoD", "bf16", False),
                                   ("dtod_bf16", "DtoD", "bf16", False),
                                   # what `GDN_main.py --mode RtoD` runs by default: the guide's four features from ONE batched
                                   # encoder-only pass (bit-identical to the reference's two full forwards, whose decoder output
                                   # is discarded -- trainer.guide_latent_loss); the lines above run the guide like the reference
                                   ("rtod_fp32_encoder_only_guide", "RtoD", "fp32", True),
                                   ("rtod_bf16_encoder_only_guide", "RtoD", "bf16", True)):
        try:
            torch.manual_seed(0)
            step, _ = make_train_step(mode, dtype, dev, (depth, rgb, sparse), fast_guide=fast)
            ms, _ = timed(step, 6, 3)
            out[key] = {"workload": "%s training step, batch %d, 128x416, %s%s%s" % (
                mode, B, dtype, ", BASELINE configs[2]" if key == "rtod_bf16" else "",
                ", guide features from one encoder-only pass (trainer default; same values)" if fast else ""),
                "ms_per_step": round(ms, 3), "value": round(B / ms * 1e3, 2), "unit": "images/s", "steps": 6, "warmup": 3}
            del step
        except Exception as e:  # noqa: BLE001
            out[key] = {"error": "%s: %s" % (type(e).__name__, e)}
        gc.collect()
        torch.cuda.empty_cache()
    try:
        out["roofline_rtod_bf16"] = ring_roofline(dev, B)
    except Exception as e:  # noqa: BLE001
        out["roofline_rtod_bf16"] = {"error": "%s: %s" % (type(e).__name__, e)}
    try:
        out["roofline_wgrad_ring_bf16"] = wgrad_ring_roofline(dev, B)
    except Exception as e:  # noqa: BLE001
        out["roofline_wgrad_ring_bf16"] = {"error": "%s: %s" % (type(e).__name__, e)}
    for key, dt in (("infer_b64_graph", "fp32"), ("infer_b64_graph_bf16", "bf16")):
        try:
            ms, chk = infer_measure(dev, 64, dt, 3, 1, graph=True)
            out[key] = {"workload": "legacy AutoEncoder eval forward, batch 64, 256x832, %s, hipGraph replay, "
                                    "BASELINE configs[4]" % dt, "ms_per_step": round(ms, 3),
                        "value": round(64 / ms * 1e3, 2), "unit": "images/s", "steps": 3, "warmup": 1,
                        "out_checksum": round(chk, 6)}
        except Exception as e:  # noqa: BLE001
            out[key] = {"error": "%s: %s" % (type(e).__name__, e)}
        gc.collect()
        torch.cuda.empty_cache()
    return out


def infer_measure(dev, B, dtype, steps, warmup, graph=True, seed=0):
    import gdn_amd.AE_model_unet as M
    H, W = 256, 832
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):          # the ctor prints '- norm : Batch' like the reference's
        model = M.AutoEncoder(height=H, width=W).to(dev).eval().compute_dtype(dtype)
    x = (torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            out = model(x, istrain=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = None
    if graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = model(x, istrain=False)

    def step():
        if g is not None:
            g.replay()
            return out
        return model(x, istrain=False)

    ms, o = timed(step, steps, warmup)
    return ms, float(o.double().abs().mean().item())


def self_launch(args, argv):
    """`python bench.py --gpus N` (N > 1) as a plain command: start N fresh child processes of this script, one per GPU,
    BEFORE anything here touches the GPU (counting devices does not), wait, forward rank 0's stdout (its last line is the
    JSON record) and return the first non-zero child exit code."""
    from gdn_amd import distributed as D
    n = args.gpus
    single = os.environ.get("GDN_SINGLE_DEVICE") == "1"          # test hook: every rank on GPU 0 (gloo backend)
    if args.selftest_launch:
        devices = [None] * n
    else:
        have = torch.cuda.device_count()
        need = 1 if single else n
        if have < need:
            print("bench.py: --gpus %d asked for but %d GPU(s) are visible on this machine (HIP_VISIBLE_DEVICES=%s); "
                  "nothing was launched" % (n, have, os.environ.get("HIP_VISIBLE_DEVICES")), file=sys.stderr)
            return 2
        devices = [None] * n if single else list(range(n))
    # bounded: a rank stuck in a collective must end as rc 124 with whatever rank 0 printed, not as a hung driver run
    limit = float(os.environ.get("GDN_LAUNCH_TIMEOUT_S") or 1500.0)
    rc, text = D.launch_ranks(argv, devices, script=str(pathlib.Path(__file__).resolve()), capture_rank0=True, timeout=limit)
    sys.stdout.write(text)
    sys.stdout.flush()
    if rc != 0:
        print("bench.py: a rank exited with code %d%s" % (rc, " (the %.0f s launch limit, GDN_LAUNCH_TIMEOUT_S)" % limit if rc == 124 else ""),
              file=sys.stderr)
    return rc


def ops_x3():
    """Whether the Winograd per-bin GEMMs run as bf16 x 3 split products in this process (ranks that share a GPU switch it off)."""
    from gdn_amd import ops
    return ops.x3_enabled()


def dist_info():
    """(ranks, backend) of the process group the gradient all-reduce runs on ("nccl" is RCCL on ROCm)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), str(dist.get_backend())
    return 1, None


def launch_selftest(args):
    """--selftest-launch: the rank plumbing of a self-launched job without any GPU work (CPU test of the launcher: gloo,
    world size 2): join the group, all-reduce a token, rank 0 prints a record that is labelled as no measurement."""
    from gdn_amd import distributed as D
    import torch.distributed as dist
    rank, local_rank, world = D.init(backend=os.environ.get("GDN_DIST_BACKEND") or "gloo")
    if world != args.gpus:
        print("bench.py: --gpus %d but WORLD_SIZE is %d" % (args.gpus, world), file=sys.stderr)
        if dist.is_initialized():
            dist.destroy_process_group()
        return 2
    t = torch.tensor([float(rank + 1)])
    if world > 1:
        dist.all_reduce(t)
        dist.barrier()
    print("rank %d of %d up (selftest)" % (rank, world), file=sys.stderr)
    flush_c_stdio()
    if rank == 0:
        ranks, backend = dist_info()
        print(json.dumps({"metric": "launch selftest (no GPU work, not a measurement)", "value": None, "unit": None,
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "rccl_ranks": ranks,
                          "dist_backend": backend, "token_sum": float(t.item()),
                          "spawned": os.environ.get("GDN_SPAWNED") == "1"}), flush=True)
    if dist.is_initialized():
        dist.destroy_process_group()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=20, help="images per GPU")
    ap.add_argument("--mode", default="DtoD", choices=["DtoD", "RtoD", "infer"])
    ap.add_argument("--no-graph", action="store_true", help="infer mode: launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--fast-guide", action="store_true",
                    help="RtoD: one batched encoder-only guide pass (identical features) instead of the reference's "
                         "two full guide forwards")
    ap.add_argument("--graph", action="store_true",
                    help="capture the whole training step (forward, losses, backward, capturable fused Adam) in one hipGraph "
                         "and replay it (single GPU; the RCCL all-reduce is not captured)")
    ap.add_argument("--latent-grad", action="store_true",
                    help="RtoD: back-propagate the latent loss through the frozen guide (--latent_grad of GDN_main)")
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"],
                    help="storage dtype of activations/MFMA operands; bf16 = BASELINE configs[2] (fp32 accumulate, fp32 "
                         "master weights/BN statistics/losses/Adam). The headline line is fp32 DtoD.")
    ap.add_argument("--no-overlap", action="store_true",
                    help="data parallel: one all-reduce of the whole gradient arena after backward instead of the bucketed "
                         "reduction overlapped with it (= GDN_OVERLAP_ALLREDUCE=0), to read a scaling curve against")
    ap.add_argument("--full", action="store_true",
                    help="after the headline line's own measurement, also run everything else the record can carry: roofline "
                         "probes and the step's kernel breakdown, gpu_state, mfma_util, other_configs, cpu_baseline")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last step computed as DIR/<name>.npy (float32 / float64, under "
                         "64 MB in all; a fixed, seeded sample of an array that does not fit)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave cpu_baseline out")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: leave the roofline records out")
    ap.add_argument("--selftest-launch", action="store_true", help=argparse.SUPPRESS)   # CPU test of the self-launcher
    ap.add_argument("--no-other-configs", action="store_true",
                    help="with --full: skip the short RtoD fp32 / RtoD bf16 / inference measurements appended as other_configs "
                         "(N=1 only)")
    args = ap.parse_args()
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")

    if args.no_overlap:
        os.environ["GDN_OVERLAP_ALLREDUCE"] = "0"        # (inherited by self-launched ranks)
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        # one command, N GPUs: this process becomes the launcher and never touches the GPU
        return self_launch(args, sys.argv[1:])
    if args.selftest_launch:
        return launch_selftest(args)

    from gdn_amd import distributed as D
    from gdn_amd.synthetic import synthetic_batch

    if args.mode == "infer":
        return infer_main(args)
    rank, local_rank, world = D.init()
    if world != args.gpus:
        # a --gpus that the launcher did not honour would report one GPU's throughput as N GPUs': refuse
        print("bench.py: --gpus %d but the launcher environment has WORLD_SIZE %d (rank %d); start it as "
              "`python bench.py --gpus N` or under torch.distributed.run with --nproc-per-node N" % (args.gpus, world, rank),
              file=sys.stderr)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()
        return 2
    dev = torch.device("cuda", 0 if os.environ.get("GDN_SINGLE_DEVICE") == "1" else local_rank)   # (test hook: all ranks on one GPU)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    B = args.batch
    depth, rgb, sparse = synthetic_batch(B, 128, 416, seed=rank, device=dev)

    keep = {} if args.dump_outputs and rank == 0 else None
    step, graphed = make_train_step(args.mode, args.dtype, dev, (depth, rgb, sparse), fast_guide=args.fast_guide,
                                    latent_grad=args.latent_grad, use_graph=args.graph and world == 1, keep=keep)

    def barrier():
        if world > 1:
            torch.distributed.barrier()

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    barrier()
    if D.active():
        D.stats_begin()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    dt_own = time.perf_counter() - t0          # this rank's own loop, before it waits for the others
    barrier()
    dt = time.perf_counter() - t0
    dp = None
    if D.active():
        # a multi-rank record that explains itself: the spread of the ranks' own step times, what the gradient all-reduce
        # cost beyond backward (time the compute stream stood still for it), how it was bucketed, which switches were on
        dp = D.stats_report(args.steps)
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
        own = [torch.zeros(2, device=dev, dtype=torch.float64) for _ in range(world)]
        torch.distributed.all_gather(own, torch.tensor([dt_own / args.steps * 1e3,
                                                        dp["allreduce_exposed_ms"] if dp["allreduce_exposed_ms"] is not None
                                                        else dp["allreduce_host_wait_ms"]], device=dev, dtype=torch.float64))
        per_rank = sorted(float(o[0].item()) for o in own)
        dp["step_ms_per_rank"] = {"min": round(per_rank[0], 3), "median": round(per_rank[len(per_rank) // 2], 3),
                                  "max": round(per_rank[-1], 3), "all": [round(float(o[0].item()), 3) for o in own]}
        dp["allreduce_exposed_ms_per_rank"] = [round(float(o[1].item()), 4) for o in own]
    final_loss = float(loss.item())
    flush_c_stdio()                  # every rank: library banners out before rank 0 prints the result line
    barrier()
    # ---- the LAST collective of the job.  Ranks != 0 go straight to destroy_process_group(); nothing rank 0 does from here on
    # ---- may involve another rank (no training step at world > 1: it holds the gradient all-reduce).
    t_tail = time.perf_counter()

    if rank == 0:
        # first, before anything below runs more steps on this model: what the timed path computed in its last step
        dumped = dump_outputs(args.dump_outputs, train_outputs(keep, loss)) if keep is not None else None
        keep = None
        ms = dt / args.steps * 1e3
        value = B * world * args.steps / dt
        gflop_img = DTOD_TRAIN_GFLOP_PER_IMG if args.mode == "DtoD" else (1595.2 if args.fast_guide else 1922.6)
        rec = {
            "metric": "training images/sec at 128x416 batch=20",
            "value": round(value, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32" if args.dtype == "fp32" else "bf16", "data": "synthetic",
            "rccl_ranks": dist_info()[0], "dist_backend": dist_info()[1],
            "data_parallel": dp,
            "config": {"workload": "%s training step (fwd + losses + bwd + fused Adam), batch %d per GPU, 128x416, "
                                   "%s, BASELINE configs[%d]" % (args.mode, B, args.dtype, 1 if args.mode == "DtoD" else (3 if world > 1 else 2)),
                       "global_batch": B * world, "parallelism": "dp%d" % world,
                       "launch": "hipGraph replay of the whole step" if graphed is not None else "eager",
                       "direct_conv_equiv_tflops_per_gpu": round(gflop_img * B * args.steps / dt / 1e3, 2),
                       "direct_conv_equiv_note": "a THROUGHPUT label, not a utilisation: FLOPs the reference's direct "
                                                 "convolutions would need / time.  The fp32 path executes 12-29x fewer "
                                                 "multiplies on the k>=5 layers (frequency domain) and 2.25x fewer on the "
                                                 "3x3 ones (Winograd), so it exceeds the 157 TFLOP/s MFMA peak; the "
                                                 "utilisation figures are roofline.frac and mfma_util",
                       "x3": bool(ops_x3()), "shared_gpu_ranks": D.SHARED_GPU_RANKS,
                       "final_loss": round(final_loss, 6),
                       "parity_bar": "fp32, tests/test_hip_model.py at this batch and size: depth map max|err| <= 1e-3 ABSOLUTE on its (-1, 1) range "
                                     "and rms <= 6e-5 against the CPU oracle (north_star's '1e-3 relative' read against the map's unit range); "
                                     "rms(HIP - fp64) <= 1.1 x rms(oracle fp32 - fp64); tensors 1e-3 relative + 1e-4 of max; "
                                     "gradients 2e-2 relative L2; bf16: <= 1.25 x the bf16 emulation's own drift"},
        }
        if dumped is not None:
            rec["outputs_dumped"] = dumped
        if args.full:
            if not args.no_roofline and args.dtype == "fp32":
                try:
                    roofline_records(rec, dev, B, step, world)
                except Exception as e:  # noqa: BLE001 -- a failed probe must not lose the measured line
                    rec["roofline_error"] = "%s: %s" % (type(e).__name__, e)
            rec["gpu_state"] = gpu_state()
            if args.dtype == "fp32" and args.mode == "DtoD":
                rec["mfma_util"] = step_mfma_util()
            if world == 1 and not args.no_other_configs and args.mode == "DtoD" and args.dtype == "fp32" and B == 20:
                del step
                torch.cuda.empty_cache()
                rec["other_configs"] = other_configs(dev, B, depth, rgb, sparse)
            if world == 1 and not args.no_cpu_baseline:
                rec["cpu_baseline"] = cpu_baseline(B)
        rec["tail_s"] = round(time.perf_counter() - t_tail, 2)      # rank 0's time between the closing barrier and this line
        flush_c_stdio()
        print(json.dumps(rec), flush=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main() or 0)
