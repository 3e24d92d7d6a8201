"""--loss silog end to end through GDN_main.run, fp32 and bf16: it trains, its first output_loss is the
float64 restatement's on that batch, --loss berhu is the run without the flag, and the SILog run is bit for bit itself under
--graph and across a stop and --resume; it runs under --accum_steps, the gradient guard and the weight average, and a step
launches no torch kernel between its first and its last library kernel.

DtoD runs at the harness shape of tests/test_hip_lr_schedule.py (--synthetic, 16 x 32, batch 2, --epoch_size 3 --epochs 2).
RtoD runs at 32 x 64, the shape tests/test_hip_graph_train.py and tests/test_hip_resume.py train AutoEncoder_2 at: at 16 x 32
its bottleneck is one row high, which its reflection padding of 1 does not admit.

A checkpoint of these networks is 65 MB whatever the image size and the runs below write some eighty of them, so a run's
directory is deleted as soon as its files are read, and what is kept of a file is a SHA-256 digest per tensor (plus whether
its weights are finite): the module never holds more than one run on disk (two while a stopped run waits to be resumed)."""
import hashlib
import os
import shutil

import numpy as np
import pytest
import torch

import pointwise_fp64 as P
import silog_fp64 as R

pytestmark = pytest.mark.gpu

SHAPE = {"DtoD": (16, 32), "RtoD": (32, 64)}
CASES = [("DtoD", "fp32"), ("DtoD", "bf16"), ("RtoD", "fp32"), ("RtoD", "bf16")]
IDS = ["%s-%s" % c for c in CASES]
SILOG = ["--loss", "silog"]
_RUNS, _FIRST, _GUARD = {}, {}, {}        # per (mode, dtype, tag): the files' digests, the first loss call, guard_stats()


class _Stop(Exception):
    pass


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("silog_train")


def _run(root, tag, mode, dtype, extra, stop_after_first_state=False, loaders=None, evaluate=True):
    """GDN_main.run in `root`/<mode>_<dtype>_<tag> (cached): {file name: _digest of every .pkl written}; _GUARD keeps the
    run's guard_stats() (None without a guard) and _FIRST (outputs, depths, sparse, output_loss) of its first loss call (an
    eager step under --graph too).  The directory is deleted before the call returns.
    stop_after_first_state: the run dies right after its first train_state.pt is on disk, as a kill would end it; its
    directory stays (the caller resumes from it and deletes it).
    loaders: (train_loader, val_loader) handed to run() in place of the synthetic ones it builds."""
    from gdn_amd import GDN_main, option
    from gdn_amd import trainer as T
    from gdn_amd import utils as U
    key = (mode, dtype, tag)
    if key in _RUNS:
        return _RUNS[key]
    spy, first_terms = [], []
    H, W = SHAPE[mode]
    where = root / ("%s_%s_%s" % (mode, dtype, tag))
    where.mkdir(parents=True, exist_ok=True)
    argv = ["synthetic", "--synthetic", "--mode", mode, "--height", str(H), "--width", str(W), "--batch_size", "2",
            "--epoch_size", "3", "--epochs", "2", "--gpu_num", "0", "--dtype", dtype, "--model_dir", str(where / "no_guide.pkl")]
    if evaluate:
        argv.append("-e")
    cwd, save, make, dtod, rtod = os.getcwd(), T.save_training_state, GDN_main._make_optimizer, U.dtod_loss, U.rtod_pixel_loss

    def save_and_stop(*a, **k):
        save(*a, **k)
        raise _Stop()

    def make_and_show(model, args):
        opt = make(model, args)
        spy.append(opt)
        return opt

    def dtod_and_show(outputs, depths, sparse=None, *a, **k):
        terms = dtod(outputs, depths, sparse, *a, **k)
        if not first_terms:
            first_terms.append((outputs.detach().float().cpu(), depths.cpu(), sparse.cpu(), terms[1].cpu()))
        return terms

    def rtod_and_show(outputs, depths, rgb, sparse=None, *a, **k):
        terms = rtod(outputs, depths, rgb, sparse, *a, **k)
        if not first_terms:
            first_terms.append((outputs.detach().float().cpu(), depths.cpu(), sparse.cpu(), terms[1].cpu()))
        return terms
    os.chdir(where)
    try:
        if stop_after_first_state:
            T.save_training_state = save_and_stop
        GDN_main._make_optimizer = make_and_show
        U.dtod_loss, U.rtod_pixel_loss = dtod_and_show, rtod_and_show
        args = option.parse_args(argv + list(extra))
        if loaders is None:
            GDN_main.run(args)
        else:
            GDN_main.run(args, train_loader=loaders[0], val_loader=loaders[1])
        assert not stop_after_first_state, "the run wrote no training state"
    except _Stop:
        pass
    except BaseException:
        os.chdir(cwd)
        shutil.rmtree(where, ignore_errors=True)             # a failed run leaves nothing on disk either
        raise
    finally:
        T.save_training_state, GDN_main._make_optimizer, U.dtod_loss, U.rtod_pixel_loss = save, make, dtod, rtod
        os.chdir(cwd)
    torch.cuda.synchronize()
    _GUARD[key], _FIRST[key] = spy[0].guard_stats() if spy[0].guarded else None, first_terms[0]
    _RUNS[key] = {p.name: _digest(torch.load(p, map_location="cpu")) for p in sorted(where.rglob("*.pkl"))}
    del spy[:]
    if not stop_after_first_state:
        shutil.rmtree(where)
    return _RUNS[key]


def _digest(sd):
    """{key: (dtype, shape, SHA-256 of the tensor's bytes)} of a state dict, and under None whether every floating-point
    tensor that is not a BatchNorm running statistic is finite."""
    out = {k: (str(v.dtype), tuple(v.shape), hashlib.sha256(v.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest())
           for k, v in sd.items()}
    out[None] = all(bool(torch.isfinite(v).all()) for k, v in sd.items() if v.is_floating_point() and "running_" not in k)
    return out


def _same_files(a, b, what):
    assert sorted(a) == sorted(b) and a, (what, sorted(a), sorted(b))
    for name in a:
        assert list(a[name]) == list(b[name])
        for k in a[name]:
            assert a[name][k] == b[name][k], (what, name, k)


def _stems(files):
    return sorted(k.split("_loss_")[0] for k in files)


@pytest.mark.parametrize("mode,dtype", CASES, ids=IDS)
def test_silog_trains_and_its_first_loss_is_the_restatement(gpu, root, mode, dtype):
    """The SILog run writes the checkpoints the BerHu run writes, with other weights; the output_loss of its first step --
    what the progress line prints in that column -- is the float64 restatement on that step's prediction within the loss
    bar of tests/test_hip_silog.py, 1 ulp of float32."""
    silog = _run(root, "silog", mode, dtype, SILOG)
    plain = _run(root, "plain", mode, dtype, [])
    assert _stems(silog) == _stems(plain) and len(silog) == (2 if mode == "DtoD" else 1)
    a, b = (sorted(r.items())[0][1] for r in (silog, plain))
    assert list(a) == list(b) and any(a[k] != b[k] for k in a if k is not None)
    assert a[None] and b[None]                                     # finite weights
    outputs, depths, sparse, output_loss = _FIRST[(mode, dtype, "silog")]
    ref, _, stats = R.silog(outputs, depths, None, None, 0.85, 10.0, 0.0125)
    u = float(P.ulps_off(output_loss, np.asarray(ref), P.F32))
    print("FIGURE %s %s first output_loss %.9g, float64 %.17g (n = %d): %.2f ulp" % (mode, dtype, float(output_loss), ref, stats[0], u))
    assert ref > 0 and stats[0] > 0 and u <= 1.0


@pytest.mark.parametrize("mode,dtype", CASES, ids=IDS)
def test_lidar_mask_trains_on_the_box(gpu, root, mode, dtype):
    """--silog_mask lidar: the first output_loss is the restatement over the pixels of the Garg box with a LiDAR return."""
    lidar = _run(root, "lidar", mode, dtype, SILOG + ["--silog_mask", "lidar", "--silog_lambda", "0.5", "--silog_weight", "2"])
    dense = _run(root, "silog", mode, dtype, SILOG)
    a, b = (sorted(r.items())[0][1] for r in (lidar, dense))
    assert any(a[k] != b[k] for k in a if k is not None) and a[None]
    outputs, depths, sparse, output_loss = _FIRST[(mode, dtype, "lidar")]
    H, W = SHAPE[mode]
    ref, _, stats = R.silog(outputs, depths, sparse, P.crop_box_kitti(H, W), 0.5, 2.0, 0.0125)
    u = float(P.ulps_off(output_loss, np.asarray(ref), P.F32))
    print("FIGURE %s %s lidar first output_loss %.9g, float64 %.17g (n = %d): %.2f ulp" % (mode, dtype, float(output_loss), ref, stats[0], u))
    assert stats[0] >= 2 and ref > 0 and u <= 1.0


@pytest.mark.parametrize("mode,dtype", CASES, ids=IDS)
def test_loss_berhu_is_the_run_without_the_flag(gpu, root, mode, dtype):
    _same_files(_run(root, "plain", mode, dtype, []), _run(root, "berhu", mode, dtype, ["--loss", "berhu"]), "--loss berhu")


@pytest.mark.parametrize("mode,dtype", CASES, ids=IDS)
def test_silog_graph_is_bitwise(gpu, root, mode, dtype):
    _same_files(_run(root, "silog", mode, dtype, SILOG),
                _run(root, "graph", mode, dtype, SILOG + ["--graph", "--graph_warmup", "2"]), "--graph")


@pytest.mark.parametrize("mode,dtype", CASES, ids=IDS)
def test_silog_resume_is_bitwise(gpu, root, mode, dtype):
    """Stopped right after the state that falls due with step 3, the end of epoch 1, and resumed with the flag repeated (it
    is not stored): together the files of the uninterrupted run."""
    full = _run(root, "silog", mode, dtype, SILOG)
    stopped = _run(root, "stopped", mode, dtype, SILOG + ["--save_state_every", "3"], stop_after_first_state=True)
    where = root / ("%s_%s_stopped" % (mode, dtype))
    try:
        (state,) = sorted(where.rglob("train_state.pt"))
        saved = torch.load(state, map_location="cpu", weights_only=True)
        assert saved["step"] == 3 and "loss" not in saved and "pixel" not in saved
        del saved
        resumed = _run(root, "resumed", mode, dtype, SILOG + ["--save_state_every", "3", "--resume", str(state)])
    finally:
        shutil.rmtree(where, ignore_errors=True)
    _same_files({k: v for k, v in full.items() if k not in stopped}, resumed, "--resume")
    assert resumed
    if stopped:
        _same_files({k: v for k, v in full.items() if k in stopped}, stopped, "epoch 1")


def _poisoned_loaders(gpu, mode):
    """Three distinct synthetic batches per epoch; the second one's network input holds one NaN."""
    from gdn_amd.synthetic import SyntheticLoader
    H, W = SHAPE[mode]
    train = SyntheticLoader(2, 3, H, W, seed=0, device=gpu, distinct=3)
    gt, rgb, sparse = train.batches[1]
    (gt if mode == "DtoD" else rgb)[0, 0, 3, 5] = float("nan")
    return train, SyntheticLoader(2, 2, H, W, seed=1000, device=gpu)


@pytest.mark.parametrize("mode,dtype", CASES, ids=IDS)
def test_silog_with_accumulation_guard_and_average(gpu, root, mode, dtype):
    """--accum_steps 2 --clip_grad_norm 1 --skip_nonfinite --ema_decay 0.9 on a loader whose second batch of three holds a
    NaN: the SILog value of that batch is non-finite, so is the gradient of the group it is in, and the guard counts the
    update as skipped -- one of the two updates of each epoch; the weights stay finite."""
    files = _run(root, "combo", mode, dtype, SILOG + ["--accum_steps", "2", "--clip_grad_norm", "1", "--skip_nonfinite",
                                                      "--ema_decay", "0.9"], loaders=_poisoned_loaders(gpu, mode), evaluate=False)
    gs = _GUARD[(mode, dtype, "combo")]
    print("FIGURE %s %s guard %r" % (mode, dtype, gs))
    assert gs["steps"] == 4 and gs["skipped"] == 2
    assert sum(n.endswith("_ema.pkl") for n in files) == len(files) // 2 and files
    assert all(sd[None] for sd in files.values())                  # finite weights, averaged ones included


def test_skip_nonfinite_counts_a_nan_batch(gpu, root):
    """Without accumulation: the poisoned batch is the second step of both epochs, 2 of 6 steps are skipped."""
    _run(root, "skip", "DtoD", "fp32", SILOG + ["--skip_nonfinite"], loaders=_poisoned_loaders(gpu, "DtoD"), evaluate=False)
    gs = _GUARD[("DtoD", "fp32", "skip")]
    assert gs["steps"] == 6 and gs["skipped"] == 2


# ---- no torch kernel inside the step ---------------------------------------------------------------------------------------
TORCH_KERNEL_MARKS = ("at::", "c10::", "Memcpy", "Memset", "memcpy", "memset", "Cijk_", "miopen", "rocblas", "hipblas")


def _kernel_names(step):
    """The device activities of one call of step(), by start time (torch.profiler, the source bench.py's breakdown reads)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    return [e.name for e in sorted(evs, key=lambda e: e.time_range.start)]


@pytest.mark.parametrize("mode", ["DtoD", "RtoD"])
def test_a_silog_step_launches_no_torch_kernel(gpu, mode):
    """One training step as the loops run it (forward, the losses with the SILog spec, zero_grad, backward with the cached
    seed, fused Adam), profiled after two warm-up steps: between the first and the last kernel of the library every device
    activity is a kernel of the library -- none of torch's (at:: / c10:: symbols), no copy, no fill, no vendor-library kernel.
    The BerHu step is held to the same and is the control: the two differ only in the loss kernels' names."""
    import gdn_amd.AE_model_unet as M
    from gdn_amd import utils as U
    from gdn_amd.optim import Adam
    from gdn_amd.synthetic import synthetic_batch
    H, W = SHAPE[mode]
    depth, rgb, sparse = synthetic_batch(2, H, W, seed=0, device=gpu)
    torch.manual_seed(4)
    net = (M.AutoEncoder_DtoD(input_dim=1, height=H, width=W) if mode == "DtoD" else M.AutoEncoder_2(input_dim=3, height=H, width=W))
    net = net.to(gpu).train()
    opt = Adam(net.parameters(), 2e-5, [0.9, 0.999], eps=1e-08, weight_decay=5e-4)
    seen = {}
    for name, pixel in (("berhu", None), ("silog", U.silog_spec()), ("silog-lidar", U.silog_spec(use_sparse=True))):
        def step():
            out = net(depth if mode == "DtoD" else rgb, istrain=False)
            if mode == "DtoD":
                terms = U.dtod_loss(out, depth, sparse, pixel=pixel)
            else:
                terms = U.rtod_pixel_loss(out, depth, rgb, sparse, pixel=pixel)
            opt.zero_grad()
            U.backward(terms[0])
            opt.step()
        step()
        step()
        names = _kernel_names(step)
        ours = [i for i, n in enumerate(names) if not any(m in n for m in TORCH_KERNEL_MARKS)]
        assert ours, names
        inside = names[ours[0]:ours[-1] + 1]
        foreign = [n for n in inside if any(m in n for m in TORCH_KERNEL_MARKS)]
        print("FIGURE %s %s: %d device activities in the step, %d inside the library's span, %d foreign" % (mode, name, len(names), len(inside), len(foreign)))
        assert not foreign, foreign
        seen[name] = inside
    assert any("silog_stats_kernel" in n for n in seen["silog"]) and any("silog_grad_kernel" in n for n in seen["silog"])
    assert not any("berhu" in n for n in seen["silog"]) and any("berhu_kernel" in n for n in seen["berhu"])
    assert len(seen["silog"]) == len(seen["berhu"]) - 1                 # three launches in place of BerHu's four
    assert len(seen["silog-lidar"]) == len(seen["silog"])
