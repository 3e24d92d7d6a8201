"""Gradient guard of the fused Adam on the GPU: the deterministic device-side gradient norm (gdn_grad_sumsq), the decision
record (gdn_grad_guard_finalize) and the guarded capturable update (gdn_adam_step_dev_guarded), from the kernels up to
optim.Adam(max_grad_norm=, skip_nonfinite=), GraphedTrainStep, state_dict() and the command line.  The float64 yardstick
is tests/grad_guard_fp64.py."""
import copy
import os
import pathlib
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import grad_guard_fp64 as R
from oracle import gdn_oracle as O
from test_hip_kernels import close

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parent.parent
U23 = 2.0 ** -23
# the sizes the issue names, one that is whole blocks x 256 x 4 plus 5, and one past the grid's cap of 1024 blocks x 4096
# elements (the only other path of the kernel: every lane then makes more than one trip of its unrolled loop)
SIZES = [1, 3, 255, 256, 257, 1023, 4099, 3_000_001, 8 * 256 * 4 + 5, 2 * 1024 * 4096 + 7]
LARGEST = sorted(SIZES)[-3:]
OFFSETS = (0, 1, 2, 3)
H, W = 32, 64


# ---------------------------------------------------------------------------------------------------------------------
def _record(gpu, sumsq=0.0, steps=0, clipped=0, skipped=0):
    raw = struct.pack(R.RECORD_FMT, sumsq, 0.0, 0.0, 0, steps, clipped, skipped)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(gpu)


def _read(rec):
    return R.unpack(rec.cpu().numpy().tobytes())


def _hyper(gpu, grad_scale=1.0):
    return torch.tensor([1e-3, 0.9, 0.999, 1e-8, 5e-4, grad_scale], dtype=torch.float32, device=gpu)


@pytest.fixture(scope="module")
def pool(gpu):
    """One seeded buffer every size and offset is a slice of: normal samples times 10**uniform(-12, 12) (host copy for the
    float64 restatement, device copy for the kernel), made once and never written."""
    rng = np.random.default_rng(20261018)
    n = max(SIZES) + max(OFFSETS)
    host = (rng.standard_normal(n) * 10.0 ** rng.uniform(-12, 12, n)).astype(np.float32)
    return host, torch.from_numpy(host).to(gpu)


def _norm32(gpu, g, max_norm=0.0, skip=False, grad_scale=1.0, halves=False):
    from gdn_amd import ops
    rec = _record(gpu)
    if halves and g.numel() > 1:
        h = g.numel() // 2
        ops.grad_sumsq(g[:h], rec)
        ops.grad_sumsq(g[h:], rec, accumulate=True)
    else:
        ops.grad_sumsq(g, rec)
    ops.grad_guard_finalize(rec, _hyper(gpu, grad_scale), max_norm, skip)
    return _read(rec)


@pytest.mark.parametrize("n", SIZES)
def test_grad_sumsq_against_float64(gpu, pool, n):
    """|norm32 - ref64| <= 2^-23 ref64 at every base alignment: the squares are exact in double, the double sum is off by at
    most n 2^-53 (< 1e-9 at the largest size), one rounding to float adds 2^-24.  The same call twice gives the same 32
    bytes; two accumulated halves meet the same bar."""
    from gdn_amd import ops
    host, dev = pool
    for off in OFFSETS:
        g = dev[off:off + n]
        assert g.data_ptr() % 16 == (dev.data_ptr() + 4 * off) % 16
        ref = R.norm64(R.sumsq(host[off:off + n]))
        got = _norm32(gpu, g)
        err = abs(float(got["norm"]) - ref) / ref
        print("n=%d offset=%d: norm32 %.9e ref64 %.9e rel err %.3e" % (n, off, float(got["norm"]), ref, err))
        assert got["skip"] == 0 and got["coef"] == np.float32(1.0) and got["steps"] == 1
        assert abs(float(got["norm"]) - ref) <= U23 * ref, (n, off, float(got["norm"]), ref)
        a, b = _record(gpu), _record(gpu)
        ops.grad_sumsq(g, a)
        ops.grad_sumsq(g, b)
        assert torch.equal(a, b) and _read(a)["sumsq"] == got["sumsq"], "not deterministic at n=%d offset=%d" % (n, off)
        two = _norm32(gpu, g, halves=True)
        assert abs(float(two["norm"]) - ref) <= U23 * ref, ("two halves", n, off, float(two["norm"]), ref)


@pytest.mark.parametrize("n", [1, 4099, 3_000_001])
def test_grad_sumsq_squares_in_double(gpu, n):
    """A single 1e30 among small values: squared in float32 it would be inf; the record stays finite and meets the bar."""
    host = np.full(n, 0.5, np.float32)
    host[n // 2] = 1e30
    got = _norm32(gpu, torch.from_numpy(host).to(gpu))
    ref = R.norm64(R.sumsq(host))
    assert np.isfinite(got["sumsq"]) and np.isfinite(got["norm"]) and got["skip"] == 0
    assert abs(float(got["norm"]) - ref) <= U23 * ref


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("n", [1] + LARGEST)
def test_nonfinite_detection(gpu, pool, n, skip):
    """NaN at the first, a middle and the last element, +Inf and -Inf: skip and coef are the restatement's, exactly."""
    host, dev = pool
    base = dev[1:1 + n].clone()                        # (an odd base: head, body and tail all exist)
    for bad in (float("nan"), float("inf"), float("-inf")):
        for pos in sorted({0, n // 2, n - 1}):
            g = base.clone()
            g[pos] = bad
            got = _norm32(gpu, g, max_norm=1.0, skip=skip)
            h = host[1:1 + n].copy()
            h[pos] = bad
            want = R.finalize(R.accumulate(R.new_record(), h), 1.0, 1.0, skip)
            assert not np.isfinite(got["sumsq"]) and not np.isfinite(got["norm"]), (n, bad, pos)
            assert got["skip"] == want["skip"] == int(skip), (n, bad, pos)
            assert got["coef"] == want["coef"] == np.float32(0.0 if skip else 1.0), (n, bad, pos)
            assert (got["steps"], got["clipped"], got["skipped"]) == (1, 0, int(skip))


@pytest.mark.parametrize("grad_scale", [1.0, 0.5, 0.125])
def test_finalize_coefficient(gpu, grad_scale):
    """coef32 within 2^-23 relative of the float64 formula for a norm above, below and equal to max_norm."""
    from gdn_amd import ops
    g = torch.tensor([3.0, 4.0, 12.0, 84.0, 0.0], device=gpu)          # norm 85 exactly
    seen = 85.0 * grad_scale
    for max_norm in (seen / 7.0, seen * 3.0, seen, 0.0):
        got = _norm32(gpu, g, max_norm=max_norm, grad_scale=grad_scale)
        want = R.coef64(seen, max_norm)
        assert got["sumsq"] == 7225.0 and got["norm"] == np.float32(seen)
        assert abs(float(got["coef"]) - want) <= U23 * want, (max_norm, float(got["coef"]), want)
        rec = R.finalize(R.accumulate(R.new_record(), g.cpu().numpy()), grad_scale, max_norm)
        assert got["coef"] == rec["coef"] and got["clipped"] == rec["clipped"]      # (equal: 1 - 1e-6 / norm, as float32)
        if max_norm != seen:
            assert got["clipped"] == (1 if 0.0 < max_norm < seen else 0)


def test_finalize_counters_over_five_steps(gpu):
    from gdn_amd import ops
    rec, want = _record(gpu), R.new_record()
    hyper = _hyper(gpu, 0.5)
    small, big = np.array([0.3, 0.4], np.float32), np.array([30.0, 40.0], np.float32)
    poison = np.array([1.0, np.inf], np.float32)
    for k, h in enumerate((big, small, poison, big, small)):          # clipped, not, skipped, clipped, not
        ops.grad_sumsq(torch.from_numpy(h).to(gpu), rec)
        ops.grad_guard_finalize(rec, hyper, 1.0, True)
        R.finalize(R.accumulate(want, h), 0.5, 1.0, True)
        got = _read(rec)
        for key in ("skip", "steps", "clipped", "skipped", "coef"):
            assert got[key] == want[key], (k, key, got, want)
        assert got["norm"] == want["norm"] or (np.isinf(got["norm"]) and np.isinf(want["norm"]))
    assert (want["steps"], want["clipped"], want["skipped"]) == (5, 2, 1)


# ---------------------------------------------------------------------------------------------------------------------
def _grads(n, steps, seed=100, scale=1.0):
    return [scale * torch.randn(n, generator=torch.Generator().manual_seed(seed + i)) for i in range(steps)]


def _loose(gpu, n, **kw):
    from gdn_amd.optim import Adam
    p = torch.nn.Parameter(torch.randn(n, generator=torch.Generator().manual_seed(1)).to(gpu))
    opt = Adam([p], 1e-3, [0.9, 0.999], eps=1e-8, weight_decay=5e-4, **kw)
    opt.grad_scale = 0.5
    return p, opt


def _snapshot(p, opt):
    st = opt.store_of(p)
    return [p.detach().clone(), st.m.clone(), st.v.clone(), st.state.clone()]


def _same(a, b, what):
    for name, x, y in zip(("p", "m", "v", "device step state"), a, b):
        assert torch.equal(x, y), "%s: %s differs" % (what, name)


@pytest.mark.parametrize("n", [1000, 4099])
def test_guarded_update_bitwise_identities(gpu, n):
    """coef == 1: bit-identical to the unguarded capturable step.  coef < 1: bit-identical to the unguarded capturable step
    run with grad_scale = float32(grad_scale * coef)."""
    grads = _grads(n, 6)
    p0, plain = _loose(gpu, n, capturable=True)
    p1, idle = _loose(gpu, n, max_grad_norm=1e6, skip_nonfinite=True)
    p2, clip = _loose(gpu, n, max_grad_norm=0.25)
    p3, ref = _loose(gpu, n, capturable=True)
    assert idle.capturable and clip.capturable
    for k, g in enumerate(grads):
        for p in (p0, p1, p2, p3):
            p.grad = g.to(gpu)
        plain.step()
        idle.step()
        _same(_snapshot(p0, plain), _snapshot(p1, idle), "step %d, clipping idle" % k)
        clip.step()
        gs = clip.guard_stats()
        want = R.finalize(R.accumulate(R.new_record(), g.numpy()), 0.5, 0.25)
        assert 0.0 < gs["coef"] < 1.0 and abs(gs["coef"] - float(want["coef"])) <= U23 * float(want["coef"])
        ref.grad_scale = float(np.float32(0.5) * np.float32(gs["coef"]))
        ref.step()
        _same(_snapshot(p2, clip), _snapshot(p3, ref), "step %d, clipping active" % k)
    assert idle.guard_stats()["clipped"] == 0 and idle.guard_stats()["steps"] == 6
    assert clip.guard_stats()["clipped"] == 6 and not torch.equal(p0, p2)


def test_skipped_step_touches_nothing(gpu):
    """An Inf written into the gradient of step 3 of 6: that step leaves p, m, v and the device step state bitwise alone, and
    the run ends bitwise where a guarded run fed only the five finite gradients ends.  Without skip_nonfinite the same Inf
    goes through, as documented."""
    n = 1000
    grads = _grads(n, 6)
    poisoned = grads[2].clone()
    poisoned[n // 3] = float("inf")
    p, opt = _loose(gpu, n, max_grad_norm=10.0, skip_nonfinite=True)
    q, five = _loose(gpu, n, max_grad_norm=10.0, skip_nonfinite=True)
    for k, g in enumerate(grads):
        p.grad = (poisoned if k == 2 else g).to(gpu)
        before = _snapshot(p, opt) if k == 2 else None
        opt.step()
        if k == 2:
            _same(before, _snapshot(p, opt), "the skipped step")
            gs = opt.guard_stats()
            assert gs["skipped"] == 1 and gs["coef"] == 0.0 and not np.isfinite(gs["norm"])
        else:
            q.grad = g.to(gpu)
            five.step()
    _same(_snapshot(p, opt), _snapshot(q, five), "after six steps, one skipped")
    assert opt.guard_stats()["steps"] == 6 and opt.guard_stats()["skipped"] == 1 and five.guard_stats()["skipped"] == 0
    assert opt.store_of(p).count(p) == 5 and bool(torch.isfinite(p).all())
    r, through = _loose(gpu, n, max_grad_norm=10.0)
    r.grad = poisoned.to(gpu)
    through.step()
    assert not bool(torch.isfinite(r).all()) and through.guard_stats()["skipped"] == 0


def test_matches_torch_clip_grad_norm_and_adam(gpu):
    """Three parameters, 10 steps whose norms straddle max_grad_norm, against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam
    on the CPU at the bar test_capturable_adam_matches_host_adam holds."""
    from gdn_amd.optim import Adam
    shapes, max_norm = [(64, 3, 3, 3), (64,), (7,)], 1.0
    gen = torch.Generator().manual_seed(3)
    init = [torch.randn(s, generator=gen) for s in shapes]
    mine = [torch.nn.Parameter(t.clone().to(gpu)) for t in init]
    theirs = [torch.nn.Parameter(t.clone()) for t in init]
    opt = Adam(mine, 1e-3, [0.9, 0.999], eps=1e-8, weight_decay=5e-4, max_grad_norm=max_norm)
    ref = torch.optim.Adam(theirs, 1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
    clipped = 0
    for k in range(10):
        scale = 0.004 if k % 2 else 0.1            # 1799 elements: norms of about 0.17 and 4.2
        for a, b in zip(mine, theirs):
            g = scale * torch.randn(b.shape, generator=gen)
            a.grad, b.grad = g.clone().to(gpu), g.clone()
        total = float(torch.nn.utils.clip_grad_norm_(theirs, max_norm))
        clipped += total > max_norm
        ref.step()
        opt.step()
        gs = opt.guard_stats()
        assert abs(gs["norm"] - total) <= 1e-5 * total and gs["clipped"] == clipped
    assert clipped == 5
    for a, b, s in zip(mine, theirs, shapes):
        close(a, b, rtol=1e-5, atol_scale=1e-6, what="guarded Adam vs torch, %s" % (s,))


# ---------------------------------------------------------------------------------------------------------------------
def _model_step(model, opt, batch):
    from gdn_amd import utils as U
    depth, _, sparse = batch
    out = model(depth, istrain=False)
    loss, _, _ = U.dtod_loss(out, depth, sparse)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss.detach()


def _model_and_opt(gpu, base, **kw):
    from gdn_amd.optim import Adam
    model = copy.deepcopy(base).to(gpu).train()
    return model, Adam(model.parameters(), 2e-4, [0.9, 0.999], eps=1e-08, weight_decay=5e-4, **kw)


@pytest.fixture(scope="module")
def base_model():
    import gdn_amd.AE_model_unet as M
    torch.manual_seed(4)
    return M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)


@pytest.fixture(scope="module")
def batches(gpu):
    return [[t.to(gpu) for t in O.synthetic_batch(2, H, W, seed=60 + i)] for i in range(6)]


def _norm_of_grads(params):
    return float(np.sqrt(sum(float(p.grad.detach().double().pow(2).sum()) for p in params if p.grad is not None)))


def test_arena_norm_and_partial_coverage(gpu, base_model, batches):
    """The one-launch path reads the whole gradient arena: the norm equals the float64 norm over the per-parameter
    gradients.  With a frozen sub-module the norm covers the parameters that have a gradient, and the frozen ones are
    bitwise untouched.  (Every parameter of this network is a whole number of alignment units, so its arena has no padding:
    test_arena_padding_contributes_nothing covers that.)"""
    model, opt = _model_and_opt(gpu, base_model, max_grad_norm=1e-3)
    _model_step(model, opt, batches[0])
    ref = _norm_of_grads(model.parameters())
    gs = opt.guard_stats()
    print("arena: norm32 %.9e ref64 %.9e" % (gs["norm"], ref))
    assert abs(gs["norm"] - ref) <= U23 * ref and gs["steps"] == 1 and gs["clipped"] == 1
    model2, opt2 = _model_and_opt(gpu, base_model, max_grad_norm=1e-3)
    _model_step(model2, opt2, batches[0])
    model2.res512_3.requires_grad_(False)
    frozen = {k: v.detach().clone() for k, v in model2.res512_3.named_parameters()}
    _model_step(model2, opt2, batches[1])
    assert all(p.grad is None for p in model2.res512_3.parameters())
    ref2 = _norm_of_grads(model2.parameters())
    gs2 = opt2.guard_stats()
    assert abs(gs2["norm"] - ref2) <= U23 * ref2 and gs2["steps"] == 2
    for k, v in model2.res512_3.named_parameters():
        assert torch.equal(v, frozen[k]), "frozen parameter %s moved" % k
    assert opt2.store_of(model2._gdn_param_arena).pstep is not None          # (the per-parameter path ran)


def test_arena_padding_contributes_nothing(gpu):
    """A block whose parameters (135, 5, 5 and 5 floats) each end short of the arena's alignment: the one-launch path reads
    the zero padding between them, and the norm is still the float64 norm over the parameters' own gradients."""
    from gdn_amd import engine as E
    from gdn_amd.optim import Adam
    torch.manual_seed(2)
    blk = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.BatchNorm2d(5)).to(gpu)
    ar = E.ParamArena(blk, gpu)
    assert ar.intact() and ar.numel > sum(n for _, _, n, _ in ar.items)
    for p, o, n, tr in ar.items:
        ar.grad[o:o + n].normal_(0.0, 3.0)
        p.grad = ar.grad_view(p)
    before = ar.data.clone()
    opt = Adam(blk.parameters(), 1e-3, [0.9, 0.999], eps=1e-8, weight_decay=5e-4, max_grad_norm=1.0)
    opt.step()
    assert opt.store_of(ar) is not None and opt.store_of(ar).pstep is None            # (the one-launch path ran)
    ref = _norm_of_grads(blk.parameters())
    gs = opt.guard_stats()
    assert abs(gs["norm"] - ref) <= U23 * ref and gs["clipped"] == 1
    assert abs(float(ar.grad.double().pow(2).sum().sqrt()) - ref) <= 1e-12 * ref      # the padding is zero
    assert not torch.equal(before, ar.data)


# max_grad_norm for the graph and resume tests.  A first eager run with a bound of 2 printed the norms of the five compared
# steps as 163.06, 62.56, 54.49, 48.83, 28.89; 40 lies between the last two with room on both sides.  (Adam's update is
# nearly invariant to the gradient's scale, so the norms move little with the bound.)  With 40 they are 128.06, 83.91,
# 35.07, 72.60, 34.78: three of the five steps clip, coefficients 0.3123, 0.4767, 1, 0.5509, 1.
GRAPH_MAX_NORM = 40.0


def test_graphed_guarded_step_matches_eager(gpu, base_model, batches):
    """test_graphed_train_step_matches_eager at fp32 with the guard on: losses, model and optimizer state after five replays
    are bitwise those of the eager loop, and guard_stats() agrees.  max_grad_norm and skip_nonfinite are baked into the
    capture."""
    from gdn_amd.graph import GraphedTrainStep
    runs = {}
    for mode in ("eager", "graph"):
        model, opt = _model_and_opt(gpu, base_model, max_grad_norm=GRAPH_MAX_NORM, skip_nonfinite=True)

        def step_fn(depth, sparse, model=model, opt=opt):
            return (_model_step(model, opt, (depth, None, sparse)),)

        if mode == "eager":
            for _ in range(3):
                step_fn(batches[0][0], batches[0][2])
            run = step_fn
        else:
            run = GraphedTrainStep(step_fn, (batches[0][0], batches[0][2]), opt, warmup=3)
        losses, stats = [], []
        for i, (d, _, s) in enumerate(batches[1:]):
            if i == 3:
                for g in opt.param_groups:
                    g["lr"] = g["lr"] * 0.5
            losses.append(float(run(d, s)[0]))
            stats.append(opt.guard_stats())
        print(mode, "norms", ["%.4f" % s["norm"] for s in stats], "coefs", ["%.4f" % s["coef"] for s in stats])
        runs[mode] = (losses, stats, {k: v.clone() for k, v in model.state_dict().items()}, opt.state_dict())
    (la, sa, ma, oa), (lb, sb, mb, ob) = runs["eager"], runs["graph"]
    assert la == lb and sa == sb
    n_clipped = sum(s["coef"] < 1.0 for s in sa)
    assert 0 < n_clipped < 5, "max_grad_norm %.3g clips %d of the five steps: %s" % (GRAPH_MAX_NORM, n_clipped, [s["norm"] for s in sa])
    assert sa[-1]["steps"] == 8 and sa[-1]["skipped"] == 0
    for k, v in ma.items():
        assert torch.equal(v, mb[k]), k
    assert oa["gdn"]["guard"] == ob["gdn"]["guard"]
    for k, s in oa["state"].items():
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(s[name], ob["state"][k][name]), (k, name)
    for ra, rb in zip(oa["gdn"]["stores"], ob["gdn"]["stores"]):
        assert torch.equal(ra["state"], rb["state"])


def test_resume_restores_counters_and_continues_bitwise(gpu, base_model, batches):
    """4 guarded steps == 2 steps, state_dict() into a fresh model and optimizer, 2 more."""
    kw = dict(max_grad_norm=GRAPH_MAX_NORM, skip_nonfinite=True)
    model, opt = _model_and_opt(gpu, base_model, **kw)
    for k in range(4):
        _model_step(model, opt, batches[k])
    first, opt1 = _model_and_opt(gpu, base_model, **kw)
    for k in range(2):
        _model_step(first, opt1, batches[k])
    saved = copy.deepcopy(opt1.state_dict())
    assert saved["gdn"]["guard"]["steps"] == 2
    second, opt2 = _model_and_opt(gpu, base_model, **kw)
    second.load_state_dict(first.state_dict())
    opt2.load_state_dict(saved)
    assert opt2.state_dict()["gdn"]["guard"] == saved["gdn"]["guard"]          # before the record exists
    for k in range(2, 4):
        _model_step(second, opt2, batches[k])
    for (k, a), b in zip(model.state_dict().items(), second.state_dict().values()):
        assert torch.equal(a, b), k
    sa, sb = opt.state_dict(), opt2.state_dict()
    for k, s in sa["state"].items():
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(s[name], sb["state"][k][name]), (k, name)
    assert sa["gdn"]["guard"] == sb["gdn"]["guard"] and sa["gdn"]["guard"]["steps"] == 4
    assert opt.guard_stats() == opt2.guard_stats()
    # a record that already exists is rewritten in place
    opt2.load_state_dict(saved)
    assert opt2.guard_stats()["steps"] == 2 and opt2.guard_stats()["clipped"] == saved["gdn"]["guard"]["clipped"]


# ---------------------------------------------------------------------------------------------------------------------
def _cli(cwd, argv, limit=240):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([str(REPO / "gdn-pytorch_amd"), str(REPO)] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    cwd.mkdir(parents=True, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "gdn_amd.GDN_main", *argv]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(cwd), timeout=limit + 60)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def test_command_line_flags(gpu, tmp_path):
    """One fresh child process per run (--gpu_num 0: the parser's default names the reference's third GPU)."""
    base = ["--synthetic", "--mode", "DtoD", "--height", "32", "--width", "64", "--batch_size", "2", "--epochs", "1",
            "--epoch_size", "3", "--gpu_num", "0"]
    out = _cli(tmp_path / "guarded", base + ["--clip_grad_norm", "1.0", "--skip_nonfinite"])
    lines = [l for l in out.splitlines() if l.startswith("grad guard:")]
    assert len(lines) == 1 and lines[0].endswith("of 3 steps"), out[-2000:]
    plain = _cli(tmp_path / "plain", base)
    assert "grad guard:" not in plain and "grad_norm:" not in plain


def test_two_ranks_take_the_same_decision(gpu, tmp_path):
    """Two ranks over RCCL, 3 guarded steps with clipping active; on step 2 rank 1 alone has a NaN in its local gradient: the
    all-reduce carries it to both, both skip, and records and parameters stay bitwise identical."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    import torch.multiprocessing as mp
    import grad_guard_worker
    mp.spawn(grad_guard_worker.run, args=(2, 29641, 3, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert len(r0["stats"]) == len(r1["stats"]) == 3
    for a, b in zip(r0["stats"], r1["stats"]):          # (the skipped step's norm is a NaN on both: compare the bits)
        assert struct.pack("<ffiii", *a.values()) == struct.pack("<ffiii", *b.values()), (a, b)
    assert r0["stats"][-1]["skipped"] == 1 and r0["stats"][-1]["steps"] == 3 and r0["stats"][-1]["clipped"] == 2
    assert r0["stats"][1]["coef"] == 0.0
    assert torch.equal(r0["data"], r1["data"]) and bool(torch.isfinite(r0["data"]).all())
