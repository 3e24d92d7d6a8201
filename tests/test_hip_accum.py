"""Gradient accumulation on the GPU: gdn_grad_accumulate bit for bit, the arena's accumulating backward
(no copy, one launch, no allocation after the first group), train_AE_DtoD / train_AE_RtoD with accum_steps against loops
written with what existed before (zero_grad / backward / backward / grad_scale = 1/k / step), Adam.micro_batches against
torch, the guard and the average per update, and resume.  Networks at 32x64 with B = 2."""
import os

import numpy as np
import pytest
import torch

from test_hip_graph_train import B, H, LR, W, _augment_loader, _bits, _loop, _networks, _same
from test_hip_kernels import close

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 256, 257, 4099, 2 ** 20 + 7]
PAD = 8            # canary floats on either side of an operand (a multiple of 4: the operand's offset decides its alignment)
CANARY = np.float32(-1234.5)
# what the issue names: subnormals, both zeros, both infinities, NaN -- and normals small enough that sums and differences
# of two of them are subnormal (a kernel that flushed its results would show there)
SPECIAL = np.array([1e-40, -1e-40, 3e-42, -7e-45, 1.4e-45, 0.0, -0.0, np.inf, -np.inf, np.nan, 1.5e-38, -1.2e-38, 2e-38,
                    3.4e38, -3.4e38, 1.0, -1.0], dtype=np.float32)


def _operand(rng, n):
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
    pick = rng.random(n) < 0.25
    x[pick] = SPECIAL[rng.integers(0, len(SPECIAL), int(pick.sum()))]
    return x


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel
@pytest.mark.parametrize("n", SIZES)
def test_grad_accumulate_is_one_float32_add_per_element(gpu, n):
    """Every pair of base offsets 0..3 floats (equal modulo 4: the 16-byte form with its head and tail lanes; different: the
    scalar form) against numpy's float32 acc + g: NaNs in the same places, every other element bit for bit; the floats
    around acc and all of g unchanged."""
    from gdn_amd import ops
    rng = np.random.default_rng(1000 + n)
    with np.errstate(all="ignore"):
        for oa in range(4):
            for og in range(4):
                a, g = _operand(rng, n), _operand(rng, n)
                if n >= 5:          # the named cases, whatever the draw: opposite infinities, a subnormal sum, a subnormal difference
                    a[:5] = np.array([np.inf, 1e-40, 1.5e-38, -0.0, np.nan], dtype=np.float32)
                    g[:5] = np.array([-np.inf, 3e-42, -1.2e-38, 0.0, 1.0], dtype=np.float32)
                abuf = np.full(n + 3 + 2 * PAD, CANARY, dtype=np.float32)
                gbuf = np.full(n + 3 + 2 * PAD, CANARY, dtype=np.float32)
                abuf[PAD + oa:PAD + oa + n] = a
                gbuf[PAD + og:PAD + og + n] = g
                ta, tg = torch.from_numpy(abuf).to(gpu), torch.from_numpy(gbuf).to(gpu)
                assert ta.data_ptr() % 16 == 0 and tg.data_ptr() % 16 == 0
                ops.grad_accumulate(ta[PAD + oa:PAD + oa + n], tg[PAD + og:PAD + og + n])
                got_a, got_g = ta.cpu().numpy(), tg.cpu().numpy()
                want = abuf.copy()
                want[PAD + oa:PAD + oa + n] = a + g
                what = "n = %d, offsets %d / %d" % (n, oa, og)
                assert got_g.view(np.uint32).tobytes() == gbuf.view(np.uint32).tobytes(), what + ": g was written"
                nan = np.isnan(want)
                assert np.array_equal(np.isnan(got_a), nan), what + ": NaN positions"
                assert np.array_equal(got_a.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what


def test_grad_accumulate_keeps_subnormal_results(gpu):
    """(the operands of the test above hold such cases; this one names them)"""
    from gdn_amd import ops
    a = np.array([1.5e-38, 1e-40, -1.4e-45, 1.1754944e-38], dtype=np.float32)
    g = np.array([-1.2e-38, 3e-42, 1.4e-45, -1.4e-45], dtype=np.float32)
    want = a + g
    assert 0 < abs(want[0]) < 1.1754944e-38 and 0 < abs(want[1]) < 1.1754944e-38 and 0 < abs(want[3]) < 1.1754944e-38
    ta, tg = torch.from_numpy(a).to(gpu), torch.from_numpy(g).to(gpu)
    ops.grad_accumulate(ta, tg)
    assert ta.cpu().numpy().view(np.uint32).tolist() == want.view(np.uint32).tolist()


def test_grad_accumulate_argument_checks(gpu):
    from gdn_amd import ops
    from gdn_amd._lib import GdnError, lib
    buf, other = torch.zeros(64, device=gpu), torch.ones(64, device=gpu)
    with pytest.raises(GdnError):
        lib.gdn_grad_accumulate(None, other.data_ptr(), 8, ops.stream())
    with pytest.raises(GdnError):
        lib.gdn_grad_accumulate(buf.data_ptr(), None, 8, ops.stream())
    with pytest.raises(GdnError):
        lib.gdn_grad_accumulate(buf.data_ptr(), other.data_ptr(), 0, ops.stream())
    with pytest.raises(GdnError):
        ops.grad_accumulate(buf, buf)
    with pytest.raises(GdnError):
        ops.grad_accumulate(buf[0:8], buf[7:15])
    with pytest.raises(GdnError):
        ops.grad_accumulate(buf[0:8], other[0:9])
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0 and float(other.sum()) == 64.0


# ---------------------------------------------------------------------------------------------------------------------
# 2. the arena
@pytest.mark.parametrize("net,dtype", [("DtoD", "fp32"), ("DtoD", "bf16"), ("RtoD_single", "fp32")])
def test_accumulating_backward_is_exact_and_allocates_nothing(gpu, monkeypatch, net, dtype):
    """g1, g2, g3 from three fresh backwards on three batches; one zero_grad and three accumulating backwards then leave
    exactly float32 (g1 + g2) + g3 in every parameter's .grad (train-mode gradients do not depend on the BatchNorm running
    statistics, and a backward is bitwise reproducible).  Each accumulating backward makes its sum with ONE
    gdn_grad_accumulate launch, and from the second group on a group leaves torch.cuda.memory_allocated() where it was."""
    from gdn_amd import ops
    from gdn_amd import utils as U
    from gdn_amd.synthetic import synthetic_batch
    model = _networks(gpu, net, dtype)[0].train()
    batches = [synthetic_batch(B, H, W, seed=40 + k, device=gpu) for k in range(3)]
    calls = []
    real = ops.grad_accumulate
    monkeypatch.setattr(ops, "grad_accumulate", lambda acc, g: (calls.append(acc.numel()), real(acc, g))[1])

    def backward(batch):
        depth, rgb, sparse = batch
        if net == "DtoD":
            loss = U.dtod_loss(model(depth, istrain=False), depth, sparse)[0]
        else:
            loss = U.rtod_pixel_loss(model(rgb, istrain=False), depth, rgb, sparse)[0]
        U.backward(loss)

    def zero():
        for p in model.parameters():
            p.grad = None

    singles = []
    for batch in batches:
        zero()
        backward(batch)
        singles.append(model._gdn_param_arena.grad.clone())
    assert not calls
    arena = model._gdn_param_arena
    want = (singles[0] + singles[1]) + singles[2]
    assert float(want.abs().max()) > 0.0 and not torch.equal(singles[0], singles[1])

    def group():
        zero()
        for batch in batches:
            backward(batch)
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated()

    mem = [group() for _ in range(3)]
    assert calls == [arena.numel] * 6, calls              # two accumulating backwards per group, one launch each
    assert _bits(arena.grad) == _bits(want)
    for p, o, n, tr in arena.items:
        assert p.grad.data_ptr() == arena.grad.data_ptr() + 4 * o
        assert _bits(p.grad) == _bits(arena._view(want, o, p.shape, tr)), "accumulated gradient of a %s" % (tuple(p.shape),)
    print("memory_allocated after groups 1..3:", mem)
    assert mem[2] == mem[1], mem


# ---------------------------------------------------------------------------------------------------------------------
# 3. the loops against loops written with what existed before
def _loader(gpu, mode, steps=5):
    from gdn_amd.synthetic import SyntheticLoader
    if mode == "RtoD":
        return SyntheticLoader(B, steps, H, W, seed=20, device=gpu, distinct=steps)
    return _augment_loader(gpu, n=B * steps)


def _hand_loop(gpu, where, mode, dtype, loader, k_max, epochs, opt_kw):
    """accum_steps = k_max written by hand: zero_grad / backward ... backward / grad_scale = 1 / k / step, the loops' losses
    and their checkpoint files."""
    from gdn_amd import trainer as T
    from gdn_amd import utils as U
    from gdn_amd.optim import Adam
    where.mkdir(parents=True, exist_ok=True)
    net, guide = _networks(gpu, mode, dtype)
    opt = Adam(net.parameters(), LR, [0.9, 0.999], eps=1e-08, weight_decay=5e-4, **opt_kw)
    kind = "DtoD" if mode == "DtoD" else "RtoD"
    save_dir = './KITTI_AE_%s_trained_model_lr000%d_color_uNet_gen2_nogradf' % (kind, LR * 100000)
    zero = torch.zeros((), device=gpu)
    cwd = os.getcwd()
    os.chdir(where)
    try:
        model_num, loss = 0, None
        for epoch in range(epochs):
            net.train()
            k = 0
            for i, (gt, rgb, sparse) in enumerate(loader):
                if mode == "DtoD":
                    loss = U.dtod_loss(net(gt, istrain=False), gt, sparse)[0]
                else:
                    out = net(rgb, istrain=False)
                    latent = zero if guide is None else T.guide_latent_loss(guide, gt, out)
                    loss = U.rtod_pixel_loss(out, gt, rgb, sparse, plus=latent)[0]
                if k == 0:
                    opt.zero_grad()
                U.backward(loss)
                k += 1
                if k == k_max or i == len(loader) - 1:
                    opt.grad_scale = 1.0 / k
                    opt.step()
                    k = 0
                if i >= len(loader) - 1:
                    break                                  # (as the loops leave their loader: epoch_size is its length)
            if mode == "DtoD":
                T._save_checkpoint(net, save_dir + '/epoch_%d_AE_depth_loss_%.4f.pkl' % (model_num + 1, loss.item()), opt)
                model_num += 1
        if mode != "DtoD":
            T._save_checkpoint(net, save_dir + '/epoch_%d_AE_depth_loss_%.4f.pkl' % (model_num + 1, loss.item()), opt)
    finally:
        os.chdir(cwd)
    torch.cuda.synchronize()
    files = sorted(where.rglob("*.pkl"))
    return {"names": [str(f.relative_to(where)) for f in files],
            "pkl": {f.name: torch.load(f, map_location="cpu") for f in files},
            "model": {k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
            "opt": T._cpu_copy(opt.state_dict())}


def _equal_runs(a, b):
    assert a["names"] == b["names"] and a["names"], (a["names"], b["names"])
    _same(a["pkl"], b["pkl"], "pkl")
    _same(a["model"], b["model"], "model")
    _same(a["opt"], b["opt"], "optimizer")


@pytest.mark.parametrize("mode,dtype,capturable", [("DtoD", "fp32", False), ("DtoD", "fp32", True), ("RtoD", "fp32", False),
                                                   ("RtoD", "bf16", False), ("RtoD_single", "fp32", False),
                                                   ("RtoD_single", "bf16", False)])
def test_accum_loop_equals_the_hand_written_loop(gpu, tmp_path, mode, dtype, capturable):
    """Two epochs of five batches with accum_steps = 2: groups of 2, 2 and 1 in each epoch.  Model state (BatchNorm buffers
    included), optimizer.state_dict() and every .pkl bit for bit."""
    opt_kw = dict(capturable=capturable)
    loop = _loop(gpu, tmp_path / "loop", mode, dtype, False, _loader(gpu, mode), epochs=2, epoch_size=5, opt_kw=opt_kw,
                 accum_steps=2)
    hand = _hand_loop(gpu, tmp_path / "hand", mode, dtype, _loader(gpu, mode), 2, 2, opt_kw)
    _equal_runs(hand, loop)
    assert len(loop["names"]) == (2 if mode == "DtoD" else 1)
    step = loop["opt"]["state"][0]["step"]
    assert float(step) == 6.0, step                        # three updates per epoch, not five


def test_accum_steps_one_is_the_loop_without_the_flag(gpu, tmp_path):
    runs = [_loop(gpu, tmp_path / name, "DtoD", "fp32", False, _loader(gpu, "DtoD"), epochs=2, epoch_size=5,
                  opt_kw=dict(capturable=False), save_state_every=4, **more)
            for name, more in (("without", {}), ("one", dict(accum_steps=1)))]
    _equal_runs(*runs)
    from gdn_amd import trainer as T
    states = [T.read_training_state(sorted((tmp_path / name).rglob(T.STATE_FILE))[0]) for name in ("without", "one")]
    _same(states[0], states[1], "train_state.pt")
    assert "accum_steps" not in states[1]


# ---------------------------------------------------------------------------------------------------------------------
# 4. Adam.micro_batches against torch
def test_micro_batches_matches_torch_on_the_mean_gradient(gpu):
    """Three loose parameters, 4 updates of K = 3 gradients each: .grad holds their float32 sum and micro_batches = 3; torch's
    clip_grad_norm_ + Adam on the CPU get the float64 mean cast to float32.  The bar of
    test_matches_torch_clip_grad_norm_and_adam."""
    from gdn_amd.optim import Adam
    shapes, max_norm, K = [(64, 3, 3, 3), (64,), (7,)], 1.0, 3
    gen = torch.Generator().manual_seed(3)
    init = [torch.randn(s, generator=gen) for s in shapes]
    mine = [torch.nn.Parameter(t.clone().to(gpu)) for t in init]
    theirs = [torch.nn.Parameter(t.clone()) for t in init]
    opt = Adam(mine, 1e-3, [0.9, 0.999], eps=1e-8, weight_decay=5e-4, max_grad_norm=max_norm)
    opt.micro_batches = K
    ref = torch.optim.Adam(theirs, 1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
    clipped = 0
    for k in range(4):
        scale = 0.004 if k % 2 else 0.1            # norms of the mean on either side of max_grad_norm
        for a, b in zip(mine, theirs):
            gs = [scale * torch.randn(b.shape, generator=gen) for _ in range(K)]
            a.grad = ((gs[0].to(gpu) + gs[1].to(gpu)) + gs[2].to(gpu))
            b.grad = (sum(g.double() for g in gs) / K).float()
        total = float(torch.nn.utils.clip_grad_norm_(theirs, max_norm))
        clipped += total > max_norm
        ref.step()
        opt.step()
        st = opt.guard_stats()
        print("update %d: norm %.7g (torch %.7g)" % (k + 1, st["norm"], total))
        assert abs(st["norm"] - total) <= 1e-5 * total and st["clipped"] == clipped
    assert clipped == 2 and opt.guard_stats()["steps"] == 4
    for a, b, s in zip(mine, theirs, shapes):
        close(a, b, rtol=1e-5, atol_scale=1e-6, what="Adam(micro_batches=3) vs torch on the mean, %s" % (s,))


# ---------------------------------------------------------------------------------------------------------------------
# 5. guard and average per update
def test_a_poisoned_micro_batch_skips_its_whole_group(gpu, tmp_path, monkeypatch):
    """K = 2 over six batches with skip_nonfinite and ema_decay; a NaN written into the gradient arena after the FIRST
    backward of the middle group stays in the sum through the second one, so that group's update is skipped: one norm, one
    decision and one count per group (3 steps, 1 skipped), and weights, moments, step counts and averages end bit for bit
    where a run over the other four batches ends.  (BatchNorm running statistics saw the skipped forwards: not compared.)"""
    from gdn_amd import engine as E
    from gdn_amd.synthetic import SyntheticLoader
    opt_kw = dict(skip_nonfinite=True, ema_decay=0.9)
    six = SyntheticLoader(B, 6, H, W, seed=60, device=gpu, distinct=6)
    four = SyntheticLoader(B, 4, H, W, seed=60, device=gpu, distinct=4)
    four.batches = [six.batches[k] for k in (0, 1, 4, 5)]
    real, n = E.end_backward, [0]

    def poisoned(arena, pending, trainable=True):
        real(arena, pending, trainable)
        n[0] += 1
        if n[0] == 3:
            arena.grad[12345] = float("nan")
    monkeypatch.setattr(E, "end_backward", poisoned)
    bad = _loop(gpu, tmp_path / "six", "DtoD", "fp32", False, six, epochs=1, epoch_size=6, opt_kw=opt_kw, accum_steps=2)
    monkeypatch.setattr(E, "end_backward", real)
    assert n[0] == 6
    good = _loop(gpu, tmp_path / "four", "DtoD", "fp32", False, four, epochs=1, epoch_size=4, opt_kw=opt_kw, accum_steps=2)
    assert bad["guard"]["steps"] == 3 and bad["guard"]["skipped"] == 1
    assert good["guard"]["steps"] == 2 and good["guard"]["skipped"] == 0
    params = [k for k in bad["model"] if "running_" not in k and "num_batches" not in k]
    _same({k: bad["model"][k] for k in params}, {k: good["model"][k] for k in params}, "weights")
    _same(bad["opt"]["state"], good["opt"]["state"], "moments and step counts")
    # (a store's host-side 'step' counts the calls of step(), skipped ones included; the device's own count is in 'state')
    _same([r["state"] for r in bad["opt"]["gdn"]["stores"]], [r["state"] for r in good["opt"]["gdn"]["stores"]],
          "device step state")
    assert [r["step"] for r in bad["opt"]["gdn"]["stores"]] == [3] and [r["step"] for r in good["opt"]["gdn"]["stores"]] == [2]
    _same(bad["opt"]["gdn"]["ema"], good["opt"]["gdn"]["ema"], "averages")
    assert float(bad["opt"]["state"][0]["step"]) == 2.0
    assert all(bool(torch.isfinite(v).all()) for v in bad["model"].values())


# ---------------------------------------------------------------------------------------------------------------------
# 6. resume
def test_a_state_due_inside_a_group_is_written_at_its_end_and_resumes_exactly(gpu, tmp_path):
    """accum_steps 2, save_state_every 3, five batches per epoch: iteration 3 is the first micro-batch of the second group, so
    the state is written after iteration 4.  The run stopped after one epoch and resumed ends bit for bit like the
    uninterrupted one; resuming with another accum_steps raises before any step."""
    from gdn_amd import trainer as T
    from gdn_amd._lib import GdnError
    kw = dict(epoch_size=5, save_state_every=3, accum_steps=2, opt_kw=dict(capturable=False))
    full = _loop(gpu, tmp_path / "full", "DtoD", "fp32", False, _loader(gpu, "DtoD"), epochs=2, **kw)
    stopped = _loop(gpu, tmp_path / "stopped", "DtoD", "fp32", False, _loader(gpu, "DtoD"), epochs=1, **kw)
    (state,) = sorted((tmp_path / "stopped").rglob(T.STATE_FILE))
    head = T.read_training_state(state)
    assert (head["step"], head["epoch"], head["i"], head["accum_steps"]) == (4, 0, 3, 2)
    assert float(head["optimizer"]["state"][0]["step"]) == 2.0          # two updates applied, no half-accumulated gradient
    resumed = _loop(gpu, tmp_path / "resumed", "DtoD", "fp32", False, _loader(gpu, "DtoD"), epochs=2, resume=state, **kw)
    assert len(full["names"]) == 2 and resumed["names"] == full["names"] and stopped["names"] == full["names"][:1]
    _same(full["pkl"], resumed["pkl"], "pkl")
    _same(full["model"], resumed["model"], "model")
    _same(full["opt"], resumed["opt"], "optimizer")
    with pytest.raises(GdnError, match="--accum_steps 2.*--accum_steps 3"):
        _loop(gpu, tmp_path / "other", "DtoD", "fp32", False, _loader(gpu, "DtoD"), epochs=2, resume=state,
              **dict(kw, accum_steps=3))
    assert not list((tmp_path / "other").rglob("*.pkl"))
