"""Weight average of the fused Adam on the GPU: gdn_ema_update and gdn_swap_f32 from the kernels up to
optim.Adam(ema_decay=), swap_averaged(), GraphedTrainStep, state_dict(), train_state.pt and the command line.  The float64
yardstick and its bound are tests/ema_fp64.py."""
import copy
import os
import pathlib
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import ema_fp64 as R
from oracle import gdn_oracle as O
from test_hip_kernels import close

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parent.parent
# Both kernels launch min(ceil(lanes / 256), 4096) blocks of 256 lanes, one lane per 16 bytes on the vector path (per float on
# the scalar one): a full trip of the capped grid is 4096 x 256 x 4 floats.  The sizes the issue names, one that is whole
# blocks x 256 x 4 plus 5, and one past that full trip (every lane of the vector body then strides, the scalar body four times).
GRID_CAP = 4096
FULL_TRIP = GRID_CAP * 256 * 4
SIZES = [1, 3, 255, 256, 257, 1023, 4099, 8 * 256 * 4 + 5, FULL_TRIP + 1029]
SMALLEST, LARGEST = SIZES[:3], SIZES[-3:]
OFFSETS = (0, 1, 2, 3)
PAD = 4                       # guard elements on either side of a slice
DECAY = 0.999
GUARD_FMT = "<dffiiii"
H, W = 32, 64


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    """Two seeded host buffers every size and offset is a slice of: normal samples times 10**uniform(-6, 2), made once and
    never written."""
    rng = np.random.default_rng(20261019)
    n = max(SIZES) + max(OFFSETS) + 2 * PAD
    a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)).astype(np.float32)
    return a, b


def _state(gpu, t):
    return torch.frombuffer(bytearray(R.state_record(t)), dtype=torch.uint8).to(gpu)


def _guard(gpu, skip):
    raw = struct.pack(GUARD_FMT, 0.0, 1.0, 0.0 if skip else 1.0, int(skip), 1, 0, int(skip))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(gpu)


def _slice(buf, off, n):
    s = buf[PAD + off:PAD + off + n]
    assert s.data_ptr() % 16 == 4 * off          # (torch's allocations are 16-byte aligned and PAD is 4 floats)
    return s


def _outside_untouched(buf, orig, off, n, what):
    assert torch.equal(buf[:PAD + off], orig[:PAD + off]), "%s: elements before the slice changed" % (what,)
    assert torch.equal(buf[PAD + off + n:], orig[PAD + off + n:]), "%s: elements after the slice changed" % (what,)


def _ema_case(gpu, pool, n, off_e, off_p, steps):
    """`steps` consecutive updates with t = 1, 2, ... and a changing p, then one at t = 20000 (w = float32(0.001)); checked
    after every update against the restatement fed the device's float32 p."""
    from gdn_amd import ops
    he, hp = pool
    m = n + max(OFFSETS) + 2 * PAD
    ebuf, pbuf = torch.from_numpy(he[:m]).to(gpu), torch.from_numpy(hp[:m]).to(gpu)
    e0 = ebuf.clone()
    e, p = _slice(ebuf, off_e, n), _slice(pbuf, off_p, n)
    p_first = hp[PAD + off_p:PAD + off_p + n]
    e64 = he[PAD + off_e:PAD + off_e + n].astype(np.float64)
    M = np.abs(e64)
    worst = 0.0
    for k, t in enumerate(list(range(1, steps + 1)) + [20000], 1):
        p_host = (p_first * np.float32(1.0 + 0.125 * (k - 1))).astype(np.float32)
        p.copy_(torch.from_numpy(p_host))
        pbefore = pbuf.clone()
        ops.ema_update(e, p, DECAY, _state(gpu, t))
        e64 = R.update(e64, p.cpu().numpy(), DECAY, t)
        M = np.maximum(M, np.maximum(np.abs(p_host.astype(np.float64)), np.abs(e64)))
        err, lim = np.abs(e.cpu().numpy().astype(np.float64) - e64), R.bound(k, M)
        worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
        assert np.all(err <= lim), "n=%d offsets (%d, %d) update %d (t=%d): %.3f of the bound" % (n, off_e, off_p, k, t, worst)
        _outside_untouched(ebuf, e0, off_e, n, "ema n=%d offsets (%d, %d) update %d" % (n, off_e, off_p, k))
        assert torch.equal(pbuf, pbefore), "p was written"
    assert R.weight(DECAY, 20000) == np.float32(0.001)
    return worst


@pytest.mark.parametrize("n", SIZES)
def test_ema_update_against_float64(gpu, pool, n):
    """Common base offsets 0 ... 3 floats (the 16-byte body with its scalar head and tail): 5 updates with t = 1 ... 5 and one
    at t = 20000, each within bound(k, M) of the float64 restatement; the neighbours of the slice stay bitwise untouched."""
    for off in OFFSETS:
        worst = _ema_case(gpu, pool, n, off, off, 5)
        print("n=%d offset=%d: worst error %.3f of the bound" % (n, off, worst))


@pytest.mark.parametrize("n", [3, 257, 4099, FULL_TRIP + 1029])
def test_ema_update_scalar_body(gpu, pool, n):
    """ema and p at different offsets modulo 16 bytes: the scalar body, same bar."""
    for off_e, off_p in ((1, 3), (0, 2)):
        worst = _ema_case(gpu, pool, n, off_e, off_p, 2)
        print("n=%d offsets (%d, %d): worst error %.3f of the bound" % (n, off_e, off_p, worst))


@pytest.mark.parametrize("n,off", [(3, 1), (4099, 1), (8 * 256 * 4 + 5, 0)])
def test_ema_update_skip_rule(gpu, pool, n, off):
    """A guard record whose skip is 1 leaves ema bitwise alone; skip 0 and no guard give bitwise the same result."""
    from gdn_amd import ops
    he, hp = pool
    m = n + max(OFFSETS) + 2 * PAD
    p = _slice(torch.from_numpy(hp[:m]).to(gpu), off, n)
    orig = torch.from_numpy(he[:m]).to(gpu)
    results = []
    for guard in (_guard(gpu, True), _guard(gpu, False), None):
        ebuf = orig.clone()
        ops.ema_update(_slice(ebuf, off, n), p, DECAY, _state(gpu, 3), guard)
        results.append(ebuf)
    assert torch.equal(results[0], orig), "a skipped step wrote the average"
    assert torch.equal(results[1], results[2]) and not torch.equal(results[1], orig)


def _swap_pairs(n):
    if n in SMALLEST or n in LARGEST:
        return [(a, b) for a in OFFSETS for b in OFFSETS]
    return [(a, a) for a in OFFSETS] + [(1, 2)]


@pytest.mark.parametrize("n", SIZES)
def test_swap_f32(gpu, pool, n):
    """After one exchange a holds the old b and b the old a, bitwise, neighbours untouched; after two both are restored."""
    from gdn_amd import ops
    ha, hb = pool
    m = n + max(OFFSETS) + 2 * PAD
    a0, b0 = torch.from_numpy(ha[:m]).to(gpu), torch.from_numpy(hb[:m]).to(gpu)
    for off_a, off_b in _swap_pairs(n):
        abuf, bbuf = a0.clone(), b0.clone()
        a, b = _slice(abuf, off_a, n), _slice(bbuf, off_b, n)
        ops.swap_(a, b)
        what = "swap n=%d offsets (%d, %d)" % (n, off_a, off_b)
        assert torch.equal(a, _slice(b0, off_b, n)) and torch.equal(b, _slice(a0, off_a, n)), what
        _outside_untouched(abuf, a0, off_a, n, what)
        _outside_untouched(bbuf, b0, off_b, n, what)
        ops.swap_(a, b)
        assert torch.equal(abuf, a0) and torch.equal(bbuf, b0), what + ": two exchanges do not restore"


def test_swap_refuses_overlap_on_the_device_path(gpu):
    from gdn_amd import ops
    from gdn_amd._lib import GdnError
    buf = torch.zeros(64, device=gpu)
    with pytest.raises(GdnError):
        ops.swap_(buf[0:32], buf[31:63])


# ---------------------------------------------------------------------------------------------------------------------
def _grads(n, steps, seed=100):
    return [torch.randn(n, generator=torch.Generator().manual_seed(seed + i)) for i in range(steps)]


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


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def test_ema_leaves_adam_alone(gpu):
    """Six steps of a loose parameter with and without ema_decay: p, m, v and the device step state are bitwise equal after
    every step, and the average follows the restatement (avg_0 = p_0)."""
    n = 4099
    grads = _grads(n, 6)
    p0, plain = _loose(gpu, n, capturable=True)
    p1, ema = _loose(gpu, n, ema_decay=DECAY)
    e64 = _np64(p1)
    M = np.abs(e64)
    assert torch.equal(ema.averaged(p1), p1.detach())
    for k, g in enumerate(grads, 1):
        p0.grad, p1.grad = g.to(gpu), g.to(gpu)
        plain.step()
        ema.step()
        _same(_snapshot(p0, plain), _snapshot(p1, ema), "step %d" % k)
        e64 = R.update(e64, p1.detach().cpu().numpy(), DECAY, k)
        M = np.maximum(M, np.maximum(np.abs(_np64(p1)), np.abs(e64)))
        assert np.all(np.abs(_np64(ema.averaged(p1)) - e64) <= R.bound(k, M)), k
    assert plain.store_of(p0).ema is None and not torch.equal(ema.averaged(p1), p1.detach())


def test_guarded_ema_takes_the_same_skip_decision(gpu):
    """max_grad_norm / skip_nonfinite with and without ema_decay, an Inf in the gradient of step 3: Adam's state is bitwise
    the same in both runs after every step; the skipped step leaves the average bitwise alone and takes no place in the
    warm-up -- the next update uses weight(d, 3), not weight(d, 4)."""
    n = 4099
    grads = _grads(n, 6)
    grads[2] = grads[2].clone()
    grads[2][n // 3] = float("inf")
    kw = dict(max_grad_norm=10.0, skip_nonfinite=True)
    p0, plain = _loose(gpu, n, **kw)
    p1, ema = _loose(gpu, n, ema_decay=DECAY, **kw)
    t = 0
    for k, g in enumerate(grads):
        p0.grad, p1.grad = g.to(gpu), g.to(gpu)
        before = ema.averaged(p1).clone() if k else p1.detach().clone()
        plain.step()
        ema.step()
        _same(_snapshot(p0, plain), _snapshot(p1, ema), "step %d" % (k + 1))
        after = ema.averaged(p1)
        if k == 2:
            assert torch.equal(after, before), "the skipped step moved the average"
            assert ema.store_of(p1).count(p1) == 2
            continue
        t += 1
        p_now = p1.detach().cpu().numpy()
        M = np.maximum(np.abs(_np64(before)), np.abs(p_now.astype(np.float64)))
        want = R.update(_np64(before), p_now, DECAY, t)
        assert np.all(np.abs(_np64(after) - want) <= R.bound(1, M)), "step %d: not weight(d, %d)" % (k + 1, t)
        if k == 3:
            assert t == 3
            other = R.update(_np64(before), p_now, DECAY, 4)
            assert np.any(np.abs(_np64(after) - other) > R.bound(1, M)), "the step after the skipped one used weight(d, 4)"
    assert ema.guard_stats()["skipped"] == 1 and ema.store_of(p1).count(p1) == 5


def test_matches_torch_adam_and_averaged_model(gpu):
    """Three parameters, 10 steps against torch.optim.Adam on the CPU with torch.optim.swa_utils.AveragedModel's update by
    hand -- avg.lerp_(p, w_t) with this library's w_t, in float64 -- at the bar test_matches_torch_clip_grad_norm_and_adam
    holds for the weights."""
    from gdn_amd.optim import Adam
    shapes = [(64, 3, 3, 3), (64,), (7,)]
    gen = torch.Generator().manual_seed(3)
    init = [torch.randn(s, generator=gen) for s in shapes]
    mine = [torch.nn.Parameter(t.clone().to(gpu)) for t in init]
    theirs = [torch.nn.Parameter(t.clone()) for t in init]
    opt = Adam(mine, 1e-3, [0.9, 0.999], eps=1e-8, weight_decay=5e-4, ema_decay=DECAY)
    ref = torch.optim.Adam(theirs, 1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
    avg = [t.detach().double().clone() for t in theirs]
    for k in range(1, 11):
        for a, b in zip(mine, theirs):
            g = 0.1 * torch.randn(b.shape, generator=gen)
            a.grad, b.grad = g.clone().to(gpu), g.clone()
        ref.step()
        opt.step()
        for e, b in zip(avg, theirs):
            e.lerp_(b.detach().double(), float(R.weight(DECAY, k)))
    for a, b, e, s in zip(mine, theirs, avg, shapes):
        close(a, b, rtol=1e-5, atol_scale=1e-6, what="Adam vs torch, %s" % (s,))
        close(opt.averaged(a), e, rtol=1e-5, atol_scale=1e-6, what="average vs lerp_ in float64, %s" % (s,))
        assert opt.averaged(a).shape == a.shape


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


def _within(avg, start, p_now, t, k, what):
    want = R.update(_np64(start), p_now.detach().cpu().numpy(), DECAY, t)
    M = np.maximum(np.maximum(np.abs(_np64(start)), np.abs(_np64(p_now))), np.abs(want))
    assert np.all(np.abs(_np64(avg) - want) <= R.bound(k, M)), what


def test_arena_one_launch_and_partial_coverage(gpu, base_model, batches):
    """One model step on the one-launch path: averaged(p) = p_0 + w_1 (p_1 - p_0) within bound(1, M) for every parameter in
    its LOGICAL shape, convolution weights (tap-major underneath) included.  Then res512_3 is frozen: step 2 runs per
    parameter with each parameter's own device step state; the frozen parameters' weights and averages stay bitwise what
    they were, the others average on with w_2.  A block frozen before the first step never moves, so its averages stay
    bitwise equal to its weights."""
    model, opt = _model_and_opt(gpu, base_model, ema_decay=DECAY)
    p0 = [p.detach().clone() for p in model.parameters()]
    _model_step(model, opt, batches[0])
    ar = model._gdn_param_arena
    assert opt.store_of(ar).pstep is None and any(tr is not None for _, _, _, tr in ar.items)
    for (name, p), start in zip(model.named_parameters(), p0):
        assert opt.averaged(p).shape == p.shape, name
        _within(opt.averaged(p), start, p, 1, 1, "%s after one step" % name)
    assert all(not torch.equal(opt.averaged(p), p.detach()) for p in model.parameters() if p.dim() == 4)
    model.res512_3.requires_grad_(False)
    frozen = {id(p) for p in model.res512_3.parameters()}
    e1 = [opt.averaged(p).clone() for p in model.parameters()]
    p1 = [p.detach().clone() for p in model.parameters()]
    _model_step(model, opt, batches[1])
    assert opt.store_of(ar).pstep is not None          # (the per-parameter path ran)
    for (name, p), e, w in zip(model.named_parameters(), e1, p1):
        if id(p) in frozen:
            assert torch.equal(p, w) and torch.equal(opt.averaged(p), e), "frozen %s moved" % name
        else:
            assert p.dim() != 4 or not torch.equal(opt.averaged(p), e), name
            _within(opt.averaged(p), e, p, 2, 1, "%s on the per-parameter path" % name)
    # frozen from the start
    model2, opt2 = _model_and_opt(gpu, base_model, ema_decay=DECAY)
    model2.res512_3.requires_grad_(False)
    for k in range(2):
        _model_step(model2, opt2, batches[k])
    for name, p in model2.named_parameters():
        if name.startswith("res512_3."):
            assert torch.equal(opt2.averaged(p), p.detach()), "frozen %s: average and weights differ" % name
        elif p.dim() == 4:
            assert not torch.equal(opt2.averaged(p), p.detach()), name


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_swap_on_a_model(gpu, base_model, batches, dtype):
    """In eval(), the output inside averaged_weights() is bitwise the output of a second model that was handed the
    averaged(p) tensors (so it does not depend on how the exchange is made) and differs from the raw output; afterwards
    output and state_dict() are bitwise what they were.  bf16: the shadow of the weights is refreshed both ways."""
    from gdn_amd._lib import GdnError
    model, opt = _model_and_opt(gpu, base_model, ema_decay=DECAY)
    model.compute_dtype(dtype)
    for k in range(3):
        _model_step(model, opt, batches[k])
    model.eval()
    x = batches[4][0]
    with torch.no_grad():
        raw = model(x, istrain=False).clone()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    ref = copy.deepcopy(base_model).to(gpu).compute_dtype(dtype)
    ref.load_state_dict(state)
    with torch.no_grad():
        for q, p in zip(ref.parameters(), model.parameters()):
            q.copy_(opt.averaged(p))
    ref.eval()
    with torch.no_grad():
        want = ref(x, istrain=False).clone()
    with opt.averaged_weights():
        with torch.no_grad():
            got = model(x, istrain=False).clone()
        with pytest.raises(GdnError):
            opt.step()
        with pytest.raises(GdnError):
            opt.state_dict()
        with pytest.raises(GdnError):
            opt.load_state_dict({})
    assert torch.equal(got, want), "%s: the exchanged model differs from a model built from the averages" % dtype
    assert not torch.equal(got, raw)
    with torch.no_grad():
        assert torch.equal(model(x, istrain=False), raw), "%s: the raw weights are not back" % dtype
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert opt._swapped is False


def test_creation_and_swap_refused_inside_a_capture(gpu):
    from gdn_amd._lib import GdnError
    p, opt = _loose(gpu, 64, ema_decay=DECAY)
    p.grad = torch.ones(64, device=gpu)
    q, done = _loose(gpu, 64, ema_decay=DECAY)
    q.grad = torch.ones(64, device=gpu)
    done.step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    errors, tick = [], torch.zeros(4, device=gpu)
    with torch.cuda.graph(g):
        tick.add_(1.0)                                     # (something to capture)
        for call in (opt.step, done.swap_averaged):
            try:
                call()
            except GdnError as e:
                errors.append(str(e))
    assert len(errors) == 2 and "capture" in errors[0] and "capture" in errors[1]
    assert done._swapped is False


@pytest.mark.parametrize("guard", [False, True])
def test_graphed_ema_step_matches_eager(gpu, base_model, batches, guard):
    """test_graphed_guarded_step_matches_eager with ema_decay, with and without the guard: losses, model state and every
    average after five replays are bitwise those of the eager loop."""
    from gdn_amd.graph import GraphedTrainStep
    kw = dict(ema_decay=DECAY)
    if guard:
        kw.update(max_grad_norm=40.0, skip_nonfinite=True)
    runs = {}
    for mode in ("eager", "graph"):
        model, opt = _model_and_opt(gpu, base_model, **kw)

        def step_fn(depth, sparse, model=model, opt=opt):
            return (_model_step(model, opt, (depth, None, sparse)),)

        if mode == "eager":
            for _ in range(3):
                step_fn(batches[0][0], batches[0][2])
            run = step_fn
        else:
            run = GraphedTrainStep(step_fn, (batches[0][0], batches[0][2]), opt, warmup=3)
        losses = []
        for i, (d, _, s) in enumerate(batches[1:]):
            if i == 3:
                for g in opt.param_groups:
                    g["lr"] = g["lr"] * 0.5
            losses.append(float(run(d, s)[0]))
        runs[mode] = (losses, {k: v.clone() for k, v in model.state_dict().items()}, opt.state_dict(),
                      [p.detach().clone() for p in model.parameters()])
    (la, ma, oa, pa), (lb, mb, ob, _) = runs["eager"], runs["graph"]
    assert la == lb
    for k, v in ma.items():
        assert torch.equal(v, mb[k]), k
    assert oa["gdn"]["ema"]["decay"] == ob["gdn"]["ema"]["decay"] == DECAY
    assert sorted(oa["gdn"]["ema"]["avg"]) == sorted(ob["gdn"]["ema"]["avg"]) == list(range(len(pa)))
    for k, a in oa["gdn"]["ema"]["avg"].items():
        assert torch.equal(a, ob["gdn"]["ema"]["avg"][k]), "average %d" % k
        if pa[k].dim() == 4:
            assert not torch.equal(a.cpu(), pa[k].cpu()), "average %d equals the weights after eight steps" % k
    for ra, rb in zip(oa["gdn"]["stores"], ob["gdn"]["stores"]):
        assert torch.equal(ra["state"], rb["state"])
    if guard:
        assert oa["gdn"]["guard"] == ob["gdn"]["guard"] and oa["gdn"]["guard"]["steps"] == 8


def test_resume_continues_bitwise(gpu, base_model, batches, tmp_path):
    """4 steps == 2 steps, the training state written and read back through trainer.save_training_state /
    read_training_state (the weights_only loader) / load_training_state into a fresh model and optimizer, 2 more; every
    average included."""
    from gdn_amd import trainer as T
    model, opt = _model_and_opt(gpu, base_model, ema_decay=DECAY)
    for k in range(4):
        _model_step(model, opt, batches[k])
    first, opt1 = _model_and_opt(gpu, base_model, ema_decay=DECAY)
    for k in range(2):
        _model_step(first, opt1, batches[k])
    path = T.save_training_state(str(tmp_path / "train_state.pt"), first, opt1, None, {"step": 2})
    state = T.read_training_state(path)
    saved = state["optimizer"]["gdn"]["ema"]
    assert saved["decay"] == DECAY and len(saved["avg"]) == len(list(first.parameters()))
    second, opt2 = _model_and_opt(gpu, base_model, ema_decay=DECAY)
    assert T.load_training_state(state, second, opt2, None)["step"] == 2
    handed_back = opt2.state_dict()["gdn"]["ema"]["avg"]          # before the stores exist
    for k, a in saved["avg"].items():
        assert torch.equal(handed_back[k].cpu(), a), k
    for k in range(2, 4):
        _model_step(second, opt2, batches[k])
    for (k, a), b in zip(model.state_dict().items(), second.state_dict().values()):
        assert torch.equal(a, b), k
    sa, sb = opt.state_dict(), opt2.state_dict()
    for k, s in sa["state"].items():
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(s[name], sb["state"][k][name]), (k, name)
    for k, a in sa["gdn"]["ema"]["avg"].items():
        assert torch.equal(a, sb["gdn"]["ema"]["avg"][k]), "average %d" % k
    # stores that exist are rewritten in place
    opt2.load_state_dict(state["optimizer"])
    again = opt2.state_dict()["gdn"]["ema"]["avg"]
    for k, a in saved["avg"].items():
        assert torch.equal(again[k].cpu(), a), k


# ---------------------------------------------------------------------------------------------------------------------
def _cli(cwd, argv, limit=240):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([str(REPO / "gdn-pytorch_amd"), str(REPO)] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    cwd.mkdir(parents=True, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "gdn_amd.GDN_main", *argv]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(cwd), timeout=limit + 60)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def test_command_line(gpu, tmp_path, base_model):
    """One fresh child process per run.  --ema_decay writes X.pkl and X_ema.pkl whose tensors differ, load_checkpoint reads
    the second, and the validation line says which weights it ran on; the plain run writes and prints neither."""
    from gdn_amd.trainer import load_checkpoint
    base = ["--synthetic", "--mode", "DtoD", "--height", "32", "--width", "64", "--batch_size", "2", "--epochs", "1",
            "--epoch_size", "3", "--gpu_num", "0", "--evaluate"]
    out = _cli(tmp_path / "ema", base + ["--ema_decay", "0.9"])
    files = sorted((tmp_path / "ema").rglob("*.pkl"))
    ema_files = [f for f in files if f.name.endswith("_ema.pkl")]
    raw_files = [f for f in files if not f.name.endswith("_ema.pkl")]
    assert len(ema_files) == 1 and len(raw_files) == 1, files
    assert ema_files[0].name == raw_files[0].name[:-4] + "_ema.pkl"
    raw, avg = torch.load(raw_files[0], map_location="cpu"), torch.load(ema_files[0], map_location="cpu")
    assert list(raw) == list(avg) and all(k.startswith("module.") for k in avg)
    names = {n for n, _ in base_model.named_parameters()}
    for k in raw:
        if k[7:] in names:
            assert not torch.equal(raw[k], avg[k]), "%s: the averaged file holds the raw weights" % k
        else:
            assert torch.equal(raw[k], avg[k]), "%s: a buffer differs" % k
    loaded = load_checkpoint(copy.deepcopy(base_model), str(ema_files[0])).state_dict()
    assert all(torch.equal(v, avg["module." + k]) for k, v in loaded.items())
    lines = [l for l in out.splitlines() if "* Avg" in l]
    assert len(lines) == 1 and lines[0].startswith("(averaged weights) * Avg"), out[-2000:]
    plain = _cli(tmp_path / "plain", base)
    assert not list((tmp_path / "plain").rglob("*_ema.pkl")) and len(list((tmp_path / "plain").rglob("*.pkl"))) == 1
    assert "(averaged weights)" not in plain and len([l for l in plain.splitlines() if l.startswith(" * Avg")]) == 1
