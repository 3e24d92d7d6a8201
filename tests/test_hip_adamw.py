"""Decoupled weight decay on the GPU: the four gdn_adamw_step* entry points against their coupled siblings,
against each other and against the float32 restatement (tests/adamw_fp64.py), all by bit identity; Adam(decoupled=True) against
torch.optim.AdamW, its launch count and what it must leave alone; and --optimizer adamw end to end through GDN_main.run at the
smallest model shapes (16 x 32, batch 2, 3 batches per epoch) with --graph, --resume and the other fine-tuning flags."""
import copy
import os
import shutil

import numpy as np
import pytest
import torch

import adamw_fp64 as R
from libcalls import count_library_calls
from oracle import gdn_oracle as O
from test_hip_kernels import close
from test_hip_seg_adam import SKIP, _arena, _bits, _guard, _layout, _same_bits, _state

pytestmark = pytest.mark.gpu

# (lr, beta1, beta2, eps, wd, grad_scale): a rate and a decay at which a wrong contraction shows, the project's own, and a
# third with other betas; hyper[5] is the optimizer's, one value
GROUPS = [(0.5, 0.9, 0.999, 1e-8, 0.3, 0.5), (2e-5, 0.9, 0.999, 1e-8, 1e-2, 0.5), (3e-3, 0.8, 0.99, 1e-6, 5e-4, 0.5)]
N_RANGE = 1000
# a 4096-float arena: 16 + 10 + 24 + 2 + 11 + 1 chunks
SIZES = [1000, 640, 1500, 65, 700, 64]
GROUP_OF = [0, SKIP, 1, 2, 0, SKIP]
STEPS = 3


def _f(x):
    return float(np.float32(x))


def _no_decay(groups):
    return [g[:4] + (0.0,) + g[5:] for g in groups]


def _range(gpu, seed, zero=False):
    """p, g, m, v: 1000 floats each, starting one float past a 16-byte boundary."""
    rng = np.random.default_rng(seed)
    out = []
    for scale, positive in ((1.0, False), (1e-2, False), (1e-3, False), (1e-6, True)):
        x = rng.standard_normal(N_RANGE).astype(np.float32) * np.float32(scale)
        buf = torch.zeros(N_RANGE + 8, dtype=torch.float32, device=gpu)
        assert buf.data_ptr() % 16 == 0
        view = buf[1:1 + N_RANGE]
        view.copy_(torch.from_numpy(np.abs(x) if positive else x))
        out.append(view)
    if zero:
        for t in out[1:]:
            t.zero_()
    return out


def _run_range(form, bufs, row, gpu, coupled=False, steps=STEPS, coef=1.0, skip=0):
    """`steps` updates of clones of `bufs` by one entry point; returns (p, m, v, step-state bytes or None)."""
    from gdn_amd import ops
    p, g, m, v = (t.clone() for t in bufs)
    # (a clone of a view is dense and 16-byte aligned: put the offset back)
    hold = [torch.zeros(N_RANGE + 8, dtype=torch.float32, device=gpu) for _ in range(4)]
    for h, t in zip(hold, (p, g, m, v)):
        h[1:1 + N_RANGE].copy_(t)
    p, g, m, v = (h[1:1 + N_RANGE] for h in hold)
    assert all(t.data_ptr() % 16 == 4 for t in (p, g, m, v))
    lr, b1, b2, eps, wd, gs = row
    hyper = torch.tensor(row, dtype=torch.float32, device=gpu)
    state = _state(gpu, 0, b1, b2)
    guard = _guard(gpu, coef=coef, skip=skip)
    name = ("adam_" if coupled else "adamw_") + form
    for t in range(1, steps + 1):
        if form == "step":
            getattr(ops, name)(p, g, m, v, _f(lr), _f(b1), _f(b2), _f(eps), _f(wd), t, _f(gs))
        elif form == "step_dev":
            getattr(ops, name)(p, g, m, v, hyper, state)
        else:
            getattr(ops, name)(p, g, m, v, hyper, state, guard)
    torch.cuda.synchronize()
    assert not any(h[0].item() or h[1 + N_RANGE:].any().item() for h in hold), "written outside the range"
    return p, m, v, None if form == "step" else state.cpu()


def _run_arena(gpu, groups, coupled=False, guard=None, steps=STEPS, seed=7, zero=False):
    """`steps` segmented updates of the arena; returns (before, after) as lists [p, g, m, v], the chunk map and the states."""
    from gdn_amd import ops
    items, n, cmap = _layout(SIZES, GROUP_OF)
    assert n == 4096
    p, g, m, v, _ = _arena(gpu, n, cmap, items, seed)
    if zero:
        live = torch.from_numpy(np.repeat(cmap != SKIP, 64)).to(gpu)
        for t in (g, m, v):
            t[live] = 0.0
    before = [t.clone() for t in (p, g, m, v)]
    dmap = torch.from_numpy(cmap).to(gpu)
    hyper = torch.tensor(groups, dtype=torch.float32, device=gpu)
    states = torch.cat([_state(gpu, 0, gr[1], gr[2]) for gr in groups])
    for _ in range(steps):
        (ops.adam_step_seg if coupled else ops.adamw_step_seg)(p, g, m, v, dmap, hyper, states, guard)
    torch.cuda.synchronize()
    skipped = torch.from_numpy(np.repeat(cmap == SKIP, 64))
    for t, b in zip((p, g, m, v), before):
        assert torch.equal(_bits(t)[skipped], _bits(b)[skipped]), "a skipped chunk was written"
    assert _same_bits(g, before[1])
    return before, [p, g, m, v], (items, cmap), states.cpu()


def _live(items):
    return [(o, k, grp) for (o, k), grp in zip(items, GROUP_OF) if grp != SKIP]


# ---- kernel level ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["step", "step_dev", "step_dev_guarded"])
def test_range_without_decay_is_the_coupled_sibling_and_the_moments_never_see_the_decay(gpu, form):
    """wd = 0: p, m, v and the step state bit-identical to the coupled entry point's.  wd > 0: m and v are still those bits
    (the decay is not in the gradient), p is not."""
    for k, row in enumerate(GROUPS):
        bufs = _range(gpu, 20 + k)
        zero = _no_decay([row])[0]
        want = _run_range(form, bufs, zero, gpu, coupled=True, coef=0.37)
        got = _run_range(form, bufs, zero, gpu, coef=0.37)
        for name, a, b in zip("pmv", got, want):
            assert _same_bits(a, b), (form, k, name)
        assert form == "step" or torch.equal(got[3], want[3])
        dec = _run_range(form, bufs, row, gpu, coef=0.37)
        assert _same_bits(dec[1], want[1]) and _same_bits(dec[2], want[2]), (form, k, "moments")
        assert not _same_bits(dec[0], want[0]), (form, k, "the decay changed nothing")


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
def test_arena_without_decay_is_the_coupled_sibling_and_the_moments_never_see_the_decay(gpu, guarded):
    guard = _guard(gpu, coef=0.37) if guarded else None
    _, want, (items, cmap), sw = _run_arena(gpu, _no_decay(GROUPS), coupled=True, guard=guard)
    _, got, _, sg = _run_arena(gpu, _no_decay(GROUPS), guard=guard)
    for name, a, b in zip("pgmv", got, want):
        assert _same_bits(a, b), name
    assert torch.equal(sg, sw)
    _, dec, _, sd = _run_arena(gpu, GROUPS, guard=guard)
    assert _same_bits(dec[2], want[2]) and _same_bits(dec[3], want[3]) and torch.equal(sd, sw)
    for o, k, grp in _live(items):
        assert not _same_bits(dec[0][o:o + k], want[0][o:o + k]), (o, "the decay changed nothing")


def test_zero_gradient_and_zero_moments_leave_the_decay_alone(gpu):
    """q = 0, so every step is p = pi - float32(dec * pi): one rounding of the product, one of the difference, whatever
    division and square root do.  All four entry points, three steps."""
    def want(p0, row):
        dec, p = R.dec32(row[0], row[4]), p0.copy()
        for _ in range(STEPS):
            p = p - R.fma32(dec, p, np.zeros_like(p))
        assert np.array_equal(p, _decayed(p0, dec))
        return p

    def _decayed(p0, dec):
        p = p0.copy()
        for _ in range(STEPS):
            p = p - (p.astype(np.float64) * float(dec)).astype(np.float32)         # (24 x 24 bits: exact in double)
        return p
    for k, row in enumerate(GROUPS):
        bufs = _range(gpu, 30 + k, zero=True)
        ref = want(bufs[0].cpu().numpy(), row)
        for form in ("step", "step_dev", "step_dev_guarded"):
            p, m, v, _ = _run_range(form, bufs, row, gpu)
            assert p.cpu().numpy().tobytes() == ref.tobytes(), (form, k)
            assert not m.any() and not v.any()
    before, after, (items, cmap), _ = _run_arena(gpu, GROUPS, zero=True)
    for o, k, grp in _live(items):
        ref = want(before[0][o:o + k].cpu().numpy(), GROUPS[grp])
        assert after[0][o:o + k].cpu().numpy().tobytes() == ref.tobytes(), (o, grp)
    # at (0.5, 0.3) the weights shrank by 0.85 a step; at the project's rate dec = 2e-7 moved the larger of them
    assert not _same_bits(after[0][:1000], before[0][:1000])


def _range_entry_points_agree(gpu, coupled):
    """On the misaligned range: host count, device count and guarded with coef 1, per group."""
    for k, row in enumerate(GROUPS):
        bufs = _range(gpu, 40 + k)
        a = _run_range("step", bufs, row, gpu, coupled=coupled)
        b = _run_range("step_dev", bufs, row, gpu, coupled=coupled)
        c = _run_range("step_dev_guarded", bufs, row, gpu, coupled=coupled, coef=1.0)
        for name, x, y, z in zip("pmv", a, b, c):
            assert _same_bits(x, y) and _same_bits(y, z), (k, name)
        assert torch.equal(b[3], c[3])


def test_the_coupled_entry_points_agree_on_the_range(gpu):
    """gdn_adam_step, gdn_adam_step_dev and gdn_adam_step_dev_guarded at the decays of GROUPS (the arena against the
    per-slice update is tests/test_hip_seg_adam.py's)."""
    _range_entry_points_agree(gpu, coupled=True)


def test_the_four_entry_points_agree(gpu):
    """The range as above.  On the arena: every live slice of the segmented update against the per-slice update with the
    group's records, plain and under a guard (coef 0.37)."""
    from gdn_amd import ops
    _range_entry_points_agree(gpu, coupled=False)
    for guarded in (False, True):
        guard = _guard(gpu, coef=0.37) if guarded else None
        before, after, (items, cmap), states = _run_arena(gpu, GROUPS, guard=guard)
        hyper = torch.tensor(GROUPS, dtype=torch.float32, device=gpu)
        for o, k, grp in _live(items):
            p, g, m, v = (t[o:o + k].clone() for t in before)
            st = _state(gpu, 0, GROUPS[grp][1], GROUPS[grp][2])
            for _ in range(STEPS):
                if guarded:
                    ops.adamw_step_dev_guarded(p, g, m, v, hyper[grp], st, guard)
                else:
                    ops.adamw_step_dev(p, g, m, v, hyper[grp], st)
            for name, x, y in (("p", p, after[0]), ("m", m, after[2]), ("v", v, after[3])):
                assert _same_bits(x, y[o:o + k]), (guarded, o, grp, name)
            assert torch.equal(st.cpu()[:28], states[32 * grp:32 * grp + 28])
            pad = slice(o + k, o + -(-k // 64) * 64)
            assert not any(t[pad].any() for t in (after[0], after[2], after[3])), "padding of the slice at %d moved" % o


# The bar of the restatement test, in float32 ulps: 0 = bit for bit, which holds where the device's divide and square root are
# correctly rounded.
RESTATEMENT_ULPS = 0


def test_against_the_float32_restatement(gpu):
    """The full update, three steps from t = 0: the range through gdn_adamw_step_dev per group, the arena through
    gdn_adamw_step_seg under a guard (coef 0.37).  Every figure is printed before it is held to the bar."""
    _against_the_float32_restatement(gpu, coupled=False)


def test_coupled_against_the_float32_restatement(gpu):
    """The same for the coupled family, gdn_adam_step_dev and gdn_adam_step_seg, against the restatement's coupled form
    (gi = fma32(wd, p, round32(g * gscale)), no decay in the final subtraction): the bits of the main training path."""
    _against_the_float32_restatement(gpu, coupled=True)


def _against_the_float32_restatement(gpu, coupled):
    worst = {"n": 0, "off": 0, "ulps": 0}

    def hold(name, got, want):
        d = R.ulps32(got, want)
        worst["n"] += d.size
        worst["off"] += int(np.count_nonzero(d))
        worst["ulps"] = max(worst["ulps"], int(d.max()))
        print("%-28s %5d elements, %d not the restatement's bits, largest distance %d ulp" % (name, d.size, np.count_nonzero(d), d.max()))

    for k, row in enumerate(GROUPS):
        bufs = _range(gpu, 50 + k)
        got = _run_range("step_dev", bufs, row, gpu, coupled=coupled)
        want = R.run32(*(t.cpu().numpy() for t in bufs), row, STEPS, coupled=coupled)
        for name, a, b in zip("pmv", got, want):
            hold("range group %d %s" % (k, name), a.cpu().numpy(), b)
        assert got[3].numpy().tobytes()[:28] == R.state_bytes(row[1], row[2], STEPS)[:28]
    before, after, (items, cmap), _ = _run_arena(gpu, GROUPS, coupled=coupled, guard=_guard(gpu, coef=0.37))
    host = [t.cpu().numpy() for t in before]
    for o, k, grp in _live(items):
        sl = slice(o, o + k)
        want = R.run32(host[0][sl], host[1][sl], host[2][sl], host[3][sl], GROUPS[grp], STEPS, coef=0.37, coupled=coupled)
        for name, a, b in zip("pmv", (after[0], after[2], after[3]), want):
            hold("arena slice %d group %d %s" % (o, grp, name), a[sl].cpu().numpy(), b)
    print("in all: %d of %d elements not the restatement's bits, largest distance %d ulp" % (worst["off"], worst["n"], worst["ulps"]))
    assert worst["ulps"] <= RESTATEMENT_ULPS


def test_a_skipped_step_touches_nothing(gpu):
    from gdn_amd import ops
    bufs = _range(gpu, 60)
    for row in GROUPS:
        p, m, v, state = _run_range("step_dev_guarded", bufs, row, gpu, coef=0.0, skip=1)
        assert _same_bits(p, bufs[0]) and _same_bits(m, bufs[2]) and _same_bits(v, bufs[3])
        assert torch.equal(state, _state(torch.device("cpu"), 0, row[1], row[2]))
    before, after, _, states = _run_arena(gpu, GROUPS, guard=_guard(gpu, coef=0.0, skip=1))
    for a, b in zip(after, before):
        assert _same_bits(a, b)
    assert torch.equal(states, torch.cat([_state(torch.device("cpu"), 0, gr[1], gr[2]) for gr in GROUPS]))


def test_bad_arguments(gpu):
    from gdn_amd import ops
    from gdn_amd._lib import GdnError, lib
    n = 256
    buf = torch.zeros(n + 64, dtype=torch.float32, device=gpu)
    p, g, m, v = (buf[:n].clone() for _ in range(4))
    cmap = torch.zeros(n // 64, dtype=torch.uint8, device=gpu)
    hyper = torch.tensor(GROUPS[:1], dtype=torch.float32, device=gpu)
    states, guard = _state(gpu, 0), _guard(gpu)
    P = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def host(p=p, g=g, m=m, v=v, n=n, step=1):
        lib.gdn_adamw_step(P(p), P(g), P(m), P(v), n, 0.5, 0.9, 0.999, 1e-8, 0.3, step, 1.0, None)

    def dev(p=p, g=g, m=m, v=v, n=n, hyper=hyper, state=states):
        lib.gdn_adamw_step_dev(P(p), P(g), P(m), P(v), n, P(hyper), P(state), None)

    def guarded(p=p, g=g, m=m, v=v, n=n, hyper=hyper, state=states, guard=guard):
        lib.gdn_adamw_step_dev_guarded(P(p), P(g), P(m), P(v), n, P(hyper), P(state), P(guard), None)

    def seg(p=p, g=g, m=m, v=v, n=n, cmap=cmap, G=1, hyper=hyper, states=states):
        lib.gdn_adamw_step_seg(P(p), P(g), P(m), P(v), n, P(cmap), G, P(hyper), P(states), None, None)

    odd = buf[1:1 + n]
    common = (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(n=-64))
    bad = [("gdn_adamw_step", host, kw) for kw in common + (dict(step=0),)]
    bad += [("gdn_adamw_step_dev", dev, kw) for kw in common + (dict(hyper=None), dict(state=None))]
    bad += [("gdn_adamw_step_dev_guarded", guarded, kw) for kw in common + (dict(hyper=None), dict(state=None), dict(guard=None))]
    bad += [("gdn_adamw_step_seg", seg, kw) for kw in common + (
        dict(cmap=None), dict(hyper=None), dict(states=None), dict(n=n - 1), dict(G=0), dict(G=255), dict(p=odd), dict(g=odd),
        dict(m=odd), dict(v=odd))]
    for name, fn, kw in bad:
        with pytest.raises(GdnError, match=name + " failed: bad argument"):
            fn(**kw)
    torch.cuda.synchronize()
    assert not buf.any() and not p.any() and not m.any() and not v.any()
    assert torch.equal(states.cpu(), _state(torch.device("cpu"), 0))
    with pytest.raises(GdnError, match="chunk map"):
        ops.adamw_step_seg(p, g, m, v, cmap[:-1], hyper, states)
    with pytest.raises(GdnError, match="step states"):
        ops.adamw_step_seg(p, g, m, v, cmap, hyper, torch.cat([states, states]))


# ---- optimizer level ---------------------------------------------------------------------------------------------------------
H, W = 16, 32
NET = "AutoEncoder_DtoD"
OPT_CALLS = ("gdn_adam_step", "gdn_adam_step_dev", "gdn_adam_step_dev_guarded", "gdn_grad_sumsq", "gdn_grad_guard_finalize",
             "gdn_ema_update", "gdn_adam_step_seg", "gdn_grad_sumsq_seg", "gdn_ema_update_seg", "gdn_lr_schedule",
             "gdn_adamw_step", "gdn_adamw_step_dev", "gdn_adamw_step_dev_guarded", "gdn_adamw_step_seg")


@pytest.fixture(scope="module")
def base():
    """One seeded network on the CPU, never modified (every case works on a deep copy)."""
    import gdn_amd.AE_model_unet as M
    torch.manual_seed(11)
    return M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)


@pytest.fixture(scope="module")
def batches(gpu):
    return [[t.to(gpu) for t in O.synthetic_batch(2, H, W, seed=70 + i)] for i in range(3)]


def _model(base, gpu, freeze=("encoder",)):
    m = copy.deepcopy(base).to(gpu).compute_dtype("fp32").train()
    if freeze:
        m.freeze(list(freeze))
    return m


def _groups(model):
    """gamma / beta without decay at half the rate, everything else."""
    named = list(model.named_parameters())
    return [{"params": [p for n, p in named if p.dim() != 1]},
            {"params": [p for n, p in named if p.dim() == 1], "lr_mult": 0.5, "weight_decay": 0.0}]


def _adamw(model, plain=False, **kw):
    from gdn_amd.optim import Adam
    return Adam(model.parameters() if plain else _groups(model), 2e-4, [0.9, 0.999], eps=1e-08, weight_decay=1e-2,
                decoupled=kw.pop("decoupled", True), **kw)


def _fwd_bwd(model, batch):
    from gdn_amd import utils as U
    depth, rgb, sparse = batch
    out = model(depth, istrain=False)
    loss, _, _ = U.dtod_loss(out, depth, sparse)
    for p in model.parameters():
        p.grad = None
    loss.backward()
    return loss.detach()


@pytest.mark.parametrize("form", ["plain", "segmented"])
def test_optimizer_matches_torch_adamw(gpu, base, batches, form):
    """torch.optim.AdamW on the CPU over the same groups at lr * lr_mult, fed the gradients of the HIP model; the bars of
    test_segmented_matches_torch_adam.  Segmented: the encoder is frozen and keeps its bits."""
    seg = form == "segmented"
    m = _model(base, gpu, freeze=("encoder",) if seg else ())
    init = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = _adamw(m, plain=not seg, segmented=seg)
    theirs = {n: torch.nn.Parameter(p.detach().cpu().clone(), requires_grad=p.requires_grad) for n, p in m.named_parameters()}
    by_id = {id(p): n for n, p in m.named_parameters()}
    ref = torch.optim.AdamW([{"params": [theirs[by_id[id(p)]] for p in g["params"]], "lr": 2e-4 * g.get("lr_mult", 1.0),
                              "weight_decay": g["weight_decay"]} for g in opt.param_groups], betas=(0.9, 0.999), eps=1e-8)
    for batch in batches:
        _fwd_bwd(m, batch)
        for n, p in m.named_parameters():
            theirs[n].grad = None if p.grad is None else p.grad.detach().cpu().clone()
        opt.step()
        ref.step()
    for n, p in m.named_parameters():
        close(p, theirs[n], rtol=1e-5, atol_scale=1e-6, what="%s AdamW vs torch, %s" % (form, n))
    st = opt.store_of(m._gdn_param_arena)
    assert (st.plan is not None) == seg and (st.pstep is None) != seg
    frozen = set(m.select_parameters("encoder")) if seg else set()
    for n, p in m.named_parameters():
        if n in frozen:
            assert torch.equal(_bits(p), _bits(init[n])), n
        elif p.dim() != 1:
            assert not torch.equal(p, init[n]), n


def test_launch_count_is_the_coupled_optimizers(gpu, base, batches):
    """Guarded, averaged, scheduled, frozen encoder, two groups: the same entry points as often, gdn_adamw_step_seg in
    gdn_adam_step_seg's place."""
    kw = dict(segmented=True, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.99,
              schedule={"kind": "cosine", "warmup": 1, "total": 4, "floor": 0.1})
    seen = {}
    for decoupled in (False, True):
        m = _model(base, gpu)
        opt = _adamw(m, decoupled=decoupled, **kw)
        seen[decoupled] = []
        for batch in batches[:2]:
            _fwd_bwd(m, batch)
            every, order = count_library_calls(opt.step)
            seen[decoupled].append([name for name in order if name in OPT_CALLS])
    assert seen[False][1] == ["gdn_grad_sumsq_seg", "gdn_grad_guard_finalize", "gdn_lr_schedule", "gdn_adam_step_seg", "gdn_ema_update_seg"]
    assert seen[True] == [[n.replace("gdn_adam_step_seg", "gdn_adamw_step_seg") for n in step] for step in seen[False]]


def test_a_parameter_without_a_gradient_is_not_decayed(gpu, base, batches):
    """Like torch: the parameter that sat out keeps its bits, decay or not; the others run per tensor."""
    m = _model(base, gpu, freeze=())
    opt = _adamw(m, plain=True)
    named = list(m.named_parameters())
    out_n, out_p = next((n, p) for n, p in named if p.dim() == 4)
    before = {n: p.detach().clone() for n, p in named}
    _fwd_bwd(m, batches[0])
    out_p.grad = None
    every, order = count_library_calls(opt.step)
    assert every["gdn_adamw_step"] == len(named) - 1 and not every["gdn_adam_step"]
    assert torch.equal(_bits(out_p), _bits(before[out_n]))
    assert all(not torch.equal(p, before[n]) for n, p in named if p.dim() == 4 and n != out_n)


def test_per_tensor_fallback_is_bitwise_the_one_launch_path(gpu, base, batches):
    """Frozen encoder, two groups, three steps: segmented (one launch) against unsegmented (one launch per tensor)."""
    ma, mb = _model(base, gpu), _model(base, gpu)
    oa, ob = _adamw(ma, segmented=True), _adamw(mb, segmented=False)
    counts = []
    for batch in batches:
        la, lb = _fwd_bwd(ma, batch), _fwd_bwd(mb, batch)
        assert torch.equal(la, lb)
        counts.append((count_library_calls(oa.step)[0], count_library_calls(ob.step)[0]))
    assert all(a["gdn_adamw_step_seg"] == 1 and b["gdn_adamw_step"] > 20 for a, b in counts)
    sa, sb = ma.state_dict(), mb.state_dict()
    assert list(sa) == list(sb)
    for k in sa:                       # (num_batches_tracked is an integer)
        assert torch.equal(_bits(sa[k]) if sa[k].dtype == torch.float32 else sa[k], _bits(sb[k]) if sb[k].dtype == torch.float32 else sb[k]), k
    da, db = oa.state_dict(), ob.state_dict()
    assert sorted(da["state"]) == sorted(db["state"])
    for k in da["state"]:
        for f in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(_bits(da["state"][k][f]), _bits(db["state"][k][f])), (k, f)


# ---- the flags, end to end -----------------------------------------------------------------------------------------------
_RUNS = {}
ADAMW = ["--optimizer", "adamw"]
COMBO = ["--lr_schedule", "cosine", "--warmup_steps", "2", "--lr_mult", "encoder=0.1", "--no_decay_norm", "--ema_decay", "0.9",
         "--clip_grad_norm", "1", "--skip_nonfinite"]


class _Stop(Exception):
    pass


@pytest.fixture(scope="module")
def loop_root(tmp_path_factory, base):
    root = tmp_path_factory.mktemp("adamw")
    torch.save({"module." + k: v.contiguous() for k, v in base.state_dict().items()}, str(root / "init.pkl"))
    yield root
    # the runs of this file hold their files in memory (_run) and leave nothing on the disk the rest of the suite shares
    _RUNS.clear()
    shutil.rmtree(root, ignore_errors=True)


def _run(root, tag, dtype, extra, init=True, stop_after_first_state=False, spy=None):
    """GDN_main.run in `root`/<dtype>_<tag> (cached): {file name: tensors of every .pkl written}, the files themselves
    deleted once they are read (60 MB each; a train_state.pt stays for the test that resumes from it).
    stop_after_first_state: the run dies right after its first train_state.pt is on disk (the end of epoch 1 under
    --save_state), as a kill would end it."""
    from gdn_amd import GDN_main, option
    from gdn_amd import trainer as T
    key = (dtype, tag)
    if key in _RUNS:
        return _RUNS[key]
    where = root / ("%s_%s" % (dtype, tag))
    where.mkdir(parents=True, exist_ok=True)
    argv = ["synthetic", "--synthetic", "--mode", "DtoD", "--height", str(H), "--width", str(W), "--batch_size", "2",
            "--epoch_size", "3", "--epochs", "2", "--gpu_num", "0", "--dtype", dtype, "-e"]
    if init:
        argv += ["--init_from", str(root / "init.pkl")]
    cwd, save, make = os.getcwd(), T.save_training_state, GDN_main._make_optimizer

    def save_and_stop(*a, **k):
        save(*a, **k)
        raise _Stop()

    def make_and_show(model, args):
        opt = make(model, args)
        spy.append(opt)
        return opt
    os.chdir(where)
    try:
        if stop_after_first_state:
            T.save_training_state = save_and_stop
        if spy is not None:
            GDN_main._make_optimizer = make_and_show
        GDN_main.run(option.parse_args(argv + list(extra)))
        assert not stop_after_first_state, "the run wrote no training state"
    except _Stop:
        pass
    finally:
        T.save_training_state, GDN_main._make_optimizer = save, make
        os.chdir(cwd)
    torch.cuda.synchronize()
    files = [p for p in sorted(where.rglob("*.pkl")) if p.name != "init.pkl"]
    _RUNS[key] = {p.name: torch.load(p, map_location="cpu") for p in files}
    for p in files:
        p.unlink()
    return _RUNS[key]


def _same_files(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
    for name in a:
        assert list(a[name]) == list(b[name])
        for k in a[name]:
            assert torch.equal(a[name][k], b[name][k]), (what, name, k)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loop_graph_is_bitwise(gpu, loop_root, dtype, capsys):
    spy, fresh = [], (dtype, "base") not in _RUNS
    base_run = _run(loop_root, "base", dtype, ADAMW, spy=spy)
    assert len(base_run) == 2
    if fresh:                          # (another test of this file may have made the run already)
        assert "=> optimizer: AdamW, decoupled weight decay 0.01" in capsys.readouterr().out
        assert spy[0].decoupled and not spy[0].capturable and spy[0].defaults["weight_decay"] == 1e-2
    _same_files(base_run, _run(loop_root, "graph", dtype, ADAMW + ["--graph", "--graph_warmup", "2"]), "--graph")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loop_adam_is_the_run_without_the_flag_and_adamw_is_not(gpu, loop_root, dtype):
    spy = []
    plain = _run(loop_root, "plain", dtype, [])
    adam = _run(loop_root, "adam", dtype, ["--optimizer", "adam"], spy=spy)
    _same_files(plain, adam, "--optimizer adam")
    assert not spy[0].decoupled and not spy[0].capturable and spy[0].defaults["weight_decay"] == 5e-4
    base_run = _run(loop_root, "base", dtype, ADAMW)
    assert sorted(k.split("_loss_")[0] for k in base_run) == sorted(k.split("_loss_")[0] for k in plain)
    a, b = (sorted(r.items())[0][1] for r in (base_run, plain))
    assert any(not torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loop_resume_is_bitwise_and_the_other_optimizer_is_refused(gpu, loop_root, dtype):
    from gdn_amd._lib import GdnError
    base_run = _run(loop_root, "base", dtype, ADAMW)
    stopped = _run(loop_root, "stopped", dtype, ADAMW + ["--save_state"], stop_after_first_state=True)
    (state,) = sorted((loop_root / ("%s_stopped" % dtype)).rglob("train_state.pt"))
    saved = torch.load(state, map_location="cpu", weights_only=True)
    assert saved["optimizer"]["gdn"]["decoupled"] is True and saved["optimizer"]["param_groups"][0]["weight_decay"] == 1e-2
    assert (saved["epoch"], saved["i"], saved["step"]) == (1, -1, 3)
    resumed = _run(loop_root, "resumed", dtype, ADAMW + ["--resume", str(state)], init=False)
    assert len(stopped) == 1 and len(resumed) == 1
    _same_files({k: v for k, v in base_run.items() if k in stopped}, stopped, "epoch 1")
    _same_files({k: v for k, v in base_run.items() if k not in stopped}, resumed, "--resume")
    for k, other in enumerate(([], ["--optimizer", "adam"])):
        spy = []
        with pytest.raises(GdnError, match="written under --optimizer adamw, this run has --optimizer adam"):
            _run(loop_root, "refused%d" % k, dtype, other + ["--resume", str(state)], init=False, spy=spy)
        assert len(spy) == 1 and not spy[0]._stores                      # before any step
        assert not list((loop_root / ("%s_refused%d" % (dtype, k))).rglob("*.pkl"))
    state.unlink()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loop_with_the_other_fine_tuning_flags_is_bitwise_under_graph(gpu, loop_root, dtype):
    spy = []
    eager = _run(loop_root, "combo", dtype, ADAMW + COMBO, spy=spy)
    assert len(eager) == 4 and sum(n.endswith("_ema.pkl") for n in eager) == 2
    _same_files(eager, _run(loop_root, "combo_graph", dtype, ADAMW + COMBO + ["--graph", "--graph_warmup", "2"]), "--graph")
    (opt,) = spy
    assert opt.decoupled and opt.segmented and opt.guarded
    # --no_decay_norm: the 1-D parameters at 0, everything else at the default 1e-2; the encoder at a tenth of the rate
    assert sorted({(g["weight_decay"], all(p.dim() == 1 for p in g["params"])) for g in opt.param_groups}) == [(0.0, True), (1e-2, False)]
    assert sorted({g.get("lr_mult", 1.0) for g in opt.param_groups}) == [0.1, 1.0]
    assert opt.guard_stats()["steps"] == 6 and opt.guard_stats()["skipped"] == 0
