"""The device-side learning-rate schedule on the GPU: gdn_lr_schedule against its plain-double restatement
(tests/lr_schedule_fp64.py), Adam(schedule=...) against a twin optimizer that is handed the very rates current_lr() reports,
skipped steps, the reference's decay underneath it, a captured step, and the flags end to end through GDN_main.run at the
smallest model shapes (16 x 32, batch 2, 3 batches per epoch)."""
import copy
import os

import numpy as np
import pytest
import torch

import lr_schedule_fp64 as R

pytestmark = pytest.mark.gpu

H, W = 16, 32
LR = 2e-4
TS = lambda w, total: [0, w - 1, w, w + 1, total - 1, total, total + 7]      # noqa: E731
BASES = [2e-5, 1e-4 * 0.5, 0.0]


# ---- the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3, 254])
def test_kernel_against_the_restatement(gpu, G):
    """Every (t, base_lr) pair of the issue in every group position: constant and linear bit for bit, cosine within one float32
    ulp (the device's double cos differs from the host's by double ulps, which a float32 rounding all but never sees: the count
    of inexact values is printed and expected to be 0); the other five fields of every row and the step states untouched."""
    from gdn_amd import ops
    gen = torch.Generator().manual_seed(G)
    inexact = checked = 0
    for warmup, total in [(3, 8), (1, 2), (0, 5), (100, 1000)]:
        ts = TS(warmup, total)
        for kind in R.KINDS:
            for floor in (0.0, 0.1):
                for r in range(21 if G < 21 else 1):             # group k of round r takes pair number k + r of the 7 x 3
                    t = [max(0, ts[(k + r) % 7]) for k in range(G)]
                    base = [BASES[((k + r) // 7) % 3] for k in range(G)]
                    hyper0 = torch.randn(G, 6, generator=gen)
                    states0 = torch.frombuffer(bytearray(b"".join(R.state_bytes(x) for x in t)), dtype=torch.uint8)
                    hyper, states = hyper0.to(gpu), states0.to(gpu)
                    ops.lr_schedule(hyper, torch.tensor(base, dtype=torch.float64).to(gpu), states, kind, warmup, total, floor)
                    got = hyper.cpu()
                    assert torch.equal(got[:, 1:].view(torch.int32), hyper0[:, 1:].view(torch.int32))
                    assert torch.equal(states.cpu(), states0)
                    for k in range(G):
                        want = R.rate32(base[k], t[k], kind, warmup, total, floor)
                        have = np.float32(got[k, 0].item())
                        checked += 1
                        if kind != "cosine":
                            assert have.tobytes() == want.tobytes(), (kind, warmup, total, floor, t[k], base[k], have, want)
                        else:
                            inexact += have.tobytes() != want.tobytes()
                            assert abs(float(have) - float(want)) <= R.ulp32(want), (warmup, total, floor, t[k], base[k], have, want)
    print("G = %d: %d rates checked, %d cosine rates not the restatement's bits" % (G, checked, inexact))


def test_kernel_with_a_plain_28_byte_state(gpu):
    """The step state of a plain store is the 28 bytes optim._step_state packs (no tail padding): G = 1 reads it as it is."""
    from gdn_amd import ops
    from gdn_amd.optim import _step_state
    hyper = torch.zeros(6, device=gpu)
    state = _step_state({"betas": (0.9, 0.999)}, 4, gpu)
    assert state.numel() == 28
    ops.lr_schedule(hyper, torch.tensor([1e-4], dtype=torch.float64).to(gpu), state, "linear", 3, 8, 0.1)
    assert np.float32(hyper[0].item()) == R.rate32(1e-4, 4, "linear", 3, 8, 0.1) and not hyper[1:].any()


# ---- the optimizer ---------------------------------------------------------------------------------------------------------
HYPER = dict(lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
COSINE = {"kind": "cosine", "warmup": 3, "total": 8, "floor": 0.1}
LINEAR = {"kind": "linear", "warmup": 3, "total": 8, "floor": 0.1}


def _net(gpu, frozen=False):
    """Six small parameters in one arena of 384 floats (the net of tests/test_optim_segments_cpu.py)."""
    from gdn_amd import engine as E
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3), torch.nn.BatchNorm2d(3), torch.nn.ConvTranspose2d(3, 2, 3)).to(gpu)
    ar = E.ParamArena(net, gpu)
    net._gdn_param_arena = ar
    assert ar.intact() and ar.numel == 384
    for p in net.parameters():
        p.grad = ar.grad_view(p)
    if frozen:
        ps = list(net.parameters())
        ps[2].requires_grad_(False)
        ps[2].grad = None
    return net, ar


def _groups(net, rates=None):
    """conv weights and biases | BatchNorm gamma (frozen), beta at half the rate without decay; `rates`: the twin's form --
    the same two groups with their rates spelled out and no multiplier."""
    ps = list(net.parameters())
    a, b = {"params": [ps[0], ps[1], ps[4], ps[5]]}, {"params": [ps[2], ps[3]], "weight_decay": 0.0}
    if rates is None:
        b["lr_mult"] = 0.5
    else:
        a["lr"], b["lr"] = rates
    return [a, b]


def _grad(ar, k, scale=1.0):
    g = torch.randn(ar.numel, generator=torch.Generator().manual_seed(100 + k)) * scale
    ar.grad.copy_(g.to(ar.grad.device))


def _adam(form, net, **kw):
    from gdn_amd.optim import Adam
    if form == "plain":
        return Adam(net.parameters(), **HYPER, **kw)
    return Adam(_groups(net), **HYPER, segmented=True, **kw)


def _dev_state(opt, ar):
    """(weights, m, v, step-state bytes) of the arena's store, on the host."""
    st = opt.store_of(ar)
    states = st.plan.states if st.plan is not None else st.state
    return [t.detach().cpu().clone() for t in (ar.data, st.m, st.v)] + [states.cpu()[:28 if st.plan is None else None].clone()]


def _assert_same(a, b, what):
    for x, y, name in zip(a, b, ("weights", "m", "v", "step states")):
        x, y = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (x, y))
        assert torch.equal(x, y), (what, name)


def _want(sched, base, u):
    return R.rate32(base, u, sched["kind"], sched["warmup"], sched["total"], sched["floor"])


@pytest.mark.parametrize("form", ["plain", "segmented"])
def test_optimizer_against_a_twin_with_the_reported_rates(gpu, form):
    """Ten updates under a cosine schedule (W = 3, total = 8).  After each one current_lr() is read and exactly those float32
    values become group['lr'] of a capturable twin without a schedule, which then takes the same update: weights, moments and
    step states stay bit-identical, so the kernel's output is what the update uses and nothing else changed.  The rates are
    the restatement's to one float32 ulp (the count that is not its bits is printed)."""
    seg = form == "segmented"
    (na, aa), (nb, ab) = _net(gpu, frozen=seg), _net(gpu, frozen=seg)
    oa = _adam(form, na, schedule=COSINE)
    from gdn_amd.optim import Adam
    ob = Adam(_groups(nb, (LR, LR)), **{k: v for k, v in HYPER.items() if k != "lr"}, segmented=True) if seg else \
        Adam(nb.parameters(), **HYPER, capturable=True)
    mults = [1.0, 0.5] if seg else [1.0]
    inexact = 0
    for u in range(10):
        _grad(aa, u)
        _grad(ab, u)
        oa.step()
        rates = oa.current_lr()
        assert len(rates) == len(mults)
        for r, mult in zip(rates, mults):
            want = _want(COSINE, LR * mult, u)
            inexact += np.float32(r).tobytes() != want.tobytes()
            assert float(np.float32(r)) == r and abs(r - float(want)) <= R.ulp32(want), (u, r, want)
        for g, r in zip(ob.param_groups, rates):
            g["lr"] = float(r)
        ob.step()
        _assert_same(_dev_state(oa, aa), _dev_state(ob, ab), "%s update %d" % (form, u))
        assert ob.current_lr() == rates
    print("%s: %d of %d rates not the restatement's bits" % (form, inexact, 10 * len(mults)))
    assert rates == [float(np.float32(LR * m * 0.1)) for m in mults]               # past `total`: the floor
    st = oa.store_of(aa)
    assert (st.plan is not None) == seg and (not seg or st.plan.states is not None)
    if seg:
        frozen = list(na.parameters())[2]
        assert torch.equal(frozen.detach().cpu(), list(_net(gpu)[0].parameters())[2].detach().cpu())


def test_per_tensor_fallback_takes_each_parameters_own_count(gpu, monkeypatch):
    """A step in which one trainable parameter has no gradient runs per tensor: each update is preceded by a launch of its
    own with that parameter's own step state, so the parameter that sat out is one update behind from then on and runs at the
    rate of ITS count.  Read at the launches themselves: the rate in the table right after each gdn_lr_schedule, the count in
    the state it was handed, and the update that follows on the same state."""
    from gdn_amd import ops
    from gdn_amd.optim import _STEP_FMT, _unpack
    net, ar = _net(gpu)
    opt = _adam("plain", net, schedule=LINEAR)
    log, real_lr, real_adam = [], ops.lr_schedule, ops.adam_step_dev

    def lr_schedule(hyper, base, states, *a):
        real_lr(hyper, base, states, *a)
        log.append(("lr", states.data_ptr(), _unpack(_STEP_FMT, states)[2], np.float32(hyper.flatten()[0].item())))

    def adam_step_dev(p, g, m, v, hyper, state):
        real_adam(p, g, m, v, hyper, state)
        log.append(("adam", state.data_ptr(), p.numel()))
    monkeypatch.setattr(ops, "lr_schedule", lr_schedule)
    monkeypatch.setattr(ops, "adam_step_dev", adam_step_dev)
    ps = list(net.parameters())
    held = ps[3].grad
    for u in range(5):
        _grad(ar, u)
        ps[3].grad = None if u == 1 else held
        del log[:]
        opt.step()
        assert [e[0] for e in log] == ["lr", "adam"] * (len(log) // 2)
        assert all(a[1] == b[1] for a, b in zip(log[0::2], log[1::2]))                     # each pair on one step state
        assert all(e[3].tobytes() == _want(LINEAR, LR, e[2]).tobytes() for e in log[0::2])
        counts = [e[2] for e in log[0::2]]
        if u == 0:
            assert counts == [0] and log[1][2] == 384                                      # one launch over the arena
        elif u == 1:
            assert counts == [1] * 5
        else:
            assert sorted(counts) == [u - 1] + [u] * 5 and [e[2] for e in log[1::2]] == [p.numel() for p in ps]
            assert counts[3] == u - 1
    assert opt.store_of(ar).pstep is not None                      # (the per-tensor path ran)


def test_a_skipped_step_does_not_advance_the_schedule(gpu):
    """skip_nonfinite: a NaN gradient at update 2 leaves t alone, the next update runs at the rate the skipped one would have
    used, and current_lr() shows it both times (linear: bit for bit)."""
    net, ar = _net(gpu)
    opt = _adam("plain", net, schedule=LINEAR, skip_nonfinite=True)
    seen, before = [], None
    for k in range(6):
        _grad(ar, k)
        if k == 2:
            ar.grad[7] = float("nan")
            before = ar.data.clone()
        opt.step()
        if k == 2:
            assert torch.equal(before, ar.data)
        seen.append(np.float32(opt.current_lr()[0]))
    applied = [0, 1, 2, 2, 3, 4]                                 # the index of the update each step ran (or would have run) as
    assert [x.tobytes() for x in seen] == [_want(LINEAR, LR, u).tobytes() for u in applied]
    gs = opt.guard_stats()
    assert gs["skipped"] == 1 and gs["steps"] == 6 and opt.store_of(ar).count(next(net.parameters())) == 5


@pytest.mark.parametrize("form", ["plain", "segmented"])
def test_the_reference_decay_composes(gpu, form):
    """Code that writes group['lr'] mid-run, as trainer._decay_lr does: the next rates are float32(new_lr * lr_mult * s(u))."""
    seg = form == "segmented"
    net, ar = _net(gpu, frozen=seg)
    opt = _adam(form, net, schedule=LINEAR)
    mults = [1.0, 0.5] if seg else [1.0]
    lr = LR
    for u in range(7):
        if u in (2, 5):
            lr -= lr / 25
            for g in opt.param_groups:
                g["lr"] = lr
        _grad(ar, u)
        opt.step()
        got = [np.float32(r).tobytes() for r in opt.current_lr()]
        assert got == [_want(LINEAR, lr * m, u).tobytes() for m in mults], u
    assert all(g.get("lr_mult", 1.0) == m for g, m in zip(opt.param_groups, mults))


@pytest.mark.parametrize("form", ["plain", "segmented"])
def test_graphed_step_matches_eager_without_a_host_push(gpu, form, monkeypatch):
    """Three eager updates, then eight replays of a captured one that cross the end of the warm-up (W = 5) and of the run
    (total = 9): the same rates and bit-identical weights, moments and step states as eleven eager updates.  No host push
    happens between replays: refresh_hyper() looks at the tables before every replay, and none of its _push_hyper
    calls writes anything (the host copies they compare against stay what they were)."""
    from gdn_amd.graph import GraphedTrainStep
    from gdn_amd.optim import Adam
    seg = form == "segmented"
    sched = {"kind": "cosine", "warmup": 5, "total": 9, "floor": 0.1}
    grads = [torch.randn(384, generator=torch.Generator().manual_seed(200 + k)).to(gpu) for k in range(11)]
    runs = {}
    for mode in ("eager", "graph"):
        net, ar = _net(gpu, frozen=seg)
        opt = _adam(form, net, schedule=sched, max_grad_norm=1.0, ema_decay=0.9)

        def step_fn(g, ar=ar, opt=opt):
            ar.grad.copy_(g)
            opt.step()
            return (ar.data,)
        rates, writes, calls = [], [], []
        for k in range(3):
            step_fn(grads[k])
            rates.append(opt.current_lr())
        run = step_fn
        if mode == "graph":
            run = GraphedTrainStep(step_fn, (grads[2],), opt, prewarmed=True)
            for name in ("_push_hyper",):
                def counted(target, *a, _f=getattr(Adam, name), _n=name):
                    host = lambda: (target.hyper_host, target.base_host)      # noqa: E731
                    before = host()
                    _f(opt, target, *a)
                    calls.append(_n)
                    if host() != before:
                        writes.append(_n)
                monkeypatch.setattr(opt, name, counted)
        for k in range(3, 11):
            run(grads[k])
            rates.append(opt.current_lr())
        if mode == "graph":
            assert run.replays == 8 and len(calls) == 8 and writes == []
        runs[mode] = (rates, _dev_state(opt, ar), opt.store_of(ar).ema.cpu(), opt.guard_stats())
    (ra, sa, ea, ga), (rb, sb, eb, gb) = runs["eager"], runs["graph"]
    assert ra == rb and len(set(r[0] for r in ra)) > 6
    _assert_same(sa, sb, "graph vs eager, %s" % form)
    assert torch.equal(ea.view(torch.int32), eb.view(torch.int32)) and ga == gb
    mults = [1.0, 0.5] if seg else [1.0]
    for u, r in enumerate(ra):
        for x, m in zip(r, mults):
            want = _want(sched, LR * m, u)
            assert abs(x - float(want)) <= R.ulp32(want), (u, x, want)


def test_current_lr_and_a_capture(gpu):
    from gdn_amd._lib import GdnError
    from gdn_amd.optim import Adam
    net, ar = _net(gpu)
    with pytest.raises(GdnError, match="current_lr"):
        Adam(net.parameters(), **HYPER).current_lr()
    opt = _adam("plain", net, schedule=LINEAR)
    assert opt.current_lr() == [None]
    _grad(ar, 0)
    opt.step()
    assert [np.float32(r).tobytes() for r in opt.current_lr()] == [_want(LINEAR, LR, 0).tobytes()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    errors, tick = [], torch.zeros(4, device=gpu)
    with torch.cuda.graph(g):
        tick.add_(1.0)                                     # (something to capture)
        try:
            opt.current_lr()
        except GdnError as e:
            errors.append(str(e))
    assert len(errors) == 1 and "current_lr() inside a graph capture" in errors[0]


# ---- the flags, end to end -----------------------------------------------------------------------------------------------
_RUNS = {}
SCHED = ["--warmup_steps", "2", "--lr_schedule", "cosine", "--lr_floor", "0.1"]
COMBO = ["--freeze", "encoder", "--lr_mult", "*.bias=0.5", "--ema_decay", "0.9", "--clip_grad_norm", "1"]


class _Stop(Exception):
    pass


@pytest.fixture(scope="module")
def loop_root(tmp_path_factory):
    import gdn_amd.AE_model_unet as M
    root = tmp_path_factory.mktemp("lr_schedule")
    torch.manual_seed(11)
    net = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
    torch.save({"module." + k: v.contiguous() for k, v in net.state_dict().items()}, str(root / "init.pkl"))
    return root


def _run(root, tag, dtype, extra, init=True, stop_after_first_state=False, spy=None):
    """GDN_main.run in `root`/<dtype>_<tag> (cached): {file name: tensors of every .pkl written}.  stop_after_first_state:
    the run dies right after its first train_state.pt is on disk (the end of epoch 1 under --save_state), as a kill would
    end it -- its command line, and with it the run's length, is the uninterrupted run's."""
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
    _RUNS[key] = {p.name: torch.load(p, map_location="cpu") for p in sorted(where.rglob("*.pkl")) if p.name != "init.pkl"}
    return _RUNS[key]


def _same_files(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
    for name in a:
        assert list(a[name]) == list(b[name])
        for k in a[name]:
            assert torch.equal(a[name][k], b[name][k]), (what, name, k)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loop_graph_is_bitwise(gpu, loop_root, dtype):
    base = _run(loop_root, "base", dtype, SCHED)
    assert len(base) == 2
    _same_files(base, _run(loop_root, "graph", dtype, SCHED + ["--graph", "--graph_warmup", "2"]), "--graph")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loop_schedule_changes_the_run_and_reference_does_not(gpu, loop_root, dtype):
    """--lr_schedule reference without a warm-up writes the files no flag at all writes (and builds no schedule); the cosine
    run's weights differ from them."""
    spy = []
    plain = _run(loop_root, "plain", dtype, [])
    ref = _run(loop_root, "reference", dtype, ["--lr_schedule", "reference", "--warmup_steps", "0"], spy=spy)
    _same_files(plain, ref, "--lr_schedule reference")
    assert spy[0].schedule is None and not spy[0].capturable
    base = _run(loop_root, "base", dtype, SCHED)
    assert sorted(k.split("_loss_")[0] for k in base) == sorted(k.split("_loss_")[0] for k in plain)
    a, b = (sorted(r.items())[0][1] for r in (base, plain))
    assert any(not torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loop_resume_is_bitwise_and_another_schedule_is_refused(gpu, loop_root, dtype):
    from gdn_amd._lib import GdnError
    base = _run(loop_root, "base", dtype, SCHED)
    stopped = _run(loop_root, "stopped", dtype, SCHED + ["--save_state"], stop_after_first_state=True)
    (state,) = sorted((loop_root / ("%s_stopped" % dtype)).rglob("train_state.pt"))
    saved = torch.load(state, map_location="cpu", weights_only=True)
    assert saved["schedule"] == {"kind": "cosine", "warmup": 2, "total": 6, "floor": 0.1, "lr_schedule": "cosine"}
    assert saved["optimizer"]["gdn"]["schedule"] == {"kind": "cosine", "warmup": 2, "total": 6, "floor": 0.1}
    assert (saved["epoch"], saved["i"], saved["step"]) == (1, -1, 3)
    resumed = _run(loop_root, "resumed", dtype, SCHED + ["--resume", str(state)], init=False)
    assert len(stopped) == 1 and len(resumed) == 1
    _same_files({k: v for k, v in base.items() if k in stopped}, stopped, "epoch 1")
    _same_files({k: v for k, v in base.items() if k not in stopped}, resumed, "--resume")
    for k, other in enumerate((["--warmup_steps", "2", "--lr_schedule", "linear", "--lr_floor", "0.1"], ["--warmup_steps", "1"] + SCHED[2:], [])):
        spy = []
        with pytest.raises(GdnError, match="learning-rate schedule"):
            _run(loop_root, "refused%d" % k, dtype, other + ["--resume", str(state)], init=False, spy=spy)
        # before any step: the optimizer of the refused run has no store
        assert len(spy) == 1 and not spy[0]._stores
        assert not list((loop_root / ("%s_refused%d" % (dtype, k))).rglob("*.pkl"))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loop_accum_counts_the_run_in_updates(gpu, loop_root, dtype):
    """--accum_steps 2 over 2 epochs of 3 batches: 4 updates, so total = 4 and the last one (index 3) ran at
    float32(lr * s(3)) of that schedule."""
    spy = []
    files = _run(loop_root, "accum", dtype, SCHED + ["--accum_steps", "2"], spy=spy)
    (opt,) = spy
    assert len(files) == 2 and opt.schedule == {"kind": "cosine", "warmup": 2, "total": 4, "floor": 0.1}
    (st,) = opt._stores.values()
    assert st.count(st.items[0][0]) == 4
    (rate,) = opt.current_lr()
    want = R.rate32(2e-5, 3, "cosine", 2, 4, 0.1)
    print("last rate %.9e, restatement %.9e" % (rate, float(want)))
    assert abs(rate - float(want)) <= R.ulp32(want)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loop_with_the_other_fine_tuning_flags_is_bitwise_under_graph(gpu, loop_root, dtype):
    spy = []
    eager = _run(loop_root, "combo", dtype, SCHED + COMBO, spy=spy)
    assert len(eager) == 4 and sum(n.endswith("_ema.pkl") for n in eager) == 2
    _same_files(eager, _run(loop_root, "combo_graph", dtype, SCHED + COMBO + ["--graph", "--graph_warmup", "2"]), "--graph")
    (opt,) = spy
    rates = opt.current_lr()
    assert len(rates) == 2 and len(opt.param_groups) == 2
    for r, g in zip(rates, opt.param_groups):
        want = R.rate32(2e-5 * g.get("lr_mult", 1.0), 5, "cosine", 2, 6, 0.1)
        assert abs(r - float(want)) <= R.ulp32(want)
    assert sorted(g.get("lr_mult", 1.0) for g in opt.param_groups) == [0.5, 1.0]
