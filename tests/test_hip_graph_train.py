"""--graph: the training loops replay their step as a hipGraph and the run is bit for bit the run without the flag
(DESIGN.md 3.4).  Every comparison is graph against eager with the same capturable optimizer, and bitwise: checkpoint file
names (they carry the loss digits), every tensor of every .pkl, the model's state (BatchNorm buffers included) and
optimizer.state_dict().  B = 2 at 32x64, 6-10 steps per run."""
import argparse
import copy
import os
import pathlib
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parent.parent
H, W, B = 32, 64, 2
LR = 2e-4


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b""


def _same(a, b, what="state"):
    """Bitwise equality of two nested states (dicts / lists / tuples / tensors / plain values)."""
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), what
        assert _bits(a) == _bits(b), what
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (what, list(a), list(b))
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (what, k))
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (what, i))
    else:
        assert a == b, (what, a, b)


def _networks(gpu, mode, dtype):
    """(the trained network, the frozen guide or None), built like GDN_main builds them; the same weights at every call."""
    import gdn_amd.AE_model_unet as M
    torch.manual_seed(4)
    if mode == "DtoD":
        return M.AutoEncoder_DtoD(input_dim=1, height=H, width=W).to(gpu).compute_dtype(dtype), None
    net = M.AutoEncoder_2(input_dim=3, height=H, width=W).to(gpu).compute_dtype(dtype)
    guide = None
    if mode == "RtoD":                       # a random frozen guide
        guide = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W).to(gpu).compute_dtype(dtype).eval()
    return net, guide


def _augment_loader(gpu, n=8, drop_last=True, resident=False, seed=3, train=True):
    from gdn_amd.datasets import GpuAugmentLoader, GpuResidentLoader, SyntheticRawKitti
    cls = GpuResidentLoader if resident else GpuAugmentLoader
    return cls(SyntheticRawKitti(n, H, W, seed=11), B, gpu, train=train, seed=seed, drop_last=drop_last)


def _loop(gpu, where, mode, dtype, graph, loader, epochs=2, epoch_size=4, opt_kw=None, val_loader=None, resume=None,
          **more):
    """One run of train_AE_DtoD / train_AE_RtoD in directory `where`; returns everything the comparisons look at."""
    from gdn_amd import trainer as T
    from gdn_amd.optim import Adam
    where.mkdir(parents=True, exist_ok=True)
    net, guide = _networks(gpu, mode, dtype)
    kw = dict(capturable=True)
    kw.update(opt_kw or {})
    opt = Adam(net.parameters(), LR, [0.9, 0.999], eps=1e-08, weight_decay=5e-4, **kw)
    args = argparse.Namespace(dataset="KITTI", epoch_size=epoch_size, batch_size=B, mode=mode, print_freq=10, graph=graph,
                              graph_warmup=2, **more)
    progress = None
    if resume is not None:
        progress = T.load_training_state(T.read_training_state(resume), net, opt, loader)
    logger = object() if val_loader is not None else None
    T.last_graph_report = None
    cwd = os.getcwd()
    os.chdir(where)
    try:
        if mode == "DtoD":
            T.train_AE_DtoD(args, net, None, None, opt, loader, val_loader, B, epochs, LR, logger, None, progress=progress)
        else:
            T.train_AE_RtoD(args, net, guide, None, None, opt, loader, val_loader, B, epochs, LR, logger, None,
                            progress=progress)
    finally:
        os.chdir(cwd)
    torch.cuda.synchronize()
    files = sorted(where.rglob("*.pkl"))
    return {"names": [str(f.relative_to(where)) for f in files],
            "pkl": {f.name: torch.load(f, map_location="cpu") for f in files},
            "model": {k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
            "opt": T._cpu_copy(opt.state_dict()),
            "guard": opt.guard_stats() if opt.guarded else None,
            "report": T.last_graph_report, "loader": loader}


def _compare(eager, graph):
    assert eager["names"] == graph["names"] and eager["names"], (eager["names"], graph["names"])
    _same(eager["pkl"], graph["pkl"], "pkl")
    _same(eager["model"], graph["model"], "model")
    _same(eager["opt"], graph["opt"], "optimizer")
    assert eager["report"] is None and graph["report"] is not None


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["DtoD", "RtoD", "RtoD_single"])
def test_graph_loop_equals_eager_loop(gpu, tmp_path, mode, dtype):
    """Two epochs of four steps, graph_warmup 2: the capture falls mid-epoch and replays cross the epoch boundary.  DtoD and
    RtoD_single read the augmenting file loader (bound to the static inputs), RtoD the SyntheticLoader (copied)."""
    from gdn_amd.synthetic import SyntheticLoader

    def loader():
        if mode == "RtoD":
            return SyntheticLoader(B, 4, H, W, seed=20, device=gpu, distinct=4)
        return _augment_loader(gpu)
    runs = {g: _loop(gpu, tmp_path / ("graph" if g else "eager"), mode, dtype, g, loader()) for g in (False, True)}
    _compare(runs[False], runs[True])
    assert runs[True]["report"] == {"replayed": 6, "warmup": 2, "eager_steps": 0}
    assert len(runs[True]["names"]) == (2 if mode == "DtoD" else 1)
    if mode != "RtoD":
        assert runs[True]["loader"]._bound is None              # the loop gave the loader its own outputs back


def test_graph_loop_with_guard_ema_and_validation(gpu, tmp_path, capsys):
    """Clipping, non-finite skipping, the weight average and the per-epoch validation on the averaged weights: the printed
    validation errors, X.pkl, X_ema.pkl and the guard's counters are those of the eager run."""
    opt_kw = dict(ema_decay=0.9, max_grad_norm=1.0, skip_nonfinite=True)
    runs, avg = {}, {}
    for g in (False, True):
        capsys.readouterr()
        runs[g] = _loop(gpu, tmp_path / ("graph" if g else "eager"), "DtoD", "fp32", g, _augment_loader(gpu), opt_kw=opt_kw,
                        val_loader=_augment_loader(gpu, n=4, train=False))
        avg[g] = [ln for ln in capsys.readouterr().out.splitlines() if " * Avg " in ln]
    _compare(runs[False], runs[True])
    assert len(avg[False]) == 2 and avg[False] == avg[True], (avg[False], avg[True])
    assert all(ln.startswith("(averaged weights)") for ln in avg[True])
    assert len(runs[True]["names"]) == 4 and sum(n.endswith("_ema.pkl") for n in runs[True]["names"]) == 2
    assert runs[False]["guard"] == runs[True]["guard"] and runs[True]["guard"]["steps"] == 8


def test_graph_run_resumed_with_graph_ends_like_the_eager_run(gpu, tmp_path):
    """A --graph --save_state_every 3 run stopped after two epochs of two steps leaves the state written at step 3 (a replayed
    step); resumed with --graph (two eager steps, then a new capture) it ends where the uninterrupted eager run ends."""
    from gdn_amd import trainer as T
    kw = dict(epoch_size=2, save_state_every=3)
    full = _loop(gpu, tmp_path / "full", "DtoD", "fp32", False, _augment_loader(gpu, n=4), epochs=4, **kw)
    stopped = _loop(gpu, tmp_path / "stopped", "DtoD", "fp32", True, _augment_loader(gpu, n=4), epochs=2, **kw)
    assert stopped["report"] == {"replayed": 2, "warmup": 2, "eager_steps": 0}
    (state,) = sorted((tmp_path / "stopped").rglob(T.STATE_FILE))
    head = T.read_training_state(state)
    assert (head["step"], head["epoch"], head["i"]) == (3, 1, 0)
    resumed = _loop(gpu, tmp_path / "resumed", "DtoD", "fp32", True, _augment_loader(gpu, n=4), epochs=4, resume=state, **kw)
    assert resumed["report"] == {"replayed": 3, "warmup": 2, "eager_steps": 0}
    assert len(full["names"]) == 4 and resumed["names"] == full["names"][1:] and stopped["names"] == full["names"][:2]
    _same({n: full["pkl"][n] for n in resumed["pkl"]}, resumed["pkl"], "pkl")
    _same(full["model"], resumed["model"], "model")
    _same(full["opt"], resumed["opt"], "optimizer")


def test_partial_last_batch_runs_eagerly(gpu, tmp_path):
    """Five samples in batches of two, drop_last off: the last batch of every epoch holds one sample, runs eagerly, and the
    run equals the eager one."""
    runs = {g: _loop(gpu, tmp_path / ("graph" if g else "eager"), "DtoD", "fp32", g,
                     _augment_loader(gpu, n=5, drop_last=False), epochs=2, epoch_size=0) for g in (False, True)}
    _compare(runs[False], runs[True])
    assert runs[True]["report"] == {"replayed": 2, "warmup": 2, "eager_steps": 2}       # one per epoch


def _dtod_step(gpu, dtype="fp32", **opt_kw):
    """(model, optimizer, fwd_bwd, step) of a DtoD training step, as the loops define them."""
    from gdn_amd import distributed as D
    from gdn_amd import utils as U
    from gdn_amd.optim import Adam
    model = _networks(gpu, "DtoD", dtype)[0].train()
    opt = Adam(model.parameters(), LR, [0.9, 0.999], eps=1e-08, weight_decay=5e-4, capturable=True, **opt_kw)

    def fwd_bwd(depth, sparse):
        terms = U.dtod_loss(model(depth, istrain=False), depth, sparse)
        opt.zero_grad()
        U.backward(terms[0])
        return terms

    def step(depth, sparse):
        terms = fwd_bwd(depth, sparse)
        D.sync_gradients(model, opt)
        opt.step()
        return terms
    return model, opt, fwd_bwd, step


@pytest.mark.parametrize("resident", [False, True])
def test_bind_outputs(gpu, resident):
    """A bound loader yields the bound tensors themselves, with the batches an unbound loader of the same seed yields; a
    batch of another size comes in fresh tensors; a graphed step fed by it refills nothing."""
    from gdn_amd import ops
    from gdn_amd._lib import GdnError
    from gdn_amd.graph import GraphedTrainStep
    plain = _augment_loader(gpu, n=5, drop_last=False, resident=resident)
    bound = _augment_loader(gpu, n=5, drop_last=False, resident=resident)
    outs = [torch.full((B, c, H, W), 7.0, device=gpu) for c in (1, 3, 1)]
    ptrs = [t.data_ptr() for t in outs]
    bound.bind_outputs(*outs)
    sizes = []
    for _ in range(2):
        for want, got in zip(plain, bound):
            sizes.append(got[0].shape[0])
            for j in range(3):
                assert _bits(want[j]) == _bits(got[j])
                assert (got[j].data_ptr() == ptrs[j]) == (got[0].shape[0] == B) and (got[j] is outs[j]) == (got[0].shape[0] == B)
    assert sizes == [2, 2, 1] * 2
    bound.bind_outputs(None, None, None)
    assert all(t.data_ptr() not in ptrs for t in next(iter(bound)))
    # a graphed step whose static inputs the loader writes
    model, opt, _, step = _dtod_step(gpu)
    loader = _augment_loader(gpu, n=8, resident=resident)
    it = iter(loader)
    for _ in range(2):
        gt, _, sparse = next(it)
        step(gt, sparse)
    graphed = GraphedTrainStep(step, (gt, sparse), opt, prewarmed=True)
    loader.bind_outputs(graphed.static_inputs[0], None, graphed.static_inputs[1])
    for gt, _, sparse in it:
        assert gt is graphed.static_inputs[0] and sparse is graphed.static_inputs[1]
        graphed(gt, sparse)
    assert graphed.replays == 2 and graphed.refills == 0
    graphed(gt.clone(), sparse)
    assert graphed.refills == 1
    # out= is checked
    src = torch.zeros((B, H, W, 1), dtype=torch.uint8, device=gpu)
    for bad in (torch.empty((B, 1, H, W + 1), device=gpu), torch.empty((B, 1, H, W), device=gpu, dtype=torch.float64),
                torch.empty((B, 1, H, W)), torch.empty((B + 1, 1, H, W), device=gpu)):
        with pytest.raises(GdnError, match="out must be"):
            ops.kitti_augment(src, None, train=False, out=bad)
    if resident:
        good = [torch.empty((1, c, H, W), device=gpu) for c in (1, 3, 1)]
        sel = [[0, 0, H, W, 0, 0]]
        ops.kitti_augment_resident(loader.pools.tensors, torch.tensor(sel, dtype=torch.int32), train=False, out=good)
        with pytest.raises(GdnError, match="out must be"):
            ops.kitti_augment_resident(loader.pools.tensors, torch.tensor(sel, dtype=torch.int32), train=False,
                                       out=[good[0], good[0], good[2]])
        with pytest.raises(GdnError, match="three"):
            ops.kitti_augment_resident(loader.pools.tensors, torch.tensor(sel, dtype=torch.int32), train=False, out=good[:2])
        with pytest.raises(GdnError, match="distinct"):
            ops.kitti_augment_resident(loader.pools.tensors, torch.tensor(sel, dtype=torch.int32), train=False,
                                       out=[good[0], good[1], good[0]])


def test_prewarmed_capture_takes_no_step_and_both_classes_equal_eager(gpu):
    """GraphedTrainStep(prewarmed=True) and GraphedDataParallelStep(prewarmed=True) at world 1: construction changes neither
    weights nor step counts, and 2 eager steps + 4 replays end bitwise where 6 eager steps end, the host-side counts of
    optimizer.state_dict() included."""
    from gdn_amd.graph import GraphedDataParallelStep, GraphedTrainStep
    from gdn_amd.synthetic import synthetic_batch
    batches = [synthetic_batch(B, H, W, seed=70 + i, device=gpu) for i in range(6)]
    ends = {}
    for kind in ("eager", "one", "two"):
        model, opt, fwd_bwd, step = _dtod_step(gpu, ema_decay=0.9, skip_nonfinite=True)
        run, losses = step, []
        for i, (d, _, s) in enumerate(batches):
            if i == 2 and kind != "eager":
                before = (model._gdn_param_arena.data.clone(), {k: v.clone() for k, v in model.state_dict().items()},
                          copy.deepcopy(opt.state_dict()))
                if kind == "one":
                    run = GraphedTrainStep(step, (d, s), opt, prewarmed=True)
                else:
                    run = GraphedDataParallelStep(fwd_bwd, model, opt, (d, s), prewarmed=True)
                torch.cuda.synchronize()
                assert run.warmup_steps == 0 and run.replays == 0
                assert torch.equal(before[0], model._gdn_param_arena.data)
                _same(before[1], dict(model.state_dict()), "model after capture")
                _same(before[2], opt.state_dict(), "optimizer after capture")
                assert opt.guard_stats()["steps"] == 2
            if i == 4:
                for g in opt.param_groups:                      # a learning-rate decay between replays
                    g["lr"] = g["lr"] * 0.5
            losses.append(run(d, s)[0].item())
        ends[kind] = {"losses": losses, "model": dict(model.state_dict()), "opt": opt.state_dict()}
        if kind != "eager":
            assert run.replays == 4 and run.refills == 8
    _same(ends["eager"], ends["one"], "GraphedTrainStep")
    _same(ends["eager"], ends["two"], "GraphedDataParallelStep")


def test_prewarmed_is_a_keyword_and_capturable_is_needed(gpu):
    from gdn_amd._lib import GdnError
    from gdn_amd.graph import GraphedDataParallelStep
    from gdn_amd.optim import Adam
    model = _networks(gpu, "DtoD", "fp32")[0]
    opt = Adam(model.parameters(), LR)
    with pytest.raises(GdnError, match="capturable"):
        GraphedDataParallelStep(lambda: None, model, opt, (), prewarmed=True)
    opt = Adam(model.parameters(), LR, capturable=True)
    with pytest.raises(GdnError, match="no gradient arena"):
        GraphedDataParallelStep(lambda: None, model, opt, (), prewarmed=True)


def test_two_ranks_graph_equals_eager(gpu, tmp_path):
    """World 2 (one GPU: both ranks on it under gloo; two or more: RCCL): 2 eager steps + 4 replays of two graphs around the
    eager whole-arena all-reduce equal 6 eager steps with the overlapped reducer, bitwise, on both ranks -- weights, moments,
    averages, guard counters, loss digits; the ranks equal each other; plain GraphedTrainStep still refuses world 2."""
    import torch.multiprocessing as mp
    import graph_dp_worker
    ctx = mp.spawn(graph_dp_worker.run, args=(2, 29631, str(tmp_path)), nprocs=2, join=False)       # a fresh child per rank
    deadline = time.time() + 240
    try:
        while not ctx.join(timeout=5):           # raises if a rank failed; every exit status is looked at
            assert time.time() < deadline, "the two ranks did not finish in time"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
            p.join()
    assert [p.exitcode for p in ctx.processes] == [0, 0]
    r = [torch.load(tmp_path / ("rank%d.pt" % k), map_location="cpu", weights_only=False) for k in (0, 1)]
    for k in (0, 1):
        assert r[k]["world"] == 2 and r[k]["backend"] == ("nccl" if torch.cuda.device_count() >= 2 else "gloo")
        assert r[k]["single_graph_refused"] is True and r[k]["capture_ran_nothing"] is True
        e, g = r[k]["eager"], r[k]["graph"]
        assert e["reducer"] and g["replays"] == graph_dp_worker.STEPS - graph_dp_worker.WARM and e["replays"] == 0
        assert e["losses"] == g["losses"] and len(g["losses"]) == graph_dp_worker.STEPS
        _same(e["sd"], g["sd"], "rank %d model" % k)
        _same(e["opt"], g["opt"], "rank %d optimizer" % k)
        assert e["guard"] == g["guard"] and g["guard"]["steps"] == graph_dp_worker.STEPS
        assert "ema" in g["opt"]["gdn"] and g["opt"]["gdn"]["grad_scale"] == 0.5
    # the ranks hold the same weights, moments and averages (BatchNorm running statistics and losses are rank-local)
    names = [n for n, _ in _networks("cpu", "DtoD", "fp32")[0].named_parameters()]
    for n in names:
        assert _bits(r[0]["graph"]["sd"][n]) == _bits(r[1]["graph"]["sd"][n]), n
    _same(r[0]["graph"]["opt"]["state"], r[1]["graph"]["opt"]["state"], "moments of the two ranks")
    _same(r[0]["graph"]["opt"]["gdn"]["ema"], r[1]["graph"]["opt"]["gdn"]["ema"], "averages of the two ranks")
    assert r[0]["graph"]["losses"] != r[1]["graph"]["losses"]           # each rank trained its own shard


def _cli(cwd, argv, limit=240):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([str(REPO / "gdn-pytorch_amd"), str(REPO)] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    cwd.mkdir(parents=True, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "gdn_amd.GDN_main", *argv]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(cwd), timeout=limit + 60)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def test_cli_graph_run_equals_the_run_without_the_flag(gpu, tmp_path):
    """python -m gdn_amd.GDN_main --synthetic --mode DtoD --graph --graph_warmup 2 ...: one fresh child per run; the same
    .pkl, byte-equal tensors, as the run without --graph (--skip_nonfinite on both sides: the same capturable optimizer)."""
    base = ["--synthetic", "--mode", "DtoD", "--epoch_size", "5", "--epochs", "1", "--batch_size", "2", "--height", str(H),
            "--width", str(W), "--gpu_num", "0", "--skip_nonfinite"]
    plain = _cli(tmp_path / "plain", base)
    graph = _cli(tmp_path / "graph", base + ["--graph", "--graph_warmup", "2"])
    assert "graph: 3 steps replayed as 1 graph, 2 eager (2 warm-up, 0 on batches of another shape)" in graph
    assert "graph:" not in plain
    a = {p.name: p for p in (tmp_path / "plain").rglob("*.pkl")}
    b = {p.name: p for p in (tmp_path / "graph").rglob("*.pkl")}
    assert len(a) == 1 and sorted(a) == sorted(b), (sorted(a), sorted(b))
    for name in a:
        _same(torch.load(a[name], map_location="cpu"), torch.load(b[name], map_location="cpu"), name)
