"""Gradient accumulation (--accum_steps, Adam.micro_batches, gdn_grad_accumulate): what needs no GPU -- the
command-line flag and its refusals, the C ABI's declaration and argument checks, the optimizer's gradient scale, the state
file's extra key, and the data-parallel rule (K micro-backwards, ONE all-reduce) on a CPU arena over gloo."""
import argparse
import ctypes
import multiprocessing as mp
import os
import pathlib
import re
import socket

import numpy as np
import pytest
import torch

REPO = pathlib.Path(__file__).resolve().parent.parent


# ---- command line ---------------------------------------------------------------------------------------------------
def _no_gpu_calls(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the check touched the GPU")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "is_initialized", boom)


def test_parser_default_and_value():
    from gdn_amd import option
    assert option.parse_args(["synthetic", "--synthetic"]).accum_steps == 1
    assert option.parse_args(["synthetic", "--synthetic", "--accum_steps", "8"]).accum_steps == 8
    text = " ".join(option.build_parser().format_help().split())
    assert "K x batch_size x ranks" in text


@pytest.mark.parametrize("bad", ["0", "-1", "x"])
def test_accum_steps_must_be_a_positive_integer(bad, capsys):
    from gdn_amd import option
    with pytest.raises(SystemExit):
        option.parse_args(["synthetic", "--synthetic", "--accum_steps", bad])
    assert "--accum_steps" in capsys.readouterr().err


@pytest.mark.parametrize("mode", ["DtoD_test", "RtoD_test"])
def test_accum_with_a_test_mode_is_refused_before_the_gpu(monkeypatch, mode):
    from gdn_amd import GDN_main, option
    _no_gpu_calls(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = option.parse_args(["synthetic", "--synthetic", "--mode", mode, "--accum_steps", "2"])
    with pytest.raises(RuntimeError, match="trains nothing"):
        GDN_main.run(a)


def test_accum_with_graph_is_refused_before_the_gpu(monkeypatch):
    from gdn_amd import GDN_main, option
    _no_gpu_calls(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = option.parse_args(["synthetic", "--synthetic", "--mode", "DtoD", "--graph", "--accum_steps", "2"])
    with pytest.raises(RuntimeError, match="--accum_steps 2.*follow-up"):
        GDN_main.run(a)
    # K = 1 is the flag off: --graph alone passes this check (and then stops at the first thing that asks for a GPU)
    a = option.parse_args(["synthetic", "--synthetic", "--mode", "DtoD", "--graph", "--accum_steps", "1"])
    GDN_main._check_accum(a)


def test_the_loops_refuse_graph_and_another_k_before_any_step():
    """train_AE_DtoD / train_AE_RtoD themselves: --graph with K > 1, and a training state written with another K (a state
    without the key was written with K = 1)."""
    from gdn_amd import trainer as T
    from gdn_amd._lib import GdnError
    ns = argparse.Namespace
    assert T._check_accum(ns(), None) == 1 and T._check_accum(ns(accum_steps=3), None) == 3
    assert T._check_accum(ns(accum_steps=2), {"accum_steps": 2}) == 2
    with pytest.raises(GdnError, match="follow-up"):
        T._check_accum(ns(accum_steps=2, graph=True), None)
    with pytest.raises(GdnError, match="--accum_steps 2.*--accum_steps 3"):
        T._check_accum(ns(accum_steps=3), {"accum_steps": 2})
    with pytest.raises(GdnError, match="--accum_steps 1.*--accum_steps 2"):
        T._check_accum(ns(accum_steps=2), {"epoch": 0})
    with pytest.raises(GdnError, match="--accum_steps 2.*--accum_steps 1"):
        T._check_accum(ns(), {"accum_steps": 2})


# ---- state file -----------------------------------------------------------------------------------------------------
class _Loader:
    def state_dict(self, epoch_done=False):
        return {"pos": 0}

    def load_state_dict(self, state):
        self.got = state


def test_progress_carries_accum_steps_only_when_it_is_on():
    from gdn_amd import trainer as T
    net = torch.nn.Linear(2, 2)
    opt = torch.optim.Adam(net.parameters())
    progress = {"epoch": 1, "i": 3, "lr": 1e-4, "model_num": 2, "seen": 16, "step": 8}
    off = T.training_state(net, opt, _Loader(), dict(progress))
    one = T.training_state(net, opt, _Loader(), dict(progress, accum_steps=1))
    on = T.training_state(net, opt, _Loader(), dict(progress, accum_steps=2))
    assert "accum_steps" not in off and list(off) == list(one)
    assert on["accum_steps"] == 2 and [k for k in on if k != "accum_steps"] == list(off)
    assert T.load_training_state(off, net, opt, _Loader()) == progress
    assert T.load_training_state(on, net, opt, _Loader()) == dict(progress, accum_steps=2)


# ---- C ABI ----------------------------------------------------------------------------------------------------------
def test_symbol_declared_built_and_bound_at_revision_223():
    from gdn_amd import _lib as L
    hdr = (REPO / "include" / "gdn_hip.h").read_text()
    assert re.search(r"\bint\s+gdn_grad_accumulate\s*\(\s*float\s*\*\s*acc,\s*const\s+float\s*\*\s*g,\s*int64_t\s+n,\s*void\s*\*\s*stream\)",
                     hdr)
    dll = ctypes.CDLL(str(L.LIB_PATH))
    assert hasattr(dll, "gdn_grad_accumulate") and "gdn_grad_accumulate" in L._SIGS and "gdn_grad_accumulate" in L.EXPORTS
    assert L._SIGS["gdn_grad_accumulate"] == L._SIGS["gdn_swap_f32"]
    assert L.ABI_VERSION == 223 and L.lib.gdn_version() == 223


def test_argument_checks_answer_before_any_launch():
    """GDN_ERR_BAD_ARG (-1) for a NULL pointer, n <= 0, a misaligned base and overlapping ranges; the pointers are never
    dereferenced, so no GPU is needed.  Through gdn_amd.ops the same answers are GdnErrors."""
    from gdn_amd import _lib as L
    P = ctypes.c_void_p
    acc = L.lib.raw("gdn_grad_accumulate")
    a, g = P(0x1000), P(0x2000)
    assert acc(None, g, 8, None) == -1 and acc(a, None, 8, None) == -1
    assert acc(a, g, 0, None) == -1 and acc(a, g, -4, None) == -1
    assert acc(P(0x1002), g, 8, None) == -1 and acc(a, P(0x2001), 8, None) == -1
    assert acc(a, a, 8, None) == -1                                    # the same range
    assert acc(a, P(0x1000 + 4 * 7), 8, None) == -1                    # one float shared at either end
    assert acc(P(0x1000 + 4 * 7), a, 8, None) == -1
    with pytest.raises(L.GdnError, match="gdn_grad_accumulate failed: bad argument"):
        L.lib.gdn_grad_accumulate(None, g, 8, None)


# ---- optimizer ------------------------------------------------------------------------------------------------------
def _arena_and_net():
    from gdn_amd import engine as E
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3), torch.nn.BatchNorm2d(3), torch.nn.ConvTranspose2d(3, 2, 3))
    ar = E.ParamArena(net, torch.device("cpu"))
    net._gdn_param_arena = ar
    ar.bind_grads()
    ar.grad.copy_(torch.randn(ar.numel, generator=torch.Generator().manual_seed(5)))
    return net, ar


def test_micro_batches_rides_in_the_gradient_scale(monkeypatch):
    """Host path: the grad_scale argument of the update is grad_scale / micro_batches in double.  Capturable path: hyper[5]
    is that value rounded to float32 once, pushed when micro_batches changes.  state_dict() does not carry it."""
    from gdn_amd import ops
    from gdn_amd.optim import Adam
    seen = []
    monkeypatch.setattr(ops, "zeros", lambda shape, device: torch.zeros(shape, dtype=torch.float32, device=device))
    monkeypatch.setattr(ops, "adam_step", lambda p, g, m, v, lr, b1, b2, eps, wd, step, scale: seen.append(scale))
    monkeypatch.setattr(ops, "adam_step_dev", lambda p, g, m, v, hyper, state: seen.append(hyper.clone()))
    net, _ = _arena_and_net()
    opt = Adam(net.parameters(), lr=1e-3)
    assert opt.micro_batches == 1
    opt.step()
    opt.micro_batches = 3
    opt.step()
    opt.grad_scale = 0.5                       # what sync_gradients leaves at world 2
    opt.step()
    assert seen == [1.0, 1.0 / 3, 0.5 / 3] and isinstance(seen[0], float)
    sd = opt.state_dict()
    assert "micro_batches" not in sd["gdn"] and sd["gdn"]["grad_scale"] == 0.5
    assert not any("micro" in str(k) for g in sd["param_groups"] for k in g)
    opt.micro_batches = 0
    with pytest.raises(ValueError, match="micro_batches"):
        opt.step()

    del seen[:]
    net, _ = _arena_and_net()
    opt = Adam(net.parameters(), lr=1e-3, capturable=True)
    opt.step()
    opt.micro_batches = 3
    opt.step()
    opt.grad_scale = 0.125
    opt.micro_batches = 7
    opt.refresh_hyper()
    (st,) = opt._stores.values()
    want = [np.float32(1.0), np.float32(1.0 / 3), np.float32(0.125 / 7)]
    assert [np.float32(h[5].item()) for h in seen] + [np.float32(st.hyper[5].item())] == want
    assert "micro_batches" not in opt.state_dict()["gdn"]


# ---- data parallelism: K micro-backwards, one all-reduce -------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _one_sync_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), GDN_OVERLAP_ALLREDUCE="1")
    import sys
    root = pathlib.Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root)); sys.path.insert(0, str(root / "gdn-pytorch_amd"))
    torch.set_num_threads(1)
    from gdn_amd import distributed as D
    from gdn_amd import engine as E
    from gdn_amd import trainer as T
    try:
        D.init(backend="gloo")
        torch.manual_seed(0)
        model = torch.nn.Sequential(torch.nn.Conv2d(4, 8, 3, bias=False), torch.nn.BatchNorm2d(8), torch.nn.Conv2d(8, 8, 1, bias=False),
                                    torch.nn.BatchNorm2d(8), torch.nn.Conv2d(8, 2, 3, bias=False))
        arena = E.ParamArena(model, torch.device("cpu"))
        model._gdn_param_arena = arena
        params = list(model.parameters())
        K = 3

        def g(step, r):                                   # the "local gradient" of rank r in backward number `step`
            gen = torch.Generator().manual_seed(1000 * step + r)
            return [torch.randn(p.shape, generator=gen) for p in params]

        def backward(step):
            """What _Bridge.backward does around the tape, with a tape that writes this rank's gradients in reverse order."""
            ctx = E.Ctx(record=True, arena=arena)
            pending = E.begin_backward(model, arena, ctx)
            for p, gp in reversed(list(zip(params, g(step, rank)))):
                p.grad.copy_(gp)
                ctx.grads_done(p)
            E.end_backward(arena, pending)
            assert arena.carry_reduced is None
            return ctx.reducer is not None

        class _Opt:
            grad_scale = 1.0
            micro_batches = 1
            steps = 0

            def zero_grad(self):
                for p in params:
                    p.grad = None

            def step(self):
                self.steps += 1
        opt = _Opt()
        # an overlapped reducer exists from an earlier, non-accumulating use of the model: a fresh backward starts it
        model._gdn_reducer = D.GradReducer(arena, bucket_elems=200)
        assert backward(0) is True
        D.sync_gradients(model, opt)
        # the loop's own bookkeeping (trainer._GroupedStep): the model is marked, no micro-batch starts the reducer
        saver = argparse.Namespace(last_batch=lambda i: False)
        overlapped = []

        def fwd_bwd(step, first=True):
            if first:
                opt.zero_grad()
            overlapped.append(backward(step))
            return step
        groups = T._GroupedStep(fwd_bwd, model, opt, K, 100, saver)
        assert model._gdn_whole_arena_sync is True and not groups.held
        D.stats_begin()
        for i in range(K):
            assert D.STATS.syncs == 0 and opt.steps == 0 and groups.held == (i > 0)
            assert groups(i, 10 + i) == 10 + i
        assert overlapped == [False] * K
        assert D.STATS.syncs == 1 and opt.steps == 1 and groups.micro == 0 and not groups.held
        assert opt.grad_scale == 1.0 / world and opt.micro_batches == K
        assert arena.carry_reduced is None and arena.reduced
        want = [sum(g(10 + s, r)[i] for s in range(K) for r in range(world)) / (world * K) for i in range(len(params))]
        for p, w in zip(params, want):
            torch.testing.assert_close(p.grad * (opt.grad_scale / opt.micro_batches), w, rtol=1e-5, atol=1e-6)
        # a shorter last group: two micro-batches, closed by the epoch's end
        groups = T._GroupedStep(fwd_bwd, model, opt, K, 5, saver)
        groups.begin_epoch()
        groups(3, 20)
        assert groups.micro == 1 and groups.held and D.STATS.syncs == 1
        groups(4, 21)
        assert groups.micro == 0 and D.STATS.syncs == 2 and opt.steps == 2 and opt.micro_batches == 2
        groups.end_epoch()                                 # nothing is open: the epoch's end adds no update
        assert D.STATS.syncs == 2 and opt.steps == 2
        want = [sum(g(20 + s, r)[i] for s in range(2) for r in range(world)) / (world * 2) for i in range(len(params))]
        for p, w in zip(params, want):
            torch.testing.assert_close(p.grad * (opt.grad_scale / opt.micro_batches), w, rtol=1e-5, atol=1e-6)
        groups.close()
        assert opt.micro_batches == 1
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, "FAIL: %s\n%s" % (e, traceback.format_exc())))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()


def test_k_micro_backwards_one_all_reduce_under_data_parallelism():
    """World 2 over gloo, a CPU arena: K = 3 accumulating micro-backwards start no overlapped reduction, the group's end runs
    ONE sync_gradients over the whole arena, and the optimizer-visible gradient times grad_scale / micro_batches is the mean
    over the 2 x 3 contributions; carry_reduced is never used."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_one_sync_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = sorted(q.get(timeout=120) for _ in ps)
    for p in ps:
        p.join(timeout=60)
    assert got == [(0, "ok"), (1, "ok")], got
