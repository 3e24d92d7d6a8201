"""The library calls of optimizer.step(), pinned: which entry point, on which range of which buffer, in which order.

A tiny arena on the CPU, the seven launch functions of gdn_amd.ops replaced by recorders, so nothing here needs a GPU.  The
expected sequences are literals recorded at the commit before the state stores became one type, by running this file
there.  At that commit only the host-path cases run as they stand: the capturable path's capture refusals asked the stream
of a process without a device (hipErrorNoDevice), so its cases were recorded with torch.cuda.is_current_stream_capturing
stubbed to False.  Since then every refusal asks torch.cuda.is_available() first and the whole file runs on a CPU.
The arena has 384 floats; its six items sit at float offsets 0 (54 floats), 64 (3), 128 (3), 192 (3), 256 (54) and 320 (2)."""
import pytest
import torch

ITEMS = [(0, 54), (64, 3), (128, 3), (192, 3), (256, 54), (320, 2)]
COVERED = [ITEMS[k] for k in (0, 1, 3, 4, 5)]         # parameters()[2] has no gradient
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
GUARD_EMA = dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.99)


@pytest.fixture
def calls(monkeypatch):
    """Recorders in place of the launches: (name, numel, float offset of the first tensor from its buffer's base, ...)."""
    from gdn_amd import ops
    log = []
    monkeypatch.setattr(ops, "zeros", lambda shape, device: torch.zeros(shape, dtype=torch.float32, device=device))
    monkeypatch.setattr(ops, "adam_step", lambda p, g, m, v, *a: log.append(
        ("adam_step", p.numel(), p.storage_offset()) + _same_range(p, g, m, v)))
    monkeypatch.setattr(ops, "adam_step_dev", lambda p, g, m, v, hyper, state: log.append(
        ("adam_step_dev", p.numel(), p.storage_offset()) + _same_range(p, g, m, v)))
    monkeypatch.setattr(ops, "adam_step_dev_guarded", lambda p, g, m, v, hyper, state, guard: log.append(
        ("adam_step_dev_guarded", p.numel(), p.storage_offset()) + _same_range(p, g, m, v)))
    monkeypatch.setattr(ops, "grad_sumsq", lambda g, guard, accumulate=False: log.append(("grad_sumsq", g.numel(), accumulate)))
    monkeypatch.setattr(ops, "grad_guard_finalize", lambda *a: log.append(("grad_guard_finalize",)))
    monkeypatch.setattr(ops, "ema_update", lambda ema, p, decay, state, guard=None: log.append(
        ("ema_update", p.numel(), ema.storage_offset()) + _same_range(ema, p)))
    monkeypatch.setattr(ops, "swap_", lambda a, b: log.append(("swap_", a.numel(), a.storage_offset())))
    return log


def _same_range(first, *others):
    """() if every tensor covers the same range of its own buffer as `first`, else what differs (and fails the comparison)."""
    return tuple((t.numel(), t.storage_offset()) for t in others
                 if (t.numel(), t.storage_offset()) != (first.numel(), first.storage_offset()))


def _arena_and_net():
    from gdn_amd import engine as E
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3), torch.nn.BatchNorm2d(3), torch.nn.ConvTranspose2d(3, 2, 3))
    ar = E.ParamArena(net, torch.device("cpu"))
    net._gdn_param_arena = ar
    assert ar.numel == 384 and [(o, n) for _, o, n, _ in ar.items] == ITEMS
    ar.bind_grads()
    ar.grad.copy_(torch.randn(ar.numel, generator=torch.Generator().manual_seed(5)))
    return net, ar


def _two_steps(calls, **kw):
    """A full-coverage step, then one without a gradient for parameters()[2]: (the calls of each, the optimizer)."""
    from gdn_amd.optim import Adam
    net, ar = _arena_and_net()
    opt = Adam(net.parameters(), **HYPER, **kw)
    opt.step()
    full = list(calls)
    del calls[:]
    list(net.parameters())[2].grad = None
    opt.step()
    return full, list(calls), opt


def _store_record(opt):
    (rec,) = opt.state_dict()["gdn"]["stores"]
    assert rec["kind"] == "arena" and rec["params"] == [0, 1, 2, 3, 4, 5]
    assert rec["step"] == 1 and rec["pstep"] == [2, 2, 1, 2, 2, 2]
    return rec


def test_host_path(calls):
    full, partial, opt = _two_steps(calls)
    assert full == [("adam_step", 384, 0)]
    assert partial == [("adam_step", n, o) for o, n in COVERED]
    rec = _store_record(opt)
    assert rec["full_dev"] is False and rec["state"] is None and rec["pdev"] == {}


def test_capturable(calls):
    full, partial, opt = _two_steps(calls, capturable=True)
    assert full == [("adam_step_dev", 384, 0)]
    assert partial == [("adam_step_dev", n, o) for o, n in COVERED]
    rec = _store_record(opt)
    assert rec["full_dev"] is True and sorted(rec["pdev"]) == [0, 1, 3, 4, 5]
    for state in [rec["state"]] + list(rec["pdev"].values()):
        assert state.dtype == torch.uint8 and state.numel() == 28


def test_guard_and_average(calls):
    full, partial, opt = _two_steps(calls, **GUARD_EMA)
    assert full == [("grad_sumsq", 384, False), ("grad_guard_finalize",), ("adam_step_dev_guarded", 384, 0), ("ema_update", 384, 0)]
    want = [("grad_sumsq", n, k > 0) for k, (o, n) in enumerate(COVERED)] + [("grad_guard_finalize",)]
    for o, n in COVERED:
        want += [("adam_step_dev_guarded", n, o), ("ema_update", n, o)]
    assert partial == want
    rec = _store_record(opt)
    assert rec["full_dev"] is True and rec["state"].numel() == 28 and sorted(rec["pdev"]) == [0, 1, 3, 4, 5]


class _OnGpuByItsOwnAccount(torch.nn.Parameter):
    """A CPU parameter for the loose path, which refuses parameters that are not on a GPU before it launches anything."""


@pytest.mark.parametrize("kw, want", [
    ({}, [("adam_step", 384, 0), ("adam_step", 5, 0)]),
    ({"capturable": True}, [("adam_step_dev", 384, 0), ("adam_step_dev", 5, 0)]),
    (GUARD_EMA, [("grad_sumsq", 384, False), ("grad_sumsq", 5, True), ("grad_guard_finalize",),
                 ("adam_step_dev_guarded", 384, 0), ("ema_update", 384, 0), ("adam_step_dev_guarded", 5, 0), ("ema_update", 5, 0)]),
], ids=["host", "capturable", "guard_ema"])
def test_a_loose_parameter_comes_after_the_arena(calls, monkeypatch, kw, want):
    from gdn_amd.optim import Adam
    monkeypatch.setattr(_OnGpuByItsOwnAccount, "is_cuda", property(lambda self: True), raising=False)
    net, ar = _arena_and_net()
    loose = _OnGpuByItsOwnAccount(torch.randn(5, generator=torch.Generator().manual_seed(6)))
    loose.grad = torch.randn(5, generator=torch.Generator().manual_seed(7))
    opt = Adam(list(net.parameters()) + [loose], **HYPER, **kw)
    opt.step()
    assert calls == want
    recs = opt.state_dict()["gdn"]["stores"]
    assert [(r["kind"], r["params"], r["step"], r["pstep"]) for r in recs] == [("arena", [0, 1, 2, 3, 4, 5], 1, None), ("loose", [6], 1, None)]
