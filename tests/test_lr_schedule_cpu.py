"""The device-side learning-rate schedule (--warmup_steps / --lr_schedule / --lr_floor, Adam(schedule=...), gdn_lr_schedule;
DESIGN.md 3.9): what needs no GPU -- the restatement's own properties, the flags and their refusals, the run's length in
updates, the C ABI's declaration and argument checks, and the optimizer's and the state file's extra key."""
import argparse
import ctypes
import pathlib
import re

import numpy as np
import pytest
import torch

import lr_schedule_fp64 as R

REPO = pathlib.Path(__file__).resolve().parent.parent
BASE = ["synthetic", "--synthetic"]


# ---- the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floor", [0.0, 0.1, 0.25, 1.0])
@pytest.mark.parametrize("warmup,total", [(1, 2), (3, 8), (5, 40), (100, 1000)])
@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_shape(kind, warmup, total, floor):
    s = [R.s(u, kind, warmup, total, floor) for u in range(total + 10)]
    assert s[0] == 1.0 / warmup
    assert s[warmup - 1] == 1.0 and s[warmup] == 1.0
    assert all(a < b for a, b in zip(s[:warmup - 1], s[1:warmup]))              # the warm-up rises
    assert all(a >= b for a, b in zip(s[warmup:], s[warmup + 1:]))               # non-increasing afterwards
    if kind == "constant":
        assert all(v == 1.0 for v in s[warmup:])
    else:
        assert all(v == floor for v in s[total:])
        assert all(floor <= v <= 1.0 for v in s[warmup:]) and all(0.0 < v <= 1.0 for v in s[:warmup])
        if floor < 1.0:
            assert s[total - 1] > floor


@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_without_warmup(kind):
    assert R.s(0, kind, 0, 10, 0.1) == 1.0
    s = [R.s(u, kind, 0, 10, 0.1) for u in range(12)]
    assert all(a >= b for a, b in zip(s, s[1:]))
    assert s[10] == s[11] == (1.0 if kind == "constant" else 0.1)
    if kind == "linear":
        assert s[5] == 0.1 + (1.0 - 0.1) * (1.0 - 5.0 / 10.0)
    if kind == "cosine":
        assert abs(s[5] - 0.55) < 1e-15


def test_rate_is_rounded_once():
    got = R.rate32(2e-5 * 0.5, 1, "linear", 3, 8, 0.1)
    assert isinstance(got, np.float32) and got == np.float32(2e-5 * 0.5 * (2.0 / 3.0))
    assert R.rate32(0.0, 4, "cosine", 3, 8, 0.1) == 0.0


# ---- command line -----------------------------------------------------------------------------------------------------
def _no_gpu_calls(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the check touched the GPU")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "is_initialized", boom)


def test_parser_defaults_and_values():
    from gdn_amd import option
    a = option.parse_args(BASE)
    assert (a.warmup_steps, a.lr_schedule, a.lr_floor) == (0, "reference", 0.0)
    a = option.parse_args(BASE + ["--warmup_steps", "100", "--lr_schedule", "cosine", "--lr_floor", "0.1"])
    assert (a.warmup_steps, a.lr_schedule, a.lr_floor) == (100, "cosine", 0.1)
    assert option.parse_args(BASE + ["--lr_floor", "1"]).lr_floor == 1.0
    text = " ".join(option.build_parser().format_help().split())
    assert "--warmup_steps" in text and "--lr_schedule" in text and "--lr_floor" in text
    assert "epochs x ceil(epoch_size / accum_steps)" in text


@pytest.mark.parametrize("flag,bad", [("--warmup_steps", "-1"), ("--warmup_steps", "x"), ("--lr_floor", "-0.1"),
                                      ("--lr_floor", "1.5"), ("--lr_floor", "nan"), ("--lr_schedule", "exponential")])
def test_parser_refuses(flag, bad, capsys):
    from gdn_amd import option
    with pytest.raises(SystemExit):
        option.parse_args(BASE + [flag, bad])
    assert flag in capsys.readouterr().err


@pytest.mark.parametrize("mode", ["DtoD_test", "RtoD_test"])
@pytest.mark.parametrize("flags", [["--warmup_steps", "2"], ["--lr_schedule", "cosine"], ["--lr_schedule", "constant"]])
def test_a_test_mode_is_refused_before_the_gpu(monkeypatch, mode, flags):
    from gdn_amd import GDN_main, option
    _no_gpu_calls(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(RuntimeError, match="trains nothing"):
        GDN_main.run(option.parse_args(BASE + ["--mode", mode] + flags))


@pytest.mark.parametrize("kind", ["reference", "constant"])
def test_a_floor_without_a_decay_is_refused_before_the_gpu(monkeypatch, kind):
    from gdn_amd import GDN_main, option
    _no_gpu_calls(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(RuntimeError, match="--lr_floor 0.1.*--lr_schedule %s" % kind):
        GDN_main.run(option.parse_args(BASE + ["--mode", "DtoD", "--lr_schedule", kind, "--lr_floor", "0.1"]))
    for ok in ("linear", "cosine"):
        GDN_main._check_schedule(option.parse_args(BASE + ["--mode", "DtoD", "--lr_schedule", ok, "--lr_floor", "0.1"]))
    GDN_main._check_schedule(option.parse_args(BASE + ["--mode", "DtoD_test"]))              # no flag: nothing to refuse


def test_total_is_counted_in_updates():
    from gdn_amd import option
    from gdn_amd import trainer as T
    from gdn_amd._lib import GdnError
    a = option.parse_args(BASE + ["--accum_steps", "2", "--epoch_size", "5", "--epochs", "2", "--lr_schedule", "cosine",
                                  "--warmup_steps", "2", "--lr_floor", "0.1"])
    assert T.schedule_total(a, a.epochs, a.epoch_size) == 6
    assert T.lr_schedule_of(a, a.epochs, a.epoch_size) == {"kind": "cosine", "warmup": 2, "total": 6, "floor": 0.1}
    a = option.parse_args(BASE + ["--epoch_size", "5", "--epochs", "2", "--lr_schedule", "linear"])
    assert T.lr_schedule_of(a, a.epochs, a.epoch_size) == {"kind": "linear", "warmup": 0, "total": 10, "floor": 0.0}
    # the reference's decay: no schedule at all without a warm-up, the device's 'constant' kind under it with one
    a = option.parse_args(BASE + ["--epoch_size", "5", "--epochs", "2"])
    assert T.lr_schedule_of(a, a.epochs, a.epoch_size) is None
    assert T.lr_schedule_of(argparse.Namespace(), 2, 5) is None
    a = option.parse_args(BASE + ["--epoch_size", "5", "--epochs", "2", "--warmup_steps", "4"])
    assert T.lr_schedule_of(a, a.epochs, a.epoch_size) == {"kind": "constant", "warmup": 4, "total": 10, "floor": 0.0}
    # a warm-up that leaves the decay nothing: both numbers in the message
    for kind in ("linear", "cosine"):
        a = option.parse_args(BASE + ["--epoch_size", "5", "--epochs", "2", "--warmup_steps", "10", "--lr_schedule", kind])
        with pytest.raises(GdnError, match="--warmup_steps 10 .* 10 updates"):
            T.lr_schedule_of(a, a.epochs, a.epoch_size)
    a = option.parse_args(BASE + ["--epoch_size", "5", "--epochs", "2", "--warmup_steps", "12", "--lr_schedule", "constant"])
    assert T.lr_schedule_of(a, a.epochs, a.epoch_size)["warmup"] == 12


def test_the_loop_checks_its_optimizer_and_the_state_it_resumes():
    from gdn_amd import trainer as T
    from gdn_amd._lib import GdnError
    ns = argparse.Namespace
    sched = {"kind": "cosine", "warmup": 2, "total": 6, "floor": 0.1}
    with_it, without = ns(schedule=dict(sched)), ns()
    assert T._check_schedule(ns(), None, without, None) is None
    assert T._check_schedule(ns(), None, without, {"epoch": 0}) is None
    entry = T._check_schedule(ns(lr_schedule="cosine"), sched, with_it, None)
    assert entry == dict(sched, lr_schedule="cosine")
    assert T._check_schedule(ns(lr_schedule="cosine"), sched, with_it, {"schedule": dict(entry)}) == entry
    with pytest.raises(GdnError, match="optimizer was built with None"):
        T._check_schedule(ns(lr_schedule="cosine"), sched, without, None)
    with pytest.raises(GdnError, match="written under.*linear.*this run has.*cosine"):
        T._check_schedule(ns(lr_schedule="cosine"), sched, with_it, {"schedule": dict(entry, kind="linear", lr_schedule="linear")})
    with pytest.raises(GdnError, match="written under.*None.*this run has.*cosine"):
        T._check_schedule(ns(lr_schedule="cosine"), sched, with_it, {"epoch": 0})
    with pytest.raises(GdnError, match="written under.*cosine.*this run has None"):
        T._check_schedule(ns(), None, without, {"schedule": dict(entry)})


def test_the_progress_line_shows_one_rate_per_group(capsys):
    from gdn_amd import trainer as T
    ns = argparse.Namespace
    T._print_lr(ns(schedule={"kind": "cosine"}, current_lr=lambda: [2e-5, 1e-5, None]))
    assert capsys.readouterr().out == "lr: 2.000000e-05  1.000000e-05  -\n"
    T._print_lr(ns(schedule=None, current_lr=lambda: 1 / 0))                  # no schedule: no device read, no line
    T._print_lr(torch.optim.Adam(torch.nn.Linear(2, 2).parameters()))
    assert capsys.readouterr().out == ""


# ---- state file -------------------------------------------------------------------------------------------------------
class _Loader:
    def state_dict(self, epoch_done=False):
        return {"pos": 0}

    def load_state_dict(self, state):
        self.got = state


def test_progress_carries_the_schedule_only_where_the_run_has_one():
    from gdn_amd import trainer as T
    from gdn_amd._lib import GdnError
    net = torch.nn.Linear(2, 2)
    opt = torch.optim.Adam(net.parameters())
    progress = {"epoch": 1, "i": 3, "lr": 1e-4, "model_num": 2, "seen": 16, "step": 8}
    entry = {"kind": "cosine", "warmup": 2, "total": 6, "floor": 0.1, "lr_schedule": "cosine"}
    off = T.training_state(net, opt, _Loader(), dict(progress))
    on = T.training_state(net, opt, _Loader(), dict(progress, schedule=dict(entry)))
    assert "schedule" not in off
    assert on["schedule"] == entry and [k for k in on if k != "schedule"] == list(off)
    assert T.load_training_state(off, net, opt, _Loader()) == progress
    # the optimizer being loaded into has no schedule: refused before anything is loaded
    before = {k: v.clone() for k, v in net.state_dict().items()}
    on["model"] = {k: v + 1 for k, v in on["model"].items()}
    with pytest.raises(GdnError, match="written under.*cosine.*this run has None"):
        T.load_training_state(on, net, opt, _Loader())
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def test_symbol_declared_built_and_bound_at_revision_223():
    from gdn_amd import _lib as L
    hdr = (REPO / "include" / "gdn_hip.h").read_text()
    assert re.search(r"\bint\s+gdn_lr_schedule\s*\(\s*float\s*\*\s*hyper,\s*const\s+double\s*\*\s*base_lr,\s*const\s+void\s*\*\s*states,"
                     r"\s*int32_t\s+G,\s*int32_t\s+kind,\s*int32_t\s+warmup,\s*int32_t\s+total,\s*double\s+floor,\s*void\s*\*\s*stream\)", hdr)
    dll = ctypes.CDLL(str(L.LIB_PATH))
    assert hasattr(dll, "gdn_lr_schedule") and "gdn_lr_schedule" in L._SIGS and "gdn_lr_schedule" in L.EXPORTS
    i32, P = ctypes.c_int32, ctypes.c_void_p
    assert L._SIGS["gdn_lr_schedule"] == (i32, [P, P, P, i32, i32, i32, i32, ctypes.c_double, P])
    assert L.ABI_VERSION == 223 and L.lib.gdn_version() == 223


def test_argument_checks_answer_before_any_launch():
    """GDN_ERR_BAD_ARG (-1) for every case of the header; the pointers are never dereferenced, so no GPU is needed.  Through
    gdn_amd the same answers are GdnErrors."""
    from gdn_amd import _lib as L
    P = ctypes.c_void_p
    f = L.lib.raw("gdn_lr_schedule")
    good = dict(hyper=P(0x1000), base=P(0x2000), states=P(0x3000), G=3, kind=2, warmup=3, total=8, floor=0.1)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["hyper"], a["base"], a["states"], a["G"], a["kind"], a["warmup"], a["total"], a["floor"], None)
    bad = [dict(hyper=None), dict(base=None), dict(states=None), dict(G=0), dict(G=-1), dict(G=255), dict(kind=-1), dict(kind=3),
           dict(warmup=-1), dict(total=0), dict(total=-5), dict(floor=-0.001), dict(floor=1.001), dict(floor=float("nan")),
           dict(floor=float("inf")), dict(base=P(0x2004)), dict(states=P(0x3004)), dict(hyper=P(0x1002))]
    for kw in bad:
        assert call(**kw) == -1, kw
    with pytest.raises(L.GdnError, match="gdn_lr_schedule failed: bad argument"):
        L.lib.gdn_lr_schedule(None, good["base"], good["states"], 3, 2, 3, 8, 0.1, None)


def test_ops_checks_its_tensors():
    from gdn_amd import ops
    from gdn_amd._lib import GdnError
    hyper, base, states = torch.zeros(2, 6), torch.zeros(2, dtype=torch.float64), torch.zeros(64, dtype=torch.uint8)
    for kw in (dict(hyper=torch.zeros(1, 6)), dict(base=torch.zeros(2)), dict(states=torch.zeros(32, dtype=torch.uint8)),
               dict(hyper=torch.zeros(2, 6, dtype=torch.float64))):
        a = dict(dict(hyper=hyper, base=base, states=states), **kw)
        with pytest.raises(GdnError, match="lr_schedule"):
            ops.lr_schedule(a["hyper"], a["base"], a["states"], "cosine", 3, 8, 0.1)


# ---- optimizer --------------------------------------------------------------------------------------------------------
def _params():
    torch.manual_seed(1)
    return [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(5))]


def test_no_schedule_is_the_optimizer_it_was():
    from gdn_amd.optim import Adam
    opt = Adam(_params(), lr=1e-3, schedule=None)
    assert opt.schedule is None and not opt.capturable
    sd = opt.state_dict()
    assert "schedule" not in sd["gdn"] and sorted(sd["gdn"]) == ["capturable", "grad_scale", "stores", "version"]
    assert sd["gdn"] == Adam(_params(), lr=1e-3).state_dict()["gdn"]


def test_a_schedule_makes_it_capturable_and_rides_in_the_state_dict():
    from gdn_amd.optim import Adam
    from gdn_amd._lib import GdnError
    sched = {"kind": "cosine", "warmup": 3, "total": 8, "floor": 0.1}
    opt = Adam(_params(), lr=1e-3, schedule=sched)
    assert opt.capturable and opt.schedule == sched and opt.schedule is not sched
    sd = opt.state_dict()
    assert sd["gdn"]["schedule"] == sched
    Adam(_params(), lr=1e-3, schedule=dict(sched)).load_state_dict(sd)
    other = Adam(_params(), lr=1e-3, schedule=dict(sched, kind="linear"))
    with pytest.raises(GdnError, match="'cosine'.*'linear'"):
        other.load_state_dict(sd)
    with pytest.raises(GdnError, match="'cosine'.*None"):
        Adam(_params(), lr=1e-3, capturable=True).load_state_dict(sd)
    with pytest.raises(GdnError, match="None.*'cosine'"):
        opt.load_state_dict(Adam(_params(), lr=1e-3, capturable=True).state_dict())
    with pytest.raises(GdnError, match="'total': 8.*'total': 9"):
        Adam(_params(), lr=1e-3, schedule=dict(sched, total=9)).load_state_dict(sd)


@pytest.mark.parametrize("bad", [{"kind": "exponential", "warmup": 0, "total": 8, "floor": 0.0},
                                 {"kind": "cosine", "warmup": -1, "total": 8, "floor": 0.0},
                                 {"kind": "cosine", "warmup": 0, "total": 0, "floor": 0.0},
                                 {"kind": "cosine", "warmup": 0, "total": 8, "floor": 1.5},
                                 {"kind": "cosine", "warmup": 0, "total": 8, "floor": float("nan")},
                                 {"warmup": 0, "total": 8}, {"kind": "cosine", "steps": 8}])
def test_a_bad_schedule_is_refused(bad):
    from gdn_amd.optim import Adam
    with pytest.raises(ValueError, match="schedule"):
        Adam(_params(), lr=1e-3, schedule=bad)


def test_the_launch_sits_in_front_of_the_update_and_the_base_rate_follows_the_group(monkeypatch):
    """On a CPU arena with the library calls recorded: one lr_schedule call per update, before it, with the store's own
    table and step state and a float64 base rate of lr * lr_mult that is rewritten in place when group['lr'] changes."""
    from gdn_amd import engine as E
    from gdn_amd import ops
    from gdn_amd.optim import Adam
    calls = []
    monkeypatch.setattr(ops, "zeros", lambda shape, device: torch.zeros(shape, dtype=torch.float32, device=device))
    monkeypatch.setattr(ops, "adam_step_dev", lambda p, g, m, v, hyper, state: calls.append(("adam", hyper, state)))
    monkeypatch.setattr(ops, "lr_schedule", lambda hyper, base, states, kind, warmup, total, floor:
                        calls.append(("lr", hyper, states, base, base.clone(), (kind, warmup, total, floor))))
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3), torch.nn.BatchNorm2d(3))
    ar = E.ParamArena(net, torch.device("cpu"))
    net._gdn_param_arena = ar
    ar.bind_grads()
    ar.grad.copy_(torch.randn(ar.numel, generator=torch.Generator().manual_seed(5)))
    opt = Adam([{"params": list(net.parameters()), "lr_mult": 0.5}], lr=2e-5, schedule={"kind": "linear", "warmup": 2, "total": 9, "floor": 0.25})
    opt.step()
    opt.step()
    opt.param_groups[0]["lr"] = 1e-5
    opt.step()
    assert [c[0] for c in calls] == ["lr", "adam"] * 3
    (st,) = opt._stores.values()
    for lr_call, adam_call in zip(calls[0::2], calls[1::2]):
        assert lr_call[1] is st.hyper and adam_call[1] is st.hyper and lr_call[2] is st.state and adam_call[2] is st.state
        assert lr_call[3] is st.base_lr and lr_call[3].dtype == torch.float64 and lr_call[5] == ("linear", 2, 9, 0.25)
    assert [c[4].item() for c in calls[0::2]] == [2e-5 * 0.5, 2e-5 * 0.5, 1e-5 * 0.5]
    # without a schedule nothing of this is launched
    del calls[:]
    opt = Adam(net.parameters(), lr=2e-5, capturable=True)
    opt.step()
    assert [c[0] for c in calls] == ["adam"]
