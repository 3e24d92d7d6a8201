"""Decoupled weight decay (--optimizer adamw, Adam(decoupled=True) / AdamW, gdn_adamw_step*): what needs no
GPU -- the restatement against torch.optim.AdamW in float64, why the decay is summed into the update and not multiplied into
the weight, the flags and their refusals, the C ABI's declarations and argument checks, and the optimizer's extra key."""
import ctypes
import fractions
import pathlib
import re

import numpy as np
import pytest
import torch

import adamw_fp64 as R

REPO = pathlib.Path(__file__).resolve().parent.parent
BASE = ["synthetic", "--synthetic"]
NAMES = ("gdn_adamw_step", "gdn_adamw_step_dev", "gdn_adamw_step_dev_guarded", "gdn_adamw_step_seg")
SIBLING = {n: n.replace("adamw", "adam") for n in NAMES}


# ---- the restatement --------------------------------------------------------------------------------------------------
def test_float64_restatement_is_torch_adamw():
    """Three steps, two groups, one of them without decay: rtol 1e-12 (the two differ in the order of the additions only)."""
    gen = torch.Generator().manual_seed(5)
    shapes = [(7, 5), (33,), (4, 3, 3, 3)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in shapes]
    groups = [dict(params=params[:2], lr=0.5, weight_decay=0.3), dict(params=params[2:], lr=2e-5, weight_decay=0.0)]
    opt = torch.optim.AdamW(groups, betas=(0.9, 0.999), eps=1e-8)
    mine = [(p.detach().numpy().copy(), np.zeros(p.shape), np.zeros(p.shape)) for p in params]
    hyper = [(0.5, 0.3), (0.5, 0.3), (2e-5, 0.0)]
    for t in range(1, 4):
        for k, p in enumerate(params):
            p.grad = torch.randn(p.shape, generator=gen, dtype=torch.float64) * 10.0 ** (k - 2)
            lr, wd = hyper[k]
            mine[k] = R.step64(*mine[k][:1], p.grad.numpy(), *mine[k][1:], lr, 0.9, 0.999, 1e-8, wd, t)
        opt.step()
    for k, p in enumerate(params):
        np.testing.assert_allclose(mine[k][0], p.detach().numpy(), rtol=1e-12, atol=0.0)
        st = opt.state[p]
        np.testing.assert_allclose(mine[k][1], st["exp_avg"].numpy(), rtol=1e-12, atol=0.0)
        np.testing.assert_allclose(mine[k][2], st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0.0)


def test_float32_restatement_rounds_the_fma_once():
    f32, F = np.float32, fractions.Fraction
    # a tie: 1 + 2^-24 lies midway between 1 and 1 + 2^-23 and goes to the even one; a product that two roundings get wrong
    assert R.round32(F(1) + F(1, 2 ** 24)) == f32(1.0)
    assert R.round32(F(1) + F(3, 2 ** 24)) == f32(1.0) + f32(2.0 ** -22)
    assert R.round32(F(1) + F(1, 2 ** 24) + F(1, 2 ** 60)) == np.nextafter(f32(1), f32(2))
    a, c = f32(1.0) + f32(2.0 ** -12), f32(-1.0)                         # a * a = 1 + 2^-11 + 2^-24, a tie in float32
    assert R.fma32(a, a, c) == f32(2.0 ** -11 + 2.0 ** -24)              # the fma keeps the 2^-24 ...
    assert f32(a * a) + c == f32(2.0 ** -11)                             # ... a product rounded first loses it
    rng = np.random.default_rng(3)
    x, y, z = (rng.standard_normal(200).astype(f32) for _ in range(3))
    got = R.fma32(x, y, z)
    twice = (x.astype(np.float64) * y.astype(np.float64) + z).astype(f32)       # (rounded in double, then again)
    assert got.dtype == f32 and np.max(R.ulps32(got, twice)) <= 1 and np.mean(got == twice) > 0.99


def test_dec_zero_is_the_coupled_element_without_decay():
    """With wd = 0 the restated element is pi - q: fma(0, pi, q) is q."""
    rng = np.random.default_rng(4)
    p, g = rng.standard_normal(64).astype(np.float32), rng.standard_normal(64).astype(np.float32)
    z = np.zeros(64, np.float32)
    bc1, bc2s = R.corrections(0.9, 0.999, 1)
    got, m, v = R.step32(p, g, z, z, 0.5, 0.9, 0.999, 1e-8, 0.0, bc1, bc2s, 0.5)
    q = (np.float32(0.5) / bc1 * m) / (np.sqrt(v) / bc2s + np.float32(1e-8))
    assert np.array_equal(got, p - q)


def test_the_coupled_form_of_the_float32_restatement():
    """step32(coupled=True), the element of gdn_adam_step*: without decay the decoupled form's bits; with it the moments see
    g + wd p (one rounding: the fma) and the result follows torch.optim.Adam in float64 to float32 accuracy."""
    rng = np.random.default_rng(6)
    p, g = rng.standard_normal(256).astype(np.float32), rng.standard_normal(256).astype(np.float32)
    z = np.zeros(256, np.float32)
    bc1, bc2s = R.corrections(0.9, 0.999, 1)
    for a, b in zip(R.step32(p, g, z, z, 0.5, 0.9, 0.999, 1e-8, 0.0, bc1, bc2s, 0.5, coupled=True),
                    R.step32(p, g, z, z, 0.5, 0.9, 0.999, 1e-8, 0.0, bc1, bc2s, 0.5)):
        assert np.array_equal(a, b)
    got, m, v = R.step32(p, g, z, z, 0.5, 0.9, 0.999, 1e-8, 0.3, bc1, bc2s, 0.5, coupled=True)
    gi = R.fma32(np.float32(0.3), p, g * np.float32(0.5))
    assert np.array_equal(m, (np.float32(1) - np.float32(0.9)) * gi)
    q = (np.float32(0.5) / bc1 * m) / (np.sqrt(v) / bc2s + np.float32(1e-8))
    assert np.array_equal(got, p - q)
    theirs = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    theirs.grad = torch.from_numpy(g.astype(np.float64) * 0.5)
    torch.optim.Adam([theirs], lr=0.5, betas=(0.9, 0.999), eps=1e-8, weight_decay=float(np.float32(0.3))).step()
    np.testing.assert_allclose(got, theirs.detach().numpy(), rtol=0, atol=4e-6)      # |p| < 8: a few float32 ulps of it


def test_the_host_and_the_device_corrections_agree_for_the_first_updates():
    """gdn_adamw_step takes pow(beta, t) in double, the device multiplies t times: the float32 corrections the kernels read are
    the same for the betas and the counts the GPU tests compare the entry points at."""
    for b1, b2 in ((0.9, 0.999), (0.8, 0.99)):
        for t in (1, 2, 3):
            f1, f2 = float(np.float32(b1)), float(np.float32(b2))
            host = (np.float32(1.0 - f1 ** t), np.float32(np.sqrt(1.0 - f2 ** t)))
            assert host == R.corrections(b1, b2, t)


def test_why_the_decay_is_summed_and_not_multiplied():
    """At the project's rate and the reference's decay the float32 factor 1 - lr wd IS 1: p * (1 - lr wd) decays nothing,
    while dec is non-zero and rides into the weight on the Adam term.  At wd 1e-2 the factor is 3 ulp below 1.
    (dec * p alone, 1e-8 |p|, is below half an ulp of p: on a weight whose moments are zero a zero gradient moves nothing in
    either form.  The decay reaches the weight because it is added to q, whose ulp is four orders finer, BEFORE the one
    subtraction: a step with zero gradient on moments that are not zero moves a share of the weights one ulp further than
    the same step without decay, about dec |p| / ulp(p) of them, which is the decay on average.)"""
    f32 = np.float32
    lr, wd = f32(2e-5), f32(5e-4)
    assert f32(1.0) - lr * wd == f32(1.0)
    assert f32(1.0) - f32(float(lr) * float(wd)) == f32(1.0)
    assert 2e-5 * 5e-4 < 2.0 ** -25
    one = f32(1.0)
    assert int(one.view(np.uint32)) - int((one - f32(2e-5) * f32(1e-2)).view(np.uint32)) == 3
    dec = R.dec32(2e-5, 5e-4)
    assert dec > 0 and abs(float(dec) - 1e-8) < 1e-15
    p = np.array([0.75, -1.5, 1e-3], f32)
    z = np.zeros(3, f32)
    bc1, bc2s = R.corrections(0.9, 0.999, 1)
    got, m, v = R.step32(p, z, z, z, 2e-5, 0.9, 0.999, 1e-8, 5e-4, bc1, bc2s, 1.0)
    assert not m.any() and not v.any()
    assert np.array_equal(got, p - (dec * p)) and np.array_equal(got, p)
    assert np.array_equal(p * (f32(1.0) - lr * wd), p)                   # the multiplicative form: nothing moved
    # one update with a gradient, then one with a zero gradient: the moments carry an Adam term of about lr
    rng = np.random.default_rng(9)
    p = rng.standard_normal(1000).astype(f32)
    g = rng.standard_normal(1000).astype(f32)
    z = np.zeros(1000, f32)
    runs = {}
    for name, decay in (("summed", 5e-4), ("none", 0.0)):
        q, m, v = R.step32(p, g, z, z, 2e-5, 0.9, 0.999, 1e-8, decay, *R.corrections(0.9, 0.999, 1), 1.0)
        runs[name] = R.step32(q, z, m, v, 2e-5, 0.9, 0.999, 1e-8, decay, *R.corrections(0.9, 0.999, 2), 1.0)
    moved = runs["summed"][0] != runs["none"][0]
    share = float(np.mean(moved))
    print("zero-gradient step at (2e-5, 5e-4): %.1f %% of the weights carry the decay (one ulp towards zero)" % (100 * share))
    # dec |p| / ulp(p) lies between 1e-8 / 2^-23 and 1e-8 / 2^-24 per step, two steps: 17 % to 34 %, less sampling noise
    assert 0.10 < share < 0.45
    assert np.all(np.abs(runs["summed"][0][moved]) < np.abs(runs["none"][0][moved]))
    assert np.array_equal(runs["summed"][1], runs["none"][1]) and np.array_equal(runs["summed"][2], runs["none"][2])
    mult = runs["none"][0] * (f32(1.0) - lr * wd)                         # the multiplicative form decays none of them
    assert np.array_equal(mult, runs["none"][0])


# ---- command line -----------------------------------------------------------------------------------------------------
def _no_gpu_calls(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the check touched the GPU")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "is_initialized", boom)


def test_parser_defaults_and_values():
    from gdn_amd import option
    a = option.parse_args(BASE)
    assert (a.optimizer, a.decoupled_wd) == ("adam", None) and option.decoupled_wd(a) is None
    a = option.parse_args(BASE + ["--optimizer", "adamw"])
    assert a.decoupled_wd is None and option.decoupled_wd(a) == 1e-2
    a = option.parse_args(BASE + ["--optimizer", "adamw", "--decoupled_wd", "0.05", "--weight-decay", "7"])
    assert option.decoupled_wd(a) == 0.05 and a.weight_decay == 7.0
    assert option.decoupled_wd(option.parse_args(BASE + ["--optimizer", "adamw", "--decoupled_wd", "0"])) == 0.0
    text = " ".join(option.build_parser().format_help().split())
    assert "--optimizer" in text and "--decoupled_wd" in text and "usual AdamW practice" in text


@pytest.mark.parametrize("flag,bad", [("--optimizer", "sgd"), ("--decoupled_wd", "-1e-2"), ("--decoupled_wd", "nan"),
                                      ("--decoupled_wd", "x")])
def test_parser_refuses(flag, bad, capsys):
    from gdn_amd import option
    with pytest.raises(SystemExit):
        option.parse_args(BASE + [flag, bad])
    assert flag in capsys.readouterr().err


@pytest.mark.parametrize("mode", ["DtoD_test", "RtoD_test"])
def test_a_test_mode_is_refused_before_the_gpu(monkeypatch, mode):
    from gdn_amd import GDN_main, option
    _no_gpu_calls(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(RuntimeError, match="--optimizer adamw.*trains nothing"):
        GDN_main.run(option.parse_args(BASE + ["--mode", mode, "--optimizer", "adamw"]))
    GDN_main._check_optimizer(option.parse_args(BASE + ["--mode", mode, "--optimizer", "adam"]))


@pytest.mark.parametrize("extra", [[], ["--optimizer", "adam"]])
def test_a_decay_without_adamw_is_refused_before_the_gpu(monkeypatch, extra):
    from gdn_amd import GDN_main, option
    _no_gpu_calls(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(RuntimeError, match="--decoupled_wd.*--optimizer adamw"):
        GDN_main.run(option.parse_args(BASE + ["--mode", "DtoD", "--decoupled_wd", "0.01"] + extra))
    GDN_main._check_optimizer(option.parse_args(BASE + ["--mode", "DtoD", "--optimizer", "adamw", "--decoupled_wd", "0.01"]))


def test_make_optimizer_passes_the_decay_decoupled():
    from gdn_amd import GDN_main, option
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3), torch.nn.BatchNorm2d(3))
    opt = GDN_main._make_optimizer(net, option.parse_args(BASE))
    assert not opt.decoupled and not opt.capturable and opt.defaults["weight_decay"] == 5e-4
    opt = GDN_main._make_optimizer(net, option.parse_args(BASE + ["--optimizer", "adamw"]))
    assert opt.decoupled and not opt.capturable and opt.defaults["weight_decay"] == 1e-2
    net.select_parameters = lambda spec: []
    opt = GDN_main._make_optimizer(net, option.parse_args(BASE + ["--optimizer", "adamw", "--decoupled_wd", "0.05", "--no_decay_norm"]))
    assert opt.decoupled and opt.segmented
    assert sorted((g["weight_decay"], sorted(p.dim() for p in g["params"])) for g in opt.param_groups) == \
        [(0.0, [1, 1, 1]), (0.05, [4])]


def test_announcement(capsys):
    from gdn_amd import GDN_main, option
    GDN_main._announce_optimizer(option.parse_args(BASE), 0)
    GDN_main._announce_optimizer(option.parse_args(BASE + ["--optimizer", "adamw"]), 1)
    assert capsys.readouterr().out == ""
    GDN_main._announce_optimizer(option.parse_args(BASE + ["--optimizer", "adamw"]), 0)
    assert capsys.readouterr().out == "=> optimizer: AdamW, decoupled weight decay 0.01\n"


# ---- optimizer --------------------------------------------------------------------------------------------------------
def _params():
    torch.manual_seed(1)
    return [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(5))]


def _cpu_arena(monkeypatch, calls):
    """A CPU arena with every Adam entry point of ops recorded in place of its launch."""
    from gdn_amd import engine as E
    from gdn_amd import ops
    monkeypatch.setattr(ops, "zeros", lambda shape, device: torch.zeros(shape, dtype=torch.float32, device=device))
    for name in ("adam_step", "adam_step_dev", "adam_step_dev_guarded", "adam_step_seg", "adamw_step", "adamw_step_dev",
                 "adamw_step_dev_guarded", "adamw_step_seg", "grad_sumsq", "grad_sumsq_seg", "grad_guard_finalize",
                 "ema_update", "ema_update_seg", "lr_schedule"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3), torch.nn.BatchNorm2d(3))
    ar = E.ParamArena(net, torch.device("cpu"))
    net._gdn_param_arena = ar
    ar.bind_grads()
    ar.grad.copy_(torch.randn(ar.numel, generator=torch.Generator().manual_seed(5)))
    return net, ar


PATHS = [({}, ["adam_step"]), ({"capturable": True}, ["adam_step_dev"]),
         ({"max_grad_norm": 1.0}, ["grad_sumsq", "grad_guard_finalize", "adam_step_dev_guarded"]),
         ({"segmented": True, "ema_decay": 0.9}, ["adam_step_seg", "ema_update_seg"]),
         ({"segmented": True, "skip_nonfinite": True, "schedule": {"kind": "cosine", "warmup": 1, "total": 4, "floor": 0.0}},
          ["grad_sumsq_seg", "grad_guard_finalize", "lr_schedule", "adam_step_seg"])]


@pytest.mark.parametrize("kw,want", PATHS, ids=["host", "capturable", "guarded", "segmented", "segmented-guarded-scheduled"])
def test_every_path_calls_the_adamw_entry_point_in_its_siblings_place(monkeypatch, kw, want):
    """decoupled=False makes the calls it always made -- no new library call; decoupled=True the same calls with the adamw
    update where the adam update was."""
    from gdn_amd.optim import Adam, AdamW
    for cls, extra, swap in ((Adam, {}, False), (Adam, {"decoupled": False}, False), (Adam, {"decoupled": True}, True),
                             (AdamW, {}, True)):
        calls = []
        net, ar = _cpu_arena(monkeypatch, calls)
        opt = cls(net.parameters(), lr=2e-5, **kw, **extra)
        assert opt.decoupled == swap and opt.capturable == bool(kw)
        opt.step()
        opt.step()
        assert calls == [n.replace("adam_step", "adamw_step") if swap else n for n in want] * 2, (cls, extra)


def test_the_per_tensor_fallback_calls_it_too(monkeypatch):
    from gdn_amd.optim import AdamW
    for kw, name in (({}, "adamw_step"), ({"capturable": True}, "adamw_step_dev"), ({"segmented": True}, "adamw_step_dev")):
        calls = []
        net, ar = _cpu_arena(monkeypatch, calls)
        opt = AdamW(net.parameters(), lr=2e-5, **kw)
        list(net.parameters())[1].grad = None                         # one parameter sits out: per tensor
        opt.step()
        assert calls == [name] * 3, kw


def test_decoupled_off_is_the_optimizer_it_was():
    from gdn_amd.optim import Adam
    opt = Adam(_params(), lr=1e-3, decoupled=False)
    assert opt.decoupled is False and not opt.capturable
    sd = opt.state_dict()
    assert sorted(sd["gdn"]) == ["capturable", "grad_scale", "stores", "version"]
    assert sd["gdn"] == Adam(_params(), lr=1e-3).state_dict()["gdn"]
    assert sorted(sd["param_groups"][0]) == sorted(Adam(_params(), lr=1e-3).state_dict()["param_groups"][0])
    assert "decoupled" not in opt.defaults and "decoupled" not in sd["param_groups"][0]


def test_decoupled_rides_in_the_state_dict_and_the_other_kind_is_refused():
    from gdn_amd.optim import Adam, AdamW
    from gdn_amd._lib import GdnError
    opt = AdamW(_params(), lr=1e-3)
    assert opt.decoupled and not opt.capturable and opt.defaults["weight_decay"] == 1e-2
    sd = opt.state_dict()
    assert sd["gdn"]["decoupled"] is True
    assert sorted(sd["gdn"]) == ["capturable", "decoupled", "grad_scale", "stores", "version"]
    Adam(_params(), lr=1e-3, decoupled=True).load_state_dict(sd)
    coupled = Adam(_params(), lr=1e-3, weight_decay=5e-4)
    with pytest.raises(GdnError, match="decoupled \\(AdamW\\) weight decay loaded into .* coupled"):
        coupled.load_state_dict(sd)
    assert coupled.param_groups[0]["weight_decay"] == 5e-4               # refused before the groups were taken
    with pytest.raises(GdnError, match="coupled \\(Adam, L2\\) weight decay loaded into .* decoupled"):
        opt.load_state_dict(coupled.state_dict())
    # a dict without the 'gdn' key loads as ever: torch's AdamW and torch's Adam, into either kind
    for theirs in (torch.optim.AdamW(_params(), lr=1e-3), torch.optim.Adam(_params(), lr=1e-3, weight_decay=5e-4)):
        for mine in (AdamW(_params(), lr=1e-3), Adam(_params(), lr=1e-3)):
            mine.load_state_dict(theirs.state_dict())
            assert mine.param_groups[0]["weight_decay"] == theirs.param_groups[0]["weight_decay"]
    with pytest.raises(ValueError, match="decoupled"):
        AdamW(_params(), decoupled=False)


class _Loader:
    def state_dict(self, epoch_done=False):
        return {"pos": 0}

    def load_state_dict(self, state):
        self.got = state


def test_the_state_file_refuses_the_other_optimizer_before_anything_is_loaded():
    from gdn_amd import trainer as T
    from gdn_amd.optim import Adam, AdamW
    from gdn_amd._lib import GdnError
    net = torch.nn.Linear(2, 2)
    progress = {"epoch": 1, "i": 3, "lr": 1e-4, "model_num": 2, "seen": 16, "step": 8}
    on = T.training_state(net, AdamW(net.parameters(), lr=1e-3), _Loader(), dict(progress))
    off = T.training_state(net, Adam(net.parameters(), lr=1e-3), _Loader(), dict(progress))
    assert on["optimizer"]["gdn"]["decoupled"] is True and "decoupled" not in off["optimizer"]["gdn"]
    assert list(on) == list(off)
    assert T.load_training_state(on, net, AdamW(net.parameters(), lr=1e-3), _Loader()) == progress
    assert T.load_training_state(off, net, Adam(net.parameters(), lr=1e-3), _Loader()) == progress
    before = {k: v.clone() for k, v in net.state_dict().items()}
    for state, opt, msg in ((on, Adam(net.parameters(), lr=1e-3), "written under --optimizer adamw, this run has --optimizer adam:"),
                            (off, AdamW(net.parameters(), lr=1e-3), "written under --optimizer adam, this run has --optimizer adamw:")):
        state = dict(state, model={k: v + 1 for k, v in state["model"].items()})
        with pytest.raises(GdnError, match=msg):
            T.load_training_state(state, net, opt, _Loader())
        assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def _prototype(hdr, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    return " ".join(m.group(1).split())


def test_symbols_declared_built_and_bound_at_revision_223():
    from gdn_amd import _lib as L
    hdr = (REPO / "include" / "gdn_hip.h").read_text()
    dll = ctypes.CDLL(str(L.LIB_PATH))
    for name in NAMES:
        assert _prototype(hdr, name) == _prototype(hdr, SIBLING[name]), name          # the sibling's argument list
        assert hasattr(dll, name) and name in L.EXPORTS and name in L._STATUS_FUNCS, name
        assert L._SIGS[name] == L._SIGS[SIBLING[name]], name
    assert L.ABI_VERSION == 223 and L.lib.gdn_version() == 223


def test_argument_checks_answer_before_any_launch():
    """GDN_ERR_BAD_ARG (-1) for every case the coupled entry points refuse, from both of each pair; the pointers are never
    dereferenced, so no GPU is needed.  Through gdn_amd the same answers are GdnErrors."""
    from gdn_amd import _lib as L
    P = ctypes.c_void_p
    bufs = dict(p=P(0x10000), g=P(0x20000), m=P(0x30000), v=P(0x40000))
    host = dict(bufs, n=1000, lr=2e-5, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=1, gs=1.0)
    dev = dict(bufs, n=1000, hyper=P(0x50000), state=P(0x60000))
    grd = dict(dev, guard=P(0x70000))
    seg = dict(bufs, n=4096, map=P(0x80000), G=3, hyper=P(0x50000), states=P(0x60000), guard=None)
    order = {"gdn_adamw_step": ("p", "g", "m", "v", "n", "lr", "b1", "b2", "eps", "wd", "step", "gs"),
             "gdn_adamw_step_dev": ("p", "g", "m", "v", "n", "hyper", "state"),
             "gdn_adamw_step_dev_guarded": ("p", "g", "m", "v", "n", "hyper", "state", "guard"),
             "gdn_adamw_step_seg": ("p", "g", "m", "v", "n", "map", "G", "hyper", "states", "guard")}
    nulls = [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(n=-4)]
    cases = {"gdn_adamw_step": (host, nulls + [dict(step=0), dict(step=-1)]),
             "gdn_adamw_step_dev": (dev, nulls + [dict(hyper=None), dict(state=None)]),
             "gdn_adamw_step_dev_guarded": (grd, nulls + [dict(hyper=None), dict(state=None), dict(guard=None)]),
             "gdn_adamw_step_seg": (seg, nulls + [dict(hyper=None), dict(states=None), dict(map=None), dict(n=4095), dict(n=100),
                                                  dict(G=0), dict(G=255), dict(p=P(0x10004)), dict(g=P(0x20008)),
                                                  dict(m=P(0x3000c)), dict(v=P(0x40004)), dict(hyper=P(0x50002)),
                                                  dict(states=P(0x60004)), dict(guard=P(0x70004))])}
    for name, (good, bad) in cases.items():
        for kw in bad:
            a = dict(good, **kw)
            args = [a[k] for k in order[name]] + [None]
            assert L.lib.raw(name)(*args) == -1, (name, kw)
            assert L.lib.raw(SIBLING[name])(*args) == -1, (SIBLING[name], kw)
    with pytest.raises(L.GdnError, match="gdn_adamw_step_seg failed: bad argument"):
        L.lib.gdn_adamw_step_seg(None, seg["g"], seg["m"], seg["v"], 4096, seg["map"], 3, seg["hyper"], seg["states"], None, None)


def test_ops_checks_its_tensors():
    from gdn_amd import ops
    from gdn_amd._lib import GdnError
    z = torch.zeros(256)
    cmap, hyper, states = torch.zeros(4, dtype=torch.uint8), torch.zeros(1, 6), torch.zeros(32, dtype=torch.uint8)
    with pytest.raises(GdnError, match="chunk map"):
        ops.adamw_step_seg(z, z, z, z, cmap[:-1], hyper, states)
    with pytest.raises(GdnError, match="step states"):
        ops.adamw_step_seg(z, z, z, z, cmap, hyper, torch.cat([states, states]))
