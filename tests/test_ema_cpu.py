"""Weight average of the fused Adam (Adam(ema_decay=), --ema_decay): what needs no GPU -- the float64 restatement the GPU
tests compare against and its bound, the command-line flag, the optimizer's constructor and state-dict contract, the C ABI's
declarations and the argument checks that answer before any launch."""
import ctypes
import pathlib
import re

import numpy as np
import pytest
import torch

import ema_fp64 as R

REPO = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ("gdn_ema_update", "gdn_swap_f32")
PLAIN_KEYS = ["capturable", "grad_scale", "stores", "version"]


# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_weight():
    """w_1 = 1 - 2/11; the warm-up ends where (1 + t) / (10 + t) >= 0.999, i.e. 0.001 t >= 8.99: from t = 8990 on and not
    before.  (The issue names t = 8981 for this; that figure contradicts its own formula and its own w_1 = 9/11 -- it is
    the threshold of t / (9 + t), for which w_1 would be 0.9 -- so the formula decides.)"""
    assert R.weight(0.999, 1) == np.float32(9 / 11)
    assert R.weight(0.999, 1).dtype == np.float32
    floor = np.float32(1 - 0.999)
    first = next(t for t in range(1, 20000) if R.weight(0.999, t) == floor)
    print("weight(0.999, t) reaches float32(1 - 0.999) = %.9g at t = %d" % (floor, first))
    assert first == 8990
    assert all(R.weight(0.999, t) > floor for t in range(1, 8990))
    assert all(R.weight(0.999, t) == floor for t in (8990, 8991, 20000, 10 ** 6, 2 ** 31 - 1))
    assert R.weight(0.9, 5) == np.float32(1.0 - 6.0 / 15.0) and R.weight(0.5, 8) == np.float32(0.5)
    assert R.weight(0.5, 7) == np.float32(1.0 - 8.0 / 17.0)
    assert R.weight(0.001, 20000) == np.float32(0.999)


def test_float32_model_stays_within_the_bound():
    """40 updates of 200,000 elements spanning 1e-6 ... 1e2 in the kernel's own float32 arithmetic against the float64
    restatement: within bound(k, M) after every step (the issue reports 0.28 of it for its own draw of this model;
    this one prints its figure)."""
    rng = np.random.default_rng(20261018)
    n, decay = 200_000, 0.999
    p = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)).astype(np.float32)
    e32, e64 = p.copy(), p.astype(np.float64)
    M = np.abs(e64)
    worst = 0.0
    for k in range(1, 41):
        p = (p + rng.standard_normal(n).astype(np.float32) * np.float32(0.05) * np.abs(p)).astype(np.float32)
        e32 = R.update32(e32, p, R.weight(decay, k))
        e64 = R.update(e64, p, decay, k)
        M = np.maximum(M, np.maximum(np.abs(p.astype(np.float64)), np.abs(e64)))
        err, lim = np.abs(e32.astype(np.float64) - e64), R.bound(k, M)
        assert np.all(err <= lim), (k, float((err / lim).max()))
        worst = max(worst, float((err / lim).max()))
    print("float32 model: worst error %.3f of the bound" % worst)
    assert 0.0 < worst <= 1.0
    assert R.bound(3, 2.0) == 3 * 2.0 ** -22 * 2.0


def test_restatement_update_and_state_record():
    e = R.update(np.array([1.0, -2.0]), np.array([3.0, -2.0], np.float32), 0.999, 1)
    w = float(np.float32(9 / 11))
    assert e.dtype == np.float64 and e[0] == 1.0 + w * 2.0 and e[1] == -2.0
    import struct
    raw = R.state_record(20000)
    assert len(raw) == 32 and struct.unpack_from("<i", raw, 16)[0] == 20000


# ---------------------------------------------------------------------------------------------------------------------
def test_flag(capsys):
    from gdn_amd import option
    assert option.parse_args(["--synthetic"]).ema_decay == 0
    assert option.parse_args(["--synthetic", "--ema_decay", "0.999"]).ema_decay == 0.999
    assert option.parse_args(["--synthetic", "--ema_decay", "0"]).ema_decay == 0
    for bad in ("1.0", "-0.1", "nan"):
        with pytest.raises(SystemExit) as e:
            option.parse_args(["--synthetic", "--ema_decay", bad])
        assert e.value.code != 0
        assert "ema_decay" in capsys.readouterr().err
    helps = option.parser.format_help()
    assert "running statistics" in helps and "one more copy" in helps


def test_test_modes_refuse_the_flag_before_touching_a_gpu(monkeypatch):
    from gdn_amd import GDN_main, option
    from gdn_amd import distributed as D

    def touched(*a, **k):
        raise AssertionError("the run went past the argument checks")
    monkeypatch.setattr(D, "env_rank", touched)
    monkeypatch.setattr(D, "init", touched)
    for mode in ("DtoD_test", "RtoD_test"):
        args = option.parse_args(["--synthetic", "--mode", mode, "--ema_decay", "0.9"])
        with pytest.raises(RuntimeError, match="trains nothing"):
            GDN_main.run(args)


def test_make_optimizer_passes_the_flag_on():
    from gdn_amd import GDN_main, option
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4))
    plain = GDN_main._make_optimizer(net, option.parse_args(["--synthetic"]))
    assert plain.ema_decay is None and plain.capturable is False
    assert sorted(plain.state_dict()["gdn"]) == PLAIN_KEYS
    ema = GDN_main._make_optimizer(net, option.parse_args(["--synthetic", "--ema_decay", "0.99"]))
    assert ema.ema_decay == 0.99 and ema.capturable is True and ema.guarded is False
    both = GDN_main._make_optimizer(net, option.parse_args(["--synthetic", "--ema_decay", "0.5", "--skip_nonfinite"]))
    assert both.ema_decay == 0.5 and both.guarded is True


def _params():
    gen = torch.Generator().manual_seed(5)
    return [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in ((4, 3, 3, 3), (4,), (7,))]


def test_constructor_contract():
    from gdn_amd._lib import GdnError
    from gdn_amd.optim import Adam
    p = _params()
    for bad in (0, 1, -1, 0.0, 1.0, float("nan")):
        with pytest.raises(ValueError):
            Adam(p, ema_decay=bad)
    assert Adam(p).ema_decay is None and Adam(p).capturable is False
    opt = Adam(p, ema_decay=0.999)
    assert opt.capturable is True and opt.guarded is False and opt.ema_decay == 0.999
    for call in (Adam(p).swap_averaged, lambda: Adam(p).averaged(p[0])):
        with pytest.raises(GdnError):
            call()
    # before any step the average of a parameter is the parameter
    assert all(torch.equal(opt.averaged(q), q.detach()) for q in p)


def test_state_dict_contract(capsys):
    from gdn_amd.optim import Adam
    p = _params()
    plain = Adam(p)
    assert sorted(plain.state_dict()["gdn"]) == PLAIN_KEYS
    assert sorted(Adam(p, capturable=True).state_dict()["gdn"]) == PLAIN_KEYS
    opt = Adam(p, ema_decay=0.999)
    sd = opt.state_dict()
    assert sorted(sd["gdn"]) == sorted(PLAIN_KEYS + ["ema"])
    assert sd["gdn"]["ema"]["decay"] == 0.999 and sorted(sd["gdn"]["ema"]["avg"]) == [0, 1, 2]
    for k, q in enumerate(p):
        a = sd["gdn"]["ema"]["avg"][k]
        assert a.shape == q.shape and a.is_contiguous() and torch.equal(a, q.detach()) and a.data_ptr() != q.data_ptr()
    # save -> load before any step hands back equal averages (made to differ from the weights, so a copy shows)
    gen = torch.Generator().manual_seed(6)
    sd["gdn"]["ema"]["avg"] = {k: torch.randn(q.shape, generator=gen) for k, q in enumerate(p)}
    fresh = Adam(p, ema_decay=0.5)
    fresh.load_state_dict(sd)
    back = fresh.state_dict()["gdn"]["ema"]
    assert back["decay"] == 0.5                       # the constructor's, not the checkpoint's
    for k, q in enumerate(p):
        assert torch.equal(back["avg"][k], sd["gdn"]["ema"]["avg"][k]) and torch.equal(fresh.averaged(q), back["avg"][k])
    assert "no weight average" not in capsys.readouterr().out
    # a state without the key: the average starts from the (loaded) weights, said once
    without = plain.state_dict()
    fresh.load_state_dict(without)
    fresh.load_state_dict(without)
    assert capsys.readouterr().out.count("holds no weight average") == 1
    assert all(torch.equal(fresh.state_dict()["gdn"]["ema"]["avg"][k], q.detach()) for k, q in enumerate(p))
    # a state with the key loaded into an optimizer without the option: ignored
    plain.load_state_dict(sd)
    assert sorted(plain.state_dict()["gdn"]) == PLAIN_KEYS and plain.ema_decay is None
    # a wrong shape is refused
    from gdn_amd._lib import GdnError
    sd["gdn"]["ema"]["avg"][1] = torch.zeros(5)
    with pytest.raises(GdnError):
        Adam(p, ema_decay=0.5).load_state_dict(sd)


# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_built_and_bound_at_revision_223():
    from gdn_amd import _lib as L
    hdr = (REPO / "include" / "gdn_hip.h").read_text()
    dll = ctypes.CDLL(str(L.LIB_PATH))
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(dll, name) and name in L.EXPORTS, name
    assert L.ABI_VERSION == 223 and L.lib.gdn_version() == 223
    csrc = REPO / "gdn-pytorch_amd" / "csrc"
    assert re.search(r"gdn_version\(void\)\s*\{\s*return 223;", (csrc / "pointwise.hip").read_text())
    assert "fmaf(w, p - e, e)" in (csrc / "optim.hip").read_text()


def test_argument_checks_answer_before_any_launch():
    """GDN_ERR_BAD_ARG (-1) for a NULL pointer, n = 0 and -- the exchange -- overlapping ranges; the pointers are never
    dereferenced, no GPU is needed."""
    from gdn_amd import _lib as L
    P = ctypes.c_void_p
    ema, swap = L.lib.raw("gdn_ema_update"), L.lib.raw("gdn_swap_f32")
    e, p, st, g = P(0x1000), P(0x2000), P(0x3000), P(0x4000)
    assert ema(None, p, 8, 0.999, st, None, None) == -1
    assert ema(e, None, 8, 0.999, st, None, None) == -1
    assert ema(e, p, 8, 0.999, None, g, None) == -1
    assert ema(e, p, 0, 0.999, st, g, None) == -1
    assert ema(e, p, -4, 0.999, st, None, None) == -1
    for decay in (0.0, 1.0, -0.5, float("nan")):
        assert ema(e, p, 8, decay, st, None, None) == -1
    assert swap(None, p, 8, None) == -1 and swap(e, None, 8, None) == -1
    assert swap(e, p, 0, None) == -1 and swap(e, p, -1, None) == -1
    assert swap(e, e, 8, None) == -1                                       # the same range
    assert swap(e, P(0x1000 + 4 * 7), 8, None) == -1                       # the last element of a is the first of b
    assert swap(P(0x1000 + 4 * 7), e, 8, None) == -1
    assert swap(P(0x1002), p, 8, None) == -1                               # not a float's alignment
