"""Fine-tuning on frozen BatchNorm statistics (--freeze_bn, _HipModule.freeze_bn, gdn_bn_frozen_*): what needs
no GPU -- the float64 restatement the GPU tests compare against (itself checked against torch's float64 autograd of
F.batch_norm(training=False)), the command-line flag and its two refusals, the C ABI's declarations and argument checks, and
the freeze_bn() / train() / eval() semantics of the three networks built on the CPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frozen_bn_fp64 as Z


# ---- the float64 restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C", [4, 12])
def test_fp64_restatement_matches_torch_autograd(C, relu):
    g = torch.Generator().manual_seed(11 + C)
    y = (torch.randn(3, 7, 5, C, generator=g, dtype=torch.float64) * 2 + 0.7).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g, dtype=torch.float64) * 0.5).requires_grad_(True)
    rm = torch.randn(C, generator=g, dtype=torch.float64) * 0.3 + 0.5
    rv = torch.rand(C, generator=g, dtype=torch.float64) * 3 + 0.5
    dout = torch.randn(3, 7, 5, C, generator=g, dtype=torch.float64)
    rm0, rv0 = rm.clone(), rv.clone()
    out = F.batch_norm(y.permute(0, 3, 1, 2), rm, rv, gamma, beta, training=False, eps=1e-5)
    if relu:
        out = torch.relu(out)
    out.backward(dout.permute(0, 3, 1, 2))
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    co = Z.coeffs(gamma.detach(), beta.detach(), rm, rv, 1e-5)
    b = Z.bwd(dout, y.detach(), co[0], co[1], co[2], co[3], relu)
    z = y.detach().numpy() * co[0] + co[1]
    np.testing.assert_allclose(np.maximum(z, 0) if relu else z, out.detach().permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(b["dy"], y.grad.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(b["dgamma"], gamma.grad.numpy(), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(b["dbeta"], beta.grad.numpy(), rtol=1e-11, atol=1e-12)
    assert b["n"] == 105 and (b["abs1"] >= np.abs(b["dbeta"])).all() and (b["abs2"] >= np.abs(b["dgamma"]) - 1e-12).all()


def test_fp64_mask_is_zero_at_zero():
    """Gradient 0 AT a pre-activation of exactly 0, as torch's ReLU."""
    y = np.array([[-1.0, 0.0, 1.0, 2.0]]).reshape(1, 1, 1, 4)
    one, zero = np.ones(4), np.zeros(4)
    b = Z.bwd(np.full((1, 1, 1, 4), 3.0), y, one, zero, zero, one, relu=True)
    assert b["dy"].ravel().tolist() == [0.0, 0.0, 3.0, 3.0]


# ---- command line -----------------------------------------------------------------------------------------------------
def _no_gpu_calls(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the check touched the GPU")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "is_initialized", boom)


def test_parser_flag():
    from gdn_amd import option
    assert option.parse_args(["synthetic", "--synthetic"]).freeze_bn is False
    assert option.parse_args(["synthetic", "--synthetic", "--freeze_bn"]).freeze_bn is True
    assert "--freeze_bn" in option.__doc__
    assert "running mean" in " ".join(option.build_parser().format_help().split())


@pytest.mark.parametrize("mode", ["DtoD_test", "RtoD_test"])
def test_freeze_bn_refuses_test_modes(monkeypatch, mode, tmp_path):
    from gdn_amd import GDN_main, option
    _no_gpu_calls(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ck = tmp_path / "w.pkl"
    ck.write_bytes(b"x")
    a = option.parse_args(["synthetic", "--synthetic", "--mode", mode, "--freeze_bn", "--init_from", str(ck)])
    with pytest.raises(RuntimeError, match="--freeze_bn.*trains nothing"):
        GDN_main.run(a)


def test_freeze_bn_refuses_a_fresh_network(monkeypatch, tmp_path):
    from gdn_amd import GDN_main, option
    _no_gpu_calls(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = option.parse_args(["synthetic", "--synthetic", "--mode", "DtoD", "--freeze_bn"])
    with pytest.raises(RuntimeError, match="--freeze_bn needs --init_from or --resume.*mean 0 / variance 1.*mistake"):
        GDN_main.run(a)
    # either of the two passes the check; without the flag there is nothing to check
    ck = tmp_path / "w.pkl"
    ck.write_bytes(b"x")
    for extra in (["--init_from", str(ck)], ["--resume", str(ck)]):
        GDN_main._check_freeze_bn(option.parse_args(["synthetic", "--synthetic", "--mode", "DtoD", "--freeze_bn"] + extra))
    GDN_main._check_freeze_bn(option.parse_args(["synthetic", "--synthetic", "--mode", "DtoD_test"]))


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_entry_points_and_checks_arguments():
    from gdn_amd import _lib as L
    dll = L.lib._load()
    for name in ("gdn_bn_frozen_coeffs", "gdn_bn_frozen_bwd_workspace_bytes", "gdn_bn_frozen_bwd"):
        assert hasattr(dll, name) and name in L.EXPORTS, name
    assert L.ABI_VERSION == L.lib.gdn_version()
    P = ctypes.c_void_p
    p = P(0x1000)
    co = L.lib.raw("gdn_bn_frozen_coeffs")
    assert co(p, p, None, p, 1e-5, 4, p, p, p, p, None) == -1           # no running mean
    assert co(p, p, p, p, 1e-5, 4, p, p, None, p, None) == -1           # no mean row
    assert co(p, p, p, p, 1e-5, 0, p, p, p, p, None) == -1
    wsb = L.lib.raw("gdn_bn_frozen_bwd_workspace_bytes")
    # the grid is a function of the pixel count alone: ceil(npix / 64) blocks, 2048 at the most; [blocks][2][C] + [2][C] floats
    assert wsb(105, 12) == (2 * 2 * 12 + 2 * 12) * 4 and wsb(1, 4) == (2 * 4 + 2 * 4) * 4
    assert wsb(64 * 2048, 64) == wsb(10 ** 7, 64) == (2048 * 2 * 64 + 2 * 64) * 4
    bwd = L.lib.raw("gdn_bn_frozen_bwd")
    nb = wsb(105, 12)
    args = lambda **k: [k.get("dout", p), 12, k.get("y", p), 12, p, p, k.get("mean", p), p, k.get("dy", p), k.get("ld_dy", 12),
                        k.get("dg", p), k.get("db", p), k.get("npix", 105), k.get("C", 12), 1, k.get("ext", None),
                        k.get("slots", 0), k.get("ws", p), k.get("nb", nb), 0, None]
    assert bwd(*args(mean=None)) == -1
    assert bwd(*args(npix=0)) == -1
    assert bwd(*args(dout=None)) == -1                                   # dy wanted, nothing to read
    assert bwd(*args(ext=p, slots=0)) == -1
    assert bwd(*args(C=6)) == -2 and bwd(*args(ld_dy=10)) == -2          # C % 4, pitch % 4
    assert bwd(*args(nb=nb - 1)) == -3 and bwd(*args(ws=None)) == -3     # workspace too small / missing
    with pytest.raises(L.GdnError, match="gdn_bn_frozen_bwd failed"):
        L.lib.gdn_bn_frozen_bwd(*args(nb=nb - 1))


# ---- freeze_bn() on the networks ---------------------------------------------------------------------------------------
def _norms(m):
    return [n for n in m.modules() if isinstance(n, (torch.nn.BatchNorm2d, torch.nn.InstanceNorm2d))]


@pytest.mark.parametrize("name", ["AutoEncoder_DtoD", "AutoEncoder_2", "AutoEncoder"])
def test_freeze_bn_semantics(name):
    import gdn_amd.AE_model_unet as M
    torch.manual_seed(0)
    m = getattr(M, name)(height=32, width=64)
    norms = _norms(m)
    others = [x for x in m.modules() if x not in norms]
    assert len(norms) > 3 and m.training and all(n.training for n in norms)
    keys = list(m.state_dict().keys())
    vals = {k: v.clone() for k, v in m.state_dict().items()}

    assert m.freeze_bn() is m                                           # returns self, like compute_dtype
    assert m.training and not any(n.training for n in norms) and all(x.training for x in others)
    assert m.train() is m
    assert m.training and not any(n.training for n in norms) and all(x.training for x in others)
    m.eval()
    assert not any(x.training for x in m.modules())
    m.train()                                                           # the validation round trip leaves them frozen
    assert m.training and not any(n.training for n in norms) and all(x.training for x in others)
    m.train(False)
    assert not any(x.training for x in m.modules())
    m.train(True)
    assert list(m.state_dict().keys()) == keys                          # key order and contents unchanged
    assert all(torch.equal(v, vals[k]) for k, v in m.state_dict().items())

    assert m.freeze_bn(False) is m
    assert all(x.training for x in m.modules())
    m.eval()
    assert not any(x.training for x in m.modules())
    m.train()
    assert all(x.training for x in m.modules())
    # frozen while the module is in eval(): nothing changes until train()
    m.eval().freeze_bn()
    assert not any(x.training for x in m.modules())
    m.train()
    assert not any(n.training for n in norms) and all(x.training for x in others)
    assert list(m.state_dict().keys()) == keys


def test_freeze_bn_on_a_block_and_on_a_sub_module():
    import gdn_amd.AE_model_unet as M
    blk = M.ResidualBlock(64, 64, 3, 1).freeze_bn()
    assert blk.training and [n.training for n in _norms(blk)] == [False, False]
    m = M.AutoEncoder_DtoD(height=32, width=64)
    sub = next(x for x in m.modules() if isinstance(x, M.ResidualBlock))
    sub.freeze_bn()
    m.train()                                                           # the parent's train() respects the sub-module's flag
    frozen = set(map(id, _norms(sub)))
    assert all(n.training == (id(n) not in frozen) for n in _norms(m))


def test_engine_frozen_stats_layer_rule():
    """A frozen-statistics trained layer: the tape records, the called module is in train(), the norm layer is in eval() and
    something of the layer trains.  A module in eval() as a whole is inference and keeps today's path."""
    from gdn_amd import engine as E
    conv, bn = torch.nn.Conv2d(64, 64, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(64)
    rec, norec, ev = E.Ctx(record=True), E.Ctx(record=False), E.Ctx(record=True, module_training=False)
    assert not E._frozen_stats(rec, conv, bn)                            # train-mode BatchNorm
    bn.eval()
    assert E._frozen_stats(rec, conv, bn) and not E._frozen_stats(norec, conv, bn) and not E._frozen_stats(ev, conv, bn)
    conv.requires_grad_(False)
    assert E._frozen_stats(rec, conv, bn)                                # gamma / beta still train
    bn.requires_grad_(False)
    assert not E._frozen_stats(rec, conv, bn)                            # nothing to train: the guide's path
