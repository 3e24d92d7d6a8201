"""optim.Adam(segmented=True), --freeze / --lr_mult / --no_decay_norm without a GPU: the chunk map, the library calls of a
step (the recorder technique and the 384-float arena of test_optim_launch_order_cpu.py), the handover to per-tensor launches,
the learning-rate multipliers under the trainer's decay, the parsers, the encoder / decoder name sets, the param groups and the
state_dict() exchange with torch.optim.Adam."""
import copy
import struct

import pytest
import torch

ITEMS = [(0, 54), (64, 3), (128, 3), (192, 3), (256, 54), (320, 2)]
COVERED = [ITEMS[k] for k in (0, 1, 3, 4, 5)]         # parameters()[2] frozen, or without a gradient
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
GUARD_EMA = dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.99)
SKIP = 0xFF


@pytest.fixture
def calls(monkeypatch):
    """Recorders in place of the launches; the segmented ones also note the chunk map and the number of groups."""
    from gdn_amd import ops
    log = _Log()
    rng = lambda t: (t.numel(), t.storage_offset())      # noqa: E731
    monkeypatch.setattr(ops, "zeros", lambda shape, device: torch.zeros(shape, dtype=torch.float32, device=device))
    monkeypatch.setattr(ops, "adam_step_dev", lambda p, g, m, v, hyper, state: log.append(
        ("adam_step_dev",) + rng(p) + tuple(rng(t) for t in (g, m, v) if rng(t) != rng(p))))
    monkeypatch.setattr(ops, "adam_step_dev_guarded", lambda p, g, m, v, hyper, state, guard: log.append(
        ("adam_step_dev_guarded",) + rng(p) + tuple(rng(t) for t in (g, m, v) if rng(t) != rng(p))))
    monkeypatch.setattr(ops, "grad_sumsq", lambda g, guard, accumulate=False: log.append(("grad_sumsq", g.numel(), accumulate)))
    monkeypatch.setattr(ops, "grad_guard_finalize", lambda *a: log.append(("grad_guard_finalize",)))
    monkeypatch.setattr(ops, "ema_update", lambda ema, p, decay, state, guard=None: log.append(
        ("ema_update", p.numel(), ema.storage_offset())))
    monkeypatch.setattr(ops, "swap_", lambda a, b: log.append(("swap_", a.numel(), a.storage_offset())))

    def adam_step_seg(p, g, m, v, cmap, hyper, states, guard=None):
        log.append(("adam_step_seg", p.numel(), cmap.tolist(), tuple(hyper.shape), states.numel(), guard is not None)
                   + tuple(rng(t) for t in (g, m, v) if rng(t) != rng(p)))
        if log.advance:                       # what the prep launch does to every group's step count
            states.view(torch.int32)[4::8] += 1
    monkeypatch.setattr(ops, "adam_step_seg", adam_step_seg)
    monkeypatch.setattr(ops, "grad_sumsq_seg", lambda g, cmap, guard, accumulate=False: log.append(
        ("grad_sumsq_seg", g.numel(), cmap.tolist(), accumulate)))
    monkeypatch.setattr(ops, "ema_update_seg", lambda ema, p, cmap, decay, states, guard=None: log.append(
        ("ema_update_seg", p.numel(), cmap.tolist(), states.numel(), guard is not None)))
    return log


class _Log(list):
    advance = True          # the adam_step_seg recorder counts the step in the group states, as the kernel does


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


def _two_groups(net, freeze=True):
    """conv weights and biases | BatchNorm gamma, beta (half the rate, no decay); parameters()[2] (gamma) frozen."""
    ps = list(net.parameters())
    if freeze:
        ps[2].requires_grad_(False)
        ps[2].grad = None
    return [{"params": [ps[0], ps[1], ps[4], ps[5]]}, {"params": [ps[2], ps[3]], "lr_mult": 0.5, "weight_decay": 0.0}]


MAP = [0, 0, SKIP, 1, 0, 0]          # chunk -> group: gamma's chunk is skipped, beta's belongs to the second group


def test_chunk_map_and_unguarded_sequence(calls):
    from gdn_amd.optim import Adam
    net, ar = _arena_and_net()
    opt = Adam(_two_groups(net), **HYPER, segmented=True)
    assert opt.capturable is True and opt.segmented is True
    opt.step()
    opt.step()
    assert calls == [("adam_step_seg", 384, MAP, (2, 6), 64, False)] * 2
    st = opt.store_of(ar)
    assert st.plan.key == (0, 0, -1, 1, 0, 0) and st.plan.groups == [0, 1] and st.plan.map.tolist() == MAP
    # the table: lr * lr_mult rounded once, each group's own decay, one gradient scale
    rows = st.plan.hyper.tolist()
    f32 = lambda x: struct.unpack("<f", struct.pack("<f", x))[0]      # noqa: E731
    assert rows[0] == [f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(5e-4), 1.0]
    assert rows[1] == [f32(1e-3 * 0.5), f32(0.9), f32(0.999), f32(1e-8), 0.0, 1.0]
    assert [st.count(p) for p in net.parameters()] == [2, 2, 0, 2, 2, 2]      # the device's counts; the frozen one's is the host's
    assert [st.pstep[id(p)] for p in net.parameters()] == [2, 2, 0, 2, 2, 2]


def test_guarded_averaged_sequence_is_constant(calls):
    from gdn_amd.optim import Adam
    net, ar = _arena_and_net()
    opt = Adam(_two_groups(net), **HYPER, segmented=True, **GUARD_EMA)
    opt.step()
    assert calls == [("grad_sumsq_seg", 384, MAP, False), ("grad_guard_finalize",),
                     ("adam_step_seg", 384, MAP, (2, 6), 64, True), ("ema_update_seg", 384, MAP, 64, True)]
    # the same frozen parameter in ONE group without the option: the per-tensor launches this replaces
    del calls[:]
    net2, _ = _arena_and_net()
    ps = list(net2.parameters())
    ps[2].requires_grad_(False)
    ps[2].grad = None
    Adam(ps, **HYPER, **GUARD_EMA).step()
    assert len(calls) == 1 + 3 * 5 and {c[0] for c in calls} == {"grad_sumsq", "grad_guard_finalize", "adam_step_dev_guarded", "ema_update"}


def test_nothing_frozen_one_group_runs_segmented_too(calls):
    from gdn_amd.optim import Adam
    net, ar = _arena_and_net()
    Adam(net.parameters(), **HYPER, segmented=True).step()
    assert calls == [("adam_step_seg", 384, [0] * 6, (1, 6), 32, False)]


@pytest.mark.parametrize("kw, name", [({}, "adam_step_dev"), (GUARD_EMA, "adam_step_dev_guarded")], ids=["plain", "guard_ema"])
def test_a_missing_gradient_hands_over_to_the_per_tensor_sequence(calls, kw, name):
    """Exactly what test_optim_launch_order_cpu.py pins for partial coverage of a capturable optimizer."""
    from gdn_amd.optim import Adam
    net, ar = _arena_and_net()
    opt = Adam(_two_groups(net, freeze=False), **HYPER, segmented=True, **kw)
    opt.step()
    assert calls[-2 if kw else -1][0] == "adam_step_seg"
    del calls[:]
    list(net.parameters())[2].grad = None
    opt.step()
    if not kw:
        assert calls == [("adam_step_dev", n, o) for o, n in COVERED]
    else:
        want = [("grad_sumsq", n, k > 0) for k, (o, n) in enumerate(COVERED)] + [("grad_guard_finalize",)]
        for o, n in COVERED:
            want += [("adam_step_dev_guarded", n, o), ("ema_update", n, o)]
        assert calls == want
    (rec,) = opt.state_dict()["gdn"]["stores"]
    assert rec["pstep"] == [2, 2, 1, 2, 2, 2] and sorted(rec["pdev"]) == [0, 1, 2, 3, 5]      # (indices in group order)
    assert all(t.dtype == torch.uint8 and t.numel() == 28 for t in rec["pdev"].values())
    # ... and stays there, as the one-launch path does
    del calls[:]
    ar.bind_grads()
    opt.step()
    assert len(calls) == (6 if not kw else 6 + 1 + 12) and not any("seg" in c[0] for c in calls)


def test_plan_follows_requires_grad(calls):
    from gdn_amd.optim import Adam
    net, ar = _arena_and_net()
    opt = Adam(_two_groups(net), **HYPER, segmented=True)
    opt.step()
    ps = list(net.parameters())
    ps[3].requires_grad_(False)
    ps[3].grad = None
    opt.step()
    assert calls[-1] == ("adam_step_seg", 384, [0, 0, SKIP, SKIP, 0, 0], (1, 6), 32, False)


def test_lr_mult_survives_the_trainers_decay(calls):
    from gdn_amd import trainer
    from gdn_amd.optim import Adam
    net, ar = _arena_and_net()
    opt = Adam(_two_groups(net), **HYPER, segmented=True)
    opt.step()
    lr = trainer._decay_lr(opt, 1e-3, 10.0)
    assert [g["lr"] for g in opt.param_groups] == [lr, lr] and [g.get("lr_mult", 1.0) for g in opt.param_groups] == [1.0, 0.5]
    opt.refresh_hyper()
    rows = opt.store_of(ar).plan.hyper.tolist()
    assert rows[0][0] == torch.tensor(lr, dtype=torch.float32).item()
    assert rows[1][0] == torch.tensor(lr * 0.5, dtype=torch.float32).item()
    with pytest.raises(ValueError, match="lr_mult"):
        Adam([{"params": list(net.parameters()), "lr_mult": -1.0}], **HYPER)


def test_every_arena_parameter_must_be_in_a_group(calls):
    from gdn_amd._lib import GdnError
    from gdn_amd.optim import Adam
    net, ar = _arena_and_net()
    opt = Adam(list(net.parameters())[:4], **HYPER, segmented=True)
    with pytest.raises(GdnError, match="in no param group"):
        opt.step()


# ---- state exchange --------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_with_torch(calls):
    from gdn_amd.optim import Adam
    net, ar = _arena_and_net()
    opt = Adam(_two_groups(net), **HYPER, segmented=True)
    for _ in range(3):
        opt.step()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3, 5]          # no entry for the frozen gamma (index 4 of the groups' order)
    assert [g.get("lr_mult") for g in sd["param_groups"]] == [None, 0.5]
    (rec,) = sd["gdn"]["stores"]
    assert rec["seg"]["key"] == [0, 0, -1, 1, 0, 0] and rec["seg"]["states"].numel() == 64 and rec["state"] is None
    # torch's optimizer over the same groups takes it and hands it back
    ref = torch.optim.Adam(_two_groups(net), **HYPER)
    ref.load_state_dict({"state": copy.deepcopy(sd["state"]), "param_groups": copy.deepcopy(sd["param_groups"])})
    back = ref.state_dict()
    assert sorted(back["state"]) == [0, 1, 2, 3, 5]
    net2, ar2 = _arena_and_net()
    opt2 = Adam(_two_groups(net2), **HYPER, segmented=True)
    opt2.load_state_dict(back)
    again = opt2.state_dict()
    assert sorted(again["state"]) == [0, 1, 2, 3, 5]
    for k in again["state"]:
        assert float(again["state"][k]["step"]) == float(sd["state"][k]["step"])
        assert torch.equal(again["state"][k]["exp_avg"], sd["state"][k]["exp_avg"])
    del calls[:]
    opt2.step()                                              # level counts: the segmented launch goes on
    assert calls == [("adam_step_seg", 384, MAP, (2, 6), 64, False)]
    # our own record brings the device states back verbatim
    net3, ar3 = _arena_and_net()
    opt3 = Adam(_two_groups(net3), **HYPER, segmented=True)
    opt3.load_state_dict(sd)
    calls.advance = False
    opt3.step()
    assert torch.equal(opt3.store_of(ar3).plan.states.cpu(), rec["seg"]["states"])


def test_flag_off_state_dict_is_unchanged(calls):
    """Key by key what an optimizer that knows nothing of the option writes: no 'seg', no 'lr_mult', the same records."""
    from gdn_amd.optim import Adam
    net, ar = _arena_and_net()
    opt = Adam(net.parameters(), **HYPER, capturable=True)
    opt.step()
    sd = opt.state_dict()
    assert sorted(sd) == ["gdn", "param_groups", "state"] and sorted(sd["gdn"]) == ["capturable", "grad_scale", "stores", "version"]
    assert sorted(sd["param_groups"][0]) == ["betas", "eps", "lr", "params", "weight_decay"]
    (rec,) = sd["gdn"]["stores"]
    assert sorted(rec) == ["full_dev", "kind", "params", "pdev", "pstep", "state", "step"]
    assert calls == [("adam_step_dev", 384, 0)] and sorted(sd["state"]) == [0, 1, 2, 3, 4, 5]


# ---- command line ----------------------------------------------------------------------------------------------------
def test_parsers():
    import argparse
    from gdn_amd import option
    a = option.parse_args(["--synthetic"])
    assert a.freeze == [] and a.lr_mult == [] and a.no_decay_norm is False
    b = option.parse_args(["--synthetic", "--freeze", "encoder, upconv4.*", "--lr_mult", "res*_up*=0.5,decoder=2,res*_up*=0",
                           "--no_decay_norm"])
    assert b.freeze == ["encoder", "upconv4.*"] and b.no_decay_norm is True
    assert b.lr_mult == [("res*_up*", 0.5), ("decoder", 2.0), ("res*_up*", 0.0)]
    for bad in ("", "encoder,,decoder"):
        with pytest.raises(argparse.ArgumentTypeError):
            option.freeze_specs(bad)
    for bad in ("encoder", "encoder=", "=2", "encoder=-1", "encoder=x", "encoder=inf", "a=1,,b=2"):
        with pytest.raises(argparse.ArgumentTypeError):
            option.lr_mults(bad)


ENCODER_TOPS = {
    "AutoEncoder_DtoD": ["downconv0", "downconv1", "downconv2", "downconv3", "downconv4", "res64_down1", "res128_down1",
                         "res256_down1", "res512_down1", "res512_down2", "res512_1", "res512_2", "res512_3", "res512_4",
                         "res512_5", "res512_6"],
    "AutoEncoder_2": ["downconv0", "downconv1", "downconv2", "downconv3", "downconv4", "res64_down1", "res128_down1",
                      "res256_down1", "res512_down1", "res512_down2", "res512_1", "res512_2", "res512_3", "res512_4",
                      "res512_5", "res512_6"],
    "AutoEncoder": ["downconv0", "downconv1", "downconv2", "downconv3", "res64_down1", "res64_down2", "res128_down1",
                    "res128_down2", "res256_down1", "res256_down2", "res512_1", "res512_2", "res512_3", "res512_4", "res512_5",
                    "res512_6", "N64_down", "N128_down", "N256_down", "N512_down"],
}
DECODER_TOPS = {
    "AutoEncoder_DtoD": ["res64_up1", "res128_up1", "res256_up1", "res512_up1", "res512_up2", "upconv0", "upconv1", "upconv2",
                         "upconv3", "upconv4"],
    "AutoEncoder_2": ["res64_up1", "res128_up1", "res256_up1", "res512_up1", "res512_up2", "upconv0", "upconv1", "upconv2",
                      "upconv3", "upconv4", "conv1x1_64", "conv1x1_128", "conv1x1_256", "conv1x1_512"],
    "AutoEncoder": ["res64_up1", "res64_up2", "res128_up1", "res128_up2", "res256_up1", "res256_up2", "upconv0", "upconv1",
                    "upconv2", "upconv3", "conv1x1_64", "conv1x1_128", "conv1x1_256", "N64_up", "N128_up", "N256_up"],
}
COUNTS = {"AutoEncoder_DtoD": (81, 43), "AutoEncoder_2": (81, 55), "AutoEncoder": (84, 49)}      # 124, 136 and 133 tensors


@pytest.fixture(scope="module")
def meta_nets():
    import contextlib
    import io
    from gdn_amd import AE_model_unet as M
    with torch.device("meta"), contextlib.redirect_stdout(io.StringIO()):
        return {"AutoEncoder_DtoD": M.AutoEncoder_DtoD(height=16, width=32), "AutoEncoder_2": M.AutoEncoder_2(height=16, width=32),
                "AutoEncoder": M.AutoEncoder(height=16, width=32)}


@pytest.mark.parametrize("name", sorted(ENCODER_TOPS))
def test_encoder_and_decoder_name_sets(meta_nets, name):
    net = meta_nets[name]
    enc, dec = net.select_parameters("encoder"), net.select_parameters("decoder")
    tops = lambda names: sorted({n.split(".")[0] for n in names})      # noqa: E731
    assert tops(enc) == sorted(ENCODER_TOPS[name]) and tops(dec) == sorted(DECODER_TOPS[name])
    assert (len(enc), len(dec)) == COUNTS[name]
    assert sorted(enc + dec) == sorted(n for n, _ in net.named_parameters()) and not set(enc) & set(dec)
    assert net.select_parameters("res*_up*") == [n for n, _ in net.named_parameters() if n.startswith("res") and "_up" in n]


def test_freeze_from_code(meta_nets):
    from gdn_amd._lib import GdnError
    net = copy.deepcopy(meta_nets["AutoEncoder_DtoD"])
    with pytest.raises(GdnError, match="selects no parameter"):
        net.freeze(["encoder", "no_such_layer.*"])
    with pytest.raises(GdnError, match="nothing to train"):
        net.freeze(["encoder", "decoder"])
    assert all(p.requires_grad for p in net.parameters())          # a refused call froze nothing
    frozen = net.freeze("encoder")
    assert frozen == net.select_parameters("encoder")
    assert [n for n, p in net.named_parameters() if not p.requires_grad] == frozen
    assert all(m.training for m in net.modules())                  # BatchNorm layers keep their mode


def test_param_groups_in_first_appearance_order(meta_nets):
    from gdn_amd import GDN_main, option
    net = meta_nets["AutoEncoder_DtoD"]
    names = {id(p): n for n, p in net.named_parameters()}
    args = option.parse_args(["--synthetic", "--lr_mult", "res*_up*=0.5,upconv4.*=0", "--no_decay_norm"])
    groups = GDN_main.param_groups(net, args)
    keys = [(g.get("lr_mult"), g.get("weight_decay")) for g in groups]
    # downconv0's conv weight, its gamma, then the first res*_up* block (res64_up1: registered second of the blocks), the head
    assert keys == [(None, None), (None, 0.0), (0.5, None), (0.5, 0.0), (0.0, None)]
    assert sum(len(g["params"]) for g in groups) == 124 and [names[id(g["params"][0])] for g in groups] == [
        "downconv0.main.1.weight", "downconv0.main.2.weight", "res64_up1.main.0.weight", "res64_up1.main.1.weight", "upconv4.weight"]
    assert all(p.dim() == 1 for g in groups if g.get("weight_decay") == 0.0 for p in g["params"])
    only_freeze = GDN_main.param_groups(net, option.parse_args(["--synthetic", "--freeze", "encoder"]))
    assert len(only_freeze) == 1 and sorted(only_freeze[0]) == ["params"] and len(only_freeze[0]["params"]) == 124
    with pytest.raises(RuntimeError, match="selects no parameter"):
        GDN_main.param_groups(net, option.parse_args(["--synthetic", "--lr_mult", "nothing*=2"]))


def test_make_optimizer_is_segmented_only_with_the_flags():
    from gdn_amd import GDN_main, option
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4))
    net.select_parameters = lambda spec: []
    plain = GDN_main._make_optimizer(net, option.parse_args(["--synthetic"]))
    assert plain.segmented is False and plain.capturable is False and len(plain.param_groups) == 1
    seg = GDN_main._make_optimizer(net, option.parse_args(["--synthetic", "--no_decay_norm"]))
    assert seg.segmented is True and seg.capturable is True
    assert [(len(g["params"]), g["weight_decay"]) for g in seg.param_groups] == [(1, 5e-4), (3, 0.0)]          # (the conv's bias is 1-D, too)


@pytest.mark.parametrize("argv, match", [
    (["--mode", "DtoD_test", "--freeze", "encoder", "--init_from", "x.pkl"], "trains nothing"),
    (["--mode", "DtoD", "--freeze", "encoder"], "needs --init_from or --resume"),
    (["--mode", "DtoD", "--freeze", "no_such*", "--init_from", "x.pkl"], "selects no parameter"),
    (["--mode", "DtoD", "--freeze", "encoder,decoder", "--init_from", "x.pkl"], "nothing to train"),
    (["--mode", "RtoD", "--freeze", "conv1x1_*,*", "--init_from", "x.pkl"], "nothing to train"),
], ids=["test_mode", "fresh_network", "no_match", "nothing_left", "nothing_left_rtod"])
def test_refused_command_lines(argv, match):
    """Each raises in run()'s checks, before the process looks for a GPU (this one has none)."""
    from gdn_amd import GDN_main, option
    args = option.parse_args(["--synthetic", "--height", "16", "--width", "32"] + argv)
    with pytest.raises(RuntimeError, match=match):
        GDN_main.run(args)
