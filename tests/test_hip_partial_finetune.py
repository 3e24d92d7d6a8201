"""Partial fine-tuning on the GPU at the smallest model shapes (16 x 32, batch 2): optim.Adam(segmented=True) against the
per-tensor launches it replaces and against torch.optim.Adam, its launch count, the pruned backward against the unpruned one,
what stays bit for bit where it was under --freeze / --lr_mult 0, and the flags end to end through GDN_main.run with --graph
and --resume."""
import copy
import os

import numpy as np
import pytest
import torch

from libcalls import count_library_calls
from oracle import gdn_oracle as O
from test_hip_kernels import close

pytestmark = pytest.mark.gpu

H, W = 16, 32
NETS = ["AutoEncoder_DtoD", "AutoEncoder_2"]
OPT_CALLS = ("gdn_adam_step", "gdn_adam_step_dev", "gdn_adam_step_dev_guarded", "gdn_grad_sumsq", "gdn_grad_guard_finalize",
             "gdn_ema_update", "gdn_adam_step_seg", "gdn_grad_sumsq_seg", "gdn_ema_update_seg")


@pytest.fixture(scope="module")
def bases():
    """One seeded network of each kind on the CPU, never modified (every case works on a deep copy)."""
    import gdn_amd.AE_model_unet as M
    torch.manual_seed(11)
    return {"AutoEncoder_DtoD": M.AutoEncoder_DtoD(input_dim=1, height=H, width=W),
            "AutoEncoder_2": M.AutoEncoder_2(input_dim=3, height=H, width=W)}


@pytest.fixture(scope="module")
def batches(gpu):
    return [[t.to(gpu) for t in O.synthetic_batch(2, H, W, seed=70 + i)] for i in range(3)]


def _model(bases, name, gpu, dtype, freeze=("encoder",)):
    m = copy.deepcopy(bases[name]).to(gpu).compute_dtype(dtype).train()
    if freeze:
        m.freeze(list(freeze))
    return m


def _groups(model, encoder_mult=None):
    """Two groups (three with encoder_mult): gamma / beta without decay at half the rate, everything else."""
    enc = set(model.select_parameters("encoder")) if encoder_mult is not None else set()
    named = list(model.named_parameters())
    groups = [{"params": [p for n, p in named if p.dim() != 1 and n not in enc]},
              {"params": [p for n, p in named if p.dim() == 1 and n not in enc], "lr_mult": 0.5, "weight_decay": 0.0}]
    if enc:
        groups.append({"params": [p for n, p in named if n in enc], "lr_mult": encoder_mult})
    return groups


def _adam(model, **kw):
    from gdn_amd.optim import Adam
    return Adam(_groups(model, kw.pop("encoder_mult", None)), 2e-4, [0.9, 0.999], eps=1e-08, weight_decay=5e-4, **kw)


def _fwd_bwd(model, batch):
    from gdn_amd import utils as U
    depth, rgb, sparse = batch
    x = depth if type(model).__name__ == "AutoEncoder_DtoD" else rgb
    out = model(x, istrain=False)
    loss, _, _ = U.dtod_loss(out, depth, sparse)
    for p in model.parameters():
        p.grad = None
    loss.backward()
    return loss.detach()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu()


def _same_state(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


def _same_optimizer_state(a, b, what):
    sa, sb = a.state_dict(), b.state_dict()
    assert sorted(sa["state"]) == sorted(sb["state"]), what
    for k in sa["state"]:
        for f in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(_bits(sa["state"][k][f]), _bits(sb["state"][k][f])), (what, k, f)


# ---- segmented against the per-tensor launches ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", NETS)
def test_segmented_is_bitwise_the_per_tensor_fallback(gpu, bases, batches, name, dtype):
    """Three steps with a frozen encoder and two groups, no guard: weights, BatchNorm buffers, moments and counts bit for bit."""
    ma, mb = _model(bases, name, gpu, dtype), _model(bases, name, gpu, dtype)
    oa, ob = _adam(ma, segmented=True), _adam(mb, segmented=False)
    init = {k: v.clone() for k, v in ma.state_dict().items()}
    for batch in batches:
        la, lb = _fwd_bwd(ma, batch), _fwd_bwd(mb, batch)
        assert torch.equal(la, lb)
        oa.step()
        ob.step()
    _same_state(ma.state_dict(), mb.state_dict(), "%s %s" % (name, dtype))
    _same_optimizer_state(oa, ob, "%s %s" % (name, dtype))
    frozen, sd = set(ma.select_parameters("encoder")), ma.state_dict()
    assert all(torch.equal(_bits(sd[k]), _bits(init[k])) for k in frozen)
    # (every trainable weight with a decay moves; a gamma or beta behind a dead ReLU need not)
    assert all(not torch.equal(sd[n], init[n]) for n, p in ma.named_parameters() if n not in frozen and p.dim() != 1)
    assert all(i not in oa.state_dict()["state"] for i, p in enumerate(q for g in oa.param_groups for q in g["params"])
               if not p.requires_grad)


@pytest.mark.parametrize("name", NETS)
def test_segmented_guard_matches_the_fallback_and_float64(gpu, bases, batches, name):
    """With max_grad_norm the two sum the squares in different orders: each norm within (n 2^-53 + 2^-24) of the float64 norm
    of the trainable gradients, the weights within test_matches_torch_clip_grad_norm_and_adam's bars of each other."""
    ma, mb = _model(bases, name, gpu, "fp32"), _model(bases, name, gpu, "fp32")
    oa, ob = _adam(ma, segmented=True, max_grad_norm=0.05), _adam(mb, segmented=False, max_grad_norm=0.05)
    for batch in batches:
        _fwd_bwd(ma, batch)
        _fwd_bwd(mb, batch)
        live = [p for p in ma.parameters() if p.requires_grad]
        assert all(p.grad is not None for p in live) and all(p.grad is None for p in ma.parameters() if not p.requires_grad)
        n = sum(p.numel() for p in live)
        ref = float(np.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in live)))
        oa.step()
        ob.step()
        ga, gb = oa.guard_stats(), ob.guard_stats()
        print("%s: norm seg %.9e fallback %.9e float64 %.9e" % (name, ga["norm"], gb["norm"], ref))
        assert abs(ga["norm"] - ref) <= (n * 2.0 ** -53 + 2.0 ** -24) * ref
        assert ga["clipped"] == gb["clipped"] and ga["skipped"] == 0
    assert oa.guard_stats()["clipped"] >= 1
    for (k, a), b in zip(ma.named_parameters(), mb.parameters()):
        close(a, b, rtol=1e-5, atol_scale=1e-6, what="guarded segmented vs fallback, %s" % k)


@pytest.mark.parametrize("name", NETS)
def test_segmented_matches_torch_adam(gpu, bases, batches, name):
    """torch.optim.Adam on the CPU over the same groups at lr * lr_mult, fed the gradients of the HIP model."""
    m = _model(bases, name, gpu, "fp32")
    opt = _adam(m, segmented=True)
    theirs = {n: torch.nn.Parameter(p.detach().cpu().clone(), requires_grad=p.requires_grad) for n, p in m.named_parameters()}
    by_id = {id(p): n for n, p in m.named_parameters()}
    ref = torch.optim.Adam([{"params": [theirs[by_id[id(p)]] for p in g["params"]], "lr": 2e-4 * g.get("lr_mult", 1.0),
                             "weight_decay": g["weight_decay"]} for g in opt.param_groups], betas=(0.9, 0.999), eps=1e-8)
    for batch in batches:
        _fwd_bwd(m, batch)
        for n, p in m.named_parameters():
            theirs[n].grad = None if p.grad is None else p.grad.detach().cpu().clone()
        opt.step()
        ref.step()
    for n, p in m.named_parameters():
        close(p, theirs[n], rtol=1e-5, atol_scale=1e-6, what="segmented Adam vs torch, %s" % n)


def test_launch_count_is_constant(gpu, bases, batches):
    """Guarded, averaged, frozen encoder, two groups: four optimizer entry points (six launches), against several hundred."""
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.99)
    want = {"gdn_grad_sumsq_seg": 1, "gdn_grad_guard_finalize": 1, "gdn_adam_step_seg": 1, "gdn_ema_update_seg": 1}
    for segmented in (True, False):
        m = _model(bases, "AutoEncoder_DtoD", gpu, "fp32")
        opt = _adam(m, segmented=segmented, **kw)
        for k, batch in enumerate(batches[:2]):
            _fwd_bwd(m, batch)
            every, _ = count_library_calls(opt.step)
            calls = {name: v for name, v in every.items() if name in OPT_CALLS}
            print("segmented=%s step %d: %d optimizer calls of %d library calls" % (segmented, k, sum(calls.values()), sum(every.values())))
            if segmented:
                assert calls == want
                assert k == 0 or dict(every) == want          # (the first step also zeroes the moments it creates)
            else:
                assert sum(calls.values()) > 100 and not any(name.endswith("_seg") for name in calls)


# ---- the pruned backward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", NETS)
def test_pruned_backward_is_bitwise_and_shorter(gpu, bases, batches, name, dtype, monkeypatch):
    from gdn_amd import engine as E
    got = {}
    for prune in (True, False):
        monkeypatch.setattr(E, "_PRUNE_FROZEN", prune)
        m = _model(bases, name, gpu, dtype)
        depth, rgb, sparse = batches[0]
        from gdn_amd import utils as U
        out = m(depth if name == "AutoEncoder_DtoD" else rgb, istrain=False)
        loss, _, _ = U.dtod_loss(out, depth, sparse)
        calls, order = count_library_calls(loss.backward)
        got[prune] = (loss.detach(), {n: None if p.grad is None else p.grad.clone() for n, p in m.named_parameters()}, order)
        frozen = set(m.select_parameters("encoder"))
    (la, ga, oa), (lb, gb, ob) = got[True], got[False]
    assert torch.equal(_bits(la), _bits(lb))
    for n in ga:
        if n in frozen:
            assert ga[n] is None and gb[n] is None, n
        else:
            assert torch.equal(_bits(ga[n]), _bits(gb[n])), n
    print("%s %s: %d library calls in the pruned backward, %d in the unpruned one" % (name, dtype, len(oa), len(ob)))
    assert len(oa) < len(ob)
    # nothing frozen: every activation is live, the same calls in the same order
    orders = []
    for prune in (True, False):
        monkeypatch.setattr(E, "_PRUNE_FROZEN", prune)
        m = _model(bases, name, gpu, dtype, freeze=())
        out = m(depth if name == "AutoEncoder_DtoD" else rgb, istrain=False)
        loss, _, _ = U.dtod_loss(out, depth, sparse)
        orders.append(count_library_calls(loss.backward)[1])
    assert orders[0] == orders[1] and len(orders[0]) > len(ob)


def test_lr_mult_zero_keeps_the_weights_while_the_moments_advance(gpu, bases, batches):
    m = _model(bases, "AutoEncoder_DtoD", gpu, "fp32", freeze=())
    opt = _adam(m, segmented=True, encoder_mult=0.0)
    init = {n: p.detach().clone() for n, p in m.named_parameters()}
    for batch in batches:
        _fwd_bwd(m, batch)
        opt.step()
    enc = set(m.select_parameters("encoder"))
    sd = opt.state_dict()["state"]
    index = {id(p): i for i, p in enumerate(q for g in opt.param_groups for q in g["params"])}
    for n, p in m.named_parameters():
        assert torch.equal(_bits(p), _bits(init[n])) == (n in enc), n
        if n in enc:
            s = sd[index[id(p)]]
            assert float(s["step"]) == 3.0 and bool(s["exp_avg"].abs().sum() > 0) and bool(s["exp_avg_sq"].sum() > 0), n


# ---- the flags, end to end -----------------------------------------------------------------------------------------------
_RUNS = {}
FLAGS = ["--freeze", "encoder", "--lr_mult", "res*_up*=0.5", "--no_decay_norm", "--clip_grad_norm", "1", "--ema_decay", "0.99"]


@pytest.fixture(scope="module")
def loop_root(tmp_path_factory, bases):
    root = tmp_path_factory.mktemp("partial_finetune")
    torch.save({"module." + k: v.contiguous() for k, v in bases["AutoEncoder_DtoD"].state_dict().items()}, str(root / "init.pkl"))
    return root


def _run(root, tag, dtype, extra, epochs=2, init=True):
    """GDN_main.run in `root`/<dtype>_<tag> (cached): {file name: tensors of every .pkl written}."""
    from gdn_amd import GDN_main, option
    key = (dtype, tag)
    if key in _RUNS:
        return _RUNS[key]
    where = root / ("%s_%s" % (dtype, tag))
    where.mkdir(parents=True, exist_ok=True)
    argv = ["synthetic", "--synthetic", "--mode", "DtoD", "--height", str(H), "--width", str(W), "--batch_size", "2",
            "--epoch_size", "3", "--epochs", str(epochs), "--gpu_num", "0", "--dtype", dtype, "-e"]
    if init:
        argv += ["--init_from", str(root / "init.pkl")]
    cwd = os.getcwd()
    os.chdir(where)
    try:
        GDN_main.run(option.parse_args(argv + list(extra)))
    finally:
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


def _is_buffer(k):
    return "running_mean" in k or "running_var" in k or "num_batches_tracked" in k


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loop_frozen_encoder_stays_the_init_file(gpu, loop_root, bases, dtype):
    """Six steps under --freeze encoder (with the guard, the average, a second rate and no decay on gamma / beta): every
    encoder weight of every .pkl and _ema.pkl is the --init_from file's, every decoder weight moved; with --freeze_bn the
    encoder's running statistics are the file's too."""
    init = torch.load(loop_root / "init.pkl", map_location="cpu")
    enc = {"module." + n for n in bases["AutoEncoder_DtoD"].select_parameters("encoder")}
    for tag, extra in (("base", FLAGS), ("bn", FLAGS + ["--freeze_bn"])):
        files = _run(loop_root, tag, dtype, extra)
        assert len(files) == 4 and sum(n.endswith("_ema.pkl") for n in files) == 2
        for name, sd in files.items():
            assert list(sd) == list(init)
            for k in sd:
                if k in enc:
                    assert torch.equal(sd[k], init[k]), (tag, name, k)
                elif not _is_buffer(k) and sd[k].dim() != 1 and not name.endswith("_ema.pkl"):
                    assert not torch.equal(sd[k], init[k]), (tag, name, k, "did not train")
                if tag == "bn" and _is_buffer(k):
                    assert torch.equal(sd[k], init[k]), (tag, name, k)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loop_graph_is_bitwise(gpu, loop_root, dtype):
    _same_files(_run(loop_root, "base", dtype, FLAGS), _run(loop_root, "graph", dtype, FLAGS + ["--graph", "--graph_warmup", "2"]),
                "--graph")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loop_resume_is_bitwise(gpu, loop_root, dtype):
    base = _run(loop_root, "base", dtype, FLAGS)
    stopped = _run(loop_root, "stopped", dtype, FLAGS + ["--save_state"], epochs=1)
    (state,) = sorted((loop_root / ("%s_stopped" % dtype)).rglob("train_state.pt"))
    resumed = _run(loop_root, "resumed", dtype, FLAGS + ["--resume", str(state)], init=False)
    assert len(stopped) == 2 and len(resumed) == 2
    _same_files({k: v for k, v in base.items() if k in stopped}, stopped, "epoch 1")
    _same_files({k: v for k, v in base.items() if k not in stopped}, resumed, "--resume")
