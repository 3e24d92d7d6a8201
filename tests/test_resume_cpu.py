"""Exact resume, the parts that need no GPU: loader position / RNG state, the optimizer's state exchange through the arena's
physical layout, the atomic state file, the command-line flags and the two-rank gather of the loader states (gloo)."""
import io
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from gdn_amd._lib import GdnError


class RecordingSet:
    """n raw KITTI-shaped samples whose pixels carry their index; every __getitem__ is logged."""

    def __init__(self, n, H=4, W=6):
        self.n, self.H, self.W, self.calls = n, H, W, []

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        self.calls.append(int(i))
        return (np.full((self.H, self.W, 1), i, np.uint8), np.full((self.H, self.W, 3), i, np.uint8),
                np.full((self.H, self.W, 1), i, np.uint8))


@pytest.fixture
def stub_augment(monkeypatch):
    from gdn_amd import datasets
    monkeypatch.setattr(datasets.ops, "kitti_augment", lambda x, params, train: x)


def _batches(loader, epochs, first_epoch_stop=None):
    """[(sample indices, draws)] of `epochs` epochs; the first one is left (break) after first_epoch_stop batches."""
    out = []
    for e in range(epochs):
        for b, (gt, _, _) in enumerate(loader):
            out.append(([int(v) for v in gt[:, 0, 0, 0]], list(loader.last_params)))
            if e == 0 and first_epoch_stop is not None and b == first_epoch_stop - 1:
                break
    return out


def _kitti_loader(ds, **kw):
    from gdn_amd.datasets import GpuAugmentLoader
    return GpuAugmentLoader(ds, 2, "cpu", train=True, seed=11 + kw.get("rank", 0), order_seed=5, drop_last=True, **kw)


@pytest.mark.parametrize("shard", [{}, {"rank": 1, "world": 2}], ids=["shuffled", "world2_rank1"])
def test_loader_resumes_mid_epoch(stub_augment, shard):
    """1.5 epochs, save, load into a fresh loader: the rest of that epoch and two more equal the uninterrupted loader's, index
    batches and augmentation draws alike, and no skipped sample is fetched."""
    n = 12
    straight_ds = RecordingSet(n)
    straight = _kitti_loader(straight_ds, **shard)
    per_epoch = len(straight)
    half = per_epoch // 2 + 1 if per_epoch < 4 else per_epoch // 2
    want = _batches(straight, 4)
    assert len(want) == 4 * per_epoch and want[0][0] != want[per_epoch][0]          # (epochs are shuffled differently)

    first = _kitti_loader(RecordingSet(n), **shard)
    got = _batches(first, 1)
    it = iter(first)
    for _ in range(half):
        gt = next(it)[0]
        got.append(([int(v) for v in gt[:, 0, 0, 0]], list(first.last_params)))
    state = first.state_dict()
    buf = io.BytesIO()
    torch.save(state, buf)
    buf.seek(0)
    state = torch.load(buf, weights_only=True)           # what a state file gives back
    assert got == want[:per_epoch + half]

    ds2 = RecordingSet(n)
    second = _kitti_loader(ds2, **shard)
    second.load_state_dict(state)
    assert second.state_dict() == first.state_dict()     # nothing moves before the next __iter__
    rest = _batches(second, 3)
    assert rest == want[per_epoch + half:]
    assert ds2.calls == [i for idxs, _ in want[per_epoch + half:] for i in idxs]      # the skipped samples were never decoded


def test_loader_state_at_an_epoch_boundary(stub_augment):
    """The training loops leave an epoch with `break`: state_dict(epoch_done=True) makes the restored loader start the NEXT
    epoch's shuffle, not the rest of the one that was left."""
    straight = _kitti_loader(RecordingSet(12))
    want = _batches(straight, 3, first_epoch_stop=4)
    first = _kitti_loader(RecordingSet(12))
    assert _batches(first, 1, first_epoch_stop=4) == want[:4]
    second = _kitti_loader(RecordingSet(12))
    second.load_state_dict(first.state_dict(epoch_done=True))
    assert _batches(second, 2) == want[4:]


def test_synthetic_loader_resumes_mid_epoch():
    from gdn_amd.synthetic import SyntheticLoader
    mk = lambda: SyntheticLoader(1, 4, H=2, W=3, seed=3, distinct=3)
    straight = mk()
    want = [b[0] for _ in range(4) for b in straight]
    first = mk()
    got = [b[0] for b in first]
    it = iter(first)
    got += [next(it)[0], next(it)[0]]
    second = mk()
    second.load_state_dict(first.state_dict())
    rest = [b[0] for _ in range(3) for b in second]
    assert len(rest) == 10 and all(torch.equal(a, b) for a, b in zip(got + rest, want))
    with pytest.raises(GdnError, match="4.*5|5.*4"):
        SyntheticLoader(1, 5, H=2, W=3).load_state_dict(first.state_dict())


def test_loader_state_mismatch_names_both_values(stub_augment):
    state = _kitti_loader(RecordingSet(12)).state_dict()
    with pytest.raises(GdnError, match=r"world size 1, this loader has 2"):
        _kitti_loader(RecordingSet(12), rank=0, world=2).load_state_dict(state)
    with pytest.raises(GdnError, match=r"dataset length 12, this loader has 10"):
        _kitti_loader(RecordingSet(10)).load_state_dict(state)
    from gdn_amd.datasets import GpuAugmentLoader
    with pytest.raises(GdnError, match=r"batch size 2, this loader has 3"):
        GpuAugmentLoader(RecordingSet(12), 3, "cpu", seed=1).load_state_dict(state)


# ---------------------------------------------------------------------------------------------------------------------
def _small_net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3), torch.nn.BatchNorm2d(3), torch.nn.ConvTranspose2d(3, 2, 3))


def _torch_state(net, steps=2):
    """A torch.optim.Adam state over `net`'s parameters after `steps` updates with seeded gradients."""
    opt = torch.optim.Adam(net.parameters(), 1e-3, (0.9, 0.999), eps=1e-8, weight_decay=5e-4)
    g = torch.Generator().manual_seed(9)
    for _ in range(steps):
        for p in net.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt.state_dict()


def test_optimizer_state_goes_through_the_tap_major_layout(monkeypatch):
    """A torch state loaded into optim.Adam lands in the flat moments in the arena's PHYSICAL order (tap-major convolution
    weights: each parameter's own strides), and comes back out in logical shape, contiguous, equal."""
    from gdn_amd import engine as E
    from gdn_amd import ops
    from gdn_amd.optim import Adam
    monkeypatch.setattr(ops, "zeros", lambda shape, device: torch.zeros(shape, device=device))      # (gdn_fill needs a GPU)
    net = _small_net()
    sd = _torch_state(net)
    ar = E.ParamArena(net, torch.device("cpu"))
    net._gdn_param_arena = ar
    opt = Adam(net.parameters(), 1e-3, (0.9, 0.999), eps=1e-8, weight_decay=5e-4)
    st = opt._stores[id(ar)] = opt._new_store(ar.items, ar)      # (as the first step would)
    assert opt.store_of(ar) is st and st.step == 0 and st.m.shape == (ar.numel,) and not st.m.any()
    gen = ar.generation
    opt.load_state_dict(sd)
    assert ar.generation > gen and st.step == 2 and st.pstep is None and not opt._parked.moments
    for k, (p, o, n, tr) in enumerate(ar.items):
        want = sd["state"][k]["exp_avg"]
        if tr is not None:
            fwd, _ = E._perm(tr)
            assert torch.equal(st.m[o:o + n], want.permute(*fwd).reshape(-1)), "parameter %d is not tap-major" % k
            assert not torch.equal(st.m[o:o + n], want.reshape(-1))
        else:
            assert torch.equal(st.m[o:o + n], want.reshape(-1))
    out = opt.state_dict()
    assert list(out["state"]) == list(range(len(ar.items))) and out["param_groups"][0]["params"] == list(range(len(ar.items)))
    for k, p in enumerate(net.parameters()):
        for name in ("exp_avg", "exp_avg_sq"):
            t = out["state"][k][name]
            assert t.shape == p.shape and t.is_contiguous() and torch.equal(t, sd["state"][k][name])
        assert float(out["state"][k]["step"]) == 2.0
    torch.optim.Adam(net.parameters(), 1e-3).load_state_dict({"state": out["state"], "param_groups": out["param_groups"]})


def test_optimizer_load_before_the_first_step_and_refusals():
    from gdn_amd.optim import Adam
    net = _small_net()
    sd = _torch_state(net)
    opt = Adam(net.parameters(), 5e-4)
    opt.load_state_dict(sd)                       # no arena, no store: parked
    assert opt.param_groups[0]["lr"] == 1e-3 and opt.param_groups[0]["betas"] == (0.9, 0.999)
    back = opt.state_dict()
    assert all(torch.equal(back["state"][k]["exp_avg_sq"], sd["state"][k]["exp_avg_sq"]) and
               float(back["state"][k]["step"]) == 2.0 for k in sd["state"])
    other = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3), torch.nn.BatchNorm2d(3))
    with pytest.raises(GdnError, match="6 parameters.*4 parameters"):
        Adam(other.parameters()).load_state_dict(sd)
    wide = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 5), torch.nn.BatchNorm2d(3), torch.nn.ConvTranspose2d(3, 2, 3))
    with pytest.raises(GdnError, match=r"shape \(3, 2, 3, 3\), the parameter has \(3, 2, 5, 5\)"):
        Adam(wide.parameters()).load_state_dict(sd)


# ---------------------------------------------------------------------------------------------------------------------
def test_save_training_state_is_atomic(tmp_path):
    """A writer that dies mid-file leaves the previous state file as it was and no temporary file behind."""
    from gdn_amd import trainer as T
    from gdn_amd.optim import Adam
    net = _small_net()
    opt = Adam(net.parameters(), 1e-3)
    opt.load_state_dict(_torch_state(net))
    path = str(tmp_path / "run" / T.STATE_FILE)
    assert T.save_training_state(path, net, opt, None, {"epoch": 1, "i": 4, "lr": 1e-3, "model_num": 2, "seen": 30, "step": 9}) == path
    before = open(path, "rb").read()

    def dying(state, f):
        f.write(b"half a file")
        f.flush()
        raise OSError("disk full")

    with pytest.raises(OSError, match="disk full"):
        T.save_training_state(path, net, opt, None, {"epoch": 2, "i": 0}, writer=dying)
    assert open(path, "rb").read() == before and os.listdir(tmp_path / "run") == [T.STATE_FILE]
    state = T.read_training_state(path)
    net2 = _small_net()
    with torch.no_grad():
        for p in net2.parameters():
            p.add_(1.0)
    opt2 = Adam(net2.parameters(), 1e-3)
    assert T.load_training_state(state, net2, opt2, None) == {"epoch": 1, "i": 4, "lr": 1e-3, "model_num": 2, "seen": 30, "step": 9}
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), net2.state_dict().values()))
    assert len(opt2.state_dict()["state"]) == 6


def test_resume_flags_and_error_paths(tmp_path):
    from gdn_amd import GDN_main, option
    from gdn_amd import trainer as T
    a = option.parse_args(["--synthetic", "--save_state", "--save_state_every", "7", "--resume", "x.pt"])
    assert a.save_state is True and a.save_state_every == 7 and a.resume == "x.pt"
    d = option.parse_args(["--synthetic"])
    assert d.save_state is False and d.save_state_every == 0 and d.resume is None
    GDN_main._check_resume(d)
    with pytest.raises(FileNotFoundError, match="no such file"):
        GDN_main._check_resume(option.parse_args(["--resume", str(tmp_path / "missing.pt")]))
    there = tmp_path / "state.pt"
    there.write_bytes(b"")
    GDN_main._check_resume(option.parse_args(["--resume", str(there)]))
    with pytest.raises(RuntimeError, match="--init_from"):
        GDN_main._check_resume(option.parse_args(["--resume", str(there), "--init_from", "w.pkl"]))
    net = _small_net()
    state = T.training_state(net, torch.optim.Adam(net.parameters()), None, {"epoch": 0, "i": 0})
    state["world"] = 2
    with pytest.raises(GdnError, match="2 rank.*this run has 1"):
        T.load_training_state(state, net, torch.optim.Adam(net.parameters()), None)


# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(300)
def test_two_ranks_gather_and_take_back_their_loader_state(tmp_path):
    """world = 2 under gloo: every rank's loader state (its own draw streams, its shard's position) is gathered to rank 0,
    which writes the file; on resume every rank reads it and goes on with ITS batches."""
    import resume_worker
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=resume_worker.run, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(60)
    assert sorted(res) == [(0, "ok"), (1, "ok")], res
