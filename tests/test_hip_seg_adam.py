"""The segmented Adam family on the GPU, kernel level: gdn_adam_step_seg, gdn_grad_sumsq_seg and gdn_ema_update_seg against
the per-slice entry points they replace (gdn_adam_step_dev[_guarded], gdn_grad_sumsq, gdn_ema_update).  The yardstick is bit
identity with those kernels on every live slice and untouched bits in every skipped chunk; the norm is held to float64
(tests/grad_guard_fp64.py)."""
import struct

import numpy as np
import pytest
import torch

import grad_guard_fp64 as R

pytestmark = pytest.mark.gpu

STEP_FMT = "<ddiff"
SKIP = 0xFF
# three groups with their own learning rate and weight decay; hyper[5] (the gradient scale) is the optimizer's, one value
GROUPS = [(1e-3, 0.9, 0.999, 1e-8, 5e-4, 0.5), (2.5e-4, 0.9, 0.999, 1e-8, 0.0, 0.5), (3e-3, 0.8, 0.99, 1e-6, 1e-2, 0.5)]
SIZES = [1, 63, 64, 65, 4097, 129]
GROUP_OF = [0, SKIP, 1, 2, 0, SKIP]          # items 1 and 5 are frozen
SENTINELS = np.array([0x7FC00000, 0xFFC12345, 0x7F800000, 0xDEADBEEF, 0x00000001, 0x80000000], dtype=np.uint32)


def _layout(sizes, group_of):
    """Offsets of 64-float aligned slices, the arena length and the chunk map (padding after an item belongs to it)."""
    items, off = [], 0
    for n in sizes:
        items.append((off, n))
        off += -(-n // 64) * 64
    cmap = np.full(off // 64, SKIP, np.uint8)
    for (o, n), k in zip(items, group_of):
        cmap[o // 64:(o + n + 63) // 64] = k
    return items, off, cmap


def _state(gpu, t=0, b1=0.9, b2=0.999):
    raw = struct.pack(STEP_FMT, float(np.float64(np.float32(b1)) ** t), float(np.float64(np.float32(b2)) ** t), t, 0.0, 0.0)
    return torch.frombuffer(bytearray(raw + b"\0" * 4), dtype=torch.uint8).to(gpu)


def _states(gpu, groups):
    return torch.cat([_state(gpu, 0, g[1], g[2]) for g in groups])


def _guard(gpu, coef=1.0, skip=0):
    raw = struct.pack(R.RECORD_FMT, 0.0, 1.0, coef, skip, 1, 0, 0)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(gpu)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _poison(buf, cmap):
    """NaNs and sentinel bit patterns into every float of every skipped chunk."""
    raw = buf.cpu().numpy().view(np.uint32).copy()
    for c in np.nonzero(cmap == SKIP)[0]:
        raw[c * 64:(c + 1) * 64] = np.resize(SENTINELS, 64)
    return torch.from_numpy(raw.view(np.float32)).to(buf.device)


def _arena(gpu, n, cmap, items, seed):
    """p, g, m, v, ema with zero padding inside live slices and poison in skipped chunks."""
    rng = np.random.default_rng(seed)
    bufs = []
    for scale, positive in ((1.0, False), (1e-2, False), (1e-3, False), (1e-6, True), (1.0, False)):
        a = np.zeros(n, np.float32)
        for o, k in items:
            x = rng.standard_normal(k).astype(np.float32) * np.float32(scale)
            a[o:o + k] = np.abs(x) if positive else x
        bufs.append(_poison(torch.from_numpy(a).to(gpu), cmap))
    return bufs


def _run_steps(gpu, sizes, group_of, guarded, steps=3, seed=7):
    from gdn_amd import ops
    items, n, cmap = _layout(sizes, group_of)
    p, g, m, v, ema = _arena(gpu, n, cmap, items, seed)
    before = [_bits(t).clone() for t in (p, g, m, v, ema)]
    rp, rm, rv, rema = p.clone(), m.clone(), v.clone(), ema.clone()
    dmap = torch.from_numpy(cmap).to(gpu)
    hyper = torch.tensor(GROUPS, dtype=torch.float32, device=gpu)
    states, rstates = _states(gpu, GROUPS), [_state(gpu, 0, gr[1], gr[2]) for gr in GROUPS]
    guard = _guard(gpu, coef=0.37) if guarded else None
    live = [(o, k, grp) for (o, k), grp in zip(items, group_of) if grp != SKIP]
    for _ in range(steps):
        ops.adam_step_seg(p, g, m, v, dmap, hyper, states, guard)
        ops.ema_update_seg(ema, p, dmap, 0.99, states, guard)
        # the reference: the existing kernels slice by slice; a group's state advances with the first slice of the group and
        # the others run on a scratch copy of the state as it was before, which the call advances to the same bytes
        seen = {}
        for o, k, grp in live:
            st = rstates[grp] if grp not in seen else seen[grp].clone()
            if grp not in seen:
                seen[grp] = st.clone()
            sl = slice(o, o + k)
            if guarded:
                ops.adam_step_dev_guarded(rp[sl], g[sl], rm[sl], rv[sl], hyper[grp], st, guard)
            else:
                ops.adam_step_dev(rp[sl], g[sl], rm[sl], rv[sl], hyper[grp], st)
            ops.ema_update(rema[sl], rp[sl], 0.99, st, guard)
            assert _same_bits(st, rstates[grp])
    torch.cuda.synchronize()
    for o, k, grp in live:
        sl = slice(o, o + k)
        for name, got, want in (("p", p, rp), ("m", m, rm), ("v", v, rv), ("ema", ema, rema)):
            assert _same_bits(got[sl], want[sl]), "%s of the slice at %d (%d floats, group %d) differs" % (name, o, k, grp)
        pad = slice(o + k, o + -(-k // 64) * 64)
        for t in (p, m, v, ema):
            assert not t[pad].any(), "padding of the slice at %d did not stay zero" % o
    for k, rs in enumerate(rstates):
        assert _same_bits(states[32 * k:32 * k + 28], rs[:28]), "step state of group %d" % k
        assert struct.unpack_from(STEP_FMT, states.cpu().numpy().tobytes(), 32 * k)[2] == steps
    skipped = torch.from_numpy(np.repeat(cmap == SKIP, 64))
    for t, b in zip((p, g, m, v, ema), before):
        assert torch.equal(_bits(t)[skipped], b[skipped]), "a skipped chunk was written"
    assert _same_bits(g, before[1].view(torch.float32))
    return p, g, dmap, cmap


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
def test_update_is_bit_identical_per_slice_and_skipped_chunks_keep_their_bits(gpu, guarded):
    """Items of 1, 63, 64, 65, 4097 and 129 floats, three groups, two frozen items full of NaNs and sentinels, three steps:
    p, m, v, the average and every group's step state equal the per-slice kernels' bit for bit."""
    from gdn_amd import ops
    p, g, dmap, cmap = _run_steps(gpu, SIZES, GROUP_OF, guarded)
    rec = _guard(gpu)
    ops.grad_sumsq_seg(g, dmap, rec)
    assert np.isfinite(R.unpack(rec.cpu().numpy().tobytes())["sumsq"])


def test_grid_stride_and_tail(gpu):
    """About 5 M floats (the update's grid covers 4096 x 256 x 4 of them per trip), a skipped block in the middle and a
    live final chunk."""
    sizes = [2_000_003, 640_000, 2_400_000, 64]
    _run_steps(gpu, sizes, [0, SKIP, 2, 1], guarded=True, steps=1)


def test_grad_sumsq_seg_against_float64(gpu):
    """|norm32 - ref64| <= (n 2^-53 + 2^-24) ref64 over the live elements; the same call twice gives the same bytes; a NaN in
    a live chunk makes the sum non-finite."""
    from gdn_amd import ops
    sizes, group_of = [4097, 300_001, 65, 2 * 1024 * 4096 + 7, 129], [0, SKIP, 1, 2, SKIP]
    items, n, cmap = _layout(sizes, group_of)
    rng = np.random.default_rng(20261019)
    host = np.zeros(n, np.float32)
    ref = 0.0
    for (o, k), grp in zip(items, group_of):
        host[o:o + k] = (rng.standard_normal(k) * 10.0 ** rng.uniform(-12, 12, k)).astype(np.float32)
        if grp != SKIP:
            ref += R.sumsq(host[o:o + k])
    g = _poison(torch.from_numpy(host).to(gpu), cmap)
    dmap = torch.from_numpy(cmap).to(gpu)
    hyper = torch.tensor(GROUPS[0][:5] + (1.0,), dtype=torch.float32, device=gpu)
    a, b = _guard(gpu), _guard(gpu)
    ops.grad_sumsq_seg(g, dmap, a)
    ops.grad_sumsq_seg(g, dmap, b)
    assert torch.equal(a, b)
    ops.grad_guard_finalize(a, hyper, 0.0, True)
    got = R.unpack(a.cpu().numpy().tobytes())
    want = R.norm64(ref)
    err = abs(float(got["norm"]) - want) / want
    print("n=%d: norm32 %.9e ref64 %.9e rel err %.3e" % (n, float(got["norm"]), want, err))
    assert got["skip"] == 0 and err <= n * 2.0 ** -53 + 2.0 ** -24
    # accumulate adds to what the record holds
    ops.grad_sumsq_seg(g, dmap, b, accumulate=True)
    assert R.unpack(b.cpu().numpy().tobytes())["sumsq"] == 2.0 * got["sumsq"]
    g[items[2][0] + 64] = float("nan")
    ops.grad_sumsq_seg(g, dmap, a)
    assert not np.isfinite(R.unpack(a.cpu().numpy().tobytes())["sumsq"])


def test_a_skipped_step_touches_nothing(gpu):
    from gdn_amd import ops
    items, n, cmap = _layout(SIZES, GROUP_OF)
    p, g, m, v, ema = _arena(gpu, n, cmap, items, 11)
    before = [_bits(t).clone() for t in (p, g, m, v, ema)]
    dmap = torch.from_numpy(cmap).to(gpu)
    hyper = torch.tensor(GROUPS, dtype=torch.float32, device=gpu)
    states = _states(gpu, GROUPS)
    s0 = states.clone()
    guard = _guard(gpu, coef=0.0, skip=1)
    ops.adam_step_seg(p, g, m, v, dmap, hyper, states, guard)
    ops.ema_update_seg(ema, p, dmap, 0.99, states, guard)
    for t, b in zip((p, g, m, v, ema), before):
        assert torch.equal(_bits(t), b)
    assert torch.equal(states, s0)


def test_bad_arguments(gpu):
    from gdn_amd import ops
    from gdn_amd._lib import GdnError, lib
    n = 256
    buf = torch.zeros(n + 64, dtype=torch.float32, device=gpu)
    p, g, m, v = (buf[:n].clone() for _ in range(4))
    cmap = torch.zeros(n // 64, dtype=torch.uint8, device=gpu)
    hyper = torch.tensor(GROUPS[:1], dtype=torch.float32, device=gpu)
    states, guard = _states(gpu, GROUPS[:1]), _guard(gpu)
    ws = torch.zeros(8192, dtype=torch.uint8, device=gpu)
    P = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def step(p=p, g=g, m=m, v=v, n=n, cmap=cmap, G=1, hyper=hyper, states=states):
        lib.gdn_adam_step_seg(P(p), P(g), P(m), P(v), n, P(cmap), G, P(hyper), P(states), None, None)

    def sumsq(g=g, n=n, cmap=cmap, guard=guard):
        lib.gdn_grad_sumsq_seg(P(g), n, P(cmap), P(guard), 0, P(ws), ws.numel(), None)

    def ema(e=m, p=p, n=n, cmap=cmap, decay=0.99, states=states):
        lib.gdn_ema_update_seg(P(e), P(p), n, P(cmap), decay, P(states), None, None)

    odd = buf[1:1 + n]
    bad = [("gdn_adam_step_seg", step, kw) for kw in (
        dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(cmap=None), dict(hyper=None), dict(states=None),
        dict(n=0), dict(n=-64), dict(n=n - 1), dict(G=0), dict(G=255), dict(p=odd), dict(g=odd), dict(m=odd), dict(v=odd))]
    bad += [("gdn_grad_sumsq_seg", sumsq, kw) for kw in (
        dict(g=None), dict(cmap=None), dict(guard=None), dict(n=0), dict(n=n - 1), dict(g=odd))]
    bad += [("gdn_ema_update_seg", ema, kw) for kw in (
        dict(e=None), dict(p=None), dict(cmap=None), dict(states=None), dict(n=0), dict(n=n + 1), dict(e=odd), dict(p=odd),
        dict(decay=0.0), dict(decay=1.0))]
    for name, fn, kw in bad:
        with pytest.raises(GdnError, match=name + " failed: bad argument"):
            fn(**kw)
    torch.cuda.synchronize()
    assert not buf.any() and not p.any() and not m.any() and not v.any()
    # the Python wrappers check what the library leaves to its caller
    with pytest.raises(GdnError, match="chunk map"):
        ops.adam_step_seg(p, g, m, v, cmap[:-1], hyper, states)
    with pytest.raises(GdnError, match="step states"):
        ops.adam_step_seg(p, g, m, v, cmap, hyper, torch.cat([states, states]))
