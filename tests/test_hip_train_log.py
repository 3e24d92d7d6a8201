"""--train_log on the GPU: gdn_step_record against a restatement of its row layout, bit for bit, eager and
replayed from a hipGraph; gdn_tensor_sumsq against math.fsum of the exact float64 squares at a derived bar; and the flags end
to end through GDN_main.run at the smallest model shapes (16 x 32, batch 2, 3 batches per epoch, 2 epochs), the harness of
tests/test_hip_lr_schedule.py.

The bar of every sum of squares is derived, not measured: a float32 squared is exact in double, and a sum of L non-negative
doubles in any order is within (L - 1) 2^-53 relative of the exact sum, so rtol = L 2^-53 per segment against math.fsum.  Two
such sums (the kernel's and torch's float64 one) differ by at most 2 L 2^-53; the square root halves that, and the two roots
and the two products by |scale| add one rounding each: norms agree within (L + 4) 2^-53."""
import collections
import json
import math
import hashlib
import os
import shutil
import struct

import pytest
import torch

import libcalls

pytestmark = pytest.mark.gpu

H, W = 16, 32
QNAN = 0x7fc00000
U53 = 2.0 ** -53


# ---- gdn_step_record ----------------------------------------------------------------------------------------------------------
TERM_BITS = [0x7fc01234, 0x80000000, 0x00000001, struct.unpack("<I", struct.pack("<f", 1e30))[0],       # NaN with payload, -0,
             0xff800000, 0x7f812345, 0x3f800000, 0x00000000]                                            # subnormal, 1e30, ...


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _row(seq, t, skip, lr, norm, coef, terms):
    return struct.pack("<QiiIIIi8I", seq, t, skip, lr, norm, coef, len(terms), *(list(terms) + [QNAN] * (8 - len(terms))))


def _dev_bytes(gpu, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(gpu)


def _records(gpu, k):
    """hyper, step state and guard record number k on the device, with the values a row shows of them."""
    lr, t, norm, coef, skip = _bits(1e-4 * (k + 1)), 100 + k, _bits(3.0 + k) if k % 3 else QNAN, _bits(1.0 / (k + 1)), k % 2
    hyper = torch.tensor([1e-4 * (k + 1), 0.9, 0.999, 1e-8, 5e-4, 1.0], dtype=torch.float32).to(gpu)
    assert _bits(hyper[0].item()) == lr
    state = _dev_bytes(gpu, struct.pack("<ddiff", 0.5, 0.25, t, 0.5, 0.75) + b"\0" * 4)
    guard = _dev_bytes(gpu, struct.pack("<dIIiiii", 9.0, norm, coef, skip, 7, 2, 1))
    return (hyper, state, guard), (lr, t, norm, coef, skip)


def _term_tensors(gpu, bits):
    buf = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).to(gpu).view(torch.float32)
    return buf, [buf[j] for j in range(len(bits))]


def test_step_record_rows_bit_for_bit(gpu):
    """cap 4, 11 calls: n_terms 0, 3 and 8, every subset of {hyper, state, guard}, the ring read after every call."""
    from gdn_amd import ops
    cap = 4
    ring = torch.zeros(64 * (1 + cap), dtype=torch.uint8, device=gpu)
    want = bytearray(64 * (1 + cap))
    _, terms = _term_tensors(gpu, TERM_BITS)
    for call in range(11):
        n = (0, 3, 8)[call % 3]
        (hyper, state, guard), (lr, t, norm, coef, skip) = _records(gpu, call)
        use = [(call >> b) & 1 == 0 for b in range(3)]                # call 0: all three, call 7: none
        ops.step_record(ring, cap, terms[:n], hyper if use[0] else None, state if use[1] else None, guard if use[2] else None)
        row = _row(call, t if use[1] else -1, skip if use[2] else -1, lr if use[0] else QNAN, norm if use[2] else QNAN,
                   coef if use[2] else QNAN, TERM_BITS[:n])
        want[64 * (1 + call % cap):64 * (2 + call % cap)] = row
        struct.pack_into("<Q", want, 0, call + 1)
        assert ring.cpu().numpy().tobytes() == bytes(want), call
    from gdn_amd import trainlog as L
    rows = L.decode_ring(ring.cpu().numpy().tobytes(), cap)
    assert [r["seq"] for r in rows] == [7, 8, 9, 10]
    assert rows[0]["t"] is None and rows[0]["skip"] is None and rows[0]["lr"] is None          # call 7: no record at all
    assert rows[1]["t"] == 108 and rows[1]["skip"] == 0 and len(rows[1]["terms"]) == 8 and rows[1]["terms"][3] == float(
        struct.unpack("<f", struct.pack("<f", 1e30))[0])


def test_step_record_with_a_plain_28_byte_state(gpu):
    from gdn_amd import ops
    from gdn_amd.optim import _step_state
    ring = torch.zeros(128, dtype=torch.uint8, device=gpu)
    state = _step_state({"betas": (0.9, 0.999)}, 4, gpu)
    assert state.numel() == 28
    ops.step_record(ring, 1, [], None, state, None)
    assert ring.cpu().numpy().tobytes()[64:] == _row(0, 4, -1, QNAN, QNAN, QNAN, [])


def test_step_record_replayed_from_a_graph(gpu):
    """Captured once on a single stream, replayed five times with the term tensors and the records rewritten in between: the
    rows advance and carry the new values (the pointers ride in the argument block, the values are read at replay)."""
    from gdn_amd import ops
    cap = 4
    ring = torch.zeros(64 * (1 + cap), dtype=torch.uint8, device=gpu)
    buf, terms = _term_tensors(gpu, TERM_BITS[:3])
    (hyper, state, guard), _ = _records(gpu, 0)
    ops.step_record(ring, cap, terms, hyper, state, guard)            # one eager call first: row 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.step_record(ring, cap, terms, hyper, state, guard)
    torch.cuda.synchronize()
    assert struct.unpack_from("<Q", ring.cpu().numpy().tobytes(), 0)[0] == 1          # capturing executed nothing
    want = bytearray(ring.cpu().numpy().tobytes())
    for k in range(1, 6):
        bits = [TERM_BITS[(k + j) % 8] for j in range(3)]
        (h2, s2, g2), (lr, t, norm, coef, skip) = _records(gpu, k)
        buf.copy_(_term_tensors(gpu, bits)[0])
        hyper.copy_(h2)
        state.copy_(s2)
        guard.copy_(g2)
        g.replay()
        want[64 * (1 + k % cap):64 * (2 + k % cap)] = _row(k, t, skip, lr, norm, coef, bits)
        struct.pack_into("<Q", want, 0, k + 1)
        assert ring.cpu().numpy().tobytes() == bytes(want), k


def test_step_record_bad_arguments_leave_the_ring_alone(gpu):
    from gdn_amd import ops
    from gdn_amd._lib import GdnError, lib
    cap = 4
    ring = torch.zeros(64 * (1 + cap), dtype=torch.uint8, device=gpu)
    _, terms = _term_tensors(gpu, TERM_BITS)
    (hyper, state, guard), _ = _records(gpu, 1)
    ops.step_record(ring, cap, terms[:3], hyper, state, guard)
    before = ring.cpu().numpy().tobytes()
    raw, s = lib.raw("gdn_step_record"), ops.stream()
    import ctypes
    ptrs = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in terms])
    hole = (ctypes.c_void_p * 8)(terms[0].data_ptr(), None, terms[2].data_ptr())
    r, h, st, gd = ring.data_ptr(), hyper.data_ptr(), state.data_ptr(), guard.data_ptr()
    for args in [(None, cap, ptrs, 3, h, st, gd), (r, 0, ptrs, 3, h, st, gd), (r, cap, ptrs, -1, h, st, gd),
                 (r, cap, ptrs, 9, h, st, gd), (r, cap, hole, 3, h, st, gd), (r, cap, None, 2, h, st, gd),
                 (r + 4, cap, ptrs, 3, h, st, gd), (r, cap, ptrs, 3, h, st + 4, gd), (r, cap, ptrs, 3, h, st, gd + 4)]:
        assert raw(*args, s) == -1, args
    with pytest.raises(GdnError, match="gdn_step_record failed"):
        ops.step_record(ring, cap, [terms[0], None], hyper, state, guard)
    with pytest.raises(GdnError, match="at most 8"):
        ops.step_record(ring, cap, terms + terms[:1], hyper, state, guard)
    with pytest.raises(GdnError, match="a ring of"):
        ops.step_record(ring, cap + 1, terms[:1], hyper, state, guard)
    torch.cuda.synchronize()
    assert ring.cpu().numpy().tobytes() == before


# ---- gdn_tensor_sumsq ---------------------------------------------------------------------------------------------------------
SLAB = 16384                                 # floats one workgroup covers
LENGTHS = [1, 63, 64, 65, 4097, 2 * SLAB + 4099, SLAB, 2]      # every tail length 0 .. 3, slabs: 1, 1 and 3


@pytest.fixture(scope="module")
def arena(gpu):
    """A hand-made arena: slices of LENGTHS at ascending multiples of 64 (one gap of several chunks), the padding poisoned
    with NaN in both buffers; (p, g, seg on the device, [(offset, length)], exact float64 sums of squares per segment)."""
    gen = torch.Generator().manual_seed(5)
    table, off = [], 0
    for k, n in enumerate(LENGTHS):
        table.append((off, n))
        off += (n + 63) // 64 * 64 + (192 if k == 2 else 0)
    total = off + 64
    p = torch.full((total,), float("nan"))
    g = torch.full((total,), float("nan"))
    for o, n in table:
        p[o:o + n] = torch.randn(n, generator=gen) * 3.0
        g[o:o + n] = torch.randn(n, generator=gen) * 1e-3
    p[table[4][0] + 7] = 1e30                                 # its square fits a double, not a float
    g[table[5][0] + SLAB + 1] = 1e-30                         # its square is a float32 subnormal's neighbourhood: exact in double
    exact = [(math.fsum((p[o:o + n].double() ** 2).tolist()), math.fsum((g[o:o + n].double() ** 2).tolist())) for o, n in table]
    seg = torch.tensor(table, dtype=torch.int64).to(gpu)
    return p.to(gpu), g.to(gpu), seg, table, exact


def _close(got, want, L):
    return abs(got - want) <= L * U53 * want


def test_tensor_sumsq_against_fsum(gpu, arena):
    from gdn_amd import ops
    p, g, seg, table, exact = arena
    out = ops.tensor_sumsq(p, g, seg).cpu().tolist()
    for k, ((o, n), (wp, wg)) in enumerate(zip(table, exact)):
        print("segment %d (length %d): p %.17g (exact %.17g, rel %.2e of %.2e), g %.17g (exact %.17g, rel %.2e)" %
              (k, n, out[k][0], wp, abs(out[k][0] - wp) / wp, n * U53, out[k][1], wg, abs(out[k][1] - wg) / wg))
        assert _close(out[k][0], wp, n) and _close(out[k][1], wg, n), (k, n, out[k], (wp, wg))


def test_tensor_sumsq_same_bytes_null_g_and_one_inf(gpu, arena):
    from gdn_amd import ops
    p, g, seg, table, exact = arena
    a = ops.tensor_sumsq(p, g, seg).cpu()
    b = ops.tensor_sumsq(p, g, seg).cpu()
    assert a.numpy().tobytes() == b.numpy().tobytes()
    only_p = ops.tensor_sumsq(p, None, seg).cpu()
    assert torch.equal(only_p[:, 0].view(torch.int64), a[:, 0].view(torch.int64)) and not only_p[:, 1].any()
    for k, where in ((5, 2 * SLAB + 4098), (0, 0), (3, 64)):              # the last element of a scalar tail, a lone float
        g2 = g.clone()
        g2[table[k][0] + where] = float("inf") if k != 3 else float("nan")
        c = ops.tensor_sumsq(p, g2, seg).cpu()
        assert torch.equal(c[:, 0].view(torch.int64), a[:, 0].view(torch.int64))
        for j in range(len(table)):
            if j == k:
                assert (math.isinf(c[j, 1].item()) and c[j, 1].item() > 0) if k != 3 else math.isnan(c[j, 1].item())
            else:
                assert c[j, 1].item() == a[j, 1].item()
    one = ops.tensor_sumsq(p, g, seg[4:5].contiguous()).cpu()                  # T = 1
    assert one.numpy().tobytes() == a[4:5].contiguous().numpy().tobytes()


def test_tensor_sumsq_bad_arguments(gpu, arena):
    from gdn_amd import ops
    from gdn_amd._lib import GdnError, lib
    p, g, seg, table, _ = arena
    n, T = p.numel(), len(table)
    out = torch.full((T, 2), -1.0, dtype=torch.float64, device=gpu)
    nb = int(lib.gdn_tensor_sumsq_workspace_bytes(n, T))
    ws = torch.zeros(nb + 64, dtype=torch.uint8, device=gpu)
    raw, s = lib.raw("gdn_tensor_sumsq"), ops.stream()
    P, G, S, O, Wk = p.data_ptr(), g.data_ptr(), seg.data_ptr(), out.data_ptr(), ws.data_ptr()
    for args in [(None, G, n, S, T, O, Wk, nb), (P, G, n, None, T, O, Wk, nb), (P, G, n, S, T, None, Wk, nb),
                 (P, G, n, S, T, O, None, nb), (P, G, 0, S, T, O, Wk, nb), (P, G, n, S, 0, O, Wk, nb),
                 (P + 4, G, n, S, T, O, Wk, nb), (P, G + 8, n, S, T, O, Wk, nb), (P, G, n, S + 4, T, O, Wk, nb),
                 (P, G, n, S, T, O + 4, Wk, nb), (P, G, n, S, T, O, Wk + 4, nb), (P, G, n, S, T, O, Wk, nb - 1)]:
        assert raw(*args, s) == -1, args
    torch.cuda.synchronize()
    assert (out == -1.0).all() and not ws.any()
    with pytest.raises(GdnError, match="int64"):
        ops.tensor_sumsq(p, g, seg.int())
    with pytest.raises(GdnError, match="one size"):
        ops.tensor_sumsq(p, g[:-1], seg)


# ---- the flags, end to end ------------------------------------------------------------------------------------------------------
GUARD = ["--clip_grad_norm", "1", "--skip_nonfinite", "--warmup_steps", "2", "--lr_schedule", "cosine"]
_RUNS = {}
Run = collections.namedtuple("Run", "files log calls seen norms capturable tensors")


class _Stop(Exception):
    pass


@pytest.fixture(scope="module")
def loop_root(tmp_path_factory):
    import gdn_amd.AE_model_unet as M
    root = tmp_path_factory.mktemp("train_log")
    torch.manual_seed(11)
    net = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
    torch.save({"module." + k: v.contiguous() for k, v in net.state_dict().items()}, str(root / "init.pkl"))
    yield root
    _RUNS.clear()
    shutil.rmtree(root, ignore_errors=True)


def _run(root, tag, extra, log=None, dtype="fp32", mode="DtoD", init=True, stop_after_first_state=False, watch=False,
         poison_step=None, warm=False):
    """GDN_main.run in `root`/<tag> (cached).  log: (file name under `root`, --train_log_every, --tensor_norms_every) adds the
    three flags.  watch: after every step read what the row should hold -- the terms' .item(), current_lr() and
    guard_stats() -- and before every norms launch the float64 torch norms of the arena's slices.  poison_step: a NaN is put
    into the gradient arena after the backward of that step (1-based).  warm: the same command runs once before, uncounted --
    what a process does once (the cached seed gradient's fill, for one) then stays out of a comparison of call counts.
    A checkpoint of this model is 0.3 GB whatever the image size, so nothing of a run stays behind but what a later run reads:
    every .pkl is reduced to a digest per tensor and deleted at once (a warm-up run's whole directory), the optimizer is let go.
    Returns Run({file name: {key: digest}}, the log's text, library calls by name, what `watch` saw per step and per norms
    row, whether the optimizer was capturable, the number of tensors in the trained model's arena)."""
    from gdn_amd import GDN_main, option
    from gdn_amd import trainer as T
    from gdn_amd import trainlog as L
    from gdn_amd import utils as U
    if tag in _RUNS:
        return _RUNS[tag]
    if warm:
        _run(root, tag + "_warm", extra, log, dtype, mode, init)
        del _RUNS[tag + "_warm"]
        shutil.rmtree(root / (tag + "_warm"), ignore_errors=True)
    where = root / tag
    where.mkdir(parents=True, exist_ok=True)
    argv = ["synthetic", "--synthetic", "--mode", mode, "--height", str(H), "--width", str(W), "--batch_size", "2",
            "--epoch_size", "3", "--epochs", "2", "--gpu_num", "0", "--dtype", dtype, "-e"]
    if init:
        argv += ["--init_from", str(root / "init.pkl")]
    if log is not None:
        argv += ["--train_log", str(root / log[0]), "--train_log_every", str(log[1])]
        if log[2] is not None:
            argv += ["--tensor_norms_every", str(log[2])]
    cwd, save, make, backward = os.getcwd(), T.save_training_state, GDN_main._make_optimizer, U.backward
    record, note, norms = L.TrainLog.record, L.TrainLog.note, L.TrainLog.tensor_norms
    spy, seen, seen_norms, last, backwards = [], [], [], {}, [0]

    def save_and_stop(*a, **k):
        save(*a, **k)
        raise _Stop()

    def make_and_show(model, args):
        spy.append(make(model, args))
        return spy[-1]

    def poisoned_backward(loss):
        backward(loss)
        backwards[0] += 1
        if backwards[0] == poison_step:
            arena = spy[0].param_groups[0]["params"][0]._gdn_arena
            arena.grad[arena.items[3][1]] = float("nan")

    def record_and_keep(self, terms, optimizer=None):
        last["terms"], last["optimizer"] = terms, optimizer
        record(self, terms, optimizer)

    def note_and_look(self, epoch, i, step):
        opt = last["optimizer"]
        row = {"step": step, "terms": [t.item() for t in last["terms"]]}
        if opt is not None and opt.capturable:
            row["lr"] = opt.current_lr()[0]
            if opt.guarded:
                row["guard"] = opt.guard_stats()
        seen.append(row)
        note(self, epoch, i, step)

    def norms_and_look(self, step, arena, scale=1.0):
        seen_norms.append({"step": step, "n": [n for _, _, n, _ in arena.items], "scale": scale,
                           "w": [float(arena.data[o:o + n].double().pow(2).sum().sqrt()) for _, o, n, _ in arena.items],
                           "g": [float(arena.grad[o:o + n].double().pow(2).sum().sqrt()) * abs(scale) for _, o, n, _ in arena.items]})
        norms(self, step, arena, scale)

    os.chdir(where)
    calls = collections.Counter()
    try:
        GDN_main._make_optimizer = make_and_show
        if stop_after_first_state:
            T.save_training_state = save_and_stop
        if poison_step is not None:
            U.backward = poisoned_backward
        if watch:
            L.TrainLog.record, L.TrainLog.note, L.TrainLog.tensor_norms = record_and_keep, note_and_look, norms_and_look
        calls, _ = libcalls.count_library_calls(lambda: GDN_main.run(option.parse_args(argv + list(extra))))
        assert not stop_after_first_state, "the run wrote no training state"
    except _Stop:
        pass
    finally:
        T.save_training_state, GDN_main._make_optimizer, U.backward = save, make, backward
        L.TrainLog.record, L.TrainLog.note, L.TrainLog.tensor_norms = record, note, norms
        os.chdir(cwd)
    torch.cuda.synchronize()
    files = {}
    for p in sorted(where.rglob("*.pkl")):
        files[p.name] = {k: _digest(v) for k, v in torch.load(p, map_location="cpu").items()}
        p.unlink()
    text = (root / log[0]).read_text() if log is not None and (root / log[0]).exists() else None
    arena = getattr(spy[0].param_groups[0]["params"][0], "_gdn_arena", None) if spy else None
    _RUNS[tag] = Run(files, text, calls, seen, seen_norms, spy[0].capturable if spy else None,
                     None if arena is None else len(arena.items))
    return _RUNS[tag]


def _digest(t):
    t = t.detach().contiguous()
    return (str(t.dtype), tuple(t.shape), hashlib.blake2b(t.reshape(-1).view(torch.uint8).numpy().tobytes(), digest_size=16).hexdigest())


def _same_files(a, b, what):
    assert sorted(a) == sorted(b) and a, (what, sorted(a), sorted(b))
    for name in a:
        assert list(a[name]) == list(b[name])
        for k in a[name]:
            assert a[name][k] == b[name][k], (what, name, k)


def _rows(text):
    lines = text.splitlines()
    header, rows = json.loads(lines[0]), [json.loads(ln) for ln in lines[1:]]
    return (header, [r for r in rows if "terms" in r], [r for r in rows if "weight_norm" in r], [r for r in rows if "val" in r])


def _logged(root):
    return _run(root, "logged", GUARD, log=("logged.jsonl", 4, 2), watch=True)


def test_loop_the_log_changes_nothing_and_holds_what_a_spy_saw(gpu, loop_root):
    from gdn_amd import trainlog as L
    plain = _run(loop_root, "plain", GUARD, warm=True)
    logged = _logged(loop_root)
    assert len(plain.files) == 2
    _same_files(plain.files, logged.files, "--train_log")
    header, steps, norms, vals = _rows(logged.log)
    assert header["gdn_train_log"] == 1 and header["terms"] == ["total_loss", "output_loss", "gradient_loss"]
    assert {k: header[k] for k in ("mode", "dtype", "loss", "world", "batch_size", "accum_steps", "optimizer", "groups",
                                   "loose_parameters")} == \
        {"mode": "DtoD", "dtype": "fp32", "loss": "berhu", "world": 1, "batch_size": 2, "accum_steps": 1, "optimizer": "adam",
         "groups": [1.0], "loose_parameters": 0}
    assert len(header["tensors"]) == logged.tensors == len(norms[0]["weight_norm"])
    assert [(r["step"], r["epoch"], r["i"]) for r in steps] == [(1, 0, 0), (2, 0, 1), (3, 0, 2), (4, 1, 0), (5, 1, 1), (6, 1, 2)]
    assert len(logged.seen) == 6 and [r["step"] for r in vals] == [3, 6] and [r["epoch"] for r in vals] == [0, 1]
    skipped = 0
    for row, saw in zip(steps, logged.seen):
        gs = saw["guard"]
        print(row)
        assert row["terms"] == [L.number(t) for t in saw["terms"]] and all(isinstance(t, float) for t in row["terms"])
        assert row["lr"] == saw["lr"] and row["grad_norm"] == L.number(gs["norm"]) and row["clip_coef"] == L.number(gs["coef"])
        assert row["update"] == gs["steps"] - gs["skipped"] == row["step"] and row["skipped"] == gs["skipped"] - skipped == 0
        skipped = gs["skipped"]
    assert any(r["clip_coef"] < 1.0 for r in steps) and len({r["lr"] for r in steps}) > 2           # the guard clips, the rate moves
    # the norms rows follow their step rows, and agree with float64 torch norms of the slices
    lines = logged.log.splitlines()
    assert [r["step"] for r in norms] == [2, 4, 6] == [r["step"] for r in logged.norms]
    for r in norms:
        k = lines.index(json.dumps(r))
        assert json.loads(lines[k - 1])["step"] == r["step"] and "terms" in json.loads(lines[k - 1])
    for r, saw in zip(norms, logged.norms):
        assert saw["scale"] == 1.0
        for j, n in enumerate(saw["n"]):
            for got, want in ((r["weight_norm"][j], saw["w"][j]), (r["grad_norm"][j], saw["g"][j])):
                assert abs(got - want) <= (n + 4) * U53 * want, (r["step"], j, n, got, want)
    # library calls: one record per loader batch and one norms pass per M steps more than without the flags, nothing else
    assert logged.calls["gdn_step_record"] == 6 and logged.calls["gdn_tensor_sumsq"] == 3
    assert plain.calls["gdn_step_record"] == 0 and plain.calls["gdn_tensor_sumsq"] == 0
    assert logged.calls - plain.calls == collections.Counter(gdn_step_record=6, gdn_tensor_sumsq=3)
    assert not plain.calls - logged.calls


def test_loop_graph_writes_the_same_bytes(gpu, loop_root):
    from gdn_amd import trainer as T
    logged = _logged(loop_root)
    graph = _run(loop_root, "graph", GUARD + ["--graph", "--graph_warmup", "2"], log=("graph.jsonl", 4, 2))
    assert T.last_graph_report["replayed"] == 4 and T.last_graph_report["warmup"] == 2
    _same_files(logged.files, graph.files, "--graph")
    assert graph.log == logged.log
    # the record is part of what is captured: the replays launch it without a library call of their own
    assert graph.calls["gdn_step_record"] == 3 and graph.calls["gdn_tensor_sumsq"] == 3


def test_loop_resume_continues_the_file(gpu, loop_root):
    logged = _logged(loop_root)
    log = ("resumed.jsonl", 4, 2)
    try:
        _resume_checks(loop_root, logged, log)
    finally:
        for p in loop_root.rglob("train_state.pt"):          # three times a checkpoint's size
            p.unlink()


def _resume_checks(loop_root, logged, log):
    from gdn_amd._lib import GdnError
    stopped = _run(loop_root, "stopped", GUARD + ["--save_state"], log=log, stop_after_first_state=True)
    (state,) = sorted((loop_root / "stopped").rglob("train_state.pt"))
    _, steps, norms, vals = _rows(stopped.log)
    # the state file never runs ahead of the log: everything up to its step is in the file when it is written
    assert [r["step"] for r in steps] == [1, 2, 3] and [r["step"] for r in norms] == [2] and [r["step"] for r in vals] == [3]
    assert logged.log.startswith(stopped.log)
    resumed = _run(loop_root, "resumed", GUARD + ["--resume", str(state)], log=log, init=False)
    assert resumed.log == logged.log
    _same_files({k: v for k, v in logged.files.items() if k not in stopped.files}, resumed.files, "--resume")
    before = (loop_root / log[0]).read_text()
    with pytest.raises(GdnError, match="header has tensors"):
        _run(loop_root, "refused", GUARD + ["--resume", str(state)], log=(log[0], 4, None), init=False)
    assert (loop_root / log[0]).read_text() == before


def test_loop_accum_rows_per_batch_updates_per_group(gpu, loop_root):
    """--accum_steps 2 over epochs of 3 batches: groups (0, 1) and (2); the batch inside the open group has no update columns."""
    run = _run(loop_root, "accum", GUARD + ["--accum_steps", "2"], log=("accum.jsonl", 4, 2))
    header, steps, norms, _ = _rows(run.log)
    assert header["accum_steps"] == 2 and len(steps) == 6 and len(norms) == 3 and run.calls["gdn_step_record"] == 6
    for r in steps:
        cols = [r[k] for k in ("update", "lr", "grad_norm", "clip_coef", "skipped")]
        assert all(c is None for c in cols) if r["i"] == 0 else all(c is not None for c in cols), r
    assert [r["update"] for r in steps] == [None, 1, 2, None, 3, 4]


def test_loop_a_nonfinite_step_shows_where(gpu, loop_root):
    run = _run(loop_root, "poisoned", GUARD, log=("poisoned.jsonl", 4, 1), poison_step=3)
    header, steps, norms, _ = _rows(run.log)
    assert [r["skipped"] for r in steps] == [0, 0, 1, 0, 0, 0] and [r["update"] for r in steps] == [1, 2, 2, 3, 4, 5]
    assert steps[2]["grad_norm"] in ("nan", "inf") and steps[2]["clip_coef"] == 0.0 and isinstance(steps[3]["grad_norm"], float)
    assert steps[2]["lr"] == steps[3]["lr"]                       # the skipped step did not advance the schedule
    (row,) = [r for r in norms if r["step"] == 3]
    bad = [header["tensors"][j] for j, v in enumerate(row["grad_norm"]) if isinstance(v, str)]
    print("non-finite gradient in", bad)
    assert bad == [header["tensors"][3]] and all(isinstance(v, float) for v in row["weight_norm"])
    assert all(isinstance(v, float) for r in norms if r["step"] != 3 for v in r["grad_norm"])


def test_loop_rtod_bf16_has_four_terms(gpu, loop_root):
    run = _run(loop_root, "rtod", [], log=("rtod.jsonl", 256, None), dtype="bf16", mode="RtoD", init=False)
    header, steps, norms, _ = _rows(run.log)
    assert header["terms"] == ["total_loss", "output_loss", "smoothness_loss", "latent_loss"] and "tensors" not in header
    assert header["mode"] == "RtoD" and header["dtype"] == "bf16" and len(steps) == 6 and not norms
    assert all(len(r["terms"]) == 4 and all(isinstance(t, float) for t in r["terms"]) for r in steps)
    assert run.calls["gdn_step_record"] == 6 and run.calls["gdn_tensor_sumsq"] == 0


def test_loop_without_device_records_the_columns_are_null(gpu, loop_root):
    """No guard, no schedule, no --graph: the optimizer steps from the host and stays that way -- the log creates no records."""
    bare = _run(loop_root, "bare", [], warm=True)
    run = _run(loop_root, "bare_logged", [], log=("bare.jsonl", 4, 2))
    assert run.capturable is False and bare.capturable is False
    _same_files(bare.files, run.files, "--train_log")
    _, steps, norms, _ = _rows(run.log)
    assert len(steps) == 6 and len(norms) == 3
    assert all(r[k] is None for r in steps for k in ("update", "lr", "grad_norm", "clip_coef", "skipped"))
    assert all(isinstance(t, float) for r in steps for t in r["terms"])
    assert run.calls - bare.calls == collections.Counter(gdn_step_record=6, gdn_tensor_sumsq=3) and not bare.calls - run.calls


def test_the_reader_on_a_real_log(gpu, loop_root):
    from gdn_amd import trainlog as L
    _logged(loop_root)
    out = L.summary(loop_root / "logged.jsonl", top=3)
    print("\n".join(out))
    assert out[1].startswith("epoch 1: 3 steps  total_loss ") and out[2].startswith("epoch 2: 3 steps")
    assert out[3] == "step 6: largest grad_norm / weight_norm" and len(out) == 7
