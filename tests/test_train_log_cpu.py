"""--train_log without a GPU: the ring's row layout decoded from hand-built bytes, the file's number and null
encoding, the host half of trainlog.TrainLog driven by a restatement of the kernel (the file of a fake run byte for byte, a
flush in the middle, rows that follow their step row), resume truncation and the header check, the command line's refusals,
the three symbols in the header, the library and the binding, the argument checks (they answer before any launch) and the
reader's summary."""
import ctypes
import json
import math
import re
import struct

import pytest
import torch

from conftest import REPO

BASE = ["synthetic", "--synthetic"]
QNAN = 0x7fc00000


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _row(seq, t, skip, lr, norm, coef, terms):
    """64 bytes as gdn_step_record writes them; lr / norm / coef / terms are BIT PATTERNS."""
    return struct.pack("<QiiIIIi8I", seq, t, skip, lr, norm, coef, len(terms), *(list(terms) + [QNAN] * (8 - len(terms))))


def _ring(cap, rows, count):
    buf = bytearray(64 * (1 + cap))
    struct.pack_into("<Q", buf, 0, count)
    for r in rows:
        (seq,) = struct.unpack_from("<Q", r, 0)
        buf[64 * (1 + seq % cap):64 * (2 + seq % cap)] = r
    return bytes(buf)


# ---- the ring ---------------------------------------------------------------------------------------------------------------
def test_decode_a_hand_built_ring():
    from gdn_amd import trainlog as L
    rows = [_row(0, 1, 0, _bits(2e-5), _bits(3.5), _bits(1.0), [_bits(0.5), _bits(-0.0), 0x7fc01234]),
            _row(1, -1, -1, QNAN, QNAN, QNAN, []),
            _row(2, 2, 1, _bits(1e-5), QNAN, _bits(0.0), [_bits(1e30)] * 8)]
    got = L.decode_ring(_ring(4, rows, 3), 4)
    assert [r["seq"] for r in got] == [0, 1, 2]
    assert got[0] == {"seq": 0, "t": 1, "skip": 0, "lr": float(struct.unpack("<f", struct.pack("<f", 2e-5))[0]), "norm": 3.5,
                      "coef": 1.0, "terms": got[0]["terms"]}
    assert got[0]["terms"][0] == 0.5 and math.copysign(1.0, got[0]["terms"][1]) == -1.0 and math.isnan(got[0]["terms"][2])
    assert got[1] == {"seq": 1, "t": None, "skip": None, "lr": None, "norm": None, "coef": None, "terms": []}
    # a guard whose norm is the quiet NaN itself (a non-finite step) is a norm, not an absent record
    assert got[2]["skip"] == 1 and math.isnan(got[2]["norm"]) and got[2]["coef"] == 0.0 and len(got[2]["terms"]) == 8
    assert L.decode_ring(_ring(4, [], 0), 4) == []


def test_decode_a_wrapped_ring():
    from gdn_amd import trainlog as L
    rows = [_row(s, s + 1, 0, _bits(1e-4), _bits(float(s)), _bits(1.0), [_bits(float(10 * s))]) for s in range(11)]
    got = L.decode_ring(_ring(4, rows, 11), 4)            # slots hold rows 8, 9, 10, 7
    assert [r["seq"] for r in got] == [7, 8, 9, 10] and [r["terms"] for r in got] == [[70.0], [80.0], [90.0], [100.0]]
    with pytest.raises(L.TrainLogError, match="bytes"):
        L.decode_ring(_ring(4, rows, 11)[:-1], 4)
    bad = bytearray(_ring(4, rows, 11))
    struct.pack_into("<Q", bad, 64, 3)                    # slot 0 claims another row
    with pytest.raises(L.TrainLogError, match="slot 0"):
        L.decode_ring(bytes(bad), 4)


def test_numbers_and_nulls_as_the_file_holds_them():
    from gdn_amd import trainlog as L
    f32 = struct.unpack("<f", struct.pack("<f", 0.1))[0]
    assert json.dumps(L.number(f32)) == "0.10000000149011612" == repr(f32)
    assert [L.number(x) for x in (float("nan"), float("inf"), float("-inf"), None)] == ["nan", "inf", "-inf", None]
    assert json.dumps(L.number(-0.0)) == "-0.0"
    assert math.isnan(L.value("nan")) and L.value("-inf") == float("-inf") and L.value(None) is None and L.value(0.25) == 0.25
    row = {"seq": 0, "t": None, "skip": None, "lr": None, "norm": None, "coef": None, "terms": [float("nan"), 1.5]}
    assert L.step_line(row, 0, 2, 3) == ('{"step": 3, "epoch": 0, "i": 2, "terms": ["nan", 1.5], "update": null, "lr": null, '
                                         '"grad_norm": null, "clip_coef": null, "skipped": null}')
    assert L.norms_line(4, [[4.0, 9.0], [float("inf"), float("nan")]], -0.5) == \
        '{"step": 4, "weight_norm": [2.0, "inf"], "grad_norm": [1.5, "nan"]}'
    assert L.validation_line(3, 0, ["abs_rel", "a1"], [0.25, float("nan")]) == '{"step": 3, "epoch": 0, "val": {"abs_rel": 0.25, "a1": "nan"}}'


# ---- the host half, on a restatement of the kernel ----------------------------------------------------------------------------
class _Event:
    def synchronize(self):
        pass


class _Opt:
    """An optimizer as TrainLog.record sees one: log_records(arena) -> (hyper, state, guard), here the values themselves."""

    def __init__(self, lr, t, guard):
        self.records = (lr, t, guard)

    def log_records(self, arena):
        return self.records


def _fake_log(path, names, cap, header=None, resume_step=None):
    """trainlog.TrainLog on the CPU: the four device primitives replaced, record() a restatement of gdn_step_record."""
    from gdn_amd import trainlog as L

    class Fake(L.TrainLog):
        copies = syncs = 0

        def _pinned(self, shape, dtype):
            return torch.empty(shape, dtype=dtype)

        def _event(self):
            return _Event()

        def _mark(self, event):
            pass

        def _sync(self):
            Fake.syncs += 1

        def _copy(self):
            Fake.copies += 1
            super()._copy()

        def _launch(self, terms, hyper, state, guard):
            buf = bytearray(self.ring.numpy().tobytes())
            (count,) = struct.unpack_from("<Q", buf, 0)
            skip, norm, coef = guard if guard is not None else (-1, None, None)
            row = _row(count, -1 if state is None else state, skip, QNAN if hyper is None else _bits(hyper),
                       QNAN if norm is None else _bits(norm), QNAN if coef is None else _bits(coef), [_bits(t) for t in terms])
            buf[64 * (1 + count % self.cap):64 * (2 + count % self.cap)] = row
            struct.pack_into("<Q", buf, 0, count + 1)
            self.ring.copy_(torch.frombuffer(buf, dtype=torch.uint8))
    return Fake(path, names, cap, "cpu", header=header, resume_step=resume_step), Fake


HEADER = {"mode": "DtoD", "dtype": "fp32", "loss": "berhu", "world": 1, "batch_size": 2, "accum_steps": 1, "optimizer": "adam",
          "groups": [1.0], "loose_parameters": 0}
HEADER_LINE = ('{"gdn_train_log": 1, "terms": ["total_loss", "output_loss"], "mode": "DtoD", "dtype": "fp32", "loss": "berhu", '
               '"world": 1, "batch_size": 2, "accum_steps": 1, "optimizer": "adam", "groups": [1.0], "loose_parameters": 0}')


def _step_text(step, epoch, i, guarded=True):
    upd = '"update": %d, "lr": 0.5, "grad_norm": %s, "clip_coef": 0.25, "skipped": 0' % (step, float(step)) if guarded else \
        '"update": null, "lr": null, "grad_norm": null, "clip_coef": null, "skipped": null'
    return '{"step": %d, "epoch": %d, "i": %d, "terms": [%s, -0.0], %s}' % (step, epoch, i, float(step) / 4, upd)


def _drive(log, steps, first=1, norms=(), val_after=(), flush_after=()):
    for step in range(first, first + steps):
        epoch, i = (step - 1) // 3, (step - 1) % 3
        open_group = step == 5
        log.record([step / 4, -0.0], None if open_group else _Opt(0.5, step, (0, float(step), 0.25)))
        log.note(epoch, i, step)
        if step in norms:
            log.followers.append((log.issued - 1, (step, torch.tensor([[4.0, 0.25]], dtype=torch.float64), _Event(), 2.0)))
        if step in val_after:
            log.validation(step, epoch, ["abs_rel"], [0.125])
        if step in flush_after:
            log.flush()


def _expected(upto, norms=(2, 4, 6), val_after=(3, 6)):
    lines = [HEADER_LINE]
    for step in range(1, upto + 1):
        lines.append(_step_text(step, (step - 1) // 3, (step - 1) % 3, guarded=step != 5))
        if step in norms:
            lines.append('{"step": %d, "weight_norm": [2.0], "grad_norm": [1.0]}' % step)
        if step in val_after:
            lines.append('{"step": %d, "epoch": %d, "val": {"abs_rel": 0.125}}' % (step, (step - 1) // 3))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("cap", [1, 4, 256])
@pytest.mark.parametrize("flush_after", [(), (3,), (2, 4), (1, 2, 3, 4, 5, 6)])
def test_the_file_of_a_fake_run_byte_for_byte(tmp_path, cap, flush_after):
    """Six steps in two epochs, norms every second step, a validation after each epoch, one micro-batch without an update:
    the same bytes whatever the ring's size and wherever the run flushes; one copy per `cap` rows plus one per flush that has
    something new."""
    path = tmp_path / "log.jsonl"
    log, Fake = _fake_log(path, ["total_loss", "output_loss"], cap, HEADER)
    _drive(log, 6, norms=(2, 4, 6), val_after=(3, 6), flush_after=flush_after)
    if cap == 4 and not flush_after:
        assert Fake.copies == 1 and Fake.syncs == 0 and path.read_text() == HEADER_LINE + "\n"     # rows 1-4 wait for their turn
    log.close()
    assert path.read_text() == _expected(6)
    assert Fake.syncs == len(flush_after) + 1
    if cap == 256:
        assert Fake.copies == len(flush_after) + (0 if 6 in flush_after else 1)
    log.close()                                          # (a second close is a no-op)


def test_steady_state_writes_the_previous_buffer(tmp_path):
    path = tmp_path / "log.jsonl"
    log, Fake = _fake_log(path, ["total_loss", "output_loss"], 2, HEADER)
    _drive(log, 6)
    log.file.flush()
    # after 6 steps at cap 2: three copies, the first two written out by note() itself, no sync
    assert Fake.copies == 3 and Fake.syncs == 0 and path.read_text() == _expected(4, (), ())
    log.close()
    assert path.read_text() == _expected(6, (), ())


def test_a_record_without_its_note_is_noticed(tmp_path):
    from gdn_amd import trainlog as L
    log, _ = _fake_log(tmp_path / "log.jsonl", ["a", "b"], 4, HEADER)
    log.record([1.0, 2.0])
    log.record([1.0, 2.0])
    log.note(0, 0, 1)
    with pytest.raises(L.TrainLogError, match="note"):
        log.flush()
    with pytest.raises(L.TrainLogError, match="2 terms"):
        log.record([1.0])
    with pytest.raises(L.TrainLogError, match="at most 8"):
        _fake_log(tmp_path / "x.jsonl", list("abcdefghi"), 4, HEADER)
    with pytest.raises(L.TrainLogError, match="at least one row"):
        _fake_log(tmp_path / "x.jsonl", ["a"], 0, HEADER)


# ---- resume ---------------------------------------------------------------------------------------------------------------------
def test_resume_drops_later_rows_and_appends(tmp_path):
    path = tmp_path / "log.jsonl"
    log, _ = _fake_log(path, ["total_loss", "output_loss"], 4, HEADER)
    _drive(log, 5, norms=(2, 4), val_after=(3,))
    log.close()                                          # the run died after step 5; its last state file is of step 3
    assert path.read_text() == _expected(5, (2, 4), (3,))
    log, _ = _fake_log(path, ["total_loss", "output_loss"], 4, HEADER, resume_step=3)
    assert path.read_text() == _expected(3, (2,), (3,))
    _drive(log, 3, first=4, norms=(4, 6), val_after=(6,))
    log.close()
    assert path.read_text() == _expected(6)
    # a fresh run overwrites; a resumed run without a file starts one
    log, _ = _fake_log(path, ["total_loss", "output_loss"], 4, HEADER)
    log.close()
    assert path.read_text() == HEADER_LINE + "\n"
    log, _ = _fake_log(tmp_path / "new.jsonl", ["total_loss", "output_loss"], 4, HEADER, resume_step=3)
    log.close()
    assert (tmp_path / "new.jsonl").read_text() == HEADER_LINE + "\n"


@pytest.mark.parametrize("key,value", [("dtype", "bf16"), ("batch_size", 4), ("groups", [1.0, 0.5]), ("tensors", ["a.weight"])])
def test_resume_refuses_another_runs_file_and_names_the_key(tmp_path, key, value):
    from gdn_amd import trainlog as L
    path = tmp_path / "log.jsonl"
    log, _ = _fake_log(path, ["total_loss", "output_loss"], 4, HEADER)
    _drive(log, 2)
    log.close()
    before = path.read_text()
    with pytest.raises(L.TrainLogError, match=r"header has %s = " % key):
        _fake_log(path, ["total_loss", "output_loss"], 4, dict(HEADER, **{key: value}), resume_step=2)
    with pytest.raises(L.TrainLogError, match="header has terms"):
        _fake_log(path, ["total_loss"], 4, HEADER, resume_step=2)
    assert path.read_text() == before
    path.write_text("not a log\n")
    with pytest.raises(L.TrainLogError, match="header"):
        _fake_log(path, ["total_loss", "output_loss"], 4, HEADER, resume_step=2)


# ---- command line ------------------------------------------------------------------------------------------------------------------
def _no_gpu_calls(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the check touched the GPU")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "is_initialized", boom)


def test_parser_defaults_and_values():
    from gdn_amd import option
    a = option.parse_args(BASE)
    assert (a.train_log, a.train_log_every, a.tensor_norms_every) == (None, None, None)
    assert option.train_log_spec(a) == (None, 256, 0)
    a = option.parse_args(BASE + ["--train_log", "x.jsonl", "--train_log_every", "4", "--tensor_norms_every", "2"])
    assert option.train_log_spec(a) == ("x.jsonl", 4, 2)
    text = " ".join(option.build_parser().format_help().split())
    assert "--train_log PATH" in text and "--train_log_every N" in text and "--tensor_norms_every M" in text
    assert "--skip_nonfinite alone gives the norm column without clipping" in text


@pytest.mark.parametrize("flags,match", [
    (["--train_log_every", "4"], "--train_log_every"),
    (["--tensor_norms_every", "2"], "--tensor_norms_every"),
    (["--tensor_norms_every", "0"], "--tensor_norms_every"),
    (["--train_log", "x.jsonl", "--mode", "DtoD_test"], "--train_log.*trains nothing"),
    (["--train_log", "x.jsonl", "--mode", "RtoD_test"], "--train_log.*trains nothing"),
    (["--train_log", "x.jsonl", "--train_log_every", "0"], "--train_log_every 0"),
    (["--train_log", "x.jsonl", "--train_log_every", "-3"], "--train_log_every -3"),
    (["--train_log", "x.jsonl", "--tensor_norms_every", "-1"], "--tensor_norms_every -1")])
def test_refused_before_the_gpu(monkeypatch, tmp_path, flags, match):
    from gdn_amd import GDN_main, option
    _no_gpu_calls(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.chdir(tmp_path)
    argv = BASE + (["--mode", "DtoD"] if "--mode" not in flags else []) + flags
    with pytest.raises(RuntimeError, match=match):
        GDN_main.run(option.parse_args(argv))
    assert not (tmp_path / "x.jsonl").exists()
    GDN_main._check_train_log(option.parse_args(BASE + ["--mode", "DtoD_test"]))             # no flag: nothing to refuse
    GDN_main._check_train_log(option.parse_args(BASE + ["--mode", "DtoD", "--train_log", "x.jsonl", "--train_log_every", "1",
                                                        "--tensor_norms_every", "0"]))


def test_parser_refuses_a_cadence_that_is_no_integer(capsys):
    from gdn_amd import option
    for flag in ("--train_log_every", "--tensor_norms_every"):
        with pytest.raises(SystemExit):
            option.parse_args(BASE + ["--train_log", "x", flag, "1.5"])
        assert flag in capsys.readouterr().err


def test_the_header_describes_the_run():
    from gdn_amd import option
    from gdn_amd import trainer as T
    from gdn_amd.optim import Adam
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 2, 3), torch.nn.BatchNorm2d(2))
    ps = list(net.parameters())
    stray = torch.nn.Parameter(torch.zeros(3))
    opt = Adam([{"params": ps[:2]}, {"params": ps[2:] + [stray], "lr_mult": 0.5}], 1e-3, segmented=True)
    args = option.parse_args(BASE + ["--mode", "RtoD", "--dtype", "bf16", "--batch_size", "4", "--optimizer", "adamw", "--loss", "silog"])
    h = T.train_log_header(args, net, opt, 2, True)
    assert h == {"mode": "RtoD", "dtype": "bf16", "loss": "silog", "world": 1, "batch_size": 4, "accum_steps": 2,
                 "optimizer": "adamw", "groups": [1.0, 0.5], "loose_parameters": 1,
                 "tensors": ["0.weight", "0.bias", "1.weight", "1.bias"]}
    assert "tensors" not in T.train_log_header(args, net, opt, 2, False)
    assert T._DTOD.terms == ("total_loss", "output_loss", "gradient_loss")
    assert T._RTOD.terms == ("total_loss", "output_loss", "smoothness_loss", "latent_loss")


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_built_and_bound_at_revision_223():
    from gdn_amd import _lib as L
    hdr = (REPO / "include" / "gdn_hip.h").read_text()
    flat = " ".join(hdr.split())
    assert ("int gdn_step_record(void* ring, int32_t cap, const float* const* terms, int32_t n_terms, const float* hyper, "
            "const void* state, const void* guard, void* stream);") in flat
    assert "size_t gdn_tensor_sumsq_workspace_bytes(int64_t n, int32_t T);" in flat
    assert ("int gdn_tensor_sumsq(const float* p, const float* g, int64_t n, const int64_t* seg, int32_t T, double* out, "
            "void* workspace, size_t workspace_bytes, void* stream);") in flat
    dll = ctypes.CDLL(str(L.LIB_PATH))
    i32, i64, P, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    for name in ("gdn_step_record", "gdn_tensor_sumsq_workspace_bytes", "gdn_tensor_sumsq"):
        assert hasattr(dll, name) and name in L.EXPORTS, name
    assert L._SIGS["gdn_step_record"] == (i32, [P, i32, P, i32, P, P, P, P])
    assert L._SIGS["gdn_tensor_sumsq_workspace_bytes"] == (sz, [i64, i32])
    assert L._SIGS["gdn_tensor_sumsq"] == (i32, [P, P, i64, P, i32, P, P, sz, P])
    assert {"gdn_step_record", "gdn_tensor_sumsq"} <= L._STATUS_FUNCS
    assert L.ABI_VERSION == 223 and L.lib.gdn_version() == 223
    assert "Added WITHOUT a new ABI revision, like gdn_grad_accumulate" in hdr[hdr.index("gdn_step_record:"):]


def test_argument_checks_answer_before_any_launch():
    """GDN_ERR_BAD_ARG (-1) for every case of the header; the pointers are never dereferenced, so no GPU is needed."""
    from gdn_amd._lib import lib
    rec, ws_bytes, sumsq = lib.raw("gdn_step_record"), lib.raw("gdn_tensor_sumsq_workspace_bytes"), lib.raw("gdn_tensor_sumsq")
    A = 0x10000                                         # a 64 KiB aligned, never dereferenced address
    terms = (ctypes.c_void_p * 8)(*[A + 4 * j for j in range(8)])
    bad_terms = (ctypes.c_void_p * 8)(A, None, A)
    odd_terms = (ctypes.c_void_p * 8)(A, A + 2, A)
    for args in [(None, 4, terms, 3, A, A, A), (A, 0, terms, 3, A, A, A), (A, -1, terms, 3, A, A, A),
                 (A, 4, terms, -1, A, A, A), (A, 4, terms, 9, A, A, A), (A, 4, None, 1, A, A, A),
                 (A, 4, bad_terms, 3, A, A, A), (A, 4, odd_terms, 3, A, A, A), (A + 4, 4, terms, 3, A, A, A),
                 (A, 4, terms, 3, A, A + 4, A), (A, 4, terms, 3, A, A, A + 4), (A, 4, terms, 3, A + 2, A, A)]:
        assert rec(*args, None) == -1, args
    n, T = 1 << 20, 5
    nb = ws_bytes(n, T)
    assert nb == (T + 1) * 8 + ((n + 16383) // 16384 + T) * 16 and ws_bytes(0, T) == 0 and ws_bytes(n, 0) == 0
    for args in [(None, A, n, A, T, A, A, nb), (A, A, n, None, T, A, A, nb), (A, A, n, A, T, None, A, nb),
                 (A, A, n, A, T, A, None, nb), (A, A, 0, A, T, A, A, nb), (A, A, -5, A, T, A, A, nb), (A, A, n, A, 0, A, A, nb),
                 (A + 4, A, n, A, T, A, A, nb), (A, A + 8, n, A, T, A, A, nb), (A, A, n, A + 4, T, A, A, nb),
                 (A, A, n, A, T, A + 4, A, nb), (A, A, n, A, T, A, A + 4, nb), (A, A, n, A, T, A, A, nb - 1),
                 (A, None, n, A, T, A, A, nb - 1)]:
        assert sumsq(*args, None) == -1, args


# ---- the reader --------------------------------------------------------------------------------------------------------------
def test_reader_summary_and_top(tmp_path, capsys):
    from gdn_amd import trainlog as L
    path = tmp_path / "log.jsonl"
    header = L.make_header(["total_loss", "output_loss"], dict(HEADER, tensors=["a.weight", "a.bias", "b.weight"]))
    lines = [json.dumps(header)]

    def step(step, epoch, i, terms, update, lr, norm, coef, skipped):
        lines.append(json.dumps({"step": step, "epoch": epoch, "i": i, "terms": [L.number(t) for t in terms], "update": update,
                                 "lr": L.number(lr), "grad_norm": L.number(norm), "clip_coef": L.number(coef), "skipped": skipped}))
    step(1, 0, 0, [1.0, 0.5], 1, 1e-5, 4.0, 0.25, 0)
    step(2, 0, 1, [3.0, 1.5], 2, 2e-5, 2.0, 0.5, 0)
    step(3, 0, 2, [2.0, 1.0], 2, 2e-5, float("nan"), 0.0, 1)
    lines.append(L.norms_line(3, [[4.0, 1.0], [1.0, float("nan")], [16.0, 64.0]], 1.0))
    lines.append(L.validation_line(3, 0, ["abs_rel"], [0.5]))
    step(4, 1, 0, [4.0, 2.0], 3, 1.5e-5, 0.5, 1.0, 0)
    step(5, 1, 1, [6.0, 3.0], None, None, None, None, None)
    path.write_text("\n".join(lines) + "\n")
    out = L.summary(path, top=2)
    assert out[0] == "log.jsonl: 5 step rows, 1 norms rows; terms: total_loss, output_loss"
    assert out[1] == ("epoch 1: 3 steps  total_loss 2  output_loss 1  grad_norm min 2 median 3 max 4  clipped 2 skipped 1  "
                      "last lr 2.000000e-05")
    assert out[2] == ("epoch 2: 2 steps  total_loss 5  output_loss 2.5  grad_norm min 0.5 median 0.5 max 0.5  clipped 0 skipped 0  "
                      "last lr 1.500000e-05")
    assert out[3] == "step 3: largest grad_norm / weight_norm"
    assert out[4].split()[:2] == ["a.bias", "nan"] and out[5].split()[:2] == ["b.weight", "2"] and len(out) == 6
    assert len(L.summary(path)) == 3
    L.main([str(path), "--top", "1"])
    printed = capsys.readouterr().out.splitlines()
    assert printed == out[:5]
    header2, steps, norms, vals = L.read_log(path)
    assert header2 == header and len(steps) == 5 and len(norms) == 1 and vals == [{"step": 3, "epoch": 0, "val": {"abs_rel": 0.5}}]
