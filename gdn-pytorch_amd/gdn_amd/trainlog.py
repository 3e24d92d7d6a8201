"""--train_log: a per-step record of a training run, kept on the device and written as JSON lines.

Every record a step's row needs already lives in device memory at a fixed place: the 0-dim loss tensors, the rate in the Adam
hyper table, the update count of the step state and the gradient guard's norm, coefficient and skip decision.  One small
launch per step (gdn_step_record, capturable: a --graph replay carries it) copies them into a ring of 64-byte rows; the host
reads the ring once every `cap` steps, with one asynchronous copy into a pinned buffer whose event it waits for only `cap`
steps later.  tensor_norms() is the heavier instrument: the norms of every parameter tensor and of its gradient in one pass
over the arena (gdn_tensor_sumsq).  No wall-clock value enters the file: the same run writes the same bytes.

    python -m gdn_amd.trainlog FILE [--top K]

prints a summary per epoch, and with --top the K tensors whose gradient is largest relative to their weights.

The file: line 1 is the header {"gdn_train_log": 1, "terms": [...], ...run description}; then
    {"step", "epoch", "i", "terms": [...], "update", "lr", "grad_norm", "clip_coef", "skipped"}     one per loader batch
    {"step", "weight_norm": [...], "grad_norm": [...]}                                             after its step row
    {"step", "epoch", "val": {name: value}}                                                        after a validation
`step` counts loader batches over the run from 1 (train_state.pt's 'step'), `update` is the device's count of applied updates;
the five update columns are null where the run has no such device record.  Finite numbers are Python's repr of the value
widened to double, non-finite ones the strings "nan", "inf", "-inf".
"""
import collections
import json
import math
import os
import struct
import sys

ROW_BYTES = 64                 # a ring row, and the ring's header (gdn_step_record)
MAX_TERMS = 8
FORMAT = 1
_ROW = struct.Struct("<QiiIIIi8I")       # seq, t, skip, lr, norm, coef (bit patterns), n_terms, terms (bit patterns)
QUIET_NAN = 0x7fc00000                   # what the kernel writes for a float whose record is absent
UPDATE_COLUMNS = ("update", "lr", "grad_norm", "clip_coef", "skipped")


class TrainLogError(RuntimeError):
    pass


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def number(x):
    """A value as the file holds it: None, a finite float (json writes its repr) or 'nan' / 'inf' / '-inf'."""
    if x is None:
        return None
    x = float(x)
    if math.isnan(x):
        return "nan"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return x


def value(x):
    """number()'s inverse for a reader: a float (NaN and the infinities included) or None."""
    return None if x is None else float(x)


def ring_bytes(cap):
    return ROW_BYTES * (1 + int(cap))


def decode_ring(buf, cap):
    """The rows a ring of `cap` rows holds, oldest first: [{'seq', 't', 'skip', 'lr', 'norm', 'coef', 'terms': [...]}] with
    floats widened to double and None where the row says its record was absent (t or skip -1; lr, norm, coef a quiet NaN
    beside it).  buf: the 64 + 64 * cap bytes of the ring.  After count > cap launches only the last `cap` rows are there."""
    buf = bytes(buf)
    if len(buf) != ring_bytes(cap):
        raise TrainLogError("a ring of %d rows is %d bytes, got %d" % (cap, ring_bytes(cap), len(buf)))
    (count,) = struct.unpack_from("<Q", buf, 0)
    rows = []
    for seq in range(max(0, count - cap), count):
        f = _ROW.unpack_from(buf, ROW_BYTES * (1 + seq % cap))
        if f[0] != seq:
            raise TrainLogError("ring slot %d holds row %d where row %d belongs (count %d)" % (seq % cap, f[0], seq, count))
        t, skip, n = f[1], f[2], f[6]
        if not 0 <= n <= MAX_TERMS:
            raise TrainLogError("ring row %d claims %d terms" % (seq, n))
        have_state, have_guard = t >= 0, skip >= 0
        # (a guard's norm may be the quiet NaN itself -- a non-finite step -- so `skip` says whether there was a guard; a
        # rate is never a NaN, so the kernel's quiet NaN says there was no hyper row)
        lr = None if f[3] == QUIET_NAN else _f32(f[3])
        rows.append({"seq": seq, "t": t if have_state else None, "skip": skip if have_guard else None, "lr": lr,
                     "norm": _f32(f[4]) if have_guard else None, "coef": _f32(f[5]) if have_guard else None,
                     "terms": [_f32(b) for b in f[7:7 + n]]})
    return rows


def step_line(row, epoch, i, step):
    """The file's line for one decoded ring row."""
    return json.dumps({"step": int(step), "epoch": int(epoch), "i": int(i), "terms": [number(v) for v in row["terms"]],
                       "update": row["t"], "lr": number(row["lr"]), "grad_norm": number(row["norm"]),
                       "clip_coef": number(row["coef"]), "skipped": row["skip"]})


def norms_line(step, sums, scale):
    """The norms row from [T][2] sums of squares (weights, gradient): square roots, the gradient's times |scale|."""
    s = abs(float(scale))
    return json.dumps({"step": int(step), "weight_norm": [number(math.sqrt(w)) for w, _ in sums],
                       "grad_norm": [number(math.sqrt(g) * s) for _, g in sums]})


def validation_line(step, epoch, names, values):
    return json.dumps({"step": int(step), "epoch": int(epoch), "val": {str(n): number(v) for n, v in zip(names, values)}})


def make_header(term_names, header):
    names = [str(n) for n in term_names]
    if len(names) > MAX_TERMS:
        raise TrainLogError("the training log holds at most %d terms per step, got %d" % (MAX_TERMS, len(names)))
    full = {"gdn_train_log": FORMAT, "terms": names}
    for k, v in (header or {}).items():
        if k in full:
            raise TrainLogError("the header key %r is the log's own" % k)
        full[k] = v
    return json.loads(json.dumps(full))          # as a reader sees it: tuples are lists


class LogFile:
    """The file side: the header line, then lines in the order they are given.  resume_step None: a fresh run, the file is
    overwritten.  Otherwise the run continues after loader batch `resume_step`: an existing file must carry this run's header
    (the first differing key is named), its rows with a larger `step` are dropped and the run appends."""

    def __init__(self, path, header, resume_step=None):
        self.path = str(path)
        keep = None
        if resume_step is not None and os.path.isfile(self.path):
            with open(self.path, "r") as f:
                lines = f.read().splitlines()
            if not lines:
                raise TrainLogError("--train_log %s exists and is empty: not a training log to continue" % self.path)
            try:
                theirs = json.loads(lines[0])
            except ValueError:
                theirs = None
            if not isinstance(theirs, dict) or theirs.get("gdn_train_log") != FORMAT:
                raise TrainLogError("--train_log %s does not start with a training-log header of format %d" % (self.path, FORMAT))
            for k in list(header) + [k for k in theirs if k not in header]:
                if theirs.get(k, None) != header.get(k, None) or (k in theirs) != (k in header):
                    raise TrainLogError("--train_log %s was written by another run: its header has %s = %r, this run has %r "
                                        "(continue into the file of the run being resumed, or name a new file)"
                                        % (self.path, k, theirs.get(k), header.get(k)))
            keep = [ln for ln in lines[1:] if ln and int(json.loads(ln)["step"]) <= int(resume_step)]
        os.makedirs(os.path.dirname(self.path) or ".", exist_ok=True)
        tmp = "%s.tmp.%d" % (self.path, os.getpid())       # (a kill during the rewrite leaves the file as it was)
        with open(tmp, "w") as f:
            f.write(json.dumps(header) + "\n")
            for ln in keep or []:
                f.write(ln + "\n")
        os.replace(tmp, self.path)
        self.f = open(self.path, "a")

    def write(self, line):
        self.f.write(line + "\n")

    def flush(self):
        self.f.flush()

    def close(self):
        if self.f is not None:
            self.f.flush()
            self.f.close()
            self.f = None


class TrainLog:
    """The training log of one run on one device (rank 0's).  header: the run's description (make_header adds the format and
    the term names); model: the trained network, whose arena store's records record() reads; resume_step: see LogFile.

    record(terms, optimizer) is the device half -- one gdn_step_record launch, capturable -- and note(epoch, i, step) the host
    half, called once per record OUTSIDE any capture: it counts, and after every `cap` records enqueues one copy of the ring
    into the free pinned buffer and an event, then writes out the other buffer, whose event is `cap` steps old.  Nothing else
    copies or reads; flush() synchronises once."""

    def __init__(self, path, term_names, cap, device, header=None, model=None, resume_step=None):
        import torch
        self.cap = int(cap)
        if self.cap < 1:
            raise TrainLogError("--train_log_every %d: the ring holds at least one row" % self.cap)
        self.n_terms = len(term_names)
        self.file = LogFile(path, make_header(term_names, header), resume_step)
        self.device, self.model = torch.device(device), model
        self.ring = torch.zeros(ring_bytes(self.cap), dtype=torch.uint8, device=self.device)
        self.host = [self._pinned((ring_bytes(self.cap),), torch.uint8) for _ in range(2)]
        self.events = [self._event(), self._event()]
        self.pending = [False, False]          # the pinned buffer holds a copy nobody has written out yet
        self.cur = 0                           # the buffer the next copy goes to
        self.issued = self.written = 0         # rows noted / rows written (the ring's seq)
        self.meta = collections.deque()        # (seq, epoch, i, step) of the rows noted and not written
        self.followers = collections.deque()   # (after seq, line or (step, pinned sums, event, scale)): rows that follow a step row
        self.seg = self.sums = None            # tensor_norms: the arena's segment table and the device result
        self._seg_key, self._free = None, []

    # ---- the four things the host half asks of the device (a test without a GPU replaces them) ---------------------------
    def _pinned(self, shape, dtype):
        import torch
        return torch.empty(shape, dtype=dtype).pin_memory()

    def _event(self):
        import torch
        return torch.cuda.Event()

    def _mark(self, event):
        import torch
        event.record(torch.cuda.current_stream(self.device))

    def _sync(self):
        import torch
        torch.cuda.current_stream(self.device).synchronize()

    # ---- device half -----------------------------------------------------------------------------------------------------
    def record(self, terms, optimizer=None):
        """The step's row: the 0-dim float32 device tensors `terms` and the records of `optimizer` (optim.Adam.log_records:
        param group 0 of the trained model's arena store); None for a micro-batch that closed no accumulation group."""
        if len(terms) != self.n_terms:
            raise TrainLogError("the training log was opened for %d terms, the step has %d" % (self.n_terms, len(terms)))
        hyper = state = guard = None
        records = getattr(optimizer, "log_records", None)
        if records is not None:
            hyper, state, guard = records(getattr(self.model, "_gdn_param_arena", None))
        self._launch(terms, hyper, state, guard)

    def _launch(self, terms, hyper, state, guard):
        from . import ops
        ops.step_record(self.ring, self.cap, terms, hyper, state, guard)

    # ---- host half -------------------------------------------------------------------------------------------------------
    def note(self, epoch, i, step):
        self.meta.append((self.issued, int(epoch), int(i), int(step)))
        self.issued += 1
        if self.issued % self.cap == 0:
            self._copy()
            other = 1 - self.cur
            if self.pending[other]:
                self.events[other].synchronize()       # `cap` steps old
                self._write(other)
            self.cur = other

    def _copy(self):
        self.host[self.cur].copy_(self.ring, non_blocking=True)
        self._mark(self.events[self.cur])
        self.pending[self.cur] = True

    def _write(self, which):
        rows = decode_ring(self.host[which].numpy().tobytes(), self.cap)
        self.pending[which] = False
        self._followers(self.written - 1)
        for row in rows:
            if row["seq"] < self.written:
                continue
            if row["seq"] != self.written or not self.meta or self.meta[0][0] != row["seq"]:
                raise TrainLogError("training log: ring row %d arrived where row %d was due (a record() without its note(), "
                                    "or more than %d records between two copies)" % (row["seq"], self.written, self.cap))
            _, epoch, i, step = self.meta.popleft()
            self.file.write(step_line(row, epoch, i, step))
            self.written += 1
            self._followers(row["seq"])

    def _followers(self, seq):
        while self.followers and self.followers[0][0] <= seq:
            _, item = self.followers.popleft()
            if isinstance(item, str):
                self.file.write(item)
                continue
            step, sums, event, scale = item
            event.synchronize()
            self.file.write(norms_line(step, sums.tolist(), scale))
            if self.sums is not None and sums.shape == self.sums.shape:
                self._free.append(sums)

    def tensor_norms(self, step, arena, scale=1.0):
        """The norms of every parameter tensor of `arena` and of its gradient, as a row that follows the last noted step row:
        one gdn_tensor_sumsq launch, one asynchronous copy of [T][2] doubles, one event."""
        import torch
        from . import ops
        key = (id(arena), arena.numel, len(arena.items))
        if self._seg_key != key:
            table = [[o, n] for _, o, n, _ in arena.items]
            self.seg = torch.tensor(table, dtype=torch.int64).to(self.device)
            self.sums = torch.empty((len(table), 2), dtype=torch.float64, device=self.device)
            self._seg_key, self._free = key, []
        ops.tensor_sumsq(arena.data, arena.grad, self.seg, self.sums)
        host = self._free.pop() if self._free else self._pinned(self.sums.shape, torch.float64)
        host.copy_(self.sums, non_blocking=True)
        event = self._event()
        self._mark(event)
        self.followers.append((self.issued - 1, (int(step), host, event, float(scale))))

    def validation(self, step, epoch, names, values):
        """A row from numbers the validation has already copied to the host; it follows the last noted step row."""
        self.followers.append((self.issued - 1, validation_line(step, epoch, names, values)))

    def flush(self):
        """One synchronisation; everything issued so far is in the file afterwards."""
        if self.file.f is None:
            return
        covered = self.written         # rows in the file, or in the copy the last multiple of `cap` made
        if self.pending[1 - self.cur]:
            covered = max(covered, self.issued // self.cap * self.cap)
        if self.issued > covered:
            self._copy()
        self._sync()
        for which in (1 - self.cur, self.cur):
            if self.pending[which]:
                self._write(which)
        self._followers(self.written - 1)
        self.file.flush()

    def close(self):
        self.flush()
        self.file.close()


# ---- the reader ------------------------------------------------------------------------------------------------------------
def read_log(path):
    """(header, step rows, norms rows, validation rows) of a training log."""
    with open(path, "r") as f:
        lines = [ln for ln in f.read().splitlines() if ln]
    if not lines:
        raise TrainLogError("%s is empty" % path)
    header = json.loads(lines[0])
    if not isinstance(header, dict) or header.get("gdn_train_log") != FORMAT:
        raise TrainLogError("%s does not start with a training-log header of format %d" % (path, FORMAT))
    steps, norms, vals = [], [], []
    for ln in lines[1:]:
        row = json.loads(ln)
        (vals if "val" in row else norms if "weight_norm" in row else steps).append(row)
    return header, steps, norms, vals


def _median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def summary(path, top=0):
    """The reader's lines: per epoch the mean of each term, min / median / max of the gradient norm (finite values), the
    clipped and skipped counts and the last rate; with top = K the K tensors with the largest grad_norm / weight_norm of the
    last norms row."""
    header, steps, norms, _ = read_log(path)
    names = header["terms"]
    out = ["%s: %d step rows, %d norms rows; terms: %s" % (os.path.basename(str(path)), len(steps), len(norms), ", ".join(names))]
    epochs = collections.OrderedDict()
    for r in steps:
        epochs.setdefault(r["epoch"], []).append(r)
    for epoch, rows in epochs.items():
        parts = ["epoch %d: %d steps" % (epoch + 1, len(rows))]
        for j, name in enumerate(names):
            vs = [value(r["terms"][j]) for r in rows]
            parts.append("%s %.6g" % (name, sum(vs) / len(vs)))
        gn = [value(r["grad_norm"]) for r in rows if r["grad_norm"] is not None]
        finite = [v for v in gn if math.isfinite(v)]
        if finite:
            parts.append("grad_norm min %.6g median %.6g max %.6g" % (min(finite), _median(finite), max(finite)))
        if gn:
            clipped = sum(1 for r in rows if r["clip_coef"] is not None and value(r["clip_coef"]) < 1.0 and not r["skipped"])
            parts.append("clipped %d skipped %d" % (clipped, sum(1 for r in rows if r["skipped"])))
        rates = [value(r["lr"]) for r in rows if r["lr"] is not None]
        if rates:
            parts.append("last lr %.6e" % rates[-1])
        out.append("  ".join(parts))
    if top and norms:
        last = norms[-1]
        tensors = header.get("tensors") or ["tensor %d" % k for k in range(len(last["weight_norm"]))]
        ratio = []
        for name, w, g in zip(tensors, last["weight_norm"], last["grad_norm"]):
            w, g = value(w), value(g)
            ratio.append((g / w if w > 0.0 else (float("inf") if g != 0.0 else 0.0), name, g, w))
        ratio.sort(key=lambda t: (-(t[0] if t[0] == t[0] else float("inf")), t[1]))
        out.append("step %d: largest grad_norm / weight_norm" % last["step"])
        for q, name, g, w in ratio[:int(top)]:
            out.append("  %-40s %.6g  (grad %.6g, weight %.6g)" % (name, q, g, w))
    return out


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="python -m gdn_amd.trainlog", description="Summarise a --train_log file")
    p.add_argument("file")
    p.add_argument("--top", type=int, default=0, metavar="K",
                   help="also list the K tensors with the largest grad_norm / weight_norm of the last norms row")
    a = p.parse_args(argv)
    print("\n".join(summary(a.file, a.top)))


if __name__ == "__main__":
    main(sys.argv[1:])
