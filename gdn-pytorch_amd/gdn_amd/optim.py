"""Fused Adam over the model's flat parameter arena.

Same update rule as the reference's ``optim.Adam(model.parameters(), lr,
[momentum, beta], eps=1e-08, weight_decay=5e-4)`` (GDN_main.py:157,173:
coupled L2 weight decay on every parameter, BN affine included), executed as
ONE kernel launch over the arena instead of 124-136 per-tensor launches.

Gradient guard (``max_grad_norm`` / ``skip_nonfinite``): the global gradient norm, ``clip_grad_norm_``'s coefficient and the
decision to skip a step whose gradient holds a NaN or an Inf are taken on the device, in one 32-byte record the update
kernel reads -- no torch kernel, no host read, capturable.

Weight average (``ema_decay``): an exponential moving average of the weights beside the moments, updated by one more launch
after each update under the same skip decision, and exchanged with the weights in place for validation and for the
checkpoint that is deployed.

Gradient accumulation (``micro_batches``): the gradient buffer holds the SUM of that many micro-batch gradients and the
update takes their mean through its gradient scale -- one norm, one decision, one update per group.

Parameter groups and frozen parameters (``segmented``): several param groups over one arena (their own ``weight_decay``, a
learning-rate multiplier ``lr_mult``) and parameters with ``requires_grad = False`` keep the constant launch count -- the
kernels read a map from 64-float chunks of the arena to groups and skip what is frozen.

Learning-rate schedule (``schedule``): warm-up and a constant / linear / cosine decay evaluated on the device from the
device's own update count, one small launch per arena in front of the update -- no host write per step, capturable
(DESIGN.md 3.9).

Decoupled weight decay (``decoupled``, ``AdamW``): the groups' ``weight_decay`` leaves the gradient and decays the weight
directly, at the update's own rate, inside the same launches -- the gdn_adamw_step* entry points in their siblings' places
(DESIGN.md 3.13).
"""
import collections
import contextlib
import struct

import torch

from . import ops
from ._lib import GdnError


# the two device records (gdn_hip.h), as the host packs and reads them
_STEP_FMT = "<ddiff"         # { double beta1^t, beta2^t; int32 t; float bc1, bc2s; }: 28 bytes, which checkpoints carry verbatim
_GUARD_FMT = "<dffiiii"      # { double sumsq; float norm, coef; int32 skip, steps, clipped, skipped; }: 32 bytes


def _record(fmt, *fields):
    return torch.frombuffer(bytearray(struct.pack(fmt, *fields)), dtype=torch.uint8)


def _unpack(fmt, record):
    return struct.unpack_from(fmt, record.cpu().numpy().tobytes())


def _guard_bytes(steps, clipped, skipped):
    """A guard record between two steps: no sum, coefficient 1, no skip, the run's counts."""
    return _record(_GUARD_FMT, 0.0, 0.0, 1.0, 0, steps, clipped, skipped)


def _step_state(group, t, device):
    """The step state for `t` steps TAKEN so far (the kernel advances it before it uses it)."""
    _no_capture("capturable Adam: a device step counter would be created (and reset by every replay) inside a graph "
                "capture; run one eager step with the same gradient coverage first")
    b1, b2 = group["betas"]
    return _record(_STEP_FMT, float(b1) ** t, float(b2) ** t, t, 0.0, 0.0).to(device)


def _f32(x):
    """`x` as the kernels receive it: rounded to float32."""
    return struct.unpack("<f", struct.pack("<f", float(x)))[0]


def _no_capture(message):
    """Refuse what a graph capture cannot hold.  (Asked of a process without a GPU, the stream query itself raises.)"""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise GdnError(message)


def _rank0():
    return not (torch.distributed.is_available() and torch.distributed.is_initialized()) or torch.distributed.get_rank() == 0


_CHUNK = 64          # floats: engine._ALIGN, the alignment of every arena slice
_SKIP = 0xFF         # chunk map entry: a frozen parameter, padding after the last parameter
_STATE_BYTES = 32    # sizeof(AdamDevState): the 28 bytes of _STEP_FMT and 4 of tail padding


def _lr(group):
    """The learning rate the kernels see: lr * lr_mult in double (they round it to float32 once)."""
    return float(group["lr"]) * float(group.get("lr_mult", 1.0))


def _base_rates(rates, device):
    """double[G] on the device: what gdn_lr_schedule scales (a blocking copy, made only when a rate changes)."""
    return torch.tensor(rates, dtype=torch.float64).to(device)


def check_schedule(schedule):
    """Adam(schedule=...) in its one spelling: None, or {'kind': 'constant' | 'linear' | 'cosine', 'warmup': W >= 0,
    'total': T >= 1, 'floor': F in [0, 1]} with plain Python numbers."""
    if schedule is None:
        return None
    unknown = set(schedule) - {"kind", "warmup", "total", "floor"}
    if unknown or "kind" not in schedule:
        raise ValueError("schedule must be a dict with the keys 'kind', 'warmup', 'total', 'floor', got %r" % (schedule,))
    kind, warmup, total = schedule["kind"], int(schedule.get("warmup", 0)), int(schedule.get("total", 1))
    floor = float(schedule.get("floor", 0.0))
    if kind not in ops.LR_SCHEDULE_KINDS:
        raise ValueError("schedule kind %r is not one of %s" % (kind, " / ".join(ops.LR_SCHEDULE_KINDS)))
    if warmup < 0 or total < 1 or not 0.0 <= floor <= 1.0:
        raise ValueError("schedule needs warmup >= 0, total >= 1 and a floor in [0, 1], got %r" % (schedule,))
    return {"kind": kind, "warmup": warmup, "total": total, "floor": floor}


_Row = collections.namedtuple("_Row", "hyper state base_lr")
# one capturable update, gathered: the ranges of the weights, the moments and the average, the gradient, and the device records
_Launch = collections.namedtuple("_Launch", "w m v ema grad hyper state base_lr map")


class _Table:
    """The device side of the capturable path for a set of rows, one per param group: what the kernels read beside the
    weights and the moments.  A plain store owns a table of one row; a segmented store's _Plan is a table with a chunk map.

    param_groups  the rows' param groups (the optimizer's own dicts); None for a table a checkpoint brought the step state
                  of, until the first step says which group it belongs to
    hyper         float32[G, 6] on the device and `hyper_host`, what the host last wrote there
    states        uint8[G * 32] on the device, one step state per row (the 28 bytes of _STEP_FMT and 4 of padding), or None
    base_lr       (Adam(schedule=...) only) float64[G] on the device, each row's lr * lr_mult, and `base_host`
    map           None: a single row, no chunk map, the plain entry points (gdn_adam_step_dev[_guarded], gdn_ema_update)"""
    map = None

    def __init__(self, param_groups, rows, device):
        self.param_groups = param_groups
        self.hyper = torch.zeros(rows, 6, dtype=torch.float32, device=device)
        self.hyper_host = self.states = self.base_lr = self.base_host = None
        self._rows = {}

    def put(self, **buffers):
        """Give the table its `states` or its `base_lr` (the views row() made of the old ones are dropped)."""
        self.__dict__.update(buffers)
        self._rows = {}

    def row(self, k):
        """Row k as the per-tensor entry points take one: hyper[k], the 28 bytes of its step state that checkpoints carry
        (None without states) and base_lr[k:k+1] (None without a schedule).  The same three views every time, so a launch
        costs the host no slicing."""
        r = self._rows.get(k)
        if r is None:
            n = struct.calcsize(_STEP_FMT)
            r = self._rows[k] = _Row(self.hyper[k], None if self.states is None else self.states[_STATE_BYTES * k:_STATE_BYTES * k + n],
                                     None if self.base_lr is None else self.base_lr[k:k + 1])
        return r


def _state_row(state):
    """A 28-byte step state as a row of a table's `states`."""
    return torch.cat([state, torch.zeros(_STATE_BYTES - state.numel(), dtype=torch.uint8, device=state.device)])


class _Plan(_Table):
    """How a segmented optimizer runs one arena: a _Table with one row per param group that has a live
    parameter in the arena, and

    key      per item of the arena the index of its param group in optimizer.param_groups, -1 for a frozen parameter
             (requires_grad False): what the plan was built from, and what makes it stale
    groups   indices of the param groups with a live parameter here, in order of first appearance; a chunk map entry k
             means groups[k], row k of the table
    map      uint8[numel / 64] on the device: the group of every 64-float chunk, or 0xFF (skip)
    states   None while the live parameters' update counts differ (an odd load_state_dict): such an arena runs per tensor
    k_of     id(param) -> its chunk map entry, live parameters only"""

    def __init__(self, items, numel, key, param_groups, device):
        self.key = tuple(key)
        self.groups = []
        for gi in self.key:
            if gi >= 0 and gi not in self.groups:
                self.groups.append(gi)
        if not 1 <= len(self.groups) <= 254:
            raise GdnError("segmented Adam: %d param groups with trainable parameters in one arena; the chunk map holds "
                           "1 to 254" % len(self.groups))
        cmap = bytearray([_SKIP]) * (numel // _CHUNK)
        self.k_of = {}
        for (p, o, n, _), gi in zip(items, self.key):
            if o % _CHUNK or numel % _CHUNK:
                raise GdnError("segmented Adam: an arena slice at float offset %d of %d is not %d-float aligned" % (o, numel, _CHUNK))
            if gi >= 0:
                k = self.k_of[id(p)] = self.groups.index(gi)
                for c in range(o // _CHUNK, (o + n + _CHUNK - 1) // _CHUNK):
                    cmap[c] = k
        super().__init__([param_groups[gi] for gi in self.groups], len(self.groups), device)
        self.map = torch.frombuffer(cmap, dtype=torch.uint8).to(device)


class _Parked:
    """What load_state_dict() read, until the store it belongs to exists (the arena is built by the first forward, the
    stores by the first step).  Tensors in each parameter's LOGICAL layout; _Store.fill() and Adam._guard_record() take
    what is theirs out of it."""

    def __init__(self, guard=None):
        self.moments = {}        # id(param) -> {"step", "m", "v"}
        self.averages = {}       # id(param) -> its weight average
        self.records = {}        # id(a store's first param) -> the store's 'gdn' record, indices replaced by ids
        self.guard = guard       # (steps, clipped, skipped) for a guard record that does not exist yet, or None

    def averages_wait_for_a_step(self):
        # (a parameter that never took a step has no moments waiting either: its average is its value)
        return any(pid in self.moments for pid in self.averages)


class _Store:
    """The Adam state of one arena, or of one loose parameter -- the same thing with one item and no arena.

    items    [(param, offset, numel, transposed or None)]: arena.items, or [(p, 0, p.numel(), None)]
    m, v     the moments in the PHYSICAL layout: flat tensors of arena.numel floats, or zeros_like(p); `ema` the weight
             average beside them (None without ema_decay); view() gives an item's logical-shape view of any of the three
    step     the host's count of updates; `pstep` is None while every parameter has taken that many and becomes
             {id(param): count} once an arena's coverage has been partial (always None for a loose parameter)
    table, plan, pdev, full_dev
             the device side of the capturable path: the store's own one-row _Table (hyper-parameters, step state, base rate;
             `hyper`, `state` and `base_lr` read its row) or -- an arena of a segmented optimizer -- its _Plan,
             {id(param): 28-byte step state} of the per-tensor path, and whether the table's or the plan's step states have
             taken every update so far (then one may be copied for a parameter: ADVICE r4)
    The optimizer keeps its stores in Adam._stores, by id(arena) or id(param); torch.optim.Optimizer.state is not used."""

    def __init__(self, items, arena=None):
        self.items, self.arena = items, arena
        if arena is not None:
            self.device = arena.device
            self.m, self.v = ops.zeros((arena.numel,), arena.device), ops.zeros((arena.numel,), arena.device)
        else:
            p = items[0][0]
            self.device = p.device
            self.m = torch.zeros_like(p, memory_format=torch.preserve_format)
            self.v = torch.zeros_like(p, memory_format=torch.preserve_format)
        self.ema, self.step, self.pstep = None, 0, None
        self._drop_dev()

    def _drop_dev(self):
        self.table, self.pdev, self.full_dev = None, {}, False
        # segmented optimizers only: the arena's _Plan, and the 'seg' entry of a loaded record until a plan takes it
        self.plan = self.seg_rec = None

    # the one row of a plain store's table, as the entry points take it
    hyper = property(lambda self: None if self.table is None or self.table.param_groups is None else self.table.row(0).hyper)
    state = property(lambda self: None if self.table is None else self.table.row(0).state)
    base_lr = property(lambda self: None if self.table is None else self.table.row(0).base_lr)

    @property
    def kind(self):
        return "loose" if self.arena is None else "arena"

    @property
    def weights(self):
        """The live weights buffer the moments run beside."""
        return self.items[0][0].data if self.arena is None else self.arena.data

    def view(self, buf, item):
        """`item`'s logical-shape view of the store buffer `buf` (tap-major underneath for convolution weights)."""
        p, o, _, tr = item
        return buf if self.arena is None else self.arena._view(buf, o, p.shape, tr)

    def ranges(self, item=None):
        """(weights, m, v, average or None): the whole buffers, or `item`'s slice of each."""
        if item is None:
            return self.weights, self.m, self.v, self.ema
        _, o, n, _ = item
        return self.weights[o:o + n], self.m[o:o + n], self.v[o:o + n], None if self.ema is None else self.ema[o:o + n]

    def touch(self):
        """The weights changed behind torch's back: bf16 shadow, eval-BatchNorm coefficients."""
        arena = self.arena if self.arena is not None else getattr(self.items[0][0], "_gdn_arena", None)
        if arena is not None:
            arena.touch()

    def count(self, p, memo=None):
        """Updates parameter `p` has taken: the device's count where the capturable path keeps one (graph replays advance
        it behind the host's back), the host's otherwise.  `memo` saves reading one step state twice."""
        memo = {} if memo is None else memo

        def dev(t, key=None):
            key = id(t) if key is None else key
            if key not in memo:
                memo[key] = _unpack(_STEP_FMT, t)[2]
            return memo[key]
        if self.plan is not None and self.plan.states is not None:
            if id(p) in self.pdev:
                return dev(self.pdev[id(p)])
            k = self.plan.k_of.get(id(p))
            if k is not None:
                return dev(self.plan.row(k).state, (id(self.plan), k))
        if self.state is not None:
            if self.pstep is None:
                return dev(self.state)
            if id(p) in self.pdev:
                return dev(self.pdev[id(p)])
            if self.full_dev:
                return dev(self.state)        # no counter of its own yet: the arena's, frozen when coverage split
        return self.step if self.pstep is None else self.pstep[id(p)]

    def record(self, index):
        """The store's entry of state_dict()['gdn']['stores']; `index`: id(param) -> its number in the param groups."""
        ids = [id(p) for p, _, _, _ in self.items]
        rec = {"kind": self.kind, "params": [index[i] for i in ids], "step": int(self.step),
               "pstep": None if self.pstep is None else [int(self.pstep[i]) for i in ids],
               "full_dev": bool(self.full_dev),
               "state": None if self.state is None else self.state.detach().cpu().clone(),
               "pdev": {index[i]: self.pdev[i].detach().cpu().clone() for i in ids if i in self.pdev}}
        if self.plan is not None:
            # a segmented optimizer's group states: what the plan was built from, and the device's own bytes
            rec["seg"] = {"key": list(self.plan.key),
                          "states": None if self.plan.states is None else self.plan.states.detach().cpu().clone()}
        elif self.seg_rec is not None:
            rec["seg"] = self.seg_rec
        return rec

    def take_record(self, rec, capturable):
        """Host counts and -- capturable -- the device step state from a record() whose indices are ids.  False: no usable
        record (a torch checkpoint, or device counts saved by a capturable optimizer and read by a host-side one), the
        counts come from 'step'."""
        self._drop_dev()
        seg = None if rec is None else rec.get("seg")
        if rec is None or ((rec.get("state") is not None or (seg or {}).get("states") is not None) and not capturable):
            return False
        self.step = int(rec["step"])
        if self.arena is not None and rec["pstep"] is not None:
            self.pstep = dict(zip(rec["params"], [int(c) for c in rec["pstep"]]))
        else:
            self.pstep = None
        if rec.get("state") is not None:
            # the device's own bytes, verbatim, in a table that waits for its param group (Adam._ensure_dev)
            self.table = _Table(None, 1, self.device)
            self.table.put(states=_state_row(rec["state"].to(device=self.device, copy=True)))
        self.seg_rec = seg
        if rec.get("state") is not None or seg is not None:
            self.full_dev = bool(rec["full_dev"])
            if seg is not None or rec["pstep"] is not None:
                self.pdev = {pid: t.to(device=self.device, copy=True) for pid, t in rec["pdev"].items()}
        return True

    def fill(self, parked, capturable, averaged, reset=False):
        """Take what load_state_dict() parked for this store's parameters: each moment and average through the parameter's
        own view of the buffer (tap-major for convolution weights), never under a logical shape.  A new store (the first
        step made it) takes what is there; reset: a store that exists is rewritten, and starts over where nothing was read.
        `averaged`: the store keeps a weight average -- made here as a copy of the weights BEFORE the first update
        (avg_0 = p_0, same physical layout), then overwritten with what was read for it."""
        ids = [id(p) for p, _, _, _ in self.items]
        if reset or any(i in parked.moments for i in ids):
            self.m.zero_()
            self.v.zero_()
            counts = {}
            for item in self.items:
                s = parked.moments.pop(id(item[0]), None)
                counts[id(item[0])] = s["step"] if s else 0
                if s:
                    self.view(self.m, item).copy_(s["m"])
                    self.view(self.v, item).copy_(s["v"])
            rec = parked.records.pop(ids[0], None)
            if rec is not None and (rec["kind"] != self.kind or rec["params"] != ids):
                rec = None
            if not self.take_record(rec, capturable):
                level = set(counts.values())
                self.step, self.pstep = (level.pop(), None) if len(level) == 1 else (max(level), counts)
        if not averaged:
            return
        if self.ema is None:
            _no_capture("Adam(ema_decay): the weight average would be created inside a graph capture; run one eager step "
                        "with the same gradient coverage first")
            self.ema = self.weights.detach().clone(memory_format=torch.preserve_format)
        elif reset:
            self.ema.copy_(self.weights)
        for item in self.items:
            avg = parked.averages.pop(id(item[0]), None)
            if avg is not None:
                self.view(self.ema, item).copy_(avg)

    # host counts under graph capture and replay
    def counts(self):
        return self.step, None if self.pstep is None else dict(self.pstep)

    def take_back(self, step, pstep):
        """Undo what a capture added since counts() gave (step, pstep); returns it as the per-replay increments."""
        dp = None
        if pstep is not None and self.pstep is not None:
            dp = {k: self.pstep[k] - c for k, c in pstep.items()}
            self.pstep.update(pstep)
        dstep, self.step = self.step - step, step
        return dstep, dp

    def advance(self, dstep, dp):
        self.step += dstep
        if dp is not None and self.pstep is not None:
            for k, d in dp.items():
                self.pstep[k] += d


class Adam(torch.optim.Optimizer):
    """Fused Adam.  max_grad_norm (positive) clips the global gradient norm -- over every parameter of every group that
    has a gradient, after grad_scale, torch.nn.utils.clip_grad_norm_'s formula; skip_nonfinite leaves parameters, moments
    and the step count untouched by a step whose gradient holds a NaN or an Inf.  Clipping alone does not change what a
    non-finite gradient does: without skip_nonfinite such a step is applied exactly as an unguarded one would apply it.
    Either option makes the optimizer a CAPTURABLE one (capturable=True is implied): a skipped step must not advance the
    step count and the host must not read the device to find out, so the count has to live on the device.  Both options
    are launch arguments: a captured graph holds the values of its capture, changing them afterwards needs a new capture.
    The guard protects parameters, moments and the step count; a forward that was itself non-finite has already written its
    BatchNorm running statistics.

    ema_decay (0 < d < 1) keeps an exponential moving average of the weights: avg += w_t (p - avg) after every APPLIED update
    t = 1, 2, ... of a parameter, w_t = 1 - min(d, (1 + t) / (10 + t)) (the warm-up of timm's ModelEmaV2 / torch's
    swa_utils), avg = p before the first update.  A step the guard skips leaves the average alone, a parameter without a
    gradient keeps its own.  Like the guard it implies capturable=True (t is the device's step count).  swap_averaged() /
    averaged_weights() exchange weights and averages in place; buffers (BatchNorm running statistics) are not averaged.

    micro_batches (an attribute, default 1; a host-side integer set between steps): the gradients hold the sum of that many
    micro-batch gradients (backwards without zero_grad), and the update kernels and the guard's norm see
    grad_scale / micro_batches -- computed in double, rounded to float32 once -- where they see grad_scale today.  A factor of
    its own because distributed.sync_gradients() overwrites grad_scale on every call.  The guard and the average stay per
    UPDATE: one norm over the mean gradient, one decision, one count, one average update per group.  A NaN or an Inf in any
    micro-batch's gradient stays in the sum, so with skip_nonfinite the WHOLE group's update is skipped.  It describes the
    step being taken, not the run: state_dict() does not carry it.  Like every hyper-parameter of the capturable path it is
    pushed to the device when it changes, which is refused inside a graph capture.

    segmented: an arena shared by several param groups, or holding parameters with requires_grad = False, is updated by the
    chunk-mapped kernels (gdn_adam_step_seg, gdn_grad_sumsq_seg, gdn_ema_update_seg) in the same number of launches as an
    arena one group covers -- without it such an arena takes one launch per tensor.  Every parameter of the arena must be in
    a param group; freezing is requires_grad = False.  Implies capturable=True (one device step state per group).  The plan
    of an arena -- chunk map, group table, step states -- follows (param group, requires_grad) of its parameters and is
    rebuilt when they change, which is refused inside a graph capture.  A step in which a trainable parameter has no
    gradient, or whose parameters have taken different numbers of updates, runs per tensor, as the one-launch path hands
    over.  Each result is bit-identical to the per-tensor update of the same slice with the same group's records.

    A param group may carry 'lr_mult' (default 1; never written into the defaults, so a state_dict() without it is what it
    was): the kernels see lr * lr_mult, in double, rounded to float32 once -- a schedule that writes group['lr'] leaves the
    multipliers alone.

    schedule ({'kind': 'constant' | 'linear' | 'cosine', 'warmup': W, 'total': T, 'floor': F}): the rate of
    every update is set on the device from the device's own update count u (0 for the first update): lr * lr_mult * s(u),
    s(u) = (u + 1) / W during the first W updates, then 1 (constant) or a linear / cosine decay from 1 to F at update T, F from
    then on.  One gdn_lr_schedule launch per arena in front of the update writes it into the hyper-parameter table; the host
    pushes nothing per step, so captured graphs replay it.  Implies capturable=True.  A skipped step does not advance u.
    Code that writes group['lr'] (the reference's decay) still works: the base rate is pushed when it changes, outside a
    capture.  current_lr() reads the rates the last update used.  state_dict()['gdn']['schedule'] carries the four values
    and load_state_dict() refuses another schedule.

    decoupled (optimizer-wide): the groups' weight_decay is torch.optim.AdamW's -- it stays out of the gradient
    and the moments, and the weight loses float32(rate * weight_decay) * p with the Adam term in one subtraction, `rate` being
    the update's own (after lr_mult and the schedule).  Every update path calls the gdn_adamw_step* entry point in its
    sibling's place: the same launches, the same records.  A parameter without a gradient, a frozen chunk and a step the
    guard skips are not decayed.  It does not imply capturable.  state_dict()['gdn'] carries 'decoupled': True only when it
    is on, and load_state_dict() refuses a 'gdn' state of the other kind: the groups' weight_decay comes from the checkpoint
    and would silently change its meaning.  A dict without a 'gdn' key (torch.optim.Adam, torch.optim.AdamW) loads as ever."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None, segmented=False, schedule=None,
                 decoupled=False):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive (None: no clipping), got %r" % (max_grad_norm,))
        if ema_decay is not None and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError("ema_decay must lie in (0, 1) (None: no weight average), got %r" % (ema_decay,))
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._stores = {}      # id(arena) or id(loose param) -> _Store, made by the first step that updates it
        self.grad_scale = 1.0  # set to 1/world_size by the data-parallel wrapper
        self.micro_batches = 1  # gradient accumulation: the gradients hold the sum of this many micro-batches (see the class)
        # capturable: the step counter, beta^t and the hyper-parameters live in device memory (gdn_adam_step_dev), so
        # step() can be captured in a hipGraph and replayed; call refresh_hyper() after changing lr outside a capture
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.segmented = bool(segmented)
        self.schedule = check_schedule(schedule)
        self.decoupled = bool(decoupled)
        self.capturable = bool(capturable) or self.guarded or self.ema_decay is not None or self.segmented or \
            self.schedule is not None
        for g in self.param_groups:
            if not float(g.get("lr_mult", 1.0)) >= 0.0:
                raise ValueError("lr_mult must not be negative, got %r" % (g["lr_mult"],))
        # guarded: step() gathers its launches in _work, then runs the norm pass, the decision and the updates; _guard is
        # the device record (made by the first step)
        self._work, self._guard = None, None
        self._parked = _Parked()       # a loaded checkpoint, until the stores it belongs to exist
        # _swapped while the weights and the averages have changed places
        self._swapped, self._ema_told = False, False

    def store_of(self, owner):
        """The state store of an arena or of a loose parameter; None before the first step that updates it."""
        return self._stores.get(id(owner))

    def _scale(self):
        """The gradient scale the kernels see, in double: they round it to float32 once."""
        k = int(self.micro_batches)
        if k < 1:
            raise ValueError("micro_batches must be a positive integer, got %r" % (self.micro_batches,))
        return float(self.grad_scale) if k == 1 else float(self.grad_scale) / k

    def refresh_hyper(self):
        """Push (lr, betas, eps, weight_decay, grad_scale / micro_batches) to the device buffers of the capturable path if they changed."""
        for st in self._stores.values():
            for table in (st.table, st.plan):
                if table is not None and table.param_groups is not None:
                    self._push_hyper(table)

    def _hyper_vals(self, group):
        return (_lr(group), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                float(group["weight_decay"]), self._scale())

    def _push_hyper(self, table):
        """The rows of a table from their param groups, every row with the optimizer's one gradient scale: written when
        the host's copy says they changed, which a graph capture cannot hold."""
        vals = tuple(self._hyper_vals(g) for g in table.param_groups)
        if table.hyper_host != vals:
            _no_capture("optimizer hyper-parameters changed inside a graph capture; call refresh_hyper() before it")
            table.hyper.copy_(torch.tensor(vals, dtype=torch.float32))
            table.hyper_host = vals
        rates = tuple(v[0] for v in vals)
        if self.schedule is not None and table.base_host != rates:
            # the rates the schedule scales, in double; hyper[k][0] above is what the next gdn_lr_schedule launch overwrites
            _no_capture("optimizer learning rate changed inside a graph capture; call refresh_hyper() before it")
            if table.base_lr is None:
                table.put(base_lr=_base_rates(rates, table.hyper.device))
            else:
                table.base_lr.copy_(torch.tensor(rates, dtype=torch.float64))    # in place: captured graphs hold its address
            table.base_host = rates

    def _ensure_dev(self, st, group, steps_taken):
        """Device side of the capturable path for one plain store: its one-row table with the step state; `steps_taken` =
        the host-side count of updates this store has had (a resume folds it in by advancing the powers on the host first)."""
        if st.table is None:
            st.table = _Table(None, 1, st.device)
        table = st.table
        if table.param_groups is None:
            if table.states is None:       # (a loaded checkpoint brings the device's own bytes: _Store.take_record)
                table.put(states=_state_row(_step_state(group, steps_taken, st.device)))
            table.param_groups = [group]
        self._push_hyper(table)

    def _host_update(self, st, group, grad, item=None):
        """One update of the host path, launched now: the whole store with its count, or `item` with that parameter's own."""
        w, m, v, _ = st.ranges(item)
        b1, b2 = group["betas"]
        self._update("")(w, grad, m, v, _lr(group), b1, b2, group["eps"], group["weight_decay"],
                         st.step if item is None else st.pstep[id(item[0])], self._scale())

    def _update(self, form):
        """ops.adam_step<form>, or with decoupled weight decay its sibling ops.adamw_step<form> (looked up per call)."""
        return getattr(ops, ("adamw_step" if self.decoupled else "adam_step") + form)

    def _launch(self, st, grad, row, state, cmap=None, item=None):
        """One capturable update of store `st` (all of it, or `item`) with `grad` in the weights' physical layout, and the
        average's over the same range from the same step state: now, or -- guarded -- gathered until the norm of ALL
        gradients is known.  `row` (a table's row(k)) gives the hyper-parameters and the base rates a schedule scales, `state`
        the step state; under `cmap` the range is a whole arena, `row` the plan itself and `state` its table of states."""
        job = _Launch(*st.ranges(item), grad, row.hyper, state, row.base_lr, cmap)
        if self._work is not None:
            self._work.append(job)
        else:
            self._issue(job, None)

    def _issue(self, job, guard):
        """One gathered update with its average's, under `guard` (None: unguarded).  The schedule launch sits right in
        front of its own update: per-tensor launches of one store share a row of the table."""
        if self.schedule is not None:         # this update's rates from the counts in `state`, written into `hyper`
            s = self.schedule
            ops.lr_schedule(job.hyper, job.base_lr, job.state, s["kind"], s["warmup"], s["total"], s["floor"])
        if job.map is not None:
            self._update("_seg")(job.w, job.grad, job.m, job.v, job.map, job.hyper, job.state, guard)
            if job.ema is not None:
                ops.ema_update_seg(job.ema, job.w, job.map, self.ema_decay, job.state, guard)
            return
        if guard is None:
            self._update("_dev")(job.w, job.grad, job.m, job.v, job.hyper, job.state)
        else:
            self._update("_dev_guarded")(job.w, job.grad, job.m, job.v, job.hyper, job.state, guard)
        if job.ema is not None:
            ops.ema_update(job.ema, job.w, self.ema_decay, job.state, guard)      # the same skip decision

    def _guard_record(self, device):
        if self._guard is None:
            _no_capture("guarded Adam: the guard record would be created (and reset by every replay) inside a graph "
                        "capture; run one eager step first")
            self._guard = _guard_bytes(*(self._parked.guard or (0, 0, 0))).to(device)
            self._parked.guard = None
        elif self._guard.device != device:
            raise GdnError("guarded Adam: parameters on %s and %s; one gradient norm needs one device" % (self._guard.device, device))
        return self._guard

    def _guarded_updates(self):
        """The two passes of a guarded step over the gathered launches: sum of squares of every gradient into the record
        and the decision; then every update under that decision."""
        work, self._work = self._work, None
        if not work:
            return
        guard = self._guard_record(work[0].w.device)
        for k, job in enumerate(work):
            if job.w.device != guard.device:
                raise GdnError("guarded Adam: parameters on %s and %s; one gradient norm needs one device" % (guard.device, job.w.device))
            if job.map is None:
                ops.grad_sumsq(job.grad, guard, accumulate=k > 0)
            else:
                ops.grad_sumsq_seg(job.grad, job.map, guard, accumulate=k > 0)      # frozen chunks are not read
        # (the decision reads the gradient scale alone, which every row of a table carries)
        ops.grad_guard_finalize(guard, work[0].hyper, self.max_grad_norm or 0.0, self.skip_nonfinite)
        for job in work:
            self._issue(job, guard)

    def guard_stats(self):
        """{'norm', 'coef', 'steps', 'clipped', 'skipped'} of the guard: norm and coefficient of the last step, counts over
        the run.  One small device-to-host copy, i.e. a sync: for print cadence, not for every step; not inside a capture."""
        if not self.guarded:
            raise GdnError("guard_stats(): this optimizer has no gradient guard (max_grad_norm / skip_nonfinite)")
        _no_capture("optimizer guard_stats() inside a graph capture")
        if self._guard is None:
            steps, clipped, skipped = self._parked.guard or (0, 0, 0)
            return {"norm": 0.0, "coef": 1.0, "steps": steps, "clipped": clipped, "skipped": skipped}
        _, norm, coef, _, steps, clipped, skipped = _unpack(_GUARD_FMT, self._guard)
        return {"norm": norm, "coef": coef, "steps": steps, "clipped": clipped, "skipped": skipped}

    def current_lr(self):
        """The float32 rates the last update used, one per param group, as the kernels read them from the device table:
        with a schedule what gdn_lr_schedule wrote, without one float32(lr * lr_mult).  None for a group no update has
        reached yet (or whose parameters are all frozen).  A small device-to-host copy per table, i.e. a sync: for print
        cadence, not for every step; not inside a capture."""
        if not self.capturable:
            raise GdnError("current_lr(): the rates of this optimizer are launch arguments, not device memory (capturable)")
        _no_capture("optimizer current_lr() inside a graph capture")
        out = [None] * len(self.param_groups)
        index = {id(g): gi for gi, g in enumerate(self.param_groups)}
        for st in self._stores.values():
            table = st.plan if st.plan is not None else st.table
            if table is None or table.param_groups is None:
                continue
            rows = [(k, index[id(g)]) for k, g in enumerate(table.param_groups) if out[index[id(g)]] is None]
            if rows:
                rates = table.hyper[:, 0].cpu().tolist()
                for k, gi in rows:
                    out[gi] = rates[k]
        return out

    def log_records(self, arena):
        """(hyper row, step state, guard record) of param group 0 in `arena`'s store, as the device tensors the update kernels
        read -- what ops.step_record copies into the training log; None for each record this optimizer does
        not keep on the device (a host-stepped optimizer keeps none, an unguarded one no guard record), or before the first
        step made it.  No device work, no read: safe inside a graph capture."""
        st = None if arena is None else self._stores.get(id(arena))
        if not self.capturable or st is None:
            return None, None, None
        hyper = state = None
        table = st.plan if st.plan is not None else st.table
        if table is not None and table.param_groups is not None:
            k = next((k for k, g in enumerate(table.param_groups) if g is self.param_groups[0]), None)
            if k is not None:
                row = table.row(k)
                hyper, state = row.hyper, row.state
        return hyper, state, self._guard if self.guarded else None

    # ---- weight average ----------------------------------------------------------------------------------------------
    def _ema_views(self):
        """id(param) -> its average as a view in the parameter's logical shape, for every parameter a store averages."""
        return {id(item[0]): st.view(st.ema, item) for st in self._live_stores() if st.ema is not None for item in st.items}

    def averaged(self, p):
        """The average of parameter `p`, in its logical shape: a view of the store's buffer once a step has made it; before
        that what a checkpoint brought for it, else the parameter's own value (avg_0 = p_0).  While swap_averaged() is in
        effect the buffer holds the raw weights instead."""
        if self.ema_decay is None:
            raise GdnError("averaged(): this optimizer keeps no weight average (ema_decay)")
        return self._averaged(p, self._ema_views())

    def _averaged(self, p, views):
        avg = views.get(id(p))
        if avg is None:
            avg = self._parked.averages.get(id(p))
        return avg if avg is not None else p.detach()

    def swap_averaged(self):
        """Exchange weights and averages of every store in place (one launch per store), so the model itself runs on the
        averaged weights -- and back with a second call.  Parameters no step has touched yet have no store: their average is
        their value.  Between the two calls step(), state_dict() and load_state_dict() raise.  Not inside a graph capture."""
        if self.ema_decay is None:
            raise GdnError("swap_averaged(): this optimizer keeps no weight average (ema_decay)")
        _no_capture("optimizer swap_averaged() inside a graph capture")
        if self._parked.averages_wait_for_a_step():
            raise GdnError("swap_averaged(): averages read from a checkpoint are put in place by the first step after "
                           "load_state_dict(); take one step first")
        for st in self._live_stores():
            if st.ema is not None:
                ops.swap_(st.weights, st.ema)
                st.touch()
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def averaged_weights(self):
        """with optimizer.averaged_weights(): the model runs on the averaged weights; the raw ones are back afterwards."""
        self.swap_averaged()
        try:
            yield self
        finally:
            self.swap_averaged()

    def _refuse_swapped(self, what):
        if self._swapped:
            raise GdnError("optimizer %s while weights and averages are exchanged: call swap_averaged() again first" % what)

    # ---- the step ----------------------------------------------------------------------------------------------------
    def _step_per_tensor(self, st, items, table=None, clone=False, group=None):
        """Per-tensor updates ON SLICES OF THE FLAT MOMENTS for those of `items` that have a gradient (torch.optim.Adam
        skips the others), each with the parameter's own step count.  Host path (`group`): the count is a launch argument.
        Capturable path (`table`: the plain store's, or the plan): the step counter is device memory, so a parameter gets a
        device state of its own the first time it runs here -- `clone`: a stream-ordered copy of its row's (no host read),
        else one made on the host for the updates it has taken -- and is updated with its row's hyper-parameters.  The
        arena stays on per-tensor launches from then on (replays advance those counters behind the host's back, so the
        host cannot tell when they are level)."""
        ar = st.arena
        for item in items:
            p, o, n, _ = item
            if p.grad is None:
                continue
            gslice = ar.grad[o:o + n]
            if p.grad.data_ptr() != gslice.data_ptr():
                # a caller-owned gradient: bring it into the parameter's physical (tap-major) order
                gslice = torch.empty_like(p, memory_format=torch.preserve_format).copy_(p.grad)
            st.pstep[id(p)] += 1
            if table is None:
                self._host_update(st, group, gslice, item)
                continue
            k = 0 if table.map is None else table.k_of[id(p)]
            row = table.row(k)
            if id(p) not in st.pdev:
                if clone:
                    _no_capture("capturable Adam: a per-parameter step counter would be created inside a graph capture "
                                "(every replay would reset it); run one eager step with this gradient coverage first")
                    st.pdev[id(p)] = row.state.clone()        # the row's device counter so far
                else:
                    st.pdev[id(p)] = _step_state(table.param_groups[k], st.pstep[id(p)] - 1, st.device)
            self._launch(st, gslice, row, st.pdev[id(p)], item=item)

    def _step_partial(self, st, group):
        """_step_per_tensor for a plain store.  Host path: per-parameter step counts (`pstep`), back to the one-launch
        update once every parameter THAT TAKES GRADIENTS is level again; the capturable path never goes back."""
        if st.pstep is None:
            st.pstep = {id(p): st.step for p, _, _, _ in st.items}
        if self.capturable:
            # the arena's device counter may be copied only if the one-launch path has driven it (then it also holds
            # the updates that graph replays made behind the host's back); when the very first step is already partial, there
            # is no such counter and every parameter starts from its host count
            had_dev = st.full_dev
            self._ensure_dev(st, group, st.step)
            return self._step_per_tensor(st, st.items, st.table, clone=had_dev)
        self._step_per_tensor(st, st.items, group=group)
        counts = {st.pstep[id(p)] for p, _, _, _ in st.items if p.requires_grad}        # (a frozen parameter never levels)
        if len(counts) == 1:              # everyone who steps is level again: back to the one-launch update
            lvl = counts.pop()
            if all(c == lvl for c in st.pstep.values()):
                st.step, st.pstep = lvl, None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._swapped:
            raise GdnError("optimizer.step() while weights and averages are exchanged: call swap_averaged() again first")
        if not self.guarded:
            self._step_groups()
            return loss
        self._work = []
        try:
            self._step_groups()
        except BaseException:
            self._work = None
            raise
        self._guarded_updates()
        return loss

    def _refuse_pending_carry(self, ar):
        if getattr(ar, "carry_reduced", None) is not None:
            # (backward, sync_gradients, backward) under data parallelism leaves the first micro-batch's
            # REDUCED gradient aside until the next sync_gradients() adds it back; stepping now would drop it silently
            raise GdnError("optimizer.step() with an accumulated, already all-reduced gradient pending: call "
                           "sync_gradients() after the last backward of an accumulation")

    def _walk(self):
        """One pass over the param groups, in the order step() updates: ([(group, [(arena, its parameters)], [loose
        parameters])], {id(param): index of its param group} for the parameters of intact arenas, segmented only).
        Unsegmented, one entry per group: its intact arenas in order of first appearance, each with the parameters THIS
        group holds of it.  Segmented, an arena is listed once, where it first appears (its plan reaches every group), with
        the parameters ANY group holds of it, and the loose parameters of all groups follow the arenas.  Either way an arena
        is covered when it is listed with all of its parameters.  (Every step walks every parameter: written for speed.)"""
        per_group, owner, intact, arenas, segmented = [], {}, {}, {}, self.segmented
        for gi, group in enumerate(self.param_groups):
            listed, loose = [], []
            if not segmented:
                arenas = {}
            for p in group["params"]:
                ar = getattr(p, "_gdn_arena", None)
                key = id(ar)
                if ar is None or not (intact[key] if key in intact else intact.setdefault(key, ar.intact())):
                    loose.append(p)
                    continue
                if key in arenas:
                    arenas[key][1].append(p)
                else:
                    arenas[key] = (ar, [p])
                    listed.append(arenas[key])
                if segmented:
                    owner[id(p)] = gi
            per_group.append((group, listed, loose))
        if segmented:
            per_group = [(g, listed, []) for g, listed, _ in per_group] + [(g, [], loose) for g, _, loose in per_group]
        return per_group, owner

    # ---- segmented: every param group of an arena in one launch -----------------------------------------
    def _plan_key(self, ar, owner):
        key = []
        for p, _, _, _ in ar.items:
            if id(p) not in owner:
                raise GdnError("segmented Adam: a parameter of shape %s of the arena is in no param group; pass every "
                               "parameter of the model and freeze with requires_grad = False" % (tuple(p.shape),))
            key.append(owner[id(p)] if p.requires_grad else -1)
        return tuple(key)

    def _build_plan(self, st, key):
        """The plan of store `st` for `key`, with step states that continue the counts the live parameters have: the bytes
        a checkpoint brought for this very key, else a state of the previous plan's for the same param group at the same
        count (graph replays and skipped steps are in it), else the host's powers for that count.  No states (the arena
        runs per tensor) when the live parameters' counts differ or per-parameter states exist already."""
        _no_capture("segmented Adam: the plan of an arena (chunk map, group table, step states) would be built inside a "
                    "graph capture; run one eager step with the same param groups and requires_grad flags first")
        plan = _Plan(st.items, st.arena.numel, key, self.param_groups, st.device)
        old, saved, st.seg_rec = st.plan, st.seg_rec, None
        memo = {}
        counts = {st.count(p, memo) for p, _, _, _ in st.items if id(p) in plan.k_of}
        if len(counts) == 1 and not st.pdev:
            t = counts.pop()
            if saved is not None and tuple(saved["key"]) == plan.key and saved["states"] is not None:
                plan.put(states=saved["states"].to(device=st.device, copy=True))     # the device's own bytes, verbatim
            else:
                rows = []
                for gi in plan.groups:
                    row = None
                    if old is not None and old.states is not None and gi in old.groups:
                        k0 = old.groups.index(gi)
                        if _unpack(_STEP_FMT, old.row(k0).state)[2] == t:   # (a group nobody was left in keeps an older count)
                            row = old.states[_STATE_BYTES * k0:_STATE_BYTES * (k0 + 1)].clone()
                    if row is None:
                        row = _state_row(_step_state(self.param_groups[gi], t, st.device))
                    rows.append(row)
                plan.put(states=torch.cat(rows))
        st.plan = plan
        return plan

    def _step_arena_segmented(self, ar, owner):
        """This step's update of one arena of a segmented optimizer."""
        key = self._plan_key(ar, owner)
        live = [item for item, gi in zip(ar.items, key) if gi >= 0]
        have = sum(item[0].grad is not None for item in live)
        if have == 0:
            return                    # nothing trainable ran backward for this model: skip it, like torch.optim.Adam
        st = self._stores.get(id(ar))
        if st is None:
            st = self._stores[id(ar)] = self._new_store(ar.items, ar)
        if st.pstep is None:          # a segmented store counts per parameter: a frozen one stays where it is
            st.pstep = {id(p): st.step for p, _, _, _ in st.items}
        plan = st.plan if st.plan is not None and st.plan.key == key else self._build_plan(st, key)
        self._push_hyper(plan)
        if plan.states is not None and not st.pdev and have == len(live):
            for p, _, _, _ in live:
                st.pstep[id(p)] += 1
            st.full_dev = True
            self._launch(st, ar.grad, plan, plan.states, plan.map)       # every group in one launch
        else:
            # each parameter's device step state a copy of its group's wherever the plan has states: they were made for, or
            # driven to, the count its live parameters share
            self._step_per_tensor(st, live, plan, clone=plan.states is not None)
        st.step = max(st.pstep.values())
        st.touch()

    def _step_groups(self):
        per_group, owner = self._walk()
        for group, arenas, loose in per_group:
            for ar, ps in arenas:
                self._refuse_pending_carry(ar)
                if self.segmented:
                    self._step_arena_segmented(ar, owner)     # (a parameter of the arena that is in no group is refused there)
                elif len(ps) == len(ar.items):
                    self._step_store(group, ar.items, ar)
                else:
                    loose = loose + ps    # partial coverage: per-tensor launches, as loose stores with moments of their own
            for p in loose:
                self._step_store(group, [(p, 0, p.numel(), None)])

    def _new_store(self, items, arena=None):
        """ONE state store per arena, one per loose parameter, filled with what a checkpoint loaded before it existed
        brought for it."""
        st = _Store(items, arena)
        st.fill(self._parked, self.capturable, self.ema_decay is not None)
        return st

    def _step_store(self, group, items, ar=None):
        """This step's update of one arena (`items` are all of its parameters) or of one loose parameter."""
        have = sum(p.grad is not None for p, _, _, _ in items)
        if have == 0:
            return                    # nothing ran backward for this model: skip it, like torch.optim.Adam
        owner = ar if ar is not None else items[0][0]
        if ar is None and not owner.is_cuda:
            raise GdnError("fused Adam needs GPU parameters: the HIP path has no CPU fallback")
        st = self._stores.get(id(owner))
        if st is None:
            st = self._stores[id(owner)] = self._new_store(items, ar)
        if st.pstep is None and have == len(items):
            st.step += 1
            if ar is not None:
                grad = ar.grad
            else:
                grad = owner.grad
                if grad.stride() != owner.stride():
                    grad = torch.empty_like(owner, memory_format=torch.preserve_format).copy_(grad)
            if self.capturable:
                self._ensure_dev(st, group, st.step - 1)      # (this update is counted already)
                st.full_dev = True        # the store's device counter has taken every update so far: a valid thing to copy
                row = st.table.row(0)
                self._launch(st, grad, row, row.state)
            else:
                self._host_update(st, group, grad)
        else:
            # part of the model got no gradient this step (frozen sub-modules, an unused branch): torch.optim.Adam
            # skips those parameters -- the one-launch update would apply weight decay and stale moments to them.
            # The others are updated per tensor ON SLICES OF THE SAME FLAT MOMENTS with their own step counts, so a
            # parameter never alternates between two sets of moments when coverage changes between steps.
            self._step_partial(st, group)
        st.touch()            # the kernel wrote the parameters behind torch's back: bf16 shadows are stale

    # ---- host counts under a graph (graph.py) --------------------------------------------------------------
    def host_counts(self):
        """The host-side update counts of every store (step() advances them; a capture runs step()'s host code once
        without executing anything, a replay executes it without running the host code)."""
        return [(st,) + st.counts() for st in self._stores.values()]

    def take_back_counts(self, before):
        """Undo what a capture added to the host counts since host_counts() gave `before`; returns it as the per-replay
        increments for count_replay()."""
        return [(st,) + st.take_back(step, pstep) for st, step, pstep in before]

    def count_replay(self, increments):
        for st, dstep, dp in increments:
            st.advance(dstep, dp)

    # ------------------------------------------------------------------------------------------------------------------
    # state exchange: torch.optim.Adam's format ({'state': {index: {'step','exp_avg','exp_avg_sq'}}, 'param_groups'}),
    # moments in each parameter's LOGICAL shape, plus a private 'gdn' key for what that format has no place for
    # ------------------------------------------------------------------------------------------------------------------
    def _live_stores(self):
        """Every store that holds the state of this optimizer's parameters as they are grouped and laid out now, parameters
        in param_groups order within a store."""
        out = []
        for _, arenas, loose in self._walk()[0]:
            for ar, ps in arenas:
                if id(ar) in self._stores and len(ps) == len(ar.items):
                    out.append(self._stores[id(ar)])
                elif not self.segmented:
                    loose = loose + ps
            out.extend(self._stores[id(p)] for p in loose if id(p) in self._stores)
        return out

    def state_dict(self):
        """torch.optim.Adam's state_dict with the real moments (logical shape, contiguous; 'step' a float32 scalar tensor like
        torch's) and a 'gdn' key: host step counts, grad_scale and -- capturable path -- the device step state's bytes."""
        _no_capture("optimizer state_dict() inside a graph capture")
        self._refuse_swapped("state_dict()")
        params = [p for g in self.param_groups for p in g["params"]]
        index = {id(p): k for k, p in enumerate(params)}
        groups = []
        for g in self.param_groups:
            packed = {key: v for key, v in g.items() if key != "params"}
            # the betas the moments were accumulated with: the kernels take them as float32, and 1 - beta2 is where that shows
            # (1 - float32(0.999) is 1.29e-5 below 0.001); an optimizer that goes on from these moments with the rounded
            # values continues the same Adam run to rounding
            packed["betas"] = tuple(_f32(b) for b in g["betas"])
            packed["params"] = [index[id(p)] for p in g["params"]]
            groups.append(packed)

        def entry(step, m, v):
            return {"step": torch.tensor(float(step)), "exp_avg": m.detach().clone(memory_format=torch.contiguous_format),
                    "exp_avg_sq": v.detach().clone(memory_format=torch.contiguous_format)}
        state, recs, memo = {}, [], {}
        for st in self._live_stores():
            for item in st.items:
                count = st.count(item[0], memo)
                if count == 0 and self.segmented and st.arena is not None:
                    continue          # a parameter that never stepped (frozen from the start) has no entry, as in torch
                state[index[id(item[0])]] = entry(count, st.view(st.m, item), st.view(st.v, item))
            recs.append(st.record(index))
        # loaded, but no step since: hand back what was loaded
        for pid, s in self._parked.moments.items():
            if pid in index and index[pid] not in state:
                state[index[pid]] = entry(s["step"], s["m"], s["v"])
        for rec in self._parked.records.values():
            recs.append(dict(rec, params=[index[i] for i in rec["params"]],
                             pdev={index[i]: t for i, t in rec["pdev"].items()}))
        priv = {"version": 1, "capturable": self.capturable, "grad_scale": float(self.grad_scale), "stores": recs}
        if self.guarded:
            gs = self.guard_stats()
            priv["guard"] = {"max_grad_norm": self.max_grad_norm, "skip_nonfinite": self.skip_nonfinite,
                             "steps": gs["steps"], "clipped": gs["clipped"], "skipped": gs["skipped"]}
        if self.schedule is not None:
            priv["schedule"] = dict(self.schedule)
        if self.decoupled:
            priv["decoupled"] = True
        if self.ema_decay is not None:
            # every parameter, so the averaged model can be put together from this key alone (no update yet: avg_0 = p_0)
            views = self._ema_views()
            priv["ema"] = {"decay": self.ema_decay,
                           "avg": {index[id(p)]: self._averaged(p, views).detach().clone(memory_format=torch.contiguous_format)
                                   for p in params}}
        return {"state": dict(sorted(state.items())), "param_groups": groups, "gdn": priv}

    def load_state_dict(self, state_dict):
        """Restore a state_dict() of this class or of torch.optim.Adam over the same parameters (count and shapes are
        checked).  Works before the first step: what was read waits until its store exists.  A store that exists already is
        rewritten in place, moments in the arena's physical layout.  With the 'gdn' key of a capturable optimizer the
        device step state is restored byte for byte; without it (a torch checkpoint) it is recomputed on the host from
        'step'.  Hyper-parameters of the groups are taken from the checkpoint (betas only if they differ in float32).  Not inside a graph capture; a graph captured
        before the load still holds the old device step state -- capture after loading."""
        _no_capture("optimizer load_state_dict() inside a graph capture")
        self._refuse_swapped("load_state_dict()")
        if "gdn" in state_dict:
            # (a torch.optim.Adam checkpoint has no such key and says nothing about a schedule)
            theirs = check_schedule((state_dict["gdn"] or {}).get("schedule"))
            if theirs != self.schedule:
                raise GdnError("optimizer state written under the learning-rate schedule %r loaded into an optimizer with the "
                               "schedule %r: the update counts it carries would mean other rates" % (theirs, self.schedule))
            theirs = bool((state_dict["gdn"] or {}).get("decoupled", False))
            if theirs != self.decoupled:
                kinds = ("coupled (Adam, L2)", "decoupled (AdamW)")
                raise GdnError("optimizer state written under %s weight decay loaded into an optimizer with %s weight decay: "
                               "the weight_decay its param groups carry would mean another update" %
                               (kinds[theirs], kinds[self.decoupled]))
        groups = state_dict["param_groups"]
        mine = [len(g["params"]) for g in self.param_groups]
        theirs = [len(g["params"]) for g in groups]
        if mine != theirs:
            raise GdnError("optimizer state for %d parameters in groups %s loaded into an optimizer with %d parameters in "
                           "groups %s" % (sum(theirs), theirs, sum(mine), mine))
        params = [p for g in self.param_groups for p in g["params"]]
        by_saved = dict(zip([i for g in groups for i in g["params"]], params))
        parked = _Parked(self._parked.guard)
        for key, s in state_dict["state"].items():
            p = by_saved.get(key)
            if p is None:
                raise GdnError("optimizer state entry %r belongs to no parameter of the checkpoint's param_groups" % (key,))
            for name in ("exp_avg", "exp_avg_sq"):
                if tuple(s[name].shape) != tuple(p.shape):
                    raise GdnError("optimizer state %r of parameter %r has shape %s, the parameter has %s" %
                                   (name, key, tuple(s[name].shape), tuple(p.shape)))
            parked.moments[id(p)] = {"step": int(round(float(s["step"]))), "m": s["exp_avg"].detach(), "v": s["exp_avg_sq"].detach()}
        for g, saved in zip(self.param_groups, groups):
            for key, v in saved.items():
                if key == "betas":
                    # betas that round to this optimizer's own in float32 are the same to the kernels: keep the own spelling (the
                    # capturable path computes its host-side powers from it, as the uninterrupted run does)
                    if [_f32(b) for b in v] != [_f32(b) for b in g["betas"]]:
                        g["betas"] = tuple(v)
                elif key != "params":
                    g[key] = v
        priv = state_dict.get("gdn") or {}
        self.grad_scale = float(priv.get("grad_scale", self.grad_scale))
        for rec in priv.get("stores", []):
            ids = [id(by_saved[i]) for i in rec["params"] if i in by_saved]
            if len(ids) != len(rec["params"]) or not ids:
                continue
            parked.records[ids[0]] = dict(rec, params=ids, pdev={id(by_saved[i]): t for i, t in rec["pdev"].items()})
        if self.guarded and priv.get("guard") is not None:
            # the run's counts go on; max_grad_norm / skip_nonfinite stay this optimizer's own (constructor arguments)
            parked.guard = tuple(int(priv["guard"][k]) for k in ("steps", "clipped", "skipped"))
            if self._guard is not None:
                self._guard.copy_(_guard_bytes(*parked.guard))
                parked.guard = None
        # the averages (ema_decay stays the constructor's): parked like the moments; an optimizer without ema_decay ignores them
        if self.ema_decay is not None:
            saved = (priv.get("ema") or {}).get("avg")
            if saved is None:
                if not self._ema_told and _rank0():
                    print("optimizer state holds no weight average: the average starts from the loaded weights")
                self._ema_told = True
            else:
                for key, a in saved.items():
                    p = by_saved.get(key)
                    if p is None:
                        raise GdnError("weight average %r belongs to no parameter of the checkpoint's param_groups" % (key,))
                    if tuple(a.shape) != tuple(p.shape):
                        raise GdnError("weight average of parameter %r has shape %s, the parameter has %s" %
                                       (key, tuple(a.shape), tuple(p.shape)))
                    parked.averages[id(p)] = a.detach()
        self._parked = parked
        # stores that exist: rewrite them now; parameters without a saved state start over
        for st in self._live_stores():
            st.fill(parked, self.capturable, self.ema_decay is not None, reset=True)
        for p in params:
            ar = getattr(p, "_gdn_arena", None)
            if ar is not None:
                ar.touch()


class AdamW(Adam):
    """Adam(..., decoupled=True) with torch.optim.AdamW's defaults: weight_decay 1e-2, decoupled from the gradient."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **kw):
        if not kw.pop("decoupled", True):
            raise ValueError("AdamW is the decoupled optimizer; Adam(decoupled=False) is the coupled one")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=True, **kw)
