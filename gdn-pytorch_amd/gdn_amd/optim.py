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
"""
import contextlib
import struct

import torch

from . import ops
from ._lib import GdnError


_GUARD_FMT = "<dffiiii"      # gdn_hip.h: { double sumsq; float norm, coef; int32 skip, steps, clipped, skipped; }


def _rank0():
    return not (torch.distributed.is_available() and torch.distributed.is_initialized()) or torch.distributed.get_rank() == 0


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
    averaged_weights() exchange weights and averages in place; buffers (BatchNorm running statistics) are not averaged."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive (None: no clipping), got %r" % (max_grad_norm,))
        if ema_decay is not None and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError("ema_decay must lie in (0, 1) (None: no weight average), got %r" % (ema_decay,))
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._flat = {}        # id(arena) -> {"m","v","step"}
        self.grad_scale = 1.0  # set to 1/world_size by the data-parallel wrapper
        # capturable: the step counter, beta^t and the hyper-parameters live in device memory (gdn_adam_step_dev), so
        # step() can be captured in a hipGraph and replayed; call refresh_hyper() after changing lr outside a capture
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.capturable = bool(capturable) or self.guarded or self.ema_decay is not None
        # guarded: step() gathers its launches in _work, then runs the norm pass, the decision and the updates; _guard is
        # the device record (made by the first step), _guard_counts what load_state_dict() read for it before it existed
        self._work, self._guard, self._guard_counts = None, None, None
        # load_state_dict() parks what it read here until the store it belongs to exists (the arena is built by the first
        # forward, the stores by the first step): id(param) -> {"step","m","v"} in LOGICAL layout, and the device step state
        # of the capturable path per store, keyed by the store's first parameter
        self._pending, self._pending_dev = {}, {}
        # weight average: one flat buffer "ema" per state store beside m and v, made by the first step; _pending_ema is what
        # load_state_dict() read for it (id(param) -> average in LOGICAL layout) until then; _swapped while the weights
        # and the averages have changed places
        self._pending_ema, self._swapped, self._ema_told = {}, False, False

    def refresh_hyper(self):
        """Push (lr, betas, eps, weight_decay, grad_scale) to the device buffers of the capturable path if they changed."""
        for group in self.param_groups:
            for st in list(self._flat.values()) + [self.state[p] for p in group["params"] if p in self.state]:
                if "hyper" in st and st.get("group") is group:
                    self._push_hyper(st, group)

    def _push_hyper(self, st, group):
        vals = (float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                float(group["weight_decay"]), float(self.grad_scale))
        if st.get("hyper_host") != vals:
            if torch.cuda.is_current_stream_capturing():
                raise GdnError("optimizer hyper-parameters changed inside a graph capture; call refresh_hyper() before it")
            st["hyper"].copy_(torch.tensor(vals, dtype=torch.float32))
            st["hyper_host"] = vals

    def _arena_groups(self, group):
        """Split a param group into (arena, covers_whole_arena) and stragglers."""
        arenas, loose = {}, []
        for p in group["params"]:
            ar = getattr(p, "_gdn_arena", None)
            if ar is not None and ar.intact():
                arenas.setdefault(id(ar), (ar, []))[1].append(p)
            else:
                loose.append(p)
        return arenas, loose

    @staticmethod
    def _dev_state(group, t, device):
        """{double beta1^t, double beta2^t, int32 t, float bc1, float bc2s} for `t` steps TAKEN so far (the kernel advances it
        before it uses it)."""
        import struct
        if torch.cuda.is_current_stream_capturing():
            raise GdnError("capturable Adam: a device step counter would be created (and reset by every replay) inside a graph "
                           "capture; run one eager step with the same gradient coverage first")
        b1, b2 = group["betas"]
        raw = struct.pack("<ddiff", float(b1) ** t, float(b2) ** t, t, 0.0, 0.0)
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)

    def _ensure_dev(self, st, group, device, steps_taken):
        """Device-side step state of the capturable path for one state store: hyper float32[6] and the step state of
        _dev_state(); `steps_taken` = the host-side count of updates this store has had (a resume folds it in by advancing the
        powers on the host first)."""
        if "hyper" not in st:
            st["hyper"] = torch.zeros(6, dtype=torch.float32, device=device)
            if "state" not in st:          # (a loaded checkpoint brings the device's own bytes: _fill_arena / _fill_loose)
                st["state"] = self._dev_state(group, steps_taken, device)
            st["group"] = group
        self._push_hyper(st, group)

    def _apply(self, pdata, grad, st, group, device):
        b1, b2 = group["betas"]
        if self.capturable:
            self._ensure_dev(st, group, device, st["step"] - 1)      # (step() has counted this update already)
            st["full_dev"] = True         # the store's device counter has taken every update so far: a valid thing to copy
            self._launch_dev(pdata, grad, st["m"], st["v"], st["hyper"], st["state"], st.get("ema"))
        else:
            ops.adam_step(pdata, grad, st["m"], st["v"], group["lr"], b1, b2, group["eps"], group["weight_decay"],
                          st["step"], self.grad_scale)

    def _launch_dev(self, pdata, grad, m, v, hyper, state, ema=None):
        """One capturable update: launched now, or -- guarded -- gathered until the norm of ALL gradients is known.  `ema`:
        the slice of the weight average that belongs to `pdata`, updated right after it from the same step state."""
        if self._work is None:
            ops.adam_step_dev(pdata, grad, m, v, hyper, state)
            if ema is not None:
                ops.ema_update(ema, pdata, self.ema_decay, state)
        else:
            self._work.append((pdata, grad, m, v, hyper, state, ema))

    def _guard_record(self, device):
        if self._guard is None:
            if torch.cuda.is_current_stream_capturing():
                raise GdnError("guarded Adam: the guard record would be created (and reset by every replay) inside a graph "
                               "capture; run one eager step first")
            steps, clipped, skipped = self._guard_counts or (0, 0, 0)
            raw = struct.pack(_GUARD_FMT, 0.0, 0.0, 1.0, 0, steps, clipped, skipped)
            self._guard = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
            self._guard_counts = None
        elif self._guard.device != device:
            raise GdnError("guarded Adam: parameters on %s and %s; one gradient norm needs one device" % (self._guard.device, device))
        return self._guard

    def _guarded_updates(self):
        """The two passes of a guarded step over the gathered launches: sum of squares of every gradient into the record
        and the decision; then every update under that decision."""
        work, self._work = self._work, None
        if not work:
            return
        guard = self._guard_record(work[0][0].device)
        for k, w in enumerate(work):
            if w[0].device != guard.device:
                raise GdnError("guarded Adam: parameters on %s and %s; one gradient norm needs one device" % (guard.device, w[0].device))
            ops.grad_sumsq(w[1], guard, accumulate=k > 0)
        ops.grad_guard_finalize(guard, work[0][4], self.max_grad_norm or 0.0, self.skip_nonfinite)
        for pdata, grad, m, v, hyper, state, ema in work:
            ops.adam_step_dev_guarded(pdata, grad, m, v, hyper, state, guard)
            if ema is not None:
                ops.ema_update(ema, pdata, self.ema_decay, state, guard)      # the same skip decision

    def guard_stats(self):
        """{'norm', 'coef', 'steps', 'clipped', 'skipped'} of the guard: norm and coefficient of the last step, counts over
        the run.  One small device-to-host copy, i.e. a sync: for print cadence, not for every step; not inside a capture."""
        if not self.guarded:
            raise GdnError("guard_stats(): this optimizer has no gradient guard (max_grad_norm / skip_nonfinite)")
        self._refuse_capture("guard_stats()")
        if self._guard is None:
            steps, clipped, skipped = self._guard_counts or (0, 0, 0)
            return {"norm": 0.0, "coef": 1.0, "steps": steps, "clipped": clipped, "skipped": skipped}
        _, norm, coef, _, steps, clipped, skipped = struct.unpack(_GUARD_FMT, self._guard.cpu().numpy().tobytes())
        return {"norm": norm, "coef": coef, "steps": steps, "clipped": clipped, "skipped": skipped}

    # ---- weight average ----------------------------------------------------------------------------------------------
    def _ensure_ema(self, st, weights, ar, p=None):
        """The average of one store, made by its first step as a copy of the weights BEFORE that step's update (avg_0 = p_0,
        same physical layout), then overwritten with what load_state_dict() read for it."""
        if self.ema_decay is None or "ema" in st:
            return
        if torch.cuda.is_current_stream_capturing():
            raise GdnError("Adam(ema_decay): the weight average would be created inside a graph capture; run one eager step "
                           "with the same gradient coverage first")
        st["ema"] = weights.detach().clone(memory_format=torch.preserve_format)
        if ar is None:
            avg = self._pending_ema.pop(id(p), None)
            if avg is not None:
                st["ema"].copy_(avg)
            return
        for q, o, n, tr in ar.items:
            avg = self._pending_ema.pop(id(q), None)
            if avg is not None:
                ar._view(st["ema"], o, q.shape, tr).copy_(avg)

    def _ema_views(self):
        """id(param) -> its average as a view in the parameter's logical shape, for every parameter a store averages."""
        out = {}
        for kind, st, ar, ps in self._stores():
            if "ema" not in st:
                continue
            if kind == "arena":
                for p, o, n, tr in ar.items:
                    out[id(p)] = ar._view(st["ema"], o, p.shape, tr)
            else:
                out[id(ps[0])] = st["ema"]
        return out

    def averaged(self, p):
        """The average of parameter `p`, in its logical shape: a view of the store's buffer once a step has made it; before
        that what a checkpoint brought for it, else the parameter's own value (avg_0 = p_0).  While swap_averaged() is in
        effect the buffer holds the raw weights instead."""
        if self.ema_decay is None:
            raise GdnError("averaged(): this optimizer keeps no weight average (ema_decay)")
        v = self._ema_views().get(id(p))
        if v is not None:
            return v
        avg = self._pending_ema.get(id(p))
        return avg if avg is not None else p.detach()

    def swap_averaged(self):
        """Exchange weights and averages of every store in place (one launch per store), so the model itself runs on the
        averaged weights -- and back with a second call.  Parameters no step has touched yet have no store: their average is
        their value.  Between the two calls step(), state_dict() and load_state_dict() raise.  Not inside a graph capture."""
        if self.ema_decay is None:
            raise GdnError("swap_averaged(): this optimizer keeps no weight average (ema_decay)")
        self._refuse_capture("swap_averaged()")
        if any(pid in self._pending for pid in self._pending_ema):
            # (a parameter that never took a step has no moments waiting either: its average is its value)
            raise GdnError("swap_averaged(): averages read from a checkpoint are put in place by the first step after "
                           "load_state_dict(); take one step first")
        for kind, st, ar, ps in self._stores():
            if "ema" not in st:
                continue
            ops.swap_(ar.data if kind == "arena" else ps[0].data, st["ema"])
            arena = ar if kind == "arena" else getattr(ps[0], "_gdn_arena", None)
            if arena is not None:
                arena.touch()     # the weights changed behind torch's back: bf16 shadow, eval-BatchNorm coefficients
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

    def _step_partial(self, ar, st, group):
        """Per-tensor updates ON SLICES OF THE FLAT MOMENTS for the parameters that have a gradient (torch.optim.Adam skips
        the others).  Host path: per-parameter step counts (`pstep`), back to the one-launch update once every parameter
        THAT TAKES GRADIENTS is level again.  Capturable path: the step counter is device memory, so each parameter gets a
        device state of its own -- a stream-ordered copy of the arena's when the one-launch path ran before -- and the
        arena stays on per-tensor launches from then on (replays advance those counters behind the host's back, so the
        host cannot tell when they are level)."""
        if st["pstep"] is None:
            st["pstep"] = {id(p): st["step"] for p, _, _, _ in ar.items}
        b1, b2 = group["betas"]
        if self.capturable:
            # the arena's device counter may be copied only if the one-launch path has driven it (then it also holds
            # the updates that graph replays made behind the host's back); when the very first step is already partial, there
            # is no such counter and every parameter starts from its host count
            had_dev = bool(st.get("full_dev"))
            self._ensure_dev(st, group, ar.device, st["step"])
            pdev = st.setdefault("pdev", {})
        for p, o, n, tr in ar.items:
            if p.grad is None:
                continue
            g = p.grad
            gslice = ar.grad[o:o + n]
            if g.data_ptr() != gslice.data_ptr():
                # a caller-owned gradient: bring it into the parameter's physical (tap-major) order
                gslice = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g)
            st["pstep"][id(p)] += 1
            if self.capturable:
                ds = pdev.get(id(p))
                if ds is None:
                    if had_dev:
                        if torch.cuda.is_current_stream_capturing():
                            raise GdnError("capturable Adam: a per-parameter step counter would be created inside a graph capture "
                                           "(every replay would reset it); run one eager step with this gradient coverage first")
                        ds = st["state"].clone()          # the arena's device counter so far (no host read)
                    else:
                        ds = self._dev_state(group, st["pstep"][id(p)] - 1, ar.device)
                    pdev[id(p)] = ds
                self._launch_dev(ar.data[o:o + n], gslice, st["m"][o:o + n], st["v"][o:o + n], st["hyper"], ds,
                                 st["ema"][o:o + n] if "ema" in st else None)
            else:
                ops.adam_step(ar.data[o:o + n], gslice, st["m"][o:o + n], st["v"][o:o + n], group["lr"], b1, b2, group["eps"],
                              group["weight_decay"], st["pstep"][id(p)], self.grad_scale)
        if self.capturable:
            return
        counts = {st["pstep"][id(p)] for p, _, _, _ in ar.items if p.requires_grad}     # (a frozen parameter never levels)
        if len(counts) == 1:              # everyone who steps is level again: back to the one-launch update
            lvl = counts.pop()
            if all(st["pstep"][id(p)] == lvl for p, _, _, _ in ar.items):
                st["step"], st["pstep"] = lvl, None

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

    def _step_groups(self):
        for group in self.param_groups:
            b1, b2 = group["betas"]
            arenas, loose = self._arena_groups(group)
            for ar, ps in arenas.values():
                if getattr(ar, "carry_reduced", None) is not None:
                    # (backward, sync_gradients, backward) under data parallelism leaves the first micro-batch's
                    # REDUCED gradient aside until the next sync_gradients() adds it back; stepping now would drop it silently
                    raise GdnError("optimizer.step() with an accumulated, already all-reduced gradient pending: call "
                                   "sync_gradients() after the last backward of an accumulation")
                if len(ps) != len(ar.items):
                    loose.extend(ps)      # partial coverage: fall back to per-tensor launches
                    continue
                if all(p.grad is None for p in ps):
                    continue              # nothing ran backward for this model: skip it, like torch.optim.Adam
                st = self._flat.get(id(ar))
                if st is None:
                    # ONE state store per arena: flat moments; `pstep` is None while every parameter has taken the same
                    # number of steps (st["step"]) and becomes a per-parameter count once coverage has been partial
                    st = {"m": ops.zeros((ar.numel,), ar.device), "v": ops.zeros((ar.numel,), ar.device), "step": 0,
                          "pstep": None}
                    self._flat[id(ar)] = st
                    self._fill_arena(ar, st)          # a checkpoint loaded before this store existed
                self._ensure_ema(st, ar.data, ar)
                if st["pstep"] is None and all(p.grad is not None for p in ps):
                    st["step"] += 1
                    self._apply(ar.data, ar.grad, st, group, ar.device)
                else:
                    # part of the model got no gradient this step (frozen sub-modules, an unused branch): torch.optim.Adam
                    # skips those parameters -- the one-launch update would apply weight decay and stale moments to them.
                    # The others are updated per tensor ON SLICES OF THE SAME FLAT MOMENTS with their own step counts, so a
                    # parameter never alternates between two sets of moments when coverage changes between steps.
                    self._step_partial(ar, st, group)
                ar.touch()        # the kernel wrote the parameters behind torch's back: bf16 shadows are stale
            for p in loose:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise GdnError("fused Adam needs GPU parameters: the HIP path has no CPU fallback")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["m"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["v"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    self._fill_loose(p, st)
                self._ensure_ema(st, p.data, None, p)
                st["step"] += 1
                g = p.grad
                if g.stride() != p.stride():
                    g = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g)
                self._apply(p.data, g, st, group, p.device)
                if getattr(p, "_gdn_arena", None) is not None:
                    p._gdn_arena.touch()

    # ------------------------------------------------------------------------------------------------------------------
    # state exchange: torch.optim.Adam's format ({'state': {index: {'step','exp_avg','exp_avg_sq'}}, 'param_groups'}),
    # moments in each parameter's LOGICAL shape, plus a private 'gdn' key for what that format has no place for
    # ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _refuse_capture(what):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise GdnError("optimizer %s inside a graph capture" % what)

    @staticmethod
    def _f32(x):
        """`x` as the kernels receive it: rounded to float32."""
        import struct
        return struct.unpack("<f", struct.pack("<f", float(x)))[0]

    @staticmethod
    def _dev_count(state):
        """The step count a device step state holds (the int32 after the two doubles of _dev_state)."""
        import struct
        return struct.unpack_from("<i", state.cpu().numpy().tobytes(), 16)[0]

    def _stores(self):
        """(kind, store, arena or None, [params]) for every state store, parameters in param_groups order within a store."""
        out = []
        for group in self.param_groups:
            arenas, loose = self._arena_groups(group)
            for ar, ps in arenas.values():
                st = self._flat.get(id(ar))
                if st is not None and len(ps) == len(ar.items):
                    out.append(("arena", st, ar, [p for p, _, _, _ in ar.items]))
                else:
                    loose.extend(ps)
            for p in loose:
                st = self.state.get(p)
                if st:
                    out.append(("loose", st, None, [p]))
        return out

    def _count(self, st, p, memo):
        """Updates parameter `p` of store `st` has taken: the device's count where the capturable path keeps one (graph
        replays advance it behind the host's back), the host's otherwise."""
        def dev(t):
            if id(t) not in memo:
                memo[id(t)] = self._dev_count(t)
            return memo[id(t)]
        pstep = st.get("pstep")
        if "state" in st:
            if pstep is None:
                return dev(st["state"])
            own = st.get("pdev", {}).get(id(p))
            if own is not None:
                return dev(own)
            if st.get("full_dev"):
                return dev(st["state"])       # no counter of its own yet: the arena's, frozen when coverage split
        return st["step"] if pstep is None else pstep[id(p)]

    def state_dict(self):
        """torch.optim.Adam's state_dict with the real moments (logical shape, contiguous; 'step' a float32 scalar tensor like
        torch's) and a 'gdn' key: host step counts, grad_scale and -- capturable path -- the device step state's bytes."""
        self._refuse_capture("state_dict()")
        self._refuse_swapped("state_dict()")
        index, k = {}, 0
        for g in self.param_groups:
            for p in g["params"]:
                index[id(p)] = k
                k += 1
        groups = []
        for g in self.param_groups:
            packed = {key: v for key, v in g.items() if key != "params"}
            # the betas the moments were accumulated with: the kernels take them as float32, and 1 - beta2 is where that shows
            # (1 - float32(0.999) is 1.29e-5 below 0.001); an optimizer that goes on from these moments with the rounded
            # values continues the same Adam run to rounding
            packed["betas"] = tuple(self._f32(b) for b in g["betas"])
            packed["params"] = [index[id(p)] for p in g["params"]]
            groups.append(packed)
        state, recs, memo = {}, [], {}
        for kind, st, ar, ps in self._stores():
            if kind == "arena":
                views = {id(p): (ar._view(st["m"], o, p.shape, tr), ar._view(st["v"], o, p.shape, tr)) for p, o, n, tr in ar.items}
            else:
                views = {id(ps[0]): (st["m"], st["v"])}
            for p in ps:
                m, v = views[id(p)]
                state[index[id(p)]] = {"step": torch.tensor(float(self._count(st, p, memo))),
                                       "exp_avg": m.detach().clone(memory_format=torch.contiguous_format),
                                       "exp_avg_sq": v.detach().clone(memory_format=torch.contiguous_format)}
            pstep = st.get("pstep")
            recs.append({"kind": kind, "params": [index[id(p)] for p in ps], "step": int(st["step"]),
                         "pstep": None if pstep is None else [int(pstep[id(p)]) for p in ps],
                         "full_dev": bool(st.get("full_dev")),
                         "state": st["state"].detach().cpu().clone() if "state" in st else None,
                         "pdev": {index[id(p)]: st["pdev"][id(p)].detach().cpu().clone() for p in ps
                                  if id(p) in st.get("pdev", {})}})
        # loaded, but no step since: hand back what was loaded
        byid = {id(p): p for g in self.param_groups for p in g["params"]}
        for pid, s in self._pending.items():
            if pid in byid and index[pid] not in state:
                state[index[pid]] = {"step": torch.tensor(float(s["step"])),
                                     "exp_avg": s["m"].detach().clone(memory_format=torch.contiguous_format),
                                     "exp_avg_sq": s["v"].detach().clone(memory_format=torch.contiguous_format)}
        for rec in self._pending_dev.values():
            recs.append(dict(rec, params=[index[i] for i in rec["params"]],
                             pdev={index[i]: t for i, t in rec["pdev"].items()}))
        priv = {"version": 1, "capturable": self.capturable, "grad_scale": float(self.grad_scale), "stores": recs}
        if self.guarded:
            gs = self.guard_stats()
            priv["guard"] = {"max_grad_norm": self.max_grad_norm, "skip_nonfinite": self.skip_nonfinite,
                             "steps": gs["steps"], "clipped": gs["clipped"], "skipped": gs["skipped"]}
        if self.ema_decay is not None:
            # every parameter, so the averaged model can be put together from this key alone
            views = self._ema_views()
            avg = {}
            for g in self.param_groups:
                for p in g["params"]:
                    a = views.get(id(p))
                    if a is None:
                        a = self._pending_ema.get(id(p))
                    if a is None:
                        a = p         # no update yet: avg_0 = p_0
                    avg[index[id(p)]] = a.detach().clone(memory_format=torch.contiguous_format)
            priv["ema"] = {"decay": self.ema_decay, "avg": avg}
        return {"state": dict(sorted(state.items())), "param_groups": groups, "gdn": priv}

    def load_state_dict(self, state_dict):
        """Restore a state_dict() of this class or of torch.optim.Adam over the same parameters (count and shapes are
        checked).  Works before the first step: what was read waits until its store exists.  A store that exists already is
        rewritten in place, moments in the arena's physical layout.  With the 'gdn' key of a capturable optimizer the
        device step state is restored byte for byte; without it (a torch checkpoint) it is recomputed on the host from
        'step'.  Hyper-parameters of the groups are taken from the checkpoint (betas only if they differ in float32).  Not inside a graph capture; a graph captured
        before the load still holds the old device step state -- capture after loading."""
        self._refuse_capture("load_state_dict()")
        self._refuse_swapped("load_state_dict()")
        groups = state_dict["param_groups"]
        mine = [len(g["params"]) for g in self.param_groups]
        theirs = [len(g["params"]) for g in groups]
        if mine != theirs:
            raise GdnError("optimizer state for %d parameters in groups %s loaded into an optimizer with %d parameters in "
                           "groups %s" % (sum(theirs), theirs, sum(mine), mine))
        params = [p for g in self.param_groups for p in g["params"]]
        by_saved = dict(zip([i for g in groups for i in g["params"]], params))
        pending = {}
        for key, s in state_dict["state"].items():
            p = by_saved.get(key)
            if p is None:
                raise GdnError("optimizer state entry %r belongs to no parameter of the checkpoint's param_groups" % (key,))
            for name in ("exp_avg", "exp_avg_sq"):
                if tuple(s[name].shape) != tuple(p.shape):
                    raise GdnError("optimizer state %r of parameter %r has shape %s, the parameter has %s" %
                                   (name, key, tuple(s[name].shape), tuple(p.shape)))
            pending[id(p)] = {"step": int(round(float(s["step"]))), "m": s["exp_avg"].detach(), "v": s["exp_avg_sq"].detach()}
        for g, saved in zip(self.param_groups, groups):
            for key, v in saved.items():
                if key == "betas":
                    # betas that round to this optimizer's own in float32 are the same to the kernels: keep the own spelling (the
                    # capturable path computes its host-side powers from it, as the uninterrupted run does)
                    if [self._f32(b) for b in v] != [self._f32(b) for b in g["betas"]]:
                        g["betas"] = tuple(v)
                elif key != "params":
                    g[key] = v
        priv = state_dict.get("gdn") or {}
        self.grad_scale = float(priv.get("grad_scale", self.grad_scale))
        pending_dev = {}
        for rec in priv.get("stores", []):
            ids = [id(by_saved[i]) for i in rec["params"] if i in by_saved]
            if len(ids) != len(rec["params"]) or not ids:
                continue
            pending_dev[ids[0]] = dict(rec, params=ids, pdev={id(by_saved[i]): t for i, t in rec["pdev"].items()})
        self._pending, self._pending_dev = pending, pending_dev
        if self.guarded and priv.get("guard") is not None:
            # the run's counts go on; max_grad_norm / skip_nonfinite stay this optimizer's own (constructor arguments)
            self._guard_counts = tuple(int(priv["guard"][k]) for k in ("steps", "clipped", "skipped"))
            if self._guard is not None:
                raw = struct.pack(_GUARD_FMT, 0.0, 0.0, 1.0, 0, *self._guard_counts)
                self._guard.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
                self._guard_counts = None
        # the averages (ema_decay stays the constructor's): parked like the moments; an optimizer without ema_decay ignores them
        self._pending_ema = {}
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
                    self._pending_ema[id(p)] = a.detach()
        # stores that exist: rewrite them now; parameters without a saved state start over
        for kind, st, ar, ps in self._stores():
            if kind == "arena":
                self._fill_arena(ar, st, reset=True)
            else:
                self._fill_loose(ps[0], st, reset=True)
            if "ema" in st:
                self._fill_ema(kind, st, ar, ps)
        for p in params:
            ar = getattr(p, "_gdn_arena", None)
            if ar is not None:
                ar.touch()

    def _fill_ema(self, kind, st, ar, ps):
        """Rewrite the average of a store that exists: what load_state_dict() read, through each parameter's own view; the
        weights as they are now where it read nothing."""
        st["ema"].copy_(ar.data if kind == "arena" else ps[0].data)
        items = ar.items if kind == "arena" else [(ps[0], 0, 0, None)]
        for p, o, n, tr in items:
            avg = self._pending_ema.pop(id(p), None)
            if avg is not None:
                (ar._view(st["ema"], o, p.shape, tr) if kind == "arena" else st["ema"]).copy_(avg)

    def _take_dev(self, st, rec, device):
        """Host counts and -- capturable -- the device step state of a store, from its 'gdn' record.  False: no usable record
        (a torch checkpoint, or device counts saved by a capturable optimizer and read by a host-side one), the counts come
        from 'step'."""
        for key in ("hyper", "hyper_host", "state", "pdev", "full_dev", "group"):
            st.pop(key, None)
        if rec is None or (rec.get("state") is not None and not self.capturable):
            return False
        st["step"] = int(rec["step"])
        st["pstep"] = None if rec["pstep"] is None else dict(zip(rec["params"], [int(c) for c in rec["pstep"]]))
        if rec.get("state") is not None:
            st["state"] = rec["state"].to(device=device, copy=True)        # the device's own bytes, verbatim
            st["full_dev"] = bool(rec["full_dev"])
            if rec["pstep"] is not None:
                st["pdev"] = {pid: t.to(device=device, copy=True) for pid, t in rec["pdev"].items()}
        return True

    def _fill_arena(self, ar, st, reset=False):
        """Write what load_state_dict() read for this arena's parameters into its flat store: each moment through the
        parameter's own view of the flat buffer (tap-major for convolution weights), never under a logical shape."""
        ids = [id(p) for p, _, _, _ in ar.items]
        if not reset and not any(i in self._pending for i in ids):
            return
        st["m"].zero_()
        st["v"].zero_()
        counts = {}
        for p, o, n, tr in ar.items:
            s = self._pending.pop(id(p), None)
            counts[id(p)] = s["step"] if s else 0
            if s:
                ar._view(st["m"], o, p.shape, tr).copy_(s["m"])
                ar._view(st["v"], o, p.shape, tr).copy_(s["v"])
        rec = self._pending_dev.pop(ids[0], None)
        if rec is not None and (rec["kind"] != "arena" or rec["params"] != ids):
            rec = None
        if not self._take_dev(st, rec, ar.device):
            level = set(counts.values())
            if len(level) == 1:
                st["step"], st["pstep"] = level.pop(), None
            else:
                st["step"], st["pstep"] = max(level), counts

    def _fill_loose(self, p, st, reset=False):
        s = self._pending.pop(id(p), None)
        if s is None and not reset:
            return
        st["m"].zero_()
        st["v"].zero_()
        st["step"] = s["step"] if s else 0
        if s:
            st["m"].copy_(s["m"])
            st["v"].copy_(s["v"])
        rec = self._pending_dev.pop(id(p), None)
        if rec is not None and (rec["kind"] != "loose" or rec["params"] != [id(p)]):
            rec = None
        self._take_dev(st, rec, p.device)
        st.pop("pstep", None)
