"""Training / validation loops of the hot path on the HIP kernels.

Same entry points and step semantics as the reference's trainer.py
(train_AE_DtoD :331-589, train_AE_RtoD :591-922, validate :17-87): per batch
H2D -> forward -> losses -> zero_grad/backward/step, the hand-rolled LR decay,
the print/checkpoint cadence and the ``module.``-prefixed checkpoint keys.  What
differs by design: losses are fused sync-free HIP kernels, the guide network runs
under no_grad exactly like the reference (latent loss is value-only, F3), data
parallelism is one process per GPU with an RCCL all-reduce of the gradient arena,
and the reference's image/feature-map dumps (and the crashes listed in SURVEY 3.5)
are not reproduced.

Added here without a reference counterpart: exact resume (--resume / --save_state), the --graph replay of the step and
gradient accumulation (--accum_steps K: K loader batches per Adam update).  In the place of the reference's
TensorBoard scalars: --train_log, a per-step record kept on the device and written as JSON lines (trainlog.py).
"""
import os
import time
import typing

import torch

from . import distributed as D
from . import option
from . import tracing
from . import utils as U
from .calculate_error import (ERROR_NAMES, ERROR_NAMES_MAKE3D, ERROR_NAMES_NYU, ERROR_NAMES_STD, compute_errors_device,
                              compute_errors_Make3D_device, compute_errors_NYU_device, compute_errors_std_device,
                              mean_errors_std)


def _is_main():
    return D.rank() == 0


def _averaging(optimizer):
    return getattr(optimizer, "ema_decay", None) is not None


def _save_checkpoint(model, path, optimizer=None):
    """state_dict with the DataParallel ``module.`` prefix the reference's files carry (F9).  With an optimizer that averages
    the weights (--ema_decay) X.pkl is followed by X_ema.pkl: the same file with the averaged weights, written by rank 0 inside
    a swap of its own (buffers -- BatchNorm running statistics -- are the live ones in both)."""
    if not _is_main():
        return
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    sd = {"module." + k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
    torch.save(sd, path)
    if _averaging(optimizer):
        with optimizer.averaged_weights():
            sd = {"module." + k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
        root, ext = os.path.splitext(path)
        torch.save(sd, root + "_ema" + ext)


def _validate_epoch(args, val_loader, model, optimizer, epoch, logger):
    """The per-epoch validation of both training loops; on the averaged weights where the optimizer keeps them.  Returns
    (names, mean errors), numbers already on the host."""
    evaluate = validate_std if option.eval_spec(args)["standard"] else validate       # --eval_protocol standard
    if _averaging(optimizer):
        with optimizer.averaged_weights():
            errors, _, names = evaluate(args, val_loader, model, epoch, logger, args.mode)
    else:
        errors, _, names = evaluate(args, val_loader, model, epoch, logger, args.mode)
    if _is_main():
        print(('(averaged weights)' if _averaging(optimizer) else '') + ' * Avg ' +
              ', '.join('{} : {:.3f}'.format(n, e) for n, e in zip(names, errors)))
    return names, errors


def load_checkpoint(model, path, map_location="cpu"):
    """Load a reference-style (``module.``-prefixed) or bare state_dict."""
    sd = torch.load(path, map_location=map_location)
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    model.load_state_dict(sd)
    return model


# ---------------------------------------------------------------------------------------------------------------------
# resume: everything a run needs to go on bit for bit as if it had never stopped
STATE_FILE = "train_state.pt"
PROGRESS_KEYS = ("epoch", "i", "lr", "model_num", "seen", "step")


def _cpu_copy(x):
    if torch.is_tensor(x):
        return x.detach().to("cpu", copy=True)
    if isinstance(x, dict):
        return {k: _cpu_copy(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_cpu_copy(v) for v in x)
    return x


def training_state(model, optimizer, loader, progress):
    """A plain dict (tensors on the host) of the model's state_dict under bare keys, the optimizer's state_dict
    (optim.Adam: real moments and the device step state), the loader's state of every rank, the torch RNG state and
    `progress`: 'epoch', 'i' (the batch of that epoch the last completed step used; -1: the epoch is about to start),
    'lr', 'model_num', 'seen', 'step' (iterations over the whole run), and 'accum_steps' where the run accumulates
    gradients (--accum_steps > 1; a run without it writes the file it always wrote) and 'schedule' where the device sets the
    learning rate (--warmup_steps / --lr_schedule: the flag and the optimizer's four values).  The guide network of RtoD is frozen and not part
    of it.  Collective under data parallelism: every rank calls it, the loader states are gathered to rank 0, which gets
    the dict; the other ranks get None (weights and moments are identical on all ranks)."""
    i = int(progress.get("i", -1))
    mine = None
    if loader is not None:
        if not hasattr(loader, "state_dict"):
            raise U.GdnError("%s has no state_dict(): a resumed run would replay its first batches" % type(loader).__name__)
        mine = loader.state_dict(epoch_done=i < 0)
    loaders = D.gather_objects(mine)
    if loaders is None:
        return None
    state = {"format": 1, "world": D.world_size(), "model": _cpu_copy(dict(model.state_dict())),
             "optimizer": _cpu_copy(optimizer.state_dict()), "loader": loaders,
             "torch_rng": torch.get_rng_state(),
             "cuda_rng": torch.cuda.get_rng_state() if torch.cuda.is_available() and torch.cuda.is_initialized() else None}
    defaults = {"epoch": 0, "i": -1, "lr": optimizer.param_groups[0]["lr"], "model_num": 0, "seen": 0, "step": 0}
    for k in PROGRESS_KEYS:
        v = progress.get(k, defaults[k])
        state[k] = float(v) if k == "lr" else int(v)
    if int(progress.get("accum_steps", 1)) > 1:
        state["accum_steps"] = int(progress["accum_steps"])
    if progress.get("schedule") is not None:
        state["schedule"] = dict(progress["schedule"])
    return state


def load_training_state(state, model, optimizer, loader):
    """Put a training_state() dict back into newly built objects and return its progress dict for the training loops.
    Every rank reads the same dict and takes its own loader entry; a world size other than the saved one is refused."""
    world, saved = D.world_size(), int(state.get("world", 1))
    if saved != world:
        raise U.GdnError("training state was saved by %d rank(s), this run has %d: the loaders' shards and streams do not "
                         "carry over" % (saved, world))
    theirs, mine = state.get("schedule"), getattr(optimizer, "schedule", None)
    if (None if theirs is None else {k: v for k, v in theirs.items() if k != "lr_schedule"}) != mine:
        raise U.GdnError("the training state was written under the learning-rate schedule %r, this run has %r "
                         "(--lr_schedule / --warmup_steps / --lr_floor / the run's length): the update counts it carries would "
                         "mean other rates" % (theirs, mine))
    # --optimizer: the optimizer state says which update rule wrote it ('decoupled', only when it is on); refused here, before
    # the weights are overwritten, as optim.Adam.load_state_dict() would refuse it after
    theirs = bool((state["optimizer"].get("gdn") or {}).get("decoupled", False))
    if theirs != bool(getattr(optimizer, "decoupled", False)):
        names = ("--optimizer adam", "--optimizer adamw")
        raise U.GdnError("the training state was written under %s, this run has %s: the weight decay its optimizer state "
                         "carries would mean another update" % (names[theirs], names[not theirs]))
    model.load_state_dict(state["model"])
    ar = getattr(model, "_gdn_param_arena", None)
    if ar is not None:
        ar.touch()               # bf16 shadows of the weights are stale
    optimizer.load_state_dict(state["optimizer"])
    if loader is not None:
        mine = state["loader"][D.rank()]
        if mine is None:
            raise U.GdnError("the training state holds no loader state for rank %d" % D.rank())
        loader.load_state_dict(mine)
    torch.set_rng_state(state["torch_rng"])
    if state.get("cuda_rng") is not None and torch.cuda.is_available():
        torch.cuda.set_rng_state(state["cuda_rng"])
    progress = {k: state[k] for k in PROGRESS_KEYS}
    if "accum_steps" in state:
        progress["accum_steps"] = int(state["accum_steps"])
    if "schedule" in state:
        progress["schedule"] = dict(state["schedule"])
    return progress


def save_training_state(path, model, optimizer, loader, progress, writer=torch.save):
    """training_state() written to `path` by rank 0: to a temporary name in the same directory, then os.replace(), so a kill
    during the write leaves the previous file, never a truncated one.  Returns the path (None on the other ranks)."""
    state = training_state(model, optimizer, loader, progress)
    if state is None:
        return None
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    tmp = "%s.tmp.%d" % (path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            writer(state, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise
    return path


def read_training_state(path):
    """The dict save_training_state() wrote (tensors, numbers, strings, lists and tuples only: no code is unpickled)."""
    return torch.load(path, map_location="cpu", weights_only=True)


class _StateSaver:
    """--save_state / --save_state_every of one training loop: the rolling <save_dir>/train_state.pt, and when it is
    written.  The loop reports what happened -- stepped(), checkpointed(), begin_epoch() -- and asks write_now(i) after a
    batch and `pending` at the epoch's end.  A state falls due every `every` steps and on every checkpoint (--save_state).
    One that falls due inside an open micro-batch group waits for the group's end; one that falls due on the loader's last
    batch waits for the epoch's own work (checkpoint, validation) and is written as the start of the next epoch."""

    def __init__(self, args, save_dir, model, optimizer, loader):
        self.accum = _accum_steps(args)
        self.schedule = None               # the state file's 'schedule' entry: set by the loop where the run has one
        self.on_checkpoint = bool(getattr(args, "save_state", False))
        self.every = max(0, int(getattr(args, "save_state_every", 0) or 0))
        self.path = save_dir + '/' + STATE_FILE
        self.objs = (model, optimizer, loader)
        self.log = None                    # --train_log: flushed before every state file, which so never runs ahead of the log
        self.batches = len(loader) if hasattr(loader, "__len__") else None
        self.pending = self.held = False

    def last_batch(self, i):
        return self.batches is not None and i >= self.batches - 1

    def begin_epoch(self):
        self.pending = self.held = False

    def stepped(self, step, held):
        """Step number `step` of the run is done; held: it left a micro-batch group open."""
        self.pending = (self.every > 0 and step % self.every == 0) or (self.held and self.pending)
        self.held = held

    def checkpointed(self):
        self.pending = self.pending or self.on_checkpoint

    def write_now(self, i):
        return self.pending and not self.held and not self.last_batch(i)

    def save(self, epoch, i, lr, model_num, seen, step):
        progress = {"epoch": epoch, "i": i, "lr": lr, "model_num": model_num, "seen": seen, "step": step}
        if self.accum > 1:
            progress["accum_steps"] = self.accum
        if self.schedule is not None:
            progress["schedule"] = self.schedule
        if self.log is not None:
            self.log.flush()
        save_training_state(self.path, *self.objs, progress)
        self.pending = False


# ---------------------------------------------------------------------------------------------------------------------
# --accum_steps: K loader batches per Adam update
def _accum_steps(args):
    return max(1, int(getattr(args, "accum_steps", 1) or 1))


def _check_accum(args, progress):
    """--accum_steps of this run against the one of the training state it resumes: the groups of an epoch are formed by
    batch position, so another K would cut them elsewhere.  Raises before any step."""
    accum = _accum_steps(args)
    if getattr(args, "graph", False) and accum > 1:
        raise U.GdnError("--graph with --accum_steps %d: a group would need graphs of its first, middle and last micro-step; "
                         "capturing those is a follow-up, not part of this version" % accum)
    if progress is not None and int(progress.get("accum_steps", 1)) != accum:
        raise U.GdnError("the training state was written with --accum_steps %d, this run has --accum_steps %d: the resumed "
                         "run would group its batches differently" % (int(progress.get("accum_steps", 1)), accum))
    return accum


# ---------------------------------------------------------------------------------------------------------------------
# --warmup_steps / --lr_schedule / --lr_floor: the rate of every update set on the device
def schedule_total(args, n_epochs, epoch_size):
    """The run's length in Adam UPDATES: n_epochs x ceil(epoch_size / accum_steps) -- the groups of --accum_steps never cross
    an epoch's end, so the one an epoch ends with may be shorter and still is one update."""
    accum = _accum_steps(args)
    return int(n_epochs) * ((int(epoch_size) + accum - 1) // accum)


def lr_schedule_of(args, n_epochs, epoch_size):
    """optim.Adam's `schedule` for this command line, None where the run has none (--lr_schedule reference without
    --warmup_steps: today's run).  reference with a warm-up is the device's 'constant' kind under the reference's decay,
    which keeps writing group['lr']; constant / linear / cosine own the rate.  A function of the command line alone, so a
    resumed run computes the same schedule."""
    flag = getattr(args, "lr_schedule", None) or "reference"
    warmup = int(getattr(args, "warmup_steps", 0) or 0)
    if flag == "reference" and warmup == 0:
        return None
    total = schedule_total(args, n_epochs, epoch_size)
    decays = flag in ("linear", "cosine")
    if total < 1:
        raise U.GdnError("--lr_schedule %s over a run of %d updates" % (flag, total))
    if decays and warmup >= total:
        raise U.GdnError("--warmup_steps %d leaves nothing of the %d updates of this run (epochs x ceil(epoch_size / "
                         "accum_steps)) to the %s decay" % (warmup, total, flag))
    return {"kind": "constant" if flag == "reference" else flag, "warmup": warmup, "total": total,
            "floor": float(getattr(args, "lr_floor", 0.0) or 0.0) if decays else 0.0}


def _check_schedule(args, schedule, optimizer, progress):
    """The loop's schedule against the optimizer it was handed and the training state it resumes; raises before any step.
    Returns the state file's 'schedule' entry (None: the run has none and writes the file it always wrote)."""
    have = getattr(optimizer, "schedule", None)
    if have != schedule:
        raise U.GdnError("this run's learning-rate schedule is %r, its optimizer was built with %r: build it with "
                         "optim.Adam(schedule=trainer.lr_schedule_of(args, epochs, epoch_size))" % (schedule, have))
    entry = None if schedule is None else dict(schedule, lr_schedule=getattr(args, "lr_schedule", None) or "reference")
    if progress is not None and progress.get("schedule") != entry:
        raise U.GdnError("the training state was written under the learning-rate schedule %r, this run has %r: the resumed "
                         "run would take other rates" % (progress.get("schedule"), entry))
    return entry


def _print_lr(optimizer):
    """The rates the last update used, one per param group (a device read: only where the loops print anyway)."""
    if getattr(optimizer, "schedule", None) is not None and _is_main():
        print("lr: " + "  ".join("-" if r is None else "%.6e" % r for r in optimizer.current_lr()))


def _start(progress, lr):
    """(first epoch, batches of it already done, lr, model_num, seen, step) of a fresh (progress None) or resumed loop."""
    if progress is None:
        return 0, 0, lr, 0, 0, 0
    return (int(progress["epoch"]), int(progress["i"]) + 1, float(progress["lr"]), int(progress["model_num"]),
            int(progress["seen"]), int(progress["step"]))


def _to_dev(t, dev):
    return t if t.device == dev else t.to(dev, non_blocking=True)


def _device_of(model):
    return next(model.parameters()).device


def _decay_lr(optimizer, lr, fast_div):
    """lr -= lr/100 below 2e-5, else lr/fast_div (trainer.py:498-506 / :784-792)."""
    lr -= lr / 100 if lr < 0.00002 else lr / fast_div
    for g in optimizer.param_groups:
        g['lr'] = lr
    if _is_main():
        print('Decayed learning rates, lr: {}'.format(lr))
    return lr


def _guard_stats(optimizer):
    """guard_stats() of an optimizer with a gradient guard (a device read: only where the loops print anyway), else None."""
    return optimizer.guard_stats() if getattr(optimizer, "guarded", False) and _is_main() else None


def _print_guard_progress(optimizer):
    gs = _guard_stats(optimizer)
    if gs is not None:
        print("grad_norm: %.4f  clip_coef: %.4f  (clipped %d, skipped %d of %d steps)" %
              (gs["norm"], gs["coef"], gs["clipped"], gs["skipped"], gs["steps"]))


def _print_guard_epoch(optimizer):
    gs = _guard_stats(optimizer)
    if gs is not None:
        print("grad guard: clipped %d, skipped %d of %d steps" % (gs["clipped"], gs["skipped"], gs["steps"]))


# ---------------------------------------------------------------------------------------------------------------------
# the step of a training loop in its three shapes: eager, replayed as a hipGraph (--graph), and as the
# micro-steps of a group (--accum_steps K > 1)
class _EagerStep:
    """What the loop driver calls per loader batch: stepper(i, *inputs) -> the loss terms of batch i of the epoch.  This
    one is the plain step -- fwd_bwd (forward, losses, zero_grad, backward), all-reduce, Adam -- and the no-op form of
    what the driver tells every stepper: begin_epoch(), end_epoch(), close()."""
    held = False                # a micro-batch group is open: the batch just taken has not reached the weights yet
    log = None                  # --train_log (rank 0): trainlog.TrainLog, set by the loop driver; its record() follows the update

    def __init__(self, fwd_bwd, model, optimizer):
        self.fwd_bwd, self.model, self.optimizer = fwd_bwd, model, optimizer

    def update(self):
        with tracing.span("gdn.allreduce"):
            D.sync_gradients(self.model, self.optimizer)
        with tracing.span("gdn.adam"):
            self.optimizer.step()

    def step(self, *inputs):
        terms = self.fwd_bwd(*inputs)
        self.update()
        self.record(terms)
        return terms

    def record(self, terms, updated=True):
        """The step's row of the training log (one small launch, part of what --graph captures); updated False: a micro-batch
        inside an open group, whose row carries no update columns."""
        if self.log is not None:
            self.log.record(terms, self.optimizer if updated else None)

    def __call__(self, i, *inputs):
        return self.step(*inputs)

    def begin_epoch(self):
        pass

    end_epoch = close = begin_epoch


last_graph_report = None       # what the last --graph loop of this process printed: {'replayed', 'warmup', 'eager_steps'}


def _shapes(inputs):
    return [(tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else None for t in inputs]


class _GraphedStep(_EagerStep):
    """The step of one --graph training loop.  The first `graph_warmup` steps of the run (or of the resumed run) are the
    loop's ordinary eager steps on their own batches.  The next batch is captured around (prewarmed: the capture executes
    nothing) and replayed, and so is every later batch of its shapes -- provided an eager step has already run at these
    shapes and no larger batch has been seen: a last partial batch is never what gets captured once a full one has run.
    Every other batch (a partial one, or one that waits for such a capture) runs eagerly and is counted in `eager_steps`.
    One graph at world 1, two around the eager all-reduce otherwise.  reads: the loader outputs the step's inputs are, in
    the step's order -- a loader that can write into the static inputs (bind_outputs) is handed them in its own order."""

    def __init__(self, args, fwd_bwd, model, optimizer, loader, reads):
        if not getattr(optimizer, "capturable", False):
            raise U.GdnError("--graph needs optim.Adam(..., capturable=True): the step count must live on the device")
        super().__init__(fwd_bwd, model, optimizer)
        self.loader, self.reads = loader, reads
        self.warmup = max(1, int(getattr(args, "graph_warmup", 3) or 3))
        self.graphed, self.shapes, self.seen, self.largest = None, None, [], 0
        self.warm = self.replayed = self.eager_steps = 0
        self.bound = False

    def _capture(self, inputs, shapes):
        from .graph import GraphedDataParallelStep, GraphedTrainStep
        if D.world_size() > 1:
            self.graphed = GraphedDataParallelStep(self.fwd_bwd, self.model, self.optimizer, inputs, prewarmed=True,
                                                   after_step=self.record if self.log is not None else None)
        else:
            self.graphed = GraphedTrainStep(self.step, inputs, self.optimizer, prewarmed=True)
        self.shapes = shapes
        if callable(getattr(self.loader, "bind_outputs", None)):
            static = self.graphed.static_inputs                     # from the next batch on nothing is copied
            self.loader.bind_outputs(*[static[self.reads.index(j)] if j in self.reads else None for j in range(3)])
            self.bound = True

    def __call__(self, i, *inputs):
        shapes = _shapes(inputs)
        if self.graphed is None:
            n = inputs[0].shape[0]
            if self.warm >= self.warmup and shapes in self.seen and n >= self.largest:
                self._capture(inputs, shapes)
            else:
                if self.warm < self.warmup:
                    self.warm += 1
                else:
                    self.eager_steps += 1
                if shapes not in self.seen:
                    self.seen.append(shapes)
                self.largest = max(self.largest, n)
                return self.step(*inputs)
        if shapes != self.shapes:
            self.eager_steps += 1
            return self.step(*inputs)
        with tracing.span("gdn.graph_step"):
            out = self.graphed(*inputs)
        self.replayed += 1
        return out

    def close(self):
        """End of the loop: the loader gets its own outputs back, rank 0 reports once."""
        global last_graph_report
        if self.bound:
            self.loader.bind_outputs(None, None, None)
            self.bound = False
        last_graph_report = {"replayed": self.replayed, "warmup": self.warm, "eager_steps": self.eager_steps}
        if _is_main():
            print("graph: %d steps replayed as %s, %d eager (%d warm-up, %d on batches of another shape)" %
                  (self.replayed, "2 graphs around the all-reduce" if D.world_size() > 1 else "1 graph",
                   self.warm + self.eager_steps, self.warm, self.eager_steps))


class _GroupedStep(_EagerStep):
    """The micro-steps of one --accum_steps K > 1 training loop.  The loader batches of an epoch form groups by position
    (i // K): zero_grad before a group's first backward, the following backwards accumulate into the gradient arena
    (engine.ParamArena.bind_grads: no copy, one gdn_grad_accumulate launch each), and after the group's last backward ONE
    sync_gradients and ONE optimizer step with micro_batches = the number of micro-batches the group has -- K, or fewer for
    the group an epoch ends with.  Groups never cross an epoch boundary.  Under data parallelism no micro-batch starts the
    overlapped reducer (the model is marked like a graphed one): the local sums accumulate and the whole arena is reduced
    once per update."""

    def __init__(self, fwd_bwd, model, optimizer, accum, epoch_size, saver):
        super().__init__(fwd_bwd, model, optimizer)
        self.accum, self.epoch_size, self.saver = accum, epoch_size, saver
        self.micro = 0                      # micro-batches of the open group so far; 0: between two groups
        if D.world_size() > 1:
            model._gdn_whole_arena_sync = True

    @property
    def held(self):
        return self.micro > 0

    def begin_epoch(self):
        self.micro = 0

    def end_epoch(self):
        """The update of the open group (the driver's own call matters only where a loader ended without notice)."""
        if self.micro > 0:
            self.optimizer.micro_batches, self.micro = self.micro, 0
            self.update()

    def __call__(self, i, *inputs):
        terms = self.fwd_bwd(*inputs, first=self.micro == 0)
        self.micro += 1
        closes = self.micro >= self.accum or i >= self.epoch_size - 1 or self.saver.last_batch(i)
        if closes:
            self.end_epoch()
        self.record(terms, updated=closes)
        return terms

    def close(self):
        self.optimizer.micro_batches = 1


# ---------------------------------------------------------------------------------------------------------------------
# --train_log: the per-step record kept on the device
def train_log_header(args, model, optimizer, accum, with_tensors):
    """The run's description in line 1 of the training log: a function of the command line and the model alone, so a resumed
    run computes the same one.  `tensors`: the parameter names in arena order (the arena takes model.parameters() in order),
    only where the norms are on; `loose_parameters`: parameters of the optimizer that are not the model's, hence in no arena
    row of the norms."""
    mine = {id(p) for p in model.parameters()}
    header = {"mode": args.mode, "dtype": str(getattr(args, "dtype", "fp32")), "loss": getattr(args, "loss", None) or "berhu",
              "world": D.world_size(), "batch_size": int(getattr(args, "batch_size", 0) or 0), "accum_steps": int(accum),
              "optimizer": getattr(args, "optimizer", None) or "adam",
              "groups": [float(g.get("lr_mult", 1.0)) for g in optimizer.param_groups],
              "loose_parameters": sum(1 for g in optimizer.param_groups for p in g["params"] if id(p) not in mine)}
    if with_tensors:
        header["tensors"] = [n for n, _ in model.named_parameters()]
    return header


def _open_train_log(args, cadence, model, optimizer, dev, progress, gstep, accum):
    """(trainlog.TrainLog, --tensor_norms_every) on rank 0 of a run with --train_log; (None, 0) everywhere else: nothing is
    allocated, launched or written.  A resumed run continues the file after its step (trainlog.LogFile)."""
    path, every, norms_every = option.train_log_spec(args)
    if not path or not _is_main():
        return None, 0
    from .trainlog import TrainLog, TrainLogError
    try:
        log = TrainLog(path, cadence.terms, every, dev,
                       header=train_log_header(args, model, optimizer, accum, norms_every > 0), model=model,
                       resume_step=None if progress is None else gstep)
    except TrainLogError as e:
        raise U.GdnError(str(e))
    return log, norms_every


def _log_arena(model, log):
    """The trained model's arena for the norms row, whose items are the header's `tensors` in order."""
    ar = getattr(model, "_gdn_param_arena", None)
    if ar is None or [id(p) for p, _, _, _ in ar.items] != [id(p) for p in model.parameters()]:
        raise U.GdnError("--tensor_norms_every: the trained model has no intact parameter arena in model.parameters() order")
    return ar


# ---------------------------------------------------------------------------------------------------------------------
# the loop driver: what train_AE_DtoD and train_AE_RtoD share
class _Cadence(typing.NamedTuple):
    """What differs between the two training loops beside the step itself (the reference's trainer.py:498-506 / :784-792)."""
    save_dir: str                   # './<dataset>' + this % (lr * 100000)
    reads: tuple                    # the loader outputs the step reads, in its order; the last: sparse depth, None off KITTI
    decay: tuple                    # (after this epoch, every so many batches, the divisor above 2e-5)
    print_every: int
    progress_line: str              # % (the step's loss terms..., images/s)
    checkpoint_every: int
    checkpoint_each_epoch: bool     # every epoch a step has run in prints its loss and ends with a checkpoint; without it a
    #                                 run that wrote no checkpoint at all ends with one (and its state)
    terms: tuple                    # the names of the step's loss terms, in the step's order (--train_log)


_DTOD = _Cadence('_AE_DtoD_trained_model_lr000%d_color_uNet_gen2_nogradf', (0, 2), (5, 1900, 25), 50,
                 "total_loss: %5f, output_loss: %5f, gradient_loss: %5f  (%.1f img/s)", 3000, True,
                 ("total_loss", "output_loss", "gradient_loss"))
_RTOD = _Cadence('_AE_RtoD_trained_model_lr000%d_color_uNet_gen2_nogradf', (1, 0, 2), (2, 2200, 60), 100,
                 "total_loss: %5f, output_loss: %5f, smoothness_loss: %5f, latent_loss: %5f  (%.1f img/s)", 700, False,
                 ("total_loss", "output_loss", "smoothness_loss", "latent_loss"))


def _run_loop(args, cadence, fwd_bwd, model, optimizer, loader, val_loader, n_epochs, lr, logger, progress):
    """The epochs of one training run: fwd_bwd(*inputs, first=True) -> loss terms (the loss first) is the loop's own forward,
    losses, zero_grad (where `first`) and backward; everything around it is here.  Returns the terms of the last step, None
    if none ran.  progress: what load_training_state() returned -- the loop goes on after that step."""
    if _is_main():
        print("Training for %d epochs..." % n_epochs)
    dev = _device_of(model)
    save_dir = './' + args.dataset + cadence.save_dir % (lr * 100000)
    epoch_size = getattr(args, "epoch_size", 0) or len(loader)
    kitti = args.dataset == "KITTI"
    dense, sparse_at = cadence.reads[:-1], cadence.reads[-1]
    decay_after, decay_every, decay_div = cadence.decay
    terms = None
    epoch0, first, lr, model_num, seen, gstep = _start(progress, lr)
    saver = _StateSaver(args, save_dir, model, optimizer, loader)
    accum = _check_accum(args, progress)
    # the device sets the rate; under constant / linear / cosine the reference's decay is off
    saver.schedule = _check_schedule(args, lr_schedule_of(args, n_epochs, epoch_size), optimizer, progress)
    host_decay = (getattr(args, "lr_schedule", None) or "reference") == "reference"
    if accum > 1:
        stepper = _GroupedStep(fwd_bwd, model, optimizer, accum, epoch_size, saver)
    elif getattr(args, "graph", False):
        stepper = _GraphedStep(args, fwd_bwd, model, optimizer, loader, cadence.reads)
    else:
        stepper = _EagerStep(fwd_bwd, model, optimizer)
    log, norms_every = _open_train_log(args, cadence, model, optimizer, dev, progress, gstep, accum)
    stepper.log = saver.log = log

    def checkpoint(counted=True):
        nonlocal model_num
        _save_checkpoint(model, save_dir + '/epoch_%d_AE_depth_loss_%.4f.pkl' % (model_num + 1, terms[0].item()), optimizer)
        if counted:
            model_num += 1
            saver.checkpointed()

    t0 = time.time()
    for epoch in range(epoch0, n_epochs):
        model.train()
        saver.begin_epoch()
        stepper.begin_epoch()
        for i, batch in enumerate(loader, first):
            inputs = [_to_dev(batch[j], dev) for j in dense]
            inputs.append(_to_dev(batch[sparse_at], dev) if kitti else None)       # None <=> NYU: unmasked BerHu
            terms = stepper(i, *inputs)
            seen += inputs[0].shape[0] * D.world_size()
            gstep += 1
            if log is not None:
                log.note(epoch, i, gstep)
                if norms_every and gstep % norms_every == 0:
                    # eager, outside the graph: the arena's gradient still holds this step's values
                    log.tensor_norms(gstep, _log_arena(model, log), optimizer._scale())
            saver.stepped(gstep, stepper.held)
            if i >= epoch_size - 1:
                break
            if host_decay and epoch > decay_after and (i + 1) % decay_every == 0:
                lr = _decay_lr(optimizer, lr, decay_div)
            if (i + 1) % cadence.print_every == 0 and _is_main():
                print("epoch: %d,  %d/%d" % (epoch + 1, i + 1, epoch_size))
                print(cadence.progress_line % (tuple(t.item() for t in terms) + (seen / (time.time() - t0),)))
                _print_guard_progress(optimizer)
                _print_lr(optimizer)
            if (i + 1) % cadence.checkpoint_every == 0:
                checkpoint()
            if saver.write_now(i):
                saver.save(epoch, i, lr, model_num, seen, gstep)
        first = 0                       # (only the epoch a resumed run starts in has batches already done)
        stepper.end_epoch()
        if not cadence.checkpoint_each_epoch:
            _print_guard_epoch(optimizer)
        elif terms is not None:
            if _is_main():
                print('\n', 'epoch: ', epoch + 1, '  loss: ', terms[0].item())
            _print_guard_epoch(optimizer)
            checkpoint()
        if logger is not None and val_loader is not None:
            names, errors = _validate_epoch(args, val_loader, model, optimizer, epoch, logger)
            if log is not None:
                log.validation(gstep, epoch, names, errors)
        if saver.pending:               # after everything this epoch does: the resumed run starts the next one
            saver.save(epoch + 1, -1, lr, model_num, seen, gstep)
    if not cadence.checkpoint_each_epoch and terms is not None and model_num == 0:
        # no cadence save happened (the reference's per-epoch save is commented out, trainer.py:877-887): a run shorter than
        # 700 steps per epoch -- a fine-tune, a trial -- leaves the weights it ends with instead of nothing
        checkpoint(counted=False)
        if saver.on_checkpoint:
            saver.save(n_epochs, -1, lr, model_num, seen, gstep)
    stepper.close()
    if log is not None:
        log.close()
    return terms


def train_AE_DtoD(args, model, criterion_L2, criterion_L1, optimizer, dataset_loader, val_loader, batch_size,
                  n_epochs, lr, logger, train_writer, progress=None):
    """Depth->depth auto-encoder training; loss = BerHu + 3*imgrad_loss (trainer.py:411-468).
    progress: what load_training_state() returned -- the loop goes on after that step."""
    pixel = option.pixel_spec(args)     # None: BerHu, as ever; --loss silog: the spec of its pixel term

    def fwd_bwd(depths, sparse, first=True):
        with tracing.span("gdn.forward"):
            outputs = model(depths, istrain=False)
        with tracing.span("gdn.losses"):
            terms = U.dtod_loss(outputs, depths, sparse, pixel=pixel)
        if first:                       # (--accum_steps: the later backwards of a group accumulate)
            optimizer.zero_grad()
        with tracing.span("gdn.backward"):
            U.backward(terms[0])        # == loss.backward(), seed gradient cached
        return terms

    terms = _run_loop(args, _DTOD, fwd_bwd, model, optimizer, dataset_loader, val_loader, n_epochs, lr, logger, progress)
    return None if terms is None else terms[0]


def _cat_batch(a, b):
    """torch.cat((a, b), 0) for two dense [B,1,H,W] device tensors without a torch kernel (two pitched copies)."""
    from . import ops
    if a.shape[1] != 1 or a.dtype != torch.float32 or b.dtype != torch.float32 or a.shape != b.shape or a.shape[3] % 4:
        return torch.cat((a, b), 0)
    B, _, H, W = a.shape
    out = torch.empty((2 * B, 1, H, W), dtype=torch.float32, device=a.device)
    ops.copy_rows(a.contiguous(), out[:B])
    ops.copy_rows(b.contiguous(), out[B:])
    return out


def guide_latent_loss(G, depths, outputs, faithful=False, latent_grad=False):
    """Latent loss of trainer.py:699-733: G's features of the ground truth vs. of the estimate.

    Default (the reference as shipped, F3): both under no_grad, value only.
    faithful=True runs the guide exactly like the reference: two full forwards with ``istrain=True``.
    Otherwise the four features come from encoder-only passes (the same layers: 52 % of the work); without
    latent_grad the frozen eval-mode guide has no cross-sample coupling, so both inputs share ONE batched pass (the
    library picks tilings / split factors from the batch size, so a 2B pass equals two B passes to rounding, bitwise only
    where the plans coincide; its peak activation memory is that of a 2B forward).
    latent_grad=True is the guided training the paper describes: the estimate's features keep their autograd
    history, so d(latent)/d(outputs) flows back through the frozen, eval-mode G into the trained network."""
    feats = (lambda x: G(x, istrain=True)[:4]) if faithful or not hasattr(G, "guide_features") else G.guide_features
    if latent_grad:
        if G.training or any(p.requires_grad for p in G.parameters()):
            raise U.GdnError("--latent_grad needs a frozen guide: G.eval() and G.requires_grad_(False)")
        with torch.no_grad():
            ft_tar = feats(depths)
        return U.latent_loss(feats(outputs), ft_tar)
    with torch.no_grad():
        if G.training:
            # (training-mode batch statistics would couple the two halves of a batched pass: keep them separate)
            ft_tar = feats(depths)
            ft = feats(outputs.detach())
        else:
            # eval-mode guide: no cross-sample coupling, so the two forwards share ONE pass over the concatenated batch --
            # the same per-sample arithmetic up to the summation order of batch-size-dependent plans, half the launches, the
            # weight transforms computed once.  `faithful` still runs the whole network (decoder included) like the
            # reference; otherwise the pass stops at the bottleneck.
            B = depths.shape[0]
            both = feats(_cat_batch(depths, outputs.detach()))
            ft_tar = [f[:B] for f in both]
            ft = [f[B:] for f in both]
    return U.latent_loss(ft, ft_tar)


def train_AE_RtoD(args, model, DtoD_model, criterion_L2, criterion_L1, optimizer, dataset_loader, val_loader,
                  batch_size, n_epochs, lr, logger, train_writer, progress=None):
    """Colour->depth training with the frozen guide G (trainer.py:670-768).
    progress: what load_training_state() returned -- the loop goes on after that step (the guide is not part of the state).

    loss = BerHu + latent (value only: G's features of the estimate are taken
    under no_grad, exactly as shipped, F3) + smoothness.  mode 'RtoD_single'
    drops the latent term."""
    single = args.mode == 'RtoD_single' or DtoD_model is None
    latent0 = torch.zeros((), device=_device_of(model))
    pixel = option.pixel_spec(args)     # None: BerHu, as ever; --loss silog: the spec of its pixel term

    def fwd_bwd(inputs, depths, sparse, first=True):
        latent = latent0
        with tracing.span("gdn.forward"):
            outputs = model(inputs, istrain=False)
        tracing.push("gdn.losses")
        if not single:
            latent = guide_latent_loss(DtoD_model, depths, outputs, faithful=getattr(args, "faithful_guide", False),
                                       latent_grad=getattr(args, "latent_grad", False))
        if latent.requires_grad:            # --latent_grad: a differentiable term joins through autograd
            pix, output_loss, smooth = U.rtod_pixel_loss(outputs, depths, inputs, sparse, pixel=pixel)
            loss = pix + latent
        else:                               # value-only latent loss (F3): summed by the loss kernel itself
            loss, output_loss, smooth = U.rtod_pixel_loss(outputs, depths, inputs, sparse, plus=latent, pixel=pixel)
        tracing.pop()
        if first:                       # (--accum_steps: the later backwards of a group accumulate)
            optimizer.zero_grad()
        with tracing.span("gdn.backward"):
            U.backward(loss)            # == loss.backward(), seed gradient cached
        return loss, output_loss, smooth, latent

    terms = _run_loop(args, _RTOD, fwd_bwd, model, optimizer, dataset_loader, val_loader, n_epochs, lr, logger, progress)
    return (None, None, latent0) if terms is None else (terms[0], terms[1], terms[3])


def _evaluate(val_loader, model, mode, metric, names, on_batch=None):
    """Forward (no_grad) + `metric(depth_np, depth, out)` per batch; returns (mean errors, mean of the abs_diff-sorted
    errors, names) like trainer.py:17-87.  Metrics stay on the device; one D2H copy at the end.  on_batch(depth, img,
    depth_np, out) sees every batch in loader order (--img_save writes its images from there)."""
    dev = _device_of(model)
    per_batch = []
    for depth, img, depth_np in val_loader:
        depth, img, depth_np = _to_dev(depth, dev), _to_dev(img, dev), _to_dev(depth_np, dev)
        x = img if mode in ('RtoD', 'RtoD_test', 'RtoD_single') else depth
        with torch.no_grad():
            out = model(x, istrain=False)
        per_batch.append(metric(depth_np, depth, out))
        if on_batch is not None:
            on_batch(depth, img, depth_np, out)
    if not per_batch:
        return [float('nan')] * len(names), [float('nan')] * len(names), names
    allv = torch.stack(per_batch).cpu()
    avg = allv.mean(0).tolist()
    order = torch.argsort(allv[:, 0])
    return avg, allv[order].mean(0).tolist(), names


def validate(args, val_loader, model, epoch, logger, mode='DtoD', on_batch=None):
    """KITTI: compute_errors (Godard crop) per batch, trainer.py:17-87."""
    return _evaluate(val_loader, model, mode, lambda s, g, o: compute_errors_device(s, g, o, crop=True), ERROR_NAMES,
                     on_batch)


def validate_std(args, val_loader, model, epoch, logger, mode='DtoD', on_batch=None, gt16=None, velo=None):
    """KITTI under the Eigen-split protocol (--eval_protocol standard): metric depth, the --min_depth /
    --max_depth cap, the --eval_crop box at the ground truth's own resolution, optional --median_scaling and --flip_test.
    The ground truth is the loader's third tensor (in [-1, 1], at the network's size) or, with gt16 (datasets.EigenGt16,
    one map per sample in loader order), the 16-bit maps at their native size, or, with velo (datasets.EigenVelodyne, one
    scan per sample in loader order), the maps ops.velo_project makes of the raw scans, batch by batch;
    rank 0 then prints the mean number of LiDAR pixels per image.  The per-image rows (and hit counts) stay on the device;
    one D2H copy (each) at the end.  Returns (the nine metrics as the float64 mean over ALL images with a valid pixel --
    not the mean of batch means --, the number of images left out, names); rank 0 prints that number whenever it is not 0."""
    from . import ops
    from .datasets import assemble_gt16, assemble_scans
    dev = _device_of(model)
    opt = option.eval_spec(args)
    rows, hits, k = [], [], 0
    if velo is not None and len(velo) != len(val_loader.ds):
        raise U.GdnError("--eval_velodyne names %d scans, the test split has %d samples" % (len(velo), len(val_loader.ds)))
    if gt16 is not None and len(gt16) != len(val_loader.ds):
        raise U.GdnError("--eval_gt_list names %d maps, the test split has %d samples" % (len(gt16), len(val_loader.ds)))
    for depth, img, depth_np in val_loader:
        depth, img, depth_np = _to_dev(depth, dev), _to_dev(img, dev), _to_dev(depth_np, dev)
        x = img if mode in ('RtoD', 'RtoD_test', 'RtoD_single') else depth
        with torch.no_grad():
            out = model(x, istrain=False)
            if opt["flip_test"]:
                out = out.detach().float().contiguous()
                mirrored = model(ops.flip_w(x.float().contiguous()), istrain=False).detach().float().contiguous()
                out = ops.flip_mean(out, mirrored, out=out)
        B = out.shape[0]
        gt_kind = None
        if velo is not None:
            scans = [velo[k + i] for i in range(B)]
            points, offsets, proj, hw, Hmax, Wmax, sizes = assemble_scans(scans, dev)
            gt, n_hit = ops.velo_project(points, offsets, proj, hw, Hmax, Wmax, depth=velo.depth, hits=True,
                                         max_points=max(len(s[0]) for s in scans))
            gt_kind = ops.GT_METRES
            hits.append(n_hit)
        elif gt16 is None:
            gt, sizes = depth_np, None
        else:
            gt, sizes = assemble_gt16([gt16[k + i] for i in range(B)], dev)
        k += B
        rows.append(compute_errors_std_device(gt, sizes, out, crop=opt["crop"], min_depth=opt["min_depth"],
                                              max_depth=opt["max_depth"], depth_scale=opt["depth_scale"],
                                              median_scaling=opt["median_scaling"], gt_kind=gt_kind))
        if on_batch is not None:
            on_batch(depth, img, depth_np, out)
    if not rows:
        return [float('nan')] * len(ERROR_NAMES_STD), 0, ERROR_NAMES_STD
    errors, left_out = mean_errors_std(torch.cat(rows).cpu())
    if hits and _is_main():
        print("=> Velodyne ground truth: %.1f LiDAR pixels per image on average (%d images)"
              % (float(torch.cat(hits).cpu().double().mean()), k))
    if left_out and _is_main():
        print("=> standard protocol: %d of %d images have no valid pixel and are left out of the mean" % (left_out, k))
    return errors, left_out, ERROR_NAMES_STD


def validate_NYU(args, val_loader, model, epoch, logger, mode='DtoD', on_batch=None):
    """NYU Depth v2: compute_errors_NYU (crop on) per batch, trainer.py:200-270."""
    return _evaluate(val_loader, model, mode, lambda s, g, o: compute_errors_NYU_device(g, o, crop=True), ERROR_NAMES_NYU,
                     on_batch)


def validate_Make3D(args, val_loader, model, epoch, logger, mode='DtoD', on_batch=None):
    """Make3D: compute_errors_Make3D per batch, trainer.py:272-327."""
    return _evaluate(val_loader, model, mode, compute_errors_Make3D_device, ERROR_NAMES_MAKE3D, on_batch)
