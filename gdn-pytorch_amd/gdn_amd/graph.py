"""Whole-training-step hipGraph capture.

The engine's forward, the fused loss kernels, the tape replay of backward and the fused Adam are all stream-ordered,
allocation-free (beyond torch's caching allocator) and sync-free, so one training step -- ~600 launches of host enqueue
time -- can be captured once and replayed as a single graph launch.  What has to live in device memory
for that: the optimizer's step counter / bias corrections / learning rate (``optim.Adam(capturable=True)`` ->
``gdn_adam_step_dev``; the gradient guard's record and the weight average are device memory too) and the batch (static
input buffers, refilled before every replay -- or written in place by a loader bound to them,
``datasets.GpuAugmentLoader.bind_outputs``).

``GraphedTrainStep`` is the single-process form: one graph from the forward to the optimizer.  It refuses world sizes > 1.
``GraphedDataParallelStep`` works at any world size: graph A (forward, losses, zero_grad, backward), the gradient
all-reduce issued EAGERLY over the whole arena, graph B (the optimizer).  No collective is ever captured, so the overlap of
the all-reduce with backward (distributed.GradReducer) is given up for such a model.

Both classes either warm up on their example batch (several real optimizer steps on it: a benchmark's way) or, with
``prewarmed=True``, only capture: the caller -- the training loops under ``--graph`` -- has run the step eagerly on real
batches, and every batch is seen exactly once.  Capturing executes nothing.
"""
import torch

from . import distributed as D
from . import engine as E
from ._lib import GdnError


def _refill(static_inputs, inputs):
    """Copy `inputs` into the static buffers; an input that already IS its buffer (a bound loader wrote it there) costs
    nothing.  Returns the number of copies made."""
    n = 0
    for dst, src in zip(static_inputs, inputs):
        if torch.is_tensor(dst) and src is not dst:
            dst.copy_(src, non_blocking=True)
            n += 1
    return n


def _need_capturable(optimizer, who):
    if not getattr(optimizer, "capturable", False):
        raise GdnError("%s needs optim.Adam(..., capturable=True) (device-side step counter)" % who)


class GraphedTrainStep:
    """Capture ``step_fn(*static_inputs)`` -- forward, losses, zero_grad, backward, optimizer.step -- and replay it.

    step_fn must use the tensors it is handed (they are the graph's static input buffers) and return a tensor or a tuple
    of device tensors (e.g. the loss terms); the same static output tensors are returned by every replay.
    optimizer must be ``gdn_amd.optim.Adam(..., capturable=True)``.
    prewarmed=True: the caller has already run step_fn eagerly on batches of these shapes (the arena, the workspaces and
    the optimizer state exist); no warm-up step is taken, construction only captures -- weights, moments and step counts are
    what they were -- and the first call replays the step for the batch it is given.
    `refills` counts the copies into the static inputs that calls had to make."""

    def __init__(self, step_fn, example_inputs, optimizer, warmup=3, prewarmed=False):
        if D.world_size() > 1:
            raise GdnError("GraphedTrainStep is single-process: the RCCL gradient all-reduce is not captured")
        _need_capturable(optimizer, "GraphedTrainStep")
        self.optimizer = optimizer
        self.static_inputs = [t.clone() if torch.is_tensor(t) else t for t in example_inputs]
        self.warmup_steps = 0
        if not prewarmed:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):            # warm-up: allocates every workspace, the arena, the optimizer state
                for _ in range(max(1, warmup)):
                    out = step_fn(*self.static_inputs)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.warmup_steps = max(1, warmup)
        before = optimizer.host_counts() if prewarmed else None
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            out = step_fn(*self.static_inputs)
        # (prewarmed: the run's host-side counts follow the replays, so a state_dict() equals the eager run's)
        self._counts = optimizer.take_back_counts(before) if prewarmed else []
        self.static_outputs = out
        self.replays = 0
        self.refills = 0
        E.bump_graph_epoch()

    def __call__(self, *inputs):
        self.refills += _refill(self.static_inputs, inputs)
        self.optimizer.refresh_hyper()           # a learning-rate decay since the last replay reaches the device here
        self.graph.replay()
        self.replays += 1
        self.optimizer.count_replay(self._counts)
        E.bump_graph_epoch()                     # BN running statistics changed behind torch's version counters
        return self.static_outputs


class GraphedDataParallelStep:
    """A training step as two graphs around an eager gradient all-reduce, at any world size.

    Graph A is ``fwd_bwd_fn(*static_inputs)`` -- forward, losses, zero_grad, backward, no optimizer -- graph B is
    ``optimizer.step()``.  A call refills the static inputs, pushes changed hyper-parameters, replays A, runs
    ``distributed.sync_gradients(model, optimizer)`` eagerly, replays B and returns A's static outputs.
    No collective may sit inside a capture: `model` is marked so that its backward never starts the overlapped
    GradReducer again and sync_gradients() reduces the whole gradient arena in one go after A (for this model only; the
    GDN_OVERLAP_ALLREDUCE switch is not touched).  Refused: a gradient accumulated across a sync that is still pending
    (ParamArena.carry_reduced) and, at world > 1, utils.GLOBAL_BERHU, whose all-reduce(MAX) sits inside the loss.
    At world 1 sync_gradients() does nothing and the class is GraphedTrainStep in two launches.

    after_step(outputs): captured into graph B right after ``optimizer.step()`` (the trainer's --train_log record, which reads
    A's static outputs and the optimizer's device records); the warm-up steps of a capture that is not prewarmed do not call it.

    prewarmed / warmup: as for GraphedTrainStep; the eager steps before a prewarmed capture must have gone through
    sync_gradients(model, optimizer), which leaves optimizer.grad_scale = 1/world -- the value graph B is captured with."""

    def __init__(self, fwd_bwd_fn, model, optimizer, example_inputs, prewarmed=False, warmup=3, after_step=None):
        from . import utils as U
        _need_capturable(optimizer, "GraphedDataParallelStep")
        world = D.world_size()
        if world > 1 and U.GLOBAL_BERHU:
            raise GdnError("GraphedDataParallelStep: utils.GLOBAL_BERHU all-reduces the BerHu threshold inside the loss; a "
                           "collective cannot be captured")
        self.model, self.optimizer = model, optimizer
        red = getattr(model, "_gdn_reducer", None)
        if red is not None and red.active:
            raise GdnError("GraphedDataParallelStep: an overlapped gradient all-reduce of this model is still in flight; call "
                           "sync_gradients() first")
        model._gdn_whole_arena_sync = True           # engine.begin_backward / distributed.attach_reducer: no overlap
        self.static_inputs = [t.clone() if torch.is_tensor(t) else t for t in example_inputs]
        self.warmup_steps = 0
        if not prewarmed:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(max(1, warmup)):
                    fwd_bwd_fn(*self.static_inputs)
                    D.sync_gradients(model, optimizer)
                    optimizer.step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.warmup_steps = max(1, warmup)
        ar = getattr(model, "_gdn_param_arena", None)
        if ar is None:
            raise GdnError("GraphedDataParallelStep(prewarmed=True): the model has no gradient arena; run the step eagerly first")
        if getattr(ar, "carry_reduced", None) is not None:
            raise GdnError("GraphedDataParallelStep: an accumulated, already all-reduced gradient is pending "
                           "(backward, sync_gradients, backward); gradient accumulation across a sync cannot be replayed")
        if D.active() and float(optimizer.grad_scale) != 1.0 / world:
            raise GdnError("GraphedDataParallelStep: optimizer.grad_scale is %r, not 1/%d: the eager steps before the capture "
                           "must go through sync_gradients(model, optimizer)" % (optimizer.grad_scale, world))
        self.graph_a = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_a):
            out = fwd_bwd_fn(*self.static_inputs)
        if getattr(ar, "carry_reduced", None) is not None:
            raise GdnError("GraphedDataParallelStep: fwd_bwd_fn accumulates onto an all-reduced gradient (no zero_grad); "
                           "that cannot be replayed")
        before = optimizer.host_counts()
        self.graph_b = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_b):
            optimizer.step()
            if after_step is not None:
                after_step(out)                      # (the training log's record: part of graph B)
        counts = optimizer.take_back_counts(before)
        if not prewarmed:                            # (as GraphedTrainStep always did: the capture counts as a step taken)
            optimizer.count_replay(counts)
            counts = []
        self._counts = counts
        self.static_outputs = out
        self.replays = 0
        self.refills = 0
        E.bump_graph_epoch()

    def __call__(self, *inputs):
        self.refills += _refill(self.static_inputs, inputs)
        self.optimizer.refresh_hyper()
        self.graph_a.replay()
        D.sync_gradients(self.model, self.optimizer)     # eager: the whole arena, summed over the ranks
        self.graph_b.replay()
        self.replays += 1
        self.optimizer.count_replay(self._counts)
        E.bump_graph_epoch()
        return self.static_outputs
