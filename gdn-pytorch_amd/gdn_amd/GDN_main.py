"""Entry point with the reference's CLI: ``python -m gdn_amd.GDN_main DATA --mode {DtoD,RtoD,...}``.

Mirrors GDN_main.py:22-307 of the reference for the hot path: same flags
(option.py), same mode dispatch (:150-201), same optimiser settings
(Adam, betas from --momentum/--beta, eps 1e-8, weight decay hard-wired to 5e-4,
:157,173).  ``--gpu_num 0,1,2,3`` trains on the listed GPUs from one command like the
reference (README.md:82): ``main`` starts one child process per device
(``distributed.launch_ranks``) and gradients are all-reduced with RCCL
(nn.DataParallel is gone); under ``python -m torch.distributed.run`` each rank
takes its LOCAL_RANK GPU instead.

The KITTI/NYU file pipeline (datasets_list.py / transform_list.py) is host I/O
outside the hot path: pass ``--synthetic`` for KITTI-shaped random batches, or
call ``run(args, train_loader, val_loader)`` with loaders that yield the
reference's sample contract ``(gt[B,1,H,W], rgb[B,3,H,W], sparse[B,1,H,W])`` in [-1,1].  DATA is laid out like the
reference's (``train.txt`` / ``val.txt`` naming scenes, per scene ``*.jpg``, ``gt/*.png`` sparse and ``color_gt2/*.png`` dense
depth, bytes with 255 = ``--depth_scale`` metres; the three ``eigen_test_files_*.txt`` for ``--real_test``);
``python -m gdn_amd.prepare_kitti RAW_ROOT DATA --train_list F ...`` writes that layout from a raw KITTI download, the dense
maps filled from the LiDAR scans on the device.

Evaluation (--mode DtoD_test / RtoD_test, :234-307): ``--real_test`` evaluates KITTI on the Eigen test split
(TestFolder) instead of val.txt; ``--dataset NYU`` evaluates the NYU Depth v2 test set with compute_errors_NYU;
``--img_save`` writes the output depth, ground truth and input colour of every test image as JPEG under --result_dir,
from the validation pass itself.  ``--resident`` (KITTI file pipeline, training and ``--real_test``) decodes every file once
and keeps the set in device memory (datasets.GpuResidentLoader); ``--resident_gb`` caps it.
NYU training: pass ``train_loader=datasets.GpuNYUAugmentLoader(...)`` (the NYU transform of :94-129 on the GPU; or its
device-resident form GpuNYUResidentLoader) and a GpuCropLoader over the test set to run() with args.dataset == 'NYU'; the command line does
not build them.  Make3D training and evaluation are not implemented.
``--rtod_arch {unet,legacy}`` picks the colour-to-depth network of the RtoD modes (default: AutoEncoder_2 for training, the
legacy AutoEncoder for RtoD_test, as ever), so a checkpoint either mode trains can be evaluated by ``--mode RtoD_test``;
``--init_from X.pkl`` loads a state dict into the network being trained before the first step (fine-tuning the published
GDN_RtoD_pretrained.pkl: ``--mode RtoD --rtod_arch legacy --init_from GDN_RtoD_pretrained.pkl``).
``--save_state`` / ``--save_state_every N`` write the rolling ``<save_dir>/train_state.pt`` (weights, optimizer, loader and
schedule state); ``--resume PATH`` with the otherwise unchanged command line continues that run bit for bit.
``--clip_grad_norm X`` clips the global gradient norm and ``--skip_nonfinite`` drops a step whose gradient holds a NaN or an
Inf, both decided on the device inside the fused Adam (no sync, no torch kernel); the progress prints report the norm, the
coefficient and the counts.  The guard protects weights, moments and the step count -- a forward that was itself
non-finite has already written its BatchNorm running statistics.
``--ema_decay D`` keeps an exponential moving average of the weights inside the fused Adam: the per-epoch
validation runs on the averaged weights and every ``X.pkl`` is followed by ``X_ema.pkl`` with them, in the same format.
BatchNorm running statistics are buffers: the averaged model uses the live ones.
``--graph`` replays the training step as a hipGraph after ``--graph_warmup`` eager steps: one graph per step
on one GPU, two around the eager gradient all-reduce under data parallelism; the run is bit for bit the run without the flag.
``--accum_steps K`` applies the mean gradient of K loader batches in one Adam update: an effective batch of
K x batch_size x ranks with one gradient all-reduce per update; guard, average and step count are per update.  Not with
``--graph`` yet.
``--freeze_bn`` fine-tunes on the stored BatchNorm running statistics: the norm layers of the trained network
stay in eval mode -- they normalise by their running mean / variance and never update them -- while conv weights, gamma and
beta train.  It needs ``--init_from`` or ``--resume`` (a fresh network's statistics are mean 0 / variance 1) and is not
stored in ``train_state.pt``: a resumed run repeats it.
``--freeze SPEC[,SPEC...]`` (``encoder``, ``decoder`` or name patterns) trains only part of the network, ``--lr_mult SPEC=M,...``
trains parts of it at a multiple of the learning rate and ``--no_decay_norm`` takes the weight decay off gamma / beta
(DESIGN.md 3.8): the param groups they build all run in the fused Adam's one launch (``optim.Adam(segmented=True)``), and the
backward does no work below the lowest trainable layer.  ``--freeze`` needs ``--init_from`` or ``--resume``; none of the three
is stored in ``train_state.pt``: a resumed run repeats them.
``--warmup_steps W`` / ``--lr_schedule {reference,constant,linear,cosine}`` / ``--lr_floor F`` set the rate of every update on
the device: one small launch in front of the fused Adam turns the device's own count of applied updates into
``lr x lr_mult x s(u)`` -- a warm-up over W updates, then the reference's decay as ever (``reference``), no decay, or a linear /
cosine decay to ``F x lr`` at the run's last update (``epochs x ceil(epoch_size / accum_steps)``).  Nothing is written from the
host per step, so ``--graph`` replays it; ``train_state.pt`` stores the schedule and a resumed run must repeat it.
``--lr_schedule reference`` without a warm-up is the run without these flags.
``--loss silog`` trains on the scale-invariant log loss in the masked BerHu's place: ``--silog_weight`` x
sqrt(mean(d^2) - ``--silog_lambda`` x mean(d)^2) with d = log depth(out) - log depth(gt), depths clamped from below at
``--silog_floor`` of the range, over every pixel whose ground truth is above that floor (``--silog_mask dense``) or only
over the pixels of the Garg box with a LiDAR return (``lidar``, KITTI).  One HIP entry point, three launches, float64 per
pixel; the Sobel / smoothness / latent terms and the progress lines (``output_loss`` is the SILog value) are as ever, and
``--graph``, ``--resume``, ``--accum_steps``, the gradient guard and bf16 run on it unchanged.  Each rank takes the statistics
of its own shard; the flag is not stored in ``train_state.pt``: a resumed run repeats it.  ``--loss berhu`` is the run
without the flag.
``--eval_protocol standard`` evaluates KITTI under the Eigen-split protocol of the literature in the
reference protocol's place, in the test modes and in the per-epoch validation: metric depth (``--depth_scale`` metres at +1),
the ``--min_depth`` / ``--max_depth`` cap, the ``--eval_crop {garg,eigen,none}`` box, optional ``--median_scaling`` and
``--flip_test``, nine metrics averaged per image.  ``--eval_gt_list FILE`` (test modes with ``--real_test``) takes the ground
truth from 16-bit KITTI depth maps at their native size; the prediction is resampled to each map inside the metrics kernel.
The result line states the protocol's parameters.  ``--eval_protocol reference`` is the run without the flag.
``--eval_velodyne LIST --kitti_raw ROOT`` (same conditions, instead of ``--eval_gt_list``) makes that ground truth on the
device from the raw Velodyne scan of each test sample: one scatter kernel per batch projects the scans
through each date's calibration, the nearest point wins a pixel, ``--velo_depth {camera,forward}`` picks the depth that is
stored; the result line names the list and the run ends with the mean number of LiDAR pixels per image.
``--optimizer adamw`` trains with decoupled weight decay: ``--decoupled_wd W`` (1e-2 when not given) takes
the place of the reference's 5e-4, stays out of the gradient and the moments and shrinks each weight by ``rate x W x weight``
inside the fused update's own launches, ``rate`` being the update's (after ``--lr_mult`` and the schedule); ``--no_decay_norm``
takes it off gamma / beta.  It runs with ``--graph``, ``--resume``, ``--accum_steps``, the gradient guard, ``--ema_decay``,
``--freeze`` / ``--lr_mult``, the schedules, ``--loss silog`` and bf16; the optimizer state in ``train_state.pt`` says which
rule wrote it and a resumed run must repeat the flag.  ``--weight-decay`` stays accepted and ignored.  ``--optimizer adam`` is
the run without the flag.
``--train_log PATH`` keeps a per-step record of the run: one small launch per step copies the loss terms, the
update count, the rate and the gradient guard's norm, coefficient and skip decision -- all already in device memory -- into a
device ring, ``--graph`` replays it, and the host reads the ring with one asynchronous copy every ``--train_log_every N`` steps
(256) and writes JSON lines; ``--tensor_norms_every M`` adds the norm of every parameter tensor and of its gradient every M
steps, one deterministic pass over the arena.  The update columns are ``null`` where the run keeps no such device record: the
flag never changes which optimizer path runs (``--skip_nonfinite`` alone gives the norm column without clipping).  Rank 0
writes; no wall-clock value enters the file, so the same run writes the same bytes; ``--resume`` continues the file after the
resumed step and refuses one whose header is another run's.  ``python -m gdn_amd.trainlog PATH [--top K]`` summarises it.
"""
import contextlib
import io
import os
import sys

import torch

from . import distributed as D
from . import option
from . import utils as U
from .AE_model_unet import AutoEncoder, AutoEncoder_2, AutoEncoder_DtoD
from .optim import Adam
from .synthetic import SyntheticLoader
from .trainer import (load_checkpoint, load_training_state, lr_schedule_of, read_training_state, train_AE_DtoD, train_AE_RtoD,
                      validate, validate_NYU, validate_std)

TEST_MODES = ('DtoD_test', 'RtoD_test')


def _make_optimizer(model, args):
    """The reference's Adam; --clip_grad_norm / --skip_nonfinite add the device-side gradient guard, --ema_decay the
    weight average (optim.Adam)."""
    guard = {}
    if getattr(args, "clip_grad_norm", 0.0) > 0.0:
        guard["max_grad_norm"] = float(args.clip_grad_norm)
    if getattr(args, "skip_nonfinite", False):
        guard["skip_nonfinite"] = True
    if getattr(args, "ema_decay", 0.0) > 0.0:
        guard["ema_decay"] = float(args.ema_decay)
    if getattr(args, "graph", False):
        guard["capturable"] = True            # the step counter lives on the device (the guard and the average imply it)
    params = model.parameters()
    if _partial(args):
        # --freeze / --lr_mult / --no_decay_norm: param groups over the one arena, all of them in the fused Adam's one launch
        params, guard["segmented"] = param_groups(model, args), True
    # --warmup_steps / --lr_schedule: the rate of every update set on the device (None: today's run, nothing is launched)
    schedule = lr_schedule_of(args, getattr(args, "epochs", 0), getattr(args, "epoch_size", 0))
    if schedule is not None:
        guard["schedule"] = schedule
    # --optimizer adamw: --decoupled_wd in the place of the reference's L2 term, decoupled from the gradient
    decay = option.decoupled_wd(args)
    if decay is not None:
        return Adam(params, args.lr, [args.momentum, args.beta], eps=1e-08, weight_decay=decay, decoupled=True, **guard)
    return Adam(params, args.lr, [args.momentum, args.beta], eps=1e-08, weight_decay=5e-4, **guard)


def _partial(args):
    return bool(getattr(args, "freeze", None) or getattr(args, "lr_mult", None) or getattr(args, "no_decay_norm", False))


def param_groups(model, args):
    """The param groups of --lr_mult / --no_decay_norm: one per distinct (lr_mult, weight_decay), in order of first
    appearance among model.parameters(); every parameter is in one (a frozen one too: the optimizer skips it by its
    requires_grad).  A group states 'lr_mult' only where it is not 1 and 'weight_decay' only where it is not the optimizer's."""
    names = [n for n, _ in model.named_parameters()]
    mult = dict.fromkeys(names, 1.0)
    for spec, m in getattr(args, "lr_mult", None) or []:
        hit = model.select_parameters(spec)
        if not hit:
            raise RuntimeError("--lr_mult %s=%g selects no parameter of %s" % (spec, m, type(model).__name__))
        mult.update(dict.fromkeys(hit, float(m)))            # later entries win
    groups = {}
    for n, p in model.named_parameters():
        decay = 0.0 if getattr(args, "no_decay_norm", False) and p.dim() == 1 else None
        groups.setdefault((mult[n], decay), []).append(p)
    out = []
    for (m, decay), ps in groups.items():
        g = {"params": ps}
        if m != 1.0:
            g["lr_mult"] = m
        if decay is not None:
            g["weight_decay"] = decay
        out.append(g)
    return out


def _rtod_network(args, H, W):
    """The colour-to-depth network of the RtoD modes (option.rtod_arch): AutoEncoder_2, or the legacy AutoEncoder."""
    if option.rtod_arch(args) == 'legacy':
        return AutoEncoder(norm=args.norm, height=H, width=W)
    return AutoEncoder_2(norm=args.norm, input_dim=3, height=H, width=W)


def _init_from(model, args, rank):
    """--init_from: the fine-tuning entry.  A missing file is an error, never a silent random initialisation."""
    path = getattr(args, "init_from", None)
    if not path:
        return
    if not os.path.isfile(path):
        raise FileNotFoundError("--init_from %r: no such file" % (path,))
    load_checkpoint(model, path)
    if rank == 0:
        print("=> initialised %s from %s" % (type(model).__name__, path))


def _check_resume(args):
    """--resume, checked before anything touches the GPU: it continues a run, so it excludes --init_from (which starts
    one), and a missing file is an error, never a silent fresh start."""
    path = getattr(args, "resume", None)
    if not path:
        return
    if getattr(args, "init_from", None):
        raise RuntimeError("--resume continues a run with its own weights; --init_from starts one: drop one of the two")
    if args.mode in TEST_MODES:
        raise RuntimeError("--resume continues a training run; --mode %s trains nothing" % args.mode)
    if not os.path.isfile(path):
        raise FileNotFoundError("--resume %r: no such file" % (path,))


def _check_ema(args):
    """--ema_decay averages the weights of a training run; checked before anything touches the GPU."""
    if getattr(args, "ema_decay", 0.0) > 0.0 and args.mode in TEST_MODES:
        raise RuntimeError("--ema_decay averages the weights of a training run; --mode %s trains nothing" % args.mode)


def _check_graph(args):
    """--graph replays the step of a training run; checked before anything touches the GPU.  The global BerHu threshold is
    an all-reduce(MAX) inside the loss: with more than one rank it would sit inside the captured forward."""
    if not getattr(args, "graph", False):
        return
    if args.mode in TEST_MODES:
        raise RuntimeError("--graph replays the step of a training run; --mode %s trains nothing" % args.mode)
    if getattr(args, "global_berhu", False) and D.env_rank()[2] > 1:
        raise RuntimeError("--graph with --global_berhu on %d ranks: the threshold's all-reduce(MAX) sits inside the loss and "
                           "no collective may be captured (drop one of the two flags)" % D.env_rank()[2])


def _check_accum(args):
    """--accum_steps groups the batches of a training run; checked before anything touches the GPU."""
    accum = int(getattr(args, "accum_steps", 1) or 1)
    if accum <= 1:
        return
    if args.mode in TEST_MODES:
        raise RuntimeError("--accum_steps accumulates the gradients of a training run; --mode %s trains nothing" % args.mode)
    if getattr(args, "graph", False):
        raise RuntimeError("--graph with --accum_steps %d is not supported yet: a group would need captured graphs of its "
                           "first, middle and last micro-step, which is a follow-up (drop one of the two flags)" % accum)


def _check_schedule(args):
    """--warmup_steps / --lr_schedule / --lr_floor set the rates of a training run; checked before anything touches the GPU.
    (Whether the warm-up fits into the run is the trainer's to say: the run's length needs the loader.)"""
    flag = getattr(args, "lr_schedule", None) or "reference"
    warmup, floor = int(getattr(args, "warmup_steps", 0) or 0), float(getattr(args, "lr_floor", 0.0) or 0.0)
    if flag == "reference" and warmup == 0 and floor == 0.0:
        return
    if args.mode in TEST_MODES:
        raise RuntimeError("--warmup_steps / --lr_schedule / --lr_floor set the learning rate of a training run; --mode %s "
                           "trains nothing" % args.mode)
    if floor != 0.0 and flag not in ("linear", "cosine"):
        raise RuntimeError("--lr_floor %g is where a decay ends, and --lr_schedule %s has none (linear or cosine do)" % (floor, flag))


def _check_optimizer(args):
    """--optimizer / --decoupled_wd pick the update rule of a training run; checked before anything touches the GPU."""
    adamw = (getattr(args, "optimizer", None) or "adam") == "adamw"
    if getattr(args, "decoupled_wd", None) is not None and not adamw:
        raise RuntimeError("--decoupled_wd sets the decoupled weight decay, which --optimizer adamw selects (add it, or drop "
                           "the flag)")
    if adamw and args.mode in TEST_MODES:
        raise RuntimeError("--optimizer adamw is the update rule of a training run; --mode %s trains nothing" % args.mode)


def _check_train_log(args):
    """--train_log / --train_log_every / --tensor_norms_every record a training run; checked before anything touches the GPU."""
    path, every, norms = option.train_log_spec(args)
    if not path:
        given = [k for k in ("train_log_every", "tensor_norms_every") if getattr(args, k, None) is not None]
        if given:
            raise RuntimeError("%s set(s) the cadence of the training log, which --train_log PATH opens (add it, or drop the "
                               "flag)" % ", ".join("--" + k for k in given))
        return
    if args.mode in TEST_MODES:
        raise RuntimeError("--train_log records the steps of a training run; --mode %s trains nothing" % args.mode)
    if every < 1:
        raise RuntimeError("--train_log_every %d: the device ring holds at least one row" % every)
    if norms < 0:
        raise RuntimeError("--tensor_norms_every %d is negative (0: no tensor norms)" % norms)


def _announce_optimizer(args, rank):
    decay = option.decoupled_wd(args)
    if decay is not None and rank == 0:
        print("=> optimizer: AdamW, decoupled weight decay %g%s" %
              (decay, " (0 on the 1-D parameters)" if getattr(args, "no_decay_norm", False) else ""))


def _check_loss(args, train_loader=None):
    """--loss / --silog_*: the pixel term of a training run; checked before anything touches the GPU.  train_loader: the
    loader run() was handed, if any -- one that declares `yields_sparse = False` cannot feed --silog_mask lidar."""
    loss = getattr(args, "loss", None) or "berhu"
    given = [k for k in option.SILOG_DEFAULTS if getattr(args, k, None) is not None]
    if loss != "silog":
        if given:
            raise RuntimeError("%s set(s) the scale-invariant log loss, which --loss silog selects (add it, or drop the flag)"
                               % ", ".join("--" + k for k in given))
        return
    if args.mode in TEST_MODES:
        raise RuntimeError("--loss silog is the pixel term of a training run; --mode %s trains nothing" % args.mode)
    _, lam, weight, floor, lidar = option.pixel_spec(args)
    if not 0.0 <= lam < 1.0:
        raise RuntimeError("--silog_lambda %g is not in [0, 1)" % lam)
    if not (weight > 0.0 and weight != float("inf")):
        raise RuntimeError("--silog_weight %g is not a positive number" % weight)
    if not 0.0 < floor < 1.0:
        raise RuntimeError("--silog_floor %g is not in (0, 1)" % floor)
    if lidar and args.dataset != "KITTI":
        raise RuntimeError("--silog_mask lidar needs the sparse LiDAR map and the Garg box of KITTI; --dataset %s has neither "
                           "(use --silog_mask dense)" % args.dataset)
    if lidar and train_loader is not None and getattr(train_loader, "yields_sparse", True) is False:
        raise RuntimeError("--silog_mask lidar: the training loader (%s) yields no sparse map (use --silog_mask dense)"
                           % type(train_loader).__name__)
    if getattr(args, "global_berhu", False):
        raise RuntimeError("--global_berhu shares the BerHu threshold between ranks and --loss silog has none: every rank "
                           "takes the statistics of its own shard (drop one of the two flags)")


def _check_eval(args):
    """--eval_protocol standard and its flags; checked before anything touches the GPU."""
    spec = option.eval_spec(args)
    if not spec["standard"]:
        given = option.eval_flags_given(args) + option.velo_flags_given(args)
        if given:
            raise RuntimeError("%s set(s) the Eigen-split evaluation, which --eval_protocol standard selects (add it, or drop "
                               "the flag)" % ", ".join("--" + k for k in given))
        return
    if args.dataset != "KITTI":
        raise RuntimeError("--eval_protocol standard is the KITTI Eigen-split protocol; --dataset %s keeps its own metrics "
                           "(drop the flag)" % args.dataset)
    if not (spec["min_depth"] > 0.0 and spec["max_depth"] > spec["min_depth"] and spec["max_depth"] != float("inf")):
        raise RuntimeError("--min_depth %g / --max_depth %g: the cap needs 0 < min_depth < max_depth" % (spec["min_depth"],
                                                                                                       spec["max_depth"]))
    if not (spec["depth_scale"] > 0.0 and spec["depth_scale"] != float("inf")):
        raise RuntimeError("--depth_scale %g is not a positive number" % spec["depth_scale"])
    if spec["gt_list"]:
        if args.mode not in TEST_MODES:
            raise RuntimeError("--eval_gt_list is the ground truth of a test run; --mode %s validates on the loader's "
                               "(use --mode DtoD_test / RtoD_test)" % args.mode)
        if not args.real_test:
            raise RuntimeError("--eval_gt_list lists the ground truth of the Eigen test split: add --real_test")
        if not os.path.isfile(spec["gt_list"]):
            raise FileNotFoundError("--eval_gt_list %r: no such file" % (spec["gt_list"],))
    _check_velodyne(args, spec)


def _check_velodyne(args, spec):
    """--eval_velodyne / --kitti_raw / --velo_depth under --eval_protocol standard."""
    given = option.velo_flags_given(args)
    if not given:
        return
    lst, root = getattr(args, "eval_velodyne", None), getattr(args, "kitti_raw", None)
    if not lst:
        raise RuntimeError("%s belong(s) to --eval_velodyne LIST, which names the scans to project (add it, or drop the "
                           "flag)" % ", ".join("--" + k for k in given))
    if not root:
        raise RuntimeError("--eval_velodyne names scans inside a raw KITTI tree: add --kitti_raw ROOT")
    if spec["gt_list"]:
        raise RuntimeError("--eval_velodyne and --eval_gt_list both supply the ground truth of the test split: drop one of "
                           "the two")
    if args.mode not in TEST_MODES:
        raise RuntimeError("--eval_velodyne is the ground truth of a test run; --mode %s validates on the loader's "
                           "(use --mode DtoD_test / RtoD_test)" % args.mode)
    if not args.real_test:
        raise RuntimeError("--eval_velodyne lists the scans of the Eigen test split: add --real_test")
    if not os.path.isfile(lst):
        raise FileNotFoundError("--eval_velodyne %r: no such file" % (lst,))
    if not os.path.isdir(root):
        raise FileNotFoundError("--kitti_raw %r: no such directory" % (root,))
    from .datasets import TestFolder
    split = os.path.join(str(getattr(args, "data", None)), TestFolder.LISTS[0])
    if not getattr(args, "synthetic", False) and os.path.isfile(split):     # (trainer.validate_std checks any other loader)
        with open(lst) as f:
            lines = sum(1 for line in f if line.strip())
        with open(split) as f:
            samples = sum(1 for line in f if line.split())
        if lines != samples:
            raise RuntimeError("--eval_velodyne names %d scans, the test split has %d samples" % (lines, samples))


def _check_freeze_bn(args):
    """--freeze_bn trains on the stored running statistics; checked before anything touches the GPU."""
    if not getattr(args, "freeze_bn", False):
        return
    if args.mode in TEST_MODES:
        raise RuntimeError("--freeze_bn freezes the BatchNorm statistics of a training run; --mode %s trains nothing" % args.mode)
    if not (getattr(args, "init_from", None) or getattr(args, "resume", None)):
        raise RuntimeError("--freeze_bn needs --init_from or --resume: the running statistics of a fresh network are mean 0 / "
                           "variance 1, and freezing those is a mistake (start from a trained checkpoint, or drop the flag)")


def _freeze_bn(model, args, rank):
    """--freeze_bn on the network being trained (after --init_from; --resume loads into it afterwards)."""
    if getattr(args, "freeze_bn", False):
        model.freeze_bn()
        if rank == 0:
            print("=> %s: normalisation layers frozen on their running statistics" % type(model).__name__)


def _check_partial(args, H, W):
    """--freeze / --lr_mult / --no_decay_norm, checked before anything touches the GPU: the SPECs are matched against the
    trained network's parameter names on a network built without storage."""
    if not _partial(args):
        return
    if args.mode in TEST_MODES:
        raise RuntimeError("--freeze / --lr_mult / --no_decay_norm shape the optimizer of a training run; --mode %s trains "
                           "nothing" % args.mode)
    if getattr(args, "freeze", None) and not (getattr(args, "init_from", None) or getattr(args, "resume", None)):
        raise RuntimeError("--freeze needs --init_from or --resume: freezing the random weights of a fresh network is a "
                           "mistake (start from a trained checkpoint, or drop the flag)")
    with torch.device("meta"), contextlib.redirect_stdout(io.StringIO()):
        net = AutoEncoder_DtoD(norm=args.norm, input_dim=1, height=H, width=W) if args.mode == 'DtoD' else _rtod_network(args, H, W)
    try:
        if getattr(args, "freeze", None):
            net.freeze(args.freeze)
    except U.GdnError as e:
        raise RuntimeError("--freeze %s: %s" % (",".join(args.freeze), e))
    param_groups(net, args)              # (an --lr_mult SPEC that selects nothing)


def _freeze(model, args, rank):
    """--freeze on the network being trained (before the optimizer is built; --resume loads into it afterwards)."""
    if getattr(args, "freeze", None):
        frozen = model.freeze(args.freeze)
        if rank == 0:
            print("=> %s: %d of %d parameter tensors frozen (%s)" % (type(model).__name__, len(frozen),
                                                                  sum(1 for _ in model.parameters()), ",".join(args.freeze)))


def _resume(args, model, opt, train_loader, rank):
    """--resume: weights, optimizer, loader and progress from the state file; None without the flag."""
    path = getattr(args, "resume", None)
    if not path:
        return None
    progress = load_training_state(read_training_state(path), model, opt, train_loader)
    if rank == 0:
        print("=> resumed %s from %s: epoch %d, batch %d, step %d, lr %g" % (type(model).__name__, path, progress["epoch"] + 1,
                                                                         progress["i"] + 1, progress["step"], progress["lr"]))
    return progress


def _check_dataset(args):
    """What the file pipeline can read, checked before anything touches the GPU."""
    resident = getattr(args, "resident", False)
    if resident and args.synthetic:
        raise RuntimeError("--resident keeps a set of FILES in device memory; it does not apply to --synthetic batches "
                           "(drop one of the two flags)")
    if args.synthetic:
        return
    if resident and args.dataset != "KITTI":
        raise RuntimeError("--resident is implemented for the KITTI file pipeline only (the NYU resident loader, "
                           "datasets.GpuNYUResidentLoader, is handed to run() like the NYU training loader)")
    if args.dataset == "Make3D":
        raise RuntimeError("--dataset Make3D is not supported: the reference's Make3D loader resizes with cv2.INTER_AREA "
                           "to 232x176, a size the U-Net cannot take (compute_errors_Make3D itself is available in "
                           "gdn_amd.calculate_error)")
    if args.dataset == "NYU" and args.mode not in TEST_MODES:
        raise RuntimeError("--dataset NYU is implemented for evaluation only (--mode DtoD_test / RtoD_test); NYU training "
                           "is out of scope")
    if args.dataset not in ("KITTI", "NYU"):
        raise RuntimeError("unknown --dataset %r (KITTI, NYU)" % (args.dataset,))


class ImageSaver:
    """--img_save (GDN_main.py:268-307): for every test image, in loader order, result_dir/output_depth/final_AE_depth_%05d.jpg,
    ground_truth/final_AE_gt_%05d.jpg and input_rgb/final_AE_rgb_%05d.jpg, bytescaled on the GPU like scipy.misc.imsave
    and written by PIL as JPEG with its default quality.  Called with each validation batch (no second forward pass)."""

    FOLDERS = (("output_depth", "final_AE_depth_"), ("ground_truth", "final_AE_gt_"), ("input_rgb", "final_AE_rgb_"))

    def __init__(self, result_dir):
        self.dirs = [os.path.join(result_dir, f) for f, _ in self.FOLDERS]
        for d in self.dirs:
            os.makedirs(d, exist_ok=True)
        self.k = 0

    def __call__(self, depth, img, depth_np, out):
        from PIL import Image
        from . import ops
        for t, d, (_, name) in zip((out, depth, img), self.dirs, self.FOLDERS):
            u8 = ops.bytescale_u8(t.detach().float()).cpu().numpy()
            for i in range(u8.shape[0]):
                im = u8[i, :, :, 0] if u8.shape[3] == 1 else u8[i]
                Image.fromarray(im).save(os.path.join(d, name + '%05d.jpg' % (self.k + i)))
        self.k += out.shape[0]


def run(args, train_loader=None, val_loader=None):
    if train_loader is None:
        _check_dataset(args)
    _check_resume(args)
    _check_ema(args)
    _check_graph(args)
    _check_accum(args)
    _check_schedule(args)
    _check_optimizer(args)
    _check_train_log(args)
    _check_loss(args, train_loader)
    _check_freeze_bn(args)
    _check_eval(args)
    _check_partial(args, args.height, args.width)
    rank, local_rank, world = D.env_rank()
    if world == 1 and "HIP_VISIBLE_DEVICES" not in os.environ and not torch.cuda.is_initialized():
        os.environ["HIP_VISIBLE_DEVICES"] = args.gpu_num.split(",")[0]   # reference: CUDA_VISIBLE_DEVICES=--gpu_num
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: the MI355X build has no CPU fallback")
    rank, local_rank, world = D.init()
    dev = torch.device("cuda", local_rank if world > 1 else 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(args.seed)          # identical init on every rank
    from . import utils as _U
    _U.GLOBAL_BERHU = bool(getattr(args, "global_berhu", False))
    H, W = args.height, args.width
    if rank == 0:
        print('=> number of GPU processes: ', world)
        print("=> creating model")
    if train_loader is None:
        from .datasets import GpuAugmentLoader, GpuResidentLoader, SequenceFolder, SyntheticRawKitti
        steps = args.epoch_size or 100
        file_loader, budget = GpuAugmentLoader, {}
        if getattr(args, "resident", False):
            # --resident: every rank preloads the whole set (its shard of the common shuffle changes every epoch)
            gb = getattr(args, "resident_gb", None)
            file_loader, budget = GpuResidentLoader, {"max_bytes": None if gb is None else int(gb * 1e9)}
        if not args.synthetic and os.path.isdir(str(args.data)) and args.mode in TEST_MODES and \
                (args.dataset == "NYU" or args.real_test):
            # evaluation only: the NYU test set (datasets_list.py:366-444) or the Eigen test split (:111-189); no train set
            from .datasets import GpuCropLoader, NYUdataset, TestFolder
            if args.dataset == "NYU":
                val_loader = GpuCropLoader(NYUdataset(args.data, args, seed=args.seed, train=False, mode=args.mode),
                                           args.batch_size, dev, H, W, workers=args.workers)
            else:
                val_loader = file_loader(TestFolder(args.data, args, seed=args.seed, train=False, mode=args.mode),
                                         args.batch_size, dev, train=False, workers=args.workers, **budget)
            train_loader = val_loader
            if rank == 0:
                print("=> test on %s: %d samples" % ("the NYU Depth v2 test set" if args.dataset == "NYU"
                                                     else "the Eigen test split", len(val_loader.ds)))
        elif not args.synthetic and os.path.isdir(str(args.data)):
            # the reference's file layout (datasets_list.py:61-76); decode on the host, augment on the GPU
            if args.dataset != "KITTI":
                raise RuntimeError("only the KITTI pipeline (GDN_main.py:56-80) is implemented; NYU is out of scope")
            train_set = SequenceFolder(args.data, args, seed=args.seed, train=True, mode=args.mode)     # same file order on every rank
            if args.real_test:          # GDN_main.py:70-79: validate on the Eigen test split
                from .datasets import TestFolder
                val_set = TestFolder(args.data, args, seed=args.seed, train=False, mode=args.mode)
            else:
                val_set = SequenceFolder(args.data, args, seed=args.seed, train=False, mode=args.mode)
            # data parallelism: a common shuffle, rank r takes samples r, r + world, ... (each sample once per epoch);
            # --batch_size is per GPU, so the global batch is world * batch_size at the given learning rate
            train_loader = file_loader(train_set, args.batch_size, dev, train=True, seed=args.seed + rank,
                                       workers=args.workers, drop_last=True, rank=rank, world=world,
                                       order_seed=args.seed + 1, **budget)
            val_loader = file_loader(val_set, args.batch_size, dev, train=False, workers=args.workers, **budget)
        elif not args.synthetic:
            raise RuntimeError("dataset directory %r not found; pass a KITTI root laid out like the reference's "
                               "(train.txt, val.txt, <scene>/*.jpg, color_gt2/, gt/) or --synthetic" % (args.data,))
        elif getattr(args, "augment", False):
            # synthetic RAW uint8 samples through the same GPU augmentation the file pipeline uses
            raw = SyntheticRawKitti(args.batch_size * min(steps, 8), H, W, seed=args.seed + rank)
            train_loader = GpuAugmentLoader(raw, args.batch_size, dev, train=True, seed=args.seed + rank, drop_last=True)
            val_loader = GpuAugmentLoader(SyntheticRawKitti(args.batch_size * 2, H, W, seed=args.seed + 1000 + rank),
                                          args.batch_size, dev, train=False)
        else:
            train_loader = SyntheticLoader(args.batch_size, steps, H, W, seed=args.seed + rank, device=dev)
            val_loader = SyntheticLoader(args.batch_size, 2, H, W, seed=args.seed + 1000 + rank, device=dev)
    if args.epoch_size == 0:
        args.epoch_size = len(train_loader)
    args.local_rank = local_rank
    logger = object() if args.evaluate else None     # reference: validation only when --evaluate

    if args.mode == 'DtoD':
        G = AutoEncoder_DtoD(norm=args.norm, input_dim=1, height=H, width=W).to(dev).compute_dtype(args.dtype)
        _init_from(G, args, rank)
        _freeze_bn(G, args, rank)
        _freeze(G, args, rank)
        D.broadcast_parameters(G)             # rank 0's weights / BN buffers everywhere (identical seeds make this a no-op)
        opt = _make_optimizer(G, args)
        _announce_optimizer(args, rank)
        loss = train_AE_DtoD(args, G, None, None, opt, train_loader, val_loader, args.batch_size, args.epochs,
                             args.lr, logger, None, progress=_resume(args, G, opt, train_loader, rank))
        if rank == 0 and loss is not None:
            print('Final loss:', loss.item())
        return loss
    if args.mode in ('RtoD', 'RtoD_single'):
        G = None
        if args.mode == 'RtoD':
            G = AutoEncoder_DtoD(norm=args.norm, input_dim=1, height=H, width=W).to(dev).compute_dtype(args.dtype)
            if os.path.exists(args.model_dir):
                load_checkpoint(G, args.model_dir)
            elif rank == 0:
                print("=> no guide checkpoint at %s: using a randomly initialised guide" % args.model_dir)
            G.eval()
            if getattr(args, "latent_grad", False):
                G.requires_grad_(False)       # the guide only passes d(latent)/d(outputs) through
        R = _rtod_network(args, H, W).to(dev).compute_dtype(args.dtype)
        _init_from(R, args, rank)
        _freeze_bn(R, args, rank)
        _freeze(R, args, rank)
        D.broadcast_parameters(R)
        opt = _make_optimizer(R, args)
        _announce_optimizer(args, rank)
        return train_AE_RtoD(args, R, G, None, None, opt, train_loader, val_loader, args.batch_size, args.epochs,
                             args.lr, logger, None, progress=_resume(args, R, opt, train_loader, rank))
    if args.mode in ('DtoD_test', 'RtoD_test'):
        if args.mode == 'DtoD_test':
            model = AutoEncoder_DtoD(norm=args.norm, input_dim=1, height=H, width=W).to(dev).compute_dtype(args.dtype)
            ckpt = args.model_dir
        else:
            model = _rtod_network(args, H, W).to(dev).compute_dtype(args.dtype)
            ckpt = args.RtoD_model_dir
        if os.path.exists(ckpt):
            load_checkpoint(model, ckpt)
        model.eval()
        saver = ImageSaver(args.result_dir) if args.img_save and rank == 0 else None
        spec = option.eval_spec(args)
        if spec["standard"]:
            # the Eigen-split protocol; --eval_gt_list: the 16-bit maps at their native size
            gt16 = None
            if spec["gt_list"]:
                from .datasets import EigenGt16
                gt16 = EigenGt16(spec["gt_list"], args.data)
            # --eval_velodyne: the raw scans, projected on the device batch by batch
            vspec, velo = option.velo_spec(args), None
            if vspec:
                from .datasets import EigenVelodyne
                velo = EigenVelodyne(vspec["list"], vspec["root"], vspec["depth"])
            errors, left_out, names = validate_std(args, val_loader, model, 0, logger, args.mode, on_batch=saver, gt16=gt16,
                                                   velo=velo)
            if rank == 0:
                print("Results: " + ", ".join("%s %.4f" % (n, e) for n, e in zip(names, errors)) +
                      " [standard: %s; %d image(s) left out]" % (option.eval_describe(spec, vspec), left_out))
            return errors
        evaluate = validate_NYU if args.dataset == "NYU" else validate
        errors, min_errors, names = evaluate(args, val_loader, model, 0, logger, args.mode, on_batch=saver)
        if rank == 0:
            print("Results: " + ", ".join("%s %.4f" % (n, e) for n, e in zip(names, errors)))
        return errors
    raise ValueError("unknown --mode %r" % args.mode)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = option.parse_args(argv)
    devices = [d for d in str(args.gpu_num).split(",") if d != ""]
    if len(devices) > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        # the reference's `--gpu_num 0,1,2,3` (README.md:82): one process per listed GPU, started before anything here
        # touches the GPU; this parent only waits and propagates a failure
        rc = D.launch_ranks(argv, devices)
        if rc != 0:
            sys.exit(rc)
        return None
    return run(args)


if __name__ == '__main__':
    main(sys.argv[1:])
