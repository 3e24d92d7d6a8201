"""Command-line flags: every flag name and default of the reference's option.py:5-48,
plus the few the MI355X build adds (--synthetic, --local_rank, --dtype, --global_berhu, --resident, --rtod_arch,
--init_from, --save_state, --save_state_every, --resume, --clip_grad_norm, --skip_nonfinite, --ema_decay, --graph,
--graph_warmup, --accum_steps, --freeze_bn, --freeze, --lr_mult, --no_decay_norm, --warmup_steps, --lr_schedule,
--lr_floor, --loss, --silog_lambda, --silog_weight, --silog_floor, --silog_mask, --eval_protocol, --eval_crop, --min_depth,
--max_depth, --depth_scale, --median_scaling, --flip_test, --eval_gt_list, --optimizer, --decoupled_wd, --train_log,
--train_log_every, --tensor_norms_every, --eval_velodyne, --kitti_raw, --velo_depth).

Unlike the reference the parser is not evaluated at import time; call ``parse_args()``.
"""
import argparse


def _non_negative_float(text):
    v = float(text)
    if not v >= 0.0:
        raise argparse.ArgumentTypeError("%r is not a non-negative number" % (text,))
    return v


def _ema_decay(text):
    v = float(text)
    if not 0.0 <= v < 1.0:
        raise argparse.ArgumentTypeError("%r is not a decay in [0, 1)" % (text,))
    return v


def _positive_int(text):
    v = int(text)
    if v < 1:
        raise argparse.ArgumentTypeError("%r is not a positive integer" % (text,))
    return v


def _non_negative_int(text):
    v = int(text)
    if v < 0:
        raise argparse.ArgumentTypeError("%r is not a non-negative integer" % (text,))
    return v


def _unit_float(text):
    v = float(text)
    if not 0.0 <= v <= 1.0:
        raise argparse.ArgumentTypeError("%r is not a number in [0, 1]" % (text,))
    return v


def freeze_specs(text):
    """--freeze: 'SPEC[,SPEC...]' -> [SPEC, ...] (encoder, decoder or fnmatch patterns on parameter names)."""
    specs = [s.strip() for s in text.split(",")]
    if not text.strip() or not all(specs):
        raise argparse.ArgumentTypeError("%r is not a comma-separated list of SPECs (encoder, decoder or a name pattern)" % (text,))
    return specs


def lr_mults(text):
    """--lr_mult: 'SPEC=M[,SPEC=M...]' -> [(SPEC, M), ...] in the order given (later entries win), M >= 0."""
    out = []
    for entry in text.split(","):
        spec, sep, mult = entry.rpartition("=")
        try:
            m = float(mult)
        except ValueError:
            m = -1.0
        if not sep or not spec.strip() or not m >= 0.0 or m == float("inf"):
            raise argparse.ArgumentTypeError("%r is not SPEC=M with a multiplier M >= 0" % (entry,))
        out.append((spec.strip(), m))
    return out


def build_parser():
    p = argparse.ArgumentParser(description='Depth AutoEncoder training on KITTI (MI355X-native hot path)',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('data', metavar='DIR', nargs='?', default='synthetic', help='path to dataset')
    p.add_argument('--dataset-format', default='sequential', metavar='STR', help='dataset format')
    p.add_argument('-j', '--workers', default=0, type=int, metavar='N', help='number of data loading workers')
    p.add_argument('--epochs', default=200, type=int, metavar='N', help='number of total epochs to run')
    p.add_argument('--epoch_size', default=0, type=int, metavar='N', help='manual epoch size')
    p.add_argument('--batch_size', default=24, type=int, metavar='N', help='mini-batch size (per GPU)')
    p.add_argument('--lr', default=0.00002, type=float, metavar='LR', help='initial learning rate')
    p.add_argument('--momentum', default=0.9, type=float, metavar='M', help='alpha parameter for adam')
    p.add_argument('--beta', default=0.999, type=float, metavar='M', help='beta parameters for adam')
    p.add_argument('--weight-decay', '--wd', default=0, type=float, metavar='W',
                   help='accepted for compatibility; like the reference the optimiser uses 5e-4')
    p.add_argument('--print-freq', default=10, type=int, metavar='N', help='print frequency')
    p.add_argument('-e', '--evaluate', dest='evaluate', action='store_true', help='evaluate model on validation set')
    p.add_argument('-i', '--img_test', dest='img_test', action='store_true', help='img test on validation set')
    p.add_argument('-r', '--real_test', dest='real_test', action='store_true', help='test on Eigen test split')
    p.add_argument('--seed', default=0, type=int, help='seed for random functions, and network initialization')
    p.add_argument('--log-summary', default='progress_log_summary.csv', metavar='PATH')
    p.add_argument('--log-full', default='progress_log_full.csv', metavar='PATH')
    p.add_argument('--result_dir', type=str, default='./AE_results')
    p.add_argument('--model_dir', type=str, default='./AE_trained_model_lr0000')
    p.add_argument('--RtoD_model_dir', type=str,
                   default='./AE_RtoD_trained_model_lr0004_color_nonMulti/epoch_18_AE_depth_loss_0.2561.pkl')
    p.add_argument('--gpu_num', type=str, default="2")
    p.add_argument('--norm', type=str, default="Batch")
    p.add_argument('--mode', type=str, default="DtoD")
    p.add_argument('--height', type=int, default=128)
    p.add_argument('--width', type=int, default=416)
    p.add_argument('--dataset', type=str, default="KITTI")
    p.add_argument('--img_save', action='store_true', help='result image save')
    # --- additions of this build ---
    p.add_argument('--synthetic', action='store_true', help='train on synthetic KITTI-shaped batches (no dataset)')
    p.add_argument('--local_rank', type=int, default=0, help='set by the launcher; RANK/LOCAL_RANK env win')
    p.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16'],
                   help='activation / MFMA operand storage type: fp32 (the reference\'s) or bf16 with fp32 accumulation, '
                        'fp32 master weights, BatchNorm statistics, losses and Adam')
    p.add_argument('--augment', action='store_true',
                   help='with --synthetic: feed synthetic RAW uint8 samples through the GPU augmentation kernel '
                        '(flip / scale-crop / normalise) instead of ready-made tensors')
    p.add_argument('--latent_grad', action='store_true',
                   help='RtoD: let the latent loss back-propagate through the frozen guide into the trained network '
                        '(the guided training of the paper; the reference as shipped computes it under no_grad, value only)')
    p.add_argument('--faithful_guide', action='store_true',
                   help='RtoD: run the frozen guide as two full forwards like the reference (default: one '
                        'batched encoder-only pass, identical features)')
    p.add_argument('--global_berhu', action='store_true',
                   help='all-reduce(MAX) the BerHu threshold like DataParallel\'s gathered batch (SURVEY 8(e))')
    p.add_argument('--resident', action='store_true',
                   help='KITTI file pipeline: decode every file once, keep the raw images in device memory and assemble each '
                        'batch there (one kernel launch and one small copy per batch instead of decoding 3 x batch_size files)')
    p.add_argument('--resident_gb', type=float, default=None, metavar='GB',
                   help='with --resident: the most device memory (GB, 1e9 bytes) one preloaded set may take '
                        '(default: half of the free memory)')
    p.add_argument('--rtod_arch', default=None, choices=['unet', 'legacy'],
                   help='colour-to-depth network of the RtoD modes: unet = AutoEncoder_2, legacy = AutoEncoder (the network of '
                        'the published GDN_RtoD_pretrained.pkl).  Default: what each mode always built -- unet for RtoD / '
                        'RtoD_single, legacy for RtoD_test')
    p.add_argument('--init_from', type=str, default=None, metavar='PATH',
                   help='DtoD / RtoD / RtoD_single: load this state dict (reference format with module. prefixes, or bare) into '
                        'the network being trained before the first step -- fine-tuning; a missing file is an error')
    p.add_argument('--save_state', action='store_true',
                   help='training: whenever a weight checkpoint is written, also write the rolling <save_dir>/train_state.pt '
                        '(weights, Adam moments and step state, loader position and RNG streams, epoch / iteration / learning '
                        'rate: about three times the weights, and one more copy of them with --ema_decay) that --resume continues '
                        'from')
    p.add_argument('--save_state_every', type=int, default=0, metavar='N',
                   help='training: also write train_state.pt every N iterations (counted over the whole run)')
    p.add_argument('--resume', type=str, default=None, metavar='PATH',
                   help='DtoD / RtoD / RtoD_single: continue the run that wrote this train_state.pt, bit for bit as if it had '
                        'never stopped (same command line otherwise); a missing file is an error, and so is --init_from with it')
    p.add_argument('--clip_grad_norm', type=_non_negative_float, default=0.0, metavar='X',
                   help='training: clip the global gradient norm (all parameters, after the data-parallel mean) to X before '
                        'the Adam update, on the device (torch.nn.utils.clip_grad_norm_\'s formula); 0 = off')
    p.add_argument('--skip_nonfinite', action='store_true',
                   help='training: a step whose gradient holds a NaN or an Inf leaves weights, Adam moments and the step '
                        'count untouched (decided on the device, no sync); the progress prints count such steps')
    p.add_argument('--ema_decay', type=_ema_decay, default=0.0, metavar='D',
                   help='training: keep an exponential moving average of the weights inside the fused Adam (decay D, warmed up '
                        'as min(D, (1 + t) / (10 + t)) over the applied steps t; a skipped step leaves it alone); the per-epoch '
                        'validation runs on the averaged weights and every X.pkl is followed by X_ema.pkl with them.  BatchNorm '
                        'running statistics are buffers, not parameters: the averaged model uses the live ones (as torch\'s '
                        'AveragedModel(use_buffers=False) does), no update_bn pass is made; 0 = off')
    p.add_argument('--graph', action='store_true',
                   help='training: capture the step (forward, losses, backward, fused Adam) as a hipGraph after the first '
                        '--graph_warmup eager steps and replay it from then on: one graph launch per step on one GPU, two '
                        'around the eager gradient all-reduce with data parallelism (which then no longer overlaps backward). '
                        'The run is bit for bit the run without the flag; a batch of another shape runs eagerly')
    p.add_argument('--graph_warmup', type=_positive_int, default=3, metavar='N',
                   help='with --graph: eager steps (on their own batches) of a run or a resumed run before the capture')
    p.add_argument('--accum_steps', type=_positive_int, default=1, metavar='K',
                   help='training: accumulate the gradients of K loader batches (by position within the epoch; the group an '
                        'epoch ends with may be shorter) and apply their mean in one Adam update: the effective batch is '
                        'K x batch_size x ranks at the given learning rate, with one gradient all-reduce per update.  '
                        'BatchNorm statistics and the BerHu threshold stay per batch, as they are per replica under data '
                        'parallelism; not with --graph yet; 1 = off')
    p.add_argument('--freeze_bn', action='store_true',
                   help='training (with --init_from or --resume): fine-tune on the stored BatchNorm running statistics -- every '
                        'normalisation layer of the trained network stays in eval mode, normalises by its running mean / '
                        'variance and never updates them, while the conv weights and the affine gamma / beta train; the flag is '
                        'not stored in train_state.pt, a resumed run repeats it')
    p.add_argument('--freeze', type=freeze_specs, default=[], metavar='SPEC[,SPEC...]',
                   help='training (with --init_from or --resume): do not train the selected parameters.  A SPEC is encoder '
                        '(every layer the forward runs before upconv0), decoder (the rest) or an fnmatch pattern on parameter '
                        'names (state_dict keys without module.).  The fused Adam skips them in its one launch and the backward '
                        'does no work below the lowest trainable layer.  Normalisation layers keep their mode, as in torch: '
                        'add --freeze_bn to hold their running statistics.  Not stored in train_state.pt, a resumed run '
                        'repeats it')
    p.add_argument('--lr_mult', type=lr_mults, default=[], metavar='SPEC=M[,SPEC=M...]',
                   help='training: the selected parameters (SPEC as for --freeze) train at M x the learning rate, M >= 0; '
                        'later entries win, parameters no entry selects keep 1.  The schedule decays --lr, the multipliers '
                        'stay.  Not stored in train_state.pt, a resumed run repeats it')
    p.add_argument('--no_decay_norm', action='store_true',
                   help='training: every 1-D parameter (BatchNorm / InstanceNorm gamma, beta) takes weight decay 0 instead of '
                        'the 5e-4 the reference applies to it too (with --optimizer adamw: instead of --decoupled_wd, the '
                        'usual AdamW practice).  Not stored in train_state.pt, a resumed run repeats it')
    p.add_argument('--warmup_steps', type=_non_negative_int, default=0, metavar='W',
                   help='training: the first W Adam updates run at (u + 1) / W of the learning rate (u = 0, 1, ... counts '
                        'APPLIED updates: a step --skip_nonfinite drops does not advance it), every --lr_mult group at its own '
                        'multiple.  Evaluated on the device in front of the fused Adam, so --graph replays it; 0 = off')
    p.add_argument('--lr_schedule', default='reference', choices=['reference', 'constant', 'linear', 'cosine'],
                   help='training: what follows the warm-up.  reference: the hand-rolled decay of the reference (after epoch 2 / '
                        '5, every 1900 / 2200 batches), as ever.  constant / linear / cosine: that decay is off and the device '
                        'holds --lr, or takes it from --lr to --lr_floor x --lr over the run, linearly or along half a cosine; '
                        'the run\'s length is counted in updates, epochs x ceil(epoch_size / accum_steps).  Stored in '
                        'train_state.pt: a resumed run must repeat it')
    p.add_argument('--lr_floor', type=_unit_float, default=0.0, metavar='F',
                   help='with --lr_schedule linear / cosine: the share of --lr the decay ends at, in [0, 1]')
    p.add_argument('--loss', default='berhu', choices=['berhu', 'silog'],
                   help='training: the pixel term of the loss.  berhu: the reference\'s masked BerHu, as ever.  silog: the '
                        'scale-invariant log loss weight x sqrt(mean(d^2) - lambda x mean(d)^2), d = log depth(out) - log '
                        'depth(gt) over the valid pixels (DESIGN.md 3.10), in its place; the Sobel / smoothness / latent terms '
                        'stay.  Every rank takes the statistics of its own shard.  Not stored in train_state.pt, a resumed run '
                        'repeats it')
    p.add_argument('--silog_lambda', type=float, default=None, metavar='L',
                   help='with --loss silog: the variance-focus weight, in [0, 1) (when not given: 0.85)')
    p.add_argument('--silog_weight', type=float, default=None, metavar='X',
                   help='with --loss silog: the factor in front of the square root, > 0 (when not given: 10)')
    p.add_argument('--silog_floor', type=float, default=None, metavar='F',
                   help='with --loss silog: depths are clamped from below at F x the range before the logarithm and a pixel '
                        'whose ground truth is not above it is left out, in (0, 1) (when not given: 0.0125, 1 m of 80 m)')
    p.add_argument('--silog_mask', default=None, choices=['dense', 'lidar'],
                   help='with --loss silog: dense = every pixel whose ground truth is above the floor; lidar = only pixels '
                        'inside the Garg box that carry a LiDAR return (KITTI only) (when not given: dense)')
    p.add_argument('--eval_protocol', default='reference', choices=['reference', 'standard'],
                   help='how KITTI is evaluated (test modes and the per-epoch validation).  reference: the reference\'s '
                        'compute_errors, as ever.  standard: the Eigen-split protocol of the literature (DESIGN.md 3.12) -- '
                        'metric depth, the --min_depth / --max_depth cap, the --eval_crop box, evaluated at the ground '
                        'truth\'s own resolution, nine metrics averaged per image')
    # (the flags below default to None so that one given without --eval_protocol standard can be refused; eval_spec()
    # resolves them: garg, 1e-3, 80, 80)
    p.add_argument('--eval_crop', default=None, choices=['garg', 'eigen', 'none'],
                   help='with --eval_protocol standard: the evaluation crop (when not given: garg)')
    p.add_argument('--min_depth', type=float, default=None, metavar='M',
                   help='with --eval_protocol standard: ground truth at or below M metres is left out and the prediction is '
                        'clamped to it, > 0 (when not given: 1e-3)')
    p.add_argument('--max_depth', type=float, default=None, metavar='M',
                   help='with --eval_protocol standard: the cap, likewise (when not given: 80)')
    p.add_argument('--depth_scale', type=float, default=None, metavar='M',
                   help='with --eval_protocol standard: the depth in metres that the network\'s +1 stands for (when not '
                        'given: 80)')
    p.add_argument('--median_scaling', action='store_true',
                   help='with --eval_protocol standard: scale each prediction by median(gt) / median(prediction) over its '
                        'valid pixels before the metrics')
    p.add_argument('--flip_test', action='store_true',
                   help='with --eval_protocol standard: evaluate the mean of the prediction and the mirrored prediction of '
                        'the mirrored input (two forwards per batch); --img_save then writes the merged map')
    p.add_argument('--eval_gt_list', type=str, default=None, metavar='FILE',
                   help='with --eval_protocol standard, a test mode and --real_test: one 16-bit KITTI depth PNG (metres x '
                        '256) per test sample, at its native size, as the ground truth; the network\'s inputs stay what '
                        'the test lists feed it')
    p.add_argument('--eval_velodyne', type=str, default=None, metavar='LIST',
                   help='with --eval_protocol standard, a test mode and --real_test: the ground truth is projected on the '
                        'device from the raw Velodyne scan of each test sample (DESIGN.md 3.15), at the camera\'s native '
                        'size.  LIST names one sample per line, DATE/DRIVE/image_0C/data/FRAME.png or DATE/DRIVE FRAME l|r, '
                        'in the order of the test lists; needs --kitti_raw, excludes --eval_gt_list')
    p.add_argument('--kitti_raw', type=str, default=None, metavar='ROOT',
                   help='with --eval_velodyne: the raw KITTI tree (ROOT/DATE/calib_*.txt, '
                        'ROOT/DATE/DRIVE/velodyne_points/data/*.bin)')
    p.add_argument('--velo_depth', default=None, choices=['camera', 'forward'],
                   help='with --eval_velodyne: camera = the depth along the camera\'s axis, as the 2017-2019 Eigen-split '
                        'tables use it; forward = the scanner\'s forward distance, monodepth2\'s export (when not given: '
                        'camera)')
    p.add_argument('--optimizer', default='adam', choices=['adam', 'adamw'],
                   help='training: the update rule of the fused optimizer.  adam: the reference\'s Adam with its L2 term of '
                        '5e-4 folded into the gradient, as ever.  adamw: decoupled weight decay (DESIGN.md 3.13) -- the decay '
                        'stays out of the gradient and the moments and shrinks the weight at the update\'s own rate, inside '
                        'the same launches.  Stored with the optimizer state in train_state.pt: a resumed run must repeat it')
    # (None so that the flag given without --optimizer adamw can be refused; decoupled_wd() resolves it)
    p.add_argument('--decoupled_wd', type=_non_negative_float, default=None, metavar='W',
                   help='with --optimizer adamw: the decoupled weight decay, >= 0 (when not given: 1e-2, torch.optim.AdamW\'s '
                        'default, a common choice that is not tuned here); --no_decay_norm takes it off the 1-D parameters')
    p.add_argument('--train_log', type=str, default=None, metavar='PATH',
                   help='training: write a JSON-lines record of every step to PATH (DESIGN.md 3.14): the loss terms, the '
                        'update count, the rate, the gradient norm, the clip coefficient and the skip decision, copied on the '
                        'device by one small launch per step (part of the --graph replay) and read by the host once every '
                        '--train_log_every steps.  The update columns are null where the run keeps no such device record '
                        '(no gradient guard, a host-stepped optimizer, a micro-batch inside an open --accum_steps group): '
                        '--skip_nonfinite alone gives the norm column without clipping.  Rank 0 writes, of its own shard; a '
                        'fresh run overwrites PATH, --resume continues it.  Summary: python -m gdn_amd.trainlog PATH')
    # (None so that either cadence flag given without --train_log can be refused; train_log_spec() resolves them)
    p.add_argument('--train_log_every', type=int, default=None, metavar='N',
                   help='with --train_log: rows the device ring holds, which is also how often it is copied to the host, '
                        '>= 1 (when not given: %d)' % TRAIN_LOG_EVERY_DEFAULT)
    p.add_argument('--tensor_norms_every', type=int, default=None, metavar='M',
                   help='with --train_log: every M steps also record the norm of every parameter tensor and of its gradient '
                        '(as the update saw it), one deterministic pass over the arena; 0 or not given: off')
    return p


TRAIN_LOG_EVERY_DEFAULT = 256


def train_log_spec(args):
    """(path or None, --train_log_every, --tensor_norms_every) with the cadence flags that were not given at their defaults."""
    every, norms = getattr(args, "train_log_every", None), getattr(args, "tensor_norms_every", None)
    return (getattr(args, "train_log", None) or None, TRAIN_LOG_EVERY_DEFAULT if every is None else int(every),
            0 if norms is None else int(norms))


DECOUPLED_WD_DEFAULT = 1e-2


def decoupled_wd(args):
    """None for --optimizer adam; for --optimizer adamw the decoupled weight decay, the flag not given at its default."""
    if (getattr(args, 'optimizer', None) or 'adam') != 'adamw':
        return None
    w = getattr(args, 'decoupled_wd', None)
    return DECOUPLED_WD_DEFAULT if w is None else float(w)


EVAL_DEFAULTS = {'eval_crop': 'garg', 'min_depth': 1e-3, 'max_depth': 80.0, 'depth_scale': 80.0}
EVAL_SWITCHES = ('median_scaling', 'flip_test', 'eval_gt_list')


def eval_spec(args):
    """The evaluation protocol as a dict: 'standard' (False: the reference's compute_errors, as ever) and, flags not given
    at their defaults, 'crop', 'min_depth', 'max_depth', 'depth_scale', 'median_scaling', 'flip_test', 'gt_list'."""
    v = {k: d if getattr(args, k, None) is None else getattr(args, k) for k, d in EVAL_DEFAULTS.items()}
    return {'standard': (getattr(args, 'eval_protocol', None) or 'reference') == 'standard', 'crop': v['eval_crop'],
            'min_depth': float(v['min_depth']), 'max_depth': float(v['max_depth']), 'depth_scale': float(v['depth_scale']),
            'median_scaling': bool(getattr(args, 'median_scaling', False)), 'flip_test': bool(getattr(args, 'flip_test', False)),
            'gt_list': getattr(args, 'eval_gt_list', None)}


def eval_flags_given(args):
    """The names of the --eval_protocol standard flags the command line sets."""
    return [k for k in EVAL_DEFAULTS if getattr(args, k, None) is not None] + \
           [k for k in EVAL_SWITCHES if getattr(args, k, None)]


VELO_FLAGS = ('eval_velodyne', 'kitti_raw', 'velo_depth')


def velo_spec(args):
    """--eval_velodyne beside eval_spec(): None without the flag, else {'list', 'root', 'depth'} with --velo_depth not given
    at its default (camera)."""
    if not getattr(args, 'eval_velodyne', None):
        return None
    return {'list': args.eval_velodyne, 'root': getattr(args, 'kitti_raw', None),
            'depth': getattr(args, 'velo_depth', None) or 'camera'}


def velo_flags_given(args):
    """The names of the --eval_velodyne flags the command line sets."""
    return [k for k in VELO_FLAGS if getattr(args, k, None)]


def eval_describe(spec, velo=None):
    """What a result line of the standard protocol says about itself (velo: velo_spec() of the same command line)."""
    if velo:
        gt = 'Velodyne scans projected on the device (%s, %s)' % (velo['list'], velo['depth'])
    elif spec['gt_list']:
        gt = '16-bit maps at native size (%s)' % spec['gt_list']
    else:
        gt = "the loader's, at the network's size"
    return "crop %s, cap %g-%g m, depth_scale %g m, median scaling %s, flip %s, gt %s" % (
        spec['crop'], spec['min_depth'], spec['max_depth'], spec['depth_scale'], 'on' if spec['median_scaling'] else 'off',
        'on' if spec['flip_test'] else 'off', gt)


SILOG_DEFAULTS = {'silog_lambda': 0.85, 'silog_weight': 10.0, 'silog_floor': 0.0125, 'silog_mask': 'dense'}


def pixel_spec(args):
    """None for --loss berhu; for --loss silog the spec utils.dtod_loss / rtod_pixel_loss take as `pixel`:
    ('silog', lambda, weight, floor, use_sparse), flags not given at their defaults."""
    if (getattr(args, 'loss', None) or 'berhu') != 'silog':
        return None
    v = {k: d if getattr(args, k, None) is None else getattr(args, k) for k, d in SILOG_DEFAULTS.items()}
    return ('silog', float(v['silog_lambda']), float(v['silog_weight']), float(v['silog_floor']), v['silog_mask'] == 'lidar')


RTOD_ARCH_DEFAULT = {'RtoD': 'unet', 'RtoD_single': 'unet', 'RtoD_test': 'legacy'}


def rtod_arch(args):
    """'unet' (AutoEncoder_2) or 'legacy' (AutoEncoder): --rtod_arch, or the mode's historical network."""
    arch = getattr(args, 'rtod_arch', None)
    if arch is None:
        arch = RTOD_ARCH_DEFAULT.get(args.mode, 'unet')
    if arch not in ('unet', 'legacy'):
        raise ValueError("--rtod_arch %r is not one of unet / legacy" % (arch,))
    return arch


parser = build_parser()


def parse_args(argv=None):
    return parser.parse_args(argv)
