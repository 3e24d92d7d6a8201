"""KITTI data pipeline with the augmentation on the GPU.

Mirrors the reference's ``datasets/datasets_list.py`` (``SequenceFolder`` :37-109: scene lists in
train.txt / val.txt / test_scenes_2.txt, per scene ``*.jpg`` colour frames, ``color_gt2/*.png`` dense
depth, ``gt/*.png`` sparse depth, shuffled for training) but the per-sample transform of
``GDN_main.py:57-62`` -- RandomHorizontalFlip, RandomScaleCrop (scipy.misc.imresize), ArrayToTensor,
Normalize -- runs in ONE HIP kernel per tensor on the whole batch (``gdn_kitti_augment``), bit-exact
with the host pipeline: the host only decodes files to uint8 and draws five random numbers per sample,
in the reference's call order.

Evaluation (GDN_main.py:64-79, :128-130): ``TestFolder`` reads the Eigen test split (KITTI files already at the network's
size: the validation transform of gdn_kitti_augment applies), ``NYUdataset(train=False)`` the NYU Depth v2 test set, whose
CenterCrop + ArrayToTensor + Normalize runs batched in ``GpuCropLoader`` (gdn_crop_normalize).

NYU training (GDN_main.py:94-129, datasets_list.py:366-443): ``NYUdataset(train=True)`` reads the training split and
``GpuNYUAugmentLoader`` runs its random crop / spline rotation / imresize / flip / colour transform in gdn_nyu_augment;
the host decodes the files and makes the reference's draws (``draw_params_nyu``).

Device-resident sets (no reference counterpart): ``ResidentPools`` decodes every file ONCE and keeps the raw bytes in device
memory; ``GpuResidentLoader`` / ``GpuNYUResidentLoader`` then assemble each batch on the device (gdn_kitti_augment_resident,
gdn_gather_samples) from the sample indices and the same host draws, in the same order, as their parents: the host's work
per batch is the draws and one small copy.
"""
import concurrent.futures as cf
import os
import pathlib
import random
import time

import numpy as np
import torch

from . import ops
from ._lib import GdnError


def _decode(path):
    """Image file -> uint8 HWC array (HW1 for single-channel files), as imageio.imread returns it."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.dtype != np.uint8:       # 16-bit depth PNGs keep their values; the float path bytescales them on the GPU
        a = a.astype(np.float32)
    return a[:, :, None] if a.ndim == 2 else a


class SequenceFolder:
    """Same constructor and sample order as the reference's SequenceFolder; samples are the RAW decoded images
    (gt, rgb, gt_sparse) -- the transform runs on the GPU in GpuAugmentLoader."""

    def __init__(self, root, args, seed=None, train=True, transform=None, target_transform=None, mode="DtoD"):
        self.root = pathlib.Path(root)
        self.train, self.mode, self.args = train, mode, args
        img_test = bool(getattr(args, "img_test", False))
        name = "test_scenes_2.txt" if img_test else ("train.txt" if train else "val.txt")
        with open(self.root / name) as f:
            self.scenes = [self.root / line.strip() for line in f if line.strip()]
        self._rng = random.Random(seed)          # the reference seeds with time(); a seed makes runs repeatable
        self.crawl_folders(shuffle=(not img_test) or train)

    def crawl_folders(self, shuffle=True):
        samples = []
        for scene in self.scenes:
            imgs = sorted(scene.glob("*.jpg"))
            gt = sorted((scene / "color_gt2").glob("*.png"))
            sp = sorted((scene / "gt").glob("*.png"))
            if not (len(imgs) == len(gt) == len(sp)):
                raise GdnError("scene %s: %d jpg, %d color_gt2 png, %d gt png" % (scene, len(imgs), len(gt), len(sp)))
            samples += [{"gt": g, "rgb": i, "gt_np": s} for g, i, s in zip(gt, imgs, sp)]
        if shuffle:
            self._rng.shuffle(samples)
        self.samples = samples

    def __getitem__(self, index):
        s = self.samples[index]
        return _decode(s["gt"]), _decode(s["rgb"]), _decode(s["gt_np"])

    def __len__(self):
        return len(self.samples)


def _decode_or_raise(path):
    try:
        return _decode(path)
    except Exception as e:        # missing, truncated or not an image
        raise GdnError("cannot decode %s: %s" % (path, e)) from e


class TestFolder:
    """The Eigen test split (datasets_list.py:111-189): root/eigen_test_files_img.txt, _color_gt.txt and _gt.txt list the
    colour frame, the dense depth and the sparse depth of each sample (first token of every line), in file order.  An
    entry is taken as written if that path exists, else relative to root.  Samples are the raw decoded
    (gt_color, rgb, gt) images.

    Deliberate divergence: the reference substitutes the previous sample when a file fails to load (and loops forever if
    the first one does); here a file that cannot be decoded raises GdnError naming it."""

    LISTS = ("eigen_test_files_img.txt", "eigen_test_files_color_gt.txt", "eigen_test_files_gt.txt")

    def __init__(self, root, args=None, seed=None, train=False, transform=None, target_transform=None, mode="DtoD"):
        self.root = pathlib.Path(root)
        self.train, self.mode, self.args = train, mode, args
        self.crawl_folders()

    def _entries(self, name):
        with open(self.root / name) as f:
            toks = [line.split()[0] for line in f if line.split()]
        return [pathlib.Path(t) if pathlib.Path(t).exists() else self.root / t for t in toks]

    def crawl_folders(self):
        imgs, color_gt, gt = (self._entries(n) for n in self.LISTS)
        if not (len(imgs) == len(color_gt) == len(gt)):
            raise GdnError("Eigen test lists differ in length: %d img, %d color_gt, %d gt" % (len(imgs), len(color_gt),
                                                                                               len(gt)))
        self.samples = [{"gt": s, "rgb": i, "gt_color": c} for i, c, s in zip(imgs, color_gt, gt)]

    def __getitem__(self, index):
        s = self.samples[index]
        return _decode_or_raise(s["gt_color"]), _decode_or_raise(s["rgb"]), _decode_or_raise(s["gt"])

    def __len__(self):
        return len(self.samples)


class EigenGt16:
    """--eval_gt_list: the ground truth of the Eigen split at its native size.  list_file names one 16-bit single-channel
    depth PNG per test sample (first token of every line; taken as written if that path exists, else relative to root), in
    the order of the test lists.  A sample is the [h, w] uint16 array as stored, WITHOUT conversion: metres x 256, 0 where
    the LiDAR has no return (the official KITTI format)."""

    def __init__(self, list_file, root=None):
        self.root = pathlib.Path(root) if root is not None else pathlib.Path(list_file).resolve().parent
        with open(list_file) as f:
            toks = [line.split()[0] for line in f if line.split()]
        self.samples = [pathlib.Path(t) if pathlib.Path(t).exists() else self.root / t for t in toks]

    def __getitem__(self, index):
        from PIL import Image
        path = self.samples[index]
        try:
            with Image.open(path) as im:
                mode = im.mode
                a = np.asarray(im) if mode.startswith("I;16") else None
        except Exception as e:
            raise GdnError("cannot decode %s: %s" % (path, e)) from e
        if a is None or a.ndim != 2:
            raise GdnError("%s is not a single-channel 16-bit image (mode %s): --eval_gt_list takes KITTI depth maps, "
                           "uint16 = metres x 256" % (path, mode))
        return np.ascontiguousarray(a, dtype=np.uint16)

    def __len__(self):
        return len(self.samples)


def assemble_gt16(maps, device):
    """B uint16 maps of any sizes -> ([B,Hmax,Wmax] uint16 on `device`, image b in the top-left corner, zero padding;
    [(h, w), ...]): one pinned staging buffer, one host-to-device copy."""
    sizes = [tuple(int(v) for v in m.shape) for m in maps]
    if not sizes or any(m.dtype != np.uint16 or m.ndim != 2 for m in maps):
        raise GdnError("assemble_gt16: a non-empty list of [h, w] uint16 arrays")
    device = torch.device(device)
    pool = torch.zeros((len(maps), max(h for h, _ in sizes), max(w for _, w in sizes)), dtype=torch.uint16)
    if device.type == "cuda":
        pool = pool.pin_memory()
    view = pool.numpy()
    for b, m in enumerate(maps):
        view[b, :m.shape[0], :m.shape[1]] = m
    return (pool.to(device, non_blocking=True) if device.type == "cuda" else pool), sizes


class EigenVelodyne:
    """--eval_velodyne: the raw Velodyne scan of each Eigen test sample (kitti_raw.parse_velo_list names them, in the order
    of the test lists).  A sample is (points float32 [N,4] as stored, P [3,4] float64, (h0, w0)): what ops.velo_project
    turns into the sample's sparse ground truth at the camera's native size.  The calibration is read once per date and
    camera.  depth ('camera' | 'forward') is kept for the caller: which depth the projected maps hold."""

    def __init__(self, list_file, raw_root, depth='camera'):
        from .kitti_raw import parse_velo_list
        if depth not in ops.VELO_DEPTHS:
            raise GdnError("EigenVelodyne: depth %r is not one of camera / forward" % (depth,))
        self.list_file, self.depth = str(list_file), depth
        self.samples = parse_velo_list(list_file, raw_root)
        self._calib = {}

    def __getitem__(self, index):
        from .kitti_raw import projection
        scan, date_dir, cam = self.samples[index]
        try:
            raw = np.fromfile(scan, dtype=np.float32)
        except OSError as e:
            raise GdnError("cannot read %s: %s" % (scan, e)) from e
        if raw.size % 4:
            raise GdnError("%s holds %d floats: not x, y, z, reflectance per point" % (scan, raw.size))
        key = (str(date_dir), cam)
        if key not in self._calib:
            self._calib[key] = projection(date_dir, cam)
        P, size = self._calib[key]
        return raw.reshape(-1, 4), P, size

    def __len__(self):
        return len(self.samples)


def assemble_scans(samples, device):
    """B samples of EigenVelodyne -> the device arguments of ops.velo_project: (points float32 [N,4], offsets int64 [B+1],
    proj float64 [B,12], sizes int32 [B,2], Hmax, Wmax, [(h0, w0), ...]).  The points travel through one pinned staging
    buffer in one host-to-device copy; offsets, matrices and sizes share one small table and one more copy."""
    B = len(samples)
    if B == 0:
        raise GdnError("assemble_scans: a non-empty list of (points, P, (h0, w0))")
    counts, sizes = [], []
    for pts, P, (h0, w0) in samples:
        if not (isinstance(pts, np.ndarray) and pts.dtype == np.float32 and pts.ndim == 2 and pts.shape[1] == 4):
            raise GdnError("assemble_scans: points must be float32 [N,4] arrays")
        if np.shape(P) != (3, 4) or int(h0) < 1 or int(w0) < 1:
            raise GdnError("assemble_scans: P must be 3 x 4 and the image size positive")
        counts.append(int(pts.shape[0]))
        sizes.append((int(h0), int(w0)))
    device = torch.device(device)
    pin = device.type == "cuda"
    total = sum(counts)
    stage = torch.empty((total, 4), dtype=torch.float32, pin_memory=pin)
    table = torch.empty(8 * (B + 1) + 96 * B + 8 * B, dtype=torch.uint8, pin_memory=pin)
    o_off, o_proj, o_size = 0, 8 * (B + 1), 8 * (B + 1) + 96 * B
    view = table.numpy()
    offsets = view[o_off:o_proj].view(np.int64)
    proj = view[o_proj:o_size].view(np.float64).reshape(B, 12)
    hw = view[o_size:].view(np.int32).reshape(B, 2)
    offsets[0] = 0
    np.cumsum(counts, out=offsets[1:])
    points = stage.numpy()
    for b, (pts, P, _) in enumerate(samples):
        points[offsets[b]:offsets[b + 1]] = pts
        proj[b] = np.asarray(P, dtype=np.float64).reshape(12)
        hw[b] = sizes[b]
    if pin:
        stage, table = stage.to(device, non_blocking=True), table.to(device, non_blocking=True)
    return (stage, table[o_off:o_proj].view(torch.int64), table[o_proj:o_size].view(torch.float64).reshape(B, 12),
            table[o_size:].view(torch.int32).reshape(B, 2), max(h for h, _ in sizes), max(w for _, w in sizes), sizes)


class NYUdataset:
    """NYU Depth v2 (datasets_list.py:366-444).  train=False: root/test/test_depths/*.png (16-bit depth) paired in sorted
    order with root/test/test_colors/*.png, in that order (the reference shuffles unless --img_test).  train=True:
    root/train/train_depths/*.png and root/train/train_colors/*.png, sorted, paired, then shuffled with random.Random(seed)
    (the reference seeds with time()).  Samples are the raw decoded (gt, rgb, gt) -- the same depth array twice, as the
    reference returns it; GpuCropLoader applies the validation transform, GpuNYUAugmentLoader the training one."""

    def __init__(self, root, args=None, seed=None, train=False, transform=None, transform_2=None, mode="DtoD"):
        self.root = pathlib.Path(root)
        self.train, self.mode, self.args = train, mode, args
        split = "train" if train else "test"
        self.depth_folder = self.root / split / (split + "_depths")
        self.img_folder = self.root / split / (split + "_colors")
        if train:
            for d in (self.depth_folder, self.img_folder):
                if not d.is_dir():
                    raise GdnError("NYU training set: %s not found (expected root/train/train_depths/*.png and "
                                   "root/train/train_colors/*.png)" % d)
        self._rng = random.Random(seed)
        self.crawl_folders()

    def crawl_folders(self):
        gt = sorted(self.depth_folder.glob("*.png"))
        rgbs = sorted(self.img_folder.glob("*.png"))
        if len(gt) != len(rgbs):
            raise GdnError("%s has %d png, %s has %d" % (self.depth_folder, len(gt), self.img_folder, len(rgbs)))
        self.samples = [{"gt": g, "rgb": r} for g, r in zip(gt, rgbs)]
        if self.train:
            self._rng.shuffle(self.samples)

    def __getitem__(self, index):
        s = self.samples[index]
        gt = _decode_or_raise(s["gt"])
        return gt, _decode_or_raise(s["rgb"]), gt

    def __len__(self):
        return len(self.samples)


class SyntheticRawKitti:
    """`n` deterministic raw samples shaped like decoded KITTI files: gt [H,W,1], rgb [H,W,3], sparse gt [H,W,1], uint8
    (sparse: 5 % valid pixels, the rest 0 -- which normalises to exactly -1, 'no LiDAR return')."""

    def __init__(self, n, H=128, W=416, seed=0):
        r = np.random.RandomState(seed)
        self.items = []
        for _ in range(n):
            gt = r.randint(0, 256, (H, W, 1)).astype(np.uint8)
            rgb = r.randint(0, 256, (H, W, 3)).astype(np.uint8)
            sp = np.where(r.rand(H, W, 1) < 0.05, r.randint(1, 256, (H, W, 1)), 0).astype(np.uint8)
            self.items.append((gt, rgb, sp))

    def __getitem__(self, i):
        return self.items[i]

    def __len__(self):
        return len(self.items)


def draw_params(in_h, in_w, py_rng, np_rng):
    """The reference's draws for one training sample, in its call order (transform_list.py:158-166, :185-199):
    random.random() -> flip; np.random.uniform(1, 1.15, 2) -> x, y scaling; np.random.randint -> y, x offsets."""
    flip = 1 if py_rng.random() < 0.5 else 0
    x_scaling, y_scaling = np_rng.uniform(1, 1.15, 2)
    scaled_h, scaled_w = int(in_h * y_scaling), int(in_w * x_scaling)
    off_y = int(np_rng.randint(scaled_h - in_h + 1))
    off_x = int(np_rng.randint(scaled_w - in_w + 1))
    return (flip, scaled_h, scaled_w, off_y, off_x)


class GpuAugmentLoader:
    """Batches of (gt, rgb, gt_sparse) as normalised NCHW float32 tensors on `device` -- what the training loops
    consume -- with the reference's train/validation transform executed by gdn_kitti_augment.

    dataset: indexable of (gt, rgb, sparse) raw HWC arrays, uint8 (or float32: bytescaled on the GPU like imresize).
    train=False applies the validation transform (ArrayToTensor + Normalize) and keeps the order."""

    def __init__(self, dataset, batch_size, device, train=True, seed=None, shuffle=None, workers=0, drop_last=False,
                 rank=0, world=1, order_seed=None):
        """rank / world: data-parallel sharding like DistributedSampler -- every rank shuffles with the SAME order_seed and
        takes order[rank::world], so one epoch visits each sample once over all ranks (batch_size is per rank: the global
        batch is world * batch_size).  The augmentation draws stay rank-specific (seed)."""
        self.ds, self.bs, self.dev, self.train = dataset, int(batch_size), torch.device(device), train
        self.shuffle = train if shuffle is None else shuffle
        self.drop_last = drop_last
        self.rank, self.world = int(rank), max(1, int(world))
        self.py_rng, self.np_rng = random.Random(seed), np.random.RandomState(seed)
        if order_seed is None:
            order_seed = None if seed is None else seed + 1
        self.order_rng = random.Random(order_seed)
        self.pool = cf.ThreadPoolExecutor(workers) if workers > 0 else None
        self.last_params = None
        # resume (state_dict / load_state_dict): the order stream's state before the current epoch's shuffle, the batch last
        # handed out in it (-1: none yet) and, after a load, the batch the next __iter__ starts with
        self._order_start, self._pos, self._resume = None, -1, None
        self._bound = None

    def bind_outputs(self, gt=None, rgb=None, sparse=None):
        """Write every full-size batch into these three tensors -- a captured training step's static inputs -- and yield
        exactly them, so nothing has to be copied before a replay.  An entry left None keeps its fresh tensor per batch;
        all None unbinds.  The tensors are checked against the batch when it is written (ops.kitti_augment(out=)); a batch
        of another size than the bound tensors' (a last partial one) is yielded in fresh tensors."""
        bound = (gt, rgb, sparse)
        for t in bound:
            if t is not None and not (isinstance(t, torch.Tensor) and t.dim() == 4 and t.dtype == torch.float32):
                raise GdnError("bind_outputs: float32 [B,C,H,W] tensors or None, got %r" % (type(t).__name__,))
        sizes = {t.shape[0] for t in bound if t is not None}
        if len(sizes) > 1:
            raise GdnError("bind_outputs: the tensors hold batches of different sizes %s" % sorted(sizes))
        self._bound = None if not sizes else bound

    def _outs(self, B):
        """The bound tensors for a batch of B samples, or None (nothing bound, or another batch size)."""
        if self._bound is None or next(t for t in self._bound if t is not None).shape[0] != B:
            return None
        return self._bound

    def _begin_epoch(self):
        """(sample order of the epoch that starts now, its first batch): batch 0 of a fresh shuffle, or -- once, after
        load_state_dict() -- the batch after the saved one in the saved epoch's order.  The skipped batches are neither
        fetched nor drawn for: the draw streams were saved after them."""
        first, self._resume = self._resume or 0, None
        self._order_start = self.order_rng.getstate()
        self._pos = first - 1
        return self._epoch_order(), first

    def _identity(self):
        return {"rank": self.rank, "world": self.world, "n": len(self.ds), "batch_size": self.bs}

    def state_dict(self, epoch_done=False):
        """Position and RNG state, nothing else (a resident loader keeps its pools).  Call it between two batches: the draw
        streams are saved as the last batch handed out left them, the order stream as it was before the current epoch's
        shuffle, so the epoch can be rebuilt.  epoch_done=True: the current epoch is over (the training loops leave it
        early with `break`), the next __iter__ of the restored loader starts a fresh one."""
        fresh = epoch_done or self._order_start is None
        np_state = self.np_rng.get_state()
        out = self._identity()
        out.update({"order_rng": self.order_rng.getstate() if fresh else self._order_start, "pos": -1 if fresh else self._pos,
                    "py_rng": self.py_rng.getstate(),
                    "np_rng": (np_state[0], [int(x) for x in np_state[1]], int(np_state[2]), int(np_state[3]), float(np_state[4]))})
        return out

    def load_state_dict(self, state):
        """Continue where state_dict() was taken: the next __iter__ rebuilds that epoch's order and starts with the batch after
        the saved one; later epochs go on as if the loader had never stopped.  rank, world, dataset length and batch size must
        be the saved ones."""
        mine = self._identity()
        for key, what in (("world", "world size"), ("n", "dataset length"), ("batch_size", "batch size"), ("rank", "rank")):
            if int(state[key]) != mine[key]:
                raise GdnError("loader state was saved with %s %d, this loader has %d" % (what, int(state[key]), mine[key]))

        def tup(x):
            return tuple(tup(y) for y in x) if isinstance(x, (list, tuple)) else x
        self.order_rng.setstate(tup(state["order_rng"]))
        self.py_rng.setstate(tup(state["py_rng"]))
        name, keys, pos, has_gauss, cached = state["np_rng"]
        self.np_rng.set_state((name, np.asarray(keys, dtype=np.uint32), int(pos), int(has_gauss), float(cached)))
        self._order_start, self._pos = self.order_rng.getstate(), int(state["pos"])
        self._resume = self._pos + 1

    def _shard_len(self):
        n = len(self.ds)
        return n // self.world if self.world > 1 else n       # equal shards: every rank runs the same number of steps

    def __len__(self):
        n = self._shard_len()
        return n // self.bs if self.drop_last else (n + self.bs - 1) // self.bs

    def _fetch(self, idxs):
        if self.pool is not None:
            return list(self.pool.map(self.ds.__getitem__, idxs))
        return [self.ds[i] for i in idxs]

    def _to_device(self, arrays):
        a = np.stack(arrays)
        t = torch.from_numpy(a)
        return t.pin_memory().to(self.dev, non_blocking=True) if self.dev.type == "cuda" else t

    def _epoch_order(self):
        order = list(range(len(self.ds)))
        if self.shuffle:
            self.order_rng.shuffle(order)
        if self.world > 1:
            order = order[self.rank::self.world][:self._shard_len()]
        return order

    def __iter__(self):
        order, first = self._begin_epoch()
        for b in range(first, len(self)):
            self._pos = b
            idxs = order[b * self.bs:(b + 1) * self.bs]
            samples = self._fetch(idxs)
            H, W = samples[0][1].shape[:2]
            for s in samples:
                if any(x.shape[:2] != (H, W) for x in s):
                    raise GdnError("all images of a batch must share one size, got %s" % ([x.shape for x in s],))
            params = None
            if self.train:
                host = [draw_params(H, W, self.py_rng, self.np_rng) for _ in samples]
                self.last_params = host
                params = torch.tensor(host, dtype=torch.int32)
                if self.dev.type == "cuda":
                    params = params.pin_memory().to(self.dev, non_blocking=True)
            outs = self._outs(len(samples))
            if outs is None:
                yield tuple(ops.kitti_augment(self._to_device([s[j] for s in samples]), params, self.train) for j in range(3))
            else:
                yield tuple(ops.kitti_augment(self._to_device([s[j] for s in samples]), params, self.train, out=outs[j])
                            for j in range(3))


class GpuCropLoader(GpuAugmentLoader):
    """Batches of (gt, rgb, gt) as normalised NCHW float32 tensors on `device`, in dataset order, with the NYU validation
    transform (CenterCrop to height x width at the centre of the colour image, ArrayToTensor, Normalize) executed by
    gdn_crop_normalize.  A sample whose third image is its first (NYUdataset) shares one output tensor."""

    bind_outputs = None      # this transform allocates its outputs: a captured step copies its batch

    def __init__(self, dataset, batch_size, device, height, width, workers=0):
        super().__init__(dataset, batch_size, device, train=False, shuffle=False, workers=workers)
        self.size = (int(height), int(width))

    def __iter__(self):
        H, W = self.size
        order, first = self._begin_epoch()
        for b in range(first, len(self)):
            self._pos = b
            samples = self._fetch(order[b * self.bs:(b + 1) * self.bs])
            H0, W0 = samples[0][1].shape[:2]
            for s in samples:
                if any(x.shape[:2] != (H0, W0) for x in s):
                    raise GdnError("all images of a batch must share one size, got %s" % ([x.shape for x in s],))
            off = ops.center_crop_offsets(H0, W0, H, W)        # CenterCrop takes its window from the colour image
            gt, rgb = (ops.crop_normalize(self._to_device([s[j] for s in samples]), H, W, off) for j in range(2))
            third = gt if all(s[2] is s[0] for s in samples) else \
                ops.crop_normalize(self._to_device([s[2] for s in samples]), H, W, off)
            yield gt, rgb, third


NYU_CROP = ops.NYU_CROP


def draw_params_nyu(h0, w0, mode, py_rng, np_rng):
    """The reference's draws for one NYU training sample, in its call order (datasets_list.py:401-402, then
    GDN_main.py:94-125 through transform_list.py): np.random.uniform(1, 1.2) -> img_s; np.random.uniform(1.0, 1.5) ->
    scale; RandomCropNumpy's randint(s) on the int(img_s * 251) x int(img_s * 340) image (none when it is already
    251 x 340; randint's upper bound is exclusive); RandomRotate's np.random.uniform(-4, 4) (DtoD) or (-5, 5) (RtoD);
    RandomHorizontalFlip's random.random() < 0.5; RtoD only: RandomColor's np.random.uniform(0.8, 1.2).
    The source size h0 x w0 enters no draw; it is checked only."""
    if mode not in ("DtoD", "RtoD"):
        raise GdnError("draw_params_nyu: mode must be DtoD or RtoD, got %r" % (mode,))
    if h0 <= 0 or w0 <= 0:
        raise GdnError("draw_params_nyu: empty source %dx%d" % (h0, w0))
    th, tw = NYU_CROP
    img_s = np_rng.uniform(1, 1.2)
    scale = np_rng.uniform(1.0, 1.5)
    h1, w1 = int(img_s * 251.0), int(img_s * 340.0)
    y1 = x1 = 0
    if h1 == th and w1 == tw:
        pass
    elif h1 == th:
        x1 = int(np_rng.randint(0, w1 - tw))
    elif w1 == tw:
        y1 = int(np_rng.randint(0, h1 - th))
    else:
        y1 = int(np_rng.randint(0, h1 - th))
        x1 = int(np_rng.randint(0, w1 - tw))
    angle = np_rng.uniform(-4, 4) if mode == "DtoD" else np_rng.uniform(-5, 5)
    flip = 1 if py_rng.random() < 0.5 else 0
    mult = np_rng.uniform(0.8, 1.2) if mode == "RtoD" else 1.0
    return dict(img_s=img_s, scale=scale, h1=h1, w1=w1, y1=y1, x1=x1, angle=angle, flip=flip, mult=mult)


class GpuNYUAugmentLoader(GpuAugmentLoader):
    """Batches of (gt, rgb, gt) as normalised NCHW float32 tensors on `device` with the reference's NYU training transform
    (GDN_main.py:94-129, datasets_list.py:399-430) executed by gdn_nyu_augment: the host decodes the files and makes the
    draws of draw_params_nyu per sample, in batch order; `last_params` keeps the last batch's draws.  Ordering, sharding
    (rank / world / order_seed) and drop_last are GpuAugmentLoader's.  height x width <= 251 x 340."""

    bind_outputs = None      # this transform allocates its outputs: a captured step copies its batch
    yields_sparse = False    # the third output is the ground truth again, not a LiDAR map (--silog_mask lidar is refused)

    def __init__(self, dataset, batch_size, device, height, width, mode="DtoD", seed=None, workers=0, drop_last=False,
                 rank=0, world=1, order_seed=None):
        if mode not in ("DtoD", "RtoD"):
            raise GdnError("GpuNYUAugmentLoader: mode must be DtoD or RtoD, got %r" % (mode,))
        if not (0 < height <= NYU_CROP[0] and 0 < width <= NYU_CROP[1]):
            raise GdnError("GpuNYUAugmentLoader: %dx%d does not fit the %dx%d crop" % ((height, width) + NYU_CROP))
        super().__init__(dataset, batch_size, device, train=True, seed=seed, workers=workers, drop_last=drop_last,
                         rank=rank, world=world, order_seed=order_seed)
        self.size, self.mode = (int(height), int(width)), mode

    def __iter__(self):
        H, W = self.size
        order, first = self._begin_epoch()
        for b in range(first, len(self)):
            self._pos = b
            samples = self._fetch(order[b * self.bs:(b + 1) * self.bs])
            H0, W0 = samples[0][1].shape[:2]
            for s in samples:
                if any(x.shape[:2] != (H0, W0) for x in s):
                    raise GdnError("all images of a batch must share one size, got %s" % ([x.shape for x in s],))
                if s[1].ndim != 3 or s[1].shape[2] != 3 or s[1].dtype != np.uint8:
                    raise GdnError("NYU colour images must be 8-bit RGB, got %s %s" % (s[1].dtype, s[1].shape))
            draws = [draw_params_nyu(H0, W0, self.mode, self.py_rng, self.np_rng) for _ in samples]
            self.last_params = draws
            depth = self._to_device([np.ascontiguousarray(s[0][:, :, 0] if s[0].ndim == 3 else s[0], dtype=np.float32)
                                     for s in samples])
            rgb = self._to_device([s[1] for s in samples])
            gt, img = ops.nyu_augment(depth, rgb, draws, H, W, self.mode)
            yield gt, img, gt


# ---------------------------------------------------------------------------------------------------------------------
# device-resident training sets

STAGING_BYTES = 64 << 20       # the one pinned host buffer every upload of a preload goes through
_FILE_KEYS = {SequenceFolder: ("gt", "rgb", "gt_np"), TestFolder: ("gt_color", "rgb", "gt"), NYUdataset: ("gt", "rgb", "gt")}


def resident_bytes(n, shapes, itemsizes=None):
    """Device bytes the pools of n samples hold: `shapes` are the array shapes of one sample, `itemsizes` their element
    sizes in bytes (default 1 each: uint8).  KITTI at 128x416: resident_bytes(n, [(128, 416, 1), (128, 416, 3),
    (128, 416, 1)]) = n * 266,240."""
    shapes = [tuple(int(d) for d in sh) for sh in shapes]
    itemsizes = [1] * len(shapes) if itemsizes is None else [int(i) for i in itemsizes]
    if n < 0 or len(itemsizes) != len(shapes) or any(d <= 0 for sh in shapes for d in sh) or any(i <= 0 for i in itemsizes):
        raise GdnError("resident_bytes: bad arguments n=%r shapes=%r itemsizes=%r" % (n, shapes, itemsizes))
    return int(n) * sum(int(np.prod(sh, dtype=np.int64)) * i for sh, i in zip(shapes, itemsizes))


def preload_threads(workers=0):
    """Decode threads of a preload: the CPUs this process may run on, 16 at the most (never the machine's CPU count)."""
    return max(1, min(workers or 16, 16, len(os.sched_getaffinity(0))))


class ResidentPools:
    """Every sample of an indexable dataset (SequenceFolder, TestFolder, SyntheticRawKitti: kind 'kitti'; NYUdataset: kind
    'nyu'), decoded once by a thread pool and held in device memory as raw bytes:
      kitti: tensors = (gt [N,H,W,Cg], rgb [N,H,W,Cr], sparse [N,H,W,Cs]) uint8 -- all images of one size, uint8, one channel
             count per pool; a float / 16-bit source raises (the per-image bytescale is not carried);
      nyu:   tensors = (depth [N,H0,W0] uint16, rgb [N,H0,W0,3] uint8) -- every depth value integral in [0, 65535].
    A violation raises GdnError naming the first offending file.  resident_bytes() of the set is compared with max_bytes
    (default: half of the device's free memory) BEFORE anything is allocated.  Uploads go through one pinned staging buffer
    of at most STAGING_BYTES."""

    def __init__(self, dataset, device, kind=None, workers=0, max_bytes=None):
        t0 = time.time()
        self.dev = torch.device(device)
        self.kind = kind or ("nyu" if isinstance(dataset, NYUdataset) else "kitti")
        if self.kind not in ("kitti", "nyu"):
            raise GdnError("ResidentPools: kind must be 'kitti' or 'nyu', got %r" % (kind,))
        self.n = len(dataset)
        if self.n == 0:
            raise GdnError("ResidentPools: the dataset is empty")
        self._ds = dataset
        first = self._arrays(0, dataset[0], None)
        self.shapes = [a.shape for a in first]
        self.itemsizes = [a.dtype.itemsize for a in first]
        self.size = tuple(first[-1].shape[:2])
        self.nbytes = resident_bytes(self.n, self.shapes, self.itemsizes)
        cuda = self.dev.type == "cuda"
        if max_bytes is None:
            if not cuda:
                raise GdnError("ResidentPools: max_bytes is required off the GPU")
            max_bytes = torch.cuda.mem_get_info(self.dev)[0] // 2
        if self.nbytes > max_bytes:
            raise GdnError("resident set needs %.3f GB (%d samples x %d bytes) but the budget is %.3f GB; raise it "
                           "(--resident_gb) or train without --resident" %
                           (self.nbytes / 1e9, self.n, self.nbytes // self.n, max_bytes / 1e9))
        sample_bytes = self.nbytes // self.n
        if sample_bytes > STAGING_BYTES:
            raise GdnError("ResidentPools: one sample (%d bytes) exceeds the staging buffer" % sample_bytes)
        per = min(self.n, STAGING_BYTES // sample_bytes)          # samples per staged chunk
        dtypes = [torch.uint8 if i == 1 else torch.uint16 for i in self.itemsizes]
        self.tensors = tuple(torch.empty((self.n,) + sh, dtype=dt, device=self.dev) for sh, dt in zip(self.shapes, dtypes))
        staging = torch.empty(per * sample_bytes, dtype=torch.uint8, pin_memory=cuda)
        views, off = [], 0
        for sh, i, dt in zip(self.shapes, self.itemsizes, dtypes):       # [per, ...] windows of the staging buffer, 2-byte pools first
            nb = per * int(np.prod(sh)) * i
            views.append(staging[off:off + nb].view(dt).view((per,) + sh))
            off += nb
        self.threads = preload_threads(workers)
        with cf.ThreadPoolExecutor(self.threads) as ex:
            for s in range(0, self.n, per):
                m = min(per, self.n - s)
                raw = list(ex.map(dataset.__getitem__, range(max(s, 1), s + m)))
                chunk = ([first] if s == 0 else []) + [self._arrays(i, r, self.shapes) for i, r in
                                                      zip(range(max(s, 1), s + m), raw)]
                if cuda:
                    torch.cuda.current_stream(self.dev).synchronize()     # the previous chunk has left the staging buffer
                for j, v in enumerate(views):
                    hv = v.numpy()
                    for k, arrs in enumerate(chunk):
                        hv[k] = arrs[j]
                    self.tensors[j][s:s + m].copy_(v[:m], non_blocking=True)
        if cuda:
            torch.cuda.current_stream(self.dev).synchronize()
        del self._ds
        self.seconds = time.time() - t0
        from . import distributed as D
        if D.rank() == 0:
            print("=> resident %s set: %d samples, %.3f GB on %s, preloaded in %.1f s by %d threads" %
                  (self.kind, self.n, self.nbytes / 1e9, self.dev, self.seconds, self.threads))

    def _name(self, i, j):
        keys = _FILE_KEYS.get(type(self._ds))
        samples = getattr(self._ds, "samples", None)
        if keys and samples is not None:
            return str(samples[i][keys[j]])
        return "sample %d, image %d" % (i, j)

    def _arrays(self, i, sample, shapes):
        """The arrays of sample i as the pools store them, checked (against `shapes` once the first sample has set them)."""
        if self.kind == "kitti":
            out = []
            for j, a in enumerate(sample):
                if a.dtype != np.uint8:
                    raise GdnError("%s: resident mode holds uint8 images only (this one decodes to %s: a float or 16-bit "
                                   "source needs the per-image bytescale of the non-resident loader)" % (self._name(i, j), a.dtype))
                if a.ndim != 3 or not 1 <= a.shape[2] <= 4:
                    raise GdnError("%s: expected an HxWxC image with C <= 4, got shape %s" % (self._name(i, j), a.shape))
                want = shapes[j] if shapes is not None else sample[1].shape[:2] + (a.shape[2],)
                if a.shape != tuple(want):
                    raise GdnError("%s: shape %s differs from the set's %s (all images of a resident set share one size "
                                   "and one channel count per pool)" % (self._name(i, j), a.shape, tuple(want)))
                out.append(a)
            return out
        d, c = sample[0], sample[1]
        d = d[:, :, 0] if d.ndim == 3 and d.shape[2] == 1 else d
        if d.ndim != 2 or not ((d >= 0).all() and (d <= 65535).all() and (d == np.floor(d)).all()):
            raise GdnError("%s: NYU depth must be one channel of integral values in [0, 65535] (shape %s, %s)" %
                           (self._name(i, 0), d.shape, d.dtype))
        if c.ndim != 3 or c.shape[2] != 3 or c.dtype != np.uint8:
            raise GdnError("%s: NYU colour images must be 8-bit RGB, got %s %s" % (self._name(i, 1), c.dtype, c.shape))
        if c.shape[:2] != d.shape or (shapes is not None and (d.shape != tuple(shapes[0]) or c.shape != tuple(shapes[1]))):
            raise GdnError("%s: size %s / %s differs from the set's (all images of a resident set share one size)" %
                           (self._name(i, 0), d.shape, c.shape))
        return [d.astype(np.uint16), c]


class _UploadRing:
    """A few pinned int32 host buffers used in turn for the small per-batch host-to-device copies: a slot is rewritten only
    after the asynchronous copy that last read it has completed (its event), so the host never waits for the GPU's queue."""

    def __init__(self, device, shape, slots=4):
        self.dev = torch.device(device)
        self.cuda = self.dev.type == "cuda"
        self.bufs = [torch.empty(shape, dtype=torch.int32, pin_memory=self.cuda) for _ in range(slots)]
        self.events = [None] * slots
        self.k = 0

    def upload(self, rows):
        if not self.cuda:
            return torch.from_numpy(np.array(rows, dtype=np.int32))
        k, self.k = self.k, (self.k + 1) % len(self.bufs)
        if self.events[k] is not None:
            self.events[k].synchronize()
        host = self.bufs[k][:rows.shape[0]]
        host.copy_(torch.from_numpy(rows))
        out = host.to(self.dev, non_blocking=True)
        self.events[k] = torch.cuda.Event()
        self.events[k].record(torch.cuda.current_stream(self.dev))
        return out


def _pools_for(dataset, device, kind, pools, workers, max_bytes):
    if pools is None:
        pools = ResidentPools(dataset, device, kind=kind, workers=workers, max_bytes=max_bytes)
    if pools.kind != kind or pools.n != len(dataset):
        raise GdnError("resident loader: the pools hold %d %s samples, the dataset has %d (%s expected)" %
                       (pools.n, pools.kind, len(dataset), kind))
    return pools


class GpuResidentLoader(GpuAugmentLoader):
    """GpuAugmentLoader over a device-resident set: the same order, sharding, drop_last, draws (draw_params, in the same
    order) and last_params, and bit-identical batches, but the dataset is decoded once, at construction (ResidentPools,
    or `pools` built before), and never indexed again.  Per batch the host builds the int32 rows {sample index, five
    draws}, copies them to the device once and gdn_kitti_augment_resident makes the three tensors in one launch.
    `workers` sizes the preload's thread pool; `max_bytes` is its budget."""

    def __init__(self, dataset, batch_size, device, train=True, seed=None, shuffle=None, workers=0, drop_last=False,
                 rank=0, world=1, order_seed=None, pools=None, max_bytes=None):
        super().__init__(dataset, batch_size, device, train=train, seed=seed, shuffle=shuffle, workers=0,
                         drop_last=drop_last, rank=rank, world=world, order_seed=order_seed)
        self.pools = _pools_for(dataset, self.dev, "kitti", pools, workers, max_bytes)
        self._ring = _UploadRing(self.dev, (self.bs, 6))

    def __iter__(self):
        H, W = self.pools.size
        order, first = self._begin_epoch()
        for b in range(first, len(self)):
            self._pos = b
            idxs = order[b * self.bs:(b + 1) * self.bs]
            rows = np.empty((len(idxs), 6), np.int32)
            rows[:, 0] = idxs
            rows[:, 1:] = (0, H, W, 0, 0)
            if self.train:
                host = [draw_params(H, W, self.py_rng, self.np_rng) for _ in idxs]
                self.last_params = host
                rows[:, 1:] = host
            sel = self._ring.upload(ops.check_sel(rows, self.pools.n, H, W, self.train))
            outs = self._outs(len(idxs))
            if outs is None:
                yield ops.kitti_augment_resident(self.pools.tensors, sel, self.train)
            else:
                outs = tuple(torch.empty((len(idxs), p.shape[3], H, W), dtype=torch.float32, device=self.dev) if o is None
                             else o for o, p in zip(outs, self.pools.tensors))
                yield ops.kitti_augment_resident(self.pools.tensors, sel, self.train, out=outs)


class GpuNYUResidentLoader(GpuNYUAugmentLoader):
    """GpuNYUAugmentLoader over a device-resident set (uint16 depth pool, uint8 colour pool): gdn_gather_samples copies the
    batch's samples out of the pools, widening the depth to float32 as decoding does, and feeds the parent's
    gdn_nyu_augment with the parent's draws (draw_params_nyu, same order).  Bit-identical batches; the dataset is never
    indexed after construction."""

    def __init__(self, dataset, batch_size, device, height, width, mode="DtoD", seed=None, workers=0, drop_last=False,
                 rank=0, world=1, order_seed=None, pools=None, max_bytes=None):
        super().__init__(dataset, batch_size, device, height, width, mode=mode, seed=seed, workers=0, drop_last=drop_last,
                         rank=rank, world=world, order_seed=order_seed)
        self.pools = _pools_for(dataset, self.dev, "nyu", pools, workers, max_bytes)
        self._ring = _UploadRing(self.dev, (self.bs,))

    def __iter__(self):
        H, W = self.size
        H0, W0 = self.pools.size
        order, first = self._begin_epoch()
        for b in range(first, len(self)):
            self._pos = b
            idxs = np.asarray(order[b * self.bs:(b + 1) * self.bs], dtype=np.int32)
            if idxs.min() < 0 or idxs.max() >= self.pools.n:
                raise GdnError("sample index outside the %d resident samples" % self.pools.n)
            draws = [draw_params_nyu(H0, W0, self.mode, self.py_rng, self.np_rng) for _ in idxs]
            self.last_params = draws
            idx = self._ring.upload(idxs)
            depth = ops.gather_samples(self.pools.tensors[0], idx, to_f32=True)
            rgb = ops.gather_samples(self.pools.tensors[1], idx)
            gt, img = ops.nyu_augment(depth, rgb, draws, H, W, self.mode)
            yield gt, img, gt
