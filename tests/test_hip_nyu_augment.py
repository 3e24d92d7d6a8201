"""GPU parity of the device-side NYU training transform (gdn_nyu_augment and its building blocks) against the numpy
restatement of tests/nyu_augment_numpy.py, itself pinned to SciPy / Pillow by tests/test_nyu_augment_cpu.py: the bar is
BIT-EXACT output tensors."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

import nyu_augment_numpy as N
from oracle.kitti_augment import resize_bilinear_u8
from test_nyu_augment_cpu import edge_draws, synthetic_nyu

pytestmark = pytest.mark.gpu


def _eq(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), "%s: %d of %d elements differ, max %.3e" % (
        what, int((got != ref).sum()), got.size, float(np.abs(got.astype(np.float64) - ref).max()))


@pytest.mark.parametrize("B", [1, 3, 8])
def test_pil_resize_block(gpu, B):
    from gdn_amd import ops
    r = np.random.RandomState(B)
    H0, W0 = 61, 83
    u8 = r.randint(0, 256, (B, H0, W0, 3)).astype(np.uint8)
    u8[:, :, :, 1] //= 2
    f32 = (r.rand(B, H0, W0, 1) * 5000 + 7).astype(np.float32)
    for oh, ow, win in [(48, 64, None), (61, 120, (5, 7, 40, 100)), (130, 83, (9, 0, 100, 83)), (30, 29, (1, 2, 20, 20)),
                        (61, 83, None)]:
        wy, wx, wh, ww = win or (0, 0, oh, ow)
        got = ops.pil_resize(torch.from_numpy(u8).to(gpu), oh, ow, win).cpu().numpy()
        got_bs = ops.pil_resize(torch.from_numpy(u8).to(gpu), oh, ow, win, bytescale=True).cpu().numpy()
        got_f8 = ops.pil_resize(torch.from_numpy(f32).to(gpu), oh, ow, win).cpu().numpy()
        got_f = ops.pil_resize(torch.from_numpy(f32).to(gpu), oh, ow, win, f_mode=True).cpu().numpy()
        for b in range(B):
            sl = (slice(wy, wy + wh), slice(wx, wx + ww))
            _eq(got[b], resize_bilinear_u8(u8[b], oh, ow)[sl], "u8 %s" % ((oh, ow, win),))
            _eq(got_bs[b], N.imresize_u8(u8[b].astype(np.float32), oh, ow)[sl], "u8 bytescale %s" % ((oh, ow, win),))
            _eq(got_f8[b], N.imresize_u8(f32[b], oh, ow)[sl], "f32 bytescale %s" % ((oh, ow, win),))
            _eq(got_f[b, :, :, 0], N.resize_f(f32[b, :, :, 0], oh, ow)[sl], "F %s" % ((oh, ow, win),))


@pytest.mark.parametrize("B", [1, 3, 8])
def test_spline_rotate_block(gpu, B):
    from gdn_amd import ops
    r = np.random.RandomState(10 + B)
    for C, H, W in [(1, 251, 340), (4, 251, 340), (2, 37, 53)]:
        a = (r.rand(B, C, H, W) * 3000).astype(np.float32)
        a[:, :, :, W // 2:] += np.float32(1500)
        for angle, clip in [(r.uniform(-5, 5), True), (0.0, True), (-5.0, False)]:
            got = ops.spline_rotate(torch.from_numpy(a).to(gpu), angle, clip=clip).cpu().numpy()
            for b in range(B):
                ref = N.rotate(a[b].transpose(1, 2, 0), angle, clip=clip).transpose(2, 0, 1)
                _eq(got[b], ref, "B=%d C=%d %dx%d angle %r clip %s" % (B, C, H, W, angle, clip))


def _gpu_batch(gpu, depths, rgbs, draws, H, W, mode):
    from gdn_amd import ops
    d = torch.from_numpy(np.stack(depths)).to(gpu)
    c = torch.from_numpy(np.stack(rgbs)).to(gpu)
    gd, gc = ops.nyu_augment(d, c, draws, H, W, mode)
    return gd.cpu().numpy(), gc.cpu().numpy()


@pytest.mark.parametrize("mode", ["DtoD", "RtoD"])
@pytest.mark.parametrize("size", [(224, 320), (64, 96)])
def test_nyu_augment_bit_exact(gpu, mode, size):
    H, W = size
    r = np.random.RandomState(H + (mode == "RtoD"))
    py, npr = random.Random(H), np.random.RandomState(H)
    n = 40 if size == (224, 320) else 16
    draws = edge_draws(mode)
    draws += [N.draw_params(mode, py, npr) for _ in range(n - len(draws))]
    srcs = [synthetic_nyu(r, 240, 320) for _ in range(8)]
    for k in range(0, n, 8):
        ds = draws[k:k + 8]
        got_d, got_c = _gpu_batch(gpu, [s[0] for s in srcs[:len(ds)]], [s[1] for s in srcs[:len(ds)]], ds, H, W, mode)
        for b, p in enumerate(ds):
            ref_d, ref_c = N.augment_sample(srcs[b][0], srcs[b][1], p, mode, H, W)
            _eq(got_d[b], ref_d, "depth, draw %d %s" % (k + b, p))
            _eq(got_c[b], ref_c, "rgb, draw %d %s" % (k + b, p))


def _write_nyu(root, n, H0, W0, seed):
    r = np.random.RandomState(seed)
    for i in range(n):
        depth, rgb = synthetic_nyu(r, H0, W0)
        for sub, arr in (("train/train_depths", depth.astype(np.uint16)), ("train/train_colors", rgb)):
            (root / sub).mkdir(parents=True, exist_ok=True)
            Image.fromarray(arr).save(root / sub / ("%05d.png" % i))


def _restated_batches(ds, loader, n_batches, H, W, mode, order_seed):
    """The restatement's tensors for the loader's first epoch, from its draws (loader.last_params) and its order."""
    order = list(range(len(ds)))
    random.Random(order_seed).shuffle(order)
    for b, _ in zip(range(n_batches), loader):
        idx = order[b * loader.bs:(b + 1) * loader.bs]
        outs = [N.augment_sample(ds[i][0], ds[i][1], p, mode, H, W) for i, p in zip(idx, loader.last_params)]
        yield np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


@pytest.mark.parametrize("mode", ["DtoD", "RtoD"])
@pytest.mark.parametrize("src", [(320, 420), (480, 640)])
def test_loader_matches_restatement(gpu, tmp_path, mode, src):
    from gdn_amd.datasets import GpuNYUAugmentLoader, NYUdataset
    _write_nyu(tmp_path, 6, src[0], src[1], seed=src[0])
    ds = NYUdataset(str(tmp_path), None, seed=3, train=True)
    H, W = 224, 320
    loader = GpuNYUAugmentLoader(ds, 3, gpu, H, W, mode=mode, seed=9)
    order = list(range(len(ds)))
    random.Random(10).shuffle(order)                          # order_seed defaults to seed + 1
    n = 0
    for b, (gt, rgb, gt2) in enumerate(loader):
        assert gt2 is gt and gt.shape == (3, 1, H, W) and rgb.shape == (3, 3, H, W)
        for k, (i, p) in enumerate(zip(order[b * 3:(b + 1) * 3], loader.last_params)):
            d, c, _ = ds[i]
            assert d.dtype == np.float32 and c.dtype == np.uint8
            ref_d, ref_c = N.augment_sample(d, c, p, mode, H, W)
            _eq(gt[k].cpu().numpy(), ref_d, "loader depth %d" % i)
            _eq(rgb[k].cpu().numpy(), ref_c, "loader rgb %d" % i)
            n += 1
    assert n == 6


def test_loaders_with_one_seed_agree(gpu, tmp_path):
    from gdn_amd.datasets import GpuNYUAugmentLoader, NYUdataset
    _write_nyu(tmp_path, 4, 320, 420, seed=1)
    runs = []
    for _ in range(2):
        ds = NYUdataset(str(tmp_path), None, seed=5, train=True)
        loader = GpuNYUAugmentLoader(ds, 2, gpu, 96, 128, mode="RtoD", seed=21, workers=2)
        runs.append([(gt.cpu().numpy(), rgb.cpu().numpy()) for gt, rgb, _ in loader])
    assert len(runs[0]) == 2
    for (a_gt, a_rgb), (b_gt, b_rgb) in zip(*runs):
        assert np.array_equal(a_gt, b_gt) and np.array_equal(a_rgb, b_rgb)


class _ListLoader:
    def __init__(self, batches, device):
        self.batches = [(torch.from_numpy(d).to(device), torch.from_numpy(c).to(device)) for d, c in batches]

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for d, c in self.batches:
            yield d, c, d


@pytest.mark.parametrize("mode", ["DtoD", "RtoD"])
def test_gdn_main_trains_on_nyu(gpu, tmp_path, monkeypatch, mode):
    from gdn_amd import GDN_main, option
    from gdn_amd.datasets import GpuCropLoader, GpuNYUAugmentLoader, NYUdataset
    monkeypatch.chdir(tmp_path)
    data = tmp_path / "nyu"
    _write_nyu(data, 6, 320, 420, seed=2)
    for i in range(2):                                        # the test split feeds the validation loader
        depth, rgb = synthetic_nyu(np.random.RandomState(50 + i), 320, 420)
        for sub, arr in (("test/test_depths", depth.astype(np.uint16)), ("test/test_colors", rgb)):
            (data / sub).mkdir(parents=True, exist_ok=True)
            Image.fromarray(arr).save(data / sub / ("%05d.png" % i))
    H, W, steps = 96, 128, 3
    args = option.parse_args([str(data), "--dataset", "NYU", "--mode", mode, "--height", str(H), "--width", str(W),
                              "--batch_size", "2", "--epochs", "1", "--epoch_size", str(steps), "--seed", "4",
                              "--model_dir", str(tmp_path / "no_guide")])

    def loaders():
        ds = NYUdataset(str(data), args, seed=args.seed, train=True, mode=mode)
        train = GpuNYUAugmentLoader(ds, args.batch_size, gpu, H, W, mode=mode, seed=args.seed, drop_last=True,
                                    order_seed=args.seed + 1)
        val = GpuCropLoader(NYUdataset(str(data), args, seed=args.seed, train=False, mode=mode), args.batch_size, gpu, H, W)
        return ds, train, val

    ds, train, val = loaders()
    out = GDN_main.run(args, train_loader=train, val_loader=val)
    loss = (out if mode == "DtoD" else out[0]).item()
    assert np.isfinite(loss)

    ds, probe, val = loaders()                                # same seeds: the same draws, in the same order
    ref = list(_restated_batches(ds, probe, steps, H, W, mode, args.seed + 1))
    out_ref = GDN_main.run(args, train_loader=_ListLoader(ref, gpu), val_loader=val)
    loss_ref = (out_ref if mode == "DtoD" else out_ref[0]).item()
    assert np.float32(loss).tobytes() == np.float32(loss_ref).tobytes(), (loss, loss_ref)
