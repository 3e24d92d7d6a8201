"""GPU tests of the Eigen-split evaluation (--eval_protocol standard): gdn_depth_metrics_std and the two
flip kernels through gdn_amd.ops / calculate_error against the float64 numpy restatement (eval_std_numpy.py, pinned
without a GPU by test_eval_std_cpu.py), validate_std, and the command line end to end.

Bars: n, ratio and a1..a3 BITWISE (the float32-rounded depths and every comparison are the restatement's); the other
metrics at rtol 1e-12, the bar of the project's fixed-order float64 reductions; silog at rtol 1e-10 for its cancellation,
on inputs whose log error has std >= 0.1 |mean| (asserted)."""
import os
import pathlib
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import eval_std_numpy as S

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parent.parent
BITWISE, CLOSE, SILOG = [0, 1, 6, 7, 8], [2, 3, 4, 5, 9], 10
LEVELS = np.array([0.0, 0.0, 0.5, 2.25, 3.5, 7.25, 12.0, 20.5, 33.0, 47.75, 61.0, 79.5, 85.0])   # metres, all k / 256


def _check_rows(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    print(what, "got", got.tolist(), "want", want.tolist())
    assert got.shape == want.shape
    assert np.array_equal(got[:, BITWISE].view(np.int64), want[:, BITWISE].view(np.int64)), \
        (what, got[:, BITWISE], want[:, BITWISE])
    np.testing.assert_allclose(got[:, CLOSE], want[:, CLOSE], rtol=1e-12, atol=0, err_msg=what)
    np.testing.assert_allclose(got[:, SILOG], want[:, SILOG], rtol=1e-10, atol=0, err_msg=what)
    assert np.array_equal(got[:, 11], np.zeros(len(got)))


def _pool(maps, dtype, fill):
    pool = np.full((len(maps), max(m.shape[0] for m in maps), max(m.shape[1] for m in maps)), fill, dtype)
    for b, m in enumerate(maps):
        pool[b, :m.shape[0], :m.shape[1]] = m
    return pool


_SMALL = {}


def _small():
    """B = 3, prediction 8 x 12, ground truth 23 x 37, 24 x 36 and 8 x 12 in one 24 x 37 pool: a non-integer ratio, an
    integer one with edge clamping, the identity.  Ground truth from a dozen levels (long runs of ties for the select);
    the third prediction is quantised too."""
    if not _SMALL:
        r = np.random.RandomState(11)
        sizes = [(23, 37), (24, 36), (8, 12)]
        pred = np.clip(r.uniform(-0.95, 0.4, (3, 1, 8, 12)) + np.linspace(-0.05, 0.4, 8)[None, None, :, None], -1, 1)
        pred = pred.astype(np.float32)
        pred[2] = np.round(pred[2] * 8) / 8
        metres = [LEVELS[r.randint(0, len(LEVELS), s)].astype(np.float32) for s in sizes]
        _SMALL.update(sizes=sizes, pred=pred, metres=metres)
    return _SMALL


def _raw(metres, kind):
    if kind == 0:
        return [m.copy() for m in metres]
    if kind == 1:
        return [np.minimum(m * 256, 65535).astype(np.uint16) for m in metres]
    return [np.clip(m.astype(np.float64) / 80.0 * 2 - 1, -1, 1).astype(np.float32) for m in metres]


def _device_rows(gpu, pool, kind, sizes, pred, crop, med):
    from gdn_amd.calculate_error import compute_errors_std_device
    return compute_errors_std_device(torch.from_numpy(pool).to(gpu), sizes, torch.from_numpy(pred).to(gpu), crop=crop,
                                     median_scaling=med, gt_kind=kind).cpu().numpy()


@pytest.mark.parametrize("med", [False, True])
@pytest.mark.parametrize("crop", ["garg", "eigen", "none"])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_small_ragged_batch(gpu, kind, crop, med):
    d = _small()
    raw = _raw(d["metres"], kind)
    pool = _pool(raw, raw[0].dtype, 0)
    boxes = [S.eval_box(h, w, crop) for h, w in d["sizes"]]
    want = S.std_rows(pool, kind, boxes, d["pred"], median_scaling=med)
    assert (want[:, 0] > 0).all()                                      # no image is left out
    for b in range(3):
        mean, std = S.log_error_stats(pool[b], kind, boxes[b], d["pred"][b, 0], median_scaling=med)
        assert std >= 0.1 * abs(mean), (b, mean, std)
    got = _device_rows(gpu, pool, kind, d["sizes"], d["pred"], crop, med)
    _check_rows(got, want, "kind %d crop %s med %s" % (kind, crop, med))
    if not med:
        assert (got[:, 1] == 1.0).all()


def test_small_batch_valid_counts_are_odd_and_even():
    """The median takes one middle value or the mean of two: the inputs above must reach both."""
    d = _small()
    parities = set()
    for kind in (0, 1, 2):
        raw = _raw(d["metres"], kind)
        pool = _pool(raw, raw[0].dtype, 0)
        for crop in ("garg", "eigen", "none"):
            boxes = [S.eval_box(h, w, crop) for h, w in d["sizes"]]
            parities |= {int(n) % 2 for n in S.std_rows(pool, kind, boxes, d["pred"])[:, 0]}
    assert parities == {0, 1}


_NATIVE = {}


def _native():
    """B = 2, prediction 128 x 416, uint16 ground truth 375 x 1242 and 370 x 1226: many workgroups per image, a pixel
    count that is no multiple of any chunk, one image smaller than its pool."""
    if not _NATIVE:
        r = np.random.RandomState(5)
        sizes = [(375, 1242), (370, 1226)]
        yy = np.linspace(0, 1, 128)[:, None]
        pred = np.clip(0.7 - 1.5 * yy + 0.1 * np.sin(np.arange(416) / 17.0)[None] + r.normal(0, 0.08, (2, 1, 128, 416)), -1, 1)
        pred = pred.astype(np.float32)
        maps = []
        for i, (h, w) in enumerate(sizes):
            depth = 5.0 + 75.0 * (1 - np.linspace(0, 1, h))[:, None] ** 2 * (1.1 + 0.2 * i) + r.normal(0, 1.0, (h, w))
            u16 = np.clip(np.round(depth * 256), 0, 65535).astype(np.uint16)
            maps.append(np.where(r.rand(h, w) < 0.2, u16, 0).astype(np.uint16))
        pool = _pool(maps, np.uint16, 0)
        boxes = [S.eval_box(h, w, "garg") for h, w in sizes]
        _NATIVE.update(sizes=sizes, pred=pred, pool=pool, boxes=boxes,
                       want={med: S.std_rows(pool, 1, boxes, pred, median_scaling=med) for med in (False, True)})
    return _NATIVE


@pytest.mark.parametrize("med", [False, True])
def test_native_size(gpu, med):
    d = _native()
    want = d["want"][med]
    assert (want[:, 0] > 20000).all()
    for b in range(2):
        mean, std = S.log_error_stats(d["pool"][b], 1, d["boxes"][b], d["pred"][b, 0], median_scaling=med)
        assert std >= 0.1 * abs(mean), (b, mean, std)
    got = _device_rows(gpu, d["pool"], 1, d["sizes"], d["pred"], "garg", med)
    _check_rows(got, want, "native med %s" % med)


class _TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(0.9))

    def forward(self, x, istrain=False):
        return torch.tanh(x[:, :1] * self.w)


def test_image_without_valid_pixel(gpu, capsys):
    from gdn_amd.trainer import validate_std
    d = _small()
    raw = _raw(d["metres"], 1)
    raw[1] = np.zeros_like(raw[1])                                     # no LiDAR return anywhere
    pool = _pool(raw, np.uint16, 0)
    for med in (False, True):
        got = _device_rows(gpu, pool, 1, d["sizes"], d["pred"], "garg", med)
        assert got[1, 0] == 0 and np.isnan(got[1, 1:11]).all() and got[1, 11] == 0
        alone = _device_rows(gpu, pool[[0, 2]], 1, [d["sizes"][0], d["sizes"][2]], d["pred"][[0, 2]], "garg", med)
        assert np.array_equal(got[[0, 2]].view(np.int64), alone.view(np.int64))      # the others are unaffected
        _check_rows(alone, S.std_rows(pool[[0, 2]], 1, [S.eval_box(*d["sizes"][0], "garg"), S.eval_box(*d["sizes"][2], "garg")],
                                      d["pred"][[0, 2]], median_scaling=med), "beside an empty image, med %s" % med)
    # validate_std: five images in two batches, one of them empty; the mean is over the other four, per image
    r = np.random.RandomState(2)
    gt = np.clip(r.uniform(-0.9, 0.9, (5, 1, 16, 24)), -1, 1).astype(np.float32)
    gt[3] = -1.0                                                       # 0 m everywhere: below the cap
    x = (gt + r.normal(0, 0.1, gt.shape)).astype(np.float32)
    x[3:] *= 0.5                                                       # the second batch is worse than the first
    T = lambda a: torch.from_numpy(a).to(gpu)
    loader = [(T(x[:3]), T(x[:3]), T(gt[:3])), (T(x[3:]), T(x[3:]), T(gt[3:]))]
    net = _TinyNet().to(gpu)
    args = types.SimpleNamespace(eval_protocol="standard", eval_crop="none", median_scaling=True)
    errors, left_out, names = validate_std(args, loader, net, 0, None, "DtoD_test")
    assert left_out == 1 and names == S.ERROR_NAMES_STD
    assert "1 of 5 images" in capsys.readouterr().out
    with torch.no_grad():
        out = torch.cat([net(b[0]) for b in loader]).cpu().numpy()
    rows = S.std_rows(gt[:, 0], 2, [S.eval_box(16, 24, "none")] * 5, out, median_scaling=True)
    want, left = S.mean_rows(rows)
    assert left == 1
    np.testing.assert_allclose(errors, want, rtol=1e-10)
    batch_means = np.mean([S.mean_rows(rows[:3])[0], S.mean_rows(rows[3:])[0]], axis=0)
    assert np.abs(batch_means - want).max() > 1e-3                     # not the mean of batch means


def test_per_epoch_validation_follows_the_protocol(gpu, capsys):
    """Training: --eval_protocol standard replaces the per-epoch validation (ground truth: the loader's third tensor, kind 2);
    without the flag the reference's metrics are printed as ever."""
    from gdn_amd import trainer
    r = np.random.RandomState(4)
    gt = r.uniform(-0.9, 0.9, (4, 1, 16, 24)).astype(np.float32)
    x = (gt + r.normal(0, 0.1, gt.shape)).astype(np.float32)
    T = lambda a: torch.from_numpy(a).to(gpu)
    loader = [(T(x[:2]), T(x[:2]), T(gt[:2])), (T(x[2:]), T(x[2:]), T(gt[2:]))]
    net = _TinyNet().to(gpu)
    trainer._validate_epoch(types.SimpleNamespace(mode="DtoD"), loader, net, None, 0, None)
    assert " * Avg abs_diff : " in capsys.readouterr().out
    trainer._validate_epoch(types.SimpleNamespace(mode="DtoD", eval_protocol="standard", eval_crop="eigen"), loader, net, None, 0, None)
    line = [ln for ln in capsys.readouterr().out.splitlines() if " * Avg " in ln]
    assert len(line) == 1
    with torch.no_grad():
        out = torch.cat([net(b[0]) for b in loader]).cpu().numpy()
    want, left = S.mean_rows(S.std_rows(gt[:, 0], 2, [S.eval_box(16, 24, "eigen")] * 4, out))
    assert left == 0
    assert line[0].strip() == "* Avg " + ", ".join("{} : {:.3f}".format(n, e) for n, e in zip(S.ERROR_NAMES_STD, want))


def test_robustness(gpu):
    from gdn_amd import ops
    from gdn_amd._lib import GdnError
    from gdn_amd.calculate_error import eval_boxes
    d = _small()
    results = {}
    for kind, poison in ((0, np.float32("nan")), (1, np.uint16(0xFFFF)), (2, np.float32("nan"))):
        raw = _raw(d["metres"], kind)
        clean = _device_rows(gpu, _pool(raw, raw[0].dtype, 0), kind, d["sizes"], d["pred"], "garg", True)
        other = _device_rows(gpu, _pool(raw, raw[0].dtype, 0), kind, d["sizes"], d["pred"], "none", False)   # dirties the workspace
        poisoned = _device_rows(gpu, _pool(raw, raw[0].dtype, poison), kind, d["sizes"], d["pred"], "garg", True)
        again = _device_rows(gpu, _pool(raw, raw[0].dtype, 0), kind, d["sizes"], d["pred"], "garg", True)
        assert not np.array_equal(other.view(np.int64), clean.view(np.int64))
        assert np.array_equal(clean.view(np.int64), poisoned.view(np.int64)), kind     # the padding is never read
        assert np.array_equal(clean.view(np.int64), again.view(np.int64)), kind        # two calls: the same 96 B bytes
        results[kind] = clean
    # a NaN prediction at a valid pixel propagates into that image's sums and counts for no threshold; the others stand
    raw = _raw(d["metres"], 1)
    pool = _pool(raw, np.uint16, 0)
    pred = d["pred"].copy()
    pred[0] = np.float32("nan")
    got = _device_rows(gpu, pool, 1, d["sizes"], pred, "garg", True)
    assert got[0, 0] == results[1][0, 0] and np.isnan(got[0, 1:6]).all() and (got[0, 6:9] == 0).all()
    assert np.array_equal(got[1:].view(np.int64), results[1][1:].view(np.int64))
    # bad arguments
    gt = torch.from_numpy(pool).to(gpu)
    p = torch.from_numpy(d["pred"]).to(gpu)
    boxes = eval_boxes(d["sizes"], "garg").to(gpu)
    for kw in (dict(min_depth=0.0), dict(min_depth=-1.0), dict(max_depth=1e-3), dict(depth_scale=0.0), dict(min_depth=float("nan"))):
        with pytest.raises(GdnError, match="gdn_depth_metrics_std failed"):
            ops.depth_metrics_std(gt, 1, boxes, p, **kw)
    with pytest.raises(GdnError):
        ops.depth_metrics_std(gt, 3, boxes, p)
    with pytest.raises(GdnError):
        ops.depth_metrics_std(gt, 0, boxes, p)                         # uint16 data is kind 1
    with pytest.raises(GdnError):
        ops.depth_metrics_std(gt, 1, boxes[:2], p)
    ok = ops.depth_metrics_std(gt, 1, boxes, p, median_scaling=True).cpu().numpy()
    assert np.array_equal(ok.view(np.int64), results[1].view(np.int64))


@pytest.mark.parametrize("shape", [(3, 2, 5, 7), (5, 1, 13, 10), (1, 1, 1, 1), (4, 3, 128, 417)])
def test_flip_kernels_bitwise(gpu, shape):
    from gdn_amd import ops
    from gdn_amd._lib import GdnError
    g = torch.Generator().manual_seed(shape[-1])
    a = (torch.randn(shape, generator=g) * 3).to(gpu)
    b = (torch.randn(shape, generator=g) * 3).to(gpu)
    assert torch.equal(ops.flip_w(a), a.flip(-1))
    want = (a + b.flip(-1)) * 0.5
    assert torch.equal(ops.flip_mean(a, b), want)
    keep = a.clone()
    out = ops.flip_mean(a, b, out=a)                                   # out aliases a
    assert out.data_ptr() == a.data_ptr() and torch.equal(a, want)
    with pytest.raises(GdnError):
        ops.flip_mean(keep, b, out=b)
    with pytest.raises(GdnError):
        ops.flip_w(keep.double())


# ---------------------------------------------------------------------------------------------------------------------
# end to end through the CLI

def _run_cli(tmp_path, data, extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([str(REPO / "gdn-pytorch_amd"), str(REPO)] +
                                        ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "gdn_amd.GDN_main", str(data), "--mode", "DtoD_test",
           "--batch_size", "4", "--gpu_num", "0", "--model_dir", str(tmp_path / "ckpt.pkl"), "--real_test", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=700)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Results: ")]
    assert len(line) == 1, r.stdout[-2000:]
    return line[0], r.stdout


def _parse_std(line):
    body, _, tail = line[len("Results: "):].partition(" [standard: ")
    return [(m.group(1), float(m.group(2))) for m in re.finditer(r"(\w+) (-?[0-9.]+|nan)", body)], tail


def _eigen_split(root, n, H=128, W=416):
    """n samples in the layout of test_hip_eval.py's split, and their 16-bit ground truth at two native sizes."""
    from PIL import Image
    r = np.random.RandomState(9)
    yy, xx = np.mgrid[0:H, 0:W]
    lists = {"img": [], "color_gt": [], "gt": []}
    native, gt16 = [(375, 1242), (370, 1226)], []
    for i in range(n):
        d = root / ("2011_09_26_drive_%04d_sync" % i)
        d.mkdir(parents=True)
        dense = np.clip(40 + 150 * yy / H + 30 * np.sin(xx / (13.0 + i)) + r.randint(0, 20, (H, W)), 0, 255).astype(np.uint8)
        sparse = np.where(r.rand(H, W) < 0.1, dense, 0).astype(np.uint8)
        Image.fromarray(r.randint(0, 256, (H, W, 3)).astype(np.uint8)).save(d / "img.png")
        Image.fromarray(dense).save(d / "color_gt.png")
        Image.fromarray(sparse).save(d / "gt.png")
        for k in lists:
            lists[k].append("%s/%s.png" % (d.name, k))
        h, w = native[i % 2]
        metres = (4.0 + 6.0 * i) + 30.0 * (1 - np.linspace(0, 1, h))[:, None] + r.normal(0, 0.5, (h, w))   # nearer, image by image
        u16 = np.where(r.rand(h, w) < 0.15, np.clip(np.round(metres * 256), 1, 65535), 0).astype(np.uint16)
        Image.fromarray(u16).save(d / "velodyne16.png")
        gt16.append(u16)
    for k, v in lists.items():
        (root / ("eigen_test_files_%s.txt" % k)).write_text("\n".join(v) + "\n")
    (root / "eigen_test_files_gt16.txt").write_text(
        "\n".join("2011_09_26_drive_%04d_sync/velodyne16.png" % i for i in range(n)) + "\n")
    return gt16


def _save_checkpoint(path, H=128, W=416):
    import gdn_amd.AE_model_unet as M
    torch.manual_seed(123)
    m = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
    torch.save({"module." + k: v for k, v in m.state_dict().items()}, path)


def _assert_printed(printed, expected):
    assert [n for n, _ in printed] == S.ERROR_NAMES_STD
    for (n, v), e in zip(printed, expected):       # printed with 4 decimals
        assert abs(v - e) <= 5.1e-5 + 1e-5 * abs(e), (n, v, e)


def test_cli_standard_protocol_native_ground_truth(gpu, tmp_path):
    import gdn_amd.AE_model_unet as M
    from gdn_amd.datasets import GpuAugmentLoader, TestFolder
    from gdn_amd.trainer import load_checkpoint
    data = tmp_path / "eigen"
    gt16 = _eigen_split(data, 6)
    _save_checkpoint(tmp_path / "ckpt.pkl")
    lst = str(data / "eigen_test_files_gt16.txt")
    m = M.AutoEncoder_DtoD(input_dim=1, height=128, width=416)
    load_checkpoint(m, str(tmp_path / "ckpt.pkl"))
    m = m.to(gpu).eval()
    plain, merged, sizes = [], [], []
    for depth, _, _ in GpuAugmentLoader(TestFolder(str(data)), 4, gpu, train=False):
        with torch.no_grad():
            out = m(depth, istrain=False).float()
            mirrored = m(depth.flip(-1).contiguous(), istrain=False).float()
        plain.append(out.cpu().numpy())
        merged.append(((out + mirrored.flip(-1)) * 0.5).cpu().numpy())
        sizes.append(out.shape[0])
    assert sizes == [4, 2]                                             # a partial last batch
    pool = _pool(gt16, np.uint16, 0)
    boxes = [S.eval_box(*g.shape, "garg") for g in gt16]
    for extra, outs, med, words in (([], plain, False, ("median scaling off", "flip off")),
                                    (["--flip_test", "--median_scaling"], merged, True, ("median scaling on", "flip on"))):
        line, stdout = _run_cli(tmp_path, data, ["--eval_protocol", "standard", "--eval_gt_list", lst, *extra])
        printed, tail = _parse_std(line)
        rows = S.std_rows(pool, 1, boxes, np.concatenate(outs), median_scaling=med)
        want, left = S.mean_rows(rows)
        assert left == 0 and "images have no valid pixel" not in stdout
        _assert_printed(printed, want)
        for word in ("crop garg", "cap 0.001-80 m", "native size", "0 image(s) left out", *words):
            assert word in tail, tail
        batch_means = np.mean([S.mean_rows(rows[:4])[0], S.mean_rows(rows[4:])[0]], axis=0)
        assert np.abs(batch_means - want).max() > 1e-3, (batch_means, want)     # the per-image mean, and it shows


def test_cli_reference_protocol_unchanged(gpu, tmp_path):
    data = tmp_path / "eigen"
    _eigen_split(data, 2)
    _save_checkpoint(tmp_path / "ckpt.pkl")
    without, _ = _run_cli(tmp_path, data, [])
    with_flag, _ = _run_cli(tmp_path, data, ["--eval_protocol", "reference"])
    assert without == with_flag and "standard" not in without
    assert [m.group(1) for m in re.finditer(r"(\w+) (-?[0-9.]+|nan)", without[len("Results: "):])] == \
        ['abs_diff', 'abs_rel', 'sq_rel', 'a1', 'a2', 'a3', 'rmse', 'rmse_log']
