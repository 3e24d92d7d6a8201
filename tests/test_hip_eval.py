"""GPU tests of the evaluation path: the NYU / Make3D metric kernels against the reference's results
(metrics_eval.npz), the NYU crop / normalise and --img_save bytescale kernels bit-exact against numpy, and the CLI end to
end (--real_test --img_save on a synthetic Eigen split, --dataset NYU on synthetic NYU files) against the numpy
restatement of the reference's metrics (eval_numpy.py)."""
import os
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_numpy as E

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parent.parent
CASES = ["kitti", "nyu", "kitti_tie", "nyu_tie", "small"]


def _case(golden, case, gpu):
    """The seeded inputs of one golden case (pinned by its digest) on the GPU, and the golden."""
    g = golden["metrics_eval"]
    arrays = E.golden_inputs(case)
    assert E.inputs_digest(arrays) == str(g[case + "_digest"]), case
    return [torch.from_numpy(a).to(gpu) for a in arrays], g


@pytest.mark.parametrize("case", CASES)
def test_nyu_make3d_metrics_match_reference(gpu, golden, case):
    from gdn_amd.calculate_error import compute_errors_Make3D, compute_errors_NYU
    (s, gt, p), g = _case(golden, case, gpu)
    np.testing.assert_allclose(compute_errors_NYU(gt, p, crop=True), g[case + "_nyu_crop"], rtol=1e-4)
    np.testing.assert_allclose(compute_errors_NYU(gt, p, crop=False), g[case + "_nyu_nocrop"], rtol=1e-4)
    np.testing.assert_allclose(compute_errors_Make3D(s, gt, p), g[case + "_make3d"], rtol=1e-4)


@pytest.mark.parametrize("case", ["kitti", "nyu_tie", "small"])
def test_metrics_single_images(gpu, golden, case):
    """B = 1: every image on its own against the reference's per-image result."""
    from gdn_amd.calculate_error import compute_errors_Make3D, compute_errors_NYU
    (s, gt, p), g = _case(golden, case, gpu)
    for b in range(gt.shape[0]):
        sl = slice(b, b + 1)
        np.testing.assert_allclose(compute_errors_NYU(gt[sl], p[sl], crop=True), g[case + "_nyu_crop_per"][b], rtol=1e-4)
        np.testing.assert_allclose(compute_errors_NYU(gt[sl], p[sl], crop=False), g[case + "_nyu_nocrop_per"][b],
                                   rtol=1e-4)
        np.testing.assert_allclose(compute_errors_Make3D(s[sl], gt[sl], p[sl]), g[case + "_make3d_per"][b], rtol=1e-4)


def test_metrics_batch_of_seven(gpu, golden):
    from gdn_amd.calculate_error import compute_errors_Make3D_device, compute_errors_NYU_device
    (s, gt, p), g = _case(golden, "small", gpu)
    assert gt.shape[0] == 7
    got = compute_errors_NYU_device(gt, p, crop=True).cpu().numpy()
    np.testing.assert_allclose(got, g["small_nyu_crop_per"].mean(0), rtol=1e-4)
    got = compute_errors_Make3D_device(s, gt, p).cpu().numpy()
    np.testing.assert_allclose(got, g["small_make3d_per"].mean(0), rtol=1e-4)


def test_metrics_without_valid_pixel_are_nan(gpu):
    """A constant ground truth leaves no valid pixel (the reference raises on the empty median): NaN for that image."""
    from gdn_amd.calculate_error import compute_errors_Make3D, compute_errors_NYU
    r = np.random.RandomState(5)
    gt = torch.from_numpy(r.rand(2, 1, 16, 24).astype(np.float32)).to(gpu)
    p = torch.from_numpy(r.rand(2, 1, 16, 24).astype(np.float32)).to(gpu)
    gt[1] = 3.0
    assert all(np.isnan(v) for v in compute_errors_NYU(gt, p))
    assert all(np.isnan(v) for v in compute_errors_Make3D(gt, gt, p))
    assert not any(np.isnan(v) for v in compute_errors_NYU(gt[:1], p[:1]))


@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape, out, off", [((320, 420), (128, 416), None), ((321, 423), (128, 416), None),
                                             ((37, 51), (20, 30), (3, 7)), ((37, 51), (20, 30), (17, 21))])
def test_crop_normalize_bit_exact(gpu, dtype, C, shape, out, off):
    from gdn_amd import ops
    r = np.random.RandomState(C + shape[0])
    B = 3
    if dtype == "u8":
        a = r.randint(0, 256, (B, *shape, C)).astype(np.uint8)
    else:           # 16-bit depth as decoded to float32: NOT bytescaled
        a = r.randint(0, 65536, (B, *shape, C)).astype(np.float32)
    H, W = out
    i, j = E.center_crop_offsets(*shape, H, W) if off is None else off
    got = ops.crop_normalize(torch.from_numpy(a).to(gpu), H, W, None if off is None else off).cpu().numpy()
    assert got.shape == (B, C, H, W)
    for b in range(B):
        ref = E.crop_normalize(a[b], i, j, H, W)
        assert np.array_equal(got[b], ref), "image %d: %d elements differ" % (b, int((got[b] != ref).sum()))


def test_crop_normalize_rejects_window_outside(gpu):
    from gdn_amd import ops
    from gdn_amd._lib import GdnError
    src = torch.zeros((1, 10, 12, 3), dtype=torch.uint8, device=gpu)
    with pytest.raises(GdnError):
        ops.crop_normalize(src, 8, 8, (3, 0))


@pytest.mark.parametrize("C", [1, 3])
def test_bytescale_bit_exact(gpu, C):
    from gdn_amd import ops
    r = np.random.RandomState(C)
    x = (r.standard_normal((4, C, 37, 53)) * r.uniform(0.01, 50)).astype(np.float32)
    x[1] = np.float32(0.75)                         # constant image: cscale 0 -> 1
    x[2] = np.round(x[2] * 4) / 4                   # many exact .5 steps after scaling
    got = ops.bytescale_u8(torch.from_numpy(x).to(gpu)).cpu().numpy()
    assert got.shape == (4, 37, 53, C) and got.dtype == np.uint8
    for b in range(4):
        assert np.array_equal(got[b], E.bytescale(x[b])), "image %d" % b
    assert (got[1] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# end to end through the CLI

def _save_checkpoint(path, H=128, W=416):
    import gdn_amd.AE_model_unet as M
    torch.manual_seed(123)
    m = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
    torch.save({"module." + k: v for k, v in m.state_dict().items()}, path)


def _run_cli(tmp_path, data, extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([str(REPO / "gdn-pytorch_amd"), str(REPO)] +
                                        ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "gdn_amd.GDN_main", str(data), "--mode", "DtoD_test",
           "--batch_size", "4", "--gpu_num", "0", "--model_dir", str(tmp_path / "ckpt.pkl"), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=700)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Results: ")]
    assert len(line) == 1, r.stdout[-2000:]
    return [(m.group(1), float(m.group(2))) for m in re.finditer(r"(\w+) (-?[0-9.]+|nan)", line[0][len("Results: "):])]


def _outputs(gpu, tmp_path, loader):
    """The model of the checkpoint over `loader`, batch by batch: (depth, rgb, depth_np, out) as numpy."""
    import gdn_amd.AE_model_unet as M
    from gdn_amd.trainer import load_checkpoint
    m = M.AutoEncoder_DtoD(input_dim=1, height=128, width=416)
    load_checkpoint(m, str(tmp_path / "ckpt.pkl"))
    m = m.to(gpu).eval()
    res = []
    for depth, img, depth_np in loader:
        with torch.no_grad():
            out = m(depth, istrain=False)
        res.append(tuple(t.cpu().numpy() for t in (depth, img, depth_np, out)))
    return res


def _assert_printed(printed, names, expected):
    assert [n for n, _ in printed] == names
    for (n, v), e in zip(printed, expected):       # printed with 4 decimals
        assert abs(v - e) <= 5.1e-5 + 1e-5 * abs(e), (n, v, e)


def _eigen_split(root, n=10, H=128, W=416):
    from PIL import Image
    r = np.random.RandomState(9)
    yy, xx = np.mgrid[0:H, 0:W]
    lists = {"img": [], "color_gt": [], "gt": []}
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
    for k, v in lists.items():
        (root / ("eigen_test_files_%s.txt" % k)).write_text("\n".join(v) + "\n")


def test_cli_eigen_real_test_img_save(gpu, tmp_path):
    from PIL import Image
    from gdn_amd.calculate_error import ERROR_NAMES
    from gdn_amd.datasets import GpuAugmentLoader, TestFolder
    data, res = tmp_path / "eigen", tmp_path / "results"
    _eigen_split(data)
    _save_checkpoint(tmp_path / "ckpt.pkl")
    printed = _run_cli(tmp_path, data, ["--real_test", "--img_save", "--result_dir", str(res)])
    batches = _outputs(gpu, tmp_path, GpuAugmentLoader(TestFolder(str(data)), 4, gpu, train=False))
    assert [b[0].shape[0] for b in batches] == [4, 4, 2]
    expected = np.mean([E.compute_errors(dn, d, o, crop=True) for d, _, dn, o in batches], axis=0)
    _assert_printed(printed, ERROR_NAMES, expected)
    for folder, name in (("output_depth", "final_AE_depth_"), ("ground_truth", "final_AE_gt_"),
                         ("input_rgb", "final_AE_rgb_")):
        files = sorted(os.listdir(res / folder))
        assert files == ["%s%05d.jpg" % (name, k) for k in range(10)], files
    with Image.open(res / "output_depth" / "final_AE_depth_00000.jpg") as im:
        assert im.mode == "L" and im.size == (416, 128)
        jpg = np.asarray(im).astype(np.float64)
    want = E.bytescale(batches[0][3][0])[..., 0]
    import io
    buf = io.BytesIO()
    Image.fromarray(want).save(buf, format="JPEG")            # PIL's default quality, as the CLI writes it
    with Image.open(buf) as im:
        want_jpg = np.asarray(im).astype(np.float64)
    # the same pixels through the same encoder: equal up to the odd byte that a last-bit difference of the
    # forward in this process can move across a bytescale rounding boundary
    assert np.abs(jpg - want_jpg).mean() < 0.05, np.abs(jpg - want_jpg).mean()
    assert np.abs(jpg - want.astype(np.float64)).mean() < 16.0                  # and JPEG-close to the raw bytes
    with Image.open(res / "input_rgb" / "final_AE_rgb_00009.jpg") as im:
        assert im.mode == "RGB" and im.size == (416, 128)


def test_cli_nyu_test_set(gpu, tmp_path):
    from PIL import Image
    from gdn_amd.calculate_error import ERROR_NAMES_NYU
    from gdn_amd.datasets import GpuCropLoader, NYUdataset
    data = tmp_path / "nyu"
    (data / "test" / "test_depths").mkdir(parents=True)
    (data / "test" / "test_colors").mkdir(parents=True)
    r = np.random.RandomState(4)
    yy, xx = np.mgrid[0:320, 0:420]
    raw = []
    for i in range(6):
        depth = (6000 + 20 * yy + 8 * xx * (i + 1) + r.randint(0, 500, (320, 420))).astype(np.uint16)
        rgb = r.randint(0, 256, (320, 420, 3)).astype(np.uint8)
        Image.fromarray(depth).save(data / "test" / "test_depths" / ("%04d.png" % i))
        Image.fromarray(rgb).save(data / "test" / "test_colors" / ("%04d.png" % i))
        raw.append((depth, rgb))
    _save_checkpoint(tmp_path / "ckpt.pkl")
    printed = _run_cli(tmp_path, data, ["--dataset", "NYU"])
    loader = GpuCropLoader(NYUdataset(str(data), None, train=False), 4, gpu, 128, 416)
    batches = _outputs(gpu, tmp_path, loader)
    # the loader's transform: CenterCrop 320x420 -> 128x416 at (96, 2), /255, Normalize
    d0, rgb0 = batches[0][0][0], batches[0][1][0]
    assert np.array_equal(d0, E.crop_normalize(raw[0][0][:, :, None].astype(np.float32), 96, 2, 128, 416))
    assert np.array_equal(rgb0, E.crop_normalize(raw[0][1], 96, 2, 128, 416))
    expected = np.mean([E.compute_errors_NYU(d, o, crop=True) for d, _, _, o in batches], axis=0)
    _assert_printed(printed, ERROR_NAMES_NYU, expected)
