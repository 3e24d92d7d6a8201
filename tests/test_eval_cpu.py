"""CPU side of the evaluation path: the numpy restatement of the reference's metrics (the GPU tests' yardstick) against
the reference's own results, the Eigen / NYU test-set readers, CenterCrop's offsets, the CLI's dataset checks and the
new C-ABI symbols."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import eval_numpy as E

REPO = pathlib.Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["gdn_depth_metrics_nyu", "gdn_depth_metrics_nyu_workspace_bytes", "gdn_depth_metrics_make3d",
               "gdn_depth_metrics_make3d_workspace_bytes", "gdn_crop_normalize", "gdn_bytescale_u8"]


def test_golden_inputs_rebuild_bit_for_bit(golden):
    """metrics_eval.npz holds results, not inputs: the seeded rebuild must give the very inputs they were computed on."""
    g = golden["metrics_eval"]
    assert [str(c) for c in g["cases"]] == [c[0] for c in E.GOLDEN_CASES]
    for name, B, H, W, _ in E.GOLDEN_CASES:
        arrays = E.golden_inputs(name)
        assert all(a.shape == (B, 1, H, W) and a.dtype == np.float32 for a in arrays)
        assert E.inputs_digest(arrays) == str(g[name + "_digest"]), name


def test_restatement_matches_reference_nyu_make3d(golden):
    g = golden["metrics_eval"]
    for case in g["cases"]:
        s, gt, p = E.golden_inputs(str(case))
        np.testing.assert_allclose(E.nyu_per_image(gt, p, True), g[case + "_nyu_crop_per"], rtol=1e-5, err_msg=case)
        np.testing.assert_allclose(E.nyu_per_image(gt, p, False), g[case + "_nyu_nocrop_per"], rtol=1e-5, err_msg=case)
        np.testing.assert_allclose(E.make3d_per_image(s, gt, p), g[case + "_make3d_per"], rtol=1e-5, err_msg=case)
        np.testing.assert_allclose(E.compute_errors_NYU(gt, p, True), g[case + "_nyu_crop"], rtol=1e-5, err_msg=case)
        np.testing.assert_allclose(E.compute_errors_Make3D(s, gt, p), g[case + "_make3d"], rtol=1e-5, err_msg=case)


def test_restatement_matches_reference_kitti(golden):
    from oracle import gdn_oracle as O
    g = golden["losses"]
    depth, _, _ = O.synthetic_batch(3, 128, 416, seed=int(g["metrics.seed_depth"]))
    args = (g["metrics.sparse"], depth.numpy(), g["metrics.pred"])
    np.testing.assert_allclose(E.compute_errors(*args, crop=True), g["metrics.errors"], rtol=1e-5)
    np.testing.assert_allclose(E.compute_errors(*args, crop=False), g["metrics.errors_nocrop"], rtol=1e-5)


def test_restatement_bytescale_constant_image():
    assert (E.bytescale(np.full((1, 4, 5), 3.5, np.float32)) == 0).all()      # cscale 0 -> 1: (x - min) = 0 -> 0
    x = np.array([[[0.0, 1.0], [0.5, 0.25]]], np.float32)
    assert E.bytescale(x)[..., 0].tolist() == [[0, 255], [128, 64]]


def _png(path, a):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(a).save(path)


def test_test_folder_reads_eigen_lists_in_order(tmp_path):
    from gdn_amd._lib import GdnError
    from gdn_amd.datasets import TestFolder
    n, rows = 4, {"img": [], "color_gt": [], "gt": []}
    for i in range(n):
        rel = "2011_09_26/drive_%d" % (3 - i)           # list order differs from the sorted one
        _png(tmp_path / rel / "img.png", np.full((6, 10, 3), 10 + i, np.uint8))
        _png(tmp_path / rel / "color_gt.png", np.full((6, 10), 20 + i, np.uint8))
        _png(tmp_path / rel / "gt.png", np.full((6, 10), 30 + i, np.uint8))
        rows["img"].append("%s/img.png extra_token" % rel)
        rows["color_gt"].append("%s/color_gt.png" % rel)
        # one absolute entry: taken as written
        rows["gt"].append(str(tmp_path / rel / "gt.png") if i == 2 else "%s/gt.png" % rel)
    for k, lines in rows.items():
        (tmp_path / ("eigen_test_files_%s.txt" % k)).write_text("\n".join(lines) + "\n\n")
    ds = TestFolder(str(tmp_path), None)
    assert len(ds) == n
    for i in range(n):
        gt, rgb, sp = ds[i]
        assert gt.shape == (6, 10, 1) and rgb.shape == (6, 10, 3) and sp.shape == (6, 10, 1)
        assert (gt == 20 + i).all() and (rgb == 10 + i).all() and (sp == 30 + i).all()
    (tmp_path / "2011_09_26/drive_1/img.png").unlink()
    with pytest.raises(GdnError, match="drive_1/img.png"):
        ds[2]


def test_nyu_dataset_pairs_sorted_files(tmp_path):
    from gdn_amd._lib import GdnError
    from gdn_amd.datasets import NYUdataset
    for i in (2, 0, 1):
        _png(tmp_path / "test/test_depths" / ("%05d.png" % i), np.full((8, 12), 1000 * (i + 1), np.uint16))
        _png(tmp_path / "test/test_colors" / ("%05d.png" % i), np.full((8, 12, 3), i, np.uint8))
    ds = NYUdataset(str(tmp_path), None, train=False)
    assert len(ds) == 3
    for i in range(3):
        gt, rgb, gt2 = ds[i]
        assert gt2 is gt and gt.dtype == np.float32 and gt.shape == (8, 12, 1) and (gt == 1000 * (i + 1)).all()
        assert rgb.dtype == np.uint8 and rgb.shape == (8, 12, 3) and (rgb == i).all()
    with pytest.raises(GdnError, match="NYU training"):
        NYUdataset(str(tmp_path), None, train=True)


def test_center_crop_offsets_round_half_even():
    from gdn_amd import ops
    assert ops.center_crop_offsets(321, 420, 128, 416) == (96, 2)     # 96.5 -> 96
    assert ops.center_crop_offsets(323, 421, 128, 416) == (98, 2)     # 97.5 -> 98, 2.5 -> 2
    assert ops.center_crop_offsets(320, 420, 320, 420) == (0, 0)
    assert E.center_crop_offsets(321, 420, 128, 416) == ops.center_crop_offsets(321, 420, 128, 416)


@pytest.mark.parametrize("argv, match", [
    (["--dataset", "NYU", "--mode", "DtoD"], "NYU training is out of scope"),
    (["--dataset", "NYU", "--mode", "RtoD"], "NYU training is out of scope"),
    (["--dataset", "Make3D", "--mode", "DtoD_test"], "Make3D is not supported"),
    (["--dataset", "Make3D", "--mode", "DtoD"], "Make3D is not supported"),
])
def test_cli_rejects_unsupported_datasets(tmp_path, argv, match):
    from gdn_amd import GDN_main, option
    args = option.parse_args([str(tmp_path)] + argv)
    with pytest.raises(RuntimeError, match=match):
        GDN_main.run(args)


def test_new_symbols_resolve_from_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gdn_build", REPO / "gdn-pytorch_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    dll = ctypes.CDLL(str(mod.build()))
    hdr = (REPO / "include" / "gdn_hip.h").read_text()
    from gdn_amd import _lib as L
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(dll, name) and name in L.EXPORTS, name
    assert L.ABI_VERSION == 223 and L.lib.gdn_version() == 223
    assert L.lib.gdn_depth_metrics_nyu_workspace_bytes(7, 320, 420) == 7 * 8 * 8
    assert L.lib.gdn_depth_metrics_make3d_workspace_bytes(7, 320, 420) == 7 * 4 * 8
    # argument checks answer before anything reaches the GPU
    rc = L.lib.raw("gdn_crop_normalize")(ctypes.c_void_p(16), 0, 1, 10, 10, 3, 1, 0, 10, 10, ctypes.c_void_p(16), None)
    assert rc == -1                                                        # window leaves the image
    rc = L.lib.raw("gdn_crop_normalize")(ctypes.c_void_p(16), 0, 1, 10, 10, 4, 0, 0, 10, 10, ctypes.c_void_p(16), None)
    assert rc == -1                                                        # C > 3
    rc = L.lib.raw("gdn_depth_metrics_nyu")(ctypes.c_void_p(16), ctypes.c_void_p(16), 2, 8, 8, 1, ctypes.c_void_p(16),
                                            ctypes.c_void_p(16), 8, None)
    assert rc == -3                                                        # workspace too small
