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


EDGE_NAMES = [c[0] for c in E.EDGE_CASES]


def _images(case):
    """(gt_np, gt, pred) [H,W] of every image of an edge case."""
    s, g, p = E.edge_inputs(case)
    return [(s[b, 0], g[b, 0], p[b, 0]) for b in range(g.shape[0])]


def test_edge_inputs_rebuild_bit_for_bit(golden):
    g = golden["metrics_edges"]
    assert [str(c) for c in g["cases"]] == EDGE_NAMES
    for name, _, B, H, W, _ in E.EDGE_CASES:
        arrays = E.edge_inputs(name)
        assert all(a.shape == (B, 1, H, W) and a.dtype == np.float32 for a in arrays), name
        assert E.inputs_digest(arrays) == str(g[name + "_digest"]), name
        assert H * W <= 3328


def test_edge_set_sizes_and_valid_counts():
    """The set straddles the 1024-thread workgroup and the 64-lane wave, holds one and two valid pixels, and even and odd
    valid counts under both masks (the lower median of an even count is where an upper median would differ)."""
    sizes = {c[3] * c[4] for c in E.EDGE_CASES}
    assert {24, 1023, 1024, 1025, 3328} <= sizes and min(sizes) < 64
    (s, g, p), = _images("s4x6")
    assert E.Rules.box(4, 6, *E.KITTI_BOX) == (int(0.33 * 4), 3, 0, 5)
    assert E.kitti_masked(s, g, p, True)[0].size == 1
    (s, g, p), = _images("two")
    assert [E.kitti_masked(s, g, p, c)[0].size for c in (True, False)] == [2, 2]
    assert [E.nyu_masked(g, p, c)[0].size for c in (True, False)] == [2, 2]
    nk = [E.kitti_masked(*im, c)[0].size for n in EDGE_NAMES for im in _images(n) for c in (True, False)]
    nn = [E.nyu_masked(im[1], im[2], c)[0].size for n in EDGE_NAMES for im in _images(n) for c in (True, False)]
    for counts in (nk, nn):
        assert any(n > 1 and n % 2 == 0 for n in counts) and any(n > 1 and n % 2 == 1 for n in counts)
        assert 0 in counts


def test_edge_medians_straddle_a_radix_bucket():
    """The two middle values of the valid gt lie on either side of 8.0, those of the valid pred on either side of 2.0: the
    top byte of the float32 bit pattern, the first digit of the kernels' radix select, changes there."""
    for case, which, edge in (("bucket_g", 0, 8.0), ("bucket_p", 1, 2.0)):
        (s, g, p), = _images(case)
        for crop in (True, False):
            v = np.sort(E.kitti_masked(s, g, p, crop)[which])
            assert v.size % 2 == 0 and v.size >= 64
            lo, hi = v[v.size // 2 - 1], v[v.size // 2]
            assert lo < edge <= hi, (case, lo, hi)
            assert lo.view(np.uint32) >> 24 != hi.view(np.uint32) >> 24
            assert E._median(v) == lo


def test_edge_thresholds_tie_exactly():
    """`thresh`: float32 thresh equals 1.25, 1.5625 and 1.953125 on at least 32 valid pixels each, under the KITTI and the
    NYU mask.  The comparison is strict, so none of them counts; a1..a3 hold exactly the pixels strictly below."""
    (s, g, p), = _images("thresh")
    for crop in (True, False):
        for (vg, vp), lo, hi, row in ((E.kitti_masked(s, g, p, crop), 1, 80, E._per_image_kitti(s, g, p, crop)),
                                      (E.nyu_masked(g, p, crop), 1e-3, 10, E._per_image_nyu(g, p, crop))):
            _, th = E.scaled_thresh(vg, vp, lo, hi)
            assert th.dtype == np.float32
            for k, bound in enumerate((1.25, 1.5625, 1.953125)):
                assert int((th == np.float32(bound)).sum()) >= 32, (crop, bound)
                assert row[3 + k] == (th < bound).sum() / th.size
                assert row[3 + k] < (th <= bound).sum() / th.size


def test_edge_sparse_nan_only_drops_its_pixel():
    (s, g, p), = _images("sparse_nan")
    y, x = E.NAN_AT
    assert np.isnan(s[y, x]) and np.isfinite(E._per_image_kitti(s, g, p, True)).all()
    s2 = s.copy()
    s2[y, x] = 0.0
    assert E.kitti_masked(s2, g, p, True)[0].size == E.kitti_masked(s, g, p, True)[0].size + 1


def _assert_rows(got, want, msg):
    assert got.shape == want.shape, msg
    assert np.array_equal(np.isnan(got), np.isnan(want)), msg
    np.testing.assert_allclose(got, want, rtol=1e-5, err_msg=msg)          # NaN == NaN here; positions checked above


def test_restatement_matches_reference_edges(golden):
    """The restatement against the reference's own results on the edge inputs, image by image: the same NaN positions
    (the reference's NaN rows where it raises included) and finite values at rtol 1e-5."""
    g = golden["metrics_edges"]
    for case in EDGE_NAMES:
        s, gt, p = E.edge_inputs(case)
        for crop, tag in ((True, "crop"), (False, "nocrop")):
            _assert_rows(E.kitti_per_image(s, gt, p, crop), g["%s_kitti_%s_per" % (case, tag)], (case, "kitti", tag))
            _assert_rows(E.nyu_per_image(gt, p, crop), g["%s_nyu_%s_per" % (case, tag)], (case, "nyu", tag))
        _assert_rows(E.make3d_per_image(s, gt, p), g[case + "_make3d_per"], (case, "make3d"))
    rows = g["pred_const_kitti_crop_per"][0]
    assert np.isnan(rows[[0, 1, 2, 6, 7]]).all() and (rows[3:6] == 0).all()
    assert np.isnan(g["gt_nan_kitti_crop_per"]).all() and np.isnan(g["gt_nan_make3d_per"]).all()
    mixed = g["mixed_kitti_crop_per"].mean(0)
    assert np.array_equal(np.isnan(mixed), np.isnan(E.compute_errors(*E.edge_inputs("mixed")))) and np.isnan(mixed).all()


def test_restatement_matches_reference_kitti_on_eval_cases(golden):
    """compute_errors of the reference on the inputs of metrics_eval.npz (the tie cases among them)."""
    g = golden["metrics_edges"]
    for case in [c[0] for c in E.GOLDEN_CASES]:
        s, gt, p = E.golden_inputs(case)
        for crop, tag in ((True, "crop"), (False, "nocrop")):
            _assert_rows(E.kitti_per_image(s, gt, p, crop), g["%s_kitti_%s_per" % (case, tag)], (case, tag))
            _assert_rows(E.compute_errors(s, gt, p, crop), g["%s_kitti_%s" % (case, tag)], (case, tag))


def _upper_median(v):
    return np.float32("nan") if np.isnan(v).any() else np.sort(v)[v.size // 2]


def _shifted(dy, dx):
    def box(H, W, fy, fx):
        y1, y2, x1, x2 = E.Rules.box(H, W, fy, fx)
        return y1 + dy, y2 + dy, x1 + dx, x2 + dx
    return staticmethod(box)


def _nanskip(f):
    def g(x):
        return f(x) if not np.isnan(x).all() else np.float32("nan")
    return staticmethod(g)


WRONG = {
    "upper median": dict(median=staticmethod(_upper_median)),
    "<= at the thresholds": dict(less=staticmethod(np.less_equal)),
    "crop one row down": dict(box=_shifted(1, 0)),
    "crop one row up": dict(box=_shifted(-1, 0)),
    "crop one column right": dict(box=_shifted(0, 1)),
    "crop one column left": dict(box=_shifted(0, -1)),
    "clamp drops NaN": dict(clip=staticmethod(lambda v, lo, hi: np.fmin(np.fmax(v, lo), hi))),
    "min/max skip NaN": dict(amin=_nanskip(np.nanmin), amax=_nanskip(np.nanmax)),
}
# the log metrics' bar of test_hip_metric_edges.py can only be smaller than this cap
LOG_BAR_CAP = 1e-5


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_edge_cases_catch_wrong_variants(wrong):
    """Each wrong variant of the arithmetic, run in the restatement's place, misses the bars the kernels are held to
    (test_hip_metric_edges.py) on at least one edge case -- per kernel it can affect: the cases can catch that error."""
    R = type("Wrong", (E.Rules,), WRONG[wrong])
    caught = {"kitti": [], "nyu": [], "make3d": []}
    for case in EDGE_NAMES:
        s, gt, p = E.edge_inputs(case)
        for crop in (True, False):
            for kind, fn, args in (("kitti", E.kitti_per_image, (s, gt, p, crop)), ("nyu", E.nyu_per_image, (gt, p, crop)),
                                   ("make3d", E.make3d_per_image, (s, gt, p))):
                for got, want in zip(fn(*args, R=R), fn(*args)):
                    if E.row_mismatch(got.astype(np.float32), want, kind, LOG_BAR_CAP):
                        caught[kind].append(case)
    applies = {"kitti", "nyu", "make3d"}
    if "threshold" in wrong or "crop" in wrong:
        applies.discard("make3d")               # Make3D has neither thresholds nor a crop box
    for kind in sorted(applies):
        assert caught[kind], "%s survives every edge case of %s" % (wrong, kind)


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
