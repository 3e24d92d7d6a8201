"""CPU: the Eigen-split evaluation (--eval_protocol standard) without a GPU -- the numpy restatement
(eval_std_numpy.py) against an independent formulation, the crop boxes, the 16-bit ground-truth reader, the flag refusals
and the ABI of the three entry points."""
import ctypes
import pathlib
import re

import numpy as np
import pytest
import torch

import eval_std_numpy as S

REPO = pathlib.Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against torch's float64 bilinear interpolation, np.median and boolean masks

def _independent_row(g32, box, pred, scale, lo, hi, med):
    import torch.nn.functional as F
    h0, w0, y1, y2, x1, x2 = box
    u = (torch.from_numpy(pred.astype(np.float64)) + 1) / 2
    t = F.interpolate(u[None, None], size=(h0, w0), mode='bilinear', align_corners=False)[0, 0].numpy()
    p = np.maximum((t * np.float64(np.float32(scale))).astype(np.float32), 0)
    rows, cols = np.mgrid[0:h0, 0:w0]
    m = (g32 > np.float32(lo)) & (g32 < np.float32(hi)) & (rows >= y1) & (rows < y2) & (cols >= x1) & (cols < x2)
    g, p = g32[m].astype(np.float64), p[m].astype(np.float64)
    ratio = np.median(g) / np.median(p) if med else 1.0
    p = np.clip(p * ratio, np.float64(np.float32(lo)), np.float64(np.float32(hi)))
    th = np.maximum(g / p, p / g)
    e = np.log(p) - np.log(g)
    return np.array([m.sum(), ratio, np.mean(np.abs(g - p) / g), np.mean((g - p) ** 2 / g), np.sqrt(np.mean((g - p) ** 2)),
                     np.sqrt(np.mean((np.log(g) - np.log(p)) ** 2)), np.mean(th < 1.25), np.mean(th < 1.25 ** 2),
                     np.mean(th < 1.25 ** 3), np.mean(np.abs(np.log10(g) - np.log10(p))), 100 * np.sqrt(np.var(e)), 0.0])


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("med", [False, True])
@pytest.mark.parametrize("crop", ["garg", "eigen", "none"])
def test_restatement_matches_independent_formulation(seed, med, crop):
    r = np.random.RandomState(seed)
    pred = np.clip(r.uniform(-0.9, 0.6, (8, 12)) + np.linspace(-0.05, 0.3, 8)[:, None], -1, 1).astype(np.float32)
    for (h0, w0) in [(23, 37), (24, 36), (8, 12), (375, 1242)]:
        metres = (r.uniform(0.5, 90.0, (h0, w0)) * (r.rand(h0, w0) < 0.7)).astype(np.float32)
        box = S.eval_box(h0, w0, crop)
        got = S.std_row(metres, 0, box, pred, 80.0, 1e-3, 80.0, med)
        want = _independent_row(metres, box, pred, 80.0, 1e-3, 80.0, med)
        assert got[0] == want[0] > 0
        assert np.array_equal(got[6:9], want[6:9]), (h0, w0, got[6:9] * got[0], want[6:9] * got[0])   # no count differs
        np.testing.assert_allclose(got, want, rtol=1e-6)


def test_restatement_kinds_identity_and_empty():
    r = np.random.RandomState(3)
    pred = r.uniform(-1, 1, (8, 12)).astype(np.float32)
    # the identity: at the prediction's own size p is (float)((pred + 1) / 2 * scale) of the same pixel
    p = S.resample(pred, 8, 12, 80.0)
    assert np.array_equal(p, ((pred.astype(np.float64) + 1) / 2 * 80.0).astype(np.float32))
    # uint16 is metres x 256, exactly; kind 2 is the loaders' [-1, 1]
    u16 = r.randint(0, 65536, (8, 12)).astype(np.uint16)
    assert np.array_equal(S.gt_metres(u16, 1, 80.0), (u16 / 256.0).astype(np.float32))
    unit = r.uniform(-1, 1, (8, 12)).astype(np.float32)
    assert np.array_equal(S.gt_metres(unit, 2, 80.0), ((unit.astype(np.float64) + 1) / 2 * 80).astype(np.float32))
    # a perfect prediction: every error 0, every threshold 1
    row = S.std_row(unit, 2, S.eval_box(8, 12, 'none'), unit, 80.0, 1e-3, 80.0, True)
    assert row[0] > 0 and row[1] == 1.0 and np.all(row[2:6] == 0) and np.all(row[6:9] == 1) and row[9] == 0 and row[10] == 0
    # no valid pixel: {0, NaN x 10, 0}
    row = S.std_row(np.zeros((8, 12), np.uint16), 1, S.eval_box(8, 12, 'garg'), pred)
    assert row[0] == 0 and np.isnan(row[1:11]).all() and row[11] == 0
    # numpy's median: the mean of the two middle values
    assert S.median(np.array([4, 1, 3, 2], np.float32)) == 2.5 and S.median(np.array([5, 1, 3], np.float32)) == 3.0
    means, left = S.mean_rows(np.stack([row, S.std_row(unit, 2, S.eval_box(8, 12, 'none'), pred)]))
    assert left == 1 and not np.isnan(means).any()


# ---------------------------------------------------------------------------------------------------------------------
# crop boxes

BOXES = {  # computed by hand from the fractions of the two crops
    ("garg", 375, 1242): [375, 1242, 153, 371, 44, 1197],
    ("garg", 352, 1216): [352, 1216, 143, 349, 43, 1172],
    ("garg", 128, 416): [128, 416, 52, 126, 14, 401],
    ("eigen", 375, 1242): [375, 1242, 124, 342, 44, 1197],
    ("eigen", 352, 1216): [352, 1216, 117, 321, 43, 1172],
    ("eigen", 128, 416): [128, 416, 42, 116, 14, 401],
    ("none", 375, 1242): [375, 1242, 0, 375, 0, 1242],
}


def test_eval_boxes_hand_computed():
    from gdn_amd.calculate_error import ERROR_NAMES_STD, eval_boxes
    from gdn_amd._lib import GdnError
    assert ERROR_NAMES_STD == ['abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'a1', 'a2', 'a3', 'log10', 'silog'] == S.ERROR_NAMES_STD
    for (crop, h, w), want in BOXES.items():
        assert eval_boxes([(h, w)], crop).tolist() == [want], (crop, h, w)
        assert S.eval_box(h, w, crop) == want
    t = eval_boxes([(375, 1242), (352, 1216), (128, 416)], "garg")
    assert t.dtype == torch.int32 and tuple(t.shape) == (3, 6) and not t.is_cuda
    assert t.tolist() == [BOXES[("garg", 375, 1242)], BOXES[("garg", 352, 1216)], BOXES[("garg", 128, 416)]]
    with pytest.raises(GdnError):
        eval_boxes([(375, 1242)], "godard")


def test_mean_errors_std_is_per_image_and_counts_left_out():
    from gdn_amd.calculate_error import mean_errors_std
    rows = np.zeros((3, 12))
    rows[0] = [10, 1, *range(1, 10), 0]
    rows[1] = [0] + [np.nan] * 10 + [0]
    rows[2] = [30, 1, *range(3, 12), 0]
    means, left = mean_errors_std(torch.from_numpy(rows))
    assert left == 1 and means == [float(v) for v in range(2, 11)]
    means, left = mean_errors_std(torch.from_numpy(rows[1:2]))
    assert left == 1 and all(np.isnan(v) for v in means)


# ---------------------------------------------------------------------------------------------------------------------
# 16-bit ground truth

def test_eigen_gt16_round_trip_padding_and_refusal(tmp_path):
    from PIL import Image
    from gdn_amd._lib import GdnError
    from gdn_amd.datasets import EigenGt16, assemble_gt16
    r = np.random.RandomState(0)
    maps = [r.randint(0, 65536, s).astype(np.uint16) for s in [(23, 37), (24, 36), (8, 12)]]
    maps[0][0, :3] = [0, 1, 65535]
    (tmp_path / "sub").mkdir()
    names = []
    for i, m in enumerate(maps):
        Image.fromarray(m).save(tmp_path / "sub" / ("%d.png" % i))
        names.append("sub/%d.png extra tokens" % i if i else str(tmp_path / "sub" / "0.png"))     # absolute and relative
    (tmp_path / "gt16.txt").write_text("\n".join(names) + "\n\n")
    ds = EigenGt16(str(tmp_path / "gt16.txt"), str(tmp_path))
    assert len(ds) == 3
    for i, m in enumerate(maps):
        got = ds[i]
        assert got.dtype == np.uint16 and np.array_equal(got, m)
    pool, sizes = assemble_gt16([ds[i] for i in range(3)], "cpu")
    assert pool.dtype == torch.uint16 and tuple(pool.shape) == (3, 24, 37) and sizes == [(23, 37), (24, 36), (8, 12)]
    view = pool.numpy()
    for i, m in enumerate(maps):
        assert np.array_equal(view[i, :m.shape[0], :m.shape[1]], m)
        pad = view[i].copy()
        pad[:m.shape[0], :m.shape[1]] = 0
        assert not pad.any()
    Image.fromarray(r.randint(0, 256, (8, 12)).astype(np.uint8)).save(tmp_path / "eight.png")
    (tmp_path / "bad.txt").write_text("eight.png\n")
    with pytest.raises(GdnError, match="eight.png"):
        EigenGt16(str(tmp_path / "bad.txt"), str(tmp_path))[0]
    Image.fromarray(r.randint(0, 256, (8, 12, 3)).astype(np.uint8)).save(tmp_path / "rgb.png")
    (tmp_path / "bad2.txt").write_text("rgb.png\nmissing.png\n")
    with pytest.raises(GdnError, match="rgb.png"):
        EigenGt16(str(tmp_path / "bad2.txt"), str(tmp_path))[0]
    with pytest.raises(GdnError, match="missing.png"):
        EigenGt16(str(tmp_path / "bad2.txt"), str(tmp_path))[1]


def test_gt_list_must_be_as_long_as_the_split():
    import types
    from gdn_amd._lib import GdnError
    from gdn_amd.trainer import validate_std
    net = torch.nn.Linear(1, 1)
    loader = types.SimpleNamespace(ds=[0, 1, 2])
    with pytest.raises(GdnError, match="--eval_gt_list names 2 maps, the test split has 3"):
        validate_std(types.SimpleNamespace(eval_protocol="standard"), loader, net, 0, None, "DtoD_test", gt16=[None, None])


# ---------------------------------------------------------------------------------------------------------------------
# flags

STD = ["--eval_protocol", "standard"]


@pytest.mark.parametrize("flag, extra", [("--eval_crop", ["eigen"]), ("--min_depth", ["1"]), ("--max_depth", ["50"]),
                                         ("--depth_scale", ["80"]), ("--median_scaling", []), ("--flip_test", []),
                                         ("--eval_gt_list", ["gt.txt"])])
@pytest.mark.parametrize("proto", [[], ["--eval_protocol", "reference"]])
def test_new_flags_need_the_standard_protocol(flag, extra, proto):
    from gdn_amd import GDN_main, option
    argv = ["--synthetic", "--mode", "DtoD_test", "--real_test", flag, *extra, *proto]
    with pytest.raises(RuntimeError, match=re.escape(flag) + r"\b.*--eval_protocol standard"):
        GDN_main._check_eval(option.parse_args(argv))
    with pytest.raises(RuntimeError, match=re.escape(flag)):          # and run() says so before it touches the GPU
        GDN_main.main(argv)


def test_gt_list_and_dataset_refusals(tmp_path):
    from gdn_amd import GDN_main, option
    lst = tmp_path / "gt.txt"
    lst.write_text("a.png\n")
    with pytest.raises(RuntimeError, match="--eval_gt_list.*--mode DtoD"):
        GDN_main._check_eval(option.parse_args([*STD, "--mode", "DtoD", "--real_test", "--eval_gt_list", str(lst)]))
    with pytest.raises(RuntimeError, match="--eval_gt_list.*--real_test"):
        GDN_main._check_eval(option.parse_args([*STD, "--mode", "DtoD_test", "--eval_gt_list", str(lst)]))
    with pytest.raises(FileNotFoundError, match="--eval_gt_list"):
        GDN_main._check_eval(option.parse_args([*STD, "--mode", "RtoD_test", "--real_test", "--eval_gt_list",
                                                str(tmp_path / "none.txt")]))
    with pytest.raises(RuntimeError, match="--eval_protocol standard.*NYU"):
        GDN_main._check_eval(option.parse_args([*STD, "--mode", "DtoD_test", "--dataset", "NYU"]))
    with pytest.raises(RuntimeError, match="--min_depth"):
        GDN_main._check_eval(option.parse_args([*STD, "--min_depth", "0"]))
    with pytest.raises(RuntimeError, match="--max_depth"):
        GDN_main._check_eval(option.parse_args([*STD, "--min_depth", "5", "--max_depth", "5"]))
    with pytest.raises(RuntimeError, match="--depth_scale"):
        GDN_main._check_eval(option.parse_args([*STD, "--depth_scale", "-1"]))
    # what passes, and what it resolves to
    args = option.parse_args([*STD, "--mode", "DtoD_test", "--real_test", "--eval_gt_list", str(lst), "--flip_test"])
    GDN_main._check_eval(args)
    spec = option.eval_spec(args)
    assert spec == {"standard": True, "crop": "garg", "min_depth": 1e-3, "max_depth": 80.0, "depth_scale": 80.0,
                    "median_scaling": False, "flip_test": True, "gt_list": str(lst)}
    text = option.eval_describe(spec)
    for word in ("crop garg", "0.001-80 m", "median scaling off", "flip on", str(lst)):
        assert word in text, text
    plain = option.parse_args([])
    GDN_main._check_eval(plain)
    assert option.eval_spec(plain)["standard"] is False and plain.eval_protocol == "reference"


# ---------------------------------------------------------------------------------------------------------------------
# ABI

NEW_SYMBOLS = ("gdn_depth_metrics_std_workspace_bytes", "gdn_depth_metrics_std", "gdn_flip_w", "gdn_flip_mean")


def test_abi_new_symbols_at_revision_223():
    from gdn_amd import _lib as L
    header = (REPO / "include" / "gdn_hip.h").read_text()
    assert "size_t gdn_depth_metrics_std_workspace_bytes(int32_t B, int32_t Hmax, int32_t Wmax);" in header
    assert "int gdn_depth_metrics_std(const void* gt, int32_t gt_kind, int32_t Hmax, int32_t Wmax," in header
    assert "int gdn_flip_w(const float* src, int64_t rows, int32_t W, float* dst, void* stream);" in header
    assert "int gdn_flip_mean(const float* a, const float* b, int64_t rows, int32_t W, float* out, void* stream);" in header
    assert L.ABI_VERSION == 223 and int(L.lib.gdn_version()) == 223
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTS and L.lib.raw(name) is not None
    assert {"gdn_depth_metrics_std", "gdn_flip_w", "gdn_flip_mean"} <= L._STATUS_FUNCS
    assert len(L._SIGS["gdn_depth_metrics_std"][1]) == 17
    # the workspace holds both float32 planes of every image and grows with each dimension; bad sizes give 0
    q = L.lib.gdn_depth_metrics_std_workspace_bytes
    assert q(8, 375, 1242) >= 8 * 375 * 1242 * 8 and q(8, 375, 1242) > q(7, 375, 1242) > q(7, 374, 1242)
    assert q(0, 375, 1242) == 0 and q(1, 65536, 65536) == 0


def test_bad_arguments_are_refused_without_a_gpu():
    from gdn_amd import _lib as L
    P = ctypes.c_void_p(256)
    f = L.lib.raw("gdn_depth_metrics_std")

    def call(gt=P, kind=1, Hm=24, Wm=37, boxes=P, pred=P, B=3, H=8, W=12, scale=80.0, lo=1e-3, hi=80.0, med=0, out=P, ws=P,
             nb=1 << 30):
        return f(gt, kind, Hm, Wm, boxes, pred, B, H, W, scale, lo, hi, med, out, ws, nb, None)
    for bad in (dict(lo=0.0), dict(lo=-1.0), dict(hi=1e-3), dict(hi=1e-4), dict(scale=0.0), dict(lo=float("nan")),
                dict(hi=float("inf")), dict(kind=3), dict(kind=-1), dict(B=0), dict(H=0), dict(Wm=0), dict(gt=None),
                dict(boxes=None), dict(pred=None), dict(out=None), dict(Hm=65536, Wm=65536)):
        assert call(**bad) == -1, bad                     # GDN_ERR_BAD_ARG
    assert call(nb=16) == -3 and call(ws=None) == -3      # GDN_ERR_WORKSPACE
    with pytest.raises(L.GdnError, match="gdn_depth_metrics_std failed"):
        L.lib.gdn_depth_metrics_std(P, 1, 24, 37, P, P, 3, 8, 12, 80.0, 0.0, 80.0, 0, P, P, 1 << 30, None)
    fw, fm = L.lib.raw("gdn_flip_w"), L.lib.raw("gdn_flip_mean")
    assert fw(P, 4, 0, ctypes.c_void_p(512), None) == -1 and fw(P, 0, 4, ctypes.c_void_p(512), None) == -1
    assert fw(P, 4, 4, P, None) == -1 and fw(None, 4, 4, P, None) == -1          # in place is not a flip
    assert fm(P, ctypes.c_void_p(512), 4, 4, ctypes.c_void_p(512), None) == -1   # out may be a, not b
    assert fm(P, None, 4, 4, P, None) == -1 and fm(P, ctypes.c_void_p(512), 4, 0, P, None) == -1
