"""CPU: the Velodyne ground truth (--eval_velodyne) without a GPU -- the float64 restatement against the
published host routine, the key transform, the calibration and list readers, the flag refusals, the entry point's argument
checks."""
import ctypes
import pathlib
import re
import types

import numpy as np
import pytest
import torch

import velo_numpy as V
import velo_synth as Y

REPO = pathlib.Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------------------------------------------------
# restatement == published routine

@pytest.mark.parametrize("vel_depth", [False, True])
def test_restatement_equals_published_routine_bitwise(vel_depth):
    """40 seeded clouds on a 24 x 40 image (960 pixels each), ~3 points per pixel, points beyond every border and behind the
    scanner.  Every projected coordinate is built >= 0.05 px away from a .5, so that np.dot's sums (BLAS may fuse them)
    cannot round to another pixel than the elementwise form.  Pixel column 0 is left empty: the published routine finds its
    duplicates through a linear index that aliases (r, w0 - 1) with (r + 1, 0) and then writes the minimum of BOTH pixels
    into one of them; the specification is the per-pixel minimum."""
    cam, velo = Y.calib_arrays(seed=1)
    P, size = Y.compose(cam, velo, 2, size=(24, 40))
    differ = filled = 0
    for seed in range(40):
        pts = Y.seeded_cloud(P, size, 3000, seed, first_col=1)
        want = V.published(pts, P, size, vel_depth).astype(np.float32)
        got, hits = V.restate(pts, P, size, int(vel_depth))
        differ += int((got.view(np.uint32) != want.view(np.uint32)).sum())
        filled += hits
        assert hits == int((want > 0).sum())
    assert differ == 0 and filled > 40 * 800


def test_restatement_semantics_by_hand():
    P = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]], np.float64)        # u = y / x, v = z / x, depth x
    pts = np.array([[2, 5, 3, 9],        # u = rint(2.5) - 1 = 1, v = rint(1.5) - 1 = 1
                    [4, 6, 8, 9],        # u = rint(1.5) - 1 = 1, v = 1: the same pixel, farther
                    [2, 7, 1, 9],        # u = rint(3.5) - 1 = 3, v = rint(0.5) - 1 = -1: dropped
                    [-1, -3, -2, 9],     # behind the scanner
                    [2, 1, 2, 9]],       # u = rint(0.5) - 1 = -1: dropped
                   np.float32)
    got, hits = V.restate(pts, P, (3, 5))
    want = np.zeros((3, 5), np.float32)
    want[1, 1] = 2.0
    assert np.array_equal(got, want) and hits == 1
    pool, _ = V.restate(pts, P, (3, 5), pool=(4, 7))
    assert pool.shape == (4, 7) and np.array_equal(pool[:3, :5], want) and not pool[3:].any() and not pool[:, 5:].any()


# ---------------------------------------------------------------------------------------------------------------------
# the order-preserving key

def test_key_round_trip_and_order():
    tiny, big = np.float32(1e-45), np.finfo(np.float32).max
    ladder = np.array([-np.inf, -big, -1.5, -1.0, -np.finfo(np.float32).tiny, -3 * tiny, -tiny, -0.0, 0.0, tiny, 3 * tiny,
                       np.finfo(np.float32).tiny, 1.0, 1.5, 79.99, 80.0, big, np.inf], np.float32)
    keys = V.key_of(ladder)
    assert keys.dtype == np.uint32 and np.all(keys[1:] > keys[:-1])                  # -0 sorts below +0
    assert np.array_equal(V.float_of(keys).view(np.uint32), ladder.view(np.uint32))  # bits, so -0 stays -0
    assert keys.max() < V.EMPTY and keys[8] == 0x80000000 and keys[7] == 0x7FFFFFFF and keys[0] == 0x007FFFFF
    r = np.random.RandomState(0)
    bits = r.randint(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    f = bits.view(np.float32)
    f = f[~np.isnan(f)]
    k = V.key_of(f)
    assert np.array_equal(V.float_of(k).view(np.uint32), f.view(np.uint32))
    order = np.argsort(k, kind="stable")
    assert np.all(np.diff(f[order].astype(np.float64)) >= 0)
    assert np.isnan(V.float_of(V.EMPTY))                                             # the sentinel decodes to "not > 0"


# ---------------------------------------------------------------------------------------------------------------------
# calibration and lists

def test_read_calib_and_projection(tmp_path):
    from gdn_amd import kitti_raw as K
    from gdn_amd._lib import GdnError
    cam, velo = Y.write_calib(tmp_path / "2011_09_26", seed=3)
    c = K.read_calib(tmp_path / "2011_09_26" / "calib_cam_to_cam.txt")
    assert "calib_time" not in c and c["corner_dist"].tolist() == [0.0995]
    for k, v in cam.items():
        assert c[k].dtype == np.float64 and np.array_equal(c[k], v), k
    v2c = K.read_calib(tmp_path / "2011_09_26" / "calib_velo_to_cam.txt")
    assert "calib_time" not in v2c and np.array_equal(v2c["R"], velo["R"]) and np.array_equal(v2c["T"], velo["T"])
    for camera in (2, 3):
        P, size = K.projection(tmp_path / "2011_09_26", camera)
        want, wsize = Y.compose(cam, velo, camera)
        assert P.dtype == np.float64 and P.shape == (3, 4) and np.array_equal(P, want)
        assert size == wsize == (375, 1242)                                          # S_rect stores the width first
    P2, _ = K.projection(tmp_path / "2011_09_26")
    assert np.array_equal(P2, Y.compose(cam, velo, 2)[0])                            # cam defaults to 2
    # size=: rows 0 and 1 of P_rect scaled BEFORE the composition
    Ps, ssize = K.projection(tmp_path / "2011_09_26", 2, size=(128, 416))
    want, _ = Y.compose(cam, velo, 2, size=(128, 416))
    assert ssize == (128, 416) and np.array_equal(Ps, want)
    full = Y.compose(cam, velo, 2)[0]
    np.testing.assert_allclose(Ps[0], full[0] * (416 / 1242), rtol=1e-12)
    np.testing.assert_allclose(Ps[1], full[1] * (128 / 375), rtol=1e-12)
    assert np.array_equal(Ps[2], full[2])
    with pytest.raises(GdnError, match="calib_cam_to_cam.txt"):
        K.projection(tmp_path / "2011_09_30")
    (tmp_path / "bad").mkdir()
    (tmp_path / "bad" / "calib_cam_to_cam.txt").write_text("S_rect_02: 1242 375\n")
    (tmp_path / "bad" / "calib_velo_to_cam.txt").write_text("R: 1 0 0 0 1 0 0 0 1\nT: 0 0 0\n")
    with pytest.raises(GdnError, match="R_rect_00"):
        K.projection(tmp_path / "bad")


def test_parse_velo_list_formats_and_missing_files(tmp_path):
    from gdn_amd import kitti_raw as K
    from gdn_amd._lib import GdnError
    raw = tmp_path / "raw"
    for date in ("2011_09_26", "2011_09_28"):
        Y.write_calib(raw / date)
    pts = np.arange(12, dtype=np.float32).reshape(3, 4)
    a = Y.write_scan(raw, "2011_09_26", "2011_09_26_drive_0002_sync", 69, pts)
    b = Y.write_scan(raw, "2011_09_28", "2011_09_28_drive_0001_sync", 5, pts)
    lst = tmp_path / "list.txt"
    lst.write_text("2011_09_26/2011_09_26_drive_0002_sync/image_02/data/0000000069.png some other tokens\n"
                   "\n"
                   "2011_09_28/2011_09_28_drive_0001_sync/image_03/data/0000000005.jpg\n"
                   "2011_09_26/2011_09_26_drive_0002_sync 69 l\n"
                   "2011_09_28/2011_09_28_drive_0001_sync 0000000005 r\n")
    got = K.parse_velo_list(lst, raw)
    assert got == [(a, raw / "2011_09_26", 2), (b, raw / "2011_09_28", 3), (a, raw / "2011_09_26", 2), (b, raw / "2011_09_28", 3)]
    lst.write_text("2011_09_26/2011_09_26_drive_0002_sync 69 l\n2011_09_26/2011_09_26_drive_0002_sync 70 l\n")
    with pytest.raises(GdnError, match=r"0000000070\.bin.*line 2"):
        K.parse_velo_list(lst, raw)
    (raw / "2011_09_28" / "calib_velo_to_cam.txt").unlink()
    lst.write_text("2011_09_28/2011_09_28_drive_0001_sync 5 r\n")
    with pytest.raises(GdnError, match=r"calib_velo_to_cam\.txt.*line 1"):
        K.parse_velo_list(lst, raw)
    lst.write_text("2011_09_26/2011_09_26_drive_0002_sync 69 x\n")
    with pytest.raises(GdnError, match="line 1"):
        K.parse_velo_list(lst, raw)


def test_eigen_velodyne_and_assemble_scans_on_the_host(tmp_path):
    from gdn_amd._lib import GdnError
    from gdn_amd.datasets import EigenVelodyne, assemble_scans
    raw = tmp_path / "raw"
    cam_a, velo_a = Y.write_calib(raw / "2011_09_26", seed=1)
    cam_b, velo_b = Y.write_calib(raw / "2011_09_28", seed=2, w0=1224, h0=370)
    r = np.random.RandomState(0)
    clouds = [r.uniform(-40, 40, (n, 4)).astype(np.float32) for n in (7, 0, 12)]
    Y.write_scan(raw, "2011_09_26", "d1", 0, clouds[0])
    Y.write_scan(raw, "2011_09_28", "d2", 3, clouds[1])
    Y.write_scan(raw, "2011_09_26", "d1", 1, clouds[2])
    lst = tmp_path / "v.txt"
    lst.write_text("2011_09_26/d1 0 l\n2011_09_28/d2 3 r\n2011_09_26/d1 1 l\n")
    ds = EigenVelodyne(str(lst), str(raw))
    assert len(ds) == 3 and ds.depth == "camera"
    samples = [ds[i] for i in range(3)]
    for (pts, P, size), c in zip(samples, clouds):
        assert pts.dtype == np.float32 and pts.shape == c.shape and np.array_equal(pts, c)
    assert np.array_equal(samples[0][1], Y.compose(cam_a, velo_a, 2)[0]) and samples[0][2] == (375, 1242)
    assert np.array_equal(samples[1][1], Y.compose(cam_b, velo_b, 3)[0]) and samples[1][2] == (370, 1224)
    assert samples[2][1] is samples[0][1] and len(ds._calib) == 2                    # one read per date and camera
    points, offsets, proj, sizes, Hmax, Wmax, size_list = assemble_scans(samples, "cpu")
    assert points.dtype == torch.float32 and tuple(points.shape) == (19, 4)
    assert np.array_equal(points.numpy(), np.concatenate(clouds))
    assert offsets.dtype == torch.int64 and offsets.tolist() == [0, 7, 7, 19]
    assert proj.dtype == torch.float64 and tuple(proj.shape) == (3, 12)
    assert np.array_equal(proj.numpy(), np.stack([s[1].reshape(12) for s in samples]))
    assert sizes.dtype == torch.int32 and sizes.tolist() == [[375, 1242], [370, 1224], [375, 1242]]
    assert (Hmax, Wmax) == (375, 1242) and size_list == [(375, 1242), (370, 1224), (375, 1242)]
    with pytest.raises(GdnError):
        assemble_scans([], "cpu")
    with pytest.raises(GdnError):
        EigenVelodyne(str(lst), str(raw), depth="radial")
    (raw / "2011_09_26" / "d1" / "velodyne_points" / "data" / "0000000001.bin").write_bytes(b"\0" * 20)
    with pytest.raises(GdnError, match="0000000001.bin"):
        ds[2]


def test_scan_list_must_be_as_long_as_the_split():
    from gdn_amd._lib import GdnError
    from gdn_amd.trainer import validate_std
    net = torch.nn.Linear(1, 1)
    loader = types.SimpleNamespace(ds=[0, 1, 2])
    with pytest.raises(GdnError, match="--eval_velodyne names 2 scans, the test split has 3"):
        validate_std(types.SimpleNamespace(eval_protocol="standard"), loader, net, 0, None, "DtoD_test", velo=[None, None])


# ---------------------------------------------------------------------------------------------------------------------
# flags

STD = ["--eval_protocol", "standard"]


@pytest.mark.parametrize("flag, extra", [("--eval_velodyne", ["v.txt"]), ("--kitti_raw", ["raw"]), ("--velo_depth", ["forward"])])
@pytest.mark.parametrize("proto", [[], ["--eval_protocol", "reference"]])
def test_velodyne_flags_need_the_standard_protocol(flag, extra, proto):
    from gdn_amd import GDN_main, option
    argv = ["--synthetic", "--mode", "DtoD_test", "--real_test", flag, *extra, *proto]
    with pytest.raises(RuntimeError, match=re.escape(flag) + r"\b.*--eval_protocol standard"):
        GDN_main._check_eval(option.parse_args(argv))
    with pytest.raises(RuntimeError, match=re.escape(flag)):          # and run() says so before it touches the GPU
        GDN_main.main(argv)


def test_velodyne_refusals_and_what_passes(tmp_path):
    from gdn_amd import GDN_main, option
    lst, raw, gt = tmp_path / "v.txt", tmp_path / "raw", tmp_path / "gt.txt"
    lst.write_text("2011_09_26/d 0 l\n2011_09_26/d 1 l\n")
    gt.write_text("a.png\nb.png\n")
    raw.mkdir()
    test = [*STD, "--mode", "DtoD_test", "--real_test"]
    both = ["--eval_velodyne", str(lst), "--kitti_raw", str(raw)]
    check = lambda argv: GDN_main._check_eval(option.parse_args(argv))
    with pytest.raises(RuntimeError, match="--eval_velodyne.*--eval_gt_list"):
        check([*test, *both, "--eval_gt_list", str(gt)])
    with pytest.raises(RuntimeError, match="--eval_velodyne.*--kitti_raw"):
        check([*test, "--eval_velodyne", str(lst)])
    with pytest.raises(RuntimeError, match="--kitti_raw.*--eval_velodyne"):
        check([*test, "--kitti_raw", str(raw)])
    with pytest.raises(RuntimeError, match="--velo_depth.*--eval_velodyne"):
        check([*test, "--velo_depth", "camera"])
    with pytest.raises(RuntimeError, match="--eval_velodyne.*--mode DtoD"):
        check([*STD, "--mode", "DtoD", "--real_test", *both])
    with pytest.raises(RuntimeError, match="--eval_velodyne.*--real_test"):
        check([*STD, "--mode", "RtoD_test", *both])
    with pytest.raises(FileNotFoundError, match="--eval_velodyne"):
        check([*test, "--eval_velodyne", str(tmp_path / "none.txt"), "--kitti_raw", str(raw)])
    with pytest.raises(FileNotFoundError, match="--kitti_raw"):
        check([*test, "--eval_velodyne", str(lst), "--kitti_raw", str(tmp_path / "nowhere")])
    # the number of lines against the test split under the data root
    data = tmp_path / "eigen"
    data.mkdir()
    (data / "eigen_test_files_img.txt").write_text("a/img.png\nb/img.png\nc/img.png\n")
    with pytest.raises(RuntimeError, match="--eval_velodyne names 2 scans, the test split has 3 samples"):
        check([str(data), *test, *both])
    with pytest.raises(RuntimeError, match="--eval_velodyne names 2 scans"):          # run(): before the GPU check
        GDN_main.main([str(data), *test, *both])
    (data / "eigen_test_files_img.txt").write_text("a/img.png\nb/img.png\n")
    # what passes, and what it resolves to: beside eval_spec(), whose keys stay
    args = option.parse_args([str(data), *test, *both])
    check([str(data), *test, *both])
    assert option.velo_spec(args) == {"list": str(lst), "root": str(raw), "depth": "camera"}
    assert sorted(option.eval_spec(args)) == sorted(["standard", "crop", "min_depth", "max_depth", "depth_scale",
                                                     "median_scaling", "flip_test", "gt_list"])
    text = option.eval_describe(option.eval_spec(args), option.velo_spec(args))
    assert "gt Velodyne scans projected on the device (%s, camera)" % lst in text and "crop garg" in text
    fwd = option.parse_args([str(data), *test, *both, "--velo_depth", "forward"])
    check([str(data), *test, *both, "--velo_depth", "forward"])
    assert option.velo_spec(fwd)["depth"] == "forward"
    assert "(%s, forward)" % lst in option.eval_describe(option.eval_spec(fwd), option.velo_spec(fwd))
    plain = option.parse_args([])
    assert option.velo_spec(plain) is None and plain.velo_depth is None and option.velo_flags_given(plain) == []
    assert "the loader's" in option.eval_describe(option.eval_spec(plain))


# ---------------------------------------------------------------------------------------------------------------------
# ABI

def test_abi_symbol_and_bad_arguments_without_a_gpu():
    from gdn_amd import _lib as L
    header = (REPO / "include" / "gdn_hip.h").read_text()
    assert ("int gdn_velo_project(const float* points, const int64_t* offsets, const double* proj, const int32_t* sizes, "
            "int32_t B,") in header
    assert "gdn_velo_project" in L.EXPORTS and "gdn_velo_project" in L._STATUS_FUNCS
    assert len(L._SIGS["gdn_velo_project"][1]) == 12
    assert int(L.lib.gdn_version()) == L.ABI_VERSION
    f = L.lib.raw("gdn_velo_project")
    P = ctypes.c_void_p(4096)

    def call(points=P, offsets=P, proj=P, sizes=P, B=3, n=100, Hm=16, Wm=24, kind=0, depth=P, hits=P):
        return f(points, offsets, proj, sizes, B, n, Hm, Wm, kind, depth, hits, None)
    for bad in (dict(B=0), dict(B=-1), dict(B=65536), dict(Hm=0), dict(Wm=0), dict(Hm=65536, Wm=32768), dict(kind=2),
                dict(kind=-1), dict(n=-1), dict(points=None), dict(offsets=None), dict(proj=None), dict(sizes=None),
                dict(depth=None), dict(points=ctypes.c_void_p(4100)), dict(depth=ctypes.c_void_p(4104))):
        assert call(**bad) == -1, bad                     # GDN_ERR_BAD_ARG, before any launch
    with pytest.raises(L.GdnError, match="gdn_velo_project failed"):
        L.lib.gdn_velo_project(P, P, P, P, 0, 100, 16, 24, 0, P, None, None)
