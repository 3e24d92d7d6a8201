"""GPU tests of the Velodyne ground truth (--eval_velodyne): gdn_velo_project through gdn_amd.ops against the
float64 numpy restatement (velo_numpy.py, pinned without a GPU by test_velo_cpu.py), its capture in a graph, and the command
line end to end.

Bars: every pool BITWISE (padding and empty images +0), hits exact, two calls the same bytes.  End to end the nine metrics
against eval_std_numpy.py fed with restatement-projected maps: rtol 1e-10 in process (the bar of test_hip_eval_std.py's
validate_std check), and the printed 4 decimals at that file's bar for printed values."""
import os
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_std_numpy as S
import velo_numpy as V
import velo_synth as Y

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parent.parent
TIES = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]], np.float64)          # u = y / x, v = z / x, depth x


def _args(gpu, clouds, Ps, sizes):
    from gdn_amd.datasets import assemble_scans
    samples = [(np.ascontiguousarray(c, np.float32).reshape(-1, 4), np.asarray(P, np.float64).reshape(3, 4), s)
               for c, P, s in zip(clouds, Ps, sizes)]
    return assemble_scans(samples, gpu)[:4]


def _project(gpu, clouds, Ps, sizes, Hmax, Wmax, kind, **kw):
    from gdn_amd import ops
    pool, hits = ops.velo_project(*_args(gpu, clouds, Ps, sizes), Hmax, Wmax, depth=("camera", "forward")[kind], hits=True, **kw)
    return pool.cpu().numpy(), hits.cpu().numpy()


def _check(gpu, clouds, Ps, sizes, Hmax, Wmax, kind, what):
    want, want_hits = V.restate_batch(clouds, Ps, sizes, Hmax, Wmax, kind)
    got, hits = _project(gpu, clouds, Ps, sizes, Hmax, Wmax, kind)
    again, hits2 = _project(gpu, clouds, Ps, sizes, Hmax, Wmax, kind)
    differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(what, "kind", kind, "cells differing", differ, "hits", hits.tolist(), "want", want_hits.tolist())
    assert got.dtype == np.float32 and got.shape == want.shape == (len(clouds), Hmax, Wmax)
    assert differ == 0, (what, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:8])
    assert hits.dtype == np.int32 and np.array_equal(hits, want_hits)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)) and np.array_equal(hits, hits2)
    return got, hits


_RAGGED = {}


def _ragged():
    if not _RAGGED:
        cam, velo = Y.calib_arrays(seed=4)
        sizes = [(6, 9), (13, 21), (5, 5)]
        Ps = [Y.compose(cam, velo, 2, size=s)[0] for s in sizes]
        clouds = [Y.seeded_cloud(Ps[0], sizes[0], 1819, 1), Y.seeded_cloud(Ps[1], sizes[1], 2728, 2),      # + 10 % behind
                  np.zeros((0, 4), np.float32)]
        _RAGGED.update(sizes=sizes, Ps=Ps, clouds=clouds)
    return _RAGGED


@pytest.mark.parametrize("kind", [0, 1])
def test_ragged_batch(gpu, kind):
    d = _ragged()
    assert [len(c) for c in d["clouds"]] == [2000, 3000, 0]
    got, hits = _check(gpu, d["clouds"], d["Ps"], d["sizes"], 16, 24, kind, "ragged")
    assert hits[0] > 40 and hits[1] > 200 and hits[2] == 0
    for b, (h, w) in enumerate(d["sizes"]):
        pad = got[b].copy()
        pad[:h, :w] = 0
        assert not pad.view(np.uint32).any()                           # +0 bits, not -0
    assert not got[2].view(np.uint32).any()


def test_rounding_ties_and_borders(gpu):
    h0, w0 = 4, 6
    rows = [  # x, y, z -> y / x, z / x
        (2, 5, 4),        # 2.5 -> 2, u = 1; v = 2 - 1 = 1
        (2, 7, 4),        # 3.5 -> 4, u = 3
        (2, 1, 4),        # 0.5 -> 0, u = -1: dropped
        (4, 6, 12),       # 1.5 -> 2, u = 1; v = 3 - 1 = 2
        (2, 4, 1),        # v: 0.5 -> 0, -1: dropped
        (2, 4, 3),        # v: 1.5 -> 2, v = 1; u = 1: the pixel of the first point, same depth
        (4, 8, 10),       # v: 2.5 -> 2, v = 1; u = 1: again that pixel, farther
        (5, 1, 5),        # u = rint(0.2) - 1 = -1: left of the image
        (5, 5, 5),        # u = 0, v = 0: the first column and row
        (5, 30, 20),      # u = w0 - 1 = 5, v = h0 - 1 = 3: the last column and row
        (5, 35, 5),       # u = w0: right of the image
        (5, 5, 1),        # v = -1: above
        (5, 5, 25),       # v = h0: below
    ]
    pts = np.array([(x, y, z, 0.5) for x, y, z in rows], np.float32)
    want = np.zeros((h0, w0), np.float32)
    want[1, 1], want[1, 3], want[2, 1], want[0, 0], want[3, 5] = 2, 2, 4, 5, 5
    ref, n = V.restate(pts, TIES, (h0, w0))
    assert np.array_equal(ref, want) and n == 5                        # the restatement agrees with the hand computation
    got, hits = _check(gpu, [pts], [TIES], [(h0, w0)], h0, w0, 0, "ties")
    assert np.array_equal(got[0], want) and hits.tolist() == [5]


def test_degenerate_points(gpu):
    Pa = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 1]], np.float64)        # r_2 = x + 1
    Pb = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, -1]], np.float64)       # r_2 = x - 1
    nan, inf = np.float32("nan"), np.float32("inf")
    a = np.array([(-0.0, 2, 1, 0),        # kept: r_2 = 1, pixel (0, 1), camera depth 1, forward depth -0 -> reads 0
                  (-0.5, 1.5, 0.5, 0),    # dropped although it projects to (0, 2) at depth 0.5
                  (1, 8, 4, 0),           # (1, 3) at depth 2
                  (nan, 8, 4, 0), (1, nan, 4, 0), (1, 8, nan, 0), (inf, 8, 4, 0), (1, inf, 4, 0), (1, 8, -inf, 0),
                  (3e38, 3e38, 3e38, 0)], np.float32)
    b = np.array([(1, 2, 2, 0),           # r_2 = 0: dropped
                  (0.5, -1, -1, 0),       # r_2 = -0.5, pixel (1, 1): the nearest point there, behind the camera
                  (3, 4, 4, 0),           # r_2 = 2, pixel (1, 1), in front
                  (5, 8, 8, 0),           # r_2 = 4, pixel (1, 1), farther
                  (3, 8, 4, 0)], np.float32)   # pixel (1, 3) at depth 2
    for kind in (0, 1):
        got, hits = _check(gpu, [a, b], [Pa, Pb], [(4, 6), (4, 6)], 4, 6, kind, "degenerate")
        if kind == 0:
            assert got[0, 0, 1] == 1.0 and got[0, 0, 2] == 0 and got[0, 1, 3] == 2.0
            assert got[1, 1, 1] == 0 and got[1, 1, 3] == 2.0 and hits.tolist() == [3, 1]     # (3e38 lands on (0, 0))
        else:
            assert got[0, 0, 1] == 0 and got[0, 1, 3] == 1.0 and got[1, 1, 1] == 0.5 and got[1, 1, 3] == 3.0
            assert hits.tolist() == [2, 2]


def test_contention(gpu):
    cam, velo = Y.calib_arrays(seed=5)
    P, size = Y.compose(cam, velo, 2, size=(4, 4))
    crowd = Y.seeded_cloud(P, size, 70000, 7, behind=0.0)
    assert len(crowd) == 70000                                         # 35 workgroups of 2048 points on 16 cells
    few = Y.cloud_at(P, [1, 2], [3, 0], [90.0, 95.0], np.random.RandomState(1))
    for kind in (0, 1):
        got, hits = _check(gpu, [crowd, few], [P, P], [size, size], 4, 4, kind, "contention")
        assert hits.tolist() == [16, 2] and (got[0] < 6.0).all()       # every cell holds one of the nearest of ~3000 points
        assert (got[1] > 80).sum() == 2                                # the second image saw none of the first's points
        back, _ = _project(gpu, [few, crowd], [P, P], [size, size], 4, 4, kind)
        assert np.array_equal(back[::-1].view(np.uint32), got.view(np.uint32))


def test_unaligned_offsets_and_finalise_tail(gpu):
    cam, velo = Y.calib_arrays(seed=6)
    sizes = [(5, 7), (4, 7), (5, 6)]
    Ps = [Y.compose(cam, velo, 3, size=s)[0] for s in sizes]
    clouds = [Y.cloud_at(Ps[0], [1, 3, 6], [0, 2, 4], [10.0, 20.0, 30.0], np.random.RandomState(1)),
              Y.seeded_cloud(Ps[1], sizes[1], 401, 2),
              Y.seeded_cloud(Ps[2], sizes[2], 250, 3)]
    assert len(clouds[0]) % 2 == 1 and (5 * 7) % 4 != 0                # image 1 starts at an odd point, images at odd cells
    for kind in (0, 1):
        _check(gpu, clouds, Ps, sizes, 5, 7, kind, "unaligned")
    # a pool whose images span several finalise workgroups, cut inside 16-byte quads
    big = [(67, 123), (66, 123), (67, 120)]
    Pb = [Y.compose(cam, velo, 2, size=s)[0] for s in big]
    cb = [Y.seeded_cloud(Pb[i], big[i], 6001 + 2 * i, 10 + i) for i in range(3)]
    assert (67 * 123) % 4 != 0 and 67 * 123 > 4096
    _check(gpu, cb, Pb, big, 67, 123, 0, "unaligned, several chunks")


def test_bad_arguments_and_no_hits(gpu):
    from gdn_amd import ops
    from gdn_amd._lib import GdnError, lib
    d = _ragged()
    points, offsets, proj, sizes = _args(gpu, d["clouds"], d["Ps"], d["sizes"])
    pool, hits = ops.velo_project(points, offsets, proj, sizes, 16, 24, hits=True)
    alone = ops.velo_project(points, offsets, proj, sizes, 16, 24)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone.view(torch.int32), pool.view(torch.int32))
    sized = ops.velo_project(points, offsets, proj, sizes, 16, 24, max_points=64)       # a grid of one workgroup: the stride
    assert torch.equal(sized.view(torch.int32), pool.view(torch.int32))
    f = lib.raw("gdn_velo_project")
    out = torch.full((3, 16, 24), 7.0, device=gpu)
    ptr = lambda t: t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream

    def call(points=ptr(points), offsets=ptr(offsets), proj=ptr(proj), sizes=ptr(sizes), B=3, n=5000, Hm=16, Wm=24, kind=0,
             depth=ptr(out), hits=None):
        return f(points, offsets, proj, sizes, B, n, Hm, Wm, kind, depth, hits, st)
    for bad in (dict(B=0), dict(B=65536), dict(Hm=65536, Wm=32768), dict(Hm=0), dict(kind=2), dict(kind=-1), dict(n=-1),
                dict(points=None), dict(offsets=None), dict(proj=None), dict(sizes=None), dict(depth=None)):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                          # refused before anything was written
    assert call() == 0
    assert torch.equal(out.view(torch.int32), pool.view(torch.int32))
    for kw in (dict(depth="radial"), dict(Hmax=0)):
        with pytest.raises(GdnError):
            ops.velo_project(points, offsets, proj, sizes, **{"Hmax": 16, "Wmax": 24, **kw})
    for swap in (dict(points=points.double()), dict(offsets=offsets.int()), dict(proj=proj.float()), dict(sizes=sizes[:2]),
                 dict(points=points.cpu())):
        a = dict(points=points, offsets=offsets, proj=proj, sizes=sizes)
        a.update(swap)
        with pytest.raises(GdnError):
            ops.velo_project(a["points"], a["offsets"], a["proj"], a["sizes"], 16, 24)


def test_graph_replay(gpu):
    from gdn_amd import ops
    d = _ragged()
    first = _args(gpu, d["clouds"], d["Ps"], d["sizes"])
    # other points, other counts (the offsets table is device memory: a replay reads what it holds then), same total
    clouds2 = [Y.seeded_cloud(d["Ps"][0], d["sizes"][0], 910, 21)[:1000], Y.seeded_cloud(d["Ps"][1], d["sizes"][1], 2728, 22),
               Y.seeded_cloud(d["Ps"][2], d["sizes"][2], 910, 23)[:1000]]
    second = _args(gpu, clouds2, d["Ps"], d["sizes"])
    assert second[0].shape == first[0].shape
    static = [t.clone() for t in first]
    eager1 = [t.clone() for t in ops.velo_project(*first, 16, 24, hits=True)]
    eager2 = [t.clone() for t in ops.velo_project(*second, 16, 24, depth="camera", hits=True)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pool, hits = ops.velo_project(*static, 16, 24, hits=True)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pool.view(torch.int32), eager1[0].view(torch.int32)) and torch.equal(hits, eager1[1])
    for s, t in zip(static, second):
        s.copy_(t)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pool.view(torch.int32), eager2[0].view(torch.int32)) and torch.equal(hits, eager2[1])
    assert not torch.equal(eager1[0], eager2[0])
    want, want_hits = V.restate_batch(clouds2, d["Ps"], d["sizes"], 16, 24, 0)
    assert np.array_equal(pool.cpu().numpy().view(np.uint32), want.view(np.uint32)) and hits.cpu().tolist() == want_hits.tolist()


# ---------------------------------------------------------------------------------------------------------------------
# end to end through the CLI

H, W = 32, 64                                                          # the network's size
FRAMES = [("2011_09_26", "2011_09_26_drive_0002_sync", 3, "l"), ("2011_09_26", "2011_09_26_drive_0002_sync", 4, "l"),
          ("2011_09_26", "2011_09_26_drive_0009_sync", 0, "r"), ("2011_09_28", "2011_09_28_drive_0002_sync", 11, "l"),
          ("2011_09_28", "2011_09_28_drive_0002_sync", 12, "r"), ("2011_09_26", "2011_09_26_drive_0009_sync", 1, "l"),
          ("2011_09_28", "2011_09_28_drive_0002_sync", 13, "l"), ("2011_09_26", "2011_09_26_drive_0002_sync", 5, "r")]
NATIVE = {"2011_09_26": (40, 64), "2011_09_28": (38, 60)}


def _raw_tree(raw):
    """Two dates, three drives, eight frames; -> the clouds, matrices and sizes in list order, and the two list files' text."""
    calib = {date: Y.write_calib(raw / date, seed=i, w0=w, h0=h) for i, (date, (h, w)) in enumerate(NATIVE.items())}
    clouds, Ps, sizes, by_path, by_drive = [], [], [], [], []
    for i, (date, drive, frame, side) in enumerate(FRAMES):
        cam = 2 if side == "l" else 3
        P, size = Y.compose(*calib[date], cam)
        pts = Y.seeded_cloud(P, size, 1400 + 50 * i, 30 + i)
        Y.write_scan(raw, date, drive, frame, pts)
        clouds.append(pts), Ps.append(P), sizes.append(size)
        by_path.append("%s/%s/image_0%d/data/%010d.png" % (date, drive, cam, frame))
        by_drive.append("%s/%s %d %s" % (date, drive, frame, side))
    return clouds, Ps, sizes, "\n".join(by_path) + "\n", "\n".join(by_drive) + "\n"


def _eigen_split(root, n):
    from PIL import Image
    r = np.random.RandomState(9)
    yy, xx = np.mgrid[0:H, 0:W]
    lists = {"img": [], "color_gt": [], "gt": []}
    for i in range(n):
        d = root / ("sample_%02d" % i)
        d.mkdir(parents=True)
        dense = np.clip(40 + 150 * yy / H + 30 * np.sin(xx / (5.0 + i)) + r.randint(0, 20, (H, W)), 0, 255).astype(np.uint8)
        Image.fromarray(r.randint(0, 256, (H, W, 3)).astype(np.uint8)).save(d / "img.png")
        Image.fromarray(dense).save(d / "color_gt.png")
        Image.fromarray(np.where(r.rand(H, W) < 0.2, dense, 0).astype(np.uint8)).save(d / "gt.png")
        for k in lists:
            lists[k].append("%s/%s.png" % (d.name, k))
    for k, v in lists.items():
        (root / ("eigen_test_files_%s.txt" % k)).write_text("\n".join(v) + "\n")


def _run_cli(tmp_path, data, extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([str(REPO / "gdn-pytorch_amd"), str(REPO)] +
                                        ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "gdn_amd.GDN_main", str(data), "--mode", "DtoD_test",
           "--batch_size", "3", "--gpu_num", "0", "--height", str(H), "--width", str(W), "--model_dir",
           str(tmp_path / "ckpt.pkl"), "--real_test", "--eval_protocol", "standard", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=400)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Results: ")]
    assert len(line) == 1, r.stdout[-2000:]
    body, _, tail = line[0][len("Results: "):].partition(" [standard: ")
    return [(m.group(1), float(m.group(2))) for m in re.finditer(r"(\w+) (-?[0-9.]+|nan)", body)], tail, r.stdout


def _assert_printed(printed, expected):
    assert [n for n, _ in printed] == S.ERROR_NAMES_STD
    for (n, v), e in zip(printed, expected):       # printed with 4 decimals
        assert abs(v - e) <= 5.1e-5 + 1e-5 * abs(e), (n, v, e)


def test_cli_velodyne_ground_truth(gpu, tmp_path, capsys):
    import types
    import gdn_amd.AE_model_unet as M
    from gdn_amd.datasets import EigenVelodyne, GpuAugmentLoader, TestFolder
    from gdn_amd.trainer import load_checkpoint, validate_std
    data, raw = tmp_path / "eigen", tmp_path / "raw"
    _eigen_split(data, len(FRAMES))
    clouds, Ps, sizes, by_path, by_drive = _raw_tree(raw)
    (tmp_path / "by_path.txt").write_text(by_path)
    (tmp_path / "by_drive.txt").write_text(by_drive)
    torch.manual_seed(123)
    m = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
    torch.save({"module." + k: v for k, v in m.state_dict().items()}, tmp_path / "ckpt.pkl")
    load_checkpoint(m, str(tmp_path / "ckpt.pkl"))
    m = m.to(gpu).eval()
    outs, loader_gt = [], []
    for depth, _, depth_np in GpuAugmentLoader(TestFolder(str(data)), 3, gpu, train=False):
        with torch.no_grad():
            outs.append(m(depth, istrain=False).float().cpu().numpy())
        loader_gt.append(depth_np.cpu().numpy())
    outs, loader_gt = np.concatenate(outs), np.concatenate(loader_gt)
    assert len(outs) == 8
    want = {}
    for kind, name in ((0, "camera"), (1, "forward")):
        pool, hits = V.restate_batch(clouds, Ps, sizes, 40, 64, kind)
        rows = S.std_rows(pool, 0, [S.eval_box(h, w, "garg") for h, w in sizes], outs)
        means, left = S.mean_rows(rows)
        assert left == 0 and (rows[:, 0] > 100).all()
        want[name] = (means, float(hits.astype(np.float64).mean()))
    assert np.abs(want["camera"][0] - want["forward"][0]).max() > 1e-4          # the two depths are told apart
    # in process: the trainer's path at the bar of the float64 reductions
    loader = GpuAugmentLoader(TestFolder(str(data)), 3, gpu, train=False)
    velo = EigenVelodyne(str(tmp_path / "by_drive.txt"), str(raw), "forward")
    errors, left_out, names = validate_std(types.SimpleNamespace(eval_protocol="standard"), loader, m, 0, None, "DtoD_test",
                                           velo=velo)
    assert left_out == 0 and names == S.ERROR_NAMES_STD
    np.testing.assert_allclose(errors, want["forward"][0], rtol=1e-10)
    assert "=> Velodyne ground truth: %.1f LiDAR pixels per image on average (8 images)" % want["forward"][1] \
        in capsys.readouterr().out
    # the command line, one list format each
    printed, tail, stdout = _run_cli(tmp_path, data, ["--eval_velodyne", str(tmp_path / "by_path.txt"), "--kitti_raw", str(raw)])
    _assert_printed(printed, want["camera"][0])
    assert "gt Velodyne scans projected on the device (%s, camera); 0 image(s) left out]" % (tmp_path / "by_path.txt") in tail
    assert "crop garg, cap 0.001-80 m" in tail
    assert "=> Velodyne ground truth: %.1f LiDAR pixels per image on average (8 images)" % want["camera"][1] in stdout
    # without the new flags: the loader's ground truth and the line as it was
    printed, tail, stdout = _run_cli(tmp_path, data, [])
    means, left = S.mean_rows(S.std_rows(loader_gt[:, 0], 2, [S.eval_box(H, W, "garg")] * 8, outs))
    _assert_printed(printed, means)
    assert tail == ("crop garg, cap 0.001-80 m, depth_scale 80 m, median scaling off, flip off, gt the loader's, at the "
                    "network's size; %d image(s) left out]" % left)
    assert "Velodyne" not in stdout
