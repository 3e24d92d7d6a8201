"""GPU tests of the depth densification and the training-set command: gdn_depth_densify and
gdn_depth_encode_u8 through gdn_amd.ops against the numpy restatement (densify_numpy.py, pinned to scipy.ndimage without a
GPU by test_densify_cpu.py), the capture in a graph, and python -m gdn_amd.prepare_kitti end to end.

The bar is BITWISE, padding included: every step is a selection (max, min, median) or a fixed-order chain of single float32
operations without contraction.  Two calls give the same bytes."""
import io
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import torch

import densify_numpy as Z
import velo_numpy as V
import velo_synth as Y

pytestmark = pytest.mark.gpu

F = np.float32
REPO = pathlib.Path(__file__).resolve().parent.parent


def _run(gpu, pool, sizes, max_depth=100.0):
    from gdn_amd import ops
    out = ops.depth_densify(torch.from_numpy(pool).to(gpu), torch.tensor(sizes, dtype=torch.int32, device=gpu), max_depth)
    return out.cpu().numpy()


def _check(gpu, pool, sizes, what, max_depth=100.0, want=None):
    want = Z.densify_pool(pool, sizes, max_depth) if want is None else want
    got, again = _run(gpu, pool, sizes, max_depth), _run(gpu, pool, sizes, max_depth)
    diff = got.view(np.uint32) != want.view(np.uint32)
    print(what, "cells differing", int(diff.sum()), "of", diff.size, "filled", float((want > 0).mean()))
    assert got.dtype == F and got.shape == want.shape
    assert not diff.any(), (what, np.argwhere(diff)[:8], got[diff][:8], want[diff][:8])
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    return got


def _sparse(r, shape, share, lo=1.0, hi=90.0):
    return np.where(r.rand(*shape) < share, r.uniform(lo, hi, shape), 0).astype(F)


def _pool(images, Hmax, Wmax, garbage=True):
    """Images in the top-left corners; the padding holds NaN, a depth and -inf, which a kernel that read it would show."""
    pool = np.zeros((len(images), Hmax, Wmax), F)
    for b, im in enumerate(images):
        h, w = im.shape
        if garbage:
            pool[b, h:, :] = np.nan
            pool[b, :h, w:] = 7.5
            pool[b, :h:2, w:] = -np.inf
        pool[b, :h, :w] = im
    return pool, [im.shape for im in images]


def test_ragged_batch(gpu):
    r = np.random.RandomState(1)
    images = [_sparse(r, (6, 9), 0.3), _sparse(r, (37, 53), 0.05), _sparse(r, (13, 21), 0.3), _sparse(r, (1, 1), 1.0)]
    pool, sizes = _pool(images, 40, 64)
    got = _check(gpu, pool, sizes, "ragged")
    clean, _ = _pool(images, 40, 64, garbage=False)
    assert np.array_equal(got.view(np.uint32), _run(gpu, clean, sizes).view(np.uint32))       # the padding was never read
    for b, (h, w) in enumerate(sizes):
        pad = got[b].copy()
        pad[:h, :w] = 0
        assert not pad.view(np.uint32).any()                           # +0 bits
        assert (got[b, :h, :w] > 0).any()


def test_edge_images(gpu):
    r = np.random.RandomState(2)
    h, w = 37, 70                                                      # two tiles each way
    empty = np.zeros((h, w), F)
    corners = empty.copy()
    corners[0, 0], corners[0, -1], corners[-1, 0], corners[-1, -1] = 10.0, 20.0, 30.0, 40.0
    column = _sparse(r, (h, w), 0.9)
    column[:, 33:35] = 0                                               # columns without returns next to full ones
    column[:, 0] = 0
    column[:, -1] = 0
    plateau = np.where(r.rand(h, w) < 0.5, F(25.0), F(0)).astype(F)    # equal values: median ties
    plateau[20:30, 10:40] = F(12.5)
    straddle = r.uniform(99.85, 99.95, (h, w)).astype(F)               # inverted values around 0.1f
    straddle[::3, ::4] = F(100) - F(0.1)
    straddle[1::3, ::4] = np.nextafter(F(100) - F(0.1), F(0))
    straddle[5, 5], straddle[30, 60] = 50.0, 0.1
    odd = _sparse(r, (h, w), 0.2)
    odd[r.rand(h, w) < 0.05] = np.nan
    odd[r.rand(h, w) < 0.05] = np.inf
    odd[r.rand(h, w) < 0.05] = -np.inf
    odd[r.rand(h, w) < 0.05] = -4.0
    odd[r.rand(h, w) < 0.02] = 3e38
    pool, sizes = _pool([empty, corners, column, plateau, straddle, odd], 40, 72)
    got = _check(gpu, pool, sizes, "edges")
    assert not got[0].view(np.uint32).any() and (got[1, :h, :w] > 0).sum() > 100 and np.isfinite(got).all()
    one_far = np.full((5, 5), 99.9, F)
    assert not _check(gpu, *_pool([one_far], 5, 5), "99.9 m").view(np.uint32).any()
    _check(gpu, *_pool([_sparse(r, (9, 11), 0.3, hi=40.0)], 12, 12), "max_depth 50", max_depth=50.0)


_BIG = {}


def _big(shape, share):
    if shape not in _BIG:
        images = [Z.lidar_like(*shape, share, seed=s) for s in (11, 12)]
        pool, sizes = _pool(images, *shape)
        _BIG[shape] = (pool, sizes, Z.densify_pool(pool, sizes))
    return _BIG[shape]


@pytest.mark.parametrize("shape, share", [((128, 416), 0.3), ((375, 1242), 0.06)])
def test_lidar_like_pools(gpu, shape, share):
    pool, sizes, want = _big(shape, share)
    got = _check(gpu, pool, sizes, "lidar %dx%d" % shape, want=want)
    assert (got > 0).all()


def test_encoder(gpu):
    from gdn_amd import ops
    r = np.random.RandomState(3)
    k = np.arange(255, dtype=np.float64)
    for scale, ties in ((80.0, (k + 0.5) * 80.0 / 255.0), (255.0, k + 0.5), (20.0, (k + 0.5) * 20.0 / 255.0)):
        x = np.concatenate([ties, [np.nan, -np.inf, np.inf, -0.0, 0.0, 1e-30, 0.1, scale, np.nextafter(F(scale), F(0)), 3e38, -3e38],
                            r.uniform(-5, 1.2 * scale, 4000)]).astype(F)
        x = x[:(len(x) - 3) // 4 * 4 + 3]                              # a tail of three after the quads
        assert len(x) % 4 == 3
        with np.errstate(invalid="ignore"):
            held = (x.astype(np.float64) / scale * 255.0) % 1.0 == 0.5
        assert held.sum() >= 5, scale                                  # true ties: 8, 24, 40, 56, 72 m at scale 80
        for keep in (False, True):
            got = ops.depth_encode_u8(torch.from_numpy(x).to(gpu), scale, keep_valid=keep).cpu().numpy()
            want = Z.encode_u8(x, scale, keep)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (scale, keep, x[got != want][:8])
            if not keep:                                               # (keep_valid lifts the tie at half a byte from 0 to 1)
                assert (got[held] % 2 == 0).all()                      # half to even
    x = torch.from_numpy(np.array([[0.05, 40.0, -1.0]], F)).to(gpu)
    assert ops.depth_encode_u8(x, keep_valid=True).cpu().tolist() == [[1, 128, 0]]
    assert ops.depth_encode_u8(x).cpu().tolist() == [[0, 128, 0]]


def test_graph_replay(gpu):
    from gdn_amd import ops
    r = np.random.RandomState(4)
    first, sizes = _pool([_sparse(r, (37, 53), 0.1), _sparse(r, (13, 21), 0.3)], 40, 64)
    second, _ = _pool([_sparse(r, (37, 53), 0.2), _sparse(r, (13, 21), 0.1)], 40, 64)
    size_t = torch.tensor(sizes, dtype=torch.int32, device=gpu)
    eager = [ops.depth_densify(torch.from_numpy(p).to(gpu), size_t).clone() for p in (first, second)]
    static, out = torch.from_numpy(first).to(gpu), torch.empty((2, 40, 64), device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.depth_densify(static, size_t, out=out)
        code = ops.depth_encode_u8(out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager[0].view(torch.int32))
    static.copy_(torch.from_numpy(second))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager[1].view(torch.int32)) and not torch.equal(eager[0], eager[1])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), Z.densify_pool(second, sizes).view(np.uint32))
    assert np.array_equal(code.cpu().numpy(), Z.encode_u8(out.cpu().numpy()))


def test_bad_arguments(gpu):
    from gdn_amd import ops
    from gdn_amd._lib import GdnError, lib
    r = np.random.RandomState(5)
    pool_np, sizes_l = _pool([_sparse(r, (13, 21), 0.3), _sparse(r, (6, 9), 0.3)], 16, 24)
    pool, sizes = torch.from_numpy(pool_np).to(gpu), torch.tensor(sizes_l, dtype=torch.int32, device=gpu)
    want = ops.depth_densify(pool, sizes)
    f = lib.raw("gdn_depth_densify")
    nb = int(lib.gdn_depth_densify_workspace_bytes(2, 16, 24))
    assert nb == pool.numel() * 4
    out, ws = torch.full((2, 16, 24), 7.0, device=gpu), torch.full((nb // 4 + 8,), 7.0, device=gpu)
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()

    def call(depth=ptr(pool), sizes=ptr(sizes), B=2, Hm=16, Wm=24, md=100.0, out=ptr(out), ws=ptr(ws), nb=nb):
        return f(depth, sizes, B, Hm, Wm, md, out, ws, nb, st)
    for bad in (dict(B=0), dict(B=65536), dict(Hm=0), dict(Wm=0), dict(Hm=65536, Wm=32768), dict(depth=None), dict(sizes=None),
                dict(out=None), dict(ws=None), dict(depth=ptr(pool) + 4), dict(out=ptr(out) + 4), dict(ws=ptr(ws) + 4),
                dict(sizes=ptr(sizes) + 2), dict(depth=ptr(out)), dict(depth=ptr(out) + 16), dict(ws=ptr(out)),
                dict(ws=ptr(pool)), dict(nb=nb - 1), dict(md=0.2), dict(md=-1.0), dict(md=float("inf")), dict(md=float("nan"))):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (ws == 7.0).all()                    # refused before anything was written
    assert call() == 0
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    g = lib.raw("gdn_depth_encode_u8")
    code = torch.full((pool.numel(),), 9, dtype=torch.uint8, device=gpu)
    for bad in (dict(n=0), dict(scale=0.0), dict(scale=float("nan")), dict(keep=2), dict(x=None), dict(o=None),
                dict(x=ptr(out) + 4), dict(o=ptr(code) + 1)):
        a = dict(x=ptr(out), n=pool.numel(), scale=80.0, keep=0, o=ptr(code))
        a.update(bad)
        assert g(a["x"], a["n"], a["scale"], a["keep"], a["o"], st) == -1, bad
    torch.cuda.synchronize()
    assert (code == 9).all()
    for kw in (dict(pool=pool.double()), dict(pool=pool.cpu()), dict(pool=pool[0]), dict(sizes=sizes.long()), dict(sizes=sizes[:1]),
               dict(max_depth=0.2), dict(max_depth=float("nan")), dict(out=pool), dict(out=out[:1]), dict(out=out.double())):
        a = dict(pool=pool, sizes=sizes, max_depth=100.0, out=None)
        a.update(kw)
        with pytest.raises(GdnError):
            ops.depth_densify(a["pool"], a["sizes"], a["max_depth"], out=a["out"])
    for kw in (dict(x=pool.double()), dict(x=pool.cpu()), dict(scale=0.0), dict(scale=float("inf"))):
        a = dict(x=pool, scale=80.0)
        a.update(kw)
        with pytest.raises(GdnError):
            ops.depth_encode_u8(a["x"], a["scale"])


# ---------------------------------------------------------------------------------------------------------------------
# end to end: raw tree -> the command -> the loaders -> two training steps

H, W = 32, 64                                                          # the smallest size an end-to-end test trains at
DATE = "2011_09_26"
DRIVES = ("2011_09_26_drive_0002_sync", "2011_09_26_drive_0009_sync")
NATIVE = (40, 80)


def _raw_tree(raw):
    from PIL import Image
    cam, velo = Y.write_calib(raw / DATE, seed=2, w0=NATIVE[1], h0=NATIVE[0])
    P = Y.compose(cam, velo, 2, size=(H, W))[0]
    r = np.random.RandomState(6)
    frames = {}
    for d, drive in enumerate(DRIVES):
        for k in range(3):
            pts = Y.seeded_cloud(P, (H, W), 500, 40 + 3 * d + k)
            Y.write_scan(raw, DATE, drive, k, pts)
            rgb = r.randint(0, 256, (NATIVE[0], NATIVE[1], 3)).astype(np.uint8)
            folder = raw / DATE / drive / "image_02" / "data"
            folder.mkdir(parents=True, exist_ok=True)
            Image.fromarray(rgb).save(folder / ("%010d.png" % k))
            frames[(drive, k)] = (pts, rgb)
    return P, frames


def test_prepare_kitti_end_to_end(gpu, tmp_path, capsys):
    from PIL import Image
    from gdn_amd import prepare_kitti as Pk
    from gdn_amd.datasets import SequenceFolder, TestFolder
    import types
    raw, out = tmp_path / "raw", tmp_path / "set"
    P, frames = _raw_tree(raw)
    (tmp_path / "train.txt").write_text("".join("%s/%s %d l\n" % (DATE, DRIVES[0], k) for k in (0, 1, 2, 1)))   # one twice
    (tmp_path / "val.txt").write_text("".join("%s/%s/image_02/data/%010d.png\n" % (DATE, DRIVES[1], k) for k in range(3)))
    (tmp_path / "test.txt").write_text("%s/%s 2 l\n%s/%s 0 l\n" % (DATE, DRIVES[1], DATE, DRIVES[0]))
    assert Pk.main([str(raw), str(out), "--train_list", str(tmp_path / "train.txt"), "--val_list", str(tmp_path / "val.txt"),
                    "--test_list", str(tmp_path / "test.txt"), "--height", str(H), "--width", str(W), "--batch", "2"]) == 0
    said = capsys.readouterr().out
    assert "=> prepare_kitti: 8 samples (train 3, val 3, test 2) at 32 x 64" in said and "sparse" in said and "dense" in said
    scenes = ["%s_%s_02" % (DATE, d) for d in DRIVES]
    assert (out / "train.txt").read_text() == scenes[0] + "\n" and (out / "val.txt").read_text() == scenes[1] + "\n"

    def expect(drive, k):
        pts, rgb = frames[(drive, k)]
        sparse, _ = V.restate(pts, P, (H, W), 0)
        return (Z.encode_u8(sparse, 80.0, True), Z.encode_u8(Z.densify(sparse), 80.0),
                np.asarray(Image.fromarray(rgb).resize((W, H), Image.BILINEAR)))
    for scene, drive in zip(scenes, DRIVES):
        for k in range(3):
            sp, de, rgb = expect(drive, k)
            assert (sp > 0).sum() > 100 and (de > 0).mean() > 0.9
            assert np.array_equal(np.asarray(Image.open(out / scene / "gt" / ("%010d.png" % k))), sp), (scene, k)
            assert np.array_equal(np.asarray(Image.open(out / scene / "color_gt2" / ("%010d.png" % k))), de), (scene, k)
            # the colour frame: the Pillow BILINEAR resize, as a JPEG of quality 95 (the decoder is deterministic)
            again = io.BytesIO()
            Image.fromarray(rgb).save(again, format="JPEG", quality=95)
            jpg = np.asarray(Image.open(out / scene / ("%010d.jpg" % k)))
            assert jpg.shape == (H, W, 3) and np.array_equal(jpg, np.asarray(Image.open(again))), (scene, k)
            assert (out / scene / ("%010d.jpg" % k)).read_bytes() == again.getvalue()
    names = [(DRIVES[1], 2), (DRIVES[0], 0)]
    for kind, suffix in (("img", ""), ("color_gt", "_color_gt"), ("gt", "_gt")):
        lines = (out / ("eigen_test_files_%s.txt" % kind)).read_text().split()
        assert lines == ["eigen_test/%s_%s_02_%010d%s.png" % (DATE, d, k, suffix) for d, k in names]
    for i, (drive, k) in enumerate(names):
        sp, de, rgb = expect(drive, k)
        base = "%s_%s_02_%010d" % (DATE, drive, k)
        assert np.array_equal(np.asarray(Image.open(out / "eigen_test" / (base + "_gt.png"))), sp)
        assert np.array_equal(np.asarray(Image.open(out / "eigen_test" / (base + "_color_gt.png"))), de)
        assert np.array_equal(np.asarray(Image.open(out / "eigen_test" / (base + ".png"))), rgb)
    # the loaders read the tree
    args = types.SimpleNamespace(img_test=False)
    train, val, test = (SequenceFolder(out, args, seed=0, train=True), SequenceFolder(out, args, seed=0, train=False),
                        TestFolder(out))
    assert (len(train), len(val), len(test)) == (3, 3, 2)
    gt, rgb, sparse = train[0]
    assert gt.shape == sparse.shape == (H, W, 1) and rgb.shape == (H, W, 3) and gt.dtype == np.uint8
    stem = train.samples[0]["rgb"].stem
    assert train.samples[0]["gt"].stem == stem == train.samples[0]["gt_np"].stem
    gt, rgb, sparse = test[1]
    assert np.array_equal(sparse[:, :, 0], expect(DRIVES[0], 0)[0]) and np.array_equal(gt[:, :, 0], expect(DRIVES[0], 0)[1])
    # a second run is refused, --overwrite is not
    assert Pk.main([str(raw), str(out), "--train_list", str(tmp_path / "train.txt"), "--height", str(H), "--width", str(W)]) == 2
    err = capsys.readouterr().err
    assert "already holds a train.txt" in err and "Traceback" not in err and len(err.strip().splitlines()) == 1
    # two training steps on it, in a fresh process
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([str(REPO / "gdn-pytorch_amd"), str(REPO)] +
                                        ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "gdn_amd.GDN_main", str(out), "--mode", "DtoD", "--height", str(H),
           "--width", str(W), "--batch_size", "2", "--epochs", "1", "--epoch_size", "2", "--gpu_num", "0"]
    run = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=400)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
