"""CPU: the depth densification and the training-set command without a GPU -- the numpy restatement
(densify_numpy.py) against scipy.ndimage stage by stage, the predicate and encoder edge cases, what the chain fills, the
extended list reader, every refusal of gdn_amd.prepare_kitti, the output naming, the entry points' argument checks."""
import ctypes
import pathlib
import types

import numpy as np
import pytest

import densify_numpy as Z
import velo_synth as Y

F = np.float32
REPO = pathlib.Path(__file__).resolve().parent.parent


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, stage by stage, against scipy.ndimage

@pytest.mark.parametrize("shape, share, seed", [((37, 53), 0.3, 1), ((6, 9), 0.5, 2), ((1, 1), 1.0, 3), ((3, 2), 0.5, 4),
                                                ((64, 96), 0.06, 5)])
def test_restatement_equals_scipy_stage_by_stage(shape, share, seed):
    ndi = pytest.importorskip("scipy.ndimage")
    r = np.random.RandomState(seed)
    D = np.where(r.rand(*shape) < share, r.uniform(1.0, 90.0, shape), 0).astype(F)
    s = Z.stages(D)
    v1 = s[0]
    assert np.array_equal(_bits(v1), _bits(np.where(D > F(0.1), F(100) - D, F(0))))
    assert np.array_equal(_bits(s[1]), _bits(ndi.grey_dilation(v1, footprint=Z.DIAMOND, mode="constant", cval=0.0)))
    box = np.ones((5, 5), bool)
    dil = ndi.grey_dilation(s[1], footprint=box, mode="constant", cval=0.0)
    assert np.array_equal(_bits(s[2]), _bits(ndi.grey_erosion(dil, footprint=box, mode="constant", cval=np.inf)))
    for k, size in ((3, 7), (5, 31)):
        d = ndi.grey_dilation(s[k - 1], footprint=np.ones((size, size), bool), mode="constant", cval=0.0)
        assert np.array_equal(_bits(s[k]), _bits(np.where(s[k - 1] > F(0.1), s[k - 1], d)))
    # step 5, column by column in plain Python
    want = s[3].copy()
    for x in range(shape[1]):
        rows = [y for y in range(shape[0]) if want[y, x] > F(0.1)]
        if rows:
            want[:rows[0], x] = want[rows[0], x]
    assert np.array_equal(_bits(s[4]), _bits(want))
    med = ndi.median_filter(s[5], size=5, mode="nearest")
    assert np.array_equal(_bits(s[6]), _bits(np.where(s[5] > F(0.1), med, s[5])))
    # step 8 against an explicit np.pad(mode='reflect'), one pass at a time
    v = s[6]

    def one_pass(a, axis):
        pad = [(0, 0), (0, 0)]
        pad[axis] = (2, 2)
        p = np.pad(a, pad, mode="reflect")
        n = a.shape[axis]
        t = [np.take(p, np.arange(k, k + n), axis=axis) for k in range(5)]
        return ((((t[0] + F(4) * t[1]) + F(6) * t[2]) + F(4) * t[3]) + t[4]) * F(0.0625)
    blurred = one_pass(one_pass(v, 1), 0)
    assert blurred.dtype == F
    assert np.array_equal(_bits(s[7]), _bits(np.where(v > F(0.1), blurred, v)))
    assert np.array_equal(_bits(s[8]), _bits(np.where(s[7] > F(0.1), F(100) - s[7], F(0))))


def test_reflect101_is_numpy_reflect():
    for n in (1, 2, 3, 4, 7):
        want = np.pad(np.arange(n), 2, mode="reflect")
        assert np.array_equal(Z.reflect101(np.arange(-2, n + 2), n), want), n


def test_predicate_cases():
    nan, inf = F("nan"), F("inf")
    for d in (F(99.9), nan, inf, -inf, F(-3.0), F(0.0), F(0.1), F(100.0), F(250.0)):
        out = Z.densify(np.full((1, 1), d, F))
        assert out.view(np.uint32)[0, 0] == 0, d                    # +0
    # exactly 0.1f is no return; the next float up is one, and it survives the whole chain on a 1 x 1 image
    up = np.nextafter(F(0.1), F(1))
    assert Z.invert(np.array([[F(0.1)]], F), 100.0)[0, 0] == 0 and Z.invert(np.array([[up]], F), 100.0)[0, 0] == F(100) - up
    assert abs(float(Z.densify(np.array([[up]], F))[0, 0]) - float(up)) < 1e-4
    # a return whose inverted value is exactly 0.1f is empty; one float nearer is kept
    edge = F(100) - F(0.1)
    assert F(100) - edge <= F(0.1) and Z.invert(np.array([[edge]], F), 100.0)[0, 0] == 0
    near = F(99.5)
    assert Z.invert(np.array([[near]], F), 100.0)[0, 0] == F(0.5)
    one = np.zeros((5, 5), F)
    one[2, 2] = nan
    assert not Z.densify(one).view(np.uint32).any()


def test_what_the_chain_fills():
    for shape in ((1, 1), (3, 2), (13, 21)):
        D = np.zeros(shape, F)
        D[-1, shape[1] // 2] = 20.0
        assert (Z.densify(D) > 0).all(), shape
    D = np.zeros((37, 53), F)
    D[36, 26] = 20.0                                                 # steps 2-4 reach 5 columns, step 6 another 15: 41 of 53
    filled = Z.densify(D) > 0
    assert filled[:, 6:47].all() and not filled[:, :6].any() and not filled[:, 47:].any()
    for shape, frac in (((128, 416), 0.3), ((375, 1242), 0.06)):
        out = Z.densify(Z.lidar_like(*shape, frac, seed=7))
        assert (out > 0).all() and out.max() < 100.0 and out.dtype == F
    assert not Z.densify(np.zeros((9, 9), F)).view(np.uint32).any()


def test_pool_padding_is_not_read():
    r = np.random.RandomState(0)
    sizes = [(6, 9), (1, 1), (8, 12)]
    pool = np.zeros((3, 8, 12), F)
    for b, (h, w) in enumerate(sizes):
        pool[b, :h, :w] = np.where(r.rand(h, w) < 0.4, r.uniform(2, 80, (h, w)), 0)
    dirty = pool.copy()
    for b, (h, w) in enumerate(sizes):
        dirty[b, h:, :] = np.nan
        dirty[b, :, w:] = 55.0
    a, b_ = Z.densify_pool(pool, sizes), Z.densify_pool(dirty, sizes)
    assert np.array_equal(_bits(a), _bits(b_)) and not _bits(a[0, 6:]).any() and not _bits(a[0, :, 9:]).any()


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' own text as serial host code, under AddressSanitizer and UBSan (tests/diag/densify_host.cpp)

def _host_compiler():
    import os
    import shutil
    for c in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.fixture(scope="module")
def densify_host(tmp_path_factory):
    import subprocess
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("densify_host") / "densify_host"
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", str(exe), str(REPO / "tests" / "diag" / "densify_host.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_kernel_text_on_the_host_under_sanitizers(densify_host, tmp_path):
    """Every index the kernels form, on the shapes of the GPU tests: LDS images are static arrays and the pools heap blocks
    here, so AddressSanitizer reports an access outside either; the pools and the encoder's bytes equal the restatement's."""
    import subprocess
    r = np.random.RandomState(1)
    sp = lambda shape, share, hi=90.0: np.where(r.rand(*shape) < share, r.uniform(1, hi, shape), 0).astype(F)

    def pool_of(images, Hm, Wm):
        pool = np.zeros((len(images), Hm, Wm), F)
        for b, im in enumerate(images):
            h, w = im.shape
            pool[b, h:, :] = np.nan
            pool[b, :h, w:] = 7.5
            pool[b, :h, :w] = im
        return pool, [im.shape for im in images]
    h, w = 37, 70
    corners = np.zeros((h, w), F)
    corners[0, 0], corners[0, -1], corners[-1, 0], corners[-1, -1] = 10, 20, 30, 40
    plateau = np.where(r.rand(h, w) < 0.5, F(25.0), F(0)).astype(F)
    odd = sp((h, w), .2)
    odd[r.rand(h, w) < .05] = np.nan
    odd[r.rand(h, w) < .05] = -np.inf
    full = r.uniform(2, 80, (h, w)).astype(F)                        # no empty cell after step 5: the pass-through of step 6
    cases = [(*pool_of([sp((6, 9), .3), sp((37, 53), .05), sp((13, 21), .3), sp((1, 1), 1.0)], 40, 64), 100.0),
             (*pool_of([np.zeros((h, w), F), corners, plateau, odd, full], 40, 72), 100.0),
             (*pool_of([sp((3, 2), .5), sp((2, 3), .5), sp((1, 7), .5), sp((7, 1), .5), sp((2, 2), 1.0)], 7, 7), 50.0),
             (*pool_of([Z.lidar_like(128, 416, .3, 11), Z.lidar_like(100, 300, .06, 12)], 128, 416), 100.0)]
    for k, (pool, sizes, md) in enumerate(cases):
        src, dst = tmp_path / ("in%d.bin" % k), tmp_path / ("out%d.bin" % k)
        src.write_bytes(np.array(pool.shape, np.int32).tobytes() + np.array([md], F).tobytes() +
                        np.array(sizes, np.int32).tobytes() + pool.tobytes())
        run = subprocess.run([str(densify_host), str(src), str(dst)], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-3000:]
        raw, n = dst.read_bytes(), pool.size
        got = np.frombuffer(raw[:4 * n], F).reshape(pool.shape)
        want = Z.densify_pool(pool, sizes, md)
        assert np.array_equal(_bits(got), _bits(want)), (k, np.argwhere(_bits(got) != _bits(want))[:8])
        flat = want.reshape(-1)[:-1]
        assert np.array_equal(np.frombuffer(raw[4 * n:4 * n + n - 1], np.uint8), Z.encode_u8(flat, 80.0, False)), k
        assert np.array_equal(np.frombuffer(raw[4 * n + n - 1:], np.uint8), Z.encode_u8(flat, 80.0, True)), k


# ---------------------------------------------------------------------------------------------------------------------
# the encoder

def test_encoder_ties_and_edges():
    k = np.arange(0, 255, dtype=np.float64)
    ties = ((k + 0.5) * 80.0 / 255.0)
    exact = ties.astype(F).astype(np.float64) / 80.0 * 255.0 == k + 0.5          # the ties float32 can hold exactly
    assert exact.sum() >= 5
    got = Z.encode_u8(ties.astype(F))
    want_even = np.where(k % 2 == 0, k, k + 1).astype(np.uint8)
    assert np.array_equal(got[exact], want_even[exact])                          # half to even
    assert Z.encode_u8(np.array([40.0 * 255 / 255], F))[0] == 128                # 127.5 -> 128
    edge = np.array([np.nan, -1.0, -0.0, 0.0, 80.0, 80.5, 1e30, np.inf, -np.inf, 0.1, 0.15, 0.16, 79.9], F)
    assert Z.encode_u8(edge).tolist() == [0, 0, 0, 0, 255, 255, 255, 255, 0, 0, 0, 1, 255]
    assert Z.encode_u8(edge, keep_valid=True).tolist() == [0, 0, 0, 0, 255, 255, 255, 255, 0, 1, 1, 1, 255]
    assert Z.encode_u8(np.array([10.0, 20.0], F), scale=20.0).tolist() == [128, 255]   # 127.5 -> 128
    assert Z.encode_u8(edge).dtype == np.uint8


# ---------------------------------------------------------------------------------------------------------------------
# the list reader and the command

DATE, DRIVES = "2011_09_26", ("2011_09_26_drive_0002_sync", "2011_09_26_drive_0009_sync")


def _raw_tree(raw, frames=3, size=(40, 64)):
    from PIL import Image
    Y.write_calib(raw / DATE, seed=1, w0=size[1], h0=size[0])
    r = np.random.RandomState(0)
    for drive in DRIVES:
        for k in range(frames):
            Y.write_scan(raw, DATE, drive, k, r.rand(50, 4).astype(F))
            d = raw / DATE / drive / "image_02" / "data"
            d.mkdir(parents=True, exist_ok=True)
            Image.fromarray(r.randint(0, 256, (size[0], size[1], 3)).astype(np.uint8)).save(d / ("%010d.png" % k))


def test_parse_frame_list(tmp_path):
    from gdn_amd import kitti_raw as K
    from gdn_amd._lib import GdnError
    raw = tmp_path / "raw"
    _raw_tree(raw)
    lst = tmp_path / "l.txt"
    lst.write_text("%s/%s/image_02/data/0000000001.png extra\n\n%s/%s 2 l\n" % (DATE, DRIVES[0], DATE, DRIVES[1]))
    got = K.parse_frame_list(lst, raw)
    assert [(f["date"], f["drive"], f["frame"], f["cam"]) for f in got] == [(DATE, DRIVES[0], 1, 2), (DATE, DRIVES[1], 2, 2)]
    assert got[0]["image"] == raw / DATE / DRIVES[0] / "image_02" / "data" / "0000000001.png"
    assert got[1]["scan"] == raw / DATE / DRIVES[1] / "velodyne_points" / "data" / "0000000002.bin"
    assert K.parse_velo_list(lst, raw) == [(f["scan"], raw / DATE, 2) for f in got]      # the scan reader is unchanged
    lst.write_text("%s/%s 1 r\n" % (DATE, DRIVES[0]))                                # camera 3: no such frame on disk
    with pytest.raises(GdnError, match=r"image_03.*0000000001\.png not found.*line 1"):
        K.parse_frame_list(lst, raw)
    assert len(K.parse_velo_list(lst, raw)) == 1 and len(K.parse_frame_list(lst, raw, images=False)) == 1


def _args(tmp_path, **kw):
    from gdn_amd import prepare_kitti as Pk
    argv = [str(kw.pop("raw", tmp_path / "raw")), str(kw.pop("out", tmp_path / "out")), "--train_list",
            str(kw.pop("train", tmp_path / "train.txt"))]
    for k, v in kw.items():
        argv += ["--" + k] if v is True else ["--" + k, str(v)]
    return Pk.build_parser().parse_args(argv)


def test_command_refusals(tmp_path, monkeypatch):
    from gdn_amd import prepare_kitti as Pk
    from gdn_amd._lib import GdnError
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a refusal touched the GPU"))
    raw = tmp_path / "raw"
    _raw_tree(raw)
    (tmp_path / "train.txt").write_text("".join("%s/%s %d l\n" % (DATE, DRIVES[0], k) for k in range(3)))
    (tmp_path / "val.txt").write_text("%s/%s 0 l\n" % (DATE, DRIVES[1]))
    frames = Pk.plan(_args(tmp_path, val_list=tmp_path / "val.txt", height=32, width=64))
    assert [len(frames[s]) for s in ("train", "val")] == [3, 1] and "test" not in frames
    with pytest.raises(GdnError, match="not a directory"):
        Pk.plan(_args(tmp_path, raw=tmp_path / "nowhere"))
    with pytest.raises(GdnError, match="--train_list.*no such file"):
        Pk.plan(_args(tmp_path, train=tmp_path / "none.txt"))
    with pytest.raises(GdnError, match="--test_list.*no such file"):
        Pk.plan(_args(tmp_path, test_list=tmp_path / "none.txt"))
    for kw in (dict(height=0), dict(width=0), dict(width=-4)):
        with pytest.raises(GdnError, match="a size of"):
            Pk.plan(_args(tmp_path, **kw))
    for kw in (dict(batch=0), dict(depth_scale=0), dict(max_depth=0.2), dict(max_depth="inf"), dict(depth_scale="nan")):
        with pytest.raises(GdnError):
            Pk.plan(_args(tmp_path, **kw))
    bad = tmp_path / "bad.txt"
    bad.write_text("%s/%s 0 l\nnot a frame\n" % (DATE, DRIVES[0]))
    with pytest.raises(GdnError, match=r"line 2 .*neither"):
        Pk.plan(_args(tmp_path, train=bad))
    bad.write_text("%s/%s 0 l\n%s/%s 7 l\n" % (DATE, DRIVES[0], DATE, DRIVES[0]))
    with pytest.raises(GdnError, match=r"velodyne_points.*0000000007\.bin not found.*line 2"):
        Pk.plan(_args(tmp_path, train=bad))
    (raw / DATE / DRIVES[0] / "image_02" / "data" / "0000000002.png").rename(tmp_path / "moved.png")
    with pytest.raises(GdnError, match=r"image_02.*0000000002\.png not found.*line 3"):
        Pk.plan(_args(tmp_path))
    (tmp_path / "moved.png").rename(raw / DATE / DRIVES[0] / "image_02" / "data" / "0000000002.png")
    (tmp_path / "both.txt").write_text("%s/%s 1 l\n%s/%s 1 l\n" % (DATE, DRIVES[1], DATE, DRIVES[0]))
    with pytest.raises(GdnError, match="scene.*%s_%s_02 in both" % (DATE, DRIVES[0])):
        Pk.plan(_args(tmp_path, val_list=tmp_path / "both.txt"))
    (tmp_path / "out").mkdir()
    (tmp_path / "out" / "train.txt").write_text("old\n")
    with pytest.raises(GdnError, match="already holds a train.txt"):
        Pk.plan(_args(tmp_path))
    assert Pk.plan(_args(tmp_path, overwrite=True))["train"]
    # a scan that holds no whole point, or none at all, is refused by its size; a frame named twice is planned once
    scan = raw / DATE / DRIVES[1] / "velodyne_points" / "data" / "0000000002.bin"
    (tmp_path / "short.txt").write_text("%s/%s 1 l\n%s/%s 2 l\n%s/%s 1 l\n" % ((DATE, DRIVES[1]) * 3))
    assert [f["frame"] for f in Pk.plan(_args(tmp_path, train=tmp_path / "short.txt", overwrite=True))["train"]] == [1, 2]
    for content, said in ((b"\0" * 20, "holds 20 bytes"), (b"", "holds 0 bytes")):
        scan.write_bytes(content)
        with pytest.raises(GdnError, match=r"0000000002\.bin %s" % said):
            Pk.plan(_args(tmp_path, train=tmp_path / "short.txt", overwrite=True))
    # the command itself answers a refusal with one line and status 2
    import contextlib
    import io
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        rc = Pk.main([str(raw), str(tmp_path / "out"), "--train_list", str(tmp_path / "short.txt"), "--overwrite"])
    assert rc == 2 and err.getvalue().startswith("prepare_kitti: ") and len(err.getvalue().strip().splitlines()) == 1
    (raw / DATE / "calib_velo_to_cam.txt").rename(tmp_path / "calib")
    with pytest.raises(GdnError, match=r"calib_velo_to_cam\.txt not found.*line 1"):
        Pk.plan(_args(tmp_path, overwrite=True))


def test_output_naming(tmp_path):
    from gdn_amd import prepare_kitti as Pk
    f = {"date": DATE, "drive": DRIVES[0], "frame": 7, "cam": 3}
    scene = "2011_09_26_2011_09_26_drive_0002_sync_03"
    assert Pk.scene_of(f) == scene
    out = pathlib.Path("/o")
    assert Pk.output_paths(out, "train", f) == Pk.output_paths(out, "val", f) == {
        "img": out / scene / "0000000007.jpg", "gt": out / scene / "gt" / "0000000007.png",
        "color_gt": out / scene / "color_gt2" / "0000000007.png"}
    assert Pk.output_paths(out, "test", f) == {
        "img": out / "eigen_test" / (scene + "_0000000007.png"), "gt": out / "eigen_test" / (scene + "_0000000007_gt.png"),
        "color_gt": out / "eigen_test" / (scene + "_0000000007_color_gt.png")}
    a = Pk.build_parser().parse_args(["raw", "out", "--train_list", "t"])
    assert (a.height, a.width, a.velo_depth, a.depth_scale, a.max_depth, a.batch, a.overwrite) == \
        (128, 416, "camera", 80.0, 100.0, 8, False)


# ---------------------------------------------------------------------------------------------------------------------
# the entry points

def test_symbols_and_bad_arguments():
    from gdn_amd import _lib as L
    header = (REPO / "include" / "gdn_hip.h").read_text()
    for name in ("gdn_depth_densify_workspace_bytes", "gdn_depth_densify", "gdn_depth_encode_u8"):
        assert name in L._SIGS and name + "(" in header
    assert int(L.lib.gdn_version()) == L.ABI_VERSION == 223
    ws = L.lib.raw("gdn_depth_densify_workspace_bytes")
    assert ws(8, 128, 416) == 8 * 128 * 416 * 4 and ws(0, 4, 4) == 0
    f = L.lib.raw("gdn_depth_densify")
    P = lambda a: ctypes.c_void_p(a)
    big = 1 << 20

    def call(depth=P(1 * big), sizes=P(64), B=2, Hm=16, Wm=24, md=100.0, out=P(2 * big), ws=P(3 * big), nb=2 * 16 * 24 * 4):
        return f(depth, sizes, B, Hm, Wm, md, out, ws, nb, None)
    for bad in (dict(B=0), dict(B=-1), dict(B=65536), dict(Hm=0), dict(Wm=0), dict(Hm=65536, Wm=32768, nb=1 << 62),
                dict(depth=None), dict(sizes=None), dict(out=None), dict(ws=None), dict(depth=P(big + 4)), dict(out=P(2 * big + 8)),
                dict(ws=P(3 * big + 4)), dict(sizes=P(66)), dict(out=P(big)), dict(out=P(big + 16)), dict(ws=P(2 * big + 64)),
                dict(ws=P(big + 256)), dict(nb=2 * 16 * 24 * 4 - 1), dict(md=0.2), dict(md=0.0), dict(md=-5.0),
                dict(md=float("inf")), dict(md=float("nan"))):
        assert call(**bad) == -1, bad                                # GDN_ERR_BAD_ARG, before any launch
    g = L.lib.raw("gdn_depth_encode_u8")

    def enc(x=P(big), n=100, scale=80.0, keep=0, out=P(2 * big)):
        return g(x, n, scale, keep, out, None)
    for bad in (dict(x=None), dict(out=None), dict(n=0), dict(n=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")),
                dict(scale=float("nan")), dict(keep=2), dict(keep=-1), dict(x=P(big + 4)), dict(out=P(2 * big + 2))):
        assert enc(**bad) == -1, bad
    with pytest.raises(L.GdnError, match="gdn_depth_densify failed"):
        L.lib.gdn_depth_densify(P(big), P(64), 0, 16, 24, 100.0, P(2 * big), P(3 * big), 4096, None)
