"""CPU checks of the NYU training transform: the numpy restatement (tests/nyu_augment_numpy.py) against SciPy's rotate and
Pillow's resamplers, the whole per-sample chain against the same PIL / SciPy calls the reference makes, the order of the
random draws, the training-set layout, and the new C ABI entry points."""
import ctypes
import random
import re

import numpy as np
import pytest
from PIL import Image

import nyu_augment_numpy as N
from conftest import REPO

NEW_SYMBOLS = ("gdn_nyu_augment_workspace_bytes", "gdn_nyu_augment", "gdn_pil_resize_workspace_bytes",
               "gdn_pil_resize_bilinear", "gdn_spline_rotate3_workspace_bytes", "gdn_spline_rotate3")


def _stepped(r, shape, hi=4000.0):
    a = (r.rand(*shape) * hi).astype(np.float32)
    a[:, shape[1] // 3:] += np.float32(hi / 2)              # step edges, where a spline rings the most
    a[shape[0] // 2:, :] *= np.float32(0.25)
    return a


@pytest.mark.parametrize("shape", [(251, 340, 1), (251, 340, 4), (37, 53, 1)])
def test_rotation_matches_scipy(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    r = np.random.RandomState(shape[2] * 7 + shape[0])
    for angle in [0.0, 5.0, -5.0, 4.0, -4.0] + list(r.uniform(-5, 5, 4)):
        a = _stepped(r, shape)
        ref = ndi.rotate(a, angle, reshape=False, axes=(0, 1), mode="constant")
        ref = np.clip(ref, a.min(), a.max())
        got = N.rotate(a, angle)
        assert got.dtype == np.float32 and np.array_equal(got, ref), "angle %r: %d of %d differ" % (
            angle, int((got != ref).sum()), got.size)


@pytest.mark.parametrize("scale", [0.5, 0.74, 1.0, 1.003, 1.27, 1.5])
def test_f_resample_matches_pillow(scale):
    r = np.random.RandomState(int(scale * 1000))
    for h, w in [(251, 340), (61, 47)]:
        a = _stepped(r, (h, w))
        oh, ow = int(h * scale), int(w * scale * 1.01)
        ref = np.asarray(Image.frombytes("F", (w, h), a.tobytes()).resize((ow, oh), Image.BILINEAR))
        got = N.resize_f(a, oh, ow)
        assert np.array_equal(got, ref), (h, w, oh, ow)


def _imresize_u8(arr, h, w):
    from oracle.kitti_augment import bytescale
    return np.asarray(Image.fromarray(bytescale(arr)).resize((w, h), Image.BILINEAR))


def _imresize_f(arr, h, w):
    hh, ww = arr.shape
    return np.asarray(Image.frombytes("F", (ww, hh), np.ascontiguousarray(arr, np.float32).tobytes())
                      .resize((w, h), Image.BILINEAR))


def _reference_chain(depth, rgb, p, mode, H, W):
    """The reference's per-sample NYU training transform (datasets_list.py:399-430, GDN_main.py:94-125) with the
    random draws replaced by `p`, written with the Pillow / SciPy calls it makes."""
    import scipy.ndimage as ndi
    rgb_f = rgb.astype(np.float32)
    h1, w1 = int(p["img_s"] * 251.0), int(p["img_s"] * 340.0)
    gt = _imresize_f(depth, h1, w1)
    rgb_img = _imresize_u8(rgb_f, 251, 340) if mode == "DtoD" else _imresize_u8(rgb_f, h1, w1)
    gt = gt / p["scale"]
    y1, x1 = p["y1"], p["x1"]
    merged = gt[:, :, None] if mode == "DtoD" else np.concatenate([rgb_img.astype(np.float32), gt[:, :, None]], 2)
    merged = merged[y1:y1 + 251, x1:x1 + 340, :]
    mi, ma = merged.min(), merged.max()
    rot = np.clip(ndi.rotate(merged, p["angle"], reshape=False, axes=(0, 1), mode="constant"), mi, ma)
    w2, h2 = (np.array([340, 251]) * p["scale"]).astype(int)
    if mode == "DtoD":
        imgs = [rgb_img, _imresize_f(rot[:, :, 0], h2, w2)[:, :, None]]
    else:
        imgs = [_imresize_u8(rot[:, :, :3], h2, w2), _imresize_f(rot[:, :, 3], h2, w2)[:, :, None]]
    i, j = int(round((imgs[0].shape[0] - H) / 2.)), int(round((imgs[0].shape[1] - W) / 2.))
    imgs = [im[i:i + H, j:j + W, :] for im in imgs]
    if p["flip"]:
        imgs = [np.copy(np.fliplr(im)) for im in imgs]
    if mode == "RtoD":
        imgs[0] = np.clip(imgs[0] * p["mult"], 0, 255)
    out = []
    for im in imgs:
        t = np.ascontiguousarray(im.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
        out.append((t - np.float32(0.5)) / np.float32(0.5))
    return out[1], out[0]


def edge_draws(mode):
    """Draws that reach the edges of the chain: no crop draw (h1 == 251 and w1 == 340), h1 == 251 with a wider image,
    an identity second resize, a second resize that keeps only the height, both flips, the angle range's ends."""
    base = dict(mult=1.13 if mode == "RtoD" else 1.0)
    out = []
    for img_s, scale, angle, flip in [(1.0, 1.2, 3.9, 0), (1.0001, 1.0001, -3.7, 1), (1.0035, 1.0001, 2.0, 0),
                                      (1.0035, 1.0035, -1.0, 1), (1.19, 1.49, 3.99, 1), (1.1, 1.003, -3.99, 0)]:
        h1, w1 = int(img_s * 251.0), int(img_s * 340.0)
        d = dict(base, img_s=img_s, scale=scale, h1=h1, w1=w1, y1=(h1 - 251) // 2, x1=max(w1 - 341, 0), angle=angle,
                 flip=flip)
        out.append(d)
    assert any(d["h1"] == 251 and d["w1"] == 340 for d in out) and any(d["h1"] == 251 and d["w1"] > 340 for d in out)
    assert any(N.second_size(d["scale"]) == (251, 340) for d in out)
    assert any(N.second_size(d["scale"])[0] == 251 and N.second_size(d["scale"])[1] > 340 for d in out)
    return out


def synthetic_nyu(r, H0, W0):
    depth = (r.rand(H0, W0) * 9000 + 500).astype(np.float32)
    depth[:, W0 // 2:] += np.float32(3000)
    rgb = r.randint(0, 256, (H0, W0, 3)).astype(np.uint8)
    rgb[: H0 // 3] //= 3                                    # not full range: bytescale stretches it
    return depth, rgb


@pytest.mark.parametrize("mode", ["DtoD", "RtoD"])
def test_chain_matches_pil_scipy(mode):
    pytest.importorskip("scipy.ndimage")
    r = np.random.RandomState(5 if mode == "DtoD" else 6)
    depth, rgb = synthetic_nyu(r, 240, 320)
    py, npr = random.Random(1), np.random.RandomState(1)
    draws = edge_draws(mode) + [N.draw_params(mode, py, npr) for _ in range(2)]
    for k, p in enumerate(draws):
        H, W = (224, 320) if k % 2 == 0 else (96, 128)
        gd, gc = N.augment_sample(depth, rgb, p, mode, H, W)
        rd, rc = _reference_chain(depth, rgb, p, mode, H, W)
        assert gd.shape == (1, H, W) and gc.shape == (3, H, W)
        assert np.array_equal(gd, rd) and np.array_equal(gc, rc), "draw %d %s" % (k, p)


class _Recorder:
    """Stands in for numpy.random / random and records every call, in order."""

    def __init__(self, log, name, rng):
        self.log, self.name, self.rng = log, name, rng

    def __getattr__(self, fn):
        def call(*a):
            v = getattr(self.rng, fn)(*a)
            self.log.append((self.name, fn, a))
            return v
        return call


@pytest.mark.parametrize("mode", ["DtoD", "RtoD"])
def test_draw_order_and_ranges(mode):
    from gdn_amd.datasets import draw_params_nyu
    for seed in range(40):
        log = []
        py, npr = _Recorder(log, "random", random.Random(seed)), _Recorder(log, "np", np.random.RandomState(seed))
        d = draw_params_nyu(480, 640, mode, py, npr)
        calls = [(n, f, a) for n, f, a in log]
        assert calls[0] == ("np", "uniform", (1, 1.2)) and calls[1] == ("np", "uniform", (1.0, 1.5))
        h1, w1 = int(d["img_s"] * 251.0), int(d["img_s"] * 340.0)
        crop = [("np", "randint", (0, h1 - 251))] if h1 > 251 else []
        crop += [("np", "randint", (0, w1 - 340))] if w1 > 340 else []
        rest = [("np", "uniform", (-4, 4) if mode == "DtoD" else (-5, 5)), ("random", "random", ())]
        rest += [("np", "uniform", (0.8, 1.2))] if mode == "RtoD" else []
        assert calls[2:] == crop + rest, calls
        assert (d["h1"], d["w1"]) == (h1, w1) and 0 <= d["y1"] <= max(h1 - 252, 0) and 0 <= d["x1"] <= max(w1 - 341, 0)
        assert 1 <= d["img_s"] < 1.2 and 1 <= d["scale"] < 1.5 and abs(d["angle"]) <= (4 if mode == "DtoD" else 5)
        assert d["flip"] in (0, 1) and (0.8 <= d["mult"] < 1.2 if mode == "RtoD" else d["mult"] == 1.0)
        # the restatement draws the same values from the same generators
        assert N.draw_params(mode, random.Random(seed), np.random.RandomState(seed)) == d


def test_draw_edge_branches():
    from gdn_amd.datasets import draw_params_nyu

    class Fixed:
        def __init__(self, img_s):
            self.u = [img_s, 1.25, 1.5, 1.0]
            self.calls = []

        def uniform(self, lo, hi):
            return self.u.pop(0)

        def randint(self, lo, hi):
            self.calls.append((lo, hi))
            return hi - 1

    for img_s, want in [(1.0, []), (1.0035, [(0, 1)]), (1.1, [(0, 25), (0, 34)])]:
        npr = Fixed(img_s)
        d = draw_params_nyu(320, 420, "DtoD", random.Random(0), npr)
        assert npr.calls == want, (img_s, npr.calls)
        assert (d["y1"], d["x1"]) == ((want[0][1] - 1, want[1][1] - 1) if len(want) == 2 else
                                      (0, want[0][1] - 1) if want else (0, 0))


def _png(path, arr):
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(arr).save(path)


def test_nyu_train_dataset_layout(tmp_path):
    from gdn_amd._lib import GdnError
    from gdn_amd.datasets import NYUdataset
    with pytest.raises(GdnError, match="NYU training set: .*train_depths not found"):
        NYUdataset(str(tmp_path), None, train=True)
    for i in (3, 0, 2, 1, 4):
        _png(tmp_path / "train/train_depths" / ("%05d.png" % i), np.full((6, 9), 1000 + i, np.uint16))
        _png(tmp_path / "train/train_colors" / ("%05d.png" % i), np.full((6, 9, 3), i, np.uint8))
    with pytest.raises(GdnError, match="NYU training set"):
        NYUdataset(str(tmp_path / "train"), None, train=True)
    ds = NYUdataset(str(tmp_path), None, seed=11, train=True)
    assert len(ds) == 5
    order = list(range(5))
    random.Random(11).shuffle(order)                        # sorted, paired, then one seeded shuffle
    for k in range(5):
        gt, rgb, gt2 = ds[k]
        assert gt2 is gt and gt.dtype == np.float32 and gt.shape == (6, 9, 1) and rgb.shape == (6, 9, 3)
        assert (gt == 1000 + order[k]).all() and (rgb == order[k]).all()
    assert [s["gt"].name for s in NYUdataset(str(tmp_path), None, seed=11, train=True).samples] == \
        [s["gt"].name for s in ds.samples]
    assert len(NYUdataset(str(tmp_path), None, train=False)) == 0        # the test split is separate


def test_new_symbols_exported_and_arguments_checked():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gdn_build", REPO / "gdn-pytorch_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    dll = ctypes.CDLL(str(mod.build()))
    hdr = (REPO / "include" / "gdn_hip.h").read_text()
    from gdn_amd import _lib as L
    from gdn_amd import ops
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(dll, name) and name in L.EXPORTS, name
    assert "gdn_nyu_aug_params;" in hdr and ops.NYU_PARAMS_DTYPE.itemsize == 120
    assert L.ABI_VERSION == 223 and L.lib.gdn_version() == 223
    P = ctypes.c_void_p(16)
    nb = L.lib.gdn_nyu_augment_workspace_bytes(2, 320, 420, 1)
    assert nb >= 2 * 4 * 251 * 340 * 12 and L.lib.gdn_nyu_augment_workspace_bytes(0, 320, 420, 1) == 0
    aug = L.lib.raw("gdn_nyu_augment")
    assert aug(P, P, 2, 320, 420, 1, P, 252, 320, P, P, P, nb, None) == -1          # H > 251
    assert aug(P, P, 2, 320, 420, 0, P, 224, 341, P, P, P, nb, None) == -1          # W > 340
    assert aug(P, P, 2, 320, 420, 0, None, 224, 320, P, P, P, nb, None) == -1       # no params
    assert aug(P, P, 2, 320, 420, 1, P, 224, 320, P, P, P, nb - 1, None) == -3      # workspace too small
    rs = L.lib.raw("gdn_pil_resize_bilinear")
    assert rs(P, 0, 1, 10, 10, 3, 0, 0, 20, 20, 15, 0, 6, 20, P, P, 1 << 20, None) == -1   # window leaves the output
    assert rs(P, 0, 1, 10, 10, 1, 1, 0, 20, 20, 0, 0, 20, 20, P, P, 1 << 20, None) == -1   # 'F' needs float32
    assert rs(P, 1, 1, 10, 10, 1, 0, 0, 20, 20, 0, 0, 20, 20, P, P, 1 << 20, None) == -1   # float32 8 bpc needs bytescale
    assert rs(P, 1, 1, 10, 10, 1, 1, 0, 20, 20, 0, 0, 20, 20, P, P, 16, None) == -3        # workspace too small
    m = (ctypes.c_double * 4)(1, 0, 0, 1)
    o = (ctypes.c_double * 2)(0, 0)
    rot = L.lib.raw("gdn_spline_rotate3")
    assert rot(P, 1, 1, 3, 10, m, o, 1, P, P, 1 << 20, None) == -1                  # H < 4
    assert rot(P, 1, 1, 10, 10, None, o, 1, P, P, 1 << 20, None) == -1              # no matrix
    assert rot(P, 2, 1, 10, 10, m, o, 1, P, P, 64, None) == -3                      # workspace too small


def test_params_struct_matches_draws():
    from gdn_amd import ops
    from gdn_amd._lib import GdnError
    pytest.importorskip("scipy.special")
    py, npr = random.Random(2), np.random.RandomState(2)
    draws = [N.draw_params("RtoD", py, npr) for _ in range(3)] + edge_draws("DtoD")[:1]
    p = ops.nyu_params(draws[:3], 224, 320, "RtoD")
    for b, d in enumerate(draws[:3]):
        h2, w2 = N.second_size(d["scale"])
        assert (p[b]["h2"], p[b]["w2"]) == (h2, w2)
        assert (p[b]["cy"], p[b]["cx"]) == N.center_offsets(h2, w2, 224, 320)
        m, off = N.rotate_matrix(d["angle"], 251, 340)
        assert list(p[b]["m"]) == m and list(p[b]["off"]) == off
        assert tuple(p[b]["zn1"]) == (N.z_pow(250), N.z_pow(339))
    q = ops.nyu_params(draws[3:], 96, 128, "DtoD")
    assert (q[0]["cy"], q[0]["cx"]) == N.center_offsets(251, 340, 96, 128)      # DtoD: from the 251 x 340 colour image
    bad = dict(draws[0], y1=draws[0]["h1"])
    with pytest.raises(GdnError, match="inconsistent"):
        ops.nyu_params([bad], 224, 320, "RtoD")
