"""CPU restatement (numpy) of the reference's NYU Depth v2 training transform -- TEST INFRASTRUCTURE ONLY.

The product path is gdn_amd.datasets.GpuNYUAugmentLoader on the HIP kernels of csrc/nyu_augment.hip, which must match
this file bit for bit.  This file in turn is pinned against SciPy 1.15 and Pillow 12 by tests/test_nyu_augment_cpu.py.

Reference path: GDN_main.py:94-129 (EnhancedCompose of Merge, RandomCropNumpy(251, 340), RandomRotate, Split, then
CenterCrop, RandomHorizontalFlip, RandomColor (RtoD), ArrayToTensor, Normalize) and datasets_list.py:399-430 (the two
imresize calls around it).  imresize is scipy.misc.imresize: bytescale, then Pillow BILINEAR; the 'F' variant resizes a
float32 image in Pillow's 'F' mode with no bytescale.

Two third-party operations are restated here:
  * Pillow's 'F' bilinear resampler (Resample.c, 32bpc path): triangle weights in double normalised to 1, one double
    accumulator per output sample, horizontal pass first (float32 result), then the vertical pass.  A pass is skipped
    when its axis keeps its size.  The 8-bpc resampler is oracle.kitti_augment.resize_bilinear_u8.
  * scipy.ndimage.rotate(a, angle, reshape=False, axes=(0, 1), mode='constant'), order 3: matrix and offset as SciPy
    computes them; cubic B-spline prefilter (pole z = sqrt(3) - 2, mirror boundaries) along axis 0, then axis 1, in
    float64; 4 x 4 taps with mirrored indices; an output whose source coordinate leaves [0, n - 1] on either axis is 0.
    At float64 this is not SciPy's exact operation order; the float32 results agree on every case tested.
"""
import math

import numpy as np

from oracle.kitti_augment import bytescale, resize_bilinear_u8

CROP_H, CROP_W = 251, 340
SPLINE_Z = math.sqrt(3.0) - 2.0
SPLINE_GAIN = (1.0 - SPLINE_Z) * (1.0 - 1.0 / SPLINE_Z)


def z_pow(n):
    """SPLINE_Z ** n as a running product (the device receives the same value)."""
    p = 1.0
    for _ in range(n):
        p = p * SPLINE_Z
    return p


# ---------------------------------------------------------------------------------------------- Pillow 'F' bilinear

def _weights_f(in_size, out_size):
    """Per output index: (xmin, taps) with the taps as normalised doubles, as Pillow's precompute_coeffs."""
    scale = float(in_size) / float(out_size)
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
            ww += w[-1]
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, w))
    return out


def resize_f(img, out_h, out_w):
    """Image.frombytes('F', ...).resize((out_w, out_h), BILINEAR) of a float32 [H, W] array."""
    a = np.asarray(img, dtype=np.float32)
    H, W = a.shape
    if W != out_w:
        tmp = np.empty((H, out_w), np.float32)
        for xx, (x0, w) in enumerate(_weights_f(W, out_w)):
            acc = np.zeros(H)
            for j, k in enumerate(w):
                acc = acc + a[:, x0 + j].astype(np.float64) * k
            tmp[:, xx] = acc.astype(np.float32)
        a = tmp
    if H != out_h:
        tmp = np.empty((out_h, a.shape[1]), np.float32)
        for yy, (y0, w) in enumerate(_weights_f(H, out_h)):
            acc = np.zeros(a.shape[1])
            for j, k in enumerate(w):
                acc = acc + a[y0 + j].astype(np.float64) * k
            tmp[yy] = acc.astype(np.float32)
        a = tmp
    return a


def imresize_u8(arr, out_h, out_w):
    """scipy.misc.imresize(arr, (out_h, out_w)): bytescale (whole array) then Pillow BILINEAR, uint8 out."""
    return resize_bilinear_u8(bytescale(arr), out_h, out_w)


# ---------------------------------------------------------------------------------------------- spline rotation

def rotate_matrix(angle, n0, n1):
    """(matrix [4], offset [2]) of scipy.ndimage.rotate(reshape=False, axes=(0, 1)) on an n0 x n1 plane."""
    from scipy import special
    c, s = special.cosdg(angle), special.sindg(angle)
    rot = np.array([[c, s], [-s, c]])
    shape = np.array([n0, n1])
    out_center = rot @ ((shape - 1) / 2)
    in_center = (shape - 1) / 2
    offset = in_center - out_center
    return [float(v) for v in rot.ravel()], [float(v) for v in offset]


def _prefilter_last(c, zn1):
    """In-place cubic B-spline prefilter along the last axis of a float64 array (mirror boundaries)."""
    z = SPLINE_Z
    n = c.shape[-1]
    c *= SPLINE_GAIN
    c0 = c[..., 0] + zn1 * c[..., n - 1]
    zi = z
    for i in range(1, n - 1):
        c0 = c0 + zi * (c[..., i] + zn1 * c[..., n - 1 - i])
        zi = zi * z
    c[..., 0] = c0 / (1.0 - zn1 * zn1)
    for i in range(1, n):
        c[..., i] = c[..., i] + z * c[..., i - 1]
    c[..., n - 1] = (z * c[..., n - 2] + c[..., n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        c[..., i] = z * (c[..., i + 1] - c[..., i])
    return c


def spline_coeffs(plane):
    """float32/64 [n0, n1] -> float64 B-spline coefficients (axis 0 first, then axis 1)."""
    n0, n1 = plane.shape
    c = np.ascontiguousarray(plane, dtype=np.float64).T.copy()
    _prefilter_last(c, z_pow(n0 - 1))
    c = c.T.copy()
    return _prefilter_last(c, z_pow(n1 - 1))


def _bspline_w(t):
    u = 1.0 - t
    w0 = u * u * u / 6.0
    w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0
    w3 = 1.0 - (w0 + w1 + w2)
    return (w0, w1, w2, w3)


def _mirror(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def spline_interp(coef, matrix, offset):
    """Order-3 affine resampling of one plane: output (y, x) reads input (m0 y + m1 x + o0, m2 y + m3 x + o1)."""
    n0, n1 = coef.shape
    y = np.arange(n0, dtype=np.float64)[:, None]
    x = np.arange(n1, dtype=np.float64)[None, :]
    c0 = (y * matrix[0] + x * matrix[1]) + offset[0]
    c1 = (y * matrix[2] + x * matrix[3]) + offset[1]
    inside = (c0 >= 0.0) & (c0 <= n0 - 1) & (c1 >= 0.0) & (c1 <= n1 - 1)
    c0 = np.where(inside, c0, 0.0)
    c1 = np.where(inside, c1, 0.0)
    f0, f1 = np.floor(c0), np.floor(c1)
    wy, wx = _bspline_w(c0 - f0), _bspline_w(c1 - f1)
    i0, i1 = f0.astype(np.int64) - 1, f1.astype(np.int64) - 1
    acc = np.zeros((n0, n1))
    for a in range(4):
        ya = _mirror(i0 + a, n0)
        for b in range(4):
            acc = acc + (coef[ya, _mirror(i1 + b, n1)] * wy[a]) * wx[b]
    return np.where(inside, acc, 0.0).astype(np.float32)


def rotate(a, angle, clip=True):
    """RandomRotate on an [n0, n1, C] float32 array: every channel plane rotated, then clipped to the input's range."""
    a = np.asarray(a, dtype=np.float32)
    n0, n1, C = a.shape
    m, off = rotate_matrix(angle, n0, n1)
    out = np.stack([spline_interp(spline_coeffs(a[:, :, c]), m, off) for c in range(C)], axis=2)
    if clip:
        out = np.clip(out, a.min(), a.max())
    return out


# ---------------------------------------------------------------------------------------------- the sample chain

def draw_params(mode, py_rng, np_rng):
    """The reference's draws for one sample, in its order (see gdn_amd.datasets.draw_params_nyu)."""
    img_s = np_rng.uniform(1, 1.2)
    scale = np_rng.uniform(1.0, 1.5)
    h1, w1 = int(img_s * 251.0), int(img_s * 340.0)
    y1 = x1 = 0
    if h1 == CROP_H and w1 == CROP_W:
        pass
    elif h1 == CROP_H:
        x1 = int(np_rng.randint(0, w1 - CROP_W))
    elif w1 == CROP_W:
        y1 = int(np_rng.randint(0, h1 - CROP_H))
    else:
        y1 = int(np_rng.randint(0, h1 - CROP_H))
        x1 = int(np_rng.randint(0, w1 - CROP_W))
    angle = np_rng.uniform(-4, 4) if mode == "DtoD" else np_rng.uniform(-5, 5)
    flip = 1 if py_rng.random() < 0.5 else 0
    mult = np_rng.uniform(0.8, 1.2) if mode == "RtoD" else 1.0
    return dict(img_s=img_s, scale=scale, h1=h1, w1=w1, y1=y1, x1=x1, angle=angle, flip=flip, mult=mult)


def second_size(scale):
    """imresize(a, scale) on a 251 x 340 image: (array(im.size) * scale).astype(int), im.size = (w, h)."""
    w2, h2 = (np.array([CROP_W, CROP_H]) * scale).astype(int)
    return int(h2), int(w2)


def center_offsets(h, w, H, W):
    return int(round((h - H) / 2.)), int(round((w - W) / 2.))


def _normalize(chw):
    t = chw.astype(np.float32) / np.float32(255)
    return (t - np.float32(0.5)) / np.float32(0.5)


def augment_sample(depth, rgb, p, mode, H, W):
    """depth float32 [H0, W0] (or [H0, W0, 1]), rgb uint8 [H0, W0, 3] -> (depth [1, H, W], rgb [3, H, W]) float32."""
    depth = np.asarray(depth, np.float32)
    if depth.ndim == 3:
        depth = depth[:, :, 0]
    rgb_f = np.asarray(rgb).astype(np.float32)
    h1, w1, y1, x1 = p["h1"], p["w1"], p["y1"], p["x1"]
    d = resize_f(depth, h1, w1) / np.float32(p["scale"])
    h2, w2 = second_size(p["scale"])
    if mode == "DtoD":
        rgb1 = imresize_u8(rgb_f, CROP_H, CROP_W)
        merged = d[y1:y1 + CROP_H, x1:x1 + CROP_W, None]
        rot = rotate(merged, p["angle"])
        d2 = resize_f(rot[:, :, 0], h2, w2)
        rgb2 = rgb1
    else:
        rgb1 = imresize_u8(rgb_f, h1, w1).astype(np.float32)
        merged = np.concatenate([rgb1, d[:, :, None]], axis=2)[y1:y1 + CROP_H, x1:x1 + CROP_W]
        rot = rotate(merged, p["angle"])
        rgb2 = imresize_u8(rot[:, :, :3], h2, w2)
        d2 = resize_f(rot[:, :, 3], h2, w2)
    i, j = center_offsets(rgb2.shape[0], rgb2.shape[1], H, W)
    d2 = d2[i:i + H, j:j + W]
    rgb2 = rgb2[i:i + H, j:j + W]
    if p["flip"]:
        d2, rgb2 = np.fliplr(d2), np.fliplr(rgb2)
    if mode == "RtoD":
        rgb2 = np.clip(rgb2 * p["mult"], 0, 255)
    return _normalize(d2[None]), _normalize(rgb2.transpose(2, 0, 1))
