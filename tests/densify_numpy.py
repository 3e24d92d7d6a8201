"""Numpy restatement of the depth densification and the byte encoder (gdn_depth_densify, gdn_depth_encode_u8).
numpy only: tests/test_densify_cpu.py pins the stages to scipy.ndimage where the two coincide, tests/test_hip_densify.py
compares the device pools with densify_pool bit for bit.

All arithmetic is float32, one operation at a time.  empty(v) := !(v > 0.1f)."""
import numpy as np

F = np.float32
EMPTY = F(0.1)
DIAMOND = np.array([[0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]], bool)
TAPS = (F(1), F(4), F(6), F(4), F(1))


def empty(v):
    with np.errstate(invalid="ignore"):
        return ~(v > EMPTY)


def window_reduce(v, footprint, fill, op):
    """op (np.maximum / np.minimum) over the cells of the odd-sized boolean footprint around every pixel; cells outside the
    image read `fill`."""
    fh, fw = footprint.shape
    ry, rx = fh // 2, fw // 2
    h, w = v.shape
    p = np.full((h + 2 * ry, w + 2 * rx), fill, F)
    p[ry:ry + h, rx:rx + w] = v
    out = None
    for dy in range(fh):
        for dx in range(fw):
            if footprint[dy, dx]:
                s = p[dy:dy + h, dx:dx + w]
                out = s.copy() if out is None else op(out, s)
    return out


def box_max(v, r):
    """The maximum over the (2r + 1)^2 box, out-of-image cells reading 0: rows, then columns (a maximum of maxima)."""
    rows = window_reduce(v, np.ones((1, 2 * r + 1), bool), F(0), np.maximum)
    return window_reduce(rows, np.ones((2 * r + 1, 1), bool), F(0), np.maximum)


def invert(D, max_depth):
    D = np.asarray(D, F)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(D > EMPTY, F(max_depth) - D, F(0)).astype(F)
    return np.where(empty(v), F(0), v).astype(F)


def dilate_diamond(v):
    return window_reduce(v, DIAMOND, F(0), np.maximum)


def close_box(v):
    return window_reduce(window_reduce(v, np.ones((5, 5), bool), F(0), np.maximum), np.ones((5, 5), bool), F(np.inf), np.minimum)


def fill_holes(v, r):
    return np.where(empty(v), box_max(v, r), v).astype(F)


def extend_top(v):
    h, w = v.shape
    full = ~empty(v)
    has, top = full.any(axis=0), full.argmax(axis=0)
    above = has[None, :] & (np.arange(h)[:, None] < top[None, :])
    return np.where(above, v[top, np.arange(w)][None, :], v).astype(F)


def median5(v):
    """The 13th smallest of the 5 x 5 window with replicated borders."""
    h, w = v.shape
    p = np.pad(v, 2, mode="edge")
    stack = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)])
    return np.partition(stack, 12, axis=0)[12]


def reflect101(i, n):
    """Index i reflected into [0, n) without repeating the edge sample: period 2 (n - 1); n = 1 reads itself."""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m >= n, p - m, m)


def blur_pass(v, axis):
    n = v.shape[axis]
    p = [np.take(v, reflect101(np.arange(n) + k - 2, n), axis=axis) for k in range(5)]
    return (((((p[0] + TAPS[1] * p[1]) + TAPS[2] * p[2]) + TAPS[3] * p[3]) + p[4]) * F(0.0625)).astype(F)


def blur(v):
    return blur_pass(blur_pass(v, 1), 0)


def stages(D, max_depth=100.0):
    """The value of v after each of the eight steps, and the output map last: a list of nine float32 [h, w] arrays."""
    out = [invert(D, max_depth)]
    out.append(dilate_diamond(out[-1]))
    out.append(close_box(out[-1]))
    out.append(fill_holes(out[-1], 3))
    out.append(extend_top(out[-1]))
    out.append(fill_holes(out[-1], 15))
    v = out[-1]
    out.append(np.where(~empty(v), median5(v), v).astype(F))
    v = out[-1]
    out.append(np.where(~empty(v), blur(v), v).astype(F))
    v = out[-1]
    out.append(np.where(empty(v), F(0), F(max_depth) - v).astype(F))
    return out


def densify(D, max_depth=100.0):
    return stages(D, max_depth)[-1]


def densify_pool(pool, sizes, max_depth=100.0):
    """float32 [B,Hmax,Wmax] and [(h0, w0), ...] -> the output pool, padding +0.  Cells outside an image are not read."""
    pool = np.asarray(pool, F)
    out = np.zeros_like(pool)
    for b, (h0, w0) in enumerate(sizes):
        if h0 > 0 and w0 > 0:
            out[b, :h0, :w0] = densify(pool[b, :h0, :w0], max_depth)
    return out


def encode_u8(d, scale=80.0, keep_valid=False):
    """rint(clamp(d, 0, scale) / scale * 255) in float64, half to even; NaN -> 0; keep_valid: d > 0 that rounds to 0 -> 1."""
    d = np.asarray(d, F)
    c = d.astype(np.float64)
    with np.errstate(invalid="ignore"):
        c = np.where(c > 0.0, c, 0.0)
        c = np.where(c > float(scale), float(scale), c)
        q = np.rint(c / float(scale) * 255.0).astype(np.uint8)
        if keep_valid:
            q = np.where((d > 0) & (q == 0), np.uint8(1), q).astype(np.uint8)
    return q


def lidar_like(h, w, share, seed, near=4.0, far=70.0):
    """A sparse map with returns on about `share` of the pixels, on scan-line-like rows of the lower two thirds, nearer towards
    the bottom, with objects standing out of the ground."""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    t = np.clip((yy - h / 3.0) / max(1.0, h * 2.0 / 3.0), 0, 1)
    depth = far - (far - near) * t + 6.0 * np.sin(xx / 23.0) * (1 - t)
    for _ in range(6):
        cy, cx = r.randint(h // 3, max(h // 3 + 1, h)), r.randint(0, w)
        box = (abs(yy - cy) < max(1, h // 10)) & (abs(xx - cx) < max(1, w // 16))
        depth = np.where(box, r.uniform(near, 30.0), depth)
    lines = (yy % 3 == 0) if share > 0.15 else (yy % 5 == 0)
    keep = (yy >= h // 3) & lines & (r.rand(h, w) < share * (3 if share > 0.15 else 5) * 1.5)
    return np.where(keep, depth, 0).astype(F)
