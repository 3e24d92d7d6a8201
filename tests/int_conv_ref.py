"""Exact-integer reference of the bf16 convolution path (not a test module).

Why an exact test is possible.  The bf16 kernels multiply bf16 operands -- the products are exact in fp32 -- and accumulate in
fp32.  With integer-valued operands every partial sum is an integer, and as long as the sum of the ABSOLUTE products that can
meet in one accumulator stays below 2^24, every partial sum of every summation order (tile shape, tap split, K-split tail,
round count, slab order) is exactly representable: nothing rounds until the kernel stores bf16 with f32_to_bf16_h
(csrc/common.h, round to nearest even).  The result is therefore fully determined -- bf16_rne(exact integer convolution) --
and torch.equal is the bar.  exactness_bound() is that sum of absolute products; every GPU test asserts it below 2^24 before it
compares anything.

The reference is torch's float64 conv2d / conv_transpose2d / pad(mode="reflect") and their autograd, all exact on these values
(|v| < 2^24 << 2^53).  It rounds with .float().bfloat16() exactly where the kernels store bf16 (the .float() is exact below
2^24), and nowhere else.  Rounding points, from the code:

  forward (gdn_conv_fwd: conv_igemm_bf16, conv_rowpatch_bf16, conv_ring_bf16, conv_ring2_bf16, splitk_combine_kernel)
      ONE: y = bf16(relu?(acc * ep_scale + ep_shift) + addsrc).  The BatchNorm statistics slots are written from the fp32
      accumulators BEFORE the epilogue: sum and sum of squares of the raw integer convolution, not rounded.
  data gradient, zero-padded / strided / transposed layer (gdn_conv_dgrad, same kernels)
      ONE: dx = bf16(acc + addsrc).
  data gradient, reflection-padded layer
      TWO: the kernels write the gradient on the PADDED domain to the workspace in bf16 (first rounding);
      reflect_fold_kernel sums the up to nine padded positions that reflect onto a pixel in fp32, adds addsrc and stores bf16
      (second rounding).  With dx_up2x = 1 reflect_fold_up2x8_kernel also applies the adjoint of the x2 bilinear interpolation
      between the two roundings: weights are products of {1/4, 3/4, 1}, multiples of 1/16, so the granule of that sum is 1/16.
  BatchNorm-backward partials of the data-gradient epilogue (bnb)
      none of their own: dz is the gradient AS STORED (bf16), masked by y * scale + shift > 0; sum dz and sum dz * xhat with
      xhat = (y - mean) * invstd are fp32 sums -- exact for integer y / mean / shift and power-of-two scale / invstd.
  fp32 results (weight gradients, statistics, partials, the head's depth map): not rounded.
  head (conv_head_mfma_bf16_kernel): the fp32 weights enter as three bf16 terms w1 + w2 + w3 (each the round-to-nearest bf16
      of the remainder), exact for weights of up to 24 significant bits, and every term of a weight m * 2^-n is a multiple of
      2^-n: that is the granule.  The sum of the terms' magnitudes exceeds |w| by at most 2^-7 |w|, which the head tests add
      to the bound.  Weights m * 2^-17, |m| < 2^17, are used up by w1 + w2 (8 + 8 bits and the remainder's sign); the tests
      also run m * 2^-20 so that w3 carries bits.

Layouts here are torch's (NCHW activations; Conv2d weight [Cout, Cin, k, k], ConvTranspose2d weight [Cin, Cout, k, k]).
"""
import collections
import functools

import torch
import torch.nn.functional as F

TWO24 = float(2 ** 24)

# one layer: channels, window, stride, padding, reflection padding, ConvTranspose2d
Geom = collections.namedtuple("Geom", "ci co k s p refl tr")


def geom_of(case):
    """(name, Cin, Cout, k, stride, pad, reflect, transposed, B, H, W) of tests/test_hip_bf16.py -> Geom, (B, H, W)."""
    _, ci, co, k, s, p, refl, tr, B, H, W = case
    return Geom(ci, co, k, s, p, bool(refl and p > 0), tr), (B, H, W)


def out_hw(g, H, W):
    if g.tr:
        return (H - 1) * g.s - 2 * g.p + g.k, (W - 1) * g.s - 2 * g.p + g.k
    return (H + 2 * g.p - g.k) // g.s + 1, (W + 2 * g.p - g.k) // g.s + 1


def bf16_rne(t):
    """Round to bfloat16 (nearest, ties to even) the way the kernels' stores do; float64 in, float64 out."""
    return t.float().bfloat16().double()


def is_bf16(t):
    return bf16_rne(t) == t


def is_tie(t):
    """True where a value lies exactly half way between two neighbouring bf16 values (8 significant bits)."""
    a = t.abs().double()
    _, e = torch.frexp(a)                                   # a = m * 2^e, m in [0.5, 1): the binade's ulp is 2^(e - 8)
    half = torch.exp2((e - 9).double())
    return (a > 0) & (torch.remainder(a, 2 * half) == half)


def conv(x, w, g):
    """The layer's raw convolution in the dtype of its operands (float64 here)."""
    if g.tr:
        return F.conv_transpose2d(x, w, None, g.s, g.p)
    if g.refl:
        return F.conv2d(F.pad(x, (g.p,) * 4, mode="reflect"), w, None, g.s, 0)
    return F.conv2d(x, w, None, g.s, g.p)


def _ch(v):
    return v.double().view(1, -1, 1, 1)


def fwd_ref(x, w, g, scale=None, shift=None, relu=False, addsrc=None, raw=None):
    """(y as stored, raw accumulator): one rounding, after ep_scale / ep_shift, ReLU and addsrc.  raw: the accumulator of an
    earlier call on the same operands (saves the convolution)."""
    raw = conv(x, w, g) if raw is None else raw
    v = raw
    if scale is not None:
        v = v * _ch(scale) + _ch(shift)
    if relu:
        v = v.clamp(min=0)
    if addsrc is not None:
        v = v + addsrc
    return bf16_rne(v), raw


def stats_ref(raw):
    """What the statistics slots add up to: per-channel sum and sum of squares of the raw accumulators."""
    return raw.sum((0, 2, 3)), (raw * raw).sum((0, 2, 3))


def _up(xl):
    return F.interpolate(xl, scale_factor=2, mode="bilinear", align_corners=False)


def dgrad_padded(dy, w, g, in_hw, rounded=True):
    """Reflection layer: the gradient on the padded domain as gdn_conv_dgrad leaves it in the workspace (bf16: first rounding)."""
    H, W = in_hw
    xp = torch.zeros(dy.shape[0], g.ci, H + 2 * g.p, W + 2 * g.p, dtype=dy.dtype, requires_grad=True)
    dxp, = torch.autograd.grad(F.conv2d(xp, w, None, g.s, 0), xp, dy)
    return bf16_rne(dxp) if rounded else dxp


def dgrad_ref(dy, w, g, in_hw, addsrc=None, up2x=0, rounded=True):
    """dx as stored.  Zero-padded, strided and transposed layers: bf16(adjoint(dy) + addsrc).  Reflection layers: the
    two-rounding model -- bf16 on the padded domain, then fold (+ the adjoint of the x2 bilinear interpolation when up2x = 1:
    dx and addsrc are then the LOW-resolution gradient), + addsrc, bf16.  rounded=False: no rounding anywhere (plain autograd)."""
    H, W = in_hw
    rnd = bf16_rne if rounded else (lambda t: t)
    if not g.refl:
        assert not up2x
        x0 = torch.zeros(dy.shape[0], g.ci, H, W, dtype=dy.dtype, requires_grad=True)
        dx, = torch.autograd.grad(conv(x0, w, g), x0, dy)
    else:
        dxp = dgrad_padded(dy, w, g, in_hw, rounded)
        lo = (H // 2, W // 2) if up2x else (H, W)
        x0 = torch.zeros(dy.shape[0], g.ci, *lo, dtype=dy.dtype, requires_grad=True)
        full = _up(x0) if up2x else x0
        dx, = torch.autograd.grad(F.pad(full, (g.p,) * 4, mode="reflect"), x0, dxp)
    if addsrc is not None:
        dx = dx + addsrc
    return rnd(dx)


def dgrad_autograd(dy, w, g, in_hw, addsrc=None):
    """Plain autograd of the layer as written (reflection padding inside the graph), nothing rounded."""
    H, W = in_hw
    x0 = torch.zeros(dy.shape[0], g.ci, H, W, dtype=dy.dtype, requires_grad=True)
    dx, = torch.autograd.grad(conv(x0, w, g), x0, dy)
    return dx if addsrc is None else dx + addsrc


def wgrad_ref(x, dy, g):
    """The weight gradient in torch's weight layout; fp32 on the device and not rounded."""
    shape = (g.ci, g.co, g.k, g.k) if g.tr else (g.co, g.ci, g.k, g.k)
    w0 = torch.zeros(shape, dtype=x.dtype, requires_grad=True)
    dw, = torch.autograd.grad(conv(x, w0, g), w0, dy)
    return dw


def bnb_ref(dx_stored, y, coef, relu):
    """Sums of the fused BatchNorm-backward reduction: dz = dx as stored, masked where relu(y * scale + shift) is off;
    (sum dz, sum dz * xhat), xhat = (y - mean) * invstd.  coef rows: scale, shift, mean, invstd.  Also returns the largest sum
    of |dz * xhat| over an aligned run of 512 pixels (NHWC pixel order): every slot -- a 256- or 512-pixel tile or a 16-pixel
    row group of the tail -- is a subset of such a run, so that number bounds every partial sum the kernels can form."""
    sc, sh, mu, isd = [_ch(c) for c in coef]
    dz = dx_stored * ((y * sc + sh) > 0) if relu else dx_stored
    t = dz * ((y - mu) * isd)
    a = t.abs().permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    a = F.pad(a, (0, 0, 0, -a.shape[0] % 512)).reshape(-1, 512, t.shape[1]).sum(1)
    return dz.sum((0, 2, 3)), t.sum((0, 2, 3)), float(a.max())


def exactness_bound(x, w, granule, g=None, mode="fwd", in_hw=None, scale=None, shift=None, addsrc=None, up2x=0):
    """max conv(|x|, |w|) / granule: no partial sum of the products, in any order, exceeds it in units of the granule (the
    largest power of two every term is a multiple of), so below 2^24 nothing rounds in fp32.
    mode "fwd": x, w the layer's operands (g None: a plain 'same' correlation, the head); the epilogue terms are included --
    max(|conv| * |scale| + |shift| + |addsrc|).  mode "dgrad": x is dy; the adjoint of the layer on |dy|, |w| (reflection layers:
    folded, + 2^-7 for the workspace's rounding, + the up2x adjoint), + |addsrc|.  mode "wgrad": x, w are the activation and dy:
    the weight gradient of |x| and |dy|."""
    ax, aw = x.abs().double(), w.abs().double()
    if mode == "wgrad":
        return float(wgrad_ref(ax, aw, g).max()) / granule
    if mode == "dgrad":
        b = dgrad_ref(ax, aw, g, in_hw, None, up2x, rounded=False)
        if g.refl:
            b = b * (1 + 2.0 ** -7)
    elif g is None:
        b = F.conv2d(ax, aw, None, 1, w.shape[-1] // 2)
    else:
        b = conv(ax, aw, g)
    if scale is not None:
        b = b * _ch(scale).abs() + _ch(shift).abs()
    if addsrc is not None:
        b = b + addsrc.abs()
    return float(b.max()) / granule


# ---------------------------------------------------------------------------------------------------------------------------
# Operand sets: seeded, every value exactly representable in bf16
# ---------------------------------------------------------------------------------------------------------------------------
Operands = collections.namedtuple("Operands", "x w dy add_y add_x")


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _narrow_ok(o, g, in_hw):
    y = conv(o.x, o.w, g)
    if not (bool(is_bf16(y).all()) and bool(is_bf16(y + o.add_y).all()) and float((y * y).sum((0, 2, 3)).max()) < TWO24):
        return False
    if g.refl and not bool(is_bf16(dgrad_padded(o.dy, o.w, g, in_hw, rounded=False)).all()):
        return False
    dx = dgrad_autograd(o.dy, o.w, g, in_hw)
    return bool(is_bf16(dx).all()) and bool(is_bf16(dx + o.add_x).all())


@functools.lru_cache(maxsize=None)
def operands(g, bhw, kind, seed=0):
    """Operands of one layer at one shape (torch layouts, float64).
    narrow: x, dy, the two addsrc tensors in {-1, 0, 1}; w in {-1, 0, 1}, thinned (a seeded keep-mask whose density is halved)
            until NOTHING rounds: the forward output, the data gradient (on the padded domain too), each with and without its
            addsrc, are all bf16 values, and every per-channel sum of y^2 over the tensor is below 2^24.
    wide:   uniform integers in [-8, 8] (addsrc too): sums of a few thousand products reach the thousands, where bf16 keeps
            multiples of 8 or 16 -- most outputs round and a good share are exact ties."""
    B, H, W = bhw
    Ho, Wo = out_hw(g, H, W)
    gen = torch.Generator().manual_seed(1000 * seed + (17 if kind == "wide" else 3))
    a = 8 if kind == "wide" else 1
    wshape = (g.ci, g.co, g.k, g.k) if g.tr else (g.co, g.ci, g.k, g.k)
    x, w = _ints(gen, (B, g.ci, H, W), -a, a), _ints(gen, wshape, -a, a)
    dy = _ints(gen, (B, g.co, Ho, Wo), -a, a)
    add_y, add_x = _ints(gen, (B, g.co, Ho, Wo), -a, a), _ints(gen, (B, g.ci, H, W), -a, a)
    o = Operands(x, w, dy, add_y, add_x)
    if kind == "wide":
        return o
    assert kind == "narrow"
    u = torch.rand(wshape, generator=gen)
    # first density from the variance of a sum of K products of two {-1, 0, 1} values (4/9 each): 5.5 sigma within 256, where
    # every integer is a bf16 value, and the sum of squares within its bound; then halve until the conditions hold
    taps = g.k * g.k / (g.s * g.s if g.tr else 1)
    K = max(g.ci, g.co) * taps
    dens = min(1.0, 4800.0 / K, 0.8 * TWO24 / (B * Ho * Wo * g.ci * taps * 4.0 / 9.0))
    for _ in range(12):
        o = o._replace(w=w * (u < dens))
        if _narrow_ok(o, g, (H, W)):
            return o
        dens *= 0.5
    raise AssertionError("no narrow weight set found for %s at %s" % (g, bhw))
