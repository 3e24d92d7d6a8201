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
# The fp32 path: nothing rounds
#
# Direct kernels (conv_igemm fp32 tiles, conv_wgrad, conv_c1, conv_head_kernel): fp32 FMA on fp32 operands -- with integer
# operands every product and partial sum is an integer, the store does not round, and exactness_bound(...) < 2^24 (granule 1;
# 1/2 with the affine() epilogue) makes the result THE integer convolution whatever the tile, K-split or combine order.
# Winograd F(2x2,3x3) (conv_wino.hip) and F(3x3,2x2) (conv_wino2.hip): the three transforms hold only 0, +-1 and 1/2, so on
# integers U = G g G^T is a multiple of 1/4, V and A dy A^T are integers, every term of the per-bin sums is a multiple of 1/4
# and so is everything after them: granule 1/4 (1/64 behind the fused x2 bilinear loader, whose weights are sixteenths; 1/8
# behind an in_affine with scale 1/2).  Subtractions in the transforms mean the plain |x| * |w| bound is not enough:
# wino_exactness_bound() runs the scheme itself on |operands| with |matrices|.  The per-bin GEMMs run as bf16 x 3 split
# products by default (gemm_x3.h: six of the nine plane products); the split is exact, and the three dropped products are zero
# when both operands have at most 16 significant bits (two planes): wino_operands_16bit().
# ---------------------------------------------------------------------------------------------------------------------------
def layer_input(x, in_affine=None, in_relu=False, up2x=0):
    """What the transform-domain loaders make of x: [relu](x * scale + shift) (in_affine) or the x2 bilinear upsampling."""
    v = x
    if in_affine is not None:
        v = v * _ch(in_affine[0]) + _ch(in_affine[1])
        if in_relu:
            v = v.clamp(min=0)
    return _up(v) if up2x else v


def fwd_ref32(x, w, g, scale=None, shift=None, relu=False, addsrc=None, raw=None):
    """fp32 kernels: (y, raw accumulator) = relu?(acc * ep_scale + ep_shift) + addsrc, nothing rounded."""
    raw = conv(x, w, g) if raw is None else raw
    v = raw
    if scale is not None:
        v = v * _ch(scale) + _ch(shift)
    if relu:
        v = v.clamp(min=0)
    if addsrc is not None:
        v = v + addsrc
    return v, raw


def dgrad_ref32(dy, w, g, in_hw, addsrc=None, up2x=0):
    """fp32 kernels: the data gradient (reflection layers: padded domain, fold, + the adjoint of the x2 interpolation when up2x;
    the workspace is fp32, so this is plain autograd), + addsrc, nothing rounded."""
    return dgrad_ref(dy, w, g, in_hw, addsrc, up2x, rounded=False)


def _wino_models():
    import test_wino2conv_model_cpu as W2
    import test_winoconv_model_cpu as W1
    return W1, W2


def _amax(*arrs):
    return max(float(abs(a).max()) for a in arrs if a is not None and a.size)


def _up_adjoint(gfull):
    """Adjoint of the x2 bilinear interpolation (align_corners False) of a numpy [C, H, W] gradient, in its own dtype."""
    t = torch.from_numpy(gfull.copy())[None]
    lo = torch.zeros(1, t.shape[1], t.shape[2] // 2, t.shape[3] // 2, dtype=t.dtype, requires_grad=True)
    return torch.autograd.grad(_up(lo), lo, t)[0][0].numpy()


def _batch(t, absolute, dt):
    return (t.abs() if absolute else t).numpy().astype(dt)


def _run_f23(mode, a, b, g, dtype="float64", absolute=False, up2x=0):
    """F(2x2,3x3) (tests/test_winoconv_model_cpu.py) on a batch with the kernels' tilings: a reflection layer reads the mirrored
    ring on load and takes its data gradient on the padded domain, folded afterwards (up2x: + the adjoint interpolation);
    g.tr is a flip_taps layer.  Returns (result, largest intermediate, transformed GEMM operands)."""
    import numpy as np
    W1, W2 = _wino_models()
    dt = np.dtype(dtype).type
    A, Bm = _batch(a, absolute, dt), _batch(b, absolute, dt)
    mats = [abs(m) for m in (W1.BT, W1.G, W1.AT)] if absolute else None
    big, ops16, out = 0.0, [], []
    if mode == "wgrad":
        P, k = None, {}
        for xi, gi in zip(A, Bm):
            kv = {}
            W1.wino_forward(xi, np.zeros((1, g.ci, 3, 3), dt), dt, reflect=g.refl, mats=mats, keep=kv)
            dw = W1.wino_wgrad(kv["V"], gi, dt, mats=mats, keep=k, P0=P)
            P = k["P"]
            big = max(big, _amax(kv["V"], k["Dv"], P, dw))
            ops16 += [kv["V"], k["Dv"]]
        if g.tr:                                   # the module's own (stored) tap order and [Cin][Cout] layout
            dw = np.ascontiguousarray(dw.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
        return torch.from_numpy(dw.astype(np.float64)), big, ops16
    # conv-form weights [n][c][3][3]; a flip_taps layer is the correlation with the stored taps reversed
    wc = np.ascontiguousarray(Bm.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]) if g.tr else Bm
    if mode == "dgrad":
        wc = np.ascontiguousarray(wc[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))
    for img in A:
        k = {}
        if mode == "dgrad" and g.refl:
            y, _ = W1.wino_forward(np.pad(img, ((0, 0), (1, 1), (1, 1))), wc, dt, mats=mats, keep=k)
            y = W2.fold_reflect1(y)
            big = max(big, _amax(y))
            if up2x:
                y = _up_adjoint(y)
        else:
            y, _ = W1.wino_forward(img, wc, dt, reflect=g.refl and mode == "fwd", mats=mats, keep=k)
        big = max(big, _amax(k["V"], k["U"], k["M"], k["Y"], y))
        ops16 += [k["V"], k["U"]]
        out.append(y)
    return torch.from_numpy(np.stack(out).astype(np.float64)), big, ops16


def _run_f32(mode, a, b, g, dtype="float64", absolute=False):
    """F(3x3,2x2) (tests/test_wino2conv_model_cpu.py) on a batch: form A for a Conv2d forward and a ConvTranspose2d data gradient,
    form B for the other two (a reflection layer's data gradient on the padded domain, then folded)."""
    import numpy as np
    W2 = _wino_models()[1]
    dt = np.dtype(dtype).type
    A, Bm = _batch(a, absolute, dt), _batch(b, absolute, dt)
    mats = [abs(m) for m in (W2.BT, W2.G, W2.AT)] if absolute else None
    big, ops16, out = 0.0, [], []
    if mode == "wgrad":
        P, k = None, {}
        for xi, gi in zip(A, Bm):
            if not g.tr:
                V = W2.form_a_input(xi, g.refl, dt, mats)[0]
                dw = W2.wgrad(V, gi, g.ci, dt, keep=k, P0=P, mats=mats)
            else:                                  # ConvTranspose2d: V of dz, the lifted tiles of the input
                V = W2.form_a_input(gi, False, dt, mats)[0]
                dw = W2.wgrad(V, xi, g.co, dt, keep=k, P0=P, mats=mats)
            P = k["P"]
            big = max(big, _amax(V, k["Dv"], P, dw))
            ops16 += [V, k["Dv"]]
        return torch.from_numpy(dw.astype(np.float64)), big, ops16
    for img in A:
        k = {}
        if (mode == "fwd") != g.tr:
            y, _ = W2.strided_conv(img, Bm, g.refl and mode == "fwd", dt, keep=k, mats=mats)
        else:
            H, W = img.shape[1] * 2, img.shape[2] * 2
            if g.refl:
                y = W2.fold_reflect1(W2.transposed_conv(img, Bm, H + 2, W + 2, 1, dt, keep=k, mats=mats))
            else:
                y = W2.transposed_conv(img, Bm, H, W, 0, dt, keep=k, mats=mats)
        big = max(big, _amax(k["V"], k.get("U"), k.get("M"), k.get("Y"), y), k.get("big", 0.0))
        ops16 += [k["V"]] + ([k["U"]] if "U" in k else k["Us"])
        out.append(y)
    return torch.from_numpy(np.stack(out).astype(np.float64)), big, ops16


def wino_run(scheme, mode, a, b, g, dtype="float64", absolute=False, up2x=0):
    """The numpy model of scheme "f23" (3x3 stride 1) or "f32" (4x4 stride 2, Conv2d and ConvTranspose2d) on a batch.
    mode "fwd": a = layer input, b = w; "dgrad": a = dy, b = w; "wgrad": a = layer input, b = dy (torch layouts, float64).
    absolute: |operands| through |matrices|.  Returns (result as a float64 tensor -- exact conversion --, the largest magnitude
    of any intermediate: transformed operands, per-bin sums, output transform before cropping, fold), and the transformed
    operands of the per-bin GEMMs."""
    assert (g.k, g.s, g.p) == ((3, 1, 1) if scheme == "f23" else (4, 2, 1))
    if scheme == "f23":
        return _run_f23(mode, a, b, g, dtype, absolute, up2x)
    assert not up2x
    return _run_f32(mode, a, b, g, dtype, absolute)


def wino_exactness_bound(scheme, mode, a, b, g, granule=0.25, scale=None, shift=None, addsrc=None, up2x=0):
    """The scheme run with every transform matrix replaced by its absolute value on |a| and |b| (wino_run), the maximum over
    every intermediate and over the epilogue max(|y| * |scale| + |shift| + |addsrc|), in units of the granule: no partial sum of
    the real computation, in any order, exceeds it, so below 2^24 nothing rounds in fp32.  `a` of a forward / weight gradient
    is the layer input as the transform sees it (layer_input()).  granule: 1/4; 1/8 behind an in_affine with scale 1/2; 1/64
    behind the x2 bilinear loader (forward and weight gradient: V is in sixteenths from the start).
    The data gradient with up2x = 1 has two stages.  The padded-domain gradient is the plain scheme on dy (quarters) and comes
    out as the exact integer gradient; the fold pass then reads THOSE values and applies mirror sums and the adjoint
    interpolation (weights in sixteenths).  So the first stage is bounded as above in quarters, and the second by the same
    fold + adjoint of the absolute TRUE padded gradient, + |addsrc|, in sixteenths (pass granule = 1/16)."""
    y, big, _ = wino_run(scheme, mode, a, b, g, absolute=True, up2x=up2x)
    if mode == "dgrad" and up2x:
        assert scheme == "f23" and g.refl and scale is None
        H, W = a.shape[2:]
        dxp = dgrad_padded(a, b, g, (H, W), rounded=False).abs()
        x0 = torch.zeros(a.shape[0], g.ci, H // 2, W // 2, dtype=a.dtype, requires_grad=True)
        y, = torch.autograd.grad(F.pad(_up(x0), (1,) * 4, mode="reflect"), x0, dxp)
        return max(big / 0.25, float((y if addsrc is None else y + addsrc.abs()).max()) / granule)
    if scale is not None:
        y = y * _ch(scale).abs() + _ch(shift).abs()
    if addsrc is not None:
        y = y + addsrc.abs()
    return max(big, float(y.max())) / granule


def sig_bits(t):
    """The largest number of significant bits of any element of a numpy array (0 for zeros), up to 30."""
    import numpy as np
    m, _ = np.frexp(np.abs(t.astype(np.float64)))
    v = np.round(m * 2.0 ** 30).astype(np.int64)                     # exact for fp32 values: 24 bits
    low = (v & -v)[v != 0]                                            # lowest set bit; the highest is 2^29
    return int(30 - np.log2(low).min()) if low.size else 0


def wino_operands_16bit(scheme, mode, a, b, g, up2x=0):
    """The bf16 x 3 condition: every transformed operand of the per-bin GEMMs (V, U, A dy A^T) has at most 16 significant bits,
    so its third split plane is zero and the three products the kernels drop (a2 b3, a3 b2, a3 b3) vanish."""
    return at_most_16bit(wino_run(scheme, mode, a, b, g, up2x=up2x)[2])


def at_most_16bit(transformed):
    return max(sig_bits(t) for t in transformed) <= 16


# ---------------------------------------------------------------------------------------------------------------------------
# bf16 x 3 split products (csrc/gemm_x3.h), plane by plane
# ---------------------------------------------------------------------------------------------------------------------------
X3_KEPT = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))          # a1 b1, a1 b2, a2 b1, a1 b3, a2 b2, a3 b1


def x3_planes(t):
    """x3_split2: three bf16 terms, each the round-to-nearest-even bf16 of what is left; their sum is the fp32 value."""
    p1 = bf16_rne(t)
    p2 = bf16_rne(t - p1)
    p3 = bf16_rne(t - p1 - p2)
    assert torch.equal(p1 + p2 + p3, t)
    return p1, p2, p3


def x3_six_products(A, B, drop=()):
    """C[bin] = A[bin] @ B[bin]^T as the kernels form it: the sum of the six kept plane products (float64: exact here).
    drop: products (i, j) left out -- what a kernel that lost plane i of A or plane j of B, or that product, would give."""
    pa, pb = x3_planes(A), x3_planes(B)
    return sum(torch.bmm(pa[i], pb[j].transpose(1, 2)) for i, j in X3_KEPT if (i, j) not in drop)


def x3_bound(A, B, granule):
    """max over outputs of the sum of the absolute plane products, in units of the granule: below 2^24 no order of the kernel's
    MFMA accumulation rounds."""
    pa, pb = x3_planes(A), x3_planes(B)
    return float(sum(torch.bmm(pa[i].abs(), pb[j].abs().transpose(1, 2)) for i, j in X3_KEPT).max()) / granule


def x3_conv_six(x, w, g, drop=(), absolute=False):
    """The fp32 head on the matrix pipe (conv_head_mfma_kernel<true>, csrc/conv_head.hip): x and w each split into three bf16
    planes, the same six plane products kept (plane i of w against plane j of x).  The layer's convolution as that sum, in
    float64; absolute: of the planes' magnitudes -- the bound on every partial sum."""
    px, pw = x3_planes(x), x3_planes(w)
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    return sum(conv(f(px[j]), f(pw[i]), g) for i, j in X3_KEPT if (i, j) not in drop)


HEAD_PLANE_SETS = {"x24": ((0, 1), (0, 2)), "w24": ((1, 0), (2, 0)), "x2w2": ((1, 1), (0, 1), (1, 0))}      # (w plane, x plane) needed


@functools.lru_cache(maxsize=None)
def head_plane_operands(name, g, bhw):
    """A 64 -> 1 head's x and w that need the second and third plane of x (23-bit integers, sparse, against weights in
    {-1, 0, 1}), of w (the same with the roles swapped), and the product of the two second planes (256 m + n on both sides)."""
    B, H, W = bhw
    gen = torch.Generator().manual_seed(len(name) + H + W)
    xs, ws = (B, g.ci, H, W), ((g.ci, 1, 9, 9) if g.tr else (1, g.ci, 9, 9))
    small = lambda s: torch.randint(-1, 2, s, generator=gen).double()
    big = lambda s: torch.randint(-(2 ** 23) + 1, 2 ** 23, s, generator=gen).double()
    two = lambda s: (256.0 * torch.randint(-3, 4, s, generator=gen) + torch.randint(-3, 4, s, generator=gen)).double()
    keep = lambda s, d: (torch.rand(s, generator=gen) < d).double()
    if name == "x24":
        return big(xs) * keep(xs, 1.5e-4), small(ws)
    if name == "w24":
        return small(xs) * keep(xs, 1.5e-4), big(ws)
    assert name == "x2w2"
    return two(xs) * keep(xs, 1.5e-3), two(ws)


# case -> the products it needs (each must change the result when dropped)
X3_PLANE_CASES = {"a24_onehot": ((1, 0), (2, 0)), "onehot_b24": ((0, 1), (0, 2)), "a2b2": ((1, 1), (0, 1), (1, 0))}


@functools.lru_cache(maxsize=None)
def x3_plane_case(name, bins=2, M=128, N=256, K=64):
    """Operands [bins, M, K] and [bins, N, K] (C = A @ B^T; the reduction GEMM takes their transposes) that need the second and
    third split plane: 23-bit integers against one-hot +-1 rows (the products a2 b1, a3 b1 -- or a1 b2, a1 b3 with the roles
    swapped), and sparse values 256 m + n, |m|, |n| <= 3, on both sides (a2 b2)."""
    gen = torch.Generator().manual_seed(len(name) + K)
    sign = lambda *s: torch.randint(0, 2, s, generator=gen).double() * 2 - 1

    def big(rows):
        return torch.randint(-(2 ** 23) + 1, 2 ** 23, (bins, rows, K), generator=gen).double()

    def onehot(rows):
        t = torch.zeros(bins, rows, K, dtype=torch.float64)
        t[:, torch.arange(rows), torch.arange(rows) % K] = sign(bins, rows)
        return t

    def two_level(rows, dens):
        v = 256.0 * torch.randint(-3, 4, (bins, rows, K), generator=gen) + torch.randint(-3, 4, (bins, rows, K), generator=gen)
        return v.double() * (torch.rand(bins, rows, K, generator=gen) < dens)
    if name == "a24_onehot":
        return big(M), onehot(N)
    if name == "onehot_b24":
        return onehot(M), big(N)
    assert name == "a2b2"
    return two_level(M, 0.25), two_level(N, 0.25)


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
