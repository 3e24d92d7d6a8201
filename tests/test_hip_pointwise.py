"""The BatchNorm and elementwise kernels of csrc/pointwise.hip, called through gdn_amd.ops, against the float64 restatement
in tests/pointwise_fp64.py (BatchNorm, tanh') or bit for bit against IEEE float32 on the CPU (everything that is one
operation plus at most one round-to-nearest-even store).

    entry point                   test
    ----------------------------  ------------------------------------------------------------------------
    gdn_bn_apply                  test_bn_apply, test_bn_dyadic_relu_ties, test_bn_training_shapes
    gdn_bn_bwd                    test_bn_bwd, test_bn_bwd_external_partial, test_bn_dyadic_relu_ties, test_bn_training_shapes,
                                  test_bn_bwd_more_channel_vectors_than_lanes
    gdn_bn_bwd_coeffs             test_bn_bwd (k1, k2), test_bn_bwd_external_partial
    gdn_bn_eval_bwd               test_bn_eval_bwd (relu 0 / 1 / 2), test_bn_dyadic_relu_ties
    gdn_bn_finalize_train         supplies the coefficients of all of the above from fp32 partial sums
    gdn_add                       test_add (sizes x the eight dtype masks)
    gdn_add_pitched               test_add_pitched, test_add_pitched_sliced_output, test_copy_rows
    gdn_cast                      test_cast, test_cast_edge_values
    gdn_scale_dev                 test_scale_dev
    gdn_fill                      test_fill_and_zeros
    gdn_tanh_bwd                  test_tanh_bwd
    gdn_nchw_to_nhwc / _to_nchw   test_layout_converting
    gdn_transpose_taps            test_transpose_taps_converting

BatchNorm bars (EPS = 2^-24, one fp32 rounding):
  bn_apply, bn_eval_bwd   <= 3 roundings per element: 2 ulp of the OUTPUT dtype against the float64 result rounded once to
      that dtype, + 1 ulp where a bf16 result lies on a rounding boundary (pointwise_fp64.ulp_bar, the one place that
      rule lives).  A bf16 result must also lie within half a bf16 ulp + 3 EPS * (|y*scale| + |shift| + |residual|) of
      the unrounded float64 value (one rounding to bf16 of an fp32 value that is 3 roundings off at most).
      The ulp bar is relative to the RESULT, so it presumes no cancellation between rounded operands: y*scale + shift is
      one fused multiply-add in the build (one rounding, whatever the operands), and the residual of the continuous
      cases is drawn with the sign of the value it is added to.  The dyadic cases (exact arithmetic) add residuals of
      either sign.
  bn_bwd sums   dgamma, dbeta, k1, k2 are fp32 sums of `terms` = ceil(ceil(npix / grid) / pixel lanes) terms per lane,
      then float64: |err| <= (terms + 4) * EPS * sum |term| per channel, sum |term| from the float64 reference
      (+ the terms of ReLU-ambiguous elements, which may fall on either side of the mask).
  bn_bwd dy     the propagated bound: |scale| * (EPS * (3 (|dz| + |k1|) + 5 |xhat * k2|) + err(k1) + |xhat| * err(k2)),
      + half a bf16 ulp when dy is stored as bf16.
  ReLU mask     a pre-activation within 4 EPS * (|y*scale| + |shift|) of zero is ambiguous: excluded, and the excluded
      share is asserted <= 5e-4 first.  test_bn_dyadic_relu_ties has exact zeros and excludes nothing.
Worst errors observed on an MI355X (also in DESIGN.md 4.1): bn_apply 1 ulp (fp32 and bf16), bn_eval_bwd 0 ulp fp32 / 1 ulp
bf16; bn_bwd sums 0.56 of the bound at 280 pixels and 0.11 at 20 x 128 x 416, fp32 dy 0.62 of its bound; excluded ReLU share
<= 3.0e-4; tanh_bwd 1 ulp; everything elementwise bit-identical.
"""
import numpy as np
import pytest
import torch

import pointwise_fp64 as R

pytestmark = pytest.mark.gpu

EPS = R.EPS32
MAX_EXCLUDED = 5e-4
BN_CHANNELS = [4, 12, 24, 64, 68, 136, 512]       # C/4, C/8 power of two or not; C % 8 != 0 (bf16 falls back to 4-wide)
SMALL_SHAPES = [(2, 10, 14), (3, 7, 5)]           # 280 pixels; 105 pixels (fewer than the pixel lanes of a reduce block)
SLICES = [None, (4, 12), (8, 16)]                 # (c0, extra width): multiples of 4 but not 8 / multiples of 8
BNB_MAXBLK = 1024


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _report(what, value):
    print("FIGURE %-58s %.4g" % (what, value))


def _ratio(err, bound):
    """err / bound with 0 / 0 = 0 (an exact result under a zero bound)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))


def _dt(t):
    return R.BF16 if t.dtype == torch.bfloat16 else R.F32


def _store(x, bf16):
    return x.bfloat16() if bf16 else x.float()


def _place(t, gpu, sl, fill=0.0):
    """t on the device: dense (sl None) or as the channel slice [c0, c0 + C) of a buffer `extra` channels wider that is
    filled with `fill` elsewhere.  Returns (tensor handed to the kernel, the wider buffer or None)."""
    if sl is None:
        return t.to(gpu), None
    c0, extra = sl
    C = t.shape[-1]
    buf = torch.full(t.shape[:-1] + (C + extra,), fill, dtype=t.dtype).to(gpu)
    view = buf[..., c0:c0 + C]
    view.copy_(t.to(gpu))
    return view, buf


def _untouched(buf, sl, C, fill, what):
    c0, _ = sl
    b = buf.cpu().float()
    assert bool((b[..., :c0] == fill).all()) and bool((b[..., c0 + C:] == fill).all()), what + ": wrote outside its channel slice"


def _coeffs(gpu, y, gamma, beta):
    """[scale, shift, mean, invstd] from gdn_bn_finalize_train on fp32 partial sums of y as it is stored."""
    from gdn_amd import ops
    C = y.shape[-1]
    flat = y.float().reshape(-1, C)
    npix = flat.shape[0]
    if npix % 4096 == 0:
        ch = flat.view(npix // 4096, 4096, C)
        st = torch.stack((ch.sum(1), (ch * ch).sum(1)), 1).contiguous()
    else:
        st = torch.stack([torch.stack((c.sum(0), (c * c).sum(0))) for c in flat.split(37)]).contiguous()
    co = ops.bn_finalize_train(st.to(gpu), npix, gamma.to(gpu), beta.to(gpu), None, None)
    return co, co.cpu()


def _bn_inputs(shape, C, seed, bf16_y):
    g = _gen(seed)
    B, H, W = shape
    y = _store(torch.randn(B, H, W, C, generator=g) * 2 + 0.7, bf16_y)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    return y, gamma, beta, g


def _dout(y, g):
    """Upstream gradient with a positive mean and a positive correlation with y, so that neither sum cancels."""
    u = torch.rand(y.shape, generator=g) * 2 - 1
    return 0.5 * u + 0.5 + 0.125 * (y.float() - 0.7)


def _check_out(got, ref, mag, what, keep=None):
    """The 2-ulp bar of the module docstring on `got` (its dtype decides the unit), and for bf16 the tight bound."""
    dt = _dt(got)
    u = R.ulps_off(got.float(), ref, dt)
    bar = R.ulp_bar(ref, dt, 2)
    err = np.abs(R.f64(got.float()) - ref)
    tight = 3 * EPS * mag + (0.5 * R.ulp(ref, R.BF16) if dt == R.BF16 else np.inf)
    if keep is not None:
        u, bar, err, tight = u[keep], bar[keep], err[keep], np.broadcast_to(tight, err.shape)[keep]
    _report(what + " worst ulps (%s)" % dt, float(u.max()))
    assert not (u > bar).any(), "%s: %d elements over 2 ulp (+1 on a bf16 boundary), worst %.2f" % (what, int((u > bar).sum()), float(u.max()))
    assert not (err > tight).any(), "%s: %d bf16 elements beyond half an ulp + 3 EPS" % (what, int((err > tight).sum()))


def _excluded_ok(amb, what):
    share = float(amb.mean())
    _report(what + " excluded share", share)
    assert share <= MAX_EXCLUDED, "%s: %.3e of the elements are ReLU-ambiguous (cap %.1e)" % (what, share, MAX_EXCLUDED)
    return ~amb


# --------------------------------------------------------------------------------------------------------- bn_apply
# dtype of (y, residual, out): all fp32; all bf16; fp32 y with a bf16 out_dtype (+ bf16 residual): engine.py conv_bn
APPLY_DTYPES = {"f32": (0, 0, 0), "bf16": (1, 1, 1), "f32y-bf16out": (0, 1, 1), "bf16y-f32out": (1, 0, 0)}


def _apply_case(gpu, C, shape, dts, relu, res, sl_y, sl_r, sl_o, seed, what):
    from gdn_amd import ops
    y, gamma, beta, g = _bn_inputs(shape, C, seed, dts[0])
    co, coc = _coeffs(gpu, y, gamma, beta)
    pre = R.bn_preact(y, coc[0], coc[1])
    r = None
    if res:
        # the sign of the value it is added to (module docstring): no cancellation between rounded operands
        sgn = np.ones(pre.shape) if relu else np.where(pre < 0, -1.0, 1.0)
        r = _store((torch.rand(y.shape, generator=g) + 0.25) * torch.from_numpy(sgn).float(), dts[1])
    yv, _ = _place(y, gpu, sl_y)
    rv = None if r is None else _place(r, gpu, sl_r)[0]
    odt = torch.bfloat16 if dts[2] else torch.float32
    if sl_o is None:
        o = ops.bn_apply(yv, co[0], co[1], relu, rv, out_dtype=odt)
    else:
        o, obuf = _place(torch.zeros(y.shape, dtype=odt), gpu, sl_o, fill=-7.0)
        assert ops.bn_apply(yv, co[0], co[1], relu, rv, out=o) is o
        _untouched(obuf, sl_o, C, -7.0, what)
    ref = R.bn_apply(y, coc[0], coc[1], relu, r)
    mag = np.abs(R.f64(y) * R.f64(coc[0])) + np.abs(R.f64(coc[1])) + (0.0 if r is None else np.abs(R.f64(r)))
    _check_out(o.cpu(), ref, mag, what)


@pytest.mark.parametrize("dtypes", list(APPLY_DTYPES))
@pytest.mark.parametrize("C", BN_CHANNELS)
def test_bn_apply(gpu, C, dtypes):
    dts = APPLY_DTYPES[dtypes]
    seed = 1000
    for shape in SMALL_SHAPES:
        for relu, res in ((False, False), (True, False), (False, True), (True, True)):
            # dense, then each operand in turn as a channel slice (both alignments), the output included
            pitches = [(None, None, None)] + [(s, None, None) for s in SLICES[1:]] + [(None, None, s) for s in SLICES[1:]]
            if res:
                pitches += [(None, s, None) for s in SLICES[1:]] + [(SLICES[1], SLICES[2], SLICES[1])]
            for sl_y, sl_r, sl_o in pitches:
                seed += 1
                what = "bn_apply C%d %s %s relu%d res%d pitch(y%s r%s o%s)" % (C, "x".join(map(str, shape)), dtypes, relu, res,
                                                                              sl_y, sl_r, sl_o)
                _apply_case(gpu, C, shape, dts, relu, res, sl_y, sl_r, sl_o, seed, what)


# -------------------------------------------------------------------------------------------------- bn_bwd / coeffs
# dtype of (dout, y, dy): all fp32; all bf16; bf16 dout with fp32 y / dy (an fp32 layer of a bf16 model); bf16 dout / y, fp32 dy
BWD_DTYPES = {"f32": (0, 0, 0), "bf16": (1, 1, 1), "bf16dout-f32": (1, 0, 0), "bf16-f32dy": (1, 1, 0)}


def _terms_per_lane(npix, C):
    nblk = min(max(-(-npix // 64), 1), BNB_MAXBLK)
    per = -(-npix // nblk)
    lanes = 256 // min(C // 4, 256)
    return -(-per // lanes)


def _sum_bounds(b, amb, dout, terms):
    """(err dbeta, err dgamma) per channel: (terms + 4) * EPS * sum |term|, plus the terms of ReLU-ambiguous elements."""
    C = b["dz"].shape[-1]
    e1, e2 = (terms + 4) * EPS * b["abs1"], (terms + 4) * EPS * b["abs2"]
    if amb is not None and amb.any():
        a = np.where(amb, np.abs(R.f64(dout)), 0.0)
        e1 = e1 + a.reshape(-1, C).sum(0)
        e2 = e2 + (a * np.abs(b["xhat"])).reshape(-1, C).sum(0)
    return e1, e2


def _check_vec(got, ref, bound, what):
    err = np.abs(R.f64(got) - ref)
    # no looser than tests/test_hip_kernels.py::test_batchnorm_train_fwd_bwd: 1e-4 of the largest + 2e-3 relative
    old = 1e-4 * np.abs(ref).max() + 2e-3 * np.abs(ref)
    assert (bound <= old).all(), "%s: derived bound looser than the existing bar" % what
    _report(what + " worst err/bound", float(_ratio(err, bound).max()))
    assert (err <= bound).all(), "%s: worst err/bound %.3g" % (what, float(_ratio(err, bound).max()))


def _check_dy(dy, b, scale, e1, e2, keep, what):
    n = b["n"]
    s = np.abs(R.f64(scale))
    p = np.abs(b["xhat"] * b["k2"])
    bound = s * (EPS * (3 * (np.abs(b["dz"]) + np.abs(b["k1"])) + 5 * p) + (e1 + EPS * np.abs(b["dbeta"])) / n
                 + np.abs(b["xhat"]) * (e2 + EPS * np.abs(b["dgamma"])) / n)
    if dy.dtype == torch.bfloat16:
        bound = bound + 0.5 * R.ulp(b["dy"], R.BF16)
    err = np.abs(R.f64(dy.float()) - b["dy"])
    # no looser than tests/test_hip_kernels.py::test_batchnorm_train_fwd_bwd on an fp32 dy (1e-4 of the largest + 1e-3 relative)
    assert dy.dtype == torch.bfloat16 or (bound <= 1e-4 * np.abs(b["dy"]).max() + 1e-3 * np.abs(b["dy"])).all(), \
        what + ": derived dy bound looser than the existing bar"
    if keep is not None:
        err, bound = err[keep], bound[keep]
    _report(what + " dy worst err/bound", float(_ratio(err, bound).max()))
    assert (err <= bound).all(), "%s: dy %d elements over the bound, worst err/bound %.3g" % (
        what, int((err > bound).sum()), float(_ratio(err, bound).max()))


def _bwd_case(gpu, C, shape, dts, relu, sl_d, sl_y, seed, what, with_grads=True):
    from gdn_amd import ops
    y, gamma, beta, g = _bn_inputs(shape, C, seed, dts[1])
    dout = _store(_dout(y, g), dts[0])
    co, coc = _coeffs(gpu, y, gamma, beta)
    dv, yv = _place(dout, gpu, sl_d)[0], _place(y, gpu, sl_y)[0]
    odt = torch.bfloat16 if dts[2] else torch.float32
    dg, db = (torch.full((C,), float("nan"), device=gpu) for _ in range(2))
    dy = ops.bn_bwd(dv, yv, gamma.to(gpu), co, relu, dg if with_grads else None, db if with_grads else None, out_dtype=odt)
    assert dy.dtype == odt
    b = R.bn_train_bwd(dout, y, coc[0], coc[1], coc[2], coc[3], relu)
    amb = keep = None
    if relu:
        amb = R.bn_relu_ambiguous(y, coc[0], coc[1])
        keep = _excluded_ok(amb, what)                                                     # asserted FIRST
    e1, e2 = _sum_bounds(b, amb, dout, _terms_per_lane(b["n"], C))
    if with_grads:
        _check_vec(db.cpu(), b["dbeta"], e1 + EPS * np.abs(b["dbeta"]), what + " dbeta")
        _check_vec(dg.cpu(), b["dgamma"], e2 + EPS * np.abs(b["dgamma"]), what + " dgamma")
    _check_dy(dy.cpu(), b, coc[0], e1, e2, keep, what)
    return dv, yv, co, dy, b, e1, e2


@pytest.mark.parametrize("dtypes", list(BWD_DTYPES))
@pytest.mark.parametrize("C", BN_CHANNELS)
def test_bn_bwd(gpu, C, dtypes):
    from gdn_amd import ops
    dts = BWD_DTYPES[dtypes]
    seed = 2000
    for shape in SMALL_SHAPES:
        for relu in (False, True):
            for sl_d, sl_y in [(None, None)] + [(s, None) for s in SLICES[1:]] + [(None, s) for s in SLICES[1:]] + [(SLICES[2], SLICES[1])]:
                seed += 1
                what = "bn_bwd C%d %s %s relu%d pitch(d%s y%s)" % (C, "x".join(map(str, shape)), dtypes, relu, sl_d, sl_y)
                dv, yv, co, dy, b, e1, e2 = _bwd_case(gpu, C, shape, dts, relu, sl_d, sl_y, seed, what)
                if sl_d is None and sl_y is None:
                    # dgamma / dbeta = None: the same dy, bit for bit
                    dy2 = ops.bn_bwd(dv, yv, None, co, relu, None, None, out_dtype=dy.dtype)
                    assert torch.equal(dy2.cpu(), dy.cpu()), what + ": dy differs without dgamma / dbeta"
                # passes 1 + 2 alone: k1, k2 (and the parameter gradients again)
                dg, db = (torch.full((C,), float("nan"), device=gpu) for _ in range(2))
                kk = ops.bn_bwd_coeffs(dv, yv, co, relu, dg, db).cpu()
                n = b["n"]
                _check_vec(kk[0], b["k1"], (e1 + 2 * EPS * np.abs(b["dbeta"])) / n, what + " k1")
                _check_vec(kk[1], b["k2"], (e2 + 2 * EPS * np.abs(b["dgamma"])) / n, what + " k2")
                _check_vec(db.cpu(), b["dbeta"], e1 + EPS * np.abs(b["dbeta"]), what + " coeffs dbeta")
                _check_vec(dg.cpu(), b["dgamma"], e2 + EPS * np.abs(b["dgamma"]), what + " coeffs dgamma")


@pytest.mark.parametrize("dtypes", ["f32", "bf16"])
def test_bn_bwd_more_channel_vectors_than_lanes(gpu, dtypes):
    """C = 1040: 260 channel quads for the 256 channel lanes of a pass-1 block (4-channel lanes for bf16 too), so the kernel's
    channel loop runs twice and only 4 lanes have a quad in the second trip; every lane must still reach the barriers of the
    LDS sum.  One pixel lane per channel lane, 105 pixels in two blocks.  Pass 3 splits its flat index by 260 quads (fp32)
    or 130 eight-channel vectors (bf16), neither a power of two."""
    C, shape = 1040, (3, 7, 5)
    assert C // 4 > 256 and (C // 4) % 256 == 4
    for relu in (False, True):
        what = "bn_bwd C%d %s %s relu%d" % (C, "x".join(map(str, shape)), dtypes, relu)
        _bwd_case(gpu, C, shape, BWD_DTYPES[dtypes], relu, None, None, 2900 + relu, what)


@pytest.mark.parametrize("slots", [1, 37, 1500])
@pytest.mark.parametrize("C,dtypes", [(12, "f32"), (64, "bf16"), (136, "bf16dout-f32")])
def test_bn_bwd_external_partial(gpu, C, dtypes, slots):
    """partial = [slots, 2, C] computed outside (as a convolution backward's epilogue would): the float64 reference's
    per-pixel terms cut into `slots` groups of pixels, each summed in float64 and rounded to fp32."""
    from gdn_amd import ops
    dts = BWD_DTYPES[dtypes]
    shape, relu = (2, 10, 14), True
    what = "bn_bwd ext partial C%d %s slots%d" % (C, dtypes, slots)
    y, gamma, beta, g = _bn_inputs(shape, C, 3000 + slots, dts[1])
    dout = _store(_dout(y, g), dts[0])
    co, coc = _coeffs(gpu, y, gamma, beta)
    b = R.bn_train_bwd(dout, y, coc[0], coc[1], coc[2], coc[3], relu)
    keep = _excluded_ok(R.bn_relu_ambiguous(y, coc[0], coc[1]), what)
    t1, t2 = b["dz"].reshape(-1, C), (b["dz"] * b["xhat"]).reshape(-1, C)
    cuts = np.array_split(np.arange(t1.shape[0]), slots)
    part = np.stack([np.stack((t1[i].sum(0), t2[i].sum(0))) for i in cuts]).astype(np.float32)        # [slots, 2, C]
    pd = torch.from_numpy(part).to(gpu)
    # the slots are exact up to their own rounding: err <= EPS * sum |slot| (the sum over slots is float64)
    e1, e2 = EPS * np.abs(part[:, 0].astype(np.float64)).sum(0), EPS * np.abs(part[:, 1].astype(np.float64)).sum(0)
    dg, db = (torch.full((C,), float("nan"), device=gpu) for _ in range(2))
    odt = torch.bfloat16 if dts[2] else torch.float32
    dy = ops.bn_bwd(dout.to(gpu), y.to(gpu), gamma.to(gpu), co, relu, dg, db, out_dtype=odt, partial=pd)
    _check_vec(db.cpu(), b["dbeta"], e1 + EPS * np.abs(b["dbeta"]), what + " dbeta")
    _check_vec(dg.cpu(), b["dgamma"], e2 + EPS * np.abs(b["dgamma"]), what + " dgamma")
    _check_dy(dy.cpu(), b, coc[0], e1, e2, keep, what)
    dg2, db2 = (torch.full((C,), float("nan"), device=gpu) for _ in range(2))
    kk = ops.bn_bwd_coeffs(dout.to(gpu), y.to(gpu), co, relu, dg2, db2, partial=pd).cpu()
    assert torch.equal(dg2.cpu(), dg.cpu()) and torch.equal(db2.cpu(), db.cpu())
    _check_vec(kk[0], b["k1"], (e1 + 2 * EPS * np.abs(b["dbeta"])) / b["n"], what + " k1")
    _check_vec(kk[1], b["k2"], (e2 + 2 * EPS * np.abs(b["dgamma"])) / b["n"], what + " k2")


# ------------------------------------------------------------------------------------------------------ bn_eval_bwd
@pytest.mark.parametrize("dtypes", list(BWD_DTYPES))
@pytest.mark.parametrize("C", BN_CHANNELS)
def test_bn_eval_bwd(gpu, C, dtypes):
    from gdn_amd import ops
    dts = BWD_DTYPES[dtypes]
    seed = 4000
    for shape in SMALL_SHAPES:
        for relu in (0, 1, 2):
            for sl_d, sl_y in [(None, None), (SLICES[1], None), (None, SLICES[2]), (SLICES[2], SLICES[1])]:
                seed += 1
                what = "bn_eval_bwd C%d %s %s relu%d pitch(d%s y%s)" % (C, "x".join(map(str, shape)), dtypes, relu, sl_d, sl_y)
                y, gamma, beta, g = _bn_inputs(shape, C, seed, dts[1])
                co, coc = _coeffs(gpu, y, gamma, beta)
                keep = None
                if relu == 2:      # y is the ACTIVATED output of a fused epilogue, stored in y's dtype
                    y = _store(torch.from_numpy(R.round_to(R.bn_apply(y, coc[0], coc[1], True), _dt(y))).float(), dts[1])
                elif relu == 1:
                    keep = _excluded_ok(R.bn_relu_ambiguous(y, coc[0], coc[1]), what)       # asserted FIRST
                dout = _store(_dout(y, g), dts[0])
                dy = ops.bn_eval_bwd(_place(dout, gpu, sl_d)[0], _place(y, gpu, sl_y)[0], co, relu,
                                     out_dtype=torch.bfloat16 if dts[2] else torch.float32)
                ref = R.bn_eval_bwd(dout, y, coc[0], coc[1], relu)
                _check_out(dy.cpu(), ref, np.abs(ref), what, keep=keep)


# --------------------------------------------------------------------------------------- exact ties of the ReLU mask
@pytest.mark.parametrize("dtypes", ["f32", "bf16"])
@pytest.mark.parametrize("C", [12, 64])
def test_bn_dyadic_relu_ties(gpu, C, dtypes):
    """Dyadic y, scale, shift (and mean, invstd, dout, residual): the pre-activation is exact in fp32 and is exactly zero
    on about a tenth of the elements.  Convention: gradient 0 AT 0 (`> 0`, as torch).  Nothing is excluded, and because
    y * scale + shift is exact the forward must equal the float64 result bit for bit, residuals of either sign included."""
    from gdn_amd import ops
    bf = dtypes == "bf16"
    g = _gen(5000 + C)
    q = lambda shape, den: torch.randint(-4, 5, shape, generator=g).float() / den
    shape = (2, 10, 14, C)
    y, dout, res = (_store(q(shape, 4), bf) for _ in range(3))
    scale = torch.tensor([0.5, -0.5, 1.0, 2.0]).repeat(C // 4)
    shift, mean, invstd = q((C,), 4), q((C,), 4), torch.tensor([1.0, 0.5, 2.0, 1.0]).repeat(C // 4)
    coc = torch.stack((scale, shift, mean, invstd))
    co = coc.to(gpu)
    pre = R.bn_preact(y, scale, shift)
    assert 0.03 < float((pre == 0).mean()) < 0.3
    odt = torch.bfloat16 if bf else torch.float32
    for relu in (False, True):
        o = ops.bn_apply(y.to(gpu), co[0], co[1], relu, res.to(gpu), out_dtype=odt)
        assert np.array_equal(R.f64(o.float()), R.round_to(R.bn_apply(y, scale, shift, relu, res), _dt(o))), "bn_apply dyadic relu%d" % relu
    for mode in (1, 2):
        yy = y if mode == 1 else _store(torch.from_numpy(np.maximum(pre, 0.0)).float(), bf)      # (exact in bf16: k/8, |k| <= 24)
        dy = ops.bn_eval_bwd(dout.to(gpu), yy.to(gpu), co, mode, out_dtype=odt)
        assert np.array_equal(R.f64(dy.float()), R.round_to(R.bn_eval_bwd(dout, yy, scale, shift, mode), _dt(dy))), "bn_eval_bwd dyadic relu%d" % mode
    what = "bn_bwd dyadic C%d %s" % (C, dtypes)
    dg, db = (torch.full((C,), float("nan"), device=gpu) for _ in range(2))
    dy = ops.bn_bwd(dout.to(gpu), y.to(gpu), None, co, True, dg, db, out_dtype=odt)
    b = R.bn_train_bwd(dout, y, scale, shift, mean, invstd, True)
    # every term is a multiple of 2^-5 of magnitude <= 4 and there are 280 of them: the fp32 sums are exact in any order
    assert np.array_equal(R.f64(db.cpu()), b["dbeta"]) and np.array_equal(R.f64(dg.cpu()), b["dgamma"]), what + ": sums not exact"
    zero = np.zeros(C)
    _check_dy(dy.cpu(), b, scale, zero, zero, None, what)                                   # nothing excluded


# ------------------------------------------------------------------------------------------ the training-step tensors
@pytest.mark.parametrize("shape,dtypes", [((20, 32, 104), "f32"), ((20, 32, 104), "bf16"), ((20, 33, 104), "f32"),
                                          ((20, 128, 416), "f32"), ((20, 128, 416), "bf16")],
                         ids=["66560px-f32", "66560px-bf16", "68640px-f32", "step-f32", "step-bf16"])
def test_bn_training_shapes(gpu, shape, dtypes):
    """C = 64.  66 560 pixels (with a residual): the stream_blocks cap (2048 blocks) and the BNB_MAXBLK cap (1024 blocks)
    are both hit; 66 560 is 65 * 1024, so 68 640 pixels are added, which the reduce grid does not divide (the last blocks
    get a short or an empty range).  20 x 128 x 416: the first-level tensors of the benchmark step (conv + BN + ReLU, no
    residual), 273 MB each in fp32."""
    C = 64
    dts_a, dts_b = APPLY_DTYPES[dtypes], BWD_DTYPES[dtypes]
    what = "training shape %s %s" % ("x".join(map(str, shape)), dtypes)
    npix = shape[0] * shape[1] * shape[2]
    assert -(-npix // 64) > BNB_MAXBLK and npix * (C // 8) > 2048 * 256 and (shape[1] != 33 or npix % BNB_MAXBLK)
    _apply_case(gpu, C, shape, dts_a, True, shape[1] == 32, None, None, None, 6000, what + " bn_apply")
    torch.cuda.empty_cache()
    _bwd_case(gpu, C, shape, dts_b, True, None, None, 6001, what + " bn_bwd")
    torch.cuda.empty_cache()


# ===================================================================================================== elementwise
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025]
ADD_CAP, CAST_CAP, SCALAR_CAP = 4 * 256 * 2048, 4 * 256 * 4096, 256 * 2048      # elements one pass of each capped grid covers


def _over(cap):
    n = cap + 4 * 100 + 3
    assert n % 4 == 3
    return n


def _rand(shape, seed, bf16=False):
    return _store(torch.randn(shape, generator=_gen(seed)) * 3, bf16)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert torch.equal(_bits(got.cpu().contiguous()), _bits(want.contiguous())), what + ": not bit-identical to IEEE float32 on the CPU"


def _out(x32, bf16):
    """The fp32 result, stored: one round-to-nearest-even when the output is bf16."""
    return x32.bfloat16() if bf16 else x32


@pytest.mark.parametrize("mask", list(range(8)))
def test_add(gpu, mask):
    from gdn_amd import ops
    for n in SIZES + [_over(ADD_CAP)]:
        a, b = _rand((n,), 7000 + n, mask & 1), _rand((n,), 7001 + n, mask & 2)
        o = ops.add(a.to(gpu), b.to(gpu), out_dtype=torch.bfloat16 if mask & 4 else torch.float32)
        _same_bits(o, _out(a.float() + b.float(), mask & 4), "add n=%d mask=%d" % (n, mask))


@pytest.mark.parametrize("mask", list(range(8)))
def test_add_pitched(gpu, mask):
    from gdn_amd import ops
    odt = torch.bfloat16 if mask & 4 else torch.float32
    seed = 7100
    for C in (4, 12, 64, 136):
        for shape in SMALL_SHAPES:
            for sl_a, sl_b in [(None, None), (SLICES[1], None), (None, SLICES[2]), (SLICES[2], SLICES[1])]:
                seed += 1
                a, b = _rand(shape + (C,), seed, mask & 1), _rand(shape + (C,), seed + 500, mask & 2)
                av, bv = _place(a, gpu, sl_a, 99.0)[0], _place(b, gpu, sl_b, 99.0)[0]
                what = "add_pitched C%d %s mask%d a%s b%s" % (C, shape, mask, sl_a, sl_b)
                _same_bits(ops.add_pitched(av, bv, out_dtype=odt), _out(a.float() + b.float(), mask & 4), what)
                if not mask & 2:        # b = None: the compacting copy (mask bit 1 has no operand then)
                    _same_bits(ops.add_pitched(av, None, out_dtype=odt), _out(a.float(), mask & 4), what + " copy")
    # one tensor above the launch cap of 2048 blocks x 256 lanes (x 4 channels)
    a, b = _rand((1, 40, 800, 68), 7198, mask & 1), _rand((1, 40, 800, 68), 7199, mask & 2)
    assert a.numel() // 4 > 256 * 2048
    _same_bits(ops.add_pitched(_place(a, gpu, SLICES[1])[0], b.to(gpu), out_dtype=odt), _out(a.float() + b.float(), mask & 4),
               "add_pitched above the cap mask%d" % mask)


@pytest.mark.parametrize("mask", [0, 5, 7])
def test_add_pitched_sliced_output(gpu, mask):
    """The C ABI takes a pitched output (ops.add_pitched always makes a dense one): out is a channel slice of a wider buffer
    filled with a sentinel, and the channels outside the slice must come back untouched."""
    from gdn_amd import ops
    from gdn_amd._lib import lib
    C, shape = 12, (3, 7, 5)
    odt = torch.bfloat16 if mask & 4 else torch.float32
    for sl in SLICES[1:]:
        a, b = _rand(shape + (C,), 7200, mask & 1), _rand(shape + (C,), 7201, mask & 2)
        av, bv = _place(a, gpu, SLICES[2])[0], b.to(gpu)
        o, obuf = _place(torch.zeros(shape + (C,), dtype=odt), gpu, sl, fill=-7.0)
        lib.gdn_add_pitched(av.data_ptr(), av.stride(-2), bv.data_ptr(), bv.stride(-2), o.data_ptr(), o.stride(-2),
                            3 * 7 * 5, C, mask, ops.stream())
        _same_bits(o.contiguous(), _out(a.float() + b.float(), mask & 4), "add_pitched sliced out %s" % (sl,))
        _untouched(obuf, sl, C, -7.0, "add_pitched sliced out %s" % (sl,))


def test_copy_rows(gpu):
    """As trainer.py stacks two batches: copy_rows(a, out[:B]); copy_rows(b, out[B:])."""
    from gdn_amd import ops
    for shape in ((2, 1, 16, 24), (3, 3, 5, 8), (1, 1, 2100, 1000)):      # the last: above the launch cap (2048 x 256 quads)
        B = shape[0]
        a, b = _rand(shape, 7300), _rand(shape, 7301)
        out = torch.full((2 * B,) + shape[1:], -7.0, device=gpu)
        ops.copy_rows(a.to(gpu), out[:B])
        assert bool((out[B:] == -7.0).all().cpu()), "copy_rows wrote past its half"
        ops.copy_rows(b.to(gpu), out[B:])
        _same_bits(out, torch.cat((a, b)), "copy_rows %s" % (shape,))


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
def test_cast(gpu, mask):
    from gdn_amd import ops
    ddt = torch.bfloat16 if mask & 2 else torch.float32
    for n in SIZES + [_over(CAST_CAP)]:
        src = _rand((n,), 7400 + n, mask & 1)
        _same_bits(ops.cast(src.to(gpu), ddt), src.to(ddt), "cast n=%d mask=%d" % (n, mask))
        dst = torch.empty(n, dtype=ddt, device=gpu)
        assert ops.cast(src.to(gpu), out=dst) is dst
        _same_bits(dst, src.to(ddt), "cast out= n=%d mask=%d" % (n, mask))


def test_cast_edge_values(gpu):
    """fp32 -> bf16, round to nearest even, on hand-built bit patterns (NaN is out of contract: common.h)."""
    from gdn_amd import ops
    pos = [0x00000000, 0x7F800000,      # 0, inf
           0x7F7FFFFF,                  # the largest finite float: rounds to inf
           0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000,      # largest bf16; just below the tie to inf; the tie (to even = inf)
           0x3F808000, 0x3F818000,      # exact ties: below an even neighbour (down to 0x3F80), below an odd one (up to 0x3F82)
           0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,      # one below / one above those ties
           0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF,      # fp32 subnormals, ties among them
           0x00800000, 0x00808000, 0x00FFFFFF,      # the smallest bf16 normal and its neighbourhood
           0x3F800000, 0x40490FDB]
    bits = np.array(pos + [p | 0x80000000 for p in pos], dtype=np.uint32)
    src = torch.from_numpy(bits.view(np.float32).copy())
    assert src.numel() % 4 == 2 and not bool(torch.isnan(src).any())           # vector body and scalar tail both used
    got = ops.cast(src.to(gpu), torch.bfloat16).cpu()
    want = R.round_bf16(src.double().numpy())
    assert np.array_equal(got.double().numpy(), want) and np.array_equal(np.signbit(got.double().numpy()), np.signbit(want))
    _same_bits(got, src.bfloat16(), "cast edge values")
    wb = (_bits(got).numpy().astype(np.int64) & 0xFFFF)[:len(pos)]
    assert list(wb[:3]) == [0x0000, 0x7F80, 0x7F80] and list(wb[3:6]) == [0x7F7F, 0x7F7F, 0x7F80]
    assert list(wb[6:12]) == [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0x3F81, 0x3F82]
    assert list(wb[12:18]) == [0x0000, 0x0000, 0x0000, 0x0001, 0x0002, 0x0080] and list(wb[18:21]) == [0x0080, 0x0080, 0x0100]
    back = ops.cast(got.to(gpu), torch.float32)                                 # bf16 -> fp32 is exact
    _same_bits(back, got.float(), "cast bf16 -> fp32 edge values")


def test_scale_dev(gpu):
    from gdn_amd import ops
    s = torch.tensor(0.7310586)
    for n in SIZES + [_over(SCALAR_CAP)]:
        x = _rand((n,), 7500 + n)
        _same_bits(ops.scale_dev(x.to(gpu), s.to(gpu)), x * s, "scale_dev n=%d" % n)
        assert np.array_equal(R.f64(x * s), R.round_to(R.scale(x, s), R.F32))


def test_fill_and_zeros(gpu):
    from gdn_amd import ops
    for n in SIZES + [_over(SCALAR_CAP)]:
        t = torch.full((n,), float("nan"), device=gpu)
        assert ops.fill_(t, 0.1) is t
        _same_bits(t, torch.full((n,), 0.1), "fill n=%d" % n)
        _same_bits(ops.zeros((n,), gpu), torch.zeros(n), "zeros n=%d" % n)
    _same_bits(ops.fill_(torch.empty((), device=gpu), 1.0), torch.tensor(1.0), "fill 0-dim")


def test_tanh_bwd(gpu):
    """d * (1 - o*o): the compiler may or may not contract 1 - o*o to an fma, so the comparison is with float64 at 2 ulp
    (one rounding for the fused form of 1 - o*o, one for the product) -- o includes +-1 exactly and values within 2^-12
    of +-1, where an unfused 1 - o*o would lose most of its bits."""
    from gdn_amd import ops
    g = _gen(7600)
    worst = 0.0
    for n in SIZES + [_over(SCALAR_CAP)]:
        o = torch.tanh(torch.randn(n, generator=g) * 2)
        edge = 1.0 - torch.rand(n, generator=g) * 2.0 ** -12
        pick = torch.randint(0, 4, (n,), generator=g)
        o = torch.where(pick == 0, edge, torch.where(pick == 1, -edge, o))
        o[::5] = 1.0
        o[2::7] = -1.0
        d = torch.randn(n, generator=g)
        got = ops.tanh_bwd(d.to(gpu), o.to(gpu)).cpu()
        u = R.ulps_off(got, R.tanh_bwd(d, o), R.F32)
        worst = max(worst, float(u.max()))
        assert (u <= 2).all(), "tanh_bwd n=%d: worst %.1f ulp" % (n, float(u.max()))
    _report("tanh_bwd worst ulps", worst)


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
def test_layout_converting(gpu, mask):
    from gdn_amd import ops
    ddt = torch.bfloat16 if mask & 2 else torch.float32
    for shape in ((2, 3, 5, 7), (1, 1, 1, 1), (3, 8, 1, 9), (2, 5, 300, 181)):       # the last: above the launch cap
        x = _rand(shape, 7700 + shape[1], mask & 1)                                  # NCHW
        nhwc = x.permute(0, 2, 3, 1).contiguous()
        _same_bits(ops.nchw_to_nhwc(x.to(gpu), dtype=ddt), nhwc.to(ddt), "nchw_to_nhwc %s mask%d" % (shape, mask))
        _same_bits(ops.nhwc_to_nchw(nhwc.to(gpu), dtype=ddt), x.to(ddt), "nhwc_to_nchw %s mask%d" % (shape, mask))


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
def test_transpose_taps_converting(gpu, mask):
    from gdn_amd import ops
    ddt = torch.bfloat16 if mask & 2 else torch.float32
    for shape in ((9, 5, 7), (1, 1, 1), (2, 33, 65), (4, 64, 32)):
        w = _rand(shape, 7800 + shape[1], mask & 1)
        _same_bits(ops.transpose_taps(w.to(gpu), dtype=ddt), w.transpose(1, 2).contiguous().to(ddt),
                   "transpose_taps %s mask%d" % (shape, mask))
