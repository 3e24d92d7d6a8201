"""The fp32 convolution kernels against exact integer results: every comparison is torch.equal.

The direct kernels (conv_igemm fp32 tiles, conv_wgrad, conv_c1, conv_head_kernel) are plain fp32 FMA: with integer operands every
product and partial sum is an integer, and while the sum of the absolute products stays below 2^24 no tile shape, K-split,
pixel split or combine order can change a bit -- nothing rounds at the store either, so the result is THE integer convolution.
The Winograd schemes F(2x2,3x3) (conv_wino.hip, run here with the F(4x4,3x3) plan off) and F(3x3,2x2) (conv_wino2.hip) transform
with 0, +-1 and 1/2 only: on integers everything is a multiple of 1/4 (1/64 behind the fused x2 bilinear loader) and the whole
pipeline is exact, with the per-bin GEMMs as bf16 x 3 split products (default) as well as on the fp32 MFMA (set_x3(False)).
tests/int_conv_ref.py holds the float64 reference, the operand sets (narrow / wide) and the bounds; each test asserts
exactness_bound(...) or wino_exactness_bound(...) < 2^24 first, then compares bit for bit.  The Gaussian bars of
tests/test_hip_kernels.py / test_hip_winoconv.py / test_hip_wino2conv.py (1e-3 relative + 1e-4 of the maximum) let a stale tile
at a ragged Winograd edge, a wrong polyphase, a dropped split plane or a statistics slot summed twice pass; these do not.
tanh is not exact and stays out; F(4x4,3x3) and the FFT path are held to the nearest integer at the end of this file.
"""
import functools

import pytest
import torch

import test_hip_wino2conv as TW2
import test_hip_winoconv as TW
from int_conv_ref import (HEAD_PLANE_SETS, TWO24, Geom, _up, bnb_ref, conv, dgrad_ref32, exactness_bound, fwd_ref32, geom_of, layer_input, operands,
                          out_hw, stats_ref, wgrad_ref, wino_exactness_bound, wino_operands_16bit, x3_conv_six, head_plane_operands)
from test_hip_bf16_exact import affine, bnb_inputs, same, taps, taps_t
from test_hip_kernels import CONV_CASES, nhwc

pytestmark = pytest.mark.gpu

KINDS = ("narrow", "wide")
# tile ids of gdn_conv_fwd / gdn_conv_dgrad, fp32 (pick_cfg_f32): 0 automatic (3; 4 for <= 32 output channels), 1-4 and 6, 7
# forced.  Kernel variant 5 -- the scalar-load one with the extra template flag -- cannot be forced: the 3- and 1-channel layers
# take it whatever the id (they run id 0 alone here), and on every other layer id 5 is the automatic choice again.
# 0x800: single stage, i.e. pick_ksplit() off; variants 4 and 5 never split
IDS = (0, 1, 2, 3, 4, 6, 7)
SPLIT_IDS = (0, 1, 2, 3, 6, 7)
SK_ROWS = 16                                   # pixels per statistics slot of splitk_combine_kernel
# conv_wgrad row-segment widths (make_plan: 32 unless another even width in 16..64 uses the rows >= 3 % better): 32, 52, 26 and
# rows no width tiles (45 -> 46, 13 -> 16); the CONV_CASES add 24, 20, 12, 40, 8, 6 and the thin / scalar plans
WGRAD_WIDTHS = [("w32", 64, 64, 3, 1, 1, False, False, 1, 6, 32), ("w45", 64, 128, 3, 1, 1, False, False, 1, 5, 45),
                ("w13", 128, 64, 5, 1, 2, False, False, 2, 4, 13), ("w52_rows", 64, 64, 3, 1, 1, False, False, 3, 40, 52)]
WGRAD_CASES = list(CONV_CASES) + WGRAD_WIDTHS
WGRAD_SPLIT_CASES = ("rb_k3_l3", "w52_rows", "cb_k7s2_refl", "ctb_k4s2")      # test_wgrad_exact asserts more than one pixel split
# (Cin, Cout, B, H, W, reflect): tests/test_hip_winoconv.py CASES + REFLECT_CASES without the 32 x 104 image (seconds of float64)
F23_CASES = [c + (False,) for c in TW.CASES] + [c + (True,) for c in TW.REFLECT_CASES if c[3] * c[4] < 32 * 104]
F23_UP2X = [(128, 256, 2, 9, 13, False), (64, 64, 3, 2, 2, False), (128, 64, 2, 9, 13, True), (64, 64, 2, 4, 4, True)]   # H, W: low resolution
# tests/test_hip_wino2conv.py CONV_CASES (without 32 x 104) and CONVT_CASES
F32_CASES = [c for c in TW2.CONV_CASES if c[3] * c[4] < 32 * 104] + [c + (False, True) for c in TW2.CONVT_CASES]      # (7 fields: ConvTranspose2d)


def cdiv(a, b):
    return -(-a // b)


def dev(t, gpu):
    """NCHW float64 -> the device's NHWC float32 tensor (exact: |v| < 2^24)."""
    return nhwc(t).float().to(gpu)


def wino_id(c):
    return "c%d_%d_%dx%dx%d%s" % (c[:5] + ("_refl" if c[5] else "",)) if len(c) == 6 else "t%d_%d_%dx%dx%d" % c[:5]


def check_stats(st, raw, what):
    """The slots, summed in float64, against the raw accumulators: the sum on every channel whose sum |y| is below 2^24, the sum
    of squares on every channel whose sum y^2 is (all of them on the narrow set of operands())."""
    s = st.double().sum(0).cpu()
    s1, s2 = stats_ref(raw)
    ok1, ok2 = raw.abs().sum((0, 2, 3)) < TWO24, s2 < TWO24
    assert bool(ok1.any())
    assert torch.equal(s[0][ok1], s1[ok1]), what + " statistics (sum)"
    assert torch.equal(s[1][ok2], s2[ok2]), what + " statistics (sum of squares)"
    return int(ok2.sum())


def x3_gemms(scheme, g):
    """Which per-bin GEMMs of a layer run as bf16 x 3 when the switch is on -- gemm_x3_ok / gemm_x3_tn_ok (csrc/gemm_x3.h: the
    GEMM's N, for the reduction GEMM both sides, a multiple of 128) as wino_geom / w2_gemm apply them; the others stay on the fp32
    MFMA whatever the switch says.  F(2x2,3x3): forward N = Cout, data gradient N = Cin.  F(3x3,2x2): form A (Conv2d forward,
    ConvTranspose2d data gradient) N = the small image's channels, form B N = 4 x the large image's: always."""
    if scheme == "f23":
        return {"fwd": g.co % 128 == 0, "dgrad": g.ci % 128 == 0, "wgrad": g.ci % 128 == 0 and g.co % 128 == 0}
    cy = g.ci if g.tr else g.co                  # channels of the small image
    return {"fwd": g.tr or cy % 128 == 0, "dgrad": (not g.tr) or cy % 128 == 0, "wgrad": cy % 128 == 0}


def x3_params(scheme, cases, geom):
    """(case, x3) pairs: the switch off only where it changes a GEMM of the layer (a 64 -> 64 channel F(2x2,3x3) layer runs the
    same fp32 kernels either way)."""
    return [(c, x3) for c in cases for x3 in (True, False) if x3 or any(x3_gemms(scheme, geom(c)).values())]


def x3_ids(pairs):
    return ["%s-%s" % (wino_id(c), "x3" if x3 else "fp32gemm") for c, x3 in pairs]


class switches:
    """F(4x4,3x3) off (every wino_ok layer then takes F(2x2,3x3)) and the bf16 x 3 GEMMs on / off; both restored on exit."""
    def __init__(self, x3, f4=False):
        self.x3, self.f4 = x3, f4

    def __enter__(self):
        from gdn_amd import ops
        self.prev = (ops.set_x3(self.x3), ops.set_wino_f4(self.f4))

    def __exit__(self, *exc):
        from gdn_amd import ops
        ops.set_x3(self.prev[0])
        ops.set_wino_f4(self.prev[1])


# ---------------------------------------------------------------------------------------------------------------------------
# Direct kernels: conv_igemm fp32 forward and data gradient
# ---------------------------------------------------------------------------------------------------------------------------
def run_fwd(gpu, case, kind, ids, flags=(0, 0x800)):
    from gdn_amd import ops
    g, bhw = geom_of(case)
    o = operands(g, bhw, kind)
    scale, shift = affine(g.co)
    assert exactness_bound(o.x, o.w, 1.0, g, addsrc=o.add_y) < TWO24
    assert exactness_bound(o.x, o.w, 0.5, g, scale=scale, shift=shift, addsrc=o.add_y) < TWO24
    y_ref, raw = fwd_ref32(o.x, o.w, g)
    y_add = fwd_ref32(o.x, o.w, g, addsrc=o.add_y, raw=raw)[0]
    y_ep = fwd_ref32(o.x, o.w, g, scale, shift, True, o.add_y, raw=raw)[0]
    y_ref, y_add, y_ep = [dev(t, gpu) for t in (y_ref, y_add, y_ep)]
    xd, wd, addd = dev(o.x, gpu), taps(o.w, g.tr).to(gpu), dev(o.add_y, gpu)
    aff = (scale.to(gpu), shift.to(gpu))
    slots = {}
    for cfg in ids:
        for fl in flags:
            op = ops.Conv(g.ci, g.co, g.k, g.s, g.p, reflect=g.refl, transposed=g.tr)
            what = "%s %s fwd id %d flags %#x" % (case[0], kind, cfg, fl)
            y, st = op.fwd(xd, wd, stats=True, tile_cfg=cfg | fl)
            same(y, y_ref, what)
            check_stats(st, raw, what)
            slots[(cfg, fl)] = st.shape[0]
            same(op.fwd(xd, wd, addsrc=addd, tile_cfg=cfg | fl), y_add, what + " + addsrc")
            same(op.fwd(xd, wd, act=ops.ACT_RELU, addsrc=addd, affine=aff, tile_cfg=cfg | fl), y_ep, what + " affine relu addsrc")
    return slots


def run_dgrad(gpu, case, kind, ids, flags=(0, 0x800)):
    from gdn_amd import ops
    g, bhw = geom_of(case)
    o = operands(g, bhw, kind)
    hw = bhw[1:]
    assert exactness_bound(o.dy, o.w, 1.0, g, mode="dgrad", in_hw=hw, addsrc=o.add_x) < TWO24
    ref0 = dev(dgrad_ref32(o.dy, o.w, g, hw), gpu)
    ref1 = dev(dgrad_ref32(o.dy, o.w, g, hw, addsrc=o.add_x), gpu)
    gyd, wt, addd = dev(o.dy, gpu), taps_t(o.w, g.tr).to(gpu), dev(o.add_x, gpu)
    for cfg in ids:
        for fl in flags:
            op = ops.Conv(g.ci, g.co, g.k, g.s, g.p, reflect=g.refl, transposed=g.tr)
            what = "%s %s dgrad id %d flags %#x" % (case[0], kind, cfg, fl)
            same(op.dgrad(gyd, wt, hw, addsrc=addd, tile_cfg=cfg | fl), ref1, what + " + addsrc")
            if cfg == 0:
                same(op.dgrad(gyd, wt, hw, tile_cfg=fl), ref0, what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_fwd_exact(gpu, case, kind):
    """y, the statistics, + addsrc, affine + ReLU + addsrc: bitwise the integer result on every tile id, with pick_ksplit()'s
    tap split on and off (0x800).  With statistics or an epilogue the one-channel heads run the MFMA kernel here."""
    slots = run_fwd(gpu, case, kind, IDS if case[1] % 4 == 0 else (0,))
    if case[0] == "rb_k3_l3":            # 1664 pixels, 128 channels: at most 64 tiles, nine taps -> three ways on every id that may split
        B, H, W = case[-3:]
        for cfg in SPLIT_IDS:
            assert slots[(cfg, 0)] == cdiv(B * H * W, SK_ROWS) != slots[(cfg, 0x800)], "id %d: no K-split" % cfg
        assert slots[(4, 0)] == slots[(4, 0x800)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [c for c in CONV_CASES if c[1] >= 32], ids=[c[0] for c in CONV_CASES if c[1] >= 32])
def test_dgrad_exact(gpu, case, kind):
    """Stride 1 / 2, transposed, the heads (reduction over one channel) and the reflection layers (padded-domain gradient in an
    fp32 workspace + reflect_fold_kernel: no rounding, plain autograd), with and without addsrc.  The 3- and 1-channel image
    layers have no data gradient."""
    from gdn_amd import ops
    from gdn_amd._lib import lib
    run_dgrad(gpu, case, kind, IDS)
    if case[0] == "rb_k3_l3":            # the K-split partials are the whole workspace of a zero-padded layer's data gradient
        g, bhw = geom_of(case)
        ref = ops.Conv(g.ci, g.co, g.k, g.s, g.p).geom(*bhw)[1]
        for cfg in SPLIT_IDS:
            assert int(lib.gdn_conv_dgrad_workspace_bytes(ref, cfg)) > int(lib.gdn_conv_dgrad_workspace_bytes(ref, cfg | 0x800)) == 0


# reflect_fold_scalar_kernel: the fold of a reflection layer whose input channels are no multiple of 4.  The network's 3- and
# 1-channel layers need no data gradient, so nothing else runs it: 3 channels, 1 x 5 x 6 pixels, pad 1 and pad 3 -- at pad 3 rows
# 1..3 are mirrored by BOTH borders (three sources per axis) and every branch of the mirror rule (csrc/reflect_fold.h) is taken.
SCALAR_FOLD_CASES = [("fold_c3_k3_refl", 3, 64, 3, 1, 1, True, False, 1, 5, 6), ("fold_c3_k7_refl", 3, 64, 7, 1, 3, True, False, 1, 5, 6)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", SCALAR_FOLD_CASES, ids=[c[0] for c in SCALAR_FOLD_CASES])
def test_dgrad_scalar_fold_exact(gpu, case, kind):
    """Padded-domain gradient with pitch 3 in the fp32 workspace + the scalar fold, with and without addsrc."""
    run_dgrad(gpu, case, kind, (0,))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["rb_k9_64", "cb_k7s2_refl", "rb_k3_l3", "ctb_k4s2_b"])
def test_kc64_exact(gpu, name, kind):
    """0x200: 64-channel slabs -- taken by the tiles of at most 64 x 128 (ids 2, 3, 6, 7) when the reduction channels are a
    multiple of 64, which they are on these layers in both directions."""
    case = next(c for c in CONV_CASES if c[0] == name)
    assert case[1] % 64 == 0 and case[2] % 64 == 0
    run_fwd(gpu, case, kind, (0, 2, 3, 6, 7), flags=(0x200, 0xa00))
    run_dgrad(gpu, case, kind, (0, 2, 3, 6, 7), flags=(0x200, 0xa00))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["cb_k1", "rb_k3_l3"])
def test_fwd_concat_exact(gpu, name, kind):
    """The fused concat: x2 a channel slice of a wider (pitch 96) tensor, integer addsrc, every id, split and single stage."""
    from gdn_amd import ops
    case = next(c for c in CONV_CASES if c[0] == name)
    g, bhw = geom_of(case)
    o = operands(g, bhw, kind)
    assert exactness_bound(o.x, o.w, 1.0, g, addsrc=o.add_y) < TWO24
    ref = dev(fwd_ref32(o.x, o.w, g, addsrc=o.add_y)[0], gpu)
    xd = dev(o.x, gpu)
    wide = torch.full(xd.shape[:3] + (96,), 7.0, device=gpu)
    wide[..., 16:80] = xd[..., 64:]
    a = xd[..., :64].contiguous()
    wd, addd = taps(o.w, False).to(gpu), dev(o.add_y, gpu)
    for cfg in IDS:
        for fl in (0, 0x800, 0x200):
            y = ops.Conv(g.ci, g.co, g.k, g.s, g.p).fwd(a, wd, x2=wide[..., 16:80], addsrc=addd, tile_cfg=cfg | fl)
            same(y, ref, "concat %s %s id %d flags %#x" % (name, kind, cfg, fl))


# ---------------------------------------------------------------------------------------------------------------------------
# conv_wgrad fp32
# ---------------------------------------------------------------------------------------------------------------------------
def wgrad_tw(g, bhw):
    """The row-segment width make_plan() (csrc/conv_wgrad.hip) picks, restated: the G-role tensor is dy for a Conv2d with >= 32
    output channels, the layer input otherwise; scalar-load layers (a channel count that is no multiple of 4) and the thin plan
    of the heads keep 32."""
    B, H, W = bhw
    head = not g.tr and g.co < 32 and g.s == 1 and not g.refl
    wg, cg, cx = (W, g.ci, g.co) if (g.tr or head) else (out_hw(g, H, W)[1], g.co, g.ci)
    if cg % 4 or min(cx, 64) % 4 or (cx * g.k <= 32 and g.s == 1):
        return 32
    best, best_eff = 32, wg / (cdiv(wg, 32) * 32)
    for tw in range(64, 15, -2):
        eff = wg / (cdiv(wg, tw) * tw) * (1.0 if tw >= 32 else 0.97)
        if eff > best_eff + 0.03:
            best, best_eff = tw, eff
    return best


def wgrad_splits(op, g, bhw, cx):
    """Pixel (row) splits of the plan: the workspace holds one [k*k][Cout][Cx] partial set per split."""
    from gdn_amd._lib import lib
    nb = int(lib.gdn_conv_wgrad_workspace_bytes(op.geom(*bhw)[1], cx))
    assert nb > 0 and nb % (g.k * g.k * g.co * cx * 4) == 0
    return nb // (g.k * g.k * g.co * cx * 4)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_wgrad_exact(gpu, case, kind):
    """conv_wgrad_f32 (every segment width: tests/test_int_conv_ref_cpu.py::test_wgrad_cases_cover_the_segment_widths),
    conv_wgrad_thin_f32 (the heads) and wgrad_reduce_kernel: dw into a NaN-filled buffer is the integer result."""
    from gdn_amd import ops
    g, bhw = geom_of(case)
    o = operands(g, bhw, kind)
    assert exactness_bound(o.x, o.dy, 1.0, g, mode="wgrad") < TWO24
    ref = taps(wgrad_ref(o.x, o.dy, g), g.tr).to(gpu)
    op = ops.Conv(g.ci, g.co, g.k, g.s, g.p, reflect=g.refl, transposed=g.tr)
    if case[0] in WGRAD_SPLIT_CASES:
        assert wgrad_splits(op, g, bhw, g.ci) > 1, "the plan has one pixel split"
    dw = torch.full(ref.shape, float("nan"), device=gpu)
    op.wgrad(dev(o.x, gpu), dev(o.dy, gpu), dw)
    same(dw, ref, "%s %s wgrad" % (case[0], kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["cb_k1", "rb_k3_l3"])
def test_wgrad_concat_halves_exact(gpu, name, kind):
    """The two halves of a concat layer's weight gradient, the second from a slice of a wider tensor, written at ci_off."""
    from gdn_amd import ops
    case = next(c for c in CONV_CASES if c[0] == name)
    g, bhw = geom_of(case)
    o = operands(g, bhw, kind)
    assert exactness_bound(o.x, o.dy, 1.0, g, mode="wgrad") < TWO24
    ref = taps(wgrad_ref(o.x, o.dy, g), False).to(gpu)
    xd, gyd = dev(o.x, gpu), dev(o.dy, gpu)
    wide = torch.full(xd.shape[:3] + (96,), 7.0, device=gpu)
    wide[..., 16:80] = xd[..., 64:]
    op = ops.Conv(g.ci, g.co, g.k, g.s, g.p)
    dw = torch.full(ref.shape, float("nan"), device=gpu)
    op.wgrad(xd[..., :64].contiguous(), gyd, dw, 0)
    op.wgrad(wide[..., 16:80], gyd, dw, 64)
    same(dw, ref, "concat wgrad %s %s" % (name, kind))


# ---------------------------------------------------------------------------------------------------------------------------
# conv_c1 (1 / 3 <-> 64 channels, 9x9) and the fp32 head
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def c1_operands(cin, B, H, W, kind):
    gen = torch.Generator().manual_seed(1000 * cin + 10 * H + W + (1 if kind == "wide" else 0))
    a = 8 if kind == "wide" else 1
    r = lambda *s: torch.randint(-a, a + 1, s, generator=gen).double()
    return r(B, cin, H, W), r(64, cin, 9, 9), r(B, 64, H, W), r(B, 64, H, W)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cin,B,H,W,reflect,flip", [(1, 2, 16, 64, True, False), (1, 1, 13, 45, False, True), (1, 2, 5, 7, True, True),
                                                    (3, 2, 16, 64, True, False), (3, 1, 13, 45, False, False), (3, 2, 5, 7, True, False)])
def test_c1_exact(gpu, cin, B, H, W, reflect, flip, kind):
    """gdn_conv_c1_fwd (CIN = 1: the first layer of G and a head's data gradient, taps flipped; CIN = 3: R's first layer on the
    patch-staged MFMA kernel) and gdn_conv_c1_wgrad: reflection / zero border, ragged 13 x 45 tiles, an image smaller than a
    tile, statistics, epilogue."""
    from gdn_amd import ops
    x, w, gy, add = c1_operands(cin, B, H, W, kind)
    g = Geom(cin, 64, 9, 1, 4, reflect, False)
    wf = torch.flip(w, (2, 3)) if flip else w
    scale, shift = affine(64)
    assert exactness_bound(x, wf, 0.5, g, scale=scale, shift=shift, addsrc=add) < TWO24 and exactness_bound(x, wf, 1.0, g) < TWO24
    y_ref, raw = fwd_ref32(x, wf, g)
    xd, wd = dev(x, gpu), taps(w, False).to(gpu)                       # [B,H,W,cin], [81][64][cin]
    assert ops.c1_ok(xd, 64, 9, 1, 4, rgb=cin == 3)
    y, st = ops.conv_c1_fwd(xd, wd, reflect=reflect, flip=flip, stats=True)
    what = "c1 cin %d %dx%dx%d %s" % (cin, B, H, W, kind)
    same(y, dev(y_ref, gpu), what)
    check_stats(st, raw, what)
    y2 = ops.conv_c1_fwd(xd, wd, reflect=reflect, flip=flip, addsrc=dev(add, gpu), affine=(scale.to(gpu), shift.to(gpu)), act=ops.ACT_RELU)
    same(y2, dev(fwd_ref32(x, wf, g, scale, shift, True, add, raw=raw)[0], gpu), what + " epilogue")
    if cin == 1:
        assert exactness_bound(x, gy, 1.0, g, mode="wgrad") < TWO24
        dw = wgrad_ref(x, gy, g)                                       # gradient of the taps as applied ...
        dw = torch.flip(dw, (2, 3)) if flip else dw                    # ... written at the stored position
        out = torch.full((81, 64), float("nan"), device=gpu)
        ops.conv_c1_wgrad(xd, dev(gy, gpu), out, reflect=reflect, flip=flip)
        same(out, dw.permute(2, 3, 0, 1).reshape(81, 64).float().to(gpu), what + " wgrad")


HEAD_CASES = [c for c in CONV_CASES if c[2] == 1]                       # 64 -> 1: the matrix-pipe head
# 32 -> 1: gdn_conv_head_fwd sends every channel count but 64 to the VALU kernel (Conv2d, ConvTranspose2d, ragged 21 x 70)
HEAD_VALU_CASES = [("head32_conv", 32, 1, 9, 1, 4, False, False, 2, 16, 24), ("head32_convt", 32, 1, 9, 1, 4, False, True, 2, 16, 24),
                   ("head32_conv_ragged", 32, 1, 9, 1, 4, False, False, 1, 21, 70), ("head32_convt_ragged", 32, 1, 9, 1, 4, False, True, 1, 21, 70)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", HEAD_VALU_CASES, ids=[c[0] for c in HEAD_VALU_CASES])
def test_head_valu_exact(gpu, case, kind):
    """conv_head_kernel<9> (packed VALU fma, plain fp32: granule 1, nothing rounds): reached without statistics or epilogue
    (those select the MFMA igemm kernel, covered by test_fwd_exact) and with a channel count other than 64."""
    from gdn_amd import ops
    g, bhw = geom_of(case)
    assert g.ci != 64 and g.ci % 4 == 0
    o = operands(g, bhw, kind)
    assert exactness_bound(o.x, o.w, 1.0, g) < TWO24
    y = ops.Conv(g.ci, 1, 9, 1, 4, transposed=g.tr).fwd(dev(o.x, gpu), taps(o.w, g.tr).to(gpu))
    same(y, dev(conv(o.x, o.w, g), gpu), "%s %s conv_head_kernel" % (case[0], kind))


@pytest.mark.parametrize("kind", KINDS + tuple(sorted(HEAD_PLANE_SETS)))
@pytest.mark.parametrize("case", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_head_mfma_exact(gpu, case, kind):
    """The 64 -> 1 fp32 heads run conv_head_mfma_kernel<true>: x and w are split into three bf16 planes each and six of the nine
    plane products are kept, as in gemm_x3.h -- exact when the three dropped products vanish, which the test asserts by
    evaluating the six-product sum in float64 (x3_conv_six), with the bound on the sum of the absolute plane products.  narrow /
    wide fill the first plane of either side only; x24 / w24 / x2w2 need planes 2 and 3 of x, of w, and the product of the two
    second planes (tests/test_int_conv_ref_cpu.py shows each set fails without the products it targets)."""
    from gdn_amd import ops
    g, bhw = geom_of(case)
    assert g.ci == 64
    x, w = head_plane_operands(kind, g, bhw) if kind in HEAD_PLANE_SETS else operands(g, bhw, kind)[:2]
    ref = conv(x, w, g)
    assert float(x3_conv_six(x, w, g, absolute=True).max()) < TWO24
    assert torch.equal(x3_conv_six(x, w, g), ref) and torch.equal(ref.float().double(), ref)
    y = ops.Conv(64, 1, 9, 1, 4, transposed=g.tr).fwd(dev(x, gpu), taps(w, g.tr).to(gpu))
    same(y, dev(ref, gpu), "%s %s conv_head_mfma_kernel" % (case[0], kind))


# ---------------------------------------------------------------------------------------------------------------------------
# Winograd F(2x2,3x3)
# ---------------------------------------------------------------------------------------------------------------------------
def f23_geom(c, tr=False):
    ci, co, B, H, W, refl = c
    return Geom(ci, co, 3, 1, 1, bool(refl), tr), (B, H, W)


def in_affine_of(ci, seed=21):
    """The producer's BatchNorm as the loader applies it: scale a power of two, integer shift."""
    gen = torch.Generator().manual_seed(seed)
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (ci,), generator=gen)], torch.randint(-2, 3, (ci,), generator=gen).float()


def f2_slots(B, H, W):
    return cdiv(B * cdiv(H, 2) * cdiv(W, 2), 4)


F23_X3 = x3_params("f23", F23_CASES, lambda c: f23_geom(c)[0])
F23_UP2X_X3 = x3_params("f23", F23_UP2X, lambda c: f23_geom(c)[0])
F23_FLIP_X3 = x3_params("f23", [(128, 256, 2, 9, 13, False), (256, 128, 1, 5, 6, False)], lambda c: f23_geom(c, tr=True)[0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case,x3", F23_X3, ids=x3_ids(F23_X3))
def test_f23_fwd_exact(gpu, case, kind, x3):
    """y, statistics, addsrc + affine + ReLU, and the producer's BatchNorm applied on load (in_affine, with and without ReLU:
    granule 1/8)."""
    from gdn_amd import ops
    g, bhw = f23_geom(case)
    o = operands(g, bhw, kind)
    scale, shift = affine(g.co)
    isc, ish = in_affine_of(g.ci)
    assert wino_exactness_bound("f23", "fwd", o.x, o.w, g, scale=scale, shift=shift, addsrc=o.add_y) < TWO24
    assert wino_operands_16bit("f23", "fwd", o.x, o.w, g)
    y_ref, raw = fwd_ref32(o.x, o.w, g)
    xd, wd = dev(o.x, gpu), taps(o.w, False).to(gpu)
    what = "F(2x2,3x3) %s %s x3=%s" % (wino_id(case), kind, x3)
    with switches(x3):
        op = ops.Conv(g.ci, g.co, 3, 1, 1, reflect=g.refl)
        assert op.wino_ok(*bhw)
        y, st = op.wino_fwd(xd, wd, stats=True)
        assert st.shape[0] == f2_slots(*bhw), "not the F(2x2,3x3) plan"
        same(y, dev(y_ref, gpu), what)
        check_stats(st, raw, what)
        y2 = op.wino_fwd(xd, wd, addsrc=dev(o.add_y, gpu), affine=(scale.to(gpu), shift.to(gpu)), act=ops.ACT_RELU)
        same(y2, dev(fwd_ref32(o.x, o.w, g, scale, shift, True, o.add_y, raw=raw)[0], gpu), what + " epilogue")
        for relu in (True, False):
            xin = layer_input(o.x, (isc, ish), relu)
            assert wino_exactness_bound("f23", "fwd", xin, o.w, g, granule=0.125) < TWO24
            assert wino_operands_16bit("f23", "fwd", xin, o.w, g)
            y3 = op.wino_fwd(xd, wd, in_affine=(isc.to(gpu), ish.to(gpu)), in_relu=relu)
            same(y3, dev(conv(xin, o.w, g), gpu), what + " in_affine relu=%s" % relu)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case,x3", F23_X3, ids=x3_ids(F23_X3))
def test_f23_bwd_exact(gpu, case, kind, x3):
    """dx (with and without addsrc and the forward's state), dw from the state, need_dx=False; reflection layers through the
    padded-domain gradient and wino_reflect_fold_kernel; zero-padded layers with the BatchNorm-backward partials (bnb)."""
    from gdn_amd import ops
    g, bhw = f23_geom(case)
    B, H, W = bhw
    o = operands(g, bhw, kind)
    assert wino_exactness_bound("f23", "dgrad", o.dy, o.w, g, addsrc=o.add_x) < TWO24
    assert wino_exactness_bound("f23", "wgrad", o.x, o.dy, g) < TWO24
    assert wino_operands_16bit("f23", "dgrad", o.dy, o.w, g) and wino_operands_16bit("f23", "wgrad", o.x, o.dy, g)
    dx0 = dgrad_ref32(o.dy, o.w, g, (H, W))
    dx1 = dgrad_ref32(o.dy, o.w, g, (H, W), addsrc=o.add_x)
    dw_ref = taps(wgrad_ref(o.x, o.dy, g), False).to(gpu)
    xd, wd, gyd, addd = dev(o.x, gpu), taps(o.w, False).to(gpu), dev(o.dy, gpu), dev(o.add_x, gpu)
    what = "F(2x2,3x3) %s %s x3=%s" % (wino_id(case), kind, x3)
    with switches(x3):
        op = ops.Conv(g.ci, g.co, 3, 1, 1, reflect=g.refl)
        y, st, sv = op.wino_fwd(xd, wd, stats=True, state=True)
        assert st.shape[0] == f2_slots(*bhw), "not the F(2x2,3x3) plan"
        dw = torch.full_like(wd, float("nan"))
        dx = op.wino_bwd(gyd, wd, (H, W), state=sv, dw_tap=dw, addsrc=addd)
        same(dx, dev(dx1, gpu), what + " dx + addsrc")
        same(dw, dw_ref, what + " dw")
        same(op.wino_bwd(gyd, wd, (H, W)), dev(dx0, gpu), what + " dx without state")
        dw2 = torch.full_like(wd, float("nan"))
        assert op.wino_bwd(gyd, wd, (H, W), state=sv, dw_tap=dw2, need_dx=False) is None
        same(dw2, dw_ref, what + " dw alone")
        if not g.refl:
            yb, coef = bnb_inputs(g, bhw)
            slots = op.wino_bnb_slots(*bhw)
            assert slots == f2_slots(*bhw)
            for relu in (True, False):
                s1, s2, _ = bnb_ref(dx1, yb, coef, relu)
                sc, sh, mu, isd = [c.double().view(1, -1, 1, 1) for c in coef]
                dz = dx1 * ((yb * sc + sh) > 0) if relu else dx1
                assert float((dz * (yb - mu) * isd).abs().sum((0, 2, 3)).max()) / 0.5 < TWO24     # granule 1/2: invstd in {1/2, 1, 2}
                part = torch.full((slots, 2, g.ci), float("nan"), device=gpu)
                same(op.wino_bwd(gyd, wd, (H, W), addsrc=addd, bnb=(dev(yb, gpu), coef.to(gpu), relu, part)), dev(dx1, gpu),
                     what + " dx with bnb")
                s = part.double().sum(0).cpu()
                assert torch.equal(s[0], s1) and torch.equal(s[1], s2), what + " bnb sums relu=%s" % relu


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case,x3", F23_UP2X_X3, ids=x3_ids(F23_UP2X_X3))
def test_f23_up2x_exact(gpu, case, kind, x3):
    """up2x = 1: the input transform upsamples the low-resolution tensor on load (weights 1/4, 3/4: sixteenths, granule 1/64);
    reflection layers also backward -- the fold pass applies the adjoint interpolation, dx and addsrc are low-resolution."""
    from gdn_amd import ops
    ci, co, B, Hl, Wl, refl = case
    H, W = 2 * Hl, 2 * Wl
    g = Geom(ci, co, 3, 1, 1, bool(refl), False)
    lo, o = operands(g, (B, Hl, Wl), kind), operands(g, (B, H, W), kind)
    xl, xin = lo.x, _up(lo.x)
    assert wino_exactness_bound("f23", "fwd", xin, o.w, g, granule=1.0 / 64) < TWO24
    assert wino_operands_16bit("f23", "fwd", xin, o.w, g)
    xd, wd = dev(xl, gpu), taps(o.w, False).to(gpu)
    what = "F(2x2,3x3) up2x %s %s x3=%s" % (wino_id(case), kind, x3)
    with switches(x3):
        op = ops.Conv(ci, co, 3, 1, 1, reflect=g.refl)
        y, st, sv = op.wino_fwd(xd, wd, stats=True, state=True, up2x=1)
        assert st.shape[0] == f2_slots(B, H, W)
        same(y, dev(conv(xin, o.w, g), gpu), what)
        if g.refl:
            assert wino_exactness_bound("f23", "dgrad", o.dy, o.w, g, granule=1.0 / 16, addsrc=lo.add_x, up2x=1) < TWO24
            assert wino_exactness_bound("f23", "wgrad", xin, o.dy, g, granule=1.0 / 64) < TWO24
            assert wino_operands_16bit("f23", "wgrad", xin, o.dy, g)
            dw = torch.full_like(wd, float("nan"))
            dx = op.wino_bwd(dev(o.dy, gpu), wd, (H, W), state=sv, dw_tap=dw, addsrc=dev(lo.add_x, gpu), up2x=1)
            same(dx, dev(dgrad_ref32(o.dy, o.w, g, (H, W), addsrc=lo.add_x, up2x=1), gpu), what + " dx")
            same(dw, taps(wgrad_ref(xin, o.dy, g), False).to(gpu), what + " dw")
            same(op.wino_bwd(dev(o.dy, gpu), wd, (H, W), up2x=1), dev(dgrad_ref32(o.dy, o.w, g, (H, W), up2x=1), gpu), what + " dx alone")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case,x3", F23_FLIP_X3, ids=x3_ids(F23_FLIP_X3))
def test_f23_flip_taps_exact(gpu, case, kind, x3):
    """A stride-1 ConvTranspose2d(3, 1, 1) as the flipped-tap convolution it is (GDN_HINT_FLIP_TAPS): forward, dx, and dw in the
    module's own (stored) tap order."""
    from gdn_amd import ops
    g, bhw = f23_geom(case, tr=True)
    B, H, W = bhw
    o = operands(g, bhw, kind)
    for mode, a, b in (("fwd", o.x, o.w), ("dgrad", o.dy, o.w), ("wgrad", o.x, o.dy)):
        assert wino_exactness_bound("f23", mode, a, b, g, addsrc=o.add_x if mode == "dgrad" else None) < TWO24
        assert wino_operands_16bit("f23", mode, a, b, g)
    xd, wd = dev(o.x, gpu), taps(o.w, True).to(gpu)
    what = "F(2x2,3x3) flip_taps %s %s x3=%s" % (wino_id(case), kind, x3)
    with switches(x3):
        op = ops.Conv(g.ci, g.co, 3, 1, 1, flip_taps=True)
        y, sv = op.wino_fwd(xd, wd, state=True)
        same(y, dev(conv(o.x, o.w, g), gpu), what)
        dw = torch.full_like(wd, float("nan"))
        dx = op.wino_bwd(dev(o.dy, gpu), wd, (H, W), state=sv, dw_tap=dw, addsrc=dev(o.add_x, gpu))
        same(dx, dev(dgrad_ref32(o.dy, o.w, g, (H, W), addsrc=o.add_x), gpu), what + " dx")
        same(dw, taps(wgrad_ref(o.x, o.dy, g), True).to(gpu), what + " dw")


def test_x3_switch_changes_the_saved_weight_set(gpu):
    """That set_x3() reaches the kernels: the data gradient's weight set in a forward's state is fp32 [16][Cin][Cout] with the
    switch off and bf16 x 3 panels with it on (Cin a multiple of 128: gemm_x3_ok) -- other bytes, same size."""
    from gdn_amd import ops
    g, bhw = f23_geom((128, 256, 2, 9, 13, False))
    o = operands(g, bhw, "wide")
    xd, wd = dev(o.x, gpu), taps(o.w, False).to(gpu)
    vb = cdiv(16 * bhw[0] * cdiv(bhw[1], 2) * cdiv(bhw[2], 2) * g.ci * 4, 256) * 256          # the transformed input V comes first
    sv = {}
    for x3 in (True, False):
        with switches(x3):
            sv[x3] = ops.Conv(g.ci, g.co, 3, 1, 1).wino_fwd(xd, wd, state=True)[1].clone()
    assert sv[True].numel() == sv[False].numel() > vb
    assert torch.equal(sv[True][:vb], sv[False][:vb]) and not torch.equal(sv[True][vb:], sv[False][vb:])


# ---------------------------------------------------------------------------------------------------------------------------
# Winograd F(3x3,2x2): the 4x4 stride-2 layers
# ---------------------------------------------------------------------------------------------------------------------------
def f32_geom(c):
    tr = len(c) == 7
    return Geom(c[0], c[1], 4, 2, 1, bool(c[5]) and not tr, tr), tuple(c[2:5])


F32_X3 = x3_params("f32", F32_CASES, lambda c: f32_geom(c)[0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case,x3", F32_X3, ids=x3_ids(F32_X3))
def test_f32_exact(gpu, case, kind, x3):
    """Conv2d (reflection and zero border; the data gradient of a reflection layer on the padded domain + fold) and
    ConvTranspose2d: y, statistics, epilogue; dx (+ addsrc), dw from the state, need_dx=False.  wino2_bwd emits no
    BatchNorm-backward partials: asking for them is an error."""
    from gdn_amd import ops
    from gdn_amd._lib import GdnError
    g, bhw = f32_geom(case)
    tr, ci, co, (B, H, W) = g.tr, g.ci, g.co, bhw
    assert x3 or any(x3_gemms("f32", g).values())
    o = operands(g, bhw, kind)
    scale, shift = affine(co)
    assert wino_exactness_bound("f32", "fwd", o.x, o.w, g, scale=scale, shift=shift, addsrc=o.add_y) < TWO24
    assert wino_exactness_bound("f32", "dgrad", o.dy, o.w, g, addsrc=o.add_x) < TWO24
    assert wino_exactness_bound("f32", "wgrad", o.x, o.dy, g) < TWO24
    for mode, a, b in (("fwd", o.x, o.w), ("dgrad", o.dy, o.w), ("wgrad", o.x, o.dy)):
        assert wino_operands_16bit("f32", mode, a, b, g)
    y_ref, raw = fwd_ref32(o.x, o.w, g)
    xd, wd, gyd = dev(o.x, gpu), taps(o.w, tr).to(gpu), dev(o.dy, gpu)
    what = "F(3x3,2x2) %s %s x3=%s" % (wino_id(case), kind, x3)
    with switches(x3):
        op = ops.Conv(ci, co, 4, 2, 1, reflect=g.refl, transposed=tr)
        assert op.wino2_ok(*bhw)
        y, st, sv = op.wino2_fwd(xd, wd, stats=True, state=True)
        same(y, dev(y_ref, gpu), what)
        check_stats(st, raw, what)
        y2 = op.wino2_fwd(xd, wd, addsrc=dev(o.add_y, gpu), affine=(scale.to(gpu), shift.to(gpu)), act=ops.ACT_RELU)
        same(y2, dev(fwd_ref32(o.x, o.w, g, scale, shift, True, o.add_y, raw=raw)[0], gpu), what + " epilogue")
        dw_ref = taps(wgrad_ref(o.x, o.dy, g), tr).to(gpu)
        dw = torch.full_like(wd, float("nan"))
        dx = op.wino2_bwd(gyd, wd, (H, W), state=sv, dw_tap=dw, addsrc=dev(o.add_x, gpu))
        same(dx, dev(dgrad_ref32(o.dy, o.w, g, (H, W), addsrc=o.add_x), gpu), what + " dx + addsrc")
        same(dw, dw_ref, what + " dw")
        same(op.wino2_bwd(gyd, wd, (H, W)), dev(dgrad_ref32(o.dy, o.w, g, (H, W)), gpu), what + " dx without state")
        dw2 = torch.full_like(wd, float("nan"))
        assert op.wino2_bwd(gyd, wd, (H, W), state=sv, dw_tap=dw2, need_dx=False) is None
        same(dw2, dw_ref, what + " dw alone")
        with pytest.raises(GdnError, match="bnb"):
            op.wino2_bwd(gyd, wd, (H, W), bnb=(xd, None, True, None))


# ---------------------------------------------------------------------------------------------------------------------------
# Sensitivity, once per kernel family: one more product must move the result -- to exactly the recomputed reference
# ---------------------------------------------------------------------------------------------------------------------------
def _case(name):
    return next(c for c in CONV_CASES if c[0] == name)


@pytest.mark.parametrize("family", ["igemm", "igemm_ksplit", "head_mfma", "head_valu", "f23", "f32"])
def test_sensitivity_fwd(gpu, family):
    """After the exact check, +1 on one weight of the device copy (an interior tap, the last input channel): the output must be
    bitwise the reference of the changed weights, and that reference differs from the first."""
    from gdn_amd import ops
    if family == "f23":
        g, bhw = f23_geom((128, 256, 2, 9, 13, False))
    elif family == "f32":
        g, bhw = Geom(64, 128, 4, 2, 1, True, False), (2, 10, 14)
    elif family == "head_valu":                    # 32 -> 1: conv_head_kernel
        g, bhw = geom_of(HEAD_VALU_CASES[2])
    else:                                          # (64 -> 1: conv_head_mfma_kernel<true>)
        g, bhw = geom_of(_case("head_conv_k9_ragged" if family == "head_mfma" else "cb_k4s2_refl"))
    o = operands(g, bhw, "wide")
    op = ops.Conv(g.ci, g.co, g.k, g.s, g.p, reflect=g.refl)
    xd, wd = dev(o.x, gpu), taps(o.w, False).to(gpu)
    run = {"igemm": lambda: op.fwd(xd, wd, tile_cfg=0x800), "igemm_ksplit": lambda: op.fwd(xd, wd, addsrc=None, tile_cfg=2),
           "head_mfma": lambda: op.fwd(xd, wd), "head_valu": lambda: op.fwd(xd, wd), "f23": lambda: op.wino_fwd(xd, wd), "f32": lambda: op.wino2_fwd(xd, wd)}[family]
    bound = (lambda w: wino_exactness_bound(family, "fwd", o.x, w, g)) if family in ("f23", "f32") else (lambda w: exactness_bound(o.x, w, 1.0, g))
    with switches(True):
        ref0 = conv(o.x, o.w, g)
        same(run(), dev(ref0, gpu), family + " before")
        ky = kx = g.k // 2
        n = min(5, g.co - 1)
        w1 = o.w.clone()
        w1[n, g.ci - 1, ky, kx] += 1
        wd[ky * g.k + kx, n, g.ci - 1] += 1
        assert bound(w1) < TWO24
        ref1 = conv(o.x, w1, g)
        assert not torch.equal(ref0, ref1)
        same(run(), dev(ref1, gpu), family + " after one more product")


@pytest.mark.parametrize("family", ["fold", "f23_fold", "f32_fold"])
def test_sensitivity_dgrad(gpu, family):
    """The same on the data gradient of a reflection layer (kernel + fold pass): the reduction runs over Cout."""
    from gdn_amd import ops
    if family == "fold":
        g, bhw = geom_of(_case("cb_k3s1_refl"))
    elif family == "f23_fold":
        g, bhw = f23_geom((128, 64, 2, 9, 13, True))
    else:
        g, bhw = Geom(64, 128, 4, 2, 1, True, False), (2, 10, 14)
    hw = bhw[1:]
    o = operands(g, bhw, "wide")
    op = ops.Conv(g.ci, g.co, g.k, g.s, g.p, reflect=True)
    gyd, wd, addd = dev(o.dy, gpu), taps(o.w, False).to(gpu), dev(o.add_x, gpu)
    if family == "fold":
        run = lambda: op.dgrad(gyd, ops.transpose_taps(wd), hw, addsrc=addd)
        bound = lambda w: exactness_bound(o.dy, w, 1.0, g, mode="dgrad", in_hw=hw, addsrc=o.add_x)
    else:
        run = lambda: (op.wino_bwd if family == "f23_fold" else op.wino2_bwd)(gyd, wd, hw, addsrc=addd)
        bound = lambda w: wino_exactness_bound(family[:3], "dgrad", o.dy, w, g, addsrc=o.add_x)
    with switches(True):
        ref0 = dgrad_ref32(o.dy, o.w, g, hw, addsrc=o.add_x)
        same(run(), dev(ref0, gpu), family + " before")
        w1 = o.w.clone()
        w1[g.co - 1, 5, 1, 1] += 1
        wd[1 * g.k + 1, g.co - 1, 5] += 1
        assert bound(w1) < TWO24
        ref1 = dgrad_ref32(o.dy, w1, g, hw, addsrc=o.add_x)
        assert not torch.equal(ref0, ref1)
        same(run(), dev(ref1, gpu), family + " after one more product")


@pytest.mark.parametrize("family", ["conv_wgrad", "c1_wgrad", "f23", "f32"])
def test_sensitivity_wgrad(gpu, family):
    """A weight gradient has no weight operand: +1 on one activation of the device copy (interior pixel, last channel)."""
    from gdn_amd import ops
    if family == "f23":
        g, bhw = f23_geom((128, 256, 2, 9, 13, False))
    elif family == "f32":
        g, bhw = Geom(64, 128, 4, 2, 1, True, False), (2, 10, 14)
    elif family == "c1_wgrad":
        g, bhw = Geom(1, 64, 9, 1, 4, True, False), (2, 16, 64)
    else:
        g, bhw = geom_of(_case("cb_k7s2_refl"))
    o = operands(g, bhw, "wide")
    op = ops.Conv(g.ci, g.co, g.k, g.s, g.p, reflect=g.refl)
    xd, gyd, wd = dev(o.x, gpu), dev(o.dy, gpu), taps(o.w, False).to(gpu)

    def run():
        dw = torch.full((g.k * g.k, g.co, g.ci), float("nan"), device=gpu)
        if family == "conv_wgrad":
            op.wgrad(xd, gyd, dw)
        elif family == "c1_wgrad":
            ops.conv_c1_wgrad(xd, gyd, dw, reflect=True)
        elif family == "f23":
            op.wino_bwd(gyd, wd, bhw[1:], state=op.wino_fwd(xd, wd, state=True)[1], dw_tap=dw, need_dx=False)
        else:
            op.wino2_bwd(gyd, wd, bhw[1:], state=op.wino2_fwd(xd, wd, state=True)[1], dw_tap=dw, need_dx=False)
        return dw
    bound = (lambda x: wino_exactness_bound(family, "wgrad", x, o.dy, g)) if family in ("f23", "f32") else (lambda x: exactness_bound(x, o.dy, 1.0, g, mode="wgrad"))
    with switches(True):
        ref0 = wgrad_ref(o.x, o.dy, g)
        same(run(), taps(ref0, False).to(gpu), family + " before")
        x1 = o.x.clone()
        b, h, w = bhw[0] - 1, bhw[1] // 2, bhw[2] // 2
        x1[b, g.ci - 1, h, w] += 1
        xd[b, h, w, g.ci - 1] += 1
        assert bound(x1) < TWO24
        ref1 = wgrad_ref(x1, o.dy, g)
        assert not torch.equal(ref0, ref1)
        same(run(), taps(ref1, False).to(gpu), family + " after one more product")


# ---------------------------------------------------------------------------------------------------------------------------
# F(4x4,3x3) and the FFT path: not exact (points 5/8 and 3/2 with non-dyadic 1/N_p; irrational twiddles), but with integer
# operands the true result is an integer (a multiple of 1/16 behind the x2 loader): any structural error -- a stale tile, a
# wrong tap, a lost product -- moves an output by at least one spacing, rounding noise by far less.  The bar is the spacing
# itself: the result rounded to the grid equals the exact one and stays within a quarter spacing of it.  (float32 numpy models
# on the CPU: at most 0.005 for F(4x4,3x3) at 128 channels and 0.0013 for FFT 9x9/64 on the wide set.)
# ---------------------------------------------------------------------------------------------------------------------------
F4_CASES = [(512, 512, 2, 8, 26), (512, 512, 1, 16, 52), (128, 128, 2, 12, 15), (256, 128, 1, 7, 8), (128, 256, 3, 4, 4)]
# (Cin, Cout, k, B, H, W, reflect): tests/test_hip_fftconv.py CASES / REFLECT_CASES, the smaller ones of each tile plan
FFT_CASES = [(64, 64, 9, 2, 40, 70, False), (128, 128, 7, 2, 26, 52, False), (64, 128, 7, 1, 17, 33, False), (64, 64, 9, 1, 9, 12, False),
             (256, 128, 5, 1, 12, 24, False), (256, 256, 3, 1, 30, 17, False), (64, 64, 3, 2, 9, 31, True), (64, 128, 9, 1, 24, 48, True),
             (256, 128, 5, 1, 26, 52, True)]


def nearest(got, exact, what, spacing=1.0):
    """got on the device against the exact float64 NCHW result: equal after rounding to the grid, and within spacing / 4."""
    ref = dev(exact, got.device) if exact.dim() == 4 else exact.to(got.device)
    d = float((got - ref).abs().max())
    print("%s: max |got - exact| = %.3g (spacing %g, max |exact| %.0f)" % (what, d, spacing, float(ref.abs().max())))
    assert d < spacing / 4, "%s: off by %.3g" % (what, d)
    same((got / spacing).round() * spacing, ref, what + " rounded")
    return d


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", F4_CASES, ids=["c%d_%d_%dx%dx%d" % c for c in F4_CASES])
def test_f4_nearest_integer(gpu, case, kind):
    """F(4x4,3x3) (the plan on, every GEMM bf16 x 3): y, the two-stream pair backward (dx + addsrc and dw from the state), dx
    alone and dw alone."""
    from gdn_amd import ops
    from gdn_amd._lib import lib
    g, bhw = f23_geom(case + (False,))
    B, H, W = bhw
    o = operands(g, bhw, kind)
    assert exactness_bound(o.x, o.w, 1.0, g, addsrc=o.add_y) < TWO24              # (the exact results are fp32 values)
    xd, wd, gyd = dev(o.x, gpu), taps(o.w, False).to(gpu), dev(o.dy, gpu)
    what = "F(4x4,3x3) %dx%d %dx%dx%d %s" % (case + (kind,))
    with switches(True, f4=True):
        op = ops.Conv(g.ci, g.co, 3, 1, 1)
        y, st, sv = op.wino_fwd(xd, wd, stats=True, state=True)
        assert st.shape[0] == cdiv(B * cdiv(H, 4) * cdiv(W, 4), 4), "not the F(4x4,3x3) plan"
        assert int(lib.gdn_winoconv_bwd_pair_workspace_bytes(op.geom(B, H, W)[1])) > 0
        nearest(y, conv(o.x, o.w, g), what + " y")
        dw_ref = taps(wgrad_ref(o.x, o.dy, g), False)
        dw = torch.full_like(wd, float("nan"))
        dx = op.wino_bwd(gyd, wd, (H, W), state=sv, dw_tap=dw, addsrc=dev(o.add_x, gpu))       # the pair: two streams
        nearest(dx, dgrad_ref32(o.dy, o.w, g, (H, W), addsrc=o.add_x), what + " pair dx")
        nearest(dw, dw_ref, what + " pair dw")
        nearest(op.wino_bwd(gyd, wd, (H, W)), dgrad_ref32(o.dy, o.w, g, (H, W)), what + " dx alone")
        dw2 = torch.full_like(wd, float("nan"))
        op.wino_bwd(gyd, wd, (H, W), state=sv, dw_tap=dw2, need_dx=False)
        nearest(dw2, dw_ref, what + " dw alone")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", FFT_CASES, ids=["c%d_%d_k%d_%dx%dx%d%s" % (c[:6] + ("_refl" if c[6] else "",)) for c in FFT_CASES])
def test_fft_nearest_integer(gpu, case, kind):
    """The frequency-domain path: forward, fft_bwd's dx (+ addsrc, with and without the saved spectra) and dw; zero and
    reflection border."""
    from gdn_amd import ops
    ci, co, k, B, H, W, refl = case
    g = Geom(ci, co, k, 1, k // 2, refl, False)
    o = operands(g, (B, H, W), kind)
    assert exactness_bound(o.x, o.w, 1.0, g, addsrc=o.add_y) < TWO24 and exactness_bound(o.x, o.dy, 1.0, g, mode="wgrad") < TWO24
    xd, wd, gyd = dev(o.x, gpu), taps(o.w, False).to(gpu), dev(o.dy, gpu)
    what = "FFT %dx%d k%d %dx%dx%d%s %s" % (case[:6] + (" reflect" if refl else "", kind))
    op = ops.Conv(ci, co, k, 1, k // 2, reflect=refl)
    assert op.fft_ok(B, H, W, backward=True)
    y, xf = op.fft_fwd(xd, wd, spectrum=True)
    nearest(y, conv(o.x, o.w, g), what + " y")
    dw = torch.full_like(wd, float("nan"))
    dx = op.fft_bwd(gyd, wd, (H, W), xf=xf, dw_tap=dw, addsrc=dev(o.add_x, gpu))
    nearest(dx, dgrad_ref32(o.dy, o.w, g, (H, W), addsrc=o.add_x), what + " dx")
    nearest(dw, taps(wgrad_ref(o.x, o.dy, g), False), what + " dw")
    nearest(op.fft_bwd(gyd, wd, (H, W)), dgrad_ref32(o.dy, o.w, g, (H, W)), what + " dx without spectra")


@pytest.mark.parametrize("kind", KINDS)
def test_fft_up2x_nearest_sixteenth(gpu, kind):
    """up2x = 1 on a reflection layer: the loader's weights are sixteenths, so y and dw live on the 1/16 grid; dx (fold + adjoint
    of the integer padded gradient) too."""
    from gdn_amd import ops
    ci, co, k, B, Hl, Wl = 128, 64, 7, 2, 10, 17
    H, W = 2 * Hl, 2 * Wl
    g = Geom(ci, co, k, 1, k // 2, True, False)
    lo, o = operands(g, (B, Hl, Wl), kind), operands(g, (B, H, W), kind)
    xin = _up(lo.x)
    assert exactness_bound(xin, o.w, 1.0 / 16, g) < TWO24 and exactness_bound(xin, o.dy, 1.0 / 16, g, mode="wgrad") < TWO24
    assert exactness_bound(o.dy, o.w, 1.0 / 16, g, mode="dgrad", in_hw=(H, W), addsrc=lo.add_x, up2x=1) < TWO24
    op = ops.Conv(ci, co, k, 1, k // 2, reflect=True)
    wd, gyd = taps(o.w, False).to(gpu), dev(o.dy, gpu)
    y, xf = op.fft_fwd(dev(lo.x, gpu), wd, spectrum=True, up2x=1)
    nearest(y, conv(xin, o.w, g), "FFT up2x y " + kind, 1.0 / 16)
    dw = torch.full_like(wd, float("nan"))
    dx = op.fft_bwd(gyd, wd, (H, W), xf=xf, dw_tap=dw, addsrc=dev(lo.add_x, gpu), up2x=1)
    nearest(dx, dgrad_ref32(o.dy, o.w, g, (H, W), addsrc=lo.add_x, up2x=1), "FFT up2x dx " + kind, 1.0 / 16)
    nearest(dw, taps(wgrad_ref(xin, o.dy, g), False), "FFT up2x dw " + kind, 1.0 / 16)


def test_fft_wide_rows_nearest_integer(gpu):
    """Rows wider than the gather pass's table (1024 pixels): the two-kernel inverse of the data gradient, no BatchNorm partials."""
    from gdn_amd import ops
    C, k, B, H, W = 64, 9, 1, 12, 1060
    g = Geom(C, C, k, 1, k // 2, False, False)
    gen = torch.Generator().manual_seed(5)
    dy, w, add = [torch.randint(-8, 9, s, generator=gen).double() for s in ((B, C, H, W), (C, C, k, k), (B, C, H, W))]
    assert exactness_bound(dy, w, 1.0, g, mode="dgrad", in_hw=(H, W), addsrc=add) < TWO24
    op = ops.Conv(C, C, k, 1, k // 2)
    assert op.fft_ok(B, H, W, backward=True) and op.fft_bnb_slots(B, H, W) == 0
    dx = op.fft_bwd(dev(dy, gpu), taps(w, False).to(gpu), (H, W), addsrc=dev(add, gpu))
    nearest(dx, dgrad_ref32(dy, w, g, (H, W), addsrc=add), "FFT wide rows dx")
