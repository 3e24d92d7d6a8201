"""Checks of the exact-integer reference (tests/int_conv_ref.py) and of the operand sets tests/test_hip_bf16_exact.py feeds the
kernels; no GPU.  A bitwise test is only as good as its reference and its data: the reference is pinned to plain autograd and
to the oracle's bf16 emulation, and for every GPU case the conditions that make the result unique are verified -- the
exactness bound below 2^24, a narrow set on which nothing rounds, a wide set on which rounding (ties included) is exercised."""
import pytest
import torch
import torch.nn.functional as F

import int_conv_ref as R
import test_hip_fp32_exact as X
from int_conv_ref import TWO24, exactness_bound, operands
from test_hip_bf16_exact import (BF16_CASES, BNB_CASES, RING2_CASES, RING_CASES, UP2X_CASE, HEAD_SETS, affine, bnb_geom, bnb_inputs,
                                 head_corr, head_operands, ring_case)

LAYER_CASES = list(BF16_CASES) + [ring_case(c) for c in RING_CASES] + [ring_case(c) for c in RING2_CASES if c not in RING_CASES]
LAYER_IDS = [c[0] for c in BF16_CASES] + ["ring_" + c[0] for c in RING_CASES] + ["ring2_" + c[0] for c in RING2_CASES if c not in RING_CASES]


def test_rounding_helpers():
    v = torch.tensor([255.0, 256.0, 257.0, 258.0, 259.0, 1028.0, 1032.0, 1036.0, -1028.0, 0.0, 3.0 / 16, 257.0 / 16])
    #                        tie->256      tie->260 tie->1024    tie->1040
    assert R.bf16_rne(v).tolist() == [255.0, 256.0, 256.0, 258.0, 260.0, 1024.0, 1032.0, 1040.0, -1024.0, 0.0, 3.0 / 16, 256.0 / 16]
    assert R.is_tie(v).tolist() == [False, False, True, False, True, True, False, True, True, False, False, True]
    assert R.is_bf16(v).tolist() == [True, True, False, True, False, False, True, False, False, True, True, False]


@pytest.mark.parametrize("case", [c for c in LAYER_CASES if c[6]] + [UP2X_CASE], ids=lambda c: c[0])
def test_reflection_model_is_autograd_when_nothing_rounds(case):
    """Narrow set: the two-rounding model of a reflection layer's data gradient (padded domain, fold) equals plain autograd
    through pad(mode='reflect') -> conv2d, with and without addsrc."""
    g, bhw = R.geom_of(case)
    o = operands(g, bhw, "narrow")
    hw = bhw[1:]
    assert torch.equal(R.dgrad_ref(o.dy, o.w, g, hw), R.dgrad_autograd(o.dy, o.w, g, hw))
    assert torch.equal(R.dgrad_ref(o.dy, o.w, g, hw, addsrc=o.add_x), R.dgrad_autograd(o.dy, o.w, g, hw, addsrc=o.add_x))
    # and on the wide set the workspace's rounding is visible: the model is not the single-rounding result everywhere
    o = operands(g, bhw, "wide")
    assert not torch.equal(R.dgrad_ref(o.dy, o.w, g, hw), R.bf16_rne(R.dgrad_autograd(o.dy, o.w, g, hw)))


def test_up2x_model_is_autograd_when_nothing_rounds():
    import torch.nn.functional as F
    g, (B, H, W) = R.geom_of(UP2X_CASE)
    o = operands(g, (B, H, W), "narrow")
    xl = torch.zeros(B, g.ci, H // 2, W // 2, dtype=torch.float64, requires_grad=True)
    up = F.interpolate(xl, scale_factor=2, mode="bilinear", align_corners=False)
    dx, = torch.autograd.grad(R.conv(up, o.w, g), xl, o.dy)
    got = R.dgrad_ref(o.dy, o.w, g, (H, W), up2x=1, rounded=False)
    assert torch.equal(got, dx) and torch.equal(got * 16, torch.round(got * 16))          # sixteenths


def test_reference_is_the_oracles_bf16_emulation():
    """The forward reference on the wide set == oracle.bf16_emulation's convolution (fp32 conv2d of the bf16 operands, result
    rounded where the HIP path stores it), which is exact here as well: the bound holds for fp32 on the CPU too."""
    from oracle import gdn_oracle as O
    case = next(c for c in BF16_CASES if c[0] == "rb_k9_64")
    g, bhw = R.geom_of(case)
    o = operands(g, bhw, "wide")
    assert exactness_bound(o.x, o.w, 1.0, g) < TWO24
    with O.bf16_emulation():
        y = O._conv(o.x.float(), o.w.float(), g.s, g.p)
    ref, raw = R.fwd_ref(o.x, o.w, g)
    assert torch.equal(y.double(), ref) and not torch.equal(ref, raw)


@pytest.mark.parametrize("case", LAYER_CASES, ids=LAYER_IDS)
def test_layer_case_data_conditions(case):
    g, bhw = R.geom_of(case)
    hw = bhw[1:]
    scale, shift = affine(g.co)
    for kind in ("narrow", "wide"):
        o = operands(g, bhw, kind)
        for t in o:
            assert bool(R.is_bf16(t).all())
        assert exactness_bound(o.x, o.w, 1.0, g, addsrc=o.add_y) < TWO24
        assert exactness_bound(o.x, o.w, 0.5, g, scale=scale, shift=shift, addsrc=o.add_y) < TWO24
        assert exactness_bound(o.dy, o.w, 1.0, g, mode="dgrad", in_hw=hw, addsrc=o.add_x) < TWO24
        assert exactness_bound(o.x, o.dy, 1.0, g, mode="wgrad") < TWO24
        raw = R.conv(o.x, o.w, g)
        if kind == "narrow":
            assert bool(o.w.abs().max() == 1) and float((o.w != 0).double().mean()) > 0.01
            assert bool(R.is_bf16(raw).all()) and bool(R.is_bf16(raw + o.add_y).all())
            assert float((raw * raw).sum((0, 2, 3)).max()) < TWO24
            dx = R.dgrad_autograd(o.dy, o.w, g, hw, addsrc=o.add_x)
            assert bool(R.is_bf16(dx).all()) and torch.equal(R.dgrad_ref(o.dy, o.w, g, hw, addsrc=o.add_x), dx)
        else:
            inexact = float((~R.is_bf16(raw)).double().mean())
            ties = float(R.is_tie(raw).double().mean())
            print("%s: %.1f %% of outputs inexact, %.1f %% ties" % (case[0], 100 * inexact, 100 * ties))
            assert inexact >= 0.15 and ties >= 0.10


def test_up2x_case_bound():
    g, (B, H, W) = R.geom_of(UP2X_CASE)
    for kind, a in (("narrow", 1), ("wide", 8)):
        o = operands(g, (B, H, W), kind)
        add = torch.full((B, g.ci, H // 2, W // 2), float(a), dtype=torch.float64)
        assert exactness_bound(o.dy, o.w, 1.0 / 16, g, mode="dgrad", in_hw=(H, W), addsrc=add, up2x=1) < TWO24


@pytest.mark.parametrize("case,cus,cfg", BNB_CASES, ids=[c[0][0] for c in BNB_CASES])
def test_bnb_case_data_conditions(case, cus, cfg):
    g, bhw = bnb_geom(case)
    y, coef = bnb_inputs(g, bhw)
    assert bool((y == y.round()).all()) and bool((coef[1:3] == coef[1:3].round()).all())
    assert bool((torch.log2(coef[0]) == torch.log2(coef[0]).round()).all()) and bool((torch.log2(coef[3]) == torch.log2(coef[3]).round()).all())
    for kind in ("narrow", "wide"):
        o = operands(g, bhw, kind)
        assert exactness_bound(o.dy, o.w, 1.0, g, mode="dgrad", in_hw=bhw[1:], addsrc=o.add_x) < TWO24
        dx = R.dgrad_ref(o.dy, o.w, g, bhw[1:], addsrc=o.add_x)
        s1, s2, chunk = R.bnb_ref(dx, y, coef, "relu_off" not in case[0])
        assert chunk / 0.5 < TWO24 and bool((s2 * 2 == (s2 * 2).round()).all()) and float(s2.abs().max()) > 0


@pytest.mark.parametrize("bits", sorted(HEAD_SETS))
@pytest.mark.parametrize("tr", [False, True])
def test_head_case_data_conditions(tr, bits):
    x, w = head_operands(tr, bits)
    m = w * 2.0 ** bits
    assert bool((m == m.round()).all()) and float(m.abs().max()) < 2 ** bits and float((m.abs() >= 2 ** (bits - 1)).double().mean()) > 0.25
    assert torch.equal(w.float().double(), w) and bool(R.is_bf16(x).all())
    # the three-term split of the kernel (round to nearest bf16 of the remainder, three times) is exact.  17-bit weights are
    # used up by two terms (8 + 8 bits and the remainder's sign); the 20-bit set is there for the third
    t1 = R.bf16_rne(w)
    t2 = R.bf16_rne(w - t1)
    t3 = R.bf16_rne(w - t1 - t2)
    assert torch.equal(t1 + t2 + t3, w) and float((t2 != 0).double().mean()) > 0.9
    assert float((t3 != 0).double().mean()) > 0.5 if bits == 20 else not bool((t3 != 0).any())
    assert exactness_bound(x, head_corr(w, tr), 2.0 ** -bits) * (1 + 2.0 ** -6) < TWO24
    assert float((x != 0).sum()) > 40


# ---------------------------------------------------------------------------------------------------------------------------
# The fp32 path (tests/test_hip_fp32_exact.py): references, the float32 Winograd models, bounds of every GPU case
# ---------------------------------------------------------------------------------------------------------------------------
FP32_LAYER_CASES = list(X.WGRAD_CASES)


@pytest.mark.parametrize("case", FP32_LAYER_CASES, ids=[c[0] for c in FP32_LAYER_CASES])
def test_fp32_references_are_plain_autograd_and_bounds_hold(case):
    """fwd_ref32 / dgrad_ref32 against torch's float64 functions written out here, and the direct kernels' data conditions:
    every bound the GPU tests assert is below 2^24 on both operand sets."""
    g, bhw = R.geom_of(case)
    hw = bhw[1:]
    scale, shift = affine(g.co)
    for kind in ("narrow", "wide"):
        o = operands(g, bhw, kind)
        x = o.x.clone().requires_grad_(True)
        if g.tr:
            raw = F.conv_transpose2d(x, o.w, None, g.s, g.p)
        else:
            raw = F.conv2d(F.pad(x, (g.p,) * 4, mode="reflect") if g.refl else F.pad(x, (g.p,) * 4), o.w, None, g.s, 0)
        full = torch.relu(raw * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)) + o.add_y
        y, r = R.fwd_ref32(o.x, o.w, g, scale, shift, True, o.add_y)
        assert torch.equal(r, raw.detach()) and torch.equal(y, full.detach()) and torch.equal(R.fwd_ref32(o.x, o.w, g)[0], r)
        dx, = torch.autograd.grad(raw, x, o.dy)
        assert torch.equal(R.dgrad_ref32(o.dy, o.w, g, hw), dx) and torch.equal(R.dgrad_ref32(o.dy, o.w, g, hw, addsrc=o.add_x), dx + o.add_x)
        assert torch.equal(y.float().double(), y) and torch.equal(dx.float().double(), dx)          # fp32 holds the results
        assert exactness_bound(o.x, o.w, 1.0, g, addsrc=o.add_y) < TWO24
        assert exactness_bound(o.x, o.w, 0.5, g, scale=scale, shift=shift, addsrc=o.add_y) < TWO24
        assert exactness_bound(o.dy, o.w, 1.0, g, mode="dgrad", in_hw=hw, addsrc=o.add_x) < TWO24
        assert exactness_bound(o.x, o.dy, 1.0, g, mode="wgrad") < TWO24
        if kind == "narrow":
            assert float((r * r).sum((0, 2, 3)).max()) < TWO24                                      # statistics exact on every channel


def test_c1_case_bounds():
    for cin, B, H, W, reflect, flip in [(1, 2, 16, 64, True, False), (1, 1, 13, 45, False, True), (1, 2, 5, 7, True, True),
                                        (3, 2, 16, 64, True, False), (3, 1, 13, 45, False, False), (3, 2, 5, 7, True, False)]:
        g = R.Geom(cin, 64, 9, 1, 4, reflect, False)
        scale, shift = affine(64)
        for kind in ("narrow", "wide"):
            x, w, gy, add = X.c1_operands(cin, B, H, W, kind)
            assert exactness_bound(x, w, 0.5, g, scale=scale, shift=shift, addsrc=add) < TWO24
            assert exactness_bound(x, gy, 1.0, g, mode="wgrad") < TWO24


def _check_wino_case(scheme, g, bhw, kind):
    """One GPU case: the bound (the model on absolute operands and matrices) is below 2^24 and really bounds the float64
    model's intermediates, every transformed operand has at most 16 significant bits, and the float32 model is bitwise the
    float64 convolution (forward, data gradient -- padded domain and fold for a reflection layer --, weight gradient).  The
    512 -> 512 channel cases keep the bound and the predicate, which every GPU case needs, and leave the float32 run to the
    same shapes at fewer channels (seconds of numpy each)."""
    o = operands(g, bhw, kind)
    hw = bhw[1:]
    scale, shift = affine(g.co)
    extra = {"fwd": dict(scale=scale, shift=shift, addsrc=o.add_y), "dgrad": dict(addsrc=o.add_x), "wgrad": {}}      # as the GPU tests ask
    refs = {"fwd": lambda: R.conv(o.x, o.w, g), "dgrad": lambda: R.dgrad_autograd(o.dy, o.w, g, hw), "wgrad": lambda: R.wgrad_ref(o.x, o.dy, g)}
    for mode, a, b in (("fwd", o.x, o.w), ("dgrad", o.dy, o.w), ("wgrad", o.x, o.dy)):
        ref = refs[mode]()
        y64, big, transformed = R.wino_run(scheme, mode, a, b, g)
        bound = R.wino_exactness_bound(scheme, mode, a, b, g, **extra[mode])
        assert torch.equal(y64, ref) and big / 0.25 <= bound < TWO24, (scheme, mode, g, bhw, kind)
        assert R.at_most_16bit(transformed)
        if g.ci * g.co < 512 * 512:
            assert torch.equal(R.wino_run(scheme, mode, a, b, g, "float32")[0], ref), (scheme, mode, g, bhw, kind)


@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("case", X.F23_CASES, ids=[X.wino_id(c) for c in X.F23_CASES])
def test_f23_float32_model_is_exact_and_bounded(case, kind):
    g, bhw = X.f23_geom(case)
    _check_wino_case("f23", g, bhw, kind)
    o = operands(g, bhw, kind)
    for relu in (True, False):                                     # the producer's BatchNorm on load: halves, granule 1/8
        xin = R.layer_input(o.x, X.in_affine_of(g.ci), relu)
        assert torch.equal(xin * 2, (xin * 2).round()) and not torch.equal(xin, xin.round())
        y, _, transformed = R.wino_run("f23", "fwd", xin, o.w, g, "float32" if g.ci * g.co < 512 * 512 else "float64")
        assert torch.equal(y, R.conv(xin, o.w, g)) and R.at_most_16bit(transformed)
        assert R.wino_exactness_bound("f23", "fwd", xin, o.w, g, granule=0.125) < TWO24


@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("case", [(128, 256, 2, 9, 13, False), (256, 128, 1, 5, 6, False)], ids=X.wino_id)
def test_f23_flip_taps_model(case, kind):
    """A flip_taps layer is ConvTranspose2d(3, 1, 1): the model with the stored taps reversed and the channel roles swapped."""
    _check_wino_case("f23", *X.f23_geom(case, tr=True), kind)


@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("case", X.F23_UP2X, ids=[X.wino_id(c) for c in X.F23_UP2X])
def test_f23_up2x_model(case, kind):
    """The x2 bilinear loader adds a granule of 1/16 (1/64 in all): forward, and for reflection layers the fold + adjoint and the
    weight gradient against autograd through interpolate -> pad(reflect) -> conv2d."""
    ci, co, B, Hl, Wl, refl = case
    g = R.Geom(ci, co, 3, 1, 1, bool(refl), False)
    lo, o = operands(g, (B, Hl, Wl), kind), operands(g, (B, 2 * Hl, 2 * Wl), kind)
    xl = lo.x.clone().requires_grad_(True)
    w = o.w.clone().requires_grad_(True)
    xin = F.interpolate(xl, scale_factor=2, mode="bilinear", align_corners=False)
    y = R.conv(xin, w, g)
    dx, dw = torch.autograd.grad(y, (xl, w), o.dy)
    xin = xin.detach()
    assert torch.equal(xin, R.layer_input(lo.x, up2x=1)) and torch.equal(xin * 16, (xin * 16).round())
    assert torch.equal(R.wino_run("f23", "fwd", xin, o.w, g, "float32")[0], y.detach())
    assert R.wino_exactness_bound("f23", "fwd", xin, o.w, g, granule=1.0 / 64) < TWO24
    assert R.wino_operands_16bit("f23", "fwd", xin, o.w, g)
    if g.refl:
        assert torch.equal(R.dgrad_ref32(o.dy, o.w, g, (2 * Hl, 2 * Wl), up2x=1), dx)
        assert torch.equal(R.wino_run("f23", "dgrad", o.dy, o.w, g, "float32", up2x=1)[0], dx)
        assert torch.equal(R.wino_run("f23", "wgrad", xin, o.dy, g, "float32")[0], dw) and torch.equal(R.wgrad_ref(xin, o.dy, g), dw)
        assert R.wino_exactness_bound("f23", "dgrad", o.dy, o.w, g, granule=1.0 / 16, addsrc=lo.add_x, up2x=1) < TWO24
        assert R.wino_exactness_bound("f23", "wgrad", xin, o.dy, g, granule=1.0 / 64) < TWO24
        assert R.wino_operands_16bit("f23", "wgrad", xin, o.dy, g)


@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("case", X.F32_CASES, ids=[X.wino_id(c) for c in X.F32_CASES])
def test_f32_float32_model_is_exact_and_bounded(case, kind):
    tr = len(case) == 7
    ci, co, B, H, W = case[:5]
    g = R.Geom(ci, co, 4, 2, 1, bool(case[5]) and not tr, tr)
    _check_wino_case("f32", g, (B, H, W), kind)


def test_issue_example_f23_128_channels():
    """Integers in [-8, 8] at 128 -> 128 channels, 9 x 13: wino_forward(dtype=float32) is bitwise the float64 convolution."""
    import numpy as np
    from test_winoconv_model_cpu import wino_forward
    rng = np.random.default_rng(0)
    x, w = rng.integers(-8, 9, (128, 9, 13)).astype(np.float64), rng.integers(-8, 9, (128, 128, 3, 3)).astype(np.float64)
    ref = F.conv2d(torch.tensor(x)[None], torch.tensor(w), padding=1)[0].numpy()
    y, _ = wino_forward(x, w, dtype=np.float32)
    assert y.dtype == np.float32 and np.array_equal(y.astype(np.float64), ref) and np.abs(ref).max() > 2000


def test_sig_bits():
    import numpy as np
    assert R.sig_bits(np.array([0.0, 1.0, 3.0, 0.75, 255.0, 256.0])) == 8 and R.sig_bits(np.array([65535.0, 0.5])) == 16
    assert R.sig_bits(np.array([65537.0])) == 17 and R.sig_bits(np.zeros(3)) == 0 and R.sig_bits(np.array([1 + 2.0 ** -20])) == 21


@pytest.mark.parametrize("name", sorted(R.X3_PLANE_CASES))
def test_x3_plane_cases_need_their_planes(name):
    """The plane-wise emulation of the six-product sum: exact on the case, and wrong as soon as one of the products the case
    targets (hence the plane behind it) is lost -- so tests/test_hip_gemm_x3.py::test_gemm_x3_planes_exact cannot pass without."""
    A, B = R.x3_plane_case(name)
    ref = torch.bmm(A, B.transpose(1, 2))
    assert R.x3_bound(A, B, 1.0) < TWO24 and torch.equal(ref.float().double(), ref)
    assert torch.equal(A.float().double(), A) and torch.equal(B.float().double(), B)
    assert torch.equal(R.x3_six_products(A, B), ref)
    for prod in R.X3_PLANE_CASES[name]:
        assert not torch.equal(R.x3_six_products(A, B, drop=(prod,)), ref), prod
    pa, pb = R.x3_planes(A), R.x3_planes(B)
    if name == "a2b2":               # 16-bit operands: the third planes are empty, the three dropped products vanish
        assert not bool(pa[2].any()) and not bool(pb[2].any()) and bool(pa[1].any()) and bool(pb[1].any())
    else:
        big = pa if name == "a24_onehot" else pb
        assert float((big[2] != 0).double().mean()) > 0.5


def test_wgrad_cases_cover_the_segment_widths():
    """The conv_wgrad cases of the GPU file reach the row-segment widths 32, 52, 26 and two rows no width tiles (45 -> 46,
    13 -> 16), by X.wgrad_tw()'s restatement of make_plan() (csrc/conv_wgrad.hip; the library exports the plan's workspace size,
    not its width), and every plan the GPU test asserts a pixel split on has one, read from gdn_conv_wgrad_workspace_bytes."""
    from gdn_amd import ops
    tws = {c[0]: X.wgrad_tw(*R.geom_of(c)) for c in X.WGRAD_CASES}
    assert {tws["w32"], tws["rb_k3_l3"], tws["rb_k3_512"], tws["w45"], tws["w13"]} == {32, 52, 26, 46, 16}, tws
    assert tws["w52_rows"] == 52
    for c in X.WGRAD_CASES:
        g, bhw = R.geom_of(c)
        op = ops.Conv(g.ci, g.co, g.k, g.s, g.p, reflect=g.refl, transposed=g.tr)
        splits = X.wgrad_splits(op, g, bhw, g.ci)
        assert splits >= 1 and (splits > 1 or c[0] not in X.WGRAD_SPLIT_CASES)


@pytest.mark.parametrize("name", sorted(R.HEAD_PLANE_SETS))
@pytest.mark.parametrize("case", X.HEAD_CASES, ids=[c[0] for c in X.HEAD_CASES])
def test_head_plane_sets_need_their_planes(case, name):
    """The 64 -> 1 fp32 head's six-product sum on the plane sets of the GPU test: exact and within the bound, and wrong as soon
    as one of the products the set targets is lost."""
    g, bhw = R.geom_of(case)
    x, w = R.head_plane_operands(name, g, bhw)
    ref = R.conv(x, w, g)
    assert torch.equal(x.float().double(), x) and torch.equal(w.float().double(), w) and torch.equal(ref.float().double(), ref)
    assert float(R.x3_conv_six(x, w, g, absolute=True).max()) < TWO24 and torch.equal(R.x3_conv_six(x, w, g), ref)
    for prod in R.HEAD_PLANE_SETS[name]:
        assert not torch.equal(R.x3_conv_six(x, w, g, drop=(prod,)), ref), prod
    assert int((ref != 0).sum()) > 200


def test_head_valu_case_bounds():
    for case in X.HEAD_VALU_CASES:
        g, bhw = R.geom_of(case)
        for kind in ("narrow", "wide"):
            o = operands(g, bhw, kind)
            assert exactness_bound(o.x, o.w, 1.0, g) < TWO24
