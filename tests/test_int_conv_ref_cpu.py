"""Checks of the exact-integer reference (tests/int_conv_ref.py) and of the operand sets tests/test_hip_bf16_exact.py feeds the
kernels; no GPU.  A bitwise test is only as good as its reference and its data: the reference is pinned to plain autograd and
to the oracle's bf16 emulation, and for every GPU case the conditions that make the result unique are verified -- the
exactness bound below 2^24, a narrow set on which nothing rounds, a wide set on which rounding (ties included) is exercised."""
import pytest
import torch

import int_conv_ref as R
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
