"""The bf16 convolution kernels against exact integer results: every comparison is torch.equal.

bf16 x bf16 products are exact in fp32 and fp32 sums of integers below 2^24 are exact in any order, so with integer-valued
operands the only rounding left is the kernels' bf16 store, and the result is bf16_rne(exact integer convolution)
(tests/int_conv_ref.py: the float64 reference, its rounding points and the operand sets).  Each test first asserts
exactness_bound(...) < 2^24 -- no summation order can round in fp32 -- then compares bit for bit: one missing or doubled
product, one stale LDS slab, a tail slab added twice or truncation in place of round-to-nearest-even all fail here, where the
Gaussian-operand bars of tests/test_hip_bf16.py let them pass.  Shapes are that file's (BF16_CASES, the GDN_RING_CUS=16 plans of
the ring tests and of the BatchNorm-backward test); every case runs the narrow and the wide operand set.
"""
import pytest
import torch

from int_conv_ref import (TWO24, Geom, bf16_rne, bnb_ref, dgrad_ref, exactness_bound, fwd_ref, geom_of, operands, out_hw,
                          stats_ref, wgrad_ref)
from test_hip_bf16 import BF16_CASES
from test_hip_kernels import nhwc, tapmajor

pytestmark = pytest.mark.gpu

KINDS = ("narrow", "wide")
# tile ids of gdn_conv_fwd / gdn_conv_dgrad: 0 automatic, 1-3 conv_igemm_bf16, 8/9 row-patch, 10/11 conv_ring_bf16, 12 conv_ring2_bf16
# (an id that does not accept the geometry runs the automatic choice); 0x800: single stage -- no tap split, no K-split tail
IDS = (0, 1, 2, 3, 8, 9, 10, 11, 12)
# (name, Cin, Cout, k, pad, reflect, B, H, W): the shapes of test_ring_kernel_rounds_and_tail_split (ids 10 / 11) and of
# test_ring2_kernel_rounds_and_tail_split (id 12), planned for a 16-CU chip: full rounds + a K-split tail
RING_CASES = [("k7_128", 128, 128, 7, 3, False, 2, 36, 64), ("k3_256", 256, 256, 3, 1, False, 3, 16, 48),
              ("k5_refl", 128, 64, 5, 2, True, 2, 36, 64), ("k9_64", 64, 64, 9, 4, False, 1, 72, 64)]
RING2_CASES = [("k7_128", 128, 128, 7, 3, False, 2, 36, 64), ("k3_256", 256, 256, 3, 1, False, 3, 16, 48),
               ("k5_refl", 128, 64, 5, 2, True, 4, 34, 64), ("k9_64", 64, 64, 9, 4, False, 2, 68, 64),
               ("k9_wide", 64, 64, 9, 4, False, 1, 21, 416)]
RING_TAIL = [(c, (10, 11)) for c in RING_CASES] + [(c, (12,)) for c in RING2_CASES]
# ((name, Cin, Cout, k, B, H, W), GDN_RING_CUS, tile id): test_ring_dgrad_emits_batchnorm_backward_partials
BNB_CASES = [(("bnb_k3_l3", 128, 128, 3, 2, 16, 52), 0, 0), (("bnb_k9_64", 64, 64, 9, 2, 24, 64), 0, 0),
             (("bnb_k5_tail", 64, 64, 5, 4, 17, 64), 16, 0), (("bnb_k7_relu_off", 64, 128, 7, 1, 16, 40), 0, 0),
             (("bnb_k9_64_ring2", 64, 64, 9, 2, 24, 64), 0, 12), (("bnb_k7_tail_ring2", 64, 64, 7, 8, 17, 64), 16, 12),
             (("bnb_k5_128_ring2", 128, 64, 5, 3, 20, 52), 0, 12)]
UP2X_CASE = ("up2x_k7_refl", 128, 64, 7, 1, 3, True, False, 2, 12, 20)      # H, W: the upsampled extent = the layer's input
HEAD_SHAPE = (1, 24, 52)                                                     # ragged: 52 is no multiple of the 16-column strips
# weight bits -> density of the non-zero activations.  17: the issue's weights m * 2^-17 -- two round-to-nearest bf16 terms already
# hold 17 significant bits (8 + 8 and a sign bit of the remainder), so the kernel's third term is zero for them; 20: m * 2^-20,
# sparser, so that the third term carries bits as well
HEAD_SETS = {17: 0.02, 20: 0.0012}


def ring_case(c):
    """A ring-test case in BF16_CASES form."""
    name, ci, co, k, p, refl, B, H, W = c
    return (name, ci, co, k, 1, p, refl, False, B, H, W)


def bnb_geom(c):
    name, ci, co, k, B, H, W = c
    return Geom(ci, co, k, 1, k // 2, False, False), (B, H, W)


def affine(co, seed=5):
    """ep_scale in {-1, 1/2, 1, 2} per channel, integer ep_shift: with integer accumulators the epilogue's granule is 1/2."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([-1.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (co,), generator=g)]
    return scale, torch.randint(-8, 9, (co,), generator=g).float()


def bnb_inputs(g, bhw, seed=9):
    """The producer's raw output y (integers), and scale (power of two), shift, mean (integers), invstd (power of two)."""
    gen = torch.Generator().manual_seed(seed)
    B, H, W = bhw
    y = torch.randint(-3, 4, (B, g.ci, H, W), generator=gen).double()
    p2 = torch.tensor([0.5, 1.0, 2.0])
    coef = torch.stack([p2[torch.randint(0, 3, (g.ci,), generator=gen)], torch.randint(-2, 3, (g.ci,), generator=gen).float(),
                        torch.randint(-1, 2, (g.ci,), generator=gen).float(), p2[torch.randint(0, 3, (g.ci,), generator=gen)]])
    return y, coef


def head_operands(tr, bits=17, seed=13):
    """Sparse {-1, 0, 1} activations and weights m * 2^-bits, |m| < 2^bits; torch layouts, float64."""
    gen = torch.Generator().manual_seed(seed + bits)
    B, H, W = HEAD_SHAPE
    x = torch.randint(-1, 2, (B, 64, H, W), generator=gen).double() * (torch.rand(B, 64, H, W, generator=gen) < HEAD_SETS[bits])
    m = torch.randint(-(2 ** bits) + 1, 2 ** bits, (64, 1, 9, 9) if tr else (1, 64, 9, 9), generator=gen).double()
    return x, m * 2.0 ** -bits


def head_corr(w, tr):
    """The head's weight as the 'same' correlation kernel [1, 64, 9, 9] it applies (a ConvTranspose2d flips the taps)."""
    return torch.flip(w.permute(1, 0, 2, 3), (2, 3)) if tr else w


def bf(t, gpu):
    """NCHW float64 holding bf16 values -> the device's NHWC bfloat16 tensor (exact)."""
    return nhwc(t).float().to(gpu).bfloat16()


def taps(w, tr):
    return tapmajor(w.float(), tr)                       # [k*k, Cout, Cin]


def taps_t(w, tr):
    return taps(w, tr).transpose(1, 2).contiguous()      # [k*k, Cin, Cout]: the data gradient's layout


def same(got, ref, what):
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s (got %r, exact %r), channels %s" % (
            what, bad.shape[0], ref.numel(), i, float(got[i]), float(ref[i]), sorted(set(bad[:, -1].tolist()))[:16]))


def check_stats(st, raw, kind, what):
    """The slots, summed in float64, against the raw accumulators: sum y and sum y^2 exactly on the narrow set (sum y^2 < 2^24
    by construction), sum y alone on the wide set and only for channels whose sum |y| stays below 2^24."""
    s = st.double().sum(0).cpu()
    s1, s2 = stats_ref(raw)
    if kind == "narrow":
        assert float(s2.max()) < TWO24
        assert torch.equal(s[0], s1) and torch.equal(s[1], s2), what + " statistics"
    else:
        ok = raw.abs().sum((0, 2, 3)) < TWO24
        assert torch.equal(s[0][ok], s1[ok]), what + " statistics (sum)"


def run_fwd(gpu, case, kind, ids, expect_split=()):
    """Forward of one layer over tile ids x {split allowed, single stage}: y, statistics, and the full epilogue."""
    from gdn_amd import ops
    g, bhw = geom_of(case)
    o = operands(g, bhw, kind)
    scale, shift = affine(g.co)
    assert exactness_bound(o.x, o.w, 1.0, g, addsrc=o.add_y) < TWO24
    assert exactness_bound(o.x, o.w, 0.5, g, scale=scale, shift=shift, addsrc=o.add_y) < TWO24
    y_ref, raw = fwd_ref(o.x, o.w, g)
    y_add = fwd_ref(o.x, o.w, g, addsrc=o.add_y, raw=raw)[0]
    y_ep = fwd_ref(o.x, o.w, g, scale, shift, True, o.add_y, raw=raw)[0]
    y_ref, y_add, y_ep = [bf(t, gpu) for t in (y_ref, y_add, y_ep)]
    xd, wd, addd = bf(o.x, gpu), taps(o.w, g.tr).to(gpu).bfloat16(), bf(o.add_y, gpu)
    aff = (scale.to(gpu), shift.to(gpu))
    slots = {}
    for cfg in ids:
        for single in (0, 0x800):
            op = ops.Conv(g.ci, g.co, g.k, g.s, g.p, reflect=g.refl, transposed=g.tr)
            what = "%s %s fwd id %d%s" % (case[0], kind, cfg, " single" if single else "")
            y, st = op.fwd(xd, wd, stats=True, tile_cfg=cfg | single)
            same(y, y_ref, what)
            check_stats(st, raw, kind, what)
            slots[(cfg, single)] = st.shape[0]
            same(op.fwd(xd, wd, addsrc=addd, tile_cfg=cfg | single), y_add, what + " + addsrc")
            same(op.fwd(xd, wd, act=ops.ACT_RELU, addsrc=addd, affine=aff, tile_cfg=cfg | single), y_ep, what + " affine relu addsrc")
    for cfg in expect_split:
        assert slots[(cfg, 0)] != slots[(cfg, 0x800)], "%s id %d: the split did not happen (same slot count)" % (case[0], cfg)
    return slots


def run_dgrad(gpu, case, kind, ids):
    from gdn_amd import ops
    g, bhw = geom_of(case)
    o = operands(g, bhw, kind)
    hw = bhw[1:]
    assert exactness_bound(o.dy, o.w, 1.0, g, mode="dgrad", in_hw=hw, addsrc=o.add_x) < TWO24
    ref0 = bf(dgrad_ref(o.dy, o.w, g, hw), gpu)
    ref1 = bf(dgrad_ref(o.dy, o.w, g, hw, addsrc=o.add_x), gpu)
    gyd, wt, addd = bf(o.dy, gpu), taps_t(o.w, g.tr).to(gpu).bfloat16(), bf(o.add_x, gpu)
    for cfg in ids:
        for single in (0, 0x800):
            op = ops.Conv(g.ci, g.co, g.k, g.s, g.p, reflect=g.refl, transposed=g.tr)
            what = "%s %s dgrad id %d%s" % (case[0], kind, cfg, " single" if single else "")
            same(op.dgrad(gyd, wt, hw, addsrc=addd, tile_cfg=cfg | single), ref1, what + " + addsrc")
            if cfg == 0:
                same(op.dgrad(gyd, wt, hw, tile_cfg=single), ref0, what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_fwd_exact(gpu, case, kind):
    """y bitwise the reference -- hence bitwise the same across every tile id -- with the tap split of ids 1-3 on and off."""
    slots = run_fwd(gpu, case, kind, IDS)
    if case[0] == "rb_k3_512":        # 416 pixels: 4-7 tiles per channel tile, so ids 1-3 cut the nine taps three ways
        B, H, W = case[-3:]
        for cfg in (1, 2, 3):
            assert slots[(cfg, 0)] == -(-B * H * W // 16) != slots[(cfg, 0x800)], "id %d: no tap split" % cfg


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_dgrad_exact(gpu, case, kind):
    """Stride 1, stride 2 and transposed layers with addsrc; reflection layers against the two-rounding model."""
    run_dgrad(gpu, case, kind, IDS)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case,ids", RING_TAIL, ids=["%s_id%d" % (c[0], i[0]) for c, i in RING_TAIL])
def test_ring_tail_exact(gpu, case, ids, kind, monkeypatch):
    """The persistent kernels over several rounds with the last round's units cut along K (16-CU plan) and with the cut off:
    the fp32 slabs splitk_combine_kernel sums are integers, so the tail changes no bit of y, of the statistics or of dx."""
    monkeypatch.setenv("GDN_RING_CUS", "16")
    c = ring_case(case)
    ids = tuple(i for i in ids if c[2] % (128 if i == 11 else 64) == 0)
    run_fwd(gpu, c, kind, ids, expect_split=ids)
    run_dgrad(gpu, c, kind, ids)


@pytest.mark.parametrize("kind", KINDS)
def test_fwd_concat_exact(gpu, kind):
    """The fused concat of a 1x1 layer: x2 a channel slice of a wider tensor, integer addsrc, ids 0-3."""
    from gdn_amd import ops
    case = next(c for c in BF16_CASES if c[0] == "cb_k1")
    g, bhw = geom_of(case)
    o = operands(g, bhw, kind)
    assert exactness_bound(o.x, o.w, 1.0, g, addsrc=o.add_y) < TWO24
    ref = bf(fwd_ref(o.x, o.w, g, addsrc=o.add_y)[0], gpu)
    xd = bf(o.x, gpu)
    wide = torch.full(xd.shape[:3] + (96,), 7.0, device=gpu).bfloat16()
    wide[..., 16:80] = xd[..., 64:]
    a = xd[..., :64].contiguous()
    wd, addd = taps(o.w, False).to(gpu).bfloat16(), bf(o.add_y, gpu)
    for cfg in (0, 1, 2, 3):
        for single in (0, 0x800):
            y = ops.Conv(g.ci, g.co, 1).fwd(a, wd, x2=wide[..., 16:80], addsrc=addd, tile_cfg=cfg | single)
            same(y, ref, "concat %s id %d single %d" % (kind, cfg, single))


@pytest.mark.parametrize("kind", KINDS)
def test_dgrad_fold_up2x_exact(gpu, kind):
    """dx_up2x = 1: the fold pass applies the adjoint of the x2 bilinear interpolation (weights in sixteenths) between the two
    roundings.  Mode 2 (align_corners) has weights that are no dyadic fractions and stays with tests/test_hip_up2x.py."""
    from gdn_amd import ops
    g, bhw = geom_of(UP2X_CASE)
    o = operands(g, bhw, kind)
    B, H, W = bhw
    gen = torch.Generator().manual_seed(4)
    a = 8 if kind == "wide" else 1
    add = torch.randint(-a, a + 1, (B, g.ci, H // 2, W // 2), generator=gen).double()
    assert exactness_bound(o.dy, o.w, 1.0 / 16, g, mode="dgrad", in_hw=(H, W), addsrc=add, up2x=1) < TWO24
    ref = bf(dgrad_ref(o.dy, o.w, g, (H, W), addsrc=add, up2x=1), gpu)
    gyd, wt = bf(o.dy, gpu), taps_t(o.w, False).to(gpu).bfloat16()
    for cfg in (0, 1, 10):
        op = ops.Conv(g.ci, g.co, g.k, 1, g.p, reflect=True)
        same(op.dgrad(gyd, wt, (H, W), addsrc=bf(add, gpu), tile_cfg=cfg, up2x=1), ref, "up2x fold %s id %d" % (kind, cfg))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case,cus,cfg", BNB_CASES, ids=[c[0][0] for c in BNB_CASES])
def test_dgrad_bnb_exact(gpu, case, cus, cfg, kind, monkeypatch):
    """The BatchNorm-backward partials of the data-gradient epilogue (ids 0 and 12, with and without the K-split tail): dx is
    unchanged bit for bit, and the slots add up to sum dz and sum dz * xhat exactly."""
    from gdn_amd import ops
    if cus:
        monkeypatch.setenv("GDN_RING_CUS", str(cus))
    g, bhw = bnb_geom(case)
    B, H, W = bhw
    o = operands(g, bhw, kind)
    y, coef = bnb_inputs(g, bhw)
    relu = "relu_off" not in case[0]
    assert exactness_bound(o.dy, o.w, 1.0, g, mode="dgrad", in_hw=(H, W), addsrc=o.add_x) < TWO24
    dx_ref = dgrad_ref(o.dy, o.w, g, (H, W), addsrc=o.add_x)
    s1, s2, chunk = bnb_ref(dx_ref, y, coef, relu)
    assert chunk / 0.5 < TWO24            # dz, y - mean: integers; invstd in {1/2, 1, 2}: granule 1/2
    dx_ref = bf(dx_ref, gpu)
    gyd, wt, addd, yd, cd = bf(o.dy, gpu), taps_t(o.w, False).to(gpu).bfloat16(), bf(o.add_x, gpu), bf(y, gpu), coef.to(gpu)
    counts = []
    for single in (0, 0x800) if cus else (0,):
        op = ops.Conv(g.ci, g.co, g.k, 1, g.k // 2)
        slots = op.dgrad_bnb_slots(B, H, W, torch.bfloat16, tile_cfg=cfg | single)
        assert slots > 0
        counts.append(slots)
        what = "%s %s single %d" % (case[0], kind, single)
        same(op.dgrad(gyd, wt, (H, W), addsrc=addd, tile_cfg=cfg | single), dx_ref, what + " dx")
        part = torch.full((slots, 2, g.ci), float("nan"), device=gpu)
        same(op.dgrad(gyd, wt, (H, W), addsrc=addd, bnb=(yd, cd, relu, part), tile_cfg=cfg | single), dx_ref, what + " dx with bnb")
        s = part.double().sum(0).cpu()
        assert torch.equal(s[0], s1), what + ": sum dz"
        assert torch.equal(s[1], s2), what + ": sum dz * xhat"
    if cus:
        assert counts[0] != counts[1], "the plan has no K-split tail"


def wgrad_cfgs(g):
    return (0, 1, 3) + ((4,) if g.s == 1 and not g.tr and g.k in (3, 5, 7, 9) else ())      # 4: wgrad_ring_bf16


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_wgrad_exact(gpu, case, kind):
    """conv_wgrad_bf16 (cfg 1, 3 and what 0 picks) and wgrad_ring_bf16 (cfg 4): dw is the integer result, in every cfg."""
    from gdn_amd import ops
    g, bhw = geom_of(case)
    o = operands(g, bhw, kind)
    assert exactness_bound(o.x, o.dy, 1.0, g, mode="wgrad") < TWO24
    ref = taps(wgrad_ref(o.x, o.dy, g), g.tr).to(gpu)
    xd, gyd = bf(o.x, gpu), bf(o.dy, gpu)
    op = ops.Conv(g.ci, g.co, g.k, g.s, g.p, reflect=g.refl, transposed=g.tr)
    for cfg in wgrad_cfgs(g):
        dw = torch.full(ref.shape, float("nan"), device=gpu)
        op.wgrad(xd, gyd, dw, cfg=cfg)
        same(dw, ref, "%s %s wgrad cfg %d" % (case[0], kind, cfg))


@pytest.mark.parametrize("kind", KINDS)
def test_wgrad_concat_halves_exact(gpu, kind):
    """The two halves of a concat 1x1 layer's weight gradient, the second from a slice of a wider tensor, written at ci_off."""
    from gdn_amd import ops
    case = next(c for c in BF16_CASES if c[0] == "cb_k1")
    g, bhw = geom_of(case)
    o = operands(g, bhw, kind)
    assert exactness_bound(o.x, o.dy, 1.0, g, mode="wgrad") < TWO24
    ref = taps(wgrad_ref(o.x, o.dy, g), False).to(gpu)
    xd, gyd = bf(o.x, gpu), bf(o.dy, gpu)
    wide = torch.full(xd.shape[:3] + (96,), 7.0, device=gpu).bfloat16()
    wide[..., 16:80] = xd[..., 64:]
    a = xd[..., :64].contiguous()
    op = ops.Conv(g.ci, g.co, 1)
    for cfg in (0, 1, 3):
        dw = torch.full(ref.shape, float("nan"), device=gpu)
        op.wgrad(a, gyd, dw, 0, cfg=cfg)
        op.wgrad(wide[..., 16:80], gyd, dw, 64, cfg=cfg)
        same(dw, ref, "concat wgrad %s cfg %d" % (kind, cfg))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H,W,reflect,flip", [(2, 16, 64, True, False), (1, 13, 45, False, True)], ids=["first_layer", "head"])
def test_wgrad_c1_mixed_exact(gpu, B, H, W, reflect, flip, kind):
    """gdn_conv_c1_wgrad with gw_bf16: a dense fp32 one-channel image against 64 bf16 channels -- the first layer's weight
    gradient (reflection) and a Conv2d head's (the one-channel d(pre-tanh) is the image, taps flipped)."""
    from gdn_amd import ops
    a = 8 if kind == "wide" else 1
    gen = torch.Generator().manual_seed(B * 100 + W)
    x1 = torch.randint(-a, a + 1, (B, 1, H, W), generator=gen).double()
    gw = torch.randint(-a, a + 1, (B, 64, H, W), generator=gen).double()
    g = Geom(1, 64, 9, 1, 4, reflect, False)
    assert exactness_bound(x1, gw, 1.0, g, mode="wgrad") < TWO24
    dw = wgrad_ref(x1, gw, g)                                           # [64, 1, 9, 9]
    if flip:
        dw = torch.flip(dw, (2, 3))
    ref = dw.permute(2, 3, 0, 1).reshape(81, 64).float().to(gpu)
    out = torch.full((81, 64), float("nan"), device=gpu)
    ops.conv_c1_wgrad(nhwc(x1).float().to(gpu), bf(gw, gpu), out, reflect=reflect, flip=flip)
    same(out, ref, "c1 wgrad with bf16 gw, %s" % kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tr", [False, True], ids=["conv", "convT"])
def test_wgrad_head_mixed_exact(gpu, tr, kind):
    """The head's weight gradient through gdn_conv_wgrad: bf16 x, fp32 one-channel dy."""
    from gdn_amd import ops
    a = 8 if kind == "wide" else 1
    gen = torch.Generator().manual_seed(31)
    B, H, W = 2, 16, 24
    x = torch.randint(-a, a + 1, (B, 64, H, W), generator=gen).double()
    dy = torch.randint(-a, a + 1, (B, 1, H, W), generator=gen).double()
    g = Geom(64, 1, 9, 1, 4, False, tr)
    assert exactness_bound(x, dy, 1.0, g, mode="wgrad") < TWO24
    ref = taps(wgrad_ref(x, dy, g), tr).to(gpu)                         # [81, 1, 64]
    dw = torch.full(ref.shape, float("nan"), device=gpu)
    ops.Conv(64, 1, 9, 1, 4, transposed=tr).wgrad(bf(x, gpu), nhwc(dy).float().to(gpu), dw)
    same(dw, ref, "head wgrad tr=%s %s" % (tr, kind))


@pytest.mark.parametrize("bits", sorted(HEAD_SETS), ids=lambda b: "w%dbit" % b)
@pytest.mark.parametrize("tr", [False, True], ids=["conv", "convT_ragged"])
def test_head_exact(gpu, tr, bits):
    """conv_head_mfma_bf16_kernel: bf16 activations, fp32 weights m * 2^-17 (and m * 2^-20, which reach the third term of the
    kernel's weight split) -- the fp32 depth map is bitwise the float64 result."""
    import torch.nn.functional as F
    from gdn_amd import ops
    x, w = head_operands(tr, bits)
    assert exactness_bound(x, head_corr(w, tr), 2.0 ** -bits) * (1 + 2.0 ** -6) < TWO24    # (+ the split's |w1| + |w2| + |w3| >= |w|)
    ref = F.conv_transpose2d(x, w, None, 1, 4) if tr else F.conv2d(x, w, None, 1, 4)
    assert torch.equal(ref.float().double(), ref)
    y = ops.Conv(64, 1, 9, 1, 4, transposed=tr).fwd(bf(x, gpu), taps(w, tr).to(gpu))
    assert y.dtype == torch.float32
    same(y, nhwc(ref).float().to(gpu), "bf16 head tr=%s, %d-bit weights" % (tr, bits))


# ---------------------------------------------------------------------------------------------------------------------------
# Sensitivity, once per kernel family: one more product must move the result -- to exactly the recomputed reference
# ---------------------------------------------------------------------------------------------------------------------------
def _case(name):
    return next(c for c in BF16_CASES if c[0] == name)


@pytest.mark.parametrize("family,name,cfg", [("igemm", "cb_k4s2_refl", 3), ("rowpatch", "rp_k5", 9), ("ring", "rb_k9_64", 10),
                                             ("ring2", "rp_k9_64", 12)], ids=lambda v: v if isinstance(v, str) else "id%d" % v)
def test_sensitivity_fwd(gpu, family, name, cfg):
    """After the exact check, +1 on one weight of the device copy -- an interior tap, the last channel of the last slab: the
    output must be bitwise the reference of the changed weights, and that reference differs from the first."""
    from gdn_amd import ops
    case = _case(name)
    g, bhw = geom_of(case)
    o = operands(g, bhw, "wide")
    op = ops.Conv(g.ci, g.co, g.k, g.s, g.p, reflect=g.refl, transposed=g.tr)
    xd, wd = bf(o.x, gpu), taps(o.w, g.tr).to(gpu).bfloat16()
    ref0 = fwd_ref(o.x, o.w, g)[0]
    y, st = op.fwd(xd, wd, stats=True, tile_cfg=cfg | 0x800)
    bm = {3: 64, 9: 256, 10: 256, 12: 512}[cfg]
    B, (Ho, Wo) = bhw[0], out_hw(g, *bhw[1:])
    assert st.shape[0] == -(-B * Ho * Wo // bm), "%s: tile id %d did not take this geometry" % (family, cfg)
    same(y, bf(ref0, gpu), family + " before")
    ky = kx = g.k // 2
    w1 = o.w.clone()
    w1[5, g.ci - 1, ky, kx] += 1
    wd[ky * g.k + kx, 5, g.ci - 1] += 1
    assert exactness_bound(o.x, w1, 1.0, g) < TWO24
    ref1 = fwd_ref(o.x, w1, g)[0]
    assert not torch.equal(ref0, ref1)
    same(op.fwd(xd, wd, tile_cfg=cfg | 0x800), bf(ref1, gpu), family + " after one more product")


def test_sensitivity_fold(gpu):
    """The same on the data gradient of a reflection layer (kernel + reflect_fold_kernel): the reduction runs over Cout."""
    from gdn_amd import ops
    case = _case("cb_k3s1_refl")
    g, bhw = geom_of(case)
    o = operands(g, bhw, "wide")
    hw = bhw[1:]
    op = ops.Conv(g.ci, g.co, g.k, g.s, g.p, reflect=True)
    gyd, wt, addd = bf(o.dy, gpu), taps_t(o.w, False).to(gpu).bfloat16(), bf(o.add_x, gpu)
    ref0 = dgrad_ref(o.dy, o.w, g, hw, addsrc=o.add_x)
    same(op.dgrad(gyd, wt, hw, addsrc=addd), bf(ref0, gpu), "fold before")
    w1 = o.w.clone()
    w1[g.co - 1, 5, 1, 1] += 1
    wt[4, 5, g.co - 1] += 1
    assert exactness_bound(o.dy, w1, 1.0, g, mode="dgrad", in_hw=hw, addsrc=o.add_x) < TWO24
    ref1 = dgrad_ref(o.dy, w1, g, hw, addsrc=o.add_x)
    assert not torch.equal(ref0, ref1)
    same(op.dgrad(gyd, wt, hw, addsrc=addd), bf(ref1, gpu), "fold after one more product")


@pytest.mark.parametrize("family,name,cfg", [("conv_wgrad_bf16", "cb_k7s2_refl", 1), ("wgrad_ring_bf16", "rb_k9_64", 4)],
                         ids=lambda v: v if isinstance(v, str) else "cfg%d" % v)
def test_sensitivity_wgrad(gpu, family, name, cfg):
    """A weight gradient has no weight operand: +1 on one activation of the device copy (interior pixel, last channel)."""
    from gdn_amd import ops
    case = _case(name)
    g, bhw = geom_of(case)
    o = operands(g, bhw, "wide")
    op = ops.Conv(g.ci, g.co, g.k, g.s, g.p, reflect=g.refl, transposed=g.tr)
    xd, gyd = bf(o.x, gpu), bf(o.dy, gpu)
    ref0 = wgrad_ref(o.x, o.dy, g)
    dw = torch.full((g.k * g.k, g.co, g.ci), float("nan"), device=gpu)
    op.wgrad(xd, gyd, dw, cfg=cfg)
    same(dw, taps(ref0, g.tr).to(gpu), family + " before")
    x1 = o.x.clone()
    b, h, w = bhw[0] - 1, bhw[1] // 2, bhw[2] // 2
    x1[b, g.ci - 1, h, w] += 1
    xd[b, h, w, g.ci - 1] += 1
    assert exactness_bound(x1, o.dy, 1.0, g, mode="wgrad") < TWO24
    ref1 = wgrad_ref(x1, o.dy, g)
    assert not torch.equal(ref0, ref1)
    dw.fill_(float("nan"))
    op.wgrad(xd, gyd, dw, cfg=cfg)
    same(dw, taps(ref1, g.tr).to(gpu), family + " after one more product")


def test_sensitivity_head(gpu):
    """The same on the head: +1 on the centre tap's last channel (an 18-bit weight, still exact in three bf16 terms)."""
    import torch.nn.functional as F
    from gdn_amd import ops
    x, w = head_operands(False)
    x[0, 63, 12, 26] = 1.0                                  # (the changed weight must meet a non-zero activation)
    op = ops.Conv(64, 1, 9, 1, 4)
    xd, wd = bf(x, gpu), taps(w, False).to(gpu)
    ref0 = F.conv2d(x, w, None, 1, 4)
    same(op.fwd(xd, wd), nhwc(ref0).float().to(gpu), "head before")
    w1 = w.clone()
    w1[0, 63, 4, 4] += 1
    wd[40, 0, 63] += 1
    assert exactness_bound(x, w1, 2.0 ** -17) * (1 + 2.0 ** -6) < TWO24
    ref1 = F.conv2d(x, w1, None, 1, 4)
    assert not torch.equal(ref0, ref1) and torch.equal(ref1.float().double(), ref1)
    same(op.fwd(xd, wd), nhwc(ref1).float().to(gpu), "head after one more product")
