"""GPU tests for training the legacy colour-to-depth AutoEncoder (reference AE_model_unet.py:96-261) on the HIP path:

  * its three stride-1 ConvTranspose2d decoder layers as flipped-tap convolutions (GDN_HINT_FLIP_TAPS, ops.Conv(flip_taps=True))
    through the frequency-domain and Winograd kernels, forward and backward, against F.conv_transpose2d autograd on the CPU;
  * engine.conv_plain's backward and one whole decoder stage against the oracle's functions;
  * one training step of the network against a CPU reference step assembled from oracle.gdn_oracle.forward_legacy, rtod_loss
    and adam_step the way O.train_step assembles it for the other two networks;
  * --rtod_arch / --init_from / depth_extract --arch from the command line.

Bars (tests/test_hip_model.py): kernels -- the `close` helper; depth map max |err| <= 1e-3 and rms <= 6e-5; losses
1e-3 relative; per-parameter gradients relative L2 <= 2e-2 on |ref| + 1e-3 x the typical gradient norm.
"""
import os
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import gdn_oracle as O
from test_hip_kernels import close, close_abs, nchw, nhwc, tapmajor

pytestmark = pytest.mark.gpu
REPO = pathlib.Path(__file__).resolve().parent.parent

# (Cin, Cout, k, B, H, W): the two geometries of test_fftconv_transposed_stride1_forward, the 3x3 layer small, then upconv0 / 1 / 2
# at their training shapes (128 x 416 input), batch 2
KCASES = [(256, 128, 5, 2, 26, 52), (128, 64, 7, 1, 40, 70), (512, 256, 3, 2, 16, 24),
          (512, 256, 3, 2, 32, 104), (256, 128, 5, 2, 64, 208), (128, 64, 7, 2, 128, 416)]
KIDS = ["c%d_%d_k%d_%dx%dx%d" % c for c in KCASES]


def _convt_reference(case, seed=0):
    ci, co, k, B, H, W = case
    g = torch.Generator().manual_seed(4321 + 7 * k + H + seed)
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(ci, co, k, k, generator=g) / (ci * k * k) ** 0.5         # ConvTranspose2d layout
    gy = torch.randn(B, co, H, W, generator=g)
    gres = torch.randn(B, ci, H, W, generator=g)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y_ref = F.conv_transpose2d(xr, wr, None, 1, k // 2)
    y_ref.backward(gy)
    return x, w, gy, gres, y_ref.detach(), xr.grad, wr.grad


def _paths(op, k):
    if k >= 5:
        return op.fft_ok, op.fft_fwd, op.fft_bwd, "spectrum", "xf"
    return op.wino_ok, op.wino_fwd, op.wino_bwd, "state", "state"


def _check_flipped(gpu, case, hint=None):
    """Forward, data gradient with addsrc and weight gradient of the flipped-tap op, with and without the forward's saved
    state, twice (identical bits)."""
    from gdn_amd import ops
    ci, co, k, B, H, W = case
    hint = hint or {}
    x, w, gy, gres, y_ref, dx_ref, dw_ref = _convt_reference(case)
    op = ops.Conv(ci, co, k, 1, k // 2, flip_taps=True)
    ok, fwd, bwd, save_kw, state_kw = _paths(op, k)
    assert ok(B, H, W, **hint) and ok(B, H, W, backward=True, **hint)
    xd, wd = nhwc(x).to(gpu), tapmajor(w, True).to(gpu)           # the module's own tap-major buffer [k*k][Cout][Cin]
    gyd, gresd = nhwc(gy).to(gpu), nhwc(gres).to(gpu)
    runs = []
    for _ in range(2):
        y, st, saved = fwd(xd, wd, stats=True, **{save_kw: True}, **hint)
        dw = torch.full_like(wd, 7.0)
        dx = bwd(gyd, wd, (H, W), **{state_kw: saved}, dw_tap=dw, addsrc=gresd, **hint)
        dx_only = bwd(gyd, wd, (H, W), **hint)                  # no saved state: the backward transforms the weights itself
        dw2 = torch.zeros_like(wd)
        assert bwd(gyd, wd, (H, W), **{state_kw: saved}, dw_tap=dw2, need_dx=False, **hint) is None
        runs.append([t.clone() for t in (y, st, dx, dw, dx_only, dw2)])
    y, st, dx, dw, dx_only, dw2 = runs[0]
    close(nchw(y), y_ref, what="flipped fwd")
    close(st[:, 0].sum(0), y_ref.sum((0, 2, 3)), rtol=1e-3, atol_scale=1e-3, what="stats sum")
    close(st[:, 1].sum(0), (y_ref ** 2).sum((0, 2, 3)), what="stats sumsq")
    close(nchw(dx), dx_ref + gres, what="flipped dgrad + addsrc")
    close(nchw(dx_only), dx_ref, what="flipped dgrad without saved state")
    close(dw, tapmajor(dw_ref, True), what="flipped wgrad (stored tap order)")
    assert torch.equal(dw2, dw)
    for a, b in zip(*runs):
        assert torch.equal(a, b), "a second identical call gave other bits"
    # the same layer as the transposed op it always was: direct kernels
    opt = ops.Conv(ci, co, k, 1, k // 2, transposed=True)
    close(y, opt.fwd(xd, wd), rtol=1e-4, atol_scale=1e-5, what="fwd vs direct transposed")
    close(dx_only, opt.dgrad(gyd, ops.transpose_taps(wd), (H, W)), rtol=1e-4, atol_scale=1e-5, what="dgrad vs direct transposed")
    dwd = torch.empty_like(wd)
    opt.wgrad(xd, gyd, dwd)
    close(dw, dwd, rtol=1e-4, atol_scale=2e-5, what="wgrad vs direct transposed")


@pytest.mark.parametrize("case", KCASES, ids=KIDS)
def test_flipped_taps_forward_backward_vs_conv_transpose(gpu, case, monkeypatch):
    monkeypatch.delenv("GDN_FFT_NP", raising=False)
    _check_flipped(gpu, case)


# the rest of what the frequency-domain form takes: a 9x9 window, 64 input channels, Cin < Cout, ragged edges
KCASES_MORE = [(64, 64, 9, 2, 40, 70), (64, 128, 5, 1, 37, 75), (64, 64, 7, 1, 17, 33)]


@pytest.mark.parametrize("case", KCASES_MORE, ids=["c%d_%d_k%d_%dx%dx%d" % c for c in KCASES_MORE])
def test_flipped_taps_k9_and_64_channels(gpu, case, monkeypatch):
    monkeypatch.delenv("GDN_FFT_NP", raising=False)
    _check_flipped(gpu, case)
    _check_flipped(gpu, case, {"train": True})


@pytest.mark.parametrize("case", [c for c in KCASES if c[2] >= 5], ids=[i for c, i in zip(KCASES, KIDS) if c[2] >= 5])
def test_flipped_taps_train_hint_and_40_point_plan(gpu, case, monkeypatch):
    """GDN_HINT_TRAIN (what a trained layer's forward and backward carry), and the 40-point plan forced through the test hint."""
    monkeypatch.delenv("GDN_FFT_NP", raising=False)
    _check_flipped(gpu, case, {"train": True})
    monkeypatch.setenv("GDN_FFT_NP", "40")
    _check_flipped(gpu, case, {"train": True})


@pytest.mark.parametrize("x3,f4", [(True, False), (False, False)], ids=["f2_x3", "f2_fp32"])
@pytest.mark.parametrize("case", [c for c in KCASES if c[2] == 3], ids=[i for c, i in zip(KCASES, KIDS) if c[2] == 3])
def test_flipped_taps_winograd_other_plans(gpu, case, x3, f4):
    """The default plan is covered above (F(4x4,3x3) where the layer qualifies); here F(2x2,3x3) with the bf16 x 3 panels
    and with the fp32 weight transform (whose backward set is a bin permutation of the forward's)."""
    from gdn_amd import ops
    px, pf = ops.set_x3(x3), ops.set_wino_f4(f4)
    try:
        _check_flipped(gpu, case)
    finally:
        ops.set_x3(px)
        ops.set_wino_f4(pf)


@pytest.mark.parametrize("case", [KCASES[0], KCASES[1]], ids=KIDS[:2])
def test_flipped_taps_fused_batchnorm_forms(gpu, case, monkeypatch):
    """dyb (this layer's BatchNorm backward applied while dy is transformed) and bnb (the producer's BatchNorm-backward
    partials from the gather) of the flipped form against the unfused passes, as test_input_affine_and_bn_backward_partials
    does for the plain form."""
    from gdn_amd import ops
    monkeypatch.delenv("GDN_FFT_NP", raising=False)
    ci, co, k, B, H, W = case
    g = torch.Generator().manual_seed(99 + k)
    op = ops.Conv(ci, co, k, 1, k // 2, flip_taps=True)
    y1 = torch.randn(B, H, W, ci, generator=g).to(gpu)
    w = (torch.randn(k * k, co, ci, generator=g) * 0.05).to(gpu)

    def coeffs(C):
        scale, shift = (torch.rand(C, generator=g) + 0.5).to(gpu), (torch.randn(C, generator=g) * 0.3).to(gpu)
        mean, invstd = (torch.randn(C, generator=g) * 0.1).to(gpu), (torch.rand(C, generator=g) + 0.7).to(gpu)
        return scale, shift, mean, invstd, torch.stack([scale, shift, mean, invstd]).contiguous()

    si, hi, mi, ii, coi = coeffs(ci)
    so, ho, mo, io, coo = coeffs(co)
    a = ops.bn_apply(y1, si, hi, True)
    close(op.fft_fwd(y1, w, in_affine=(si, hi), in_relu=True), op.fft_fwd(a, w), rtol=1e-5, atol_scale=1e-6, what="in_affine")
    dy = torch.randn(B, H, W, co, generator=g).to(gpu)
    skip = torch.randn(B, H, W, ci, generator=g).to(gpu)
    y_raw, st, xf = op.fft_fwd(a, w, stats=True, spectrum=True)
    dg, db, dgf, dbf = [torch.empty(co, device=gpu) for _ in range(4)]
    dw0, dw1 = torch.empty_like(w), torch.empty_like(w)
    for relu in (True, False):
        dy_mat = ops.bn_bwd(dy, y_raw, so, coo, relu, dg, db)
        ref_dx = op.fft_bwd(dy_mat, w, (H, W), xf=xf, dw_tap=dw0, addsrc=skip)
        kk = ops.bn_bwd_coeffs(dy, y_raw, coo, relu, dgf, dbf)
        got_dx = op.fft_bwd(dy, w, (H, W), xf=xf, dw_tap=dw1, addsrc=skip, dyb=(y_raw, coo, kk, relu))
        close(got_dx, ref_dx, rtol=1e-4, atol_scale=1e-5, what="dyb dx relu=%s" % relu)
        close(dw1, dw0, rtol=1e-4, atol_scale=1e-5, what="dyb dw relu=%s" % relu)
    slots = op.fft_bnb_slots(B, H, W)
    assert slots > 0
    for relu in (True, False):
        part = torch.full((slots, 2, ci), float("nan"), device=gpu)
        dx_ref = op.fft_bwd(dy, w, (H, W), addsrc=skip)
        dx = op.fft_bwd(dy, w, (H, W), addsrc=skip, bnb=(y1, coi, relu, part))
        assert torch.equal(dx, dx_ref) and torch.isfinite(part).all()
        dz = dx.double()
        if relu:
            dz = dz * ((y1 * si + hi) > 0)
        xhat = (y1.double() - mi.double()) * ii.double()
        s = part.double().sum(0)
        close(s[0], dz.sum((0, 1, 2)), rtol=1e-4, atol_scale=1e-5, what="bnb sum dz relu=%s" % relu)
        close(s[1], (dz * xhat).sum((0, 1, 2)), rtol=1e-4, atol_scale=1e-5, what="bnb sum dz*xhat relu=%s" % relu)


def test_flip_taps_is_a_transform_domain_form_only(gpu):
    """The hint is part of the layer's definition: the direct entry points refuse it instead of computing the un-flipped
    convolution, and it cannot be combined with transposed / reflection / other strides."""
    from gdn_amd import ops
    from gdn_amd._lib import GdnError
    op = ops.Conv(128, 64, 7, 1, 3, flip_taps=True)
    x = torch.randn(1, 20, 24, 128, device=gpu)
    w = torch.randn(49, 64, 128, device=gpu)
    with pytest.raises(GdnError):
        op.fwd(x, w)
    with pytest.raises(GdnError):
        op.dgrad(torch.randn(1, 20, 24, 64, device=gpu), ops.transpose_taps(w), (20, 24))
    with pytest.raises(GdnError):
        op.wgrad(x, torch.randn(1, 20, 24, 64, device=gpu), torch.empty_like(w))
    for bad in (dict(transposed=True), dict(reflect=True), dict(stride=2)):
        kw = dict(stride=1, pad=3)
        kw.update(bad)
        with pytest.raises(GdnError):
            ops.Conv(128, 64, 7, flip_taps=True, **kw)
    with pytest.raises(GdnError):
        ops.Conv(128, 64, 4, 1, 2, flip_taps=True)
    # what a transposed = 1 geometry answers is unchanged
    t = ops.Conv(128, 64, 7, 1, 3, transposed=True)
    assert t.fft_ok(1, 20, 24) and not t.fft_ok(1, 20, 24, backward=True)
    assert not ops.Conv(512, 256, 3, 1, 1, transposed=True).wino_ok(1, 20, 24)


# ----------------------------------------------------------------------------
# Engine
# ----------------------------------------------------------------------------
def _plain_module():
    import gdn_amd.AE_model_unet as M
    from gdn_amd import engine as E

    class Plain(M._HipModule):
        """y = conv1x1_b(cat(conv1x1_a(x), x)): conv_plain without and with the concatenated second input."""

        def __init__(self):
            super().__init__()
            self.a = nn.Conv2d(64, 64, 1, bias=False)
            self.b = nn.Conv2d(128, 64, 1, bias=False)

        def _run(self, ctx, x):
            return (E.conv_plain(ctx, E.conv_plain(ctx, x, self.a), self.b, x2=x),)

        def forward(self, x):
            return self._forward_impl(x, (0,))
    return Plain()


def test_conv_plain_backward_vs_autograd(gpu):
    torch.manual_seed(3)
    m = _plain_module()
    x = torch.randn(2, 64, 18, 28)
    gy = torch.randn(2, 64, 18, 28)
    xr = x.clone().requires_grad_(True)
    wa, wb = m.a.weight.detach().clone().requires_grad_(True), m.b.weight.detach().clone().requires_grad_(True)
    y_ref = F.conv2d(torch.cat((F.conv2d(xr, wa), xr), 1), wb)
    y_ref.backward(gy)
    m = m.to(gpu).train()
    xg = x.to(gpu).requires_grad_(True)
    y = m(xg)
    assert y.requires_grad
    y.backward(gy.to(gpu))
    close(y, y_ref, what="conv_plain forward")
    close(xg.grad, xr.grad, what="conv_plain dx (split over x and x2, accumulated)")
    close(m.a.weight.grad, wa.grad, what="conv_plain dw")
    close(m.b.weight.grad, wb.grad, what="conv_plain dw with x2")


_STAGES = {256: ("upconv0", "N256_up", "conv1x1_256", "res256_up1", "res256_up2", 512, 1),
           128: ("upconv1", "N128_up", "conv1x1_128", "res128_up1", "res128_up2", 256, 2),
           64: ("upconv2", "N64_up", "conv1x1_64", "res64_up1", "res64_up2", 128, 3)}


def _stage_module(net, level, skip):
    import gdn_amd.AE_model_unet as M
    from gdn_amd import engine as E
    up, bn, c1, r1, r2, _, _ = _STAGES[level]

    class Stage(M._HipModule):
        """One decoder stage of the legacy network on its own modules (AutoEncoder._run)."""

        def __init__(self):
            super().__init__()
            self.net = net

        def _run(self, ctx, x):
            n = self.net
            a = E.conv_bn_act(ctx, E.upsample(ctx, x, True), getattr(n, up), getattr(n, bn), relu=True)
            a = E.conv_plain(ctx, a, getattr(n, c1), x2=skip)
            return (getattr(n, r2).run(ctx, getattr(n, r1).run(ctx, a)),)

        def forward(self, x):
            return self._forward_impl(x, (0,))
    return Stage()


@pytest.mark.parametrize("transform", [True, False], ids=["transform", "direct"])
@pytest.mark.parametrize("level", [256, 128, 64])
def test_legacy_decoder_stage_vs_oracle(gpu, monkeypatch, level, transform):
    """upsample(align_corners=True) -> ConvTranspose2d -> BatchNorm -> ReLU -> 1x1 over cat -> two ResidualBlocks, train mode,
    against the oracle's functions; with the transform-domain paths on (the ConvTranspose2d runs as a flipped-tap convolution)
    and refused (fft_ok / wino_ok say no: everything on the direct kernels, the layer the transposed op it always was)."""
    import gdn_amd.AE_model_unet as M
    from gdn_amd import ops
    up, bn, c1, r1, r2, ci, pad = _STAGES[level]
    B, h, w = 2, 10, 14
    torch.manual_seed(level)
    net = M.AutoEncoder(height=32, width=64)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(level + 1)
    x = torch.randn(B, ci, h, w, generator=g)
    skip = torch.randn(B, level, 2 * h, 2 * w, generator=g)
    gy = torch.randn(B, level, 2 * h, 2 * w, generator=g)
    leaves = {k: v.detach().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}
    work = dict(sd)
    work.update(leaves)
    xr = x.clone().requires_grad_(True)
    a = O._conv(O._up_ac1(xr), work[up + ".weight"], 1, pad, transposed=True)
    a = F.relu(O._bn(a, work, bn, True))
    a = O._conv(torch.cat((a, skip), 1), work[c1 + ".weight"], 1, 0)
    y_ref = O._rb(O._rb(a, work, r1, True), work, r2, True)
    y_ref.backward(gy)
    used = []
    if transform:
        for name in ("fft_bwd", "wino_bwd"):
            orig = getattr(ops.Conv, name)
            monkeypatch.setattr(ops.Conv, name, lambda self, *a, _o=orig, **k: (used.append(self.flip_taps), _o(self, *a, **k))[1])
    else:
        monkeypatch.setattr(ops.Conv, "fft_ok", lambda self, *a, **k: False)
        monkeypatch.setattr(ops.Conv, "wino_ok", lambda self, *a, **k: False)
    net = net.to(gpu).train()
    stage = _stage_module(net, level, nhwc(skip).to(gpu)).to(gpu).train()
    xg = x.to(gpu).requires_grad_(True)
    y = stage(xg)
    y.backward(gy.to(gpu))
    assert (True in used) == transform, "the ConvTranspose2d layer did not take the expected path"
    close(y, y_ref, rtol=1e-3, atol_scale=1e-4, what="stage output")
    close(xg.grad, xr.grad, rtol=1e-3, atol_scale=2e-4, what="stage dx")
    prefixes = (up, bn, c1, r1, r2)
    grads = {k: p.grad for k, p in net.named_parameters()}
    typical = float(np.median([leaves[k].grad.double().norm().item() for k in leaves if k.startswith(prefixes)]))
    for k, p in net.named_parameters():
        if not k.startswith(prefixes):
            assert grads[k] is None, k
            continue
        gr, rr = grads[k].detach().cpu().double(), leaves[k].grad.double()
        rel = float((gr - rr).norm() / (rr.norm() + 1e-3 * typical))
        assert rel < 2e-2, "%s: relative gradient error %.3e" % (k, rel)
    hip_sd = net.state_dict()
    for k in sd:
        if "running_" in k and k.startswith(prefixes):
            close(hip_sd[k], sd[k], rtol=1e-3, atol_scale=1e-3, what=k)


# ----------------------------------------------------------------------------
# Network
# ----------------------------------------------------------------------------
def _reference_step(sd, batch, g_sd=None, lr=2e-5):
    """O.train_step for the legacy network: forward_legacy (train mode) -> rtod_loss -> backward -> adam_step.  `sd` is updated
    in place (weights, BatchNorm running statistics)."""
    depths, rgb, sparse = batch
    keys = O.trainable_keys(sd)
    leaves = {k: sd[k].detach().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(leaves)
    out = O.forward_legacy(work, rgb, istrain=False, training=True)
    loss, ol, lat, sm = O.rtod_loss(out, depths, rgb, sparse, g_sd)
    out.retain_grad()
    loss.backward()
    grads = {k: leaves[k].grad for k in keys}
    with torch.no_grad():
        O.adam_step({k: sd[k] for k in keys}, grads, {}, lr=lr)
    loss, ol, lat, sm = [float(v.detach()) for v in (loss, ol, lat, sm)]
    return {"loss": loss, "output_loss": ol, "latent_loss": lat, "smoothness_loss": sm,
            "outputs": out.detach(), "dout": out.grad.detach(), "grads": grads}


def _grad_errors(model, ref):
    typical = float(np.median([ref["grads"][k].double().norm().item() for k, _ in model.named_parameters()]))
    worst, worst_k = 0.0, None
    for k, p in model.named_parameters():
        assert p.grad is not None, "no gradient for " + k
        gr, rr = p.grad.detach().cpu().double(), ref["grads"][k].double()
        rel = float((gr - rr).norm() / (rr.norm() + 1e-3 * typical))
        if rel > worst:
            worst, worst_k = rel, k
    return worst, worst_k, typical


def _hip_step(gpu, sd, g_sd, batch, H, W, seed_dout=None):
    import gdn_amd.AE_model_unet as M
    from gdn_amd import trainer as T
    from gdn_amd import utils as U
    from gdn_amd.optim import Adam
    depth, rgb, sparse = [t.to(gpu) for t in batch]
    model = M.AutoEncoder(height=H, width=W)
    model.load_state_dict(sd)
    model = model.to(gpu).train()
    G = None
    if g_sd is not None:
        G = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W)
        G.load_state_dict(g_sd)
        G = G.to(gpu).eval().requires_grad_(False)
    opt = Adam(model.parameters(), 2e-5, [0.9, 0.999], eps=1e-08, weight_decay=5e-4)
    out = model(rgb, istrain=False)
    assert out.requires_grad, "a train-mode forward with grad enabled must record a tape"
    lat = torch.zeros((), device=gpu) if G is None else T.guide_latent_loss(G, depth, out)
    loss, ol, sm = U.rtod_pixel_loss(out, depth, rgb, sparse, plus=lat)
    out.retain_grad()
    opt.zero_grad()
    if seed_dout is None:
        loss.backward()
    else:
        out.backward(seed_dout.to(gpu))
    return model, opt, out, loss, ol, lat, sm


def _check_step(model, opt, out, loss, ol, lat, sm, ref, ref_sd, what, guided):
    assert loss.item() == pytest.approx(ref["loss"], rel=1e-3)
    assert ol.item() == pytest.approx(ref["output_loss"], rel=1e-3) and sm.item() == pytest.approx(ref["smoothness_loss"], rel=1e-3)
    if guided:
        assert lat.item() == pytest.approx(ref["latent_loss"], rel=2e-3)
    d = out.detach().cpu().double() - ref["outputs"].double()
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    print("%s: depth map max err %.3e rms %.3e" % (what, mx, rms))
    assert mx <= 1e-3 and rms <= 6e-5, "%s depth map: max err %.3e rms %.3e" % (what, mx, rms)
    close(out.grad, ref["dout"], rtol=2e-3, atol_scale=2e-3, what=what + " dL/dout", outliers=1e-3)
    opt.step()
    hip_sd = model.state_dict()
    for k, v in ref_sd.items():
        if "running_" in k:
            close(hip_sd[k], v, rtol=1e-3, atol_scale=1e-3, what=what + " " + k)
        elif k.endswith("num_batches_tracked"):
            assert int(hip_sd[k]) == int(v) == 1, k
        elif v.dim() == 4:
            a, b = hip_sd[k].detach().cpu().double(), v.double()
            assert float((a - b).norm() / b.norm()) < 1e-3, "post-Adam " + k


@pytest.mark.parametrize("mode", ["RtoD_single", "RtoD"])
def test_legacy_train_step_vs_oracle(gpu, mode):
    """One training step of AutoEncoder at B = 2, 64 x 128 against the CPU reference step: losses, depth map, dL/dout, parameters
    after Adam, BatchNorm running statistics from the network's own loss; every parameter gradient from a backward that starts
    at the ORACLE's dL/dout (the L1-type losses' gradient is a sign function of out - gt: at this size a handful of flipped signs
    moves the heavily cancelling sums by percents whatever the kernels do -- test_train_step_gradients_vs_oracle)."""
    H, W = 64, 128
    batch = O.synthetic_batch(2, H, W, seed=11)
    sd = O.init_state_dict("AutoEncoder", seed=2)
    g_sd = O.init_state_dict("AutoEncoder_DtoD", seed=3) if mode == "RtoD" else None
    ref_sd = {k: v.clone() for k, v in sd.items()}
    ref = _reference_step(ref_sd, batch, None if g_sd is None else {k: v.clone() for k, v in g_sd.items()})
    step = _hip_step(gpu, sd, g_sd, batch, H, W)
    _check_step(*step, ref, ref_sd, "legacy %s B=2" % mode, g_sd is not None)
    model = _hip_step(gpu, sd, g_sd, batch, H, W, seed_dout=ref["dout"])[0]
    worst, worst_k, typical = _grad_errors(model, ref)
    print("legacy %s B=2: worst per-parameter gradient rel-L2 error %.3e (%s), typical grad norm %.3e" % (mode, worst, worst_k, typical))
    assert worst < 2e-2, "%s: relative gradient error %.3e" % (worst_k, worst)


def test_legacy_train_step_b20_vs_oracle(gpu):
    """The same at the benchmark shape, B = 20, 128 x 416, RtoD with a frozen random guide, everything from the network's own
    loss -- as test_rtod_train_step_b20_vs_oracle does for AutoEncoder_2."""
    B, H, W = 20, 128, 416
    batch = O.synthetic_batch(B, H, W, seed=1)
    sd = O.init_state_dict("AutoEncoder", seed=0)
    g_sd = O.init_state_dict("AutoEncoder_DtoD", seed=1)
    ref_sd = {k: v.clone() for k, v in sd.items()}
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 32)))
    ref = _reference_step(ref_sd, batch, {k: v.clone() for k, v in g_sd.items()})
    model, opt, out, loss, ol, lat, sm = _hip_step(gpu, sd, g_sd, batch, H, W)
    worst, worst_k, typical = _grad_errors(model, ref)
    print("legacy RtoD B=20: worst per-parameter gradient rel-L2 error %.3e (%s), typical grad norm %.3e" % (worst, worst_k, typical))
    _check_step(model, opt, out, loss, ol, lat, sm, ref, ref_sd, "legacy RtoD B=20", True)
    assert worst < 2e-2, "%s: relative gradient error %.3e" % (worst_k, worst)


def test_legacy_training_step_is_bitwise_reproducible(gpu):
    import gdn_amd.AE_model_unet as M
    from gdn_amd import optim
    from gdn_amd import utils as U
    H, W, B = 128, 416, 2
    depth, rgb, sparse = [t.to(gpu) for t in O.synthetic_batch(B, H, W, seed=21)]

    def run():
        torch.manual_seed(7)
        net = M.AutoEncoder(height=H, width=W).to(gpu).train()
        opt = optim.Adam(net.parameters(), lr=2e-5)
        out = net(rgb, istrain=False)
        loss = U.rtod_pixel_loss(out, depth, rgb, sparse)[0]
        opt.zero_grad()
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
        opt.step()
        torch.cuda.synchronize()
        return loss.detach().clone(), out.detach().clone(), grads, {k: v.detach().clone() for k, v in net.state_dict().items()}

    a, b = run(), run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys() and len(a[2]) == len(list(M.AutoEncoder(height=H, width=W).parameters()))
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), "gradient of %s differs between two identical steps" % k
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), "%s differs after two identical steps" % k


def test_legacy_gradient_accumulation(gpu):
    """Two backwards without zero_grad hold the sum of the two micro-steps' gradients, to the bar of
    test_gradient_accumulation_and_unwritten_params (BatchNorm running statistics move between the two, batch statistics do not)."""
    import gdn_amd.AE_model_unet as M
    from gdn_amd import utils as U
    H, W = 32, 64
    depth, rgb, sparse = [t.to(gpu) for t in O.synthetic_batch(2, H, W, seed=3)]
    torch.manual_seed(2)
    model = M.AutoEncoder(height=H, width=W).to(gpu).train()

    def run(sl):
        out = model(rgb[sl], istrain=False)
        U.rtod_pixel_loss(out, depth[sl], rgb[sl], sparse[sl])[0].backward()

    run(slice(0, 1))
    g1 = {k: p.grad.clone() for k, p in model.named_parameters()}
    for p in model.parameters():
        p.grad = None
    run(slice(1, 2))
    g2 = {k: p.grad.clone() for k, p in model.named_parameters()}
    for p in model.parameters():
        p.grad = None
    run(slice(0, 1))
    run(slice(1, 2))                                        # no zero_grad in between
    for k, p in model.named_parameters():
        close(p.grad, g1[k] + g2[k], rtol=2e-3, atol_scale=2e-3, what="accumulated " + k)


def test_legacy_eval_forward_records_nothing(gpu, monkeypatch):
    """eval() with grad enabled, and train() under no_grad: no tape, no saved-for-backward state, outputs without history."""
    import gdn_amd.AE_model_unet as M
    from gdn_amd import engine as E
    H, W = 32, 64
    ctxs = []
    orig = E.Ctx.__init__
    monkeypatch.setattr(E.Ctx, "__init__", lambda self, *a, **k: (orig(self, *a, **k), ctxs.append(self))[0])
    torch.manual_seed(0)
    model = M.AutoEncoder(height=H, width=W).to(gpu)
    x = torch.randn(1, 3, H, W, device=gpu)
    outs = model.eval()(x, istrain=True)
    with torch.no_grad():
        out2 = model.train()(x, istrain=False)
    assert len(ctxs) == 2 and all(not c.record and c.tape == [] and not c.grads and not c.bn_src for c in ctxs)
    assert len(outs) == 8 and not any(o.requires_grad for o in outs) and not out2.requires_grad
    assert not any(hasattr(m, "_gdn_op_flip") for m in model.modules())     # inference never builds the flipped-tap form
    out3 = model.train()(x, istrain=False)
    assert out3.requires_grad and ctxs[-1].record and len(ctxs[-1].tape) > 0
    assert all(hasattr(getattr(model, n), "_gdn_op_flip") for n in ("upconv0", "upconv1", "upconv2"))


def test_legacy_refusals(gpu):
    """Out of scope, and said so: train-mode InstanceNorm for this network."""
    import gdn_amd.AE_model_unet as M
    from gdn_amd._lib import GdnError
    H, W = 32, 64
    x = torch.randn(1, 3, H, W, device=gpu)
    inst = M.AutoEncoder(norm='Instance', height=H, width=W).to(gpu)
    with pytest.raises(GdnError, match="InstanceNorm"):
        inst.train()(x, istrain=False)
    assert inst.eval()(x, istrain=False).shape == (1, 1, H, W)


def test_legacy_bf16_train_step_vs_emulation(gpu):
    """compute_dtype('bf16'): the existing bf16 direct kernels take every legacy geometry (the three ConvTranspose2d layers
    stay transposed ops there), so bf16 training simply works.  One RtoD_single step at B = 2, 128 x 416 against
    oracle.bf16_emulation(), with the bars tests/test_hip_bf16.py::test_bf16_rtod_vs_emulation holds AutoEncoder_2 to: feature
    maps no further from the emulation than 1.25 x the emulation is from the fp32 oracle (+2e-3), and <= 2e-2 on the first two;
    loss terms within 2e-2 relative; the median relative L2 distance of the parameter gradients to the emulation's no larger
    than 1.25 x the emulation's distance to the fp32 oracle (+2e-2)."""
    import gdn_amd.AE_model_unet as M
    from gdn_amd import utils as U
    from test_hip_bf16 import rel_l2
    H, W = 128, 416
    batch = O.synthetic_batch(2, H, W, seed=0)
    sd = O.init_state_dict("AutoEncoder", seed=0)
    cl = lambda d: {k: v.clone() for k, v in d.items()}
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 32)))
    ref32 = _reference_step(cl(sd), batch)
    with torch.no_grad():
        f32 = O.forward_legacy(cl(sd), batch[1], istrain=True, training=True)
    with O.bf16_emulation():
        emu = _reference_step(cl(sd), batch)
        with torch.no_grad():
            f_emu = O.forward_legacy(cl(sd), batch[1], istrain=True, training=True)
    depth, rgb, sparse = [t.to(gpu) for t in batch]
    model = M.AutoEncoder(height=H, width=W)
    model.load_state_dict(sd)
    model = model.to(gpu).train().compute_dtype("bf16")
    feats = model(rgb, istrain=True)
    out = feats[7]
    assert out.dtype == torch.float32 and out.requires_grad
    loss, ol, sm = U.rtod_pixel_loss(out, depth, rgb, sparse)
    loss.backward()
    hip = [rel_l2(a.detach().float().cpu(), b) for a, b in zip(feats, f_emu)]
    emu_drift = [rel_l2(a, b) for a, b in zip(f_emu, f32)]
    print("legacy features HIP bf16 vs emulation : " + " ".join("%.4f" % v for v in hip))
    print("legacy features emulation vs fp32     : " + " ".join("%.4f" % v for v in emu_drift))
    print("loss HIP %.5f (berhu %.5f smooth %.5f) | emulation %.5f (%.5f %.5f) | fp32 oracle %.5f"
          % (loss.item(), ol.item(), sm.item(), emu["loss"], emu["output_loss"], emu["smoothness_loss"], ref32["loss"]))
    g_hip = {k: p.grad.detach().cpu() for k, p in model.named_parameters()}
    med = np.median([float(v.norm()) for v in ref32["grads"].values()])
    keys = [k for k in g_hip if ref32["grads"][k].norm() > 1e-3 * med]
    dh = np.array([rel_l2(g_hip[k], emu["grads"][k]) for k in keys])
    dc = np.array([rel_l2(emu["grads"][k], ref32["grads"][k]) for k in keys])
    print("gradient distance (median / 90th pct): HIP-vs-emulation %.3f / %.3f, emulation-vs-fp32 %.3f / %.3f"
          % (np.median(dh), np.percentile(dh, 90), np.median(dc), np.percentile(dc, 90)))
    assert hip[0] <= 2e-2 and hip[1] <= 2e-2
    for i, (h, c) in enumerate(zip(hip, emu_drift)):
        assert h <= 1.25 * c + 2e-3, "feature %d: HIP-vs-emulation %.4f, emulation-vs-fp32 %.4f" % (i, h, c)
    assert ol.item() == pytest.approx(emu["output_loss"], rel=2e-2)
    assert sm.item() == pytest.approx(emu["smoothness_loss"], rel=2e-2)
    assert np.median(dh) <= 1.25 * np.median(dc) + 2e-2


# ----------------------------------------------------------------------------
# Interface
# ----------------------------------------------------------------------------
def _child(cwd, module, argv, limit=600):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([str(REPO / "gdn-pytorch_amd"), str(REPO)] +
                                        ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    cwd.mkdir(parents=True, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", module, *argv]
    return subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(cwd), timeout=limit + 60)


def _cli(cwd, argv):
    r = _child(cwd, "gdn_amd.GDN_main", argv)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


_TRAIN = ["synthetic", "--synthetic", "--epochs", "1", "--epoch_size", "3", "--batch_size", "2", "--gpu_num", "0", "--seed", "3"]


@pytest.mark.parametrize("arch,cls", [("legacy", "AutoEncoder"), ("unet", "AutoEncoder_2")])
def test_cli_train_then_evaluate_same_architecture(gpu, tmp_path, arch, cls):
    """--mode RtoD_single --rtod_arch A writes a checkpoint that --mode RtoD_test --rtod_arch A --evaluate loads (a finite
    metrics line) and --init_from reproduces bit for bit before the first step."""
    import gdn_amd.AE_model_unet as M
    from gdn_amd import GDN_main, option
    _cli(tmp_path / "train", _TRAIN + ["--mode", "RtoD_single", "--rtod_arch", arch])
    ck = sorted((tmp_path / "train").rglob("*.pkl"))
    assert len(ck) == 1, ck
    saved = torch.load(ck[0], map_location="cpu")
    ref_keys = ["module." + k for k in getattr(M, cls)().state_dict()]
    assert list(saved) == ref_keys
    out = _cli(tmp_path / "test", _TRAIN + ["--mode", "RtoD_test", "--rtod_arch", arch, "--evaluate", "--RtoD_model_dir", str(ck[0])])
    res = [ln for ln in out.splitlines() if ln.startswith("Results: ")]
    assert len(res) == 1, out[-2000:]
    vals = [float(v) for v in re.findall(r"\w+ (-?[0-9.]+(?:e-?\d+)?|nan|inf)", res[0])]
    assert len(vals) == 8 and all(np.isfinite(vals)), res[0]
    # the architecture the checkpoint does not belong to fails on the keys instead of evaluating something else
    other = "unet" if arch == "legacy" else "legacy"
    r = _child(tmp_path / "other", "gdn_amd.GDN_main", _TRAIN + ["--mode", "RtoD_test", "--rtod_arch", other, "--RtoD_model_dir", str(ck[0])])
    assert r.returncode != 0 and "state_dict" in r.stderr
    # --init_from: the fine-tuning entry
    args = option.parse_args(_TRAIN + ["--mode", "RtoD_single", "--rtod_arch", arch, "--init_from", str(ck[0])])
    net = GDN_main._rtod_network(args, args.height, args.width).to(gpu)
    assert type(net).__name__ == cls
    GDN_main._init_from(net, args, 0)
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), saved["module." + k]), k
    out = _cli(tmp_path / "tune", _TRAIN + ["--mode", "RtoD_single", "--rtod_arch", arch, "--init_from", str(ck[0])])
    assert "=> initialised %s from" % cls in out and len(sorted((tmp_path / "tune").rglob("*.pkl"))) == 1


def test_cli_init_from_missing_file_raises(gpu, tmp_path):
    r = _child(tmp_path, "gdn_amd.GDN_main", _TRAIN + ["--mode", "RtoD_single", "--rtod_arch", "legacy", "--init_from",
                                                        str(tmp_path / "nothing.pkl")])
    assert r.returncode != 0 and "FileNotFoundError" in r.stderr and "nothing.pkl" in r.stderr
    assert not list(tmp_path.rglob("*.pkl"))


def test_depth_extract_arch_unet(gpu, tmp_path):
    from PIL import Image
    import gdn_amd.AE_model_unet as M
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    r = np.random.RandomState(0)
    for i in range(2):
        Image.fromarray(r.randint(0, 256, (60, 200, 3)).astype(np.uint8)).save(imgs / ("%02d.png" % i))
    torch.manual_seed(1)
    torch.save({"module." + k: v for k, v in M.AutoEncoder_2().state_dict().items()}, tmp_path / "unet.pkl")
    for arch, ok in (("unet", True), ("legacy", False)):
        res = _child(tmp_path, "gdn_amd.depth_extract", ["--model_dir", str(tmp_path / "unet.pkl"), "--img_dir", str(imgs),
                                                         "--out_dir", str(tmp_path / arch), "--arch", arch, "--batch", "2"])
        assert (res.returncode == 0) == ok, (res.stdout[-1000:], res.stderr[-2000:])
    outs = sorted((tmp_path / "unet").glob("*_depth.png"))
    assert len(outs) == 2 and Image.open(outs[0]).size == (200, 60)
