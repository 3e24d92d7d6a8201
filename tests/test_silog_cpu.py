"""The scale-invariant log loss without a GPU: the float64 restatement (tests/silog_fp64.py) against torch's float64
autograd of the formula written with torch ops and against a three-pixel case worked by hand, its degenerate cases, the
measure of the pixels a float32 comparison could decide otherwise, the flags with every refusal of GDN_main._check_loss, and
the `pixel=None` branch of the two training losses."""
import argparse
import math

import numpy as np
import pytest
import torch

import silog_fp64 as R

BASE = ["synthetic", "--synthetic"]
SHAPES = [(2, 1, 8, 12), (3, 1, 5, 7), (1, 1, 1, 9)]
BOXES = {(2, 1, 8, 12): (2, 7, 1, 11), (3, 1, 5, 7): (1, 5, 0, 6), (1, 1, 1, 9): (0, 1, 1, 8)}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _uniform(shape, seed):
    return torch.rand(shape, generator=_gen(seed)) * 2 - 1


def _sparse(shape, seed):
    """A LiDAR return (a value above -1) on about two thirds of the pixels, exactly -1 elsewhere."""
    hole = torch.rand(shape, generator=_gen(seed)) < 0.33
    return torch.where(hole, torch.tensor(-1.0), _uniform(shape, seed + 1) * 0.999)


def _torch_silog(out, gt, sparse, box, lam, weight, floor):
    """The formula with torch ops in float64; autograd gives the gradient (clamp passes none below its bound)."""
    lam, weight, fl = R.scalars(lam, weight, floor)
    o = out.double().requires_grad_(True)
    g = gt.double()
    valid = (g + 1) / 2 > fl
    if sparse is not None:
        y1, y2, x1, x2 = box
        crop = torch.zeros_like(valid)
        crop[:, :, y1:y2, x1:x2] = True
        valid = valid & crop & (sparse.double()[:, 0:1] > -1)
    d = (torch.log(torch.clamp((o + 1) / 2, min=fl)) - torch.log(torch.clamp((g + 1) / 2, min=fl)))[valid]
    n = d.numel()
    m1, m2 = d.sum() / n, (d * d).sum() / n
    D = m2 - lam * m1 * m1
    loss = weight * torch.sqrt(D)
    loss.backward()
    return loss.item(), o.grad.numpy(), (float(n), m1.item(), m2.item(), D.item())


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "box+sparse"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_restatement_against_torch_autograd(shape, masked):
    """Float64 on both sides, a dozen roundings per pixel and a sum over at most 192 of them: 1e-13 relative (of the largest
    gradient element) is hundreds of float64 ulps of headroom; the worst difference is printed."""
    out, gt = _uniform(shape, 1), _uniform(shape, 2)
    out.view(-1)[0] = -0.99                              # one clamped prediction, ...
    gt.view(-1)[1] = -0.99                               # ... one pixel whose ground truth is below the floor
    sparse = _sparse(shape, 3) if masked else None
    box = BOXES[shape] if masked else None
    for lam, weight in ((0.85, 10.0), (0.0, 0.5), (0.5, 0.85)):
        loss, grad, stats = R.silog(out, gt, sparse, box, lam, weight, 0.0125)
        tl, tg, ts = _torch_silog(out, gt, sparse, box, lam, weight, 0.0125)
        assert stats[0] >= 2 and stats[3] > 0
        assert abs(loss - tl) <= 1e-13 * abs(tl)
        worst = float(np.abs(grad - tg).max())
        print("FIGURE restatement vs autograd %s %s lam %g: max |dgrad| %.3g" % (shape, "masked" if masked else "dense", lam, worst))
        assert worst <= 1e-13 * float(np.abs(tg).max())
        assert all(abs(a - b) <= 1e-13 * abs(b) for a, b in zip(stats, ts))
        assert grad.reshape(-1)[0] == 0.0 and grad.reshape(-1)[1] == 0.0
        assert not grad[~R.valid_mask(gt, sparse, box)].any()


def test_three_pixels_by_hand():
    """depths (1/2, 1/4, 1) against (1/4, 1/4, 1/2) of the range: d = (L, 0, L) with L = ln 2, m1 = 2L/3, m2 = 2L^2/3 and,
    at lambda = 1/2, D = 4L^2/9; weight 3 gives loss = 2L, a = 3 / (2L), b = L/3 and the gradient (1, -1, 1/2)."""
    L = math.log(2.0)
    out = torch.tensor([0.0, -0.5, 1.0]).view(1, 1, 1, 3)
    gt = torch.tensor([-0.5, -0.5, 0.0]).view(1, 1, 1, 3)
    loss, grad, (n, m1, m2, D) = R.silog(out, gt, None, None, 0.5, 3.0, 0.0125)
    assert n == 3.0
    for got, want in ((loss, 2 * L), (m1, 2 * L / 3), (m2, 2 * L * L / 3), (D, 4 * L * L / 9)):
        assert abs(got - want) <= 4e-16 * want
    assert np.abs(grad.reshape(-1) - np.array([1.0, -1.0, 0.5])).max() <= 1e-15
    # a fourth pixel without ground truth: whatever is predicted there -- a NaN -- is never looked at
    out4 = torch.tensor([0.0, -0.5, 1.0, float("nan")]).view(1, 1, 1, 4)
    gt4 = torch.tensor([-0.5, -0.5, 0.0, -1.0]).view(1, 1, 1, 4)
    loss4, grad4, stats4 = R.silog(out4, gt4, None, None, 0.5, 3.0, 0.0125)
    assert loss4 == loss and stats4 == (n, m1, m2, D) and np.array_equal(grad4.reshape(-1), np.append(grad.reshape(-1), 0.0))
    # the same NaN where there is ground truth: the loss and the gradient of every valid pixel show it
    out4[0, 0, 0, 3], gt4[0, 0, 0, 3] = float("nan"), 0.25
    loss5, grad5, _ = R.silog(out4, gt4, None, None, 0.5, 3.0, 0.0125)
    assert loss5 != loss5 and np.isnan(grad5).all()


def test_degenerate_cases():
    shape = (2, 1, 4, 6)
    out, gt = _uniform(shape, 5), _uniform(shape, 6)
    # no valid pixel: ground truth at or below the floor everywhere / a sparse map without a single return
    for g, sparse, box in ((torch.full(shape, -0.98), None, None), (gt, torch.full(shape, -1.0), (0, 4, 0, 6))):
        loss, grad, stats = R.silog(out, g, sparse, box)
        assert loss == 0.0 and not grad.any() and stats == (0.0, 0.0, 0.0, 0.0)
    # out == gt everywhere: d = 0, D = 0
    gt_ok = gt.clamp(min=-0.9)
    loss, grad, stats = R.silog(gt_ok.clone(), gt_ok)
    assert loss == 0.0 and not grad.any() and stats == (float(gt_ok.numel()), 0.0, 0.0, 0.0)
    # every prediction clamped: a loss (log floor - log u(gt) varies), no gradient anywhere
    loss, grad, stats = R.silog(torch.full(shape, -0.99), gt_ok)
    assert loss > 0.0 and stats[3] > 0.0 and not grad.any()


def test_ambiguous_band_is_far_inside_the_cap():
    """Uniform inputs: t(x) is uniform on (0, 1), the band around the floor has measure 2 * BAND = 1.2e-7; the share found
    in a million draws stays far below the project's cap of 5e-4 on excluded pixels."""
    assert 2 * R.BAND < 1.3e-7
    x = _uniform((1 << 20,), 7)
    share = float(R.ambiguous(x).mean())
    print("FIGURE share of 2^20 uniform draws inside the band: %.3g" % share)
    assert share <= 5e-4 / 100
    # grid inputs k / 64 - 1: nothing near the floor at all
    k = torch.arange(0, 129).float()
    assert not R.ambiguous(k / 64 - 1).any()


# ---- command line -----------------------------------------------------------------------------------------------------
def _no_gpu_calls(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the check touched the GPU")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "is_initialized", boom)


def test_flags_parse():
    from gdn_amd import option
    a = option.parse_args(BASE)
    assert a.loss == "berhu" and option.pixel_spec(a) is None
    assert (a.silog_lambda, a.silog_weight, a.silog_floor, a.silog_mask) == (None, None, None, None)
    assert option.pixel_spec(option.parse_args(BASE + ["--loss", "silog"])) == ("silog", 0.85, 10.0, 0.0125, False)
    a = option.parse_args(BASE + ["--loss", "silog", "--silog_lambda", "0.5", "--silog_weight", "2", "--silog_floor", "0.05",
                                  "--silog_mask", "lidar"])
    assert option.pixel_spec(a) == ("silog", 0.5, 2.0, 0.05, True)
    assert option.pixel_spec(argparse.Namespace()) is None
    text = " ".join(option.build_parser().format_help().split())
    assert all(f in text for f in ("--loss", "--silog_lambda", "--silog_weight", "--silog_floor", "--silog_mask"))


@pytest.mark.parametrize("flag,bad", [("--loss", "l2"), ("--silog_mask", "box"), ("--silog_lambda", "x")])
def test_flags_reject_at_parse_time(flag, bad, capsys):
    from gdn_amd import option
    with pytest.raises(SystemExit):
        option.parse_args(BASE + ["--loss", "silog"] * (flag != "--loss") + [flag, bad])
    assert flag in capsys.readouterr().err


REFUSALS = [
    (["--mode", "DtoD_test", "--loss", "silog"], "trains nothing"),
    (["--mode", "RtoD_test", "--loss", "silog"], "trains nothing"),
    (["--mode", "DtoD", "--silog_lambda", "0.5"], "--loss silog"),
    (["--mode", "DtoD", "--silog_weight", "2"], "--loss silog"),
    (["--mode", "DtoD", "--silog_floor", "0.1"], "--loss silog"),
    (["--mode", "DtoD", "--silog_mask", "dense"], "--loss silog"),
    (["--mode", "DtoD", "--loss", "berhu", "--silog_mask", "lidar"], "--loss silog"),
    (["--mode", "DtoD", "--loss", "silog", "--silog_lambda", "1"], r"--silog_lambda 1 is not in \[0, 1\)"),
    (["--mode", "DtoD", "--loss", "silog", "--silog_lambda", "-0.1"], "--silog_lambda"),
    (["--mode", "DtoD", "--loss", "silog", "--silog_lambda", "nan"], "--silog_lambda"),
    (["--mode", "DtoD", "--loss", "silog", "--silog_weight", "0"], "--silog_weight"),
    (["--mode", "DtoD", "--loss", "silog", "--silog_weight", "-1"], "--silog_weight"),
    (["--mode", "DtoD", "--loss", "silog", "--silog_weight", "inf"], "--silog_weight"),
    (["--mode", "DtoD", "--loss", "silog", "--silog_floor", "0"], "--silog_floor"),
    (["--mode", "DtoD", "--loss", "silog", "--silog_floor", "1"], "--silog_floor"),
    (["--mode", "RtoD", "--loss", "silog", "--silog_mask", "lidar", "--dataset", "NYU"], "--silog_mask lidar"),
    (["--mode", "DtoD", "--loss", "silog", "--global_berhu"], "--global_berhu"),
]


@pytest.mark.parametrize("flags,match", REFUSALS, ids=[" ".join(f[2:]) + " " + f[1] for f, _ in REFUSALS])
def test_check_loss_refuses_before_the_gpu(flags, match, monkeypatch):
    from gdn_amd import GDN_main, option
    _no_gpu_calls(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = option.parse_args(BASE + flags)
    with pytest.raises(RuntimeError, match=match):
        GDN_main._check_loss(args)
    with pytest.raises(RuntimeError, match=match):
        GDN_main.run(args)


def test_check_loss_refuses_a_loader_without_a_sparse_map(monkeypatch):
    from gdn_amd import GDN_main, datasets, option
    _no_gpu_calls(monkeypatch)

    class NoSparse:
        yields_sparse = False
    args = option.parse_args(BASE + ["--mode", "DtoD", "--loss", "silog", "--silog_mask", "lidar"])
    with pytest.raises(RuntimeError, match="yields no sparse map"):
        GDN_main._check_loss(args, NoSparse())
    with pytest.raises(RuntimeError, match="yields no sparse map"):
        GDN_main.run(args, train_loader=NoSparse())
    assert datasets.GpuNYUAugmentLoader.yields_sparse is False and datasets.GpuNYUResidentLoader.yields_sparse is False
    GDN_main._check_loss(args, object())                                       # a loader that says nothing: KITTI's contract
    GDN_main._check_loss(option.parse_args(BASE + ["--mode", "DtoD", "--loss", "silog", "--silog_mask", "dense"]), NoSparse())


def test_check_loss_accepts():
    from gdn_amd import GDN_main, option
    for flags in ([], ["--loss", "berhu"], ["--loss", "silog"], ["--loss", "silog", "--silog_lambda", "0", "--silog_weight", "0.5"],
                  ["--loss", "silog", "--silog_mask", "lidar"], ["--loss", "berhu", "--global_berhu"]):
        GDN_main._check_loss(option.parse_args(BASE + ["--mode", "RtoD"] + flags))
    GDN_main._check_loss(option.parse_args(BASE + ["--mode", "DtoD_test"]))             # no flag: nothing to refuse
    GDN_main._check_loss(argparse.Namespace(mode="DtoD"))                              # a caller's bare namespace


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_symbol_declared_built_and_bound():
    """gdn_silog_masked is in the header, in the library and in the binding; the loss workspace carries three partial arrays
    of 1024 doubles behind its 64-byte header; every bad argument is refused before anything is launched (status -1, which
    needs no GPU), a short workspace with status -3."""
    import ctypes
    import pathlib
    from gdn_amd import _lib as L
    header = (pathlib.Path(__file__).resolve().parent.parent / "include" / "gdn_hip.h").read_text()
    assert "int gdn_silog_masked(const float* out, const float* gt, const float* sparse, int32_t Cs," in header
    assert "gdn_silog_masked" in L.EXPORTS and "gdn_silog_masked" in L._STATUS_FUNCS
    f = L.lib.raw("gdn_silog_masked")
    for npix in (0, 1, 35, 20 * 128 * 416):
        assert L.lib.gdn_loss_workspace_bytes(npix) == 64 + 3 * 1024 * 8 + 2 * 4 * npix
    P = ctypes.c_void_p
    box = (ctypes.c_int32 * 4)(0, 4, 0, 6)
    good = dict(out=P(0x1000), gt=P(0x2000), sparse=None, Cs=0, B=1, H=4, W=6, box=None, lam=0.85, weight=10.0, floor=0.0125,
                loss=P(0x3000), ws=P(0x4000), nb=L.lib.gdn_loss_workspace_bytes(24))

    def call(**kw):
        a = dict(good, **kw)
        return f(a["out"], a["gt"], a["sparse"], a["Cs"], a["B"], a["H"], a["W"], a["box"], a["lam"], a["weight"], a["floor"],
                 a["loss"], None, None, a["ws"], a["nb"], None)
    bad = [dict(out=None), dict(gt=None), dict(loss=None), dict(B=0), dict(H=-1), dict(W=0), dict(lam=1.0), dict(lam=-0.01),
           dict(lam=float("nan")), dict(weight=0.0), dict(weight=-1.0), dict(weight=float("nan")), dict(floor=0.0), dict(floor=1.0),
           dict(floor=float("nan")), dict(sparse=P(0x5000), Cs=1, box=None), dict(sparse=P(0x5000), Cs=0, box=box)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(ws=None) == -3 and call(nb=good["nb"] - 1) == -3
    with pytest.raises(L.GdnError, match="gdn_silog_masked failed"):
        L.lib.gdn_silog_masked(None, good["gt"], None, 0, 1, 4, 6, None, 0.85, 10.0, 0.0125, good["loss"], None, None, good["ws"],
                               good["nb"], None)


# ---- pixel=None is the old branch -------------------------------------------------------------------------------------
class _Spy:
    def __init__(self, monkeypatch):
        from gdn_amd import ops
        from gdn_amd import utils as U
        self.calls = []
        for name in ("berhu_masked", "silog_masked", "sobel_l1", "smoothness", "absdiff_max"):
            monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: self.calls.append((_n, a, k)))
        monkeypatch.setattr(U, "_c1", lambda t, name: t.detach())
        monkeypatch.setattr(U, "_nchw", lambda t, name: t.detach())
        monkeypatch.setattr(U, "GLOBAL_BERHU", False)

    def names(self):
        return [c[0] for c in self.calls]


def test_pixel_none_takes_the_old_branch(monkeypatch):
    from gdn_amd import utils as U
    spy = _Spy(monkeypatch)
    out, gt, rgb, sparse = torch.zeros(1, 1, 4, 6), torch.zeros(1, 1, 4, 6), torch.zeros(1, 3, 4, 6), torch.zeros(1, 1, 4, 6)
    kinds = []
    real = U._PixelLoss.apply
    monkeypatch.setattr(U._PixelLoss, "apply", staticmethod(lambda pred, kind, args: (kinds.append(kind), real(pred, kind, args))[1]))
    for call in (lambda: U.dtod_loss(out, gt, sparse), lambda: U.dtod_loss(out, gt, sparse, None, None),
                 lambda: U.dtod_loss(out, gt, sparse, pixel=None)):
        del spy.calls[:], kinds[:]
        call()
        assert kinds == ["dtod"] and spy.names() == ["berhu_masked", "sobel_l1"]
        assert spy.calls[0][1][3] == U.crop_box_kitti(4, 6) and spy.calls[0][2] == {"ext_max": None}
    for call in (lambda: U.rtod_pixel_loss(out, gt, rgb, sparse), lambda: U.rtod_pixel_loss(out, gt, rgb, sparse, pixel=None)):
        del spy.calls[:], kinds[:]
        call()
        assert kinds == ["rtod"] and spy.names() == ["berhu_masked", "smoothness"]


def test_pixel_spec_swaps_only_the_pixel_term(monkeypatch):
    from gdn_amd import utils as U
    from gdn_amd._lib import GdnError
    spy = _Spy(monkeypatch)
    out, gt, rgb, sparse = torch.zeros(1, 1, 4, 6), torch.zeros(1, 1, 4, 6), torch.zeros(1, 3, 4, 6), torch.zeros(1, 1, 4, 6)
    U.dtod_loss(out, gt, sparse, pixel=U.silog_spec(0.5, 2.0, 0.05))                  # dense: the sparse map is not handed on
    (name, a, k), (name2, a2, k2) = spy.calls
    assert name == "silog_masked" and a[2] is None and a[3] is None and a[6:] == (0.5, 2.0, 0.05) and not k
    assert name2 == "sobel_l1" and a2[2] == 3.0 and k2["plus"] is a[5] and k2["total"] is not None
    del spy.calls[:]
    U.rtod_pixel_loss(out, gt, rgb, sparse, pixel=U.silog_spec(use_sparse=True))
    (name, a, k), (name2, a2, k2) = spy.calls
    assert name == "silog_masked" and a[2] is not None and a[3] == U.crop_box_kitti(4, 6) and a[6:] == (0.85, 10.0, 0.0125)
    assert name2 == "smoothness" and k2["plus"] is a[5]
    with pytest.raises(GdnError, match="no sparse map"):
        U.dtod_loss(out, gt, None, pixel=U.silog_spec(use_sparse=True))
    with pytest.raises(GdnError, match="pixel must be"):
        U.dtod_loss(out, gt, None, pixel=("huber", 1.0))
    assert U.silog_spec() == ("silog", 0.85, 10.0, 0.0125, False)
