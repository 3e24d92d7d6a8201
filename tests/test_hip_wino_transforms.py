"""GPU tests of the F(4x4,3x3) Winograd data transforms (csrc/conv_wino.hip: wino4_input_kernel and its up2x form,
wino4_output_kernel), driven through the layer entry points: the forward with saved state (V is the head of the state buffer),
gdn_winoconv_bwd_pair, and the single-gradient gdn_winoconv_bwd.

Two checks per case:
  * bitwise, against what the parent commit of the branch-free loaders computed (tests/golden/wino_transforms.npz, written by
    tests/golden/gen_wino_transforms.py, which also owns the cases, the inputs and the calls): the loaders were rescheduled, the
    arithmetic per element was not, so V, y, the BatchNorm partials, dx, dw and the BatchNorm-backward partials keep every bit;
  * against the float64 model of tests/test_winoconv_model_cpu.py at that file's bars: an output (y, dx) within 1e-4 of the
    model's rms, a weight gradient within 1e-4 of its largest entry.

The generator's PLANS / UP2X_REFLECT cases run the same calls through every other plan the host side selects -- F(2x2,3x3)
with the fp32 or bf16 x 3 GEMM per direction, the NO_X3 / NO_WINO_F4 hints, reflection padding (padded-domain data gradient and
its fold, with and without the x2 upsampling's adjoint), flipped taps -- and get the bitwise check against the bits recorded
before the host side was rebuilt as stage launchers and two chains.
"""
import importlib.util
import pathlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_winoconv_model_cpu import wino4_forward, wino4_wgrad

pytestmark = pytest.mark.gpu

_GEN = pathlib.Path(__file__).resolve().parent / "golden" / "gen_wino_transforms.py"
_spec = importlib.util.spec_from_file_location("gen_wino_transforms", _GEN)
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

U32 = 2.0 ** -24           # unit roundoff of fp32


@pytest.fixture(scope="module")
def recorded():
    return np.load(G.DEFAULT_OUT, allow_pickle=False)


class Case:
    """Inputs (numpy), the library's outputs (numpy) and the float64 model's pieces (computed on first use, once)."""

    def __init__(self, dev, g, up=False, plan=None):
        self.g, self.up, self.plan = g, up, plan or {}
        self.inp = G.inputs(g, up, up_bwd=up and plan is not None)
        self.out = {k: v.detach().cpu().numpy() for k, v in (G.run_up2x if up else G.run)(dev, g, self.inp, plan).items()}
        B, ci, co = g[:3]
        self.x = self.inp["xw"][..., 32:32 + ci].astype(np.float64)
        self.w = self.inp["w"].astype(np.float64).reshape(3, 3, co, ci).transpose(2, 3, 0, 1)          # [N, C, 3, 3]
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def conv(self, x, w):
        """Model convolution of NHWC x with [N, C, 3, 3] weights; returns (y NHWC, [V per image])."""
        ys, Vs = zip(*[wino4_forward(np.ascontiguousarray(xb.transpose(2, 0, 1)), w) for xb in x])
        return np.stack([y.transpose(1, 2, 0) for y in ys]), Vs

    def dx_model(self):
        wflip = np.ascontiguousarray(self.w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))
        return self.memo("dx", lambda: self.conv(self.inp["dy"].astype(np.float64), wflip)[0])


@pytest.fixture(scope="module", params=G.GEOMS, ids=[G.gid(g) for g in G.GEOMS])
def case(gpu, request):
    return Case(gpu, request.param)


@pytest.fixture(scope="module", params=G.UP2X, ids=[G.gid(g) for g in G.UP2X])
def upcase(gpu, request):
    return Case(gpu, request.param, up=True)


_PLANS = [(p, False) for p in G.PLANS] + [(p, True) for p in G.UP2X_REFLECT]


@pytest.fixture(scope="module", params=_PLANS, ids=[p[0] for p, _ in _PLANS])
def plancase(gpu, request):
    (pid, g, plan), up = request.param
    c = Case(gpu, g, up=up, plan=plan)
    c.pid = pid
    return c


def assert_bits(c, recorded, prefix):
    bad = []
    for name, a in c.out.items():
        key = "%s%s/%s" % (prefix, G.gid(c.g), name)
        assert np.isfinite(a).all() and np.abs(a).max() > 0, name
        if not np.array_equal(G.digest(a), recorded[key + "/sha"]):
            s, r = G.sample(a), recorded[key + "/sample"]
            diff = s.view(np.int32).astype(np.int64) - r.view(np.int32).astype(np.int64)
            bad.append("%s: %d of %d sampled values differ, up to %d ulp" % (name, int((diff != 0).sum()), s.size,
                                                                             int(np.abs(diff).max())))
    assert not bad, "not the recorded bits -- " + "; ".join(bad)


def assert_output(got, ref, rms_of, what):
    """The model file's bar for an F(4x4,3x3) output: worst element within 1e-4 of the convolution's rms."""
    rms = float(np.sqrt((rms_of ** 2).mean()))
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("%s: max err %.3e, bar %.3e" % (what, err, 1e-4 * rms))
    assert err < 1e-4 * rms, what


def test_cases_are_f4_plans(case):
    from gdn_amd import ops
    from gdn_amd._lib import lib
    B, ci, co, H, W = case.g
    _, ref, _, _ = ops.Conv(ci, co, 3, 1, 1).geom(B, H, W)
    assert lib.gdn_winoconv_bwd_pair_workspace_bytes(ref) > 0          # (0 for every plan but F(4x4,3x3))
    assert case.out["f1.V"].size == 36 * G.tiles(B, H, W) * ci


def test_bits_are_the_parents(case, recorded):
    assert_bits(case, recorded, "")


def test_up2x_bits_are_the_parents(upcase, recorded):
    assert_bits(upcase, recorded, "up2x_")


def test_plan_cases_run_the_plan_they_name(plancase):
    """The library's own queries, under the case's switches: the two-chain backward exists for F(4x4,3x3) plans only, a
    statistics slot is 4 tiles of the plan's tiling, and a reflection layer emits no BatchNorm-backward partials."""
    from gdn_amd._lib import lib
    B, ci, co, H, W = plancase.g
    if plancase.up:
        H, W = 2 * H, 2 * W
    T = plancase.plan["T"]
    with G.switches(plancase.plan):
        op, nV = G.layer((B, ci, co, H, W), plancase.plan)
        _, ref, _, _ = op.geom(B, H, W)
        assert (lib.gdn_winoconv_bwd_pair_workspace_bytes(ref) > 0) == (T == 4)
        assert lib.gdn_winoconv_stats_slots(ref) == (G.tiles(B, H, W, T) + 3) // 4
        assert (op.wino_bnb_slots(B, H, W) == 0) == bool(plancase.plan.get("reflect"))
    assert plancase.out["u1.V" if plancase.up else "f1.V"].size == nV


def test_plan_bits_are_the_parents(plancase, recorded):
    """Every output of every plan, bit for bit, as the library computed it before its host side became stage launchers."""
    assert ("b1.part" in plancase.out) == (not plancase.up and not plancase.plan.get("reflect"))
    assert_bits(plancase, recorded, plancase.pid + "_")


def test_forward_plain_matches_model(case):
    y64, _ = case.memo("f1", lambda: case.conv(case.x, case.w))
    assert_output(case.out["f1.y"], y64, y64, "f1.y")


def test_forward_bn_relu_on_load_affine_relu_residual_matches_model(case):
    i = case.inp
    xin = np.maximum(case.x * i["in_s"].astype(np.float64) + i["in_t"].astype(np.float64), 0.0)
    y64, _ = case.conv(xin, case.w)
    co = case.g[2]
    ref = np.maximum(y64 * i["ep_s"].astype(np.float64) + i["ep_t"].astype(np.float64), 0.0) + i["addw"][..., :co].astype(np.float64)
    assert_output(case.out["f2.y"], ref, y64, "f2.y")          # (ep_s <= 1: the epilogue does not enlarge the error)


def test_forward_bn_on_load_matches_model(case):
    i = case.inp
    y64, _ = case.conv(case.x * i["in_s"].astype(np.float64) + i["in_t"].astype(np.float64), case.w)
    assert_output(case.out["f3.y"], y64, y64, "f3.y")


def test_data_gradients_match_model(case):
    dx64 = case.dx_model()
    ci = case.g[1]
    assert_output(case.out["b1.dx"], dx64 + case.inp["gaddw"][..., :ci].astype(np.float64), dx64, "b1.dx (pair, + residual)")
    assert_output(case.out["b2.dx"], dx64, dx64, "b2.dx (single, saved weights)")
    assert_output(case.out["b3.dx"], dx64, dx64, "b3.dx (single, no state)")


def test_weight_gradients_match_model(case):
    _, Vs = case.memo("f1", lambda: case.conv(case.x, case.w))
    gy = case.inp["dy"].astype(np.float64)
    dw64 = sum(wino4_wgrad(V, np.ascontiguousarray(g.transpose(2, 0, 1))) for V, g in zip(Vs, gy))      # [N, C, 3, 3]
    co, ci = case.g[2], case.g[1]
    ref = dw64.transpose(2, 3, 0, 1).reshape(9, co, ci)
    for name in ("b1.dw", "b4.dw"):
        err = float(np.abs(case.out[name].astype(np.float64) - ref).max())
        print("%s: max err %.3e, bar %.3e" % (name, err, 1e-4 * np.abs(ref).max()))
        assert err < 1e-4 * np.abs(ref).max(), name


def test_partials_are_the_sums_of_what_was_written(case):
    """The BatchNorm partials (forward) and BatchNorm-backward partials (data gradient) against float64 sums over the tensor
    the same launch wrote.  A slot is 4 tiles x 16 pixels per channel, summed in fp32: 16 sequential additions per thread and
    3 across threads, so its error is below 19 u sum|term|; the backward's second term (dz * ((y - mean) * istd)) is itself
    rounded twice before the fused multiply-add, 2 u more.  Bars: 32 u sum|term| over the whole tensor."""
    i, o = case.inp, case.out
    y = o["f1.y"].astype(np.float64)
    st = o["f1.stats"].astype(np.float64).sum(axis=0)
    for k, term in enumerate((y, y * y)):
        ref, mag = term.sum(axis=(0, 1, 2)), np.abs(term).sum(axis=(0, 1, 2))
        assert (np.abs(st[k] - ref) <= 32 * U32 * mag).all(), "stats[%d]" % k
    dz = o["b2.dx"].astype(np.float64)
    bco = i["bco"].astype(np.float64)
    xhat = (i["by"].astype(np.float64) - bco[2]) * bco[3]
    pt = o["b2.part"].astype(np.float64).sum(axis=0)
    for k, term in enumerate((dz, dz * xhat)):
        ref, mag = term.sum(axis=(0, 1, 2)), np.abs(term).sum(axis=(0, 1, 2))
        assert (np.abs(pt[k] - ref) <= 32 * U32 * mag).all(), "bnb partial[%d]" % k


@pytest.mark.parametrize("mode", [1, 2], ids=["half_pixel", "align_corners"])
def test_up2x_forward_matches_model(upcase, mode):
    xl = torch.from_numpy(np.ascontiguousarray(upcase.x.transpose(0, 3, 1, 2)))
    xu = F.interpolate(xl, scale_factor=2, mode="bilinear", align_corners=(mode == 2)).numpy().transpose(0, 2, 3, 1)
    y64, _ = upcase.conv(xu, upcase.w)
    assert_output(upcase.out["u%d.y" % mode], y64, y64, "u%d.y" % mode)
