"""GPU tests of the two-chain F(4x4,3x3) Winograd backward (csrc/conv_wino.hip: gdn_winoconv_bwd_pair;
ops.Conv.wino_bwd's fork / join).  The arithmetic is gdn_winoconv_bwd's and only the schedule differs, so every comparison is
bitwise equality -- between the forked form, the phased entry point on one stream and gdn_winoconv_bwd.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, Cin, Cout, H, W): whole tiles; a partial last tile row with Cin != Cout; a partial last tile column with 42 tiles (not a
# multiple of the 4 tiles of a transform workgroup)
CASES = [(2, 128, 128, 8, 12), (1, 128, 256, 11, 12), (3, 256, 128, 8, 26)]
IDS = ["b%d_c%d_%d_%dx%d" % c for c in CASES]
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3


def al256(v):
    return (v + 255) // 256 * 256


class Layer:
    """One layer's forward state, inputs of the backward, and the argument lists of the two C entry points."""

    def __init__(self, gpu, case):
        from gdn_amd import ops
        from gdn_amd._lib import lib
        self.ops, self.lib = ops, lib
        B, ci, co, H, W = self.case = case
        gen = torch.Generator(device=gpu).manual_seed(5 + H * W)
        rnd = lambda *s: torch.randn(*s, device=gpu, generator=gen)
        self.op = ops.Conv(ci, co, 3, 1, 1)
        self.x, self.w = rnd(B, H, W, ci), rnd(9, co, ci) / (ci * 9) ** 0.5
        self.dy, self.gres, self.by = rnd(B, H, W, co), rnd(B, H, W, ci), rnd(B, H, W, ci)
        self.bco = torch.stack([torch.rand(ci, device=gpu, generator=gen) + 0.5, rnd(ci), rnd(ci) * 0.1,
                                torch.rand(ci, device=gpu, generator=gen) + 0.5]).contiguous()
        _, self.sv = self.op.wino_fwd(self.x, self.w, state=True)
        _, self.ref, _, _ = self.op.geom(B, H, W)
        self.tiles = B * ((H + 3) // 4) * ((W + 3) // 4)
        self.slots = self.op.wino_bnb_slots(B, H, W)
        self.nb = int(lib.gdn_winoconv_bwd_workspace_bytes(self.ref))
        self.npair = int(lib.gdn_winoconv_bwd_pair_workspace_bytes(self.ref))

    def outputs(self, bnb):
        B, ci, co, H, W = self.case
        dx = torch.full((B, H, W, ci), 3.0, device=self.x.device)
        dw = torch.full_like(self.w, 7.0)
        part = torch.full((self.slots, 2, ci), 5.0, device=self.x.device) if bnb else None
        return dx, dw, part

    def args(self, dx, dw, addsrc, part, state=True):
        p, ld = self.ops._p, self.ops._ld
        return [self.ref, p(self.dy), ld(self.dy), p(self.w), p(self.sv) if state else None, p(dx), 0 if dx is None else ld(dx),
                p(addsrc), 0 if addsrc is None else ld(addsrc), p(dw), p(self.by) if part is not None else None,
                ld(self.by) if part is not None else 0, p(self.bco) if part is not None else None, 1, p(part), 0]

    def single(self, addsrc=None, bnb=False, dx=True, dw=True):
        """gdn_winoconv_bwd; returns (dx, dw, partial, workspace)."""
        odx, odw, part = self.outputs(bnb)
        ws = torch.zeros(self.nb, dtype=torch.uint8, device=self.x.device)
        self.lib.gdn_winoconv_bwd(*self.args(odx if dx else None, odw if dw else None, addsrc, part), ws.data_ptr(), self.nb,
                                  self.ops.stream())
        return odx, odw, part, ws

    def pair(self, phases, addsrc=None, bnb=False):
        """gdn_winoconv_bwd_pair on the current stream; returns (dx, dw, partial, workspace)."""
        odx, odw, part = self.outputs(bnb)
        ws = torch.zeros(self.npair, dtype=torch.uint8, device=self.x.device)
        self.lib.gdn_winoconv_bwd_pair(*self.args(odx, odw, addsrc, part), phases, ws.data_ptr(), self.npair, self.ops.stream())
        return odx, odw, part, ws

    def forked(self, addsrc=None, bnb=False):
        """ops.Conv.wino_bwd with both gradients; returns (dx, dw, partial)."""
        _, odw, part = self.outputs(bnb)
        B, ci, co, H, W = self.case
        odx = self.op.wino_bwd(self.dy, self.w, (H, W), state=self.sv, dw_tap=odw, addsrc=addsrc,
                               bnb=(self.by, self.bco, True, part) if bnb else None)
        return odx, odw, part


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def layer(gpu, request):
    return Layer(gpu, request.param)


def test_pair_query_is_nonzero_for_the_cases(layer):
    assert layer.npair > 0 and layer.nb > 0
    assert layer.lib.gdn_winoconv_state_bytes(layer.ref) >= 36 * layer.tiles * layer.case[1] * 4      # 36 bins: an F(4x4,3x3) plan


def test_pair_transform_is_bitwise_the_two_transforms(layer):
    """Phase 1 alone: Vd and Dv (the first two regions of the pair workspace) against what wino4_input_kernel / wino4_dy_kernel
    leave at the start of gdn_winoconv_bwd's workspace in a dx-only / dw-only call."""
    B, ci, co, H, W = layer.case
    n = 36 * layer.tiles * co
    _, _, _, ws = layer.pair(1)
    f = ws.view(torch.float32)
    vd, dv = f[:n], f[al256(4 * n) // 4:al256(4 * n) // 4 + n]
    vd_ref = layer.single(dw=False)[3].view(torch.float32)[:n]
    dv_ref = layer.single(dx=False)[3].view(torch.float32)[:n]
    assert float(vd_ref.abs().max()) > 0 and float(dv_ref.abs().max()) > 0
    assert torch.equal(vd.view(torch.int32), vd_ref.view(torch.int32)), "Vd"
    assert torch.equal(dv.view(torch.int32), dv_ref.view(torch.int32)), "Dv"
    # phase 1 wrote nothing else: the partial-product and GEMM-output regions are still zero
    assert not bool(f[2 * (al256(4 * n) // 4):].any())


@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "addsrc"])
@pytest.mark.parametrize("with_bnb", [False, True], ids=["nobnb", "bnb"])
def test_pair_gradients_are_bitwise_equal_in_all_three_forms(layer, with_add, with_bnb):
    add = layer.gres if with_add else None
    ref = layer.single(add, with_bnb)[:3]
    one = layer.pair(0, add, with_bnb)[:3]
    fork = layer.forked(add, with_bnb)
    torch.cuda.synchronize()
    assert float(ref[0].abs().max()) > 0 and float(ref[1].abs().max()) > 0
    for what, got in (("phases = 0", one), ("forked", fork)):
        for name, a, b in zip(("dx", "dw", "bnb partial"), got, ref):
            if b is None:
                assert a is None
                continue
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: %s differs from gdn_winoconv_bwd" % (what, name)


def test_pair_phases_one_by_one_equal_phase_zero(layer):
    a = layer.pair(0, layer.gres, True)
    odx, odw, part = layer.outputs(True)
    ws = torch.zeros(layer.npair, dtype=torch.uint8, device=odx.device)
    for ph in (1, 4, 2):          # the two chains in the other order: they do not depend on each other
        layer.lib.gdn_winoconv_bwd_pair(*layer.args(odx, odw, layer.gres, part), ph, ws.data_ptr(), layer.npair, layer.ops.stream())
    for x, y in zip((odx, odw, part, ws), a):
        assert torch.equal(x, y)


def test_forked_form_repeats_bitwise(layer):
    first = layer.forked(layer.gres, True)
    for _ in range(10):
        again = layer.forked(layer.gres, True)
        for a, b in zip(again, first):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_forked_form_captures_in_a_graph(layer):
    """The fork / join is capturable (GraphedTrainStep captures the whole step) and a replay equals the eager result."""
    eager = layer.forked(layer.gres, True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        layer.forked(layer.gres, True)          # sizes the workspace outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = layer.forked(layer.gres, True)
    for t in out:
        t.fill_(9.0)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _count_calls(monkeypatch, lib):
    calls = {"gdn_winoconv_bwd": 0, "gdn_winoconv_bwd_pair": 0}
    for name in calls:
        fn = getattr(lib, name)

        def counted(*a, _fn=fn, _name=name):
            calls[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counted)
    return calls


def test_dispatch_pair_only_for_both_gradients_of_f4_layers(gpu, layer, monkeypatch):
    ops, lib = layer.ops, layer.lib
    B, ci, co, H, W = layer.case
    calls = _count_calls(monkeypatch, lib)
    dw = torch.empty_like(layer.w)
    layer.op.wino_bwd(layer.dy, layer.w, (H, W), state=layer.sv, dw_tap=dw)
    assert calls == {"gdn_winoconv_bwd": 0, "gdn_winoconv_bwd_pair": 3}          # phases 1, 2, 4
    layer.op.wino_bwd(layer.dy, layer.w, (H, W), state=layer.sv)                    # dx only
    layer.op.wino_bwd(layer.dy, layer.w, (H, W))                                    # dx only, no state
    layer.op.wino_bwd(layer.dy, layer.w, (H, W), state=layer.sv, dw_tap=dw, need_dx=False)
    assert calls == {"gdn_winoconv_bwd": 3, "gdn_winoconv_bwd_pair": 3}
    # F(2x2,3x3) by the switch, and a reflection-padded layer: both gradients, single-stream form
    ops.set_wino_f4(False)
    try:
        _, sv2 = layer.op.wino_fwd(layer.x, layer.w, state=True)
        _, ref2, _, _ = layer.op.geom(B, H, W)
        assert lib.gdn_winoconv_bwd_pair_workspace_bytes(ref2) == 0
        layer.op.wino_bwd(layer.dy, layer.w, (H, W), state=sv2, dw_tap=dw)
    finally:
        ops.set_wino_f4(True)
    opr = ops.Conv(ci, co, 3, 1, 1, reflect=True)
    _, svr = opr.wino_fwd(layer.x, layer.w, state=True)
    _, refr, _, _ = opr.geom(B, H, W)
    assert lib.gdn_winoconv_bwd_pair_workspace_bytes(refr) == 0
    opr.wino_bwd(layer.dy, layer.w, (H, W), state=svr, dw_tap=dw)
    torch.cuda.synchronize()
    assert calls == {"gdn_winoconv_bwd": 5, "gdn_winoconv_bwd_pair": 3}


def test_pair_entry_point_refuses_what_it_is_not_for(gpu, layer):
    ops, lib = layer.ops, layer.lib
    B, ci, co, H, W = layer.case
    raw = lib.raw("gdn_winoconv_bwd_pair")
    odx, odw, part = layer.outputs(False)
    ws = torch.zeros(layer.npair, dtype=torch.uint8, device=gpu)
    tail = lambda nbytes, phases=0: [phases, ws.data_ptr(), nbytes, ops.stream()]
    assert raw(*layer.args(None, odw, None, None), *tail(layer.npair)) == BAD_ARG           # dw only
    assert raw(*layer.args(odx, None, None, None), *tail(layer.npair)) == BAD_ARG           # dx only
    assert raw(*layer.args(odx, odw, None, None, state=False), *tail(layer.npair)) == BAD_ARG
    assert raw(*layer.args(odx, odw, None, None), *tail(layer.npair, 8)) == BAD_ARG
    assert raw(*layer.args(odx, odw, None, None), *tail(layer.npair - 256)) == WORKSPACE
    assert raw(*layer.args(odx, odw, None, None), 0, None, layer.npair, ops.stream()) == WORKSPACE
    for hints, reflect in ((ops.HINT_NO_WINO_F4, False), (0, True)):
        _, ref, _, _ = ops.Conv(ci, co, 3, 1, 1, reflect=reflect).geom(B, H, W, hints=hints)
        a = layer.args(odx, odw, None, None)
        a[0] = ref
        assert lib.gdn_winoconv_bwd_pair_workspace_bytes(ref) == 0
        assert raw(*a, *tail(layer.npair)) == UNSUPPORTED
    torch.cuda.synchronize()
    # nothing was launched by the refused calls
    assert bool((odx == 3.0).all()) and bool((odw == 7.0).all()) and not bool(ws.any())
