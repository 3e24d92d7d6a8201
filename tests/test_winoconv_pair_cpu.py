"""CPU-side checks of the two-chain F(4x4,3x3) backward's host interface (gdn_winoconv_bwd_pair*): the exports resolve at the
unchanged C ABI revision, and the workspace query covers the four regions the phases keep apart."""
import ctypes
import importlib.util
import pathlib

import pytest

REPO = pathlib.Path(__file__).resolve().parent.parent

# (B, Cin, Cout, H, W): the three cases of test_hip_winoconv_pair.py, then levels 3 and 4 of the BASELINE batch
CASES = [(2, 128, 128, 8, 12), (1, 128, 256, 11, 12), (3, 256, 128, 8, 26), (20, 512, 512, 16, 52), (20, 512, 512, 8, 26)]


@pytest.fixture(scope="module")
def built_lib():
    spec = importlib.util.spec_from_file_location("gdn_build", REPO / "gdn-pytorch_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build()


def test_pair_exports_resolve_at_revision_223(built_lib):
    from gdn_amd._lib import ABI_VERSION, EXPORTS, lib
    dll = ctypes.CDLL(str(built_lib))
    for name in ("gdn_winoconv_bwd_pair_workspace_bytes", "gdn_winoconv_bwd_pair"):
        assert hasattr(dll, name) and name in EXPORTS
        assert lib.raw(name) is not None
    assert ABI_VERSION == 223 and lib.gdn_version() == 223


def al256(v):
    return (v + 255) // 256 * 256


@pytest.mark.parametrize("case", CASES, ids=["b%d_c%d_%d_%dx%d" % c for c in CASES])
def test_pair_workspace_covers_its_four_regions(built_lib, case):
    from gdn_amd._lib import ConvGeom, lib
    B, ci, co, H, W = case
    g = ConvGeom(B, H, W, ci, co, 3, 1, 1, 0, 0)
    tiles = B * ((H + 3) // 4) * ((W + 3) // 4)
    # the layer plans F(4x4,3x3): its saved input transform has 36 bins
    assert lib.gdn_winoconv_state_bytes(ctypes.byref(g)) >= 36 * tiles * ci * 4
    splits = int(lib.gdn_gemm_x3_tn_splits(36, tiles, co, ci))
    assert splits >= 1
    vd = dv = al256(36 * tiles * co * 4)
    p = splits * al256(36 * co * ci * 4)
    eo = al256(36 * tiles * ci * 4)
    assert lib.gdn_winoconv_bwd_pair_workspace_bytes(ctypes.byref(g)) >= vd + dv + p + eo


def test_pair_query_is_zero_where_the_single_stream_form_stays(built_lib):
    from gdn_amd import ops
    from gdn_amd._lib import ConvGeom, lib
    q = lambda g: lib.gdn_winoconv_bwd_pair_workspace_bytes(ctypes.byref(g))
    assert q(ConvGeom(2, 8, 12, 128, 128, 3, 1, 1, 1, 0)) == 0                       # reflection padding
    assert q(ConvGeom(2, 8, 12, 128, 128, 3, 1, 1, 0, 0, ops.HINT_NO_WINO_F4)) == 0   # F(2x2,3x3) by hint
    assert q(ConvGeom(2, 9, 13, 128, 256, 3, 1, 1, 0, 0)) == 0                       # F(2x2,3x3): +64 % tile padding
    assert q(ConvGeom(2, 8, 12, 64, 64, 3, 1, 1, 0, 0)) == 0                         # F(2x2,3x3): 64 channels
    assert q(ConvGeom(2, 8, 12, 128, 128, 4, 2, 1, 0, 0)) == 0                       # not a Winograd layer at all
    for g in (ConvGeom(2, 8, 12, 128, 128, 3, 1, 1, 1, 0), ConvGeom(2, 9, 13, 128, 256, 3, 1, 1, 0, 0)):
        assert lib.gdn_winoconv_bwd_workspace_bytes(ctypes.byref(g)) > 0
