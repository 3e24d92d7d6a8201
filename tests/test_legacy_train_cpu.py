"""CPU-side tests for training the legacy AutoEncoder: the command line (--rtod_arch, --init_from, depth_extract --arch), the
GDN_HINT_FLIP_TAPS bit in header, binding and host queries, and the engine's choice of the flipped-tap form."""
import pathlib
import re

import pytest
import torch

REPO = pathlib.Path(__file__).resolve().parent.parent


def test_parser_defaults_and_historical_architectures():
    from gdn_amd import option
    a = option.parse_args(["DATA"])
    assert a.rtod_arch is None and a.init_from is None
    # the pre-existing commands build what they always built
    for mode, arch in (("RtoD", "unet"), ("RtoD_single", "unet"), ("RtoD_test", "legacy")):
        assert option.rtod_arch(option.parse_args(["DATA", "--mode", mode])) == arch
    for mode in ("RtoD", "RtoD_single", "RtoD_test"):
        for arch in ("unet", "legacy"):
            assert option.rtod_arch(option.parse_args(["DATA", "--mode", mode, "--rtod_arch", arch])) == arch
    with pytest.raises(SystemExit):
        option.parse_args(["DATA", "--rtod_arch", "resnet"])
    # a Namespace built by hand (tests, notebooks) without the new attributes still resolves
    import argparse
    assert option.rtod_arch(argparse.Namespace(mode="RtoD_test")) == "legacy"
    assert option.parse_args(["DATA", "--init_from", "x.pkl"]).init_from == "x.pkl"


def test_rtod_network_and_init_from(tmp_path):
    import gdn_amd.AE_model_unet as M
    from gdn_amd import GDN_main, option
    mk = lambda *extra: option.parse_args(["DATA", "--height", "32", "--width", "64", *extra])
    assert type(GDN_main._rtod_network(mk("--mode", "RtoD"), 32, 64)) is M.AutoEncoder_2
    assert type(GDN_main._rtod_network(mk("--mode", "RtoD_test"), 32, 64)) is M.AutoEncoder
    assert type(GDN_main._rtod_network(mk("--mode", "RtoD", "--rtod_arch", "legacy"), 32, 64)) is M.AutoEncoder
    assert type(GDN_main._rtod_network(mk("--mode", "RtoD_test", "--rtod_arch", "unet"), 32, 64)) is M.AutoEncoder_2
    # --init_from: reference-format (module.-prefixed) and bare state dicts, bit for bit; a missing file is an error
    torch.manual_seed(1)
    src = M.AutoEncoder(height=32, width=64)
    for name, sd in (("ref.pkl", {"module." + k: v for k, v in src.state_dict().items()}), ("bare.pkl", src.state_dict())):
        torch.save(sd, tmp_path / name)
        torch.manual_seed(2)
        net = GDN_main._rtod_network(mk("--mode", "RtoD", "--rtod_arch", "legacy"), 32, 64)
        assert not torch.equal(net.upconv1.weight, src.upconv1.weight)
        GDN_main._init_from(net, mk("--init_from", str(tmp_path / name)), 0)
        for k, v in net.state_dict().items():
            assert torch.equal(v, src.state_dict()[k]), k
    with pytest.raises(FileNotFoundError, match="nothing.pkl"):
        GDN_main._init_from(net, mk("--init_from", str(tmp_path / "nothing.pkl")), 0)
    GDN_main._init_from(net, mk(), 0)                    # no flag: nothing to do
    with pytest.raises(RuntimeError, match="state_dict"):      # the other architecture's keys do not load
        GDN_main._init_from(M.AutoEncoder_2(height=32, width=64), mk("--init_from", str(tmp_path / "ref.pkl")), 0)


def test_depth_extract_has_arch_flag():
    from gdn_amd import depth_extract
    with pytest.raises(SystemExit):
        depth_extract.main(["--img_dir", "x", "--arch", "resnet"])


def test_flip_taps_hint_in_header_binding_and_host_queries():
    import ctypes
    from gdn_amd import ops
    from gdn_amd._lib import ConvGeom, lib
    header = (REPO / "include" / "gdn_hip.h").read_text()
    m = re.search(r"GDN_HINT_FLIP_TAPS\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == ops.HINT_FLIP_TAPS == 32
    assert int(lib.gdn_hints_supported()) & ops.HINT_FLIP_TAPS
    q = lambda fn, g: int(getattr(lib, fn)(ctypes.byref(g)))
    for ci, co, k, H, W in ((256, 128, 5, 64, 208), (128, 64, 7, 128, 416)):
        plain = ConvGeom(20, H, W, ci, co, k, 1, k // 2, 0, 0, 0)
        flip = ConvGeom(20, H, W, ci, co, k, 1, k // 2, 0, 0, ops.HINT_FLIP_TAPS)
        tr = ConvGeom(20, H, W, ci, co, k, 1, k // 2, 0, 1, 0)
        # the flipped form plans exactly like the plain convolution of the same shape ...
        for fn in ("gdn_fftconv_spectrum_bytes", "gdn_fftconv_fwd_workspace_bytes", "gdn_fftconv_bwd_workspace_bytes",
                   "gdn_fftconv_bnb_slots", "gdn_fftconv_stats_slots"):
            assert q(fn, flip) == q(fn, plain) > 0, fn
        # ... and what a transposed = 1 geometry answers is what it always answered: forward only
        assert q("gdn_fftconv_spectrum_bytes", tr) > 0
        assert q("gdn_fftconv_bwd_workspace_bytes", tr) == 0 and q("gdn_fftconv_bnb_slots", tr) == 0
    plain = ConvGeom(20, 32, 104, 512, 256, 3, 1, 1, 0, 0, 0)
    flip = ConvGeom(20, 32, 104, 512, 256, 3, 1, 1, 0, 0, ops.HINT_FLIP_TAPS)
    for fn in ("gdn_winoconv_state_bytes", "gdn_winoconv_fwd_workspace_bytes", "gdn_winoconv_bwd_workspace_bytes",
               "gdn_winoconv_bnb_slots"):
        assert q(fn, flip) == q(fn, plain) > 0, fn
    assert q("gdn_winoconv_state_bytes", ConvGeom(20, 32, 104, 512, 256, 3, 1, 1, 0, 1, 0)) == 0
    # not a layer the hint describes: reflection padding, or together with transposed
    for bad in (ConvGeom(2, 32, 64, 128, 64, 7, 1, 3, 1, 0, ops.HINT_FLIP_TAPS), ConvGeom(2, 32, 64, 128, 64, 7, 1, 3, 0, 1, ops.HINT_FLIP_TAPS)):
        assert q("gdn_fftconv_spectrum_bytes", bad) == 0
    assert q("gdn_winoconv_state_bytes", ConvGeom(2, 32, 64, 128, 64, 3, 1, 1, 1, 0, ops.HINT_FLIP_TAPS)) == 0
    # ops.Conv: the constructor argument and the answers of fft_ok / wino_ok
    f5, t5 = ops.Conv(256, 128, 5, 1, 2, flip_taps=True), ops.Conv(256, 128, 5, 1, 2, transposed=True)
    assert f5.fft_ok(20, 64, 208) and f5.fft_ok(20, 64, 208, backward=True) and f5.fft_ok(20, 64, 208, backward=True, train=True)
    assert t5.fft_ok(20, 64, 208) and not t5.fft_ok(20, 64, 208, backward=True)
    f3 = ops.Conv(512, 256, 3, 1, 1, flip_taps=True)
    assert f3.wino_ok(20, 32, 104) and f3.wino_ok(20, 32, 104, backward=True) and not f3.fft_ok(20, 32, 104)
    assert not ops.Conv(512, 256, 3, 1, 1, transposed=True).wino_ok(20, 32, 104, backward=True)


def test_engine_selects_the_flipped_form_only_under_a_recorded_fp32_tape():
    import torch.nn as nn
    from gdn_amd import engine as E
    bn = nn.BatchNorm2d(128)
    up = nn.ConvTranspose2d(256, 128, 5, 1, 2, bias=False)
    rec, norec = E.Ctx(record=True), E.Ctx(record=False)
    op = E._flip_op(rec, up, bn, torch.float32, None)
    assert op is not None and op.flip_taps and not op.transposed and (op.cin, op.cout, op.k, op.pad) == (256, 128, 5, 2)
    assert E._flip_op(rec, up, bn, torch.float32, None) is op                     # built once per module
    assert E._flip_op(norec, up, bn, torch.float32, None) is None                 # inference: the transposed op, as ever
    assert E._flip_op(E.Ctx(record=True, dtype=torch.bfloat16), up, bn, torch.bfloat16, None) is None
    assert E._flip_op(rec, up, bn, torch.float32, torch.zeros(1)) is None         # concatenated input
    assert E._flip_op(rec, nn.ConvTranspose2d(256, 128, 4, 2, 1, bias=False), bn, torch.float32, None) is None
    assert E._flip_op(rec, nn.ConvTranspose2d(256, 128, 5, 1, 1, bias=False), bn, torch.float32, None) is None
    assert E._flip_op(rec, nn.Conv2d(256, 128, 5, 1, 2, bias=False), bn, torch.float32, None) is None
    inorm = nn.InstanceNorm2d(128, affine=True, track_running_stats=True)
    assert E._flip_op(rec, up, inorm, torch.float32, None) is None
    assert E._flip_op(rec, up, inorm.eval(), torch.float32, None) is op
