"""Gradient guard of the fused Adam (gradient-norm clipping, non-finite step skipping): what needs no GPU -- the C ABI's
declarations, the command-line flags, the optimizer's constructor contract and the float64 restatement of the device
record the GPU tests compare against."""
import pathlib
import re
import struct

import numpy as np
import pytest
import torch

import grad_guard_fp64 as R

REPO = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ("gdn_grad_sumsq", "gdn_grad_guard_finalize", "gdn_adam_step_dev_guarded")


def test_symbols_declared_and_bound_without_a_revision_bump():
    from gdn_amd import _lib
    hdr = (REPO / "include" / "gdn_hip.h").read_text()
    declared = set(re.findall(r"\b(gdn_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS + ("gdn_grad_sumsq_workspace_bytes",):
        assert name in declared, name
        assert name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 223
    csrc = REPO / "gdn-pytorch_amd" / "csrc"
    assert re.search(r"gdn_version\(void\)\s*\{\s*return 223;", (csrc / "pointwise.hip").read_text())
    # every kernel of the feature files under the optimizer in tools/kernel_family.py: its name contains 'adam'
    src = (csrc / "optim.hip").read_text()
    kernels = re.findall(r"__global__(?:\s+__launch_bounds__\(\d+\))?\s+void\s+(\w+)\s*\(", src)
    new_kernels = [k for k in kernels if "gradnorm" in k or "guard" in k]
    assert len(new_kernels) >= 4 and all("adam" in k for k in new_kernels), new_kernels


def test_flags_defaults_and_refusal(capsys):
    from gdn_amd import option
    a = option.parse_args(["--synthetic"])
    assert a.clip_grad_norm == 0 and a.skip_nonfinite is False
    b = option.parse_args(["--synthetic", "--clip_grad_norm", "1.5", "--skip_nonfinite"])
    assert b.clip_grad_norm == 1.5 and b.skip_nonfinite is True
    with pytest.raises(SystemExit) as e:
        option.parse_args(["--synthetic", "--clip_grad_norm", "-1"])
    assert e.value.code != 0
    assert "clip_grad_norm" in capsys.readouterr().err


def test_make_optimizer_passes_the_flags_on():
    from gdn_amd import GDN_main, option
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4))
    plain = GDN_main._make_optimizer(net, option.parse_args(["--synthetic"]))
    assert plain.capturable is False and plain.guarded is False and plain.max_grad_norm is None
    assert "guard" not in plain.state_dict()["gdn"]
    assert sorted(plain.state_dict()["gdn"]) == ["capturable", "grad_scale", "stores", "version"]
    both = GDN_main._make_optimizer(net, option.parse_args(["--synthetic", "--clip_grad_norm", "2.5", "--skip_nonfinite"]))
    assert both.max_grad_norm == 2.5 and both.skip_nonfinite is True and both.capturable is True
    assert both.state_dict()["gdn"]["guard"] == {"max_grad_norm": 2.5, "skip_nonfinite": True, "steps": 0, "clipped": 0,
                                                 "skipped": 0}
    clip = GDN_main._make_optimizer(net, option.parse_args(["--synthetic", "--clip_grad_norm", "1"]))
    assert clip.max_grad_norm == 1.0 and clip.skip_nonfinite is False and clip.capturable is True
    skip = GDN_main._make_optimizer(net, option.parse_args(["--synthetic", "--skip_nonfinite"]))
    assert skip.max_grad_norm is None and skip.skip_nonfinite is True and skip.capturable is True


def test_constructor_contract():
    from gdn_amd._lib import GdnError
    from gdn_amd.optim import Adam
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (0, -1, 0.0, float("nan")):
        with pytest.raises(ValueError):
            Adam(p, max_grad_norm=bad)
    assert Adam(p).capturable is False and Adam(p, capturable=True).guarded is False
    with pytest.raises(GdnError):
        Adam(p).guard_stats()
    opt = Adam(p, max_grad_norm=3.0)
    assert opt.guard_stats() == {"norm": 0.0, "coef": 1.0, "steps": 0, "clipped": 0, "skipped": 0}
    # counters read from a checkpoint wait for the record and are handed back meanwhile
    sd = opt.state_dict()
    sd["gdn"]["guard"].update(steps=7, clipped=3, skipped=2)
    fresh = Adam(p, max_grad_norm=3.0)
    fresh.load_state_dict(sd)
    assert fresh.state_dict()["gdn"]["guard"] == {"max_grad_norm": 3.0, "skip_nonfinite": False, "steps": 7, "clipped": 3,
                                                  "skipped": 2}
    # an unguarded optimizer ignores the key, and its own dict stays what it was
    plain = Adam(p)
    plain.load_state_dict(sd)
    assert "guard" not in plain.state_dict()["gdn"]


def test_restatement_record_layout():
    assert R.RECORD_BYTES == 32
    raw = struct.pack("<dffiiii", 2.25, 1.5, 0.5, 1, 9, 4, 3)
    rec = R.unpack(raw)
    assert rec == {"sumsq": 2.25, "norm": np.float32(1.5), "coef": np.float32(0.5), "skip": 1, "steps": 9, "clipped": 4,
                   "skipped": 3}


def test_restatement_sumsq():
    assert R.sumsq(np.array([3.0, 4.0], np.float32)) == 25.0
    big = R.sumsq(np.array([1e30, 1.0], np.float32))
    assert np.isfinite(big) and big == pytest.approx(float(np.float32(1e30)) ** 2, rel=1e-15)   # float32 squaring would be inf
    for bad in (np.nan, np.inf, -np.inf):
        assert not np.isfinite(R.sumsq(np.array([1.0, bad, 2.0], np.float32)))
    rec = R.accumulate(R.new_record(), np.array([3.0], np.float32))
    rec = R.accumulate(rec, np.array([4.0], np.float32), accumulate=True)
    assert rec["sumsq"] == 25.0
    assert R.accumulate(rec, np.array([2.0], np.float32))["sumsq"] == 4.0          # accumulate=False starts over


def test_restatement_four_branches_and_counters():
    g = np.array([3.0, 4.0], np.float32)               # norm 5
    rec = R.new_record()
    # finite, clipping on: above, equal (the 1e-6 in the denominator keeps it a hair under 1), below
    r = R.finalize(R.accumulate(rec, g), 1.0, 2.0)
    assert r["norm"] == np.float32(5.0) and r["coef"] == np.float32(2.0 / (5.0 + 1e-6)) and r["skip"] == 0
    assert (r["steps"], r["clipped"], r["skipped"]) == (1, 1, 0)
    r = R.finalize(R.accumulate(rec, g), 1.0, 5.0)
    assert r["coef"] == np.float32(5.0 / (5.0 + 1e-6)) and r["coef"] < 1 and (r["steps"], r["clipped"]) == (2, 2)
    r = R.finalize(R.accumulate(rec, g), 1.0, 50.0)
    assert r["coef"] == np.float32(1.0) and (r["steps"], r["clipped"], r["skipped"]) == (3, 2, 0)
    # grad_scale enters the norm: 5 * 0.125 = 0.625 under a bound of 1 is not clipped, 5 * 0.5 is
    assert R.finalize(R.accumulate(rec, g), 0.125, 1.0)["coef"] == np.float32(1.0)
    r = R.finalize(R.accumulate(rec, g), -0.5, 1.0)
    assert r["norm"] == np.float32(2.5) and r["coef"] == np.float32(1.0 / (2.5 + 1e-6)) and r["clipped"] == 3
    # finite, clipping off
    r = R.finalize(R.accumulate(rec, g), 1.0, 0.0)
    assert r["coef"] == np.float32(1.0) and r["skip"] == 0 and (r["steps"], r["clipped"]) == (6, 3)
    # non-finite with skip_nonfinite: skipped, coefficient 0, not counted as clipped
    bad = np.array([3.0, np.inf], np.float32)
    r = R.finalize(R.accumulate(rec, bad), 1.0, 2.0, skip_nonfinite=True)
    assert r["skip"] == 1 and r["coef"] == np.float32(0.0) and not np.isfinite(r["norm"])
    assert (r["steps"], r["clipped"], r["skipped"]) == (7, 3, 1)
    # non-finite without it: passes through exactly like an unguarded step, whatever max_norm says
    for mx in (2.0, 0.0):
        r = R.finalize(R.accumulate(rec, np.array([np.nan], np.float32)), 1.0, mx, skip_nonfinite=False)
        assert r["skip"] == 0 and r["coef"] == np.float32(1.0)
    assert (r["steps"], r["clipped"], r["skipped"]) == (9, 3, 1)
    # the skip flag is the LAST step's: a finite step after a skipped one clears it
    r = R.finalize(R.accumulate(rec, g), 1.0, 2.0, skip_nonfinite=True)
    assert r["skip"] == 0 and (r["steps"], r["clipped"], r["skipped"]) == (10, 4, 1)
