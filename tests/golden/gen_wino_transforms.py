#!/usr/bin/env python3
"""Recorded bits of the F(4x4,3x3) Winograd data transforms (csrc/conv_wino.hip: wino4_input_kernel, wino4_output_kernel),
for tests/test_hip_wino_transforms.py.

The transforms may be rescheduled but must keep computing the same bits, so the test compares every call below against what
the library computed when this file was last run.  Run it on the GPU box at the commit whose arithmetic is the reference (the
parent of the change under test):

    python tests/golden/gen_wino_transforms.py [OUT.npz]        (default: tests/golden/wino_transforms.npz)

Per call and output it stores the SHA-256 of the array's bytes (the check: every element, bit for bit) and a strided sample of
at most 512 values (for a useful message when the digest differs); the whole file is a few hundred KB.  The test imports the
cases, the inputs and the calls from here, so both sides run exactly the same thing.
"""
import collections
import hashlib
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
DEFAULT_OUT = HERE / "wino_transforms.npz"
SAMPLE = 512

# (B, Cin, Cout, H, W), all F(4x4,3x3) plans (<= 15 % tile padding, bf16 x 3 GEMM shapes): whole tiles; 6 tiles (the last
# transform workgroup has two dead waves inside its LDS reduce); two ragged rows; a ragged column on an odd width; the
# workload's level-4 image; channel counts that differ between the input and the output side, both ways
GEOMS = [(2, 128, 128, 8, 12), (1, 128, 128, 8, 12), (3, 128, 128, 14, 16), (2, 128, 128, 16, 27), (2, 128, 128, 8, 26),
         (2, 128, 256, 8, 12), (2, 256, 128, 8, 12)]
# x2 upsampling on load: (B, Cin, Cout, h, w) of the LOW-resolution input; the convolution runs at 2h x 2w (8x12, 14x16)
UP2X = [(2, 128, 128, 4, 6), (1, 128, 128, 7, 8)]


def gid(g):
    return "b%d_c%d_%d_%dx%d" % g


def tiles(B, H, W):
    return B * ((H + 3) // 4) * ((W + 3) // 4)


def inputs(g, up=False):
    """Seeded float32 inputs of one case (numpy).  The activations that the test passes as channel-slice views are made wider
    than the layer: `x` is xw[..., 32:32 + Cin], the residuals are the leading channels of theirs."""
    B, ci, co, H, W = g
    rng = np.random.default_rng(1000 * B + 7 * H * W + ci + 2 * co + (5 if up else 0))
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    u = lambda lo, hi, n: rng.uniform(lo, hi, n).astype(np.float32)
    d = collections.OrderedDict()
    d["xw"] = r(B, H, W, ci + 64)
    d["w"] = r(9, co, ci) / np.float32(np.sqrt(9.0 * ci))
    if up:
        return d
    d["dy"] = r(B, H, W, co)
    d["addw"] = r(B, H, W, co + 32)          # forward residual, pitch Cout + 32
    d["gaddw"] = r(B, H, W, ci + 32)         # backward residual, pitch Cin + 32
    d["by"] = r(B, H, W, ci)                 # raw output of the producer BatchNorm's convolution
    d["in_s"], d["in_t"] = u(0.5, 1.5, ci), r(ci) * np.float32(0.5)
    d["ep_s"], d["ep_t"] = u(0.5, 1.0, co), r(co) * np.float32(0.5)
    d["bco"] = np.stack([u(0.5, 1.5, ci), r(ci), r(ci) * np.float32(0.1), u(0.5, 1.5, ci)])      # scale, shift, mean, 1/std
    return d


def run(dev, g, inp=None):
    """Every call of one case through the layer entry points; returns name -> tensor (on the device)."""
    import torch
    from gdn_amd import ops
    B, ci, co, H, W = g
    t = {k: torch.from_numpy(v).to(dev) for k, v in (inp or inputs(g)).items()}
    op = ops.Conv(ci, co, 3, 1, 1)
    x, add, gadd = t["xw"][..., 32:32 + ci], t["addw"][..., :co], t["gaddw"][..., :ci]
    xc, w, dy = x.contiguous(), t["w"], t["dy"]
    nV = 36 * tiles(B, H, W) * ci
    V = lambda sv: sv[:4 * nV].view(torch.float32).clone()
    out = collections.OrderedDict()
    # forward, saved state: plain with BatchNorm partials; BatchNorm + ReLU on load from a channel slice, folded affine + ReLU
    # + residual with its own pitch; BatchNorm on load without ReLU, no epilogue, no partials
    out["f1.y"], out["f1.stats"], sv = op.wino_fwd(xc, w, stats=True, state=True)
    out["f1.V"] = V(sv)
    out["f2.y"], sv2 = op.wino_fwd(x, w, addsrc=add, state=True, affine=(t["ep_s"], t["ep_t"]), act=ops.ACT_RELU,
                                   in_affine=(t["in_s"], t["in_t"]), in_relu=True)
    out["f2.V"] = V(sv2)
    out["f3.y"], sv3 = op.wino_fwd(x, w, state=True, in_affine=(t["in_s"], t["in_t"]))
    out["f3.V"] = V(sv3)
    # backward: both gradients (gdn_winoconv_bwd_pair) with residual and BatchNorm-backward partials behind a ReLU; the data
    # gradient alone with partials, no ReLU; the data gradient alone without saved state; the weight gradient alone
    slots = op.wino_bnb_slots(B, H, W)
    out["b1.dw"], out["b1.part"] = torch.zeros_like(w), torch.zeros(slots, 2, ci, device=dev)
    out["b1.dx"] = op.wino_bwd(dy, w, (H, W), state=sv, dw_tap=out["b1.dw"], addsrc=gadd, bnb=(t["by"], t["bco"], True, out["b1.part"]))
    out["b2.part"] = torch.zeros(slots, 2, ci, device=dev)
    out["b2.dx"] = op.wino_bwd(dy, w, (H, W), state=sv, bnb=(t["by"], t["bco"], False, out["b2.part"]))
    out["b3.dx"] = op.wino_bwd(dy, w, (H, W))
    out["b4.dw"] = torch.zeros_like(w)
    op.wino_bwd(dy, w, (H, W), state=sv, dw_tap=out["b4.dw"], need_dx=False)
    torch.cuda.synchronize()
    return out


def run_up2x(dev, g, inp=None):
    """Forward on a low-resolution channel-slice input, both interpolation modes (1: align_corners = False, 2: True)."""
    import torch
    from gdn_amd import ops
    B, ci, co, h, w_ = g
    t = {k: torch.from_numpy(v).to(dev) for k, v in (inp or inputs(g, up=True)).items()}
    op = ops.Conv(ci, co, 3, 1, 1)
    x = t["xw"][..., 32:32 + ci]
    nV = 36 * tiles(B, 2 * h, 2 * w_) * ci
    out = collections.OrderedDict()
    for mode in (1, 2):
        out["u%d.y" % mode], sv = op.wino_fwd(x, t["w"], state=True, up2x=mode)
        out["u%d.V" % mode] = sv[:4 * nV].view(torch.float32).clone()
    torch.cuda.synchronize()
    return out


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)


def sample(a):
    f = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    return f[::max(1, f.size // SAMPLE)][:SAMPLE].copy()


def main():
    import torch
    sys.path.insert(0, str(HERE.parent.parent / "gdn-pytorch_amd"))
    dev = torch.device("cuda:0")
    rec = {}
    for cases, fn, tag in ((GEOMS, run, ""), (UP2X, run_up2x, "up2x_")):
        for g in cases:
            for name, v in fn(dev, g).items():
                a = v.detach().cpu().numpy()
                assert np.isfinite(a).all() and np.abs(a).max() > 0, (g, name)
                rec["%s%s/%s/sha" % (tag, gid(g), name)] = digest(a)
                rec["%s%s/%s/sample" % (tag, gid(g), name)] = sample(a)
    out = pathlib.Path(sys.argv[1]) if len(sys.argv) > 1 else DEFAULT_OUT
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez(out, **rec)
    print("wrote %s: %d arrays, %d bytes" % (out, len(rec), out.stat().st_size))


if __name__ == "__main__":
    main()
