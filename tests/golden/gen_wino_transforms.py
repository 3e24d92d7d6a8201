#!/usr/bin/env python3
"""Recorded bits of the 3x3 Winograd layer (csrc/conv_wino.hip) for tests/test_hip_wino_transforms.py: the F(4x4,3x3) data
transforms (wino4_input_kernel, wino4_output_kernel; GEOMS, UP2X) and every other plan the host side chooses between --
F(2x2,3x3) with fp32 or bf16 x 3 GEMMs per direction, the plan hints, reflection padding with its fold, flipped taps (PLANS,
UP2X_REFLECT).

The kernels may be rescheduled and the host code rearranged but must keep computing the same bits, so the test compares every call below against what
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


# The other plans of the layer and the selectors between them, recorded when the host side of conv_wino.hip was rebuilt around one
# launcher per stage.  (id, (B, Cin, Cout, H, W), plan): plan = the layer's keyword arguments (reflect, flip_taps), the switches
# the case runs under (x3, f4: ops.set_x3 / set_wino_f4, default on) and T, the outputs per tile side the library must choose
# (2: F(2x2,3x3), 16 bins; 4: F(4x4,3x3), 36 bins).
PLANS = [
    ("f2_mfma", (2, 64, 64, 5, 6), dict(T=2)),                        # 64 channels: every GEMM on the fp32 MFMA
    ("f2_fwd_panels", (2, 64, 128, 5, 7), dict(T=2)),                 # forward set as bf16 x 3 panels, data-gradient set fp32
    ("f2_dgrad_panels", (2, 128, 64, 5, 7), dict(T=2)),               # ... and the reverse
    ("f2_x3", (2, 128, 128, 5, 6), dict(T=2)),                        # every GEMM bf16 x 3, the TN one too (4x4 tiles would pad 113 %)
    ("f2_no_x3", (2, 128, 128, 5, 6), dict(T=2, x3=False)),
    ("f2_no_f4", (2, 128, 128, 8, 12), dict(T=2, f4=False)),          # F(4x4,3x3)-eligible, held back by GDN_HINT_NO_WINO_F4
    ("reflect", (2, 128, 64, 9, 13), dict(T=2, reflect=True)),
    ("reflect_retiled", (2, 128, 128, 6, 5), dict(T=2, reflect=True)),      # padded domain 8x7: 4x4 tiles against the forward's 3x3
    ("f2_flip", (2, 64, 64, 5, 6), dict(T=2, flip_taps=True)),
    ("f4_flip", (2, 128, 128, 8, 12), dict(T=4, flip_taps=True)),
]
# reflection padding with x2 upsampling on load, and the fold with the upsampling's adjoint behind its data gradient
UP2X_REFLECT = [("reflect_up2x", (2, 128, 128, 3, 4), dict(T=2, reflect=True))]


def gid(g):
    return "b%d_c%d_%d_%dx%d" % g


def tiles(B, H, W, T=4):
    return B * ((H + T - 1) // T) * ((W + T - 1) // T)


def layer(g, plan):
    """The layer of one case: (ops.Conv, bins * tiles * Cin = the elements of its saved input transform at the size the
    convolution runs at)."""
    from gdn_amd import ops
    B, ci, co, H, W = g
    T = plan.get("T", 4)
    op = ops.Conv(ci, co, 3, 1, 1, reflect=plan.get("reflect", False), flip_taps=plan.get("flip_taps", False))
    return op, (T + 2) ** 2 * tiles(B, H, W, T) * ci


class switches:
    """The bf16 x 3 and F(4x4,3x3) switches of ops.py as the plan wants them, put back on exit."""

    def __init__(self, plan):
        self.want = (plan.get("x3", True), plan.get("f4", True))

    def __enter__(self):
        from gdn_amd import ops
        self.prev = (ops.set_x3(self.want[0]), ops.set_wino_f4(self.want[1]))

    def __exit__(self, *exc):
        from gdn_amd import ops
        ops.set_x3(self.prev[0]); ops.set_wino_f4(self.prev[1])


def inputs(g, up=False, up_bwd=False):
    """Seeded float32 inputs of one case (numpy).  The activations that the test passes as channel-slice views are made wider
    than the layer: `x` is xw[..., 32:32 + Cin], the residuals are the leading channels of theirs.  up_bwd: an up2x case that
    also runs backward (dy at the upsampled size, drawn after the forward's inputs)."""
    B, ci, co, H, W = g
    rng = np.random.default_rng(1000 * B + 7 * H * W + ci + 2 * co + (5 if up else 0))
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    u = lambda lo, hi, n: rng.uniform(lo, hi, n).astype(np.float32)
    d = collections.OrderedDict()
    d["xw"] = r(B, H, W, ci + 64)
    d["w"] = r(9, co, ci) / np.float32(np.sqrt(9.0 * ci))
    if up:
        if up_bwd:
            d["dy"] = r(B, 2 * H, 2 * W, co)
        return d
    d["dy"] = r(B, H, W, co)
    d["addw"] = r(B, H, W, co + 32)          # forward residual, pitch Cout + 32
    d["gaddw"] = r(B, H, W, ci + 32)         # backward residual, pitch Cin + 32
    d["by"] = r(B, H, W, ci)                 # raw output of the producer BatchNorm's convolution
    d["in_s"], d["in_t"] = u(0.5, 1.5, ci), r(ci) * np.float32(0.5)
    d["ep_s"], d["ep_t"] = u(0.5, 1.0, co), r(co) * np.float32(0.5)
    d["bco"] = np.stack([u(0.5, 1.5, ci), r(ci), r(ci) * np.float32(0.1), u(0.5, 1.5, ci)])      # scale, shift, mean, 1/std
    return d


def run(dev, g, inp=None, plan=None):
    """Every call of one case through the layer entry points; returns name -> tensor (on the device).  plan: as in PLANS
    (default: the F(4x4,3x3) plan of a zero-padded layer under the default switches)."""
    with switches(plan or {}):
        return _run(dev, g, inp, plan or {})


def _run(dev, g, inp, plan):
    import torch
    from gdn_amd import ops
    B, ci, co, H, W = g
    t = {k: torch.from_numpy(v).to(dev) for k, v in (inp or inputs(g)).items()}
    op, nV = layer(g, plan)
    x, add, gadd = t["xw"][..., 32:32 + ci], t["addw"][..., :co], t["gaddw"][..., :ci]
    xc, w, dy = x.contiguous(), t["w"], t["dy"]
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
    # (a reflection layer's data gradient emits no BatchNorm-backward partials -- gdn_winoconv_bnb_slots is 0: the same calls without)
    slots = op.wino_bnb_slots(B, H, W)
    bnb = lambda relu, name: dict(bnb=(t["by"], t["bco"], relu, out.setdefault(name, torch.zeros(slots, 2, ci, device=dev)))) if slots else {}
    out["b1.dw"] = torch.zeros_like(w)
    out["b1.dx"] = op.wino_bwd(dy, w, (H, W), state=sv, dw_tap=out["b1.dw"], addsrc=gadd, **bnb(True, "b1.part"))
    out["b2.dx"] = op.wino_bwd(dy, w, (H, W), state=sv, **bnb(False, "b2.part"))
    out["b3.dx"] = op.wino_bwd(dy, w, (H, W))
    out["b4.dw"] = torch.zeros_like(w)
    op.wino_bwd(dy, w, (H, W), state=sv, dw_tap=out["b4.dw"], need_dx=False)
    torch.cuda.synchronize()
    return out


def run_up2x(dev, g, inp=None, plan=None):
    """Forward on a low-resolution channel-slice input, both interpolation modes (1: align_corners = False, 2: True); with
    `dy` among the inputs also the backward of each: both gradients, dx being the low-resolution tensor's."""
    import torch
    plan = plan or {}
    B, ci, co, h, w_ = g
    t = {k: torch.from_numpy(v).to(dev) for k, v in (inp or inputs(g, up=True)).items()}
    out = collections.OrderedDict()
    with switches(plan):
        op, nV = layer((B, ci, co, 2 * h, 2 * w_), plan)
        x = t["xw"][..., 32:32 + ci]
        for mode in (1, 2):
            out["u%d.y" % mode], sv = op.wino_fwd(x, t["w"], state=True, up2x=mode)
            out["u%d.V" % mode] = sv[:4 * nV].view(torch.float32).clone()
            if "dy" in t:
                out["u%d.dw" % mode] = torch.zeros_like(t["w"])
                out["u%d.dx" % mode] = op.wino_bwd(t["dy"], t["w"], (2 * h, 2 * w_), state=sv, dw_tap=out["u%d.dw" % mode], up2x=mode)
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
    runs = [("", g, run(dev, g)) for g in GEOMS] + [("up2x_", g, run_up2x(dev, g)) for g in UP2X]
    runs += [(pid + "_", g, run(dev, g, plan=plan)) for pid, g, plan in PLANS]
    runs += [(pid + "_", g, run_up2x(dev, g, inputs(g, up=True, up_bwd=True), plan)) for pid, g, plan in UP2X_REFLECT]
    for tag, g, outs in runs:
        for name, v in outs.items():
            a = v.detach().cpu().numpy()
            assert np.isfinite(a).all() and np.abs(a).max() > 0, (tag, g, name)
            rec["%s%s/%s/sha" % (tag, gid(g), name)] = digest(a)
            rec["%s%s/%s/sample" % (tag, gid(g), name)] = sample(a)
    out = pathlib.Path(sys.argv[1]) if len(sys.argv) > 1 else DEFAULT_OUT
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez(out, **rec)
    print("wrote %s: %d arrays, %d bytes" % (out, len(rec), out.stat().st_size))


if __name__ == "__main__":
    main()
