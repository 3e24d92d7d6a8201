#!/usr/bin/env python3
"""GPU box: one F(4x4,3x3) layer's backward (both gradients) at B=20, 512 -> 512, levels 3 (16x52) and 4 (8x26):
gdn_winoconv_bwd on one stream  |  gdn_winoconv_bwd_pair, phases = 0, on one stream  |  the forked form of ops.Conv.wino_bwd
(weight-gradient chain on the side stream).  Interleaved rounds, best of three per form; also checks the three forms agree
bit for bit.   usage: wino_bwd_pair_time.py [reps]"""
import pathlib, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "gdn-pytorch_amd"))
import torch
from gdn_amd import ops
from gdn_amd._lib import lib
dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50


def timeit(fn):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per call


for level, (H, W) in ((3, (16, 52)), (4, (8, 26))):
    B, C = 20, 512
    op = ops.Conv(C, C, 3, 1, 1)
    x = torch.randn(B, H, W, C, device=dev)
    w = torch.randn(9, C, C, device=dev) * 0.02
    gy = torch.randn(B, H, W, C, device=dev)
    add = torch.randn(B, H, W, C, device=dev)
    _, sv = op.wino_fwd(x, w, state=True)
    _, ref, _, _ = op.geom(B, H, W)
    nb, npair = int(lib.gdn_winoconv_bwd_workspace_bytes(ref)), int(lib.gdn_winoconv_bwd_pair_workspace_bytes(ref))
    ws = torch.empty(max(nb, npair, 256), dtype=torch.uint8, device=dev)
    dx = [torch.empty_like(x) for _ in range(3)]
    dw = [torch.empty_like(w) for _ in range(3)]
    p, ld = ops._p, ops._ld

    def single():
        lib.gdn_winoconv_bwd(ref, p(gy), ld(gy), p(w), p(sv), p(dx[0]), ld(dx[0]), p(add), ld(add), p(dw[0]), None, 0, None, 0,
                             None, 0, p(ws), nb, ops.stream())

    def pair0():
        lib.gdn_winoconv_bwd_pair(ref, p(gy), ld(gy), p(w), p(sv), p(dx[1]), ld(dx[1]), p(add), ld(add), p(dw[1]), None, 0, None,
                                  0, None, 0, 0, p(ws), npair, ops.stream())

    def forked():
        dx[2] = op.wino_bwd(gy, w, (H, W), state=sv, dw_tap=dw[2], addsrc=add)

    forms = [("gdn_winoconv_bwd", single)]
    if npair:
        forms += [("pair, one stream", pair0), ("pair, forked", forked)]
    best = {n: float("inf") for n, _ in forms}
    for _ in range(3):
        for n, fn in forms:
            best[n] = min(best[n], timeit(fn))
    torch.cuda.synchronize()
    same = all(torch.equal(dx[i], dx[0]) and torch.equal(dw[i], dw[0]) for i in range(1, len(forms)))
    print("level %d  %dx%d  pair workspace %.1f MB (single %.1f MB)  " % (level, H, W, npair / 1e6, nb / 1e6)
          + "  ".join("%s %.1f us" % (n, best[n]) for n, _ in forms) + "  bitwise equal: %s" % same, flush=True)
