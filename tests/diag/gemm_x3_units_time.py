"""GPU box: the persistent unit walk of the bf16 x 3 NT GEMMs against the one-shot launch, on every NT shape of the B = 20
DtoD step (level 3, level 4 and the F(3x3,2x2) stride-2 layers), three interleaved rounds; also checks bit equality.

    python tests/diag/gemm_x3_units_time.py [reps] [auto]

`auto`: only the form the library dispatches (for a library of another revision, through GDN_HIP_LIB).
"""
import sys, pathlib
ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "gdn-pytorch_amd")]
import torch
from gdn_amd import ops
dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
auto_only = len(sys.argv) > 2 and sys.argv[2] == "auto"


def timed(fn):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


# (name, bins, M, N, K): F(4x4,3x3) levels 3 / 4; F(3x3,2x2) forms A (N = Cy, K = 4 Cx) and B (N = 4 Cx, K = Cy)
SHAPES = [("wino l3 512->512", 36, 1040, 512, 512), ("wino l4 512->512", 36, 280, 512, 512),
          ("w2 A 64->128", 16, 30800, 128, 256), ("w2 B 64->128", 16, 30800, 256, 128),
          ("w2 A 128->256", 16, 7700, 256, 512), ("w2 B 128->256", 16, 7700, 512, 256),
          ("w2 A 256->512", 16, 2160, 512, 1024), ("w2 B 256->512", 16, 2160, 1024, 512),
          ("w2 A 512->512", 16, 540, 512, 2048), ("w2 B 512->512", 16, 540, 2048, 512)]
for name, bins, M, N, K in SHAPES:
    A = torch.randn(bins, M, K, device=dev)
    Bp = ops.gemm_x3_pack(torch.randn(bins, N, K, device=dev) * 0.05)
    C = torch.empty(bins, M, N, device=dev)
    small = ((M + 127) // 128) * (N // 128) * bins < 1024
    one, units = (ops.X3_NT_ONESHOT_64, ops.X3_NT_UNITS_64) if small else (ops.X3_NT_ONESHOT_128, ops.X3_NT_UNITS_128)
    forms = [("dispatched", ops.X3_NT_AUTO), ("one-shot", one), ("units", units), ("units,bins", units | ops.X3_NT_KEEP_BINS),
             ("units,no halves", units | ops.X3_NT_NO_HALVES)]
    if auto_only:
        rounds = [timed(lambda: ops.gemm_x3_nt(A, Bp, N, out=C)) for _ in range(3)]
        print("%-18s bins %2d M %5d N %4d K %4d dispatched  %s us" % (name, bins, M, N, K, "  ".join("%7.1f" % r for r in rounds)), flush=True)
        continue
    ref = ops.gemm_x3_nt(A, Bp, N, tile_cfg=one)
    same = all(torch.equal(ops.gemm_x3_nt(A, Bp, N, tile_cfg=c), ref) for _, c in forms[1:]) and torch.equal(ops.gemm_x3_nt(A, Bp, N), ref)
    rounds = [[timed(lambda: ops.gemm_x3_nt(A, Bp, N, out=C, tile_cfg=c)) for _, c in forms] for _ in range(3)]
    print("%-18s bins %2d M %5d N %4d K %4d %s  bit-equal %s" % (name, bins, M, N, K, "nt8<64>" if small else "nt 128 ", same))
    for i, (fn, _) in enumerate(forms):
        print("    %-16s %s us" % (fn, "  ".join("%7.1f" % r[i] for r in rounds)), flush=True)
    del A, Bp, C, ref
