"""The persistent unit walk of the bf16 x 3 NT GEMMs (csrc/gemm_x3.hip) against the one-shot launch of the same kernel.

Only which workgroup computes which output block, and when its loads and stores are issued, differs between the two forms:
every output element sees the same MFMA sequence, so the yardstick is BIT equality -- on random operands (where any other
summation order would show) and, in the style of test_hip_gemm_x3.py, exactness on small integers (where a wrong row, bin or
plane shows whatever the order).  Forced grids of 8 and 16 workgroups make tiny problems walk several rounds, with the last
round halved or not and a tail unit directly behind a full one."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MS = (1, 31, 33, 64, 65, 129, 200, 280)          # a tail inside the first row block, on a block edge, level 4's M
NS = (128, 256)
KS = (32, 96)                                    # a single stage, an odd stage count
SENTINEL = -12345.0
GUARD = 128 * 256                                # floats before and behind C: a whole padded row tile at the widest N

_cache = {}


def _operands(gpu, bins, M, N, K):
    """Random and small-integer operands of one shape, made once and shared (never written to)."""
    key = (bins, M, N, K)
    if key not in _cache:
        from gdn_amd import ops
        g = torch.Generator(device=gpu).manual_seed(bins * 100003 + M * 1009 + N * 7 + K)
        A = torch.randn(bins, M, K, device=gpu, generator=g)
        B = torch.randn(bins, N, K, device=gpu, generator=g) * torch.logspace(-2, 2, N, device=gpu).view(1, N, 1)
        Ai = torch.randint(-8, 9, (bins, M, K), device=gpu, generator=g).float()
        Bi = torch.randint(-8, 9, (bins, N, K), device=gpu, generator=g).float() + torch.arange(N, device=gpu).view(1, N, 1).float()
        ref_i = torch.bmm(Ai.double(), Bi.double().transpose(1, 2)).float()        # exact: |sum| < 2^24
        _cache[key] = (A, ops.gemm_x3_pack(B), Ai, ops.gemm_x3_pack(Bi), ref_i, {})
    return _cache[key]


def _oneshot(gpu, bins, M, N, K, oneshot):
    from gdn_amd import ops
    A, Bp, _, _, _, refs = _operands(gpu, bins, M, N, K)
    if oneshot not in refs:
        refs[oneshot] = ops.gemm_x3_nt(A, Bp, N, tile_cfg=oneshot)
    return refs[oneshot]


def _guarded(gpu, bins, M, N):
    buf = torch.full((2 * GUARD + bins * M * N,), SENTINEL, device=gpu)
    return buf, buf[GUARD:GUARD + bins * M * N].view(bins, M, N)


def _forms():
    from gdn_amd import ops
    return {"k128": (ops.X3_NT_ONESHOT_128, ops.X3_NT_UNITS_128), "k64": (ops.X3_NT_ONESHOT_64, ops.X3_NT_UNITS_64)}


def _flags():
    from gdn_amd import ops
    return {"pairs+halves": 0, "bins+halves": ops.X3_NT_KEEP_BINS, "pairs": ops.X3_NT_NO_HALVES}


@pytest.mark.parametrize("flags", ["pairs+halves", "bins+halves", "pairs"])
@pytest.mark.parametrize("grid", [8, 16])
@pytest.mark.parametrize("bins", [1, 5, 9])
@pytest.mark.parametrize("kern", ["k128", "k64"])
def test_units_bitwise_equal_oneshot(gpu, kern, bins, grid, flags):
    """Every (M, N, K) of the issue's list on a forced grid: the persistent launch equals the one-shot launch bit for bit on
    random operands, equals the integer result exactly on small integers, and leaves everything outside C (the rows a padded
    tile would have) untouched."""
    from gdn_amd import ops
    oneshot, units = _forms()[kern]
    cfg = units | _flags()[flags]
    bad = []
    for M in MS:
        for N in NS:
            for K in KS:
                A, Bp, Ai, Bpi, ref_i, _ = _operands(gpu, bins, M, N, K)
                ref = _oneshot(gpu, bins, M, N, K, oneshot)
                buf, C = _guarded(gpu, bins, M, N)
                ops.gemm_x3_nt(A, Bp, N, out=C, tile_cfg=cfg, grid=grid)
                same = torch.equal(C, ref)
                clean = bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
                buf_i, Ci = _guarded(gpu, bins, M, N)
                ops.gemm_x3_nt(Ai, Bpi, N, out=Ci, tile_cfg=cfg, grid=grid)
                exact = torch.equal(Ci, ref_i)
                clean_i = bool((buf_i[:GUARD] == SENTINEL).all()) and bool((buf_i[-GUARD:] == SENTINEL).all())
                if not (same and clean and exact and clean_i):
                    bad.append((M, N, K, "bitwise" if not same else "", "integers" if not exact else "",
                                "padding" if not (clean and clean_i) else "", int((C != ref).sum()), int((Ci != ref_i).sum())))
    assert not bad, "%s bins %d grid %d %s: %s" % (kern, bins, grid, flags, bad)


@pytest.mark.parametrize("kern", ["k128", "k64"])
def test_oneshot_exact_on_integers(gpu, kern):
    """The yardstick of the test above is itself exact: the one-shot launches (which now skip the row blocks beyond M) on the
    tail shapes."""
    from gdn_amd import ops
    oneshot, _ = _forms()[kern]
    for M in MS:
        _, _, Ai, Bpi, ref_i, _ = _operands(gpu, 5, M, 256, 96)
        buf, C = _guarded(gpu, 5, M, 256)
        ops.gemm_x3_nt(Ai, Bpi, 256, out=C, tile_cfg=oneshot)
        assert torch.equal(C, ref_i), "M %d" % M
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), "M %d: padding written" % M


@pytest.mark.parametrize("M", [1040, 280])
def test_units_default_launch_at_step_shapes(gpu, M):
    """What the Winograd layers run (default form, default grid) on the level-3 and level-4 GEMMs of the B = 20 step, 36 bins x
    [M x 512] x [512 x 512]: bit-equal to both one-shot kernels' launch of the form it replaces, and to every walk variant."""
    from gdn_amd import ops
    g = torch.Generator(device=gpu).manual_seed(M)
    A = torch.randn(36, M, 512, device=gpu, generator=g)
    Bp = ops.gemm_x3_pack(torch.randn(36, 512, 512, device=gpu, generator=g) * 0.02)
    oneshot, units = _forms()["k128" if M == 1040 else "k64"]
    ref = ops.gemm_x3_nt(A, Bp, 512, tile_cfg=oneshot)
    buf, C = _guarded(gpu, 36, M, 512)
    ops.gemm_x3_nt(A, Bp, 512, out=C)
    assert torch.equal(C, ref)
    assert torch.equal(ops.gemm_x3_nt(A, Bp, 512, tile_cfg=ops.X3_NT_SHARED), ref)      # the forked backward's launch
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
    for flags in _flags().values():
        assert torch.equal(ops.gemm_x3_nt(A, Bp, 512, tile_cfg=units | flags), ref), "flags %#x" % flags


def test_units_rejects_bad_selector(gpu):
    from gdn_amd import GdnError, ops
    A = torch.zeros(1, 64, 64, device=gpu)
    Bp = ops.gemm_x3_pack(torch.zeros(1, 128, 64, device=gpu))
    for cfg, grid in ((ops.X3_NT_UNITS_128, 12), (ops.X3_NT_UNITS_128, -8), (5, 8), (0x800, 8), (ops.X3_NT_UNITS_64 | ops.X3_NT_SHARED, 8)):
        with pytest.raises(GdnError):
            ops.gemm_x3_nt(A, Bp, 128, tile_cfg=cfg, grid=grid)
