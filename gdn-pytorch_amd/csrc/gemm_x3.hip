// fp32 per-bin GEMMs as bf16 x 3 split products on v_mfma_f32_32x32x16_bf16 (see gemm_x3.h for the arithmetic and the layout).
#include "gemm_x3.h"


namespace {

// ---- packing: fp32 [bins][rows][K] -> panels.  thread = (row, 8 consecutive k): two 16-byte loads, three 16-byte stores ----
__global__ __launch_bounds__(256) void x3_pack_rows_kernel(const float* __restrict__ src, unsigned char* __restrict__ dst, int rows,
                                                           int K, int rows_pad) {
    const int KB = K / X3_BK, k8n = K / 8;
    const int bin = blockIdx.y;
    const size_t per_bin = x3_packed_bytes(rows, K);
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < (int64_t)rows_pad * k8n; i += (int64_t)gridDim.x * 256) {
        // a wave = 16 consecutive rows x the 4 chunks of one k block: 1 KB contiguous per plane in the packed layout
        const int row = (int)((i >> 2) % rows_pad), k8 = (int)(i & 3) + 4 * (int)((i >> 2) / rows_pad);
        f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
        if (row < rows) {
            const float* s = src + ((size_t)bin * rows + row) * K + k8 * 8;
            lo = *reinterpret_cast<const f32x4*>(s);
            hi = *reinterpret_cast<const f32x4*>(s + 4);
        }
        unsigned h[3][4];
        x3_split2(lo[0], lo[1], h[0][0], h[1][0], h[2][0]);
        x3_split2(lo[2], lo[3], h[0][1], h[1][1], h[2][1]);
        x3_split2(hi[0], hi[1], h[0][2], h[1][2], h[2][2]);
        x3_split2(hi[2], hi[3], h[0][3], h[1][3], h[2][3]);
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const uint4 v = {h[p][0], h[p][1], h[p][2], h[p][3]};
            *reinterpret_cast<uint4*>(dst + (size_t)bin * per_bin + x3_off(row, k8 * 8, p, KB)) = v;
        }
    }
}

// One 32-deep stage of a wave's 64 x 64 tile from the LDS images As / Bs ([plane][128 rows][64 B], chunk-swizzled): two
// sub-steps of 6 + 6 fragment reads and 24 MFMAs.  DYN: `ni` (wave-uniform, 1 or 2) row blocks are multiplied -- the second one
// may lie beyond the last row, or the unit is a half-height one; a row block's MFMA sequence is the same either way.  (One
// body with a scalar branch around the second block: two instantiations side by side spill the accumulators.)
template <bool DYN = false>
__device__ __forceinline__ void x3_stage_mfma(const unsigned char* As, const unsigned char* Bs, int a_base, int b_base, int h, int f_sw,
                                              f32x16 (&acc)[2][2], f32x16 (&cor)[2][2], int ni = 2) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int co = ((2 * s + h) ^ f_sw) * 16;
        x3_bf16x8 af[2][3], bf[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                af[i][p] = __builtin_bit_cast(x3_bf16x8, *reinterpret_cast<const uint4*>(&As[p * 8192 + a_base + i * 2048 + co]));
                bf[i][p] = __builtin_bit_cast(x3_bf16x8, *reinterpret_cast<const uint4*>(&Bs[p * 8192 + b_base + i * 2048 + co]));
            }
        // The bf16 MFMA aligns its 16 products AND the C input to the largest exponent among them and truncates what
        // falls below ~half an ulp of it, per addend, toward zero (measured: tests/diag/mfma_rounding.py); the sum itself is
        // rounded to nearest.  A leading product a1*b1 has a 16-bit significand, so against a running sum sqrt(K) larger
        // it loses nothing; a correction product sits 8 or 16 bits lower and WOULD be cut at the running sum's ulp.  Hence
        // two accumulators: `acc` chains the leading products, `cor` chains the five correction products (its own ulp is
        // 2^-8 of acc's), and the two meet once, in the epilogue.  No vector-ALU work in the loop; 32 roundings per
        // K = 512 instead of the 512 of the k-ordered fp32 MFMA chain this replaces.
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (DYN && i >= ni) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                cor[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][2], bf[j][0], cor[i][j], 0, 0, 0);
                cor[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], bf[j][1], cor[i][j], 0, 0, 0);
                cor[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[j][2], cor[i][j], 0, 0, 0);
                cor[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], bf[j][0], cor[i][j], 0, 0, 0);
                cor[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[j][1], cor[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[j][0], acc[i][j], 0, 0, 0);
            }
        }
    }
}

// ---- the unit walk of the NT kernels ----
// A unit is one output block (bin, M tile, N tile).  One-shot launch (UNITS = false): a workgroup per unit, XCD j owns bins
// j, j + 8, ...  Persistent launch (UNITS = true): a grid of G = 8 G8 workgroups, workgroup w on XCD w & 7 in slot w >> 3.  An
// XCD's units are numbered (pair, N tile) with the N tiles of one (bin, M tile) pair back to back, and slot s takes units
// s, s + G8, ...: a static list -- no counter, nothing to reset, capturable.  X3_UNITS_PAIRS deals the bins * MT pairs to the
// XCDs in contiguous ranges (every XCD within one pair of an eighth of the work, and still on ~bins / 8 + 1 weight panels);
// without it an XCD keeps whole bins as in the one-shot launch.  X3_UNITS_HALVE: a last round that would fill at most half of
// the slots is cut along M into half-height units dealt to twice as many slots.  Everything here is wave-uniform (blockIdx,
// gridDim and kernel arguments only), so it lives in scalar registers.
struct X3Walk { int xcd, slot, G8, NT, MT, p0, pairs, full, halved, n; };
struct X3Unit { int bin, m0, nt, hm; };          // hm: half-height unit (rows m0 .. m0 + TM / 2)

template <bool UNITS, int TM>
__device__ __forceinline__ X3Unit x3_unit(const X3Walk& w, int i) {
    X3Unit u;
    int ul = i * w.G8 + w.slot, half = 0;
    u.hm = 0;
    if (UNITS && i >= w.full && w.halved) {
        ul = w.full * w.G8 + (w.slot >> 1);
        half = w.slot & 1;
        u.hm = 1;
    }
    const int pl = ul / w.NT, pg = w.p0 + pl, b = pg / w.MT;
    u.nt = ul - pl * w.NT;
    u.bin = w.pairs ? b : b * 8 + w.xcd;
    u.m0 = (pg - b * w.MT) * TM + half * (TM / 2);
    return u;
}

template <bool UNITS, int TM>
__device__ __forceinline__ X3Walk x3_walk(int M, int N, int bins, int mode) {
    X3Walk w;
    w.xcd = blockIdx.x & 7;
    w.slot = blockIdx.x >> 3;
    w.G8 = UNITS ? (int)(gridDim.x >> 3) : 0;
    w.NT = N / 128;
    w.MT = (M + TM - 1) / TM;
    w.pairs = UNITS && (mode & X3_UNITS_PAIRS);
    w.p0 = 0;
    w.full = 1;
    w.halved = 0;
    if (!UNITS) {
        w.n = (w.slot / (w.NT * w.MT)) * 8 + w.xcd < bins ? 1 : 0;
        return w;
    }
    const int P = bins * w.MT;
    int np = w.xcd < bins ? ((bins - 1 - w.xcd) / 8 + 1) * w.MT : 0;
    if (w.pairs) {
        w.p0 = P * w.xcd / 8;
        np = P * (w.xcd + 1) / 8 - w.p0;
    }
    const int U = np * w.NT;
    w.full = U / w.G8;
    const int R = U - w.full * w.G8;
    w.halved = (mode & X3_UNITS_HALVE) && R > 0 && 2 * R <= w.G8;
    w.n = w.full + (w.slot < (w.halved ? 2 * R : R) ? 1 : 0);
    // the upper half of a tail tile may hold no row at all: no unit
    if (w.halved && w.n > w.full && x3_unit<UNITS, TM>(w, w.full).m0 >= M) --w.n;
    return w;
}

// ---- the GEMM ----
// Workgroup = 128 x 128 output tile, 4 waves (2 x 2) of 64 x 64 = 2 x 2 MFMA tiles; a stage is 32 k: per wave 2 sub-steps of
// (6 + 6 fragment reads, 24 MFMAs).  LDS: three bf16 planes of A and of B, [plane][128 rows][64 B] each (48 KB); two
// workgroups per CU (232 registers: two accumulator sets).  A is staged global (fp32) -> registers -> split -> LDS with the loads of stage i + 1 issued
// before the MFMAs of stage i; B's stage is a linear 24 KB copy of its panel.
// XCD-aware order (as wino_gemm_kernel): XCD j owns bins j, j + 8, ... and walks them with the N tiles of one M tile back to
// back, so an A tile is fetched from the fabric once and a bin's weight panels stay in that XCD's L2.
// UNITS: the persistent form (x3_walk above).  The unit loop is the k loop continued: the first slab of the next unit is
// requested where a further stage of this one would be, its LDS write follows the barrier that ends this unit's last stage,
// and only THEN are this unit's results stored -- the wait for those loads never stands behind a store in the in-order
// memory counter, and the stores drain under the next unit's first MFMAs.  A wave skips the fragment reads and MFMAs of a
// 32-row block that lies at or beyond M (one-shot form too); a half-height unit gives every wave one row block instead of two.
// Every output element sees the MFMA sequence of the one-shot launch: results are bit-identical.
template <bool UNITS>
__global__ __launch_bounds__(256, 2) void gemm_x3_nt_kernel(const float* __restrict__ A, const unsigned char* __restrict__ Bp,
                                                            float* __restrict__ C, int M, int N, int K, int bins, int mode) {
    __shared__ __attribute__((aligned(16))) unsigned char As[3 * 128 * 64], Bs[3 * 128 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
    const int KB = K / X3_BK;
    const X3Walk w = x3_walk<UNITS, 128>(M, N, bins, mode);
    if (w.n == 0) return;

    f32x16 acc[2][2], cor[2][2];

    // A staging: 8 lanes fetch one row's 32 k = a full 128-byte line (lane = 4 k), a wave instruction 8 rows; a thread holds
    // rows rb, rb + 32, rb + 64, rb + 96.  (Fetching 16 k per thread -- 16-byte pieces of 32 different lines per instruction --
    // measured 1.2x slower: the texture path, not the matrix pipe, set the pace.)  Rows past M read row M - 1.  A half-height
    // unit stages all 128 rows from its first and multiplies 64: loads under a branch make the compiler wait for them at once.
    // ap / Bb are the staging cursor: aimed at the next unit while this one is still multiplied.
    const int k4 = tid & 7, rb0 = tid >> 3;
    const float* ap[4];
    const unsigned char* Bb;
    auto aim = [&](const X3Unit& u) {
        const float* Ab = A + (size_t)u.bin * M * K;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int row = v * 32 + rb0;
            ap[v] = Ab + (size_t)(u.m0 + row < M ? u.m0 + row : M - 1) * K + k4 * 4;
        }
        Bb = Bp + (size_t)u.bin * x3_packed_bytes(N, K) + (size_t)u.nt * KB * (3 * 128 * 64);
    };
    f32x4 ra[4];
    f32x4 rb[6];
    auto gload = [&](int kb) {
#pragma unroll
        for (int v = 0; v < 4; ++v) ra[v] = *reinterpret_cast<const f32x4*>(ap[v] + (size_t)kb * X3_BK);
        const unsigned char* bsrc = Bb + (size_t)kb * (3 * 128 * 64) + tid * 16;
#pragma unroll
        for (int v = 0; v < 6; ++v) rb[v] = *reinterpret_cast<const f32x4*>(bsrc + v * 4096);
    };
    auto lstore = [&]() {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int row = v * 32 + rb0;
            unsigned h0[3], h1[3];
            x3_split2(ra[v][0], ra[v][1], h0[0], h0[1], h0[2]);
            x3_split2(ra[v][2], ra[v][3], h1[0], h1[1], h1[2]);
            const int off = row * 64 + (((k4 >> 1) ^ x3_sw(row)) * 16) + (k4 & 1) * 8;
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const uint2 w = {h0[p], h1[p]};
                *reinterpret_cast<uint2*>(&As[p * 8192 + off]) = w;
            }
        }
#pragma unroll
        for (int v = 0; v < 6; ++v) *reinterpret_cast<f32x4*>(&Bs[v * 4096 + tid * 16]) = rb[v];
    };
    // fragment addresses: lane (r = lane & 31, h = lane >> 5) reads 16 B of row (tile row base + r) at chunk (2 s + h) ^ swz(row)
    const int r32 = lane & 31, h = lane >> 5;
    const int f_sw = x3_sw(r32);                                       // tile row bases are multiples of 32: same swizzle
    const int b_base = (wn * 64 + r32) * 64;
    // a wave's rows inside a unit: wrow .. wrow + 32 nb, nb = its row blocks that hold a row below M (wave-uniform)
    auto wave_rows = [&](const X3Unit& u, int& wrow, int& nb) {
        wrow = u.hm ? wm * 32 : wm * 64;
        const int left = (M - u.m0 - wrow + 31) >> 5, most = u.hm ? 1 : 2;
        nb = left < 0 ? 0 : left < most ? left : most;
    };
    auto store = [&](const X3Unit& u, int wrow, int nb) {
        float* Cb = C + (size_t)u.bin * M * N;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (i >= nb) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = u.nt * 128 + wn * 64 + j * 32 + r32;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = u.m0 + wrow + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (m < M) Cb[(size_t)m * N + col] = acc[i][j][r] + cor[i][j][r];
                }
            }
        }
    };

    X3Unit cu = x3_unit<UNITS, 128>(w, 0), pu = cu;
    int wrow, nb, pwrow = 0, pnb = 0;
    aim(cu);
    gload(0);
    for (int u = 0;; ++u) {
        const bool more = UNITS && u + 1 < w.n;
        wave_rows(cu, wrow, nb);
        const int a_base = (wrow + r32) * 64;
        lstore();
        __syncthreads();
        if (UNITS && u > 0) store(pu, pwrow, pnb);                      // the previous unit's results, behind this unit's first slab
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; cor[i][j][r] = 0.f; }
        for (int kb = 0; kb < KB; ++kb) {
            if (kb > 0) {
                lstore();
                __syncthreads();
            }
            if (kb + 1 < KB) gload(kb + 1);
            else if (more) {
                aim(x3_unit<UNITS, 128>(w, u + 1));
                gload(0);
            }
            if (nb) x3_stage_mfma<true>(As, Bs, a_base, b_base, h, f_sw, acc, cor, nb);
            __syncthreads();
        }
        if (!more) break;
        pu = cu; pwrow = wrow; pnb = nb;
        cu = x3_unit<UNITS, 128>(w, u + 1);
    }
    store(cu, wrow, nb);
}

// ---- NT kernel, second structure: 512 threads, double-buffered LDS, ONE barrier per stage ----
// 8 waves (2 x 4): wave tile (TM/2) x 32 = MI x 1 MFMA tiles (TM = 128: MI = 2; TM = 64 for GEMMs with few rows: MI = 1).  Both
// operands' stage k + 1 is written to the other LDS buffer while stage k is multiplied, so the split arithmetic and the LDS
// writes of one wave run under the MFMAs of the wave it shares a SIMD with, and a stage costs one barrier:
//     iteration k:  split(regs) -> buf[(k+1)&1];  global loads of stage k + 2 -> regs;  MFMAs from buf[k&1];  barrier
// LDS 2 x (3 TM + 3 x 128) x 64 B = 96 KB at TM = 128: one workgroup (two waves per SIMD) per CU.
// UNITS: the persistent form.  The stages of a workgroup's units form ONE stream through the two LDS buffers: the staging
// cursor (unit lu, stage lk) runs two stages ahead of the multiplication whatever unit either is in, so a unit boundary costs
// no pipeline fill, and a unit's results are stored behind the LDS write of the stage after its last (see gemm_x3_nt_kernel).
// A half-height unit is the first TM / 2 rows of its staged tile: the waves of the other rows skip their MFMAs and stores.
template <int TM, bool UNITS>
__global__ __launch_bounds__(512, 2) void gemm_x3_nt8_kernel(const float* __restrict__ A, const unsigned char* __restrict__ Bp,
                                                             float* __restrict__ C, int M, int N, int K, int bins, int mode) {
    constexpr int MI = TM / 64, A_BYTES = 3 * TM * 64, B_BYTES = 3 * 128 * 64;
    __shared__ __attribute__((aligned(16))) unsigned char As[2][A_BYTES], Bs[2][B_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 2, wn = wave & 3;
    const int KB = K / X3_BK;
    const X3Walk w = x3_walk<UNITS, TM>(M, N, bins, mode);
    if (w.n == 0) return;
    f32x16 acc[MI], cor[MI];
    // A staging: 8 lanes per row (a full 128-byte line), 64 rows per pass, MI passes
    const int k4 = tid & 7, rb0 = tid >> 3;
    const float* ap[MI];
    const unsigned char* Bb;
    auto aim = [&](const X3Unit& u) {
        const float* Ab = A + (size_t)u.bin * M * K;
#pragma unroll
        for (int v = 0; v < MI; ++v) {
            const int row = v * 64 + rb0;
            ap[v] = Ab + (size_t)(u.m0 + row < M ? u.m0 + row : M - 1) * K + k4 * 4;
        }
        Bb = Bp + (size_t)u.bin * x3_packed_bytes(N, K) + (size_t)u.nt * KB * B_BYTES;
    };
    f32x4 ra[MI], rb[3];
    auto gload = [&](int kb) {
#pragma unroll
        for (int v = 0; v < MI; ++v) ra[v] = *reinterpret_cast<const f32x4*>(ap[v] + (size_t)kb * X3_BK);
        const unsigned char* bsrc = Bb + (size_t)kb * B_BYTES + tid * 16;
#pragma unroll
        for (int v = 0; v < 3; ++v) rb[v] = *reinterpret_cast<const f32x4*>(bsrc + v * 8192);
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int v = 0; v < MI; ++v) {
            const int row = v * 64 + rb0;
            unsigned h0[3], h1[3];
            x3_split2(ra[v][0], ra[v][1], h0[0], h0[1], h0[2]);
            x3_split2(ra[v][2], ra[v][3], h1[0], h1[1], h1[2]);
            const int off = row * 64 + (((k4 >> 1) ^ x3_sw(row)) * 16) + (k4 & 1) * 8;
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const uint2 w = {h0[p], h1[p]};
                *reinterpret_cast<uint2*>(&As[buf][p * TM * 64 + off]) = w;
            }
        }
#pragma unroll
        for (int v = 0; v < 3; ++v) *reinterpret_cast<f32x4*>(&Bs[buf][v * 8192 + tid * 16]) = rb[v];
    };
    const int r32 = lane & 31, h = lane >> 5;
    const int f_sw = x3_sw(r32);
    const int wrow = wm * (TM / 2);
    const int a_base = (wrow + r32) * 64, b_base = (wn * 32 + r32) * 64;
    // the rows of a unit end at mend; nb = the wave's row blocks that hold a row below it (wave-uniform)
    auto wave_rows = [&](const X3Unit& u, int& mend, int& nb) {
        const int top = u.m0 + (u.hm ? TM / 2 : TM);
        mend = top < M ? top : M;
        const int left = (mend - u.m0 - wrow + 31) >> 5;
        nb = left < 0 ? 0 : left < MI ? left : MI;
    };
    auto store = [&](const X3Unit& u, int mend, int nb) {
        float* Cb = C + (size_t)u.bin * M * N;
        const int col = u.nt * 128 + wn * 32 + r32;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            if (i >= nb) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = u.m0 + wrow + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < mend) Cb[(size_t)m * N + col] = acc[i][r] + cor[i][r];
            }
        }
    };
    // staging cursor
    int lu = 0, lk = 0;
    auto fetch = [&]() {
        gload(lk);
        if (++lk == KB) {
            lk = 0;
            ++lu;
            if (UNITS && lu < w.n) aim(x3_unit<UNITS, TM>(w, lu));
        }
    };
    const int S = w.n * KB;                                  // stages of this workgroup, all units
    aim(x3_unit<UNITS, TM>(w, 0));
    fetch();
    lstore(0);
    if (S > 1) fetch();
    __syncthreads();
    X3Unit cu = x3_unit<UNITS, TM>(w, 0), pu = cu;
    int mend, nb, pmend = 0, pnb = 0;
    for (int u = 0, g = 0;; ++u) {
        wave_rows(cu, mend, nb);
        for (int kb = 0; kb < KB; ++kb, ++g) {
            const int cur = g & 1;
            if (g + 1 < S) lstore(cur ^ 1);                  // stage g + 1 (in registers since the last iteration)
            if (kb == 0) {
                if (UNITS && u > 0) store(pu, pmend, pnb);   // the previous unit's results, behind the loads just consumed
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { acc[i][r] = 0.f; cor[i][r] = 0.f; }
            }
            if (g + 2 < S) fetch();
            if (nb > 0) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int co = ((2 * s + h) ^ f_sw) * 16;
                    x3_bf16x8 af[MI][3], bf[3];
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        bf[p] = __builtin_bit_cast(x3_bf16x8, *reinterpret_cast<const uint4*>(&Bs[cur][p * 8192 + b_base + co]));
#pragma unroll
                        for (int i = 0; i < MI; ++i)
                            if (MI == 1 || i < nb)
                                af[i][p] = __builtin_bit_cast(x3_bf16x8, *reinterpret_cast<const uint4*>(&As[cur][p * TM * 64 + a_base + i * 2048 + co]));
                    }
#pragma unroll
                    for (int i = 0; i < MI; ++i) {            // (accumulator roles: see x3_stage_mfma)
                        if (MI > 1 && i >= nb) continue;
                        cor[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][2], bf[0], cor[i], 0, 0, 0);
                        cor[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], bf[1], cor[i], 0, 0, 0);
                        cor[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[2], cor[i], 0, 0, 0);
                        cor[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], bf[0], cor[i], 0, 0, 0);
                        cor[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[1], cor[i], 0, 0, 0);
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[0], acc[i], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }
        if (!(UNITS && u + 1 < w.n)) break;
        pu = cu; pmend = mend; pnb = nb;
        cu = x3_unit<UNITS, TM>(w, u + 1);
    }
    store(cu, mend, nb);
}

// Reduction-over-rows GEMM (the weight gradients):  P[split][bin][i][j] = sum_t A[bin][t][i] * Bm[bin][t][j], t in the split's
// chunk of the T rows -- both operands fp32 row-major [bins][T][NI] / [bins][T][NJ], read as they lie (rows = the reduction).
// The MFMA wants 8 consecutive t per lane: a thread loads 8 rows x 2 channels (coalesced 8-byte loads, a wave covers 128
// channels of one row), so the 8 t values of a channel already sit in one thread's registers -- the transposition is the
// register naming -- splits them and writes one 16-byte chunk per plane and channel: the LDS image is the NT kernel's
// ([plane][channel][32 t], chunk-swizzled) and the MFMA stage is shared.  Both operands are split on the fly here (32 values
// per thread and stage, ~176 vector instructions under 48 MFMAs per wave).
__global__ __launch_bounds__(256, 2) void gemm_x3_tn_kernel(const float* __restrict__ A, const float* __restrict__ Bm,
                                                            float* __restrict__ P, int T, int NI, int NJ, int nsplit, int bins) {
    __shared__ __attribute__((aligned(16))) unsigned char As[3 * 128 * 64], Bs[3 * 128 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int TI = NI / 128, TJ = NJ / 128;
    const int xcd = blockIdx.x & 7, sq = blockIdx.x >> 3;
    const int bin = (sq / (TI * TJ * nsplit)) * 8 + xcd;
    if (bin >= bins) return;
    const int split = (sq / (TI * TJ)) % nsplit, i0 = ((sq / TJ) % TI) * 128, j0 = (sq % TJ) * 128;
    const int chunk = ((T + nsplit - 1) / nsplit + 31) / 32 * 32;
    const int tb = split * chunk, te = tb + chunk < T ? tb + chunk : T;        // this workgroup reduces rows [tb, te)
    f32x16 acc[2][2], cor[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; cor[i][j][r] = 0.f; }
    // staging: thread = (t8 = tid >> 6: rows t8*8 .. t8*8+7 of the stage, cp = tid & 63: channels cp and cp + 64) -- a wave
    // instruction reads 64 consecutive channels of one row (256 B), and the eight lanes of a ds_write_b128 group write eight
    // CONSECUTIVE LDS rows at one chunk: conflict-free under x3_sw (with channels 2 cp, 2 cp + 1 per thread -- 8-byte loads --
    // the groups wrote even rows only: two-way conflicts on a third of all LDS cycles, profiles/r03_gemm_x3_pmc.json)
    const int t8 = tid >> 6, cp = tid & 63;
    const float* ap = A + ((size_t)bin * T) * NI + i0 + cp;
    const float* bp = Bm + ((size_t)bin * T) * NJ + j0 + cp;
    float ra[2][8], rb[2][8];
    auto gload = [&](int t0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int t = t0 + t8 * 8 + e;
            const bool in = t < te;
            const int tc = t < T ? t : T - 1;               // rows past the chunk are read (and dropped) from a row that exists
            const size_t ta = (size_t)tc * NI, tbo = (size_t)tc * NJ;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float va = ap[ta + c * 64], vb = bp[tbo + c * 64];
                ra[c][e] = in ? va : 0.f;
                rb[c][e] = in ? vb : 0.f;
            }
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int c = 0; c < 2; ++c) {                    // the thread's two channels = two LDS rows
            const int row = cp + c * 64;
            const int off = row * 64 + ((t8 ^ x3_sw(row)) * 16);
            unsigned ha[3][4], hb[3][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                x3_split2(ra[c][2 * q], ra[c][2 * q + 1], ha[0][q], ha[1][q], ha[2][q]);
                x3_split2(rb[c][2 * q], rb[c][2 * q + 1], hb[0][q], hb[1][q], hb[2][q]);
            }
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const uint4 va = {ha[p][0], ha[p][1], ha[p][2], ha[p][3]}, vb = {hb[p][0], hb[p][1], hb[p][2], hb[p][3]};
                *reinterpret_cast<uint4*>(&As[p * 8192 + off]) = va;
                *reinterpret_cast<uint4*>(&Bs[p * 8192 + off]) = vb;
            }
        }
    };
    const int r32 = lane & 31, h = lane >> 5;
    const int f_sw = x3_sw(r32);
    const int a_base = (wm * 64 + r32) * 64, b_base = (wn * 64 + r32) * 64;
    gload(tb);
    for (int t0 = tb; t0 < te; t0 += 32) {
        lstore();
        __syncthreads();
        if (t0 + 32 < te) gload(t0 + 32);
        x3_stage_mfma(As, Bs, a_base, b_base, h, f_sw, acc, cor);
        __syncthreads();
    }
    float* Pb = P + (((size_t)split * bins + bin) * NI) * NJ;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = j0 + wn * 64 + j * 32 + r32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                Pb[(size_t)row * NJ + col] = acc[i][j][r] + cor[i][j][r];
            }
        }
}

}  // namespace

void launch_x3_pack_rows(const float* src, void* dst, int bins, int rows, int K, hipStream_t st) {
    const int rows_pad = (rows + X3_TILE - 1) / X3_TILE * X3_TILE;
    const int64_t n = (int64_t)rows_pad * (K / 8);
    const int64_t nb = cdiv64(n, 256);
    hipLaunchKernelGGL(x3_pack_rows_kernel, dim3((unsigned)(nb < 4096 ? nb : 4096), bins), dim3(256), 0, st, src,
                       (unsigned char*)dst, rows, K, rows_pad);
}

// persistent grid of the NT kernels: two resident workgroups per CU, ROUNDED DOWN to a multiple of 8 (at least 8) -- the walk
// takes its stride from gridDim.x >> 3 (as cgemm_grid, conv_fft.hip)
// (Leaving one slot per XCD free where that costs no round was tried, for kernels of other streams: the 2160- and 540-row
// shapes lost what the walk had gained and the step 0.2 ms, profiles/x3_units_ab.txt.)
static int x3_units_grid() {
    const int g = 2 * gdn_num_cus() / 8 * 8;
    return g < 8 ? 8 : g;
}

void launch_gemm_x3_nt_cfg(const float* A, const void* Bp, float* C, int bins, int M, int N, int K, int cfg, int grid, hipStream_t st) {
    const int NT = N / 128, MT = (M + 127) / 128, bg = (bins + 7) / 8;
    int kern = cfg & 0xff;
    // Measured one-shot (B = 20, profiles/r03_gemm_x3_time_*.txt): the 256-thread kernel (two workgroups per CU, two barriers
    // per stage) is the fastest on the large GEMMs (level 3: 0.264 ms against 0.281 for the 512-thread double-buffered one);
    // with few row tiles (level 4, M = 1040: 576 tiles of 128 rows = 2.25 rounds of the chip) 64-row tiles win (0.067 against
    // 0.078 ms).  (gemm_x3_nt8_kernel<128> was measured against these two and is not dispatched.)
    // Persistent or one-shot, by the unit arithmetic and the ten NT shapes of the B = 20 step (profiles/x3_units_ab.txt): with
    // at most three rounds of units on the resident grid the static walk wins (2 - 8 %: no ragged dispatch, no fill and drain
    // per unit); with more rounds the hardware's dynamic dispatch balances units of unequal length better than a static list
    // (0 - 2 % for one-shot), so those shapes stay one-shot.  Half-height units in the last round: a workgroup's time is set by
    // its stage count, not by its MFMAs, so a half unit costs 0.9 of a whole one -- it pays only where a unit is long (32 or
    // more stages: 3 - 4 %) and costs 10 - 15 % at 16 stages, where the halves only add staging traffic.
    const int gfull = x3_units_grid();
    if (kern == X3_NT_AUTO) {
        const bool small = (int64_t)MT * NT * bins < 4 * 256;
        const int64_t units = (int64_t)(small ? (M + 63) / 64 : MT) * NT * bins;
        // Beside another stream's GEMM chain (the forked Winograd backward) the 64-row walk is one residency of every slot
        // for its whole run, and the other chain's GEMM waits for it instead of sharing the rounds: level 4's backward
        // 123.7 us with the walk, 120.0 one-shot (the 128-row walk at level 3 wins there too: 349.9 against 355.0).
        const bool walk = units <= 3 * (int64_t)gfull && !(small && (cfg & X3_NT_SHARED));
        kern = small ? (walk ? X3_NT_UNITS_64 : X3_NT_ONESHOT_64) : (walk ? X3_NT_UNITS_128 : X3_NT_ONESHOT_128);
        if (K / X3_BK < 32) cfg |= X3_NT_NO_HALVES;
    }
    const int mode = (cfg & X3_NT_KEEP_BINS ? 0 : X3_UNITS_PAIRS) | (cfg & X3_NT_NO_HALVES ? 0 : X3_UNITS_HALVE);
    const int g = grid > 0 ? grid : gfull;
    const unsigned char* B = (const unsigned char*)Bp;
    switch (kern) {
    case X3_NT_ONESHOT_128:
        hipLaunchKernelGGL(gemm_x3_nt_kernel<false>, dim3(MT * NT * bg * 8), dim3(256), 0, st, A, B, C, M, N, K, bins, 0);
        break;
    case X3_NT_ONESHOT_64:
        hipLaunchKernelGGL((gemm_x3_nt8_kernel<64, false>), dim3(((M + 63) / 64) * NT * bg * 8), dim3(512), 0, st, A, B, C, M, N, K, bins, 0);
        break;
    case X3_NT_UNITS_128:
        hipLaunchKernelGGL(gemm_x3_nt_kernel<true>, dim3(g), dim3(256), 0, st, A, B, C, M, N, K, bins, mode);
        break;
    default:
        hipLaunchKernelGGL((gemm_x3_nt8_kernel<64, true>), dim3(g), dim3(512), 0, st, A, B, C, M, N, K, bins, mode);
        break;
    }
}

void launch_gemm_x3_nt(const float* A, const void* Bp, float* C, int bins, int M, int N, int K, hipStream_t st) {
    launch_gemm_x3_nt_cfg(A, Bp, C, bins, M, N, K, X3_NT_AUTO, 0, st);
}

void launch_gemm_x3_tn(const float* A, const float* Bm, float* P, int bins, int T, int NI, int NJ, int nsplit, hipStream_t st) {
    const int bg = (bins + 7) / 8;
    hipLaunchKernelGGL(gemm_x3_tn_kernel, dim3((NI / 128) * (NJ / 128) * nsplit * bg * 8), dim3(256), 0, st, A, Bm, P, T, NI, NJ,
                       nsplit, bins);
}

// ---- C ABI: measurement / test hooks (the product path calls the launchers from the Winograd entry points) ----
extern "C" size_t gdn_gemm_x3_packed_bytes(int32_t bins, int32_t rows, int32_t K) {
    if (bins < 1 || rows < 1 || K < X3_BK || (K % X3_BK)) return 0;
    return (size_t)bins * x3_packed_bytes(rows, K);
}

extern "C" int gdn_gemm_x3_pack(const float* src, void* dst, int32_t bins, int32_t rows, int32_t K, void* stream) {
    (void)hipGetLastError();
    if (!src || !dst || bins < 1 || rows < 1 || K < X3_BK || (K % X3_BK)) return GDN_ERR_BAD_ARG;
    launch_x3_pack_rows(src, dst, bins, rows, K, (hipStream_t)stream);
    return gdn_launch_status();
}

extern "C" int gdn_gemm_x3_nt(const float* A, const void* Bp, float* C, int32_t bins, int32_t M, int32_t N, int32_t K,
                              void* stream) {
    (void)hipGetLastError();
    if (!A || !Bp || !C || bins < 1) return GDN_ERR_BAD_ARG;
    if (!gemm_x3_ok(M, N, K)) return GDN_ERR_UNSUPPORTED;
    launch_gemm_x3_nt(A, Bp, C, bins, M, N, K, (hipStream_t)stream);
    return gdn_launch_status();
}

// test / measurement hook: the same GEMM with the kernel form (one-shot or persistent, GDN_X3_NT_*) and, for the persistent
// forms, the grid chosen by the caller -- a tiny problem on 8 or 16 workgroups walks several rounds
extern "C" int gdn_gemm_x3_nt_cfg(const float* A, const void* Bp, float* C, int32_t bins, int32_t M, int32_t N, int32_t K,
                                  int32_t cfg, int32_t grid, void* stream) {
    (void)hipGetLastError();
    if (!A || !Bp || !C || bins < 1) return GDN_ERR_BAD_ARG;
    if ((cfg & 0xff) > X3_NT_UNITS_64 || (cfg & ~(0xff | X3_NT_KEEP_BINS | X3_NT_NO_HALVES | X3_NT_SHARED))) return GDN_ERR_BAD_ARG;
    if ((cfg & X3_NT_SHARED) && (cfg & 0xff) != X3_NT_AUTO) return GDN_ERR_BAD_ARG;
    if (grid < 0 || grid % 8 || grid > 8192) return GDN_ERR_BAD_ARG;
    if (!gemm_x3_ok(M, N, K)) return GDN_ERR_UNSUPPORTED;
    launch_gemm_x3_nt_cfg(A, Bp, C, bins, M, N, K, cfg, grid, (hipStream_t)stream);
    return gdn_launch_status();
}

// host query: the split count the reduction GEMM's callers use (gemm_x3.h cost model)
extern "C" int64_t gdn_gemm_x3_tn_splits(int32_t bins, int32_t T, int32_t NI, int32_t NJ) {
    if (bins < 1 || !gemm_x3_tn_ok(T, NI, NJ)) return 0;
    return gemm_x3_tn_splits(bins, T, NI, NJ);
}

extern "C" int gdn_gemm_x3_tn(const float* A, const float* Bm, float* P, int32_t bins, int32_t T, int32_t NI, int32_t NJ,
                              int32_t nsplit, void* stream) {
    (void)hipGetLastError();
    if (!A || !Bm || !P || bins < 1 || T < 1 || nsplit < 1) return GDN_ERR_BAD_ARG;
    if (!gemm_x3_tn_ok(T, NI, NJ)) return GDN_ERR_UNSUPPORTED;
    launch_gemm_x3_tn(A, Bm, P, bins, T, NI, NJ, nsplit, (hipStream_t)stream);
    return gdn_launch_status();
}
