// What conv_ring_bf16 (conv_ring.h) and conv_ring2_bf16 (conv_ring2.h) do identically, once: the per-form constants, the walk
// over work items, the per-tile tables, the LDS-DMA source offsets and the activation descriptor, the tail-range slab store
// and the epilogue.  Each kernel keeps what is its own: its LDS map, its DMA issue schedule, load_frags and its stage / tap loop.
// (included by conv_igemm.hip after IgemmParams / bf16x8 and before the two kernels)
#pragma once
#define RG_KMAX 9                         // filter rows
#define RG_AV 5                           // A pieces per wave and stage

// One record per kernel form (M-tile x N-tile), read by the kernels and by the host's ring_kw / ring_plan / ring_ws_bytes.
//   BM x BN the tile; SLAB the channels of a stage; ROWB the bytes of an LDS row (one position, SLAB channels), whose 16-byte
//   chunks are XOR-permuted by (row >> SWZ) & (ROWB / 16 - 1); NRMAX the image rows a tile may touch; APOS the staged patch
//   positions per A buffer (5 LDS-DMA pieces of 1 KB per wave); TAIL_SLABS the fp32 slabs a tail range writes.
template <int BN_>
struct RingForm256 {                      // conv_ring_bf16: 64-channel slabs (W >= 26)
    static constexpr int BM = 256, BN = BN_, SLAB = 64, ROWB = 128, SWZ = 1, NRMAX = 12, APOS = 320;
    static constexpr int TAIL_SLABS = 128 / BN_;                      // BN = 64: the two halves of the reduction write one each
};
template <int BN_>
struct RingForm512 {                      // conv_ring2_bf16: 32-channel slabs (W >= 52)
    static constexpr int BM = 512, BN = BN_, SLAB = 32, ROWB = 64, SWZ = 2, NRMAX = 12, APOS = 640;
    static constexpr int TAIL_SLABS = 1;
};
struct RingFormV { int bm, slab, nrmax, apos, tail_slabs; };          // the host's view of a record
template <class F> constexpr RingFormV ring_form_v() { return {F::BM, F::SLAB, F::NRMAX, F::APOS, F::TAIL_SLABS}; }
inline RingFormV ring_form(int cfg) {     // tile ids 10 / 11 / 12; 13 (512 x 128) is planned as the 512 form and never launched
    return cfg == 10 ? ring_form_v<RingForm256<64>>() : cfg == 11 ? ring_form_v<RingForm256<128>>() :
           cfg >= 12 ? ring_form_v<RingForm512<64>>() : RingFormV{};       // (no ring form: every caller checks cfg >= 10 first)
}

// a table set: row_out[BM] output pixel index or -1 | rowoff[RG_KMAX][NRMAX] byte offset of input row or -1 |
//              rbase[NRMAX + 1] first patch position of each touched image row | rxlo[NRMAX] first output column of
//              the tile in that row | {nrows, b_first}
template <class F>
struct RingTab {
    static constexpr int ROWOFF = F::BM, RBASE = ROWOFF + RG_KMAX * F::NRMAX, RXLO = RBASE + F::NRMAX + 1, MISC = RXLO + F::NRMAX;
    static constexpr int N = MISC + 3;                                // ints per table set (392 / 648)
};

template <int N> __device__ __forceinline__ void rg_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
typedef __attribute__((address_space(3))) void* rg_lds_ptr;
// The kernel body is compiled in the DEVICE pass only: the host pass of hipcc needs the kernel's stub, not its body, and it
// gives up on the stub without a diagnostic when the body uses the LDS-DMA builtin inside nested lambdas (ROCm 7.2).
#if defined(__HIP_DEVICE_COMPILE__)
#define RG_DEVICE_BODY 1
#else
#define RG_DEVICE_BODY 0
#endif
#if RG_DEVICE_BODY
// (lane_e / tid_e / lane_p: the epilogue's and the slab store's lane-dependent addresses are invariant across tiles, and hoisted
//  out of the tile loop they would occupy ~60 registers throughout the tap loop -- an opaque copy of the lane index keeps them
//  inside the epilogue)
__device__ __forceinline__ int rg_opaque(int v) { asm volatile("" : "+v"(v)); return v; }

// ---- a workgroup's work items.  Workgroups b, b + 8, ... share an XCD (its L2): an XCD owns a contiguous band of units
// ((M-tile, N-tile), N-tiles adjacent; neighbouring tiles re-read each other's halo rows), walked by its workgroups side by
// side.  B = 20 gives 65/64 of a power of two tiles at every level of the pyramid: the last, nearly empty round would cost
// a whole tile time.  So when the host planned a split (p.ksplit = parts > 1), the p.ring_main units of the full rounds are
// walked as bands and each unit of the last round is cut into `parts` ranges of p.ring_sp stages, one per workgroup, whose
// raw fp32 accumulators go to slabs in p.part; splitk_combine_kernel sums them and applies the epilogue for those pixels.
struct RingItem { int mt, nt, s0, s1, part; };                        // (M-tile, N-tile, stage range, slab index or -1)
struct RingWalk {
    int bid, xcd, wg_in_xcd, wgs_per_xcd, parts, per_xcd, units_xcd, rounds_main, tail_items, nstage;
    // nstage: (filter row, channel slab) stages; knob bit 0: skip the loop, bit 3: a third of it (what a tile costs outside / per stage)
    __device__ __forceinline__ RingWalk(const IgemmParams& p, int knobs, int stages)
        : bid(blockIdx.x), xcd(bid & 7), wg_in_xcd(bid >> 3), wgs_per_xcd((int)gridDim.x >> 3), parts((knobs & 9) ? 1 : p.ksplit),
          per_xcd((p.grid_m + 7) >> 3), units_xcd(parts > 1 ? p.ring_main >> 3 : per_xcd * p.grid_n),
          rounds_main(parts > 1 ? units_xcd / wgs_per_xcd : (units_xcd + wgs_per_xcd - 1) / wgs_per_xcd),
          tail_items(parts > 1 ? (p.grid_m * p.grid_n - p.ring_main) * parts : 0),
          nstage((knobs & 1) ? 0 : (knobs & 8) ? stages / 3 : stages) {}
    // item k of this workgroup; false: no such item
    __device__ __forceinline__ bool get(const IgemmParams& p, int k, RingItem& it) const {
        if (k < rounds_main) {
            const int q = wg_in_xcd + k * wgs_per_xcd;
            if (q >= units_xcd) return false;
            const int u = parts > 1 ? xcd * units_xcd + q : (xcd * per_xcd + q / p.grid_n) * p.grid_n + q % p.grid_n;
            it.mt = u / p.grid_n; it.nt = u % p.grid_n; it.s0 = 0; it.s1 = nstage; it.part = -1;
            return it.mt < p.grid_m;
        }
        if (k == rounds_main && bid < tail_items) {
            const int u = p.ring_main + bid / parts;
            it.part = bid % parts;
            it.mt = u / p.grid_n; it.nt = u % p.grid_n;
            it.s0 = it.part * p.ring_sp; it.s1 = min(nstage, it.s0 + p.ring_sp);
            return it.s0 < it.s1;
        }
        return false;
    }
    // the item after item k (k = -1: the first): k and it are updated; a workgroup without a main unit there may still own a tail range
    __device__ __forceinline__ bool next(const IgemmParams& p, int& k, RingItem& it) const {
        if (get(p, ++k, it)) return true;
        if (k >= rounds_main) return false;
        k = rounds_main;
        return get(p, k, it);
    }
};

// tables of the tile with first pixel m0 into set t (every thread takes part; the caller orders them with a barrier)
template <class F, int KW>
__device__ __forceinline__ void ring_setup_tables(int* t, const IgemmParams& p, const IgemmPhase& ph, int m0, int M, int kh, int tid) {
    using T = RingTab<F>;
    const int Wo = ph.Wo, Ho = ph.Ho;
    const int mlast = min(m0 + F::BM, M) - 1;
    const int row0 = m0 / Wo, nrows = mlast / Wo - row0 + 1;
    const int b_first = row0 / Ho;
    if (F::BM == 512 || tid < F::BM) {
        const int m = m0 + tid;
        int v = -1;
        if (m < M) {
            const int ox = m % Wo, tt = m / Wo, oy = tt % Ho, b_ = tt / Ho;
            v = (b_ * p.Hy + oy * p.osy + ph.oy0) * p.Wy + ox * p.osx + ph.ox0;
        }
        t[tid] = v;
    }
    if (tid <= nrows) {
        const int xlo0 = m0 - row0 * Wo;
        const int before = tid == 0 ? 0 : (Wo - xlo0) + (tid - 1) * Wo;
        t[T::RBASE + tid] = (tid == nrows ? min(F::BM, M - m0) : before) + tid * (KW - 1);
        if (tid < nrows) t[T::RXLO + tid] = tid == 0 ? xlo0 : 0;
    }
    if (tid == 511) { t[T::MISC] = nrows; t[T::MISC + 1] = b_first; }
    if (tid >= 256 && tid < 256 + kh * F::NRMAX) {
        const int i = tid - 256;
        const int ky = i / F::NRMAX, j = i - ky * F::NRMAX;
        int off = -1;
        if (j < nrows) {
            const int tt = row0 + j, oy = tt % Ho, b_ = tt / Ho;
            int iy = oy * p.stride + p.tdy[ph.tap_begin + ky * KW];
            if (p.pad_mode == 1) iy = reflect_idx(iy, p.Hi);
            if ((unsigned)iy < (unsigned)p.Hi) off = (((b_ - b_first) * p.Hi + iy) * p.Wi) * p.ldx1 * 2;
        }
        t[T::ROWOFF + i] = off;
    }
}

// ---- LDS-DMA sources.  A piece writes 1 KB = 1024 / ROWB rows linearly, lane l the 16-byte slot l % (ROWB / 16) of row
// l / (ROWB / 16): the chunk permutation is applied to the per-lane SOURCE address (same line: the global side stays fully
// coalesced) and again on the read.
constexpr unsigned RG_OOB = 0xFFFFFF00u;  // a source offset the descriptor's range check drops
template <class F> __device__ __forceinline__ int ring_piece_row(int piece, int lane) { return piece * (1024 / F::ROWB) + lane / (F::ROWB / 16); }
template <class F> __device__ __forceinline__ unsigned ring_src_chunk(int row, int lane) {     // logical chunk stored at this lane's physical slot, in bytes
    return (unsigned)((lane & (F::ROWB / 16 - 1)) ^ ((row >> F::SWZ) & (F::ROWB / 16 - 1))) * 16u;
}
// row n < BN of the weight tile at output channel n0
template <class F> __device__ __forceinline__ unsigned ring_w_offset(const IgemmParams& p, int n0, int n, int lane) {
    return (n0 + n) < p.N ? (unsigned)((n0 + n) * p.Cred) * 2u + ring_src_chunk<F>(n, lane) : RG_OOB;
}
// The tile whose tables are t: pk[e], patch piece e of this wave = piece e * 8 + wave of the stage's 40: per-lane column offset, with
// the image-row index j of the position in its low 4 bits (the offset is a multiple of 16); returns the activation descriptor
// (its words through readfirstlane: a descriptor the compiler cannot PROVE wave-uniform gets a waterfall loop around every LDS-DMA)
template <class F>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ring_tile_sources(const int* t, const IgemmParams& p, int dxmin, int knobs, int wave, int lane,
                                                                    unsigned (&pk)[RG_AV]) {
    using T = RingTab<F>;
    const int nrows = __builtin_amdgcn_readfirstlane(t[T::MISC]), b_first = __builtin_amdgcn_readfirstlane(t[T::MISC + 1]);
    const int npatch = t[T::RBASE + nrows];
#pragma unroll
    for (int e = 0; e < RG_AV; ++e) {
        const int q = ring_piece_row<F>(e * 8 + wave, lane);
        int j = 0;
        for (int jj = 1; jj < nrows; ++jj) j += (q >= t[T::RBASE + jj]) ? 1 : 0;
        int ix = t[T::RXLO + j] + dxmin + (q - t[T::RBASE + j]);
        if (p.pad_mode == 1) ix = reflect_idx(ix, p.Wi);
        const bool ok = q < npatch && (unsigned)ix < (unsigned)p.Wi;
        pk[e] = ok ? ((unsigned)(ix * p.ldx1) * 2u + ring_src_chunk<F>(q, lane)) | (unsigned)j : RG_OOB;
    }
    const unsigned long long img1 = (unsigned long long)p.Hi * p.Wi * p.ldx1 * 2ull * b_first;
    const unsigned long long rem1 = p.x_bytes - img1, cap = 0xFF000000ull;
    const unsigned long long xb = reinterpret_cast<unsigned long long>(p.x) + img1;
    const unsigned long long xbu = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(xb >> 32)) << 32) |
                                   (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)xb);
    const int xlen = __builtin_amdgcn_readfirstlane((knobs & 4) ? 0 : (int)(unsigned)(rem1 < cap ? rem1 : cap));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(xbu), 0, xlen, 0x00020000);
}

// A new tile: zeroed accumulators, and apos -- pixel r of the tile sits at patch position r + j(r) * (KW - 1) (+ the tap's shift);
// this lane's rows of pixel group wm
template <class F, int KW, int NJ>
__device__ __forceinline__ void ring_tile_begin(int m0, int M, int Wo, int wm, int lane, unsigned (&apos)[2], f32x16 (&acc)[2][NJ]) {
    const int mlast = min(m0 + F::BM, M) - 1;
    const int row0 = m0 / Wo;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = wm * 64 + i * 32 + (lane & 31);
        const int m = min(m0 + r, mlast);
        apos[i] = (unsigned)(min(r, mlast - m0) + (m / Wo - row0) * (KW - 1));
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r2 = 0; r2 < 16; ++r2) acc[i][j][r2] = 0.f;
    }
}

// ---- a tail range: the raw fp32 accumulators of pixel group wm, columns [ncol, ncol + 32 NJ) go to slab `slab_i` of p.part;
// splitk_combine_kernel does the rest ----
template <class F, int NJ>
__device__ __forceinline__ void ring_store_tail(const IgemmParams& p, const int* t, const f32x16 (&acc)[2][NJ], int slab_i, int m0, int M,
                                                int ncol, int wm, int lane) {
    const int lane_p = rg_opaque(lane);
    const int m_tail0 = (p.ring_main / p.grid_n) * F::BM;
    const size_t tail_px = (size_t)(M - m_tail0);
    float* slab = p.part + ((size_t)slab_i * tail_px + (size_t)(m0 - m_tail0)) * p.N + ncol + (lane_p & 31);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane_p >> 5);
            if (t[row] >= 0) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) slab[(size_t)row * p.N + j * 32] = acc[i][j][r];
            }
        }
}

// ---- epilogue of tile (mt, n0) whose row_out table is t.  This wave finalises NI row tiles of 32 pixels from tile row rbase0
// (row tile ii covers tile rows rbase0 + 32 ii + rowmap(r, lane_e)) and NJ column tiles of 32 channels from column ncol0 (waves
// with the same ncol0 hold the same columns: BN / (32 NJ) column halves of 8 / halves waves each).  sc: at least 34 KB of scratch
// behind the LDS the next prologue lands in; coef: [4][BN] floats.  The fusions are the ones of conv_igemm_bf16: BatchNorm sum /
// sum-of-squares partials, eval-BN affine, ReLU, residual, tanh; BNB: the instantiation that can also emit BatchNorm-backward partials.
template <class F, int NI, int NJ, bool BNB>
__device__ __forceinline__ void ring_epilogue(const IgemmParams& p, const int* t, float* sc, float* coef, const f32x16 (&acc)[2][NJ], int mt, int n0,
                                              int rbase0, int ncol0, int wave, int lane_e, int tid_e) {
    constexpr int BN = F::BN, CW = 32 * NJ;          // CW: columns a wave holds
    const int col_l = lane_e & 31, rsh = 4 * (lane_e >> 5);
    if (p.stats && !(BNB && p.bnb_y)) {
        float* red = sc;                             // [8 waves][CW columns][2]
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int ii = 0; ii < NI; ++ii)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
#pragma clang fp contract(off)      // (every square rounded before it is added, as these kernels always compiled it; the exact-result tests pin it)
                    const int row = rbase0 + ii * 32 + (r & 3) + 8 * (r >> 2) + rsh;
                    const float v = t[row] >= 0 ? acc[ii][j][r] : 0.f;
                    s1 += v; s2 += v * v;
                }
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            if (lane_e < 32) {
                red[(wave * CW + j * 32 + lane_e) * 2 + 0] = s1;
                red[(wave * CW + j * 32 + lane_e) * 2 + 1] = s2;
            }
        }
        __syncthreads();
        if (tid_e < BN && n0 + tid_e < p.N) {
            // column half z of the tile is held by the waves [z 8 CW / BN, (z + 1) 8 CW / BN): summed in a fixed order
            float s1 = 0.f, s2 = 0.f;
            const float* rc = red + (tid_e & (CW - 1)) * 2;
            const int z = tid_e / CW;
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                if (CW < BN && w / (8 * CW / BN) != z) continue;
                s1 += rc[w * CW * 2];
                s2 += rc[w * CW * 2 + 1];
            }
            p.stats[((size_t)mt * 2 + 0) * p.N + n0 + tid_e] = s1;
            p.stats[((size_t)mt * 2 + 1) * p.N + n0 + tid_e] = s2;
        }
        __syncthreads();
    }
    // output: 8192 values per round go through an fp32 LDS tile [pixel][BN + 4] and leave as whole 128-byte lines
    // (16 bytes = 8 channels per lane_e); the eval-BN affine / ReLU are applied on the way in, the residual is read 16
    // bytes at a time and added (in fp32, before the one rounding to bf16) on the way out
    const bool has_affine = p.ep_scale != nullptr;
    float es[NJ], et[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int n = n0 + ncol0 + j * 32 + col_l;
        es[j] = (has_affine && n < p.N) ? p.ep_scale[n] : 1.f;
        et[j] = (has_affine && n < p.N) ? p.ep_shift[n] : 0.f;
    }
    constexpr int RS = BN + 4;                       // row stride of the transposition tile in floats
    constexpr int PXR = 8192 / BN;                   // pixels per round: 128 (BN = 64) or 64 (BN = 128); a wave's rows all fall into round rbase0 / PXR
    constexpr int NRND = F::BM / PXR;
    constexpr int TPP = BN / 8;                      // threads per pixel on the way out
    unsigned short* yo = reinterpret_cast<unsigned short*>(p.y);
    const unsigned short* ad = reinterpret_cast<const unsigned short*>(p.addsrc);
    // bnb mode (a data gradient that is the final gradient of z = [relu](BN_train(bnb_y))): the BatchNorm backward's partial
    // sums sum dz, sum dz * xhat over this tile's pixels, from the values as they are stored (rounded to bf16), so the
    // stand-alone reduce pass over (dx, y) disappears; slot = tile, like the forward's sum / sum of squares
    const bool bnb = BNB && p.bnb_y != nullptr;
    float bs1[8] = {}, bs2[8] = {};
    if (BNB && bnb) {
        for (int i = tid_e; i < 4 * BN; i += 512) {
            const int n = n0 + i % BN;
            coef[i] = n < p.N ? p.bnb_co[(size_t)(i / BN) * p.N + n] : 0.f;
        }
    }
#pragma unroll 1
    for (int rr = 0; rr < NRND; ++rr) {
        if (rbase0 / PXR == rr) {
#pragma unroll
            for (int ii = 0; ii < NI; ++ii)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = rbase0 + ii * 32 + (r & 3) + 8 * (r >> 2) + rsh - rr * PXR;
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        float v = acc[ii][j][r];
                        if (has_affine) v = v * es[j] + et[j];
                        if (p.act & GDN_ACT_RELU) v = fmaxf(v, 0.f);
                        sc[row * RS + ncol0 + j * 32 + col_l] = v;
                    }
                }
        }
        __syncthreads();
#pragma unroll
        for (int ps = 0; ps < PXR * TPP / 512; ++ps) {
            const int px = ps * (512 / TPP) + tid_e / TPP, cg = tid_e % TPP;
            const int op = t[rr * PXR + px];
            if (op >= 0 && n0 + cg * 8 < p.N) {
                f32x4 lo = *reinterpret_cast<const f32x4*>(sc + px * RS + cg * 8);
                f32x4 hi = *reinterpret_cast<const f32x4*>(sc + px * RS + cg * 8 + 4);
                if (ad) {
                    f32x4 alo, ahi;
                    ld8_any(ad, (size_t)op * p.ld_add + n0 + cg * 8, 1, alo, ahi);
                    lo += alo; hi += ahi;
                }
                if (p.act & GDN_ACT_TANH) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { lo[e] = tanhf(lo[e]); hi[e] = tanhf(hi[e]); }
                }
                st8_any(yo, (size_t)op * p.ldy + n0 + cg * 8, lo, hi, 1);
                if (BNB && bnb) {
                    f32x4 ylo, yhi;
                    ld8_any(p.bnb_y, (size_t)op * p.ld_bnb + n0 + cg * 8, 1, ylo, yhi);
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        const f32x4 yv = hh ? yhi : ylo, dv = hh ? hi : lo;
                        const f32x4 csc = *reinterpret_cast<const f32x4*>(coef + cg * 8 + hh * 4);
                        const f32x4 csh = *reinterpret_cast<const f32x4*>(coef + BN + cg * 8 + hh * 4);
                        const f32x4 cmu = *reinterpret_cast<const f32x4*>(coef + 2 * BN + cg * 8 + hh * 4);
                        const f32x4 cis = *reinterpret_cast<const f32x4*>(coef + 3 * BN + cg * 8 + hh * 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float dz = bn_dz(bf16_h_to_f32(f32_to_bf16_h(dv[e])), yv[e], csc[e], csh[e], p.bnb_relu);
                            bs1[hh * 4 + e] += dz;
                            bs2[hh * 4 + e] += dz * bn_xhat(yv[e], cmu[e], cis[e]);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    if (BNB && bnb) {
        // thread (pixel lane q = tid / TPP, channel group cg = tid % TPP) -> per-channel sums over the 512 / TPP pixel lanes
#pragma unroll
        for (int e = 0; e < 8; ++e) { sc[tid_e * 16 + e] = bs1[e]; sc[tid_e * 16 + 8 + e] = bs2[e]; }
        __syncthreads();
        if (tid_e < 2 * BN) {
            const int c = tid_e % BN, which = tid_e / BN;
            float a = 0.f;
            for (int q = 0; q < 512 / TPP; ++q) a += sc[(q * TPP + (c >> 3)) * 16 + which * 8 + (c & 7)];
            if (n0 + c < p.N) p.stats[((size_t)mt * 2 + which) * p.N + n0 + c] = a;
        }
        __syncthreads();
    }
}
#endif  // RG_DEVICE_BODY
