// conv_ring2_bf16: the LDS-DMA ring kernel (conv_ring.h) with ONE barrier per (filter row, slab) stage (round 5).
// (included by conv_igemm.hip after ring_common.h and conv_ring.h)
//
// conv_ring_bf16 synchronises its eight waves at every tap step -- 8 MFMAs per wave between two raw barriers, with two waves
// per SIMD and nobody else on the CU: 45-55 % of the matrix pipe's cycles inside the tap loop go to barrier skew and counted
// vmcnt waits (r04b_ring_probe.txt; NOT to LDS-DMA bytes: a third less traffic bought 3 %).  wgrad_ring_bf16 (wgrad_ring.h),
// which synchronises once per stage, keeps the pipe 67 % busy.  This kernel gives the forward / data-gradient the same shape:
//   * a stage is (filter row, 32-CHANNEL slab): LDS rows are 64 bytes; the patch of a 512-pixel tile with its halos is 40 KB
//     (640 positions) and the KW weight tiles of the stage are KW x 4 KB (BN = 64) -- small enough to hold TWO whole stages
//     (patch + every weight tile: 2 x 76 KB for a 9-tap row) in LDS.  While stage s computes, every wave fires its ten pieces
//     of stage s + 1 into the other pair, one or two per tap step under the MFMAs; the boundary (vmcnt(0) lgkmcnt(0), barrier)
//     sits inside the last k-substep in front of its MFMAs, and the first fragment reads of the next stage land under them.
//     72 MFMAs per wave run between two barriers.
//   * 512-pixel tiles: the 8 waves are 8 pixel groups of 64 (no split of the reduction between waves, no exchange in the
//     epilogue), every weight tile serves twice the pixels of conv_ring_bf16's, and the ~7 us a tile spends outside its tap loop
//     are paid half as often;
//   * 64-byte rows: the four 16-byte chunks of a row are XOR-permuted by (row >> 2) & 3, so the 16 rows a ds_read_b128 lane
//     group touches fall on 16 different 16-byte bank slots; an LDS-DMA piece is 16 rows; the permutation is applied to the
//     per-lane SOURCE address and on the read;
//   * everything else -- persistent workgroups, tables, the next tile's prologue before the epilogue, the K-split tail, the
//     epilogue fusions -- is ring_common.h's, shared with conv_ring_bf16.
// One-stage-ahead prefetch needs a stage longer than the DMA latency: 9 / 7-tap rows (2.2 / 1.7 us of MFMA work per stage); the
// 5- and 3-tap layers stay on conv_ring_bf16's four-step-ahead ring.  B = 20, 9x9 64 -> 64: 1249 vs 1155 TFLOP/s.
#pragma once
// BNB: as conv_ring_bf16's
template <int BN, int KW, bool BNB = false>
__global__ __launch_bounds__(512, 2) void conv_ring2_bf16(const IgemmParams p) {
#if RG_DEVICE_BODY
    using F = RingForm512<BN>;
    using T = RingTab<F>;
    constexpr int BM = F::BM, ABYTES = F::APOS * F::ROWB;
    constexpr int TILE_B = BN * 64;                          // weight tile: BN rows of 32 channels
    constexpr int PT = BN / 16;                              // LDS-DMA pieces per weight tile (16 rows x 64 bytes each)
    constexpr int NBW = (KW * PT + 7) / 8;                   // weight pieces per wave and stage (all KW tiles of the stage)
    constexpr int NG = 2;                                    // 16-channel k-substeps per step
    constexpr int NJ = BN / 32;                              // column tiles per wave
    static_assert(PT == 4 || PT == 8, "a wave's pieces all cover the same rows of their tiles");
    // LDS map: [A buffer 0 | weight set 0 | A buffer 1 | weight set 1 | two table sets | coefficients].  A stage reads one
    // (A buffer, weight set) pair while the LDS-DMA of the next stage fills the other.  The next tile's prologue lands in pair
    // 0; pair 1 is the epilogue's scratch meanwhile.
    constexpr int A0 = 0, B0 = ABYTES, A1 = B0 + KW * TILE_B, B1 = A1 + ABYTES, TAB0 = B1 + KW * TILE_B;
    constexpr int SC0 = A1;                                  // epilogue scratch: [SC0, TAB0)
    constexpr int TABSET = T::N * 4;
    static_assert(TAB0 - SC0 >= 35 * 1024, "LDS map");
    // ONE shared object: the compiler must see a single LDS array beside the LDS-DMA instructions
    constexpr int COEF0 = TAB0 + 2 * TABSET + 64;            // [4][BN] floats: the BatchNorm coefficients of a data gradient's bnb mode
    static_assert(COEF0 + 4 * 128 * 4 <= 160 * 1024, "LDS size");
    __shared__ __attribute__((aligned(16))) unsigned char sm[COEF0 + 4 * 128 * 4];
    int* const wirow = reinterpret_cast<int*>(sm + TAB0 + 2 * TABSET);    // [RG_KMAX] weight index of the first tap of each filter row
    auto tab = [&](int b) { return reinterpret_cast<int*>(sm + TAB0 + b * TABSET); };

    const int knobs = p.kc;                                  // measurement knobs (0 in production)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave;                                     // pixel group: tile rows [64 wm, 64 wm + 64)
    const IgemmPhase ph = p.ph[0];
    const int M = p.B * ph.Ho * ph.Wo;
    const int kh = (ph.tap_end - ph.tap_begin) / KW;
    // (taps of a filter row: consecutive in the weight tensor and in dx, as in conv_ring_bf16)
    const int dx_first = p.tdx[ph.tap_begin], dx_last = p.tdx[ph.tap_begin + KW - 1];
    const int dxmin = min(dx_first, dx_last);
    const bool dx_up = dx_last >= dx_first;
    const int nchunks = p.Cred / F::SLAB;
    const int tap2 = p.w_tap_stride * 2;
    const RingWalk walk(p, knobs, kh * nchunks);
    // ---- per-tile state ----
    unsigned pk[RG_AV];             // patch piece e of this wave (16 positions x 4 chunks): ring_tile_sources
    unsigned boff;               // this wave's weight pieces are rows [16 (wave % PT), + 16) of their tiles (16 rows x 4 chunks)
    unsigned a_vo[RG_AV];           // per-lane source offsets of the patch pieces of one stage
    __amdgpu_buffer_rsrc_t rs_x;
    // (knob bits 1 / 2: zero-length weight / activation descriptor, as in conv_ring_bf16)
    __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, (knobs & 2) ? 0 : (int)p.w_bytes, 0x00020000);

    auto tile_dma_state = [&](int b, int n0) {      // pk / boff / the activation descriptor of the tile whose tables are set b
        rs_x = ring_tile_sources<F>(tab(b), p, dxmin, knobs, wave, lane, pk);
        boff = ring_w_offset<F>(p, n0, ring_piece_row<F>(wave & (PT - 1), lane), lane);
    };
    auto a_offsets = [&](int b, int ky) {                    // (read from the row table once per stage, not under the MFMAs)
        const int* t = tab(b);
#pragma unroll
        for (int e = 0; e < RG_AV; ++e) {
            const int ro = t[T::ROWOFF + ky * F::NRMAX + (int)(pk[e] & 15u)];
            a_vo[e] = (ro >= 0 && pk[e] != RG_OOB) ? (unsigned)ro + (pk[e] & ~15u) : RG_OOB;
        }
    };
    auto dma_a = [&](int par, int cc, int e) {               // piece e of the patch whose offsets are in a_vo -> A buffer `par`
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (rg_lds_ptr)(sm + (par ? A1 : A0) + (e * 8 + wave) * 1024), 16, a_vo[e], cc * 64, 0, 0);
    };
    // piece e of this wave of the KW weight tiles of the stage whose first tap lies at scalar offset soff -> weight set `par`:
    // piece e * 8 + wave of the KW * PT (tile kx = piece / PT at soff + kx * tap2).  A piece past the last one re-loads the wave's
    // previous piece (same bytes to the same place), so that every wave issues the same number of loads.
    auto dma_bw = [&](int par, int soff, int e) {
        int pi = e * 8 + wave;
        if (pi >= KW * PT) pi -= 8;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (rg_lds_ptr)(sm + (par ? B1 : B0) + pi * 1024), 16, boff,
                                                 soff + (pi / PT) * tap2, 0, 0);
    };
    // (stage cursor: as conv_ring_bf16's; past the last stage the "next" stage is the last one again, reloaded into the idle pair)
    auto stage_soff = [&](int ky_, int cc_) { return __builtin_amdgcn_readfirstlane(wirow[ky_]) * tap2 + cc_ * F::ROWB; };
    int ky_n = 0, cc_n = 0, soff_c = 0, soff_n = 0;
    auto start_item = [&](int b, int n0, int s0, int ns) {   // tile_dma_state, then the first stage's patch and weight tiles of the item in table set b
        tile_dma_state(b, n0);
        const int ky0 = s0 / nchunks, cc0 = s0 - ky0 * nchunks;
        ky_n = ky0; cc_n = cc0;
        if (ns > 1) { if (++cc_n == nchunks) { cc_n = 0; ++ky_n; } }
        soff_c = stage_soff(ky0, cc0); soff_n = stage_soff(ky_n, cc_n);
        a_offsets(b, ky0);
#pragma unroll
        for (int e = 0; e < RG_AV; ++e) dma_a(0, cc0, e);
#pragma unroll
        for (int e = 0; e < NBW; ++e) dma_bw(0, soff_c, e);
    };
    // ---- fragment addressing ----
    // k-substep g of a step covers channels [16 g, 16 g + 16) of the slab: lane half h reads chunk 2 g + h
    const unsigned hbit = (unsigned)(lane >> 5) << 4;
    unsigned bfix[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const unsigned n = (unsigned)(j * 32 + (lane & 31));
        bfix[j] = ((n << 6) ^ (((n >> 2) & 3u) << 4)) ^ hbit;
    }
    unsigned apos[2];                                // ring_tile_begin
    f32x16 acc[2][NJ];
    bf16x8 fa[2][2], fb[2][NJ];                      // [register set][row tile / column tile]
    auto load_frags = [&](int set, int par, int kx, int g) {     // fragments of (pair par, tap kx, k-substep g)
        const unsigned sh = (unsigned)(dx_up ? kx : KW - 1 - kx);
        const unsigned abase = (unsigned)(par ? A1 : A0);
        const unsigned bbase = (unsigned)((par ? B1 : B0) + kx * TILE_B);
        const unsigned gx = (unsigned)g << 5;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const unsigned q = apos[i] + sh;
            const unsigned a = abase + (((q << 6) ^ (((q >> 2) & 3u) << 4)) ^ hbit ^ gx);
            fa[set][i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const f32x4*>(sm + a));
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            fb[set][j] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const f32x4*>(sm + bbase + (bfix[j] ^ gx)));
    };
    // ---- first item ----
    int k_item = -1, tb = 0;
    RingItem it{0, 0, 0, 0, -1};
    if (!walk.next(p, k_item, it)) return;
    if (tid < kh) wirow[tid] = p.twi[ph.tap_begin + tid * KW];
    ring_setup_tables<F, KW>(tab(0), p, ph, it.mt * BM, M, kh, tid);
    __syncthreads();
    start_item(0, it.nt * BN, it.s0, it.s1 - it.s0);
    for (;;) {
        const int m0 = it.mt * BM, n0 = it.nt * BN, ns = it.s1 - it.s0;
        int k_n = k_item;
        RingItem nx{0, 0, 0, 0, -1};
        const bool has_next = walk.next(p, k_n, nx);
        const int* const t = tab(tb);
        ring_tile_begin<F, KW>(m0, M, ph.Wo, wm, lane, apos, acc);
        if (has_next) ring_setup_tables<F, KW>(tab(tb ^ 1), p, ph, nx.mt * BM, M, kh, tid);   // (the other set: ordered by the loop's barriers before anyone reads it)
        rg_wait_vm<0>();                                            // the prologue pieces (and the previous epilogue's stores)
        __builtin_amdgcn_s_barrier();
        if (ns > 0) load_frags(0, 0, 0, 0);

        // ---- stage walk: ONE barrier per stage.  During stage s every wave fires its pieces of stage s + 1 (patch and all KW
        // weight tiles) into the other pair, one or two per tap step under the MFMAs; the boundary -- vmcnt(0) lgkmcnt(0), barrier --
        // sits inside the last k-substep, in front of its MFMAs, whose operands are in registers by then: behind the barrier the
        // first fragments of the next stage are requested and land under those MFMAs.  Between two boundaries a wave runs
        // 2 KW NJ MFMAs (72 for a 9-tap row) with no synchronisation at all.
        for (int stage = 0; stage < ns; ++stage) {         // (stage: local index -- the pair parity starts at 0 for every item)
            const int par = stage & 1;
            a_offsets(tb, ky_n);                              // (ky_n, cc_n): the NEXT stage; the last stage reloads itself into the idle pair
            const bool more = stage + 1 < ns;
#pragma unroll
            for (int kx = 0; kx < KW; ++kx) {
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const int cur = g & 1;
                    if (g + 1 < NG) load_frags(cur ^ 1, par, kx, g + 1);
                    else if (kx + 1 < KW) load_frags(cur ^ 1, par, kx + 1, 0);
                    else {
                        __builtin_amdgcn_sched_barrier(0);
                        if (more) {
                            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // the next stage has landed; this wave's reads of this one too
                            __builtin_amdgcn_s_barrier();                              // ... everyone's
                            load_frags(cur ^ 1, par ^ 1, 0, 0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[cur][i], fb[cur][j], acc[i][j], 0, 0, 0);
                    if (g == 0) {
                        // this step's share of the next stage's LDS-DMA, under the MFMAs: patch piece e at step e (KW - 1) / RG_AV,
                        // weight piece e at step e (KW - 1) / NBW -- nothing in the last step, whose boundary waits for them
#pragma unroll
                        for (int e = 0; e < RG_AV; ++e)
                            if (e * (KW - 1) / RG_AV == kx) dma_a(par ^ 1, cc_n, e);
#pragma unroll
                        for (int e = 0; e < NBW; ++e)
                            if (e * (KW - 1) / NBW == kx) dma_bw(par ^ 1, soff_n, e);
                    }
                    // (conv_ring_bf16's schedule: one MFMA, one fragment read of the NEXT k-substep, a couple of vector / scalar
                    //  instructions and at most one LDS-DMA per group)
                    if (g + 1 < NG || kx + 1 < KW) {
#pragma unroll
                        for (int i = 0; i < 2 * NJ; ++i) {
                            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                            __builtin_amdgcn_sched_group_barrier(0x004, 3, 0);
                            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            soff_c = soff_n;
            if (stage + 2 < ns) { if (++cc_n == nchunks) { cc_n = 0; ++ky_n; } }
            soff_n = stage_soff(ky_n, cc_n);
        }
        rg_wait_vm<0>();
        __syncthreads();                             // every DMA landed, every fragment read done: LDS is free; the next tile's tables are visible
        // ---- the next tile's prologue goes out before this tile's epilogue ----
        if (has_next) start_item(tb ^ 1, nx.nt * BN, nx.s0, nx.s1 - nx.s0);

        if (it.part >= 0) ring_store_tail<F, NJ>(p, t, acc, it.part, m0, M, n0, wm, lane);
        else     // ---- epilogue (scratch: [SC0, TAB0), behind the LDS the next prologue lands in): both row tiles, every column ----
            ring_epilogue<F, 2, NJ, BNB>(p, t, reinterpret_cast<float*>(sm + SC0), reinterpret_cast<float*>(sm + COEF0), acc, it.mt, n0,
                                         wm * 64, 0, wave, rg_opaque(lane), rg_opaque(tid));
        if (!has_next) break;
        k_item = k_n; it = nx;
        tb ^= 1;
    }
#endif  // RG_DEVICE_BODY
}
