// conv_ring_bf16: the bf16 implicit-GEMM core of the stride-1 layers with a k x k window, k >= 3 (round 4).
// (included by conv_igemm.hip after ring_common.h, which holds what this kernel shares with conv_ring2_bf16: the work-item walk,
//  the tables, the LDS-DMA source offsets, the tail-range slab store and the epilogue)
//
// What the round-1 kernels (conv_rowpatch_bf16 / conv_igemm_bf16) left on the table: a k-step of 16 MFMAs between TWO
// workgroup barriers, operands staged global -> registers -> LDS, and three resident workgroups per CU as the only means of
// hiding the barriers, the LDS refill and the fragment-read latency (MFMA pipe 36 % busy).  This kernel is the
// other structure:
//
//   * ONE persistent 512-thread workgroup per CU (8 waves, two per SIMD) walks tiles of 256 consecutive output pixels x BN
//     output channels.  Outside its tap loop a tile costs ~10 us of 40 (tables, the first LDS-DMA round trip, the epilogue's
//     stores -- measured with the loop skipped), and one workgroup per CU has nobody to hide that behind: so the NEXT tile's
//     first patch and weight tiles are requested before the epilogue of the current one starts, and the epilogue writes whole
//     128-byte lines (accumulators transposed through LDS) instead of 2-byte scattered stores.
//   * The row-patch idea is kept: per (filter row, 64-channel slab) -- a STAGE -- the input rows those pixels need, each with
//     its k-1 halo, are staged once; the k taps of the row read that image at a shifted position.
//   * Everything is staged by LDS-DMA (buffer_load_dwordx4 ... lds): no staging registers, no ds_write.  The A patch is
//     double-buffered (2 x 40 KB), the weight tiles (BN x 64 channels per tap) go through a ring of NSLOT slots
//     (8 x 8 KB for BN = 64, 4 x 16 KB for BN = 128): 147 KB of the CU's 160 KB.
//   * ONE raw s_barrier per tap step and counted s_waitcnt vmcnt(N): the pieces of tap t+1 are waited for at the start of step
//     t, become visible to every wave at that step's barrier and are first read one phase later (the read-ahead of step t+1's
//     first fragments, issued under the last MFMAs of step t); the pieces of tap t+1+DP are issued right after the barrier
//     into the slot whose last reader was step t-1 or earlier.  Nothing ever drains to vmcnt(0) inside the loop.
//   * LDS images are row-major 128-byte rows (64 channels) with the 16-byte chunks of a row XOR-permuted by (row >> 1) & 7:
//     a ds_read_b128 fragment read of 16 rows out of any 28 consecutive ones then touches 16 different 16-byte bank slots
//     (conflict-free, also at every tap shift).  An LDS-DMA piece writes 1 KB = 8 rows linearly, so the permutation is applied
//     to the per-lane SOURCE address (same 128-byte line: the global side stays fully coalesced) and again on the read.
//   * BN = 64 (the 9x9 / 64-channel layers): the 8 waves are 4 (pixels) x 2 (halves of the 64-channel slab): every wave keeps
//     a 64 x 64 accumulator tile -- one 16-byte fragment read per MFMA, as a 128 x 128 GEMM tile -- and the two halves meet once,
//     through LDS, in the epilogue.  BN = 128: 4 (pixels) x 2 (64 output channels each).
#pragma once
// Which LDS-DMA pieces a wave issues at which tap step: its BV pieces of the weight tile of step u + 1 + DP at every step, and
// its RG_AV pieces of the NEXT stage's patch at tap steps 0 .. KW-1-DP (they must have landed when the stage's last barrier
// publishes them), spread as evenly as that allows.  (Measured and not kept: the two halves of the workgroup issuing one stream
// each -- vmcnt retires a wave's loads in order, so a weight tile waits for an older patch piece of the same wave -- and the two
// waves of a SIMD issuing at different points of the step: no difference, 1013-1018 TFLOP/s either way.)
template <int KW, int DP>
struct RingSched {
    static constexpr int last = KW - 1 - DP;
    static constexpr int a_cnt(int kx) { return kx <= last ? RG_AV / (last + 1) + (kx < RG_AV % (last + 1) ? 1 : 0) : 0; }
    static constexpr int a_first(int kx) { int n = 0; for (int k = 0; k < kx; ++k) n += a_cnt(k); return n; }
    // loads this thread may still have in flight after the wait at tap step kx: those issued at the DP-1 previous steps
    static constexpr int wait_n(int kx, int bv) {
        int n = 0;
        for (int i = 1; i <= DP - 1; ++i) n += bv + a_cnt(((kx - i) % KW + KW) % KW);
        return n;
    }
};

// BNB: the data-gradient instantiation whose epilogue also emits the producer BatchNorm's backward partials (p.bnb_y; kept out of
// the other instantiations: its 16 running sums cost the 256 x 128 form ~30 spilled registers)
template <int BN, int KW, bool BNB = false>
__global__ __launch_bounds__(512, 2) void conv_ring_bf16(const IgemmParams p) {
#if RG_DEVICE_BODY
    using F = RingForm256<BN>;
    using T = RingTab<F>;
    constexpr int BM = F::BM, ABYTES = F::APOS * F::ROWB;
    constexpr int NSLOT = BN == 64 ? 8 : 4, TILE_B = BN * 128;
    constexpr int DPA = NSLOT - 2 < KW - 1 ? NSLOT - 2 : KW - 1;
    constexpr int DP = DPA < 4 ? DPA : 4;                    // prefetch distance in tap steps (>= 1)
    constexpr int BV = BN / 64;                              // B pieces per wave and step
    constexpr int NG = BN == 64 ? 2 : 4;                     // 16-channel k-substeps per wave and step
    using S = RingSched<KW, DP>;
    static_assert(DP >= 1 && S::last >= 0, "schedule");
    // LDS map: [A buffer 0 | weight ring | A buffer 1 | two table sets].  The next tile's prologue lands in A buffer 0 and ring
    // slots 0 .. DP; what is behind them (64 KB: the last ring slots and A buffer 1) is the epilogue's scratch meanwhile.
    constexpr int A0 = 0, B0 = ABYTES, A1 = B0 + NSLOT * TILE_B, TAB0 = A1 + ABYTES;
    constexpr int SC0 = B0 + (DP + 1) * TILE_B;              // epilogue scratch: [SC0, TAB0)
    static_assert(TAB0 - SC0 >= 34 * 1024 && T::N * 4 <= 1600, "LDS map");
    // ONE shared object: the compiler must see a single LDS array beside the LDS-DMA instructions
    constexpr int COEF0 = TAB0 + 2 * 1600 + 64;              // [4][BN] floats: the BatchNorm coefficients of a data gradient's bnb mode
    __shared__ __attribute__((aligned(16))) unsigned char sm[COEF0 + 4 * 128 * 4];
    int* const wirow = reinterpret_cast<int*>(sm + TAB0 + 2 * 1600);      // [RG_KMAX] weight index of the first tap of each filter row
    auto tab = [&](int b) { return reinterpret_cast<int*>(sm + TAB0 + b * 1600); };

    const int knobs = p.kc;                                  // measurement knobs (0 in production)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 3, wz = wave >> 2;
    const IgemmPhase ph = p.ph[0];
    const int M = p.B * ph.Ho * ph.Wo;
    const int kh = (ph.tap_end - ph.tap_begin) / KW;
    // taps of a filter row are consecutive in the weight tensor and in dx (ring_kw() checked it): ascending dx for a forward
    // convolution, descending for a data gradient -- no per-tap table is read inside the loop (a kernarg table indexed at run
    // time becomes a vector-memory load, whose wait would drain the LDS-DMA pipeline)
    const int dx_first = p.tdx[ph.tap_begin], dx_last = p.tdx[ph.tap_begin + KW - 1];
    const int dxmin = min(dx_first, dx_last);
    const bool dx_up = dx_last >= dx_first;
    const int nchunks = p.Cred / F::SLAB;
    const int tap2 = p.w_tap_stride * 2;
    const RingWalk walk(p, knobs, kh * nchunks);
    // ---- per-tile state ----
    unsigned pk[RG_AV];             // patch piece e of this wave (8 positions x 8 chunks): ring_tile_sources
    unsigned boff[BV];           // weight-tile piece e of this wave = piece e * 8 + wave of the tile's 8 BV (8 rows x 8 chunks)
    unsigned a_vo[RG_AV];           // per-lane source offsets of the patch pieces of one stage
    __amdgpu_buffer_rsrc_t rs_x;
    // (p.kc carries measurement knobs for this kernel: bit 1 / bit 2 give the weight / activation descriptor zero records, so
    //  the range check drops every LDS-DMA through it while the instruction stream, the waits and the barriers stay: what the
    //  loop costs without that operand's traffic.  Timing only -- the results are wrong.)
    __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, (knobs & 2) ? 0 : (int)p.w_bytes, 0x00020000);

    auto tile_dma_state = [&](int b, int n0) {      // pk / boff / the activation descriptor of the tile whose tables are set b
        rs_x = ring_tile_sources<F>(tab(b), p, dxmin, knobs, wave, lane, pk);
#pragma unroll
        for (int e = 0; e < BV; ++e) boff[e] = ring_w_offset<F>(p, n0, ring_piece_row<F>(e * 8 + wave, lane), lane);
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
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (rg_lds_ptr)(sm + (par ? A1 : A0) + (e * 8 + wave) * 1024), 16, a_vo[e], cc * 128, 0, 0);
    };
    auto dma_b = [&](int v, int soff) {                      // this wave's pieces of the weight tile at scalar offset soff -> ring slot v % NSLOT
        const int slot = v & (NSLOT - 1);
#pragma unroll
        for (int e = 0; e < BV; ++e)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (rg_lds_ptr)(sm + B0 + slot * TILE_B + (e * 8 + wave) * 1024), 16, boff[e], soff, 0, 0);
    };
    // The weight tile of tap step v = stage * KW + kx lies at scalar offset soff(stage) + kx * tap2: with KW unrolled, the
    // tile that step (stage, kx) prefetches -- step v + 1 + DP -- is tap (kx + 1 + DP) % KW of this stage or of the next one
    // (DP < KW), so two scalars per stage replace all per-step bookkeeping.  Past the last step the "next" stage is the last
    // stage again: harmless reloads into free slots keep the number of loads per step -- what the counted waits rely on -- fixed.
    auto stage_soff = [&](int ky_, int cc_) { return __builtin_amdgcn_readfirstlane(wirow[ky_]) * tap2 + cc_ * F::ROWB; };
    int ky_n = 0, cc_n = 0, soff_c = 0, soff_n = 0;
    // (measured and not kept: every workgroup starting at another filter row, so that the workgroups of an XCD read different
    //  weight tiles at any moment: 1049 vs 1100 TFLOP/s -- sharing the lines helps)
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
        for (int v = 0; v <= DP; ++v) dma_b(v, (v < KW ? soff_c : soff_n) + (v % KW) * tap2);
    };
    // ---- fragment addressing ----
    const unsigned hbit = (unsigned)(lane >> 5) << 6;                 // chunk 4h of the slab: lane half h owns channels [32h, 32h+32)
    const int ncol0 = BN == 64 ? 0 : wz * 64;                         // first output channel of this wave's column tiles
    unsigned bfix[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const unsigned n = (unsigned)(ncol0 + j * 32 + (lane & 31));
        bfix[j] = ((n << 7) ^ (((n >> 1) & 7u) << 4)) ^ hbit;
    }
    const int g_first = BN == 64 ? 2 * wz : 0;
    unsigned apos[2];                                // ring_tile_begin
    f32x16 acc[2][2];
    bf16x8 fa[2][2], fb[2][2];                       // [register set][row tile / column tile]
    auto load_frags = [&](int set, int par, int kx, int slot, int g) {     // fragments of (A buffer par, tap kx, ring slot, k-substep g)
        const unsigned sh = (unsigned)(dx_up ? kx : KW - 1 - kx);
        const unsigned abase = (unsigned)(par ? A1 : A0);
        const unsigned bbase = (unsigned)(B0 + slot * TILE_B);
        const unsigned gx = (unsigned)(g_first + g) << 4;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const unsigned q = apos[i] + sh;
            const unsigned a = abase + (((q << 7) ^ (((q >> 1) & 7u) << 4)) ^ hbit ^ gx);
            fa[set][i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const f32x4*>(sm + a));
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
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
        if (ns > 0) load_frags(0, 0, 0, 0, 0);

        for (int stage = 0; stage < ns; ++stage) {         // (stage: local index -- buffer parity and ring slots start at 0 for every item)
            const int par = stage & 1;
            const int ubase = stage * KW;
            a_offsets(tb, ky_n);                              // (ky_n, cc_n): the NEXT stage; the last stage reloads itself into the idle buffer
#pragma unroll
            for (int kx = 0; kx < KW; ++kx) {
                // pieces issued DP or more steps ago have landed (this thread's); the barrier makes everyone's visible and says
                // that every wave has finished the LDS reads of step u-1
                switch (kx) {
                    case 0: rg_wait_vm<S::wait_n(0, BV)>(); break;
                    case 1: rg_wait_vm<S::wait_n(1, BV)>(); break;
                    case 2: rg_wait_vm<S::wait_n(2, BV)>(); break;
                    case 3: rg_wait_vm<S::wait_n(3 % KW, BV)>(); break;
                    case 4: rg_wait_vm<S::wait_n(4 % KW, BV)>(); break;
                    case 5: rg_wait_vm<S::wait_n(5 % KW, BV)>(); break;
                    case 6: rg_wait_vm<S::wait_n(6 % KW, BV)>(); break;
                    case 7: rg_wait_vm<S::wait_n(7 % KW, BV)>(); break;
                    default: rg_wait_vm<S::wait_n(8 % KW, BV)>(); break;
                }
                __builtin_amdgcn_s_barrier();
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const int cur = g & 1;
                    // read-ahead: the next k-substep's fragments -- of the NEXT step under this step's last MFMAs
                    if (g + 1 < NG) load_frags(cur ^ 1, par, kx, (ubase + kx) & (NSLOT - 1), g + 1);
                    else if (stage + 1 < ns || kx + 1 < KW)
                        load_frags(cur ^ 1, kx + 1 < KW ? par : par ^ 1, kx + 1 < KW ? kx + 1 : 0, (ubase + kx + 1) & (NSLOT - 1), 0);
                    // (measured and not kept: the same operands through v_mfma_f32_16x16x32_bf16 -- 1080 vs 1092-1098 TFLOP/s)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[cur][i], fb[cur][j], acc[i][j], 0, 0, 0);
                    if (g == 0) {
                        // this step's LDS-DMA issue sits UNDER the MFMAs (whose operands the read-ahead already delivered):
                        // straight after the barrier the matrix pipe would idle while every wave issues its pieces
                        const int vb = kx + 1 + DP;                // compile-time after unrolling
                        dma_b(ubase + vb, (vb < KW ? soff_c : soff_n) + (vb % KW) * tap2);
#pragma unroll
                        for (int e = 0; e < RG_AV; ++e)
                            if (e >= S::a_first(kx) && e < S::a_first(kx) + S::a_cnt(kx)) dma_a(par ^ 1, cc_n, e);
                    }
                    // Round 5 (the schedule wgrad_ring.h arrived at): one MFMA, one fragment read of the NEXT k-substep, a
                    // couple of vector / scalar instructions and at most one LDS-DMA, four times -- instead of the blocks
                    // [4 reads][4 MFMAs][DMA] the scheduler was pinned to before, in which every read waited for issue behind the
                    // block in front of it
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                        __builtin_amdgcn_sched_group_barrier(0x004, 3, 0);
                        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
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

        if (it.part >= 0) ring_store_tail<F, 2>(p, t, acc, BN == 64 ? it.part * 2 + wz : it.part, m0, M, n0 + ncol0, wm, lane);
        else {
            // ---- epilogue (scratch: [SC0, TAB0), behind the LDS the next prologue lands in) ----
            const int lane_e = rg_opaque(lane), tid_e = rg_opaque(tid);
            float* const sc = reinterpret_cast<float*>(sm + SC0);
            if constexpr (BN == 64) {
                // the two halves of the reduction meet: wave (wm, wz) hands row tile 1-wz to its partner and finalises row tile wz
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        sc[wave * 2048 + (j * 16 + r) * 64 + lane_e] = wz == 0 ? acc[1][j][r] : acc[0][j][r];
                __syncthreads();
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float o = sc[(wave ^ 4) * 2048 + (j * 16 + r) * 64 + lane_e];
                        if (wz == 0) acc[0][j][r] += o; else acc[0][j][r] = acc[1][j][r] + o;
                    }
                __syncthreads();
            }
            // BN = 64: one row tile (wz) of all 64 columns; BN = 128: both row tiles of column half wz
            ring_epilogue<F, BN == 64 ? 1 : 2, 2, BNB>(p, t, sc, reinterpret_cast<float*>(sm + COEF0), acc, it.mt, n0,
                                                       BN == 64 ? wm * 64 + wz * 32 : wm * 64, ncol0, wave, lane_e, tid_e);
        }
        if (!has_next) break;
        k_item = k_n; it = nx;
        tb ^= 1;
    }
#endif  // RG_DEVICE_BODY
}
