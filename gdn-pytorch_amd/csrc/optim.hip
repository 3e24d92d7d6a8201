// The optimizer of the GDN hot path for gfx950: fused Adam / AdamW (host scalars, capturable, segmented), the gradient guard,
// weight EMA with the exchange and the accumulation sum, the learning-rate schedule, the step record and the per-tensor norms.
// All stream at HBM speed over float32 ranges: 16 bytes per lane where the bases allow, grid-stride, no atomics.
#include <type_traits>

#include "common.h"

namespace {

// ------------------------------------------------------------------------ Adam
// Capturable Adam: the step counter and the running powers beta^t live in device memory, so a captured training step
// advances them on every replay.  state = { double beta1^t, double beta2^t, int32 t, float bc1, float bc2s }.
struct AdamDevState { double p1, p2; int step; float bc1, bc2s; };
static_assert(sizeof(AdamDevState) == 32, "the step-state table is G x 32 bytes (include/gdn_hip.h)");
// The gradient guard's record (below; include/gdn_hip.h): every capturable kernel takes one, or null for an unguarded update.
struct AdamGuard { double sumsq; float norm, coef; int skip, steps, clipped, skipped; };
static_assert(sizeof(AdamGuard) == 32, "guard record layout is part of the C ABI");
// A skipped step: the kernel that asks returns before it reads or writes anything.
__device__ __forceinline__ bool guard_skips(const AdamGuard* guard) { return guard != nullptr && guard->skip != 0; }
__device__ __forceinline__ void adam_advance(AdamDevState* st, const float* __restrict__ hyper) {
    st->step += 1;
    st->p1 *= (double)hyper[1];
    st->p2 *= (double)hyper[2];
    st->bc1 = (float)(1.0 - st->p1);
    st->bc2s = (float)sqrt(1.0 - st->p2);
}
// The prep launch of every capturable update: lane k advances the step state of row k of a G-row table (G = 1: the one state
// of gdn_adam_step_dev[_guarded], of which only the 28 bytes before the tail padding are touched).
__global__ __launch_bounds__(256) void adam_prep_kernel(AdamDevState* states, const float* __restrict__ hyper, int G,
                                                        const AdamGuard* guard) {
    if (guard_skips(guard)) return;                      // a skipped step takes no place in any row's bias corrections
    const int k = (int)threadIdx.x;
    if (k < G) adam_advance(states + k, hyper + 6 * k);
}
inline dim3 adam_prep_block(int G) { return dim3(G <= 64 ? 64 : 256); }       // one wave where it holds every row

// The scalars of one update: `step` = lr / bc1, `gscale` the gradient's scale (grad_scale, times the guard's coefficient under a
// guard), `decay` the weight decay wd of the coupled form or dec of the decoupled one.
// dec = (float)((double)lr * (double)wd): the double product of two floats is exact (48 bits), so its one rounding to float IS
// the IEEE float product -- written as that, which keeps double-rate instructions out of a loop that streams at HBM speed.
__device__ __forceinline__ float adamw_dec(float lr, float wd) { return lr * wd; }
struct AdamScalars { float step, b1, b2, eps, decay, bc2s, gscale; };
template <bool DECOUPLED>
__device__ __forceinline__ AdamScalars adam_scalars(float lr, float b1, float b2, float eps, float wd, float bc1, float bc2s,
                                                    float gscale) {
    return AdamScalars{lr / bc1, b1, b2, eps, DECOUPLED ? adamw_dec(lr, wd) : wd, bc2s, gscale};
}
// the same from a hyper row (lr, beta1, beta2, eps, wd, grad_scale), its step state and the guard (or null)
template <bool DECOUPLED>
__device__ __forceinline__ AdamScalars adam_scalars(const float* __restrict__ h, const AdamDevState* st, const AdamGuard* guard) {
    return adam_scalars<DECOUPLED>(h[0], h[1], h[2], h[3], h[4], st->bc1, st->bc2s, guard != nullptr ? h[5] * guard->coef : h[5]);
}
// The one element every update kernel goes through, so the bits of all entry points agree whatever the compiler would contract
// in a scalar or a four-wide body: every product, sum, quotient and root is rounded on its own but the one fma.
//   coupled (torch.optim.Adam): g += wd*p; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps),
//     the weight decay fused into the scaled gradient, fma(wd, p, g * gscale).
//   decoupled (AdamW): the gradient carries no decay term, so the moments never see it; the decay dec * p is
//     added to the Adam term q and the sum is subtracted from the weight ONCE: p (1 - lr wd) in float32 loses the decay
//     altogether at this project's rates (1 - 1e-8 rounds to 1).  With dec = 0 it is the coupled element at wd = 0.
template <bool DECOUPLED>
__device__ __forceinline__ void adam_update1(float& p, float g, float& m, float& v, const AdamScalars& s) {
#pragma clang fp contract(off)
    const float pi = p;
    const float gi = DECOUPLED ? g * s.gscale : fmaf(s.decay, pi, g * s.gscale);
    const float mi = s.b1 * m + (1.f - s.b1) * gi;
    const float vi = s.b2 * v + (1.f - s.b2) * gi * gi;
    m = mi; v = vi;
    const float q = s.step * mi / (sqrtf(vi) / s.bc2s + s.eps);
    p = DECOUPLED ? pi - fmaf(s.decay, pi, q) : pi - q;
}
// a scalar grid-stride loop over any start and n
template <bool DECOUPLED>
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, int64_t n, const AdamScalars& s) {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float pi = p[i], mi = m[i], vi = v[i];
        adam_update1<DECOUPLED>(pi, g[i], mi, vi, s);
        m[i] = mi; v[i] = vi;
        p[i] = pi;
    }
}
template <bool DECOUPLED>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                   float b1, float b2, float eps, float wd, float bc1, float bc2s,
                                                   float gscale) {
    adam_update<DECOUPLED>(p, g, m, v, n, adam_scalars<DECOUPLED>(lr, b1, b2, eps, wd, bc1, bc2s, gscale));
}
// The capturable update of a contiguous range.
template <bool DECOUPLED>
__global__ __launch_bounds__(256) void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                       const float* __restrict__ hyper, const AdamDevState* st,
                                                       const AdamGuard* guard) {
    if (guard_skips(guard)) return;                      // p, m, v are neither read nor written: a skipped step does not decay
    adam_update<DECOUPLED>(p, g, m, v, n, adam_scalars<DECOUPLED>(hyper, st, guard));
}

// ---- gradient guard: global gradient norm, clipping coefficient and the decision to skip a non-finite step, all in device
// memory (capturable; no host read).  The record (include/gdn_hip.h) is written with ordinary stores by single threads.

// blocks of the partial-sum launch: a function of n alone, so the order of every addition is too
constexpr int GRADNORM_MAX_BLOCKS = 1024;
inline int gradnorm_blocks(int64_t n) { return stream_blocks(cdiv64(n, 16), 256, GRADNORM_MAX_BLOCKS); }

__device__ __forceinline__ double sq4_d(f32x4 a) {
    const double x = (double)a.x, y = (double)a.y, z = (double)a.z, w = (double)a.w;       // 1e30f squared fits a double
    return (x * x + y * y) + (z * z + w * w);
}
// The head/body/tail split of `n` floats starting at `base`.
struct StreamSplit { int64_t head, nvec, tail0; };
__device__ __forceinline__ StreamSplit stream_split(const void* base, int64_t n) {
    StreamSplit s;
    s.head = (int64_t)((4u - (unsigned)(((uintptr_t)base >> 2) & 3u)) & 3u);
    if (s.head > n) s.head = n;
    s.nvec = (n - s.head) >> 2;
    s.tail0 = s.head + s.nvec * 4;
    return s;
}
// stage 1: partial[b] = sum of squares of block b's share.  Up to 3 head elements bring the body to a 16-byte boundary
// (ar.grad[o:o+n] slices and loose parameters start anywhere); the body is read as float4, 4 loads in flight per lane;
// head and tail (< 4 elements each) go to lanes of block 0.  Per-lane partials -> xor-butterfly over the 64 lanes -> the
// block's 4 waves through LDS -> one double per block: no atomics, no ticket, the same additions in the same order every run.
__global__ __launch_bounds__(256) void adam_gradnorm_partial_kernel(const float* __restrict__ g, int64_t n,
                                                                   double* __restrict__ partial) {
    __shared__ double sh[4];
    const StreamSplit sp = stream_split(g, n);
    const int64_t head = sp.head, nvec = sp.nvec, tail0 = sp.tail0;
    const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g + head);
    const int64_t T = (int64_t)gridDim.x * 256;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int64_t i = blockIdx.x * 256ll + threadIdx.x;
    for (; i + 3 * T < nvec; i += 4 * T) {
        const f32x4 x0 = gv[i], x1 = gv[i + T], x2 = gv[i + 2 * T], x3 = gv[i + 3 * T];
        a0 += sq4_d(x0); a1 += sq4_d(x1); a2 += sq4_d(x2); a3 += sq4_d(x3);
    }
    for (; i < nvec; i += T) a0 += sq4_d(gv[i]);
    if (blockIdx.x == 0) {
        const int64_t t = threadIdx.x;
        if (t < head) { const double x = (double)g[t]; a1 += x * x; }
        if (t >= 64 && tail0 + (t - 64) < n) { const double x = (double)g[tail0 + (t - 64)]; a2 += x * x; }
    }
    const double s = block_sum_d256((a0 + a1) + (a2 + a3), sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// stage 2 (one block): lane t adds partial[t], partial[t + 256], ... in index order, then the same block reduction
__global__ __launch_bounds__(256) void adam_gradnorm_final_kernel(const double* __restrict__ partial, int nb, AdamGuard* guard,
                                                                 int accumulate) {
    __shared__ double sh[4];
    double a = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) a += partial[i];
    const double s = block_sum_d256(a, sh);
    if (threadIdx.x == 0) guard->sumsq = accumulate ? guard->sumsq + s : s;
}
// the decision: norm of the gradient as Adam sees it (after grad_scale), torch.nn.utils.clip_grad_norm_'s coefficient, skip
__global__ void adam_guard_finalize_kernel(AdamGuard* guard, const float* __restrict__ hyper, double max_norm, int skip_nonfinite) {
    const double norm = sqrt(guard->sumsq) * fabs((double)hyper[5]);
    const bool finite = isfinite(norm);
    double coef = 1.0;
    int skip = 0;
    if (finite) {
        if (max_norm > 0.0) coef = fmin(1.0, max_norm / (norm + 1e-6));
    } else if (skip_nonfinite) {
        skip = 1;
        coef = 0.0;
    }
    const float coef32 = (float)coef;
    guard->norm = (float)norm;
    guard->coef = coef32;
    guard->skip = skip;
    guard->steps += 1;
    if (coef32 < 1.f && !skip) guard->clipped += 1;
    guard->skipped += skip;
}

// ---- weight EMA, the in-place exchange of two float ranges and the gradient-accumulation sum (include/gdn_hip.h): three element
// operations on one streaming skeleton over two ranges a and b.  The body moves 16 bytes per lane, up to 3 head elements bring it
// to a 16-byte boundary of `a` and fewer than 4 tail elements follow it (lanes of block 0, as in adam_gradnorm_partial_kernel);
// VEC = false is the scalar form for operands whose bases differ modulo 16.  No atomics, no LDS.  An Op has
//     B              float, or const float where `b` is only read (then nothing is stored there)
//     begin()        once per thread before anything is read; false: the launch reads and writes nothing
//     op(a, b)       the element operation, on copies of a[i] and b[i] that go back afterwards
template <bool VEC, class Op>
__global__ __launch_bounds__(256) void stream2_kernel(float* __restrict__ a, typename Op::B* __restrict__ b, int64_t n, Op op) {
    constexpr bool WRITES_B = !std::is_const<typename Op::B>::value;
    using B4 = typename std::conditional<WRITES_B, f32x4, const f32x4>::type;
    if (!op.begin()) return;
    const auto one = [&](int64_t i) {
        float x = a[i], y = b[i];
        op(x, y);
        a[i] = x;
        if constexpr (WRITES_B) b[i] = y;
    };
    const int64_t T = (int64_t)gridDim.x * 256, tid = blockIdx.x * 256ll + threadIdx.x;
    if (!VEC) {
        for (int64_t i = tid; i < n; i += T) one(i);
        return;
    }
    const StreamSplit s = stream_split(a, n);
    f32x4* __restrict__ av = reinterpret_cast<f32x4*>(a + s.head);
    B4* __restrict__ bv = reinterpret_cast<B4*>(b + s.head);
    for (int64_t i = tid; i < s.nvec; i += T) {
        const f32x4 y4 = bv[i], x4 = av[i];
        float x[4] = {x4.x, x4.y, x4.z, x4.w}, y[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) op(x[e], y[e]);
        av[i] = f32x4{x[0], x[1], x[2], x[3]};
        if constexpr (WRITES_B) bv[i] = f32x4{y[0], y[1], y[2], y[3]};
    }
    if (blockIdx.x == 0) {
        const int64_t l = threadIdx.x;
        if (l < s.head) one(l);
        if (l >= 64 && s.tail0 + (l - 64) < n) one(s.tail0 + (l - 64));
    }
}
__device__ __forceinline__ float ema1(float w, float p, float e) { return fmaf(w, p - e, e); }
// the warm-up weight w_t = 1 - min(decay, (1 + t) / (10 + t)) after t updates, in double, rounded once
__device__ __forceinline__ float ema_weight(double decay, int step) {
    const double t = (double)step;
    return (float)(1.0 - fmin(decay, (1.0 + t) / (10.0 + t)));
}
// e += w_t (p - e), t = the step count the Adam update of this store has just advanced; every thread computes w_t itself.
// A skipped step (guard->skip) reads and writes nothing.
struct EmaOp {
    using B = const float;
    double decay; const AdamDevState* st; const AdamGuard* guard; float w;
    __device__ bool begin() {
        if (guard_skips(guard)) return false;
        w = ema_weight(decay, st->step);
        return true;
    }
    __device__ void operator()(float& e, float p) const { e = ema1(w, p, e); }
};
struct SwapOp {
    using B = float;
    __device__ bool begin() { return true; }
    __device__ void operator()(float& a, float& b) const { const float x = a; a = b; b = x; }
};
// acc[i] = acc[i] + g[i]: one IEEE float32 add per element (nothing to contract into an FMA, subnormals kept), the sum of a
// gradient-accumulation group.  `g` is only read.
struct AccumulateOp {
    using B = const float;
    __device__ bool begin() { return true; }
    __device__ void operator()(float& acc, float g) const { acc = acc + g; }
};
// one lane per 16 bytes (VEC) or per float, capped like the Adam update's grid; the rest is grid-strided
inline int stream_rw_blocks(int64_t n, bool vec) { return stream_blocks(vec ? cdiv64(n, 4) : n, 256, 4096); }
// stream2_kernel in the form the two bases allow: VEC where they sit at the same offset within 16 bytes
template <class Op>
inline void stream2_launch(float* a, typename Op::B* b, int64_t n, Op op, void* stream) {
    const bool vec = (((uintptr_t)a ^ (uintptr_t)b) & 15) == 0;
    const auto kernel = vec ? stream2_kernel<true, Op> : stream2_kernel<false, Op>;
    hipLaunchKernelGGL(kernel, dim3(stream_rw_blocks(n, vec)), dim3(256), 0, ST(stream), a, b, n, op);
}

// ---- segmented forms (include/gdn_hip.h): one launch over an arena whose 64-float chunks belong to parameter groups.  map[c] is
// the group of chunk c or SEG_SKIP.  A lane moves 16 bytes, so the 16 lanes l, l+1, ... l+15 (l % 16 == 0) of a wave share one
// chunk in every trip of the grid-stride loop (the stride is a multiple of 256 and n of 64, so such a lane group is inside the
// arena or outside it as a whole): its first lane reads the map byte and the others take it from that lane.  No atomics, no LDS.
constexpr int SEG_SKIP = 0xFF;
__device__ __forceinline__ int seg_group(const uint8_t* __restrict__ map, int64_t i, bool inside) {
    const int lane = (int)(threadIdx.x & 63u);
    int k = SEG_SKIP;
    if (inside && (lane & 15) == 0) k = (int)map[i >> 4];
    return __shfl(k, lane & ~15);
}
// adam_dev_kernel per chunk, four elements per lane, with the scalars of the chunk's own group
// (tests/test_hip_seg_adam.py and tests/test_hip_adamw.py hold the two forms to bit identity)
template <bool DECOUPLED>
__global__ __launch_bounds__(256) void adam_seg_kernel(f32x4* __restrict__ p, const f32x4* __restrict__ g, f32x4* __restrict__ m,
                                                       f32x4* __restrict__ v, int64_t nvec, const uint8_t* __restrict__ map,
                                                       const float* __restrict__ hyper, const AdamDevState* __restrict__ states,
                                                       const AdamGuard* guard) {
    if (guard_skips(guard)) return;                      // p, m, v are neither read nor written
    const int64_t T = (int64_t)gridDim.x * 256;
    for (int64_t i0 = blockIdx.x * 256ll; i0 < nvec; i0 += T) {      // (block-uniform bound: every lane reaches the shuffle)
        const int64_t i = i0 + threadIdx.x;
        const int k = seg_group(map, i, i < nvec);
        if (k == SEG_SKIP) continue;
        const AdamScalars s = adam_scalars<DECOUPLED>(hyper + 6 * k, states + k, guard);
        const f32x4 gi = g[i];
        const f32x4 p4 = p[i], m4 = m[i], v4 = v[i];
        float pe[4] = {p4.x, p4.y, p4.z, p4.w}, me[4] = {m4.x, m4.y, m4.z, m4.w}, ve[4] = {v4.x, v4.y, v4.z, v4.w};
        const float ge[4] = {gi.x, gi.y, gi.z, gi.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) adam_update1<DECOUPLED>(pe[e], ge[e], me[e], ve[e], s);
        m[i] = f32x4{me[0], me[1], me[2], me[3]};
        v[i] = f32x4{ve[0], ve[1], ve[2], ve[3]};
        p[i] = f32x4{pe[0], pe[1], pe[2], pe[3]};
    }
}
// stage 1 of gdn_grad_sumsq_seg: adam_gradnorm_partial_kernel over the chunks that are not skipped (a skipped chunk is not
// read, so a NaN there stays out of the sum); the same grid, the same per-lane partials and the same block reduction.
__global__ __launch_bounds__(256) void adam_gradnorm_seg_partial_kernel(const f32x4* __restrict__ gv, int64_t nvec,
                                                                  const uint8_t* __restrict__ map, double* __restrict__ partial) {
    __shared__ double sh[4];
    const int64_t T = (int64_t)gridDim.x * 256;
    double a0 = 0.0, a1 = 0.0;
    for (int64_t i0 = blockIdx.x * 256ll; i0 < nvec; i0 += 2 * T) {
        const int64_t i = i0 + threadIdx.x, j = i + T;
        const int k0 = seg_group(map, i, i < nvec), k1 = seg_group(map, j, j < nvec);
        f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = {0.f, 0.f, 0.f, 0.f};
        if (k0 != SEG_SKIP) x0 = gv[i];
        if (k1 != SEG_SKIP) x1 = gv[j];
        a0 += sq4_d(x0); a1 += sq4_d(x1);
    }
    const double s = block_sum_d256(a0 + a1, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// EmaOp per chunk: the warm-up weight comes from the step count of the chunk's own group
__global__ __launch_bounds__(256) void ema_update_seg_kernel(f32x4* __restrict__ ev, const f32x4* __restrict__ pv, int64_t nvec,
                                                      const uint8_t* __restrict__ map, double decay,
                                                      const AdamDevState* __restrict__ states, const AdamGuard* guard) {
    if (guard_skips(guard)) return;
    const int64_t T = (int64_t)gridDim.x * 256;
    for (int64_t i0 = blockIdx.x * 256ll; i0 < nvec; i0 += T) {
        const int64_t i = i0 + threadIdx.x;
        const int k = seg_group(map, i, i < nvec);
        if (k == SEG_SKIP) continue;
        const float w = ema_weight(decay, states[k].step);
        const f32x4 x = pv[i];
        f32x4 a = ev[i];
        a.x = ema1(w, x.x, a.x); a.y = ema1(w, x.y, a.y); a.z = ema1(w, x.z, a.z); a.w = ema1(w, x.w, a.w);
        ev[i] = a;
    }
}

// ---- learning-rate schedule on the device (include/gdn_hip.h): lane k turns the update count of group k into the rate of the
// update about to run, hyper[k][0] = (float)(base_lr[k] * s(u)).  Contraction is off for the whole function and the division is
// the IEEE one, so warm-up, the linear decay and the final product are the host's plain double arithmetic bit for bit; only
// cos() is the device library's.  Ordinary loads and stores, no LDS, no atomics; lanes >= G do nothing.
__global__ __launch_bounds__(256) void lr_schedule_kernel(float* __restrict__ hyper, const double* __restrict__ base_lr,
                                                          const AdamDevState* __restrict__ states, int G, int kind, int warmup,
                                                          int total, double floor) {
#pragma clang fp contract(off)
    const int k = (int)threadIdx.x;
    if (k >= G) return;
    const double u = (double)states[k].step;
    double s = 1.0;
    if (u < (double)warmup) {
        s = __ddiv_rn(u + 1.0, (double)warmup);
    } else if (kind != 0) {
        const int span = total - warmup > 1 ? total - warmup : 1;
        const double x = fmin(1.0, __ddiv_rn(u - (double)warmup, (double)span));
        const double shape = kind == 1 ? 1.0 - x : 0.5 * (1.0 + cos(3.141592653589793 * x));
        s = floor + (1.0 - floor) * shape;
    }
    hyper[6 * k] = (float)(base_lr[k] * s);
}

// ---- per-step training record kept on the device (include/gdn_hip.h): one wave writes row count % cap of a
// ring of 64-byte rows from records that already sit in device memory, then advances the counter.  Lane j < 16 stores dword j
// of the row; floats travel as bit patterns (a NaN keeps its payload, -0 its sign).  The term pointers ride in the argument
// block.  Ordinary loads and stores, no atomics: calls on one stream are ordered.
struct StepRecordTerms { const float* p[8]; };
constexpr unsigned STEP_RECORD_QNAN = 0x7fc00000u;
__global__ __launch_bounds__(64) void step_record_kernel(unsigned long long* __restrict__ ring, int cap, StepRecordTerms terms,
                                                         int n_terms, const float* __restrict__ hyper, const AdamDevState* st,
                                                         const AdamGuard* guard) {
    const int l = (int)threadIdx.x;
    const unsigned long long count = ring[0];
    unsigned* __restrict__ row = reinterpret_cast<unsigned*>(ring + 8 + 8 * (count % (unsigned long long)cap));
    if (l < 16) {
        unsigned v = STEP_RECORD_QNAN;
        if (l == 0) v = (unsigned)count;
        else if (l == 1) v = (unsigned)(count >> 32);
        else if (l == 2) v = st != nullptr ? (unsigned)st->step : 0xffffffffu;
        else if (l == 3) v = guard != nullptr ? (unsigned)guard->skip : 0xffffffffu;
        else if (l == 4) { if (hyper != nullptr) v = __float_as_uint(hyper[0]); }
        else if (l == 5) { if (guard != nullptr) v = __float_as_uint(guard->norm); }
        else if (l == 6) { if (guard != nullptr) v = __float_as_uint(guard->coef); }
        else if (l == 7) v = (unsigned)n_terms;
        else {
            const float* src = nullptr;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (l == 8 + j && j < n_terms) src = terms.p[j];
            if (src != nullptr) v = *reinterpret_cast<const unsigned*>(src);
        }
        row[l] = v;
    }
    __syncthreads();       // every lane has read the counter and written its dword
    if (l == 0) ring[0] = count + 1ull;
}

// ---- per-tensor sums of squares of the weights and the gradient over an arena's slices (include/gdn_hip.h).
// Work items are (segment, slab of TSS_SLAB floats): tss_items_kernel turns the segment table into first[k], the index of
// segment k's first item (first[T]: the number of items); tss_partial_kernel is one workgroup per item -- it finds its segment
// by bisection of `first`, streams its slab of p (and g) as float4 with four loads in flight per array, and leaves one double
// pair; tss_final_kernel is one workgroup per segment adding its items in index order.  Slabs start at multiples of 64 floats
// from 16-byte aligned bases, so only a segment's last slab has a scalar tail (< 4 floats), and nothing outside
// [offset, offset + length) is read.  No atomics; every addition has a fixed place.  A table entry that leaves [0, n) is cut to
// it (the table's contents are the caller's, an out-of-range read is not).
constexpr int64_t TSS_SLAB = 16384;
__device__ __forceinline__ void tss_segment(const int64_t* __restrict__ seg, int k, int64_t n, int64_t& off, int64_t& len) {
    off = seg[2 * k];
    len = seg[2 * k + 1];
    if (off < 0 || off >= n || len < 0) { off = 0; len = 0; }
    if (len > n - off) len = n - off;
}
__global__ __launch_bounds__(256) void tss_items_kernel(const int64_t* __restrict__ seg, int T, int64_t n,
                                                        int64_t* __restrict__ first) {
    __shared__ int64_t sh[256];
    int64_t carry = 0;
    for (int k0 = 0; k0 < T; k0 += 256) {        // (block-uniform bound: every thread reaches the barriers)
        const int k = k0 + (int)threadIdx.x;
        int64_t items = 0;
        if (k < T) {
            int64_t off, len;
            tss_segment(seg, k, n, off, len);
            items = cdiv64(len, TSS_SLAB);
        }
        sh[threadIdx.x] = items;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {      // inclusive scan
            const int64_t add = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (k < T) first[k] = carry + sh[threadIdx.x] - items;
        carry += sh[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) first[T] = carry;
}
__device__ __forceinline__ double sq1_d(float a) { const double x = (double)a; return x * x; }
__global__ __launch_bounds__(256) void tss_partial_kernel(const float* __restrict__ p, const float* __restrict__ g, int64_t n,
                                                          const int64_t* __restrict__ seg, int T,
                                                          const int64_t* __restrict__ first, double* __restrict__ partial) {
    __shared__ double sh[8];
    const int64_t item = blockIdx.x;
    if (item >= first[T]) return;                // (block-uniform)
    int lo = 0, hi = T;                          // the segment k with first[k] <= item < first[k + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= item) lo = mid; else hi = mid;
    }
    int64_t off, len;
    tss_segment(seg, lo, n, off, len);
    const int64_t s0 = (item - first[lo]) * TSS_SLAB;
    const int64_t cnt = len - s0 < TSS_SLAB ? len - s0 : TSS_SLAB;      // 1 .. TSS_SLAB floats of this slab
    const int nv = (int)(cnt >> 2), tail = (int)(cnt & 3);
    const int t = (int)threadIdx.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    const f32x4* __restrict__ pv = reinterpret_cast<const f32x4*>(p + off + s0);
    int i = t;
    for (; i + 768 < nv; i += 1024) {
        const f32x4 x0 = pv[i], x1 = pv[i + 256], x2 = pv[i + 512], x3 = pv[i + 768];
        a0 += sq4_d(x0); a1 += sq4_d(x1); a2 += sq4_d(x2); a3 += sq4_d(x3);
    }
    for (; i < nv; i += 256) a0 += sq4_d(pv[i]);
    if (t < tail) a1 += sq1_d(p[off + s0 + 4 * (int64_t)nv + t]);
    if (g != nullptr) {
        const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g + off + s0);
        i = t;
        for (; i + 768 < nv; i += 1024) {
            const f32x4 x0 = gv[i], x1 = gv[i + 256], x2 = gv[i + 512], x3 = gv[i + 768];
            b0 += sq4_d(x0); b1 += sq4_d(x1); b2 += sq4_d(x2); b3 += sq4_d(x3);
        }
        for (; i < nv; i += 256) b0 += sq4_d(gv[i]);
        if (t < tail) b1 += sq1_d(g[off + s0 + 4 * (int64_t)nv + t]);
    }
    const double sp = block_sum_d256((a0 + a1) + (a2 + a3), sh);
    const double sg = block_sum_d256((b0 + b1) + (b2 + b3), sh + 4);
    if (t == 0) { partial[2 * item] = sp; partial[2 * item + 1] = sg; }
}
__global__ __launch_bounds__(256) void tss_final_kernel(const int64_t* __restrict__ first, const double* __restrict__ partial,
                                                        int64_t max_items, double* __restrict__ out) {
    __shared__ double sh[8];
    const int k = (int)blockIdx.x;
    const int64_t lo = first[k];
    const int64_t hi = first[k + 1] < max_items ? first[k + 1] : max_items;
    double a = 0.0, b = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) { a += partial[2 * i]; b += partial[2 * i + 1]; }
    const double sp = block_sum_d256(a, sh);
    const double sg = block_sum_d256(b, sh + 4);
    if (threadIdx.x == 0) { out[2 * k] = sp; out[2 * k + 1] = sg; }
}

// ---- the three forms of the update behind gdn_adam_step* (DECOUPLED false) and gdn_adamw_step* (true): argument lists, checks
// and launch geometry are the same for both families, and the capturable forms share the prep launch.
template <bool DECOUPLED>
int adam_step_host(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int32_t step, float grad_scale, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!p || !g || !m || !v || n <= 0 || step < 1) return GDN_ERR_BAD_ARG;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL((adam_kernel<DECOUPLED>), dim3(stream_blocks(n, 256, 4096)), dim3(256), 0, ST(stream), p, g, m, v, n, lr,
                       beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), grad_scale);
    return gdn_launch_status();
}
// the prep launch for the one state, then the update; `guarded`: the entry point that requires a guard record
template <bool DECOUPLED>
int adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, void* state, const void* guard,
                  bool guarded, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!p || !g || !m || !v || n <= 0 || !hyper || !state || (guarded && !guard)) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(adam_prep_kernel, dim3(1), adam_prep_block(1), 0, ST(stream), (AdamDevState*)state, hyper, 1,
                       (const AdamGuard*)guard);
    hipLaunchKernelGGL((adam_dev_kernel<DECOUPLED>), dim3(stream_blocks(n, 256, 4096)), dim3(256), 0, ST(stream), p, g, m, v, n,
                       hyper, (const AdamDevState*)state, (const AdamGuard*)guard);
    return gdn_launch_status();
}
// The map's CONTENTS are the caller's: entries < G or 0xFF.
bool seg_bad_range(int64_t n, const void* map, const void* a, const void* b, const void* c, const void* d) {
    return n <= 0 || (n & 63) != 0 || !map || (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) != 0;
}
template <bool DECOUPLED>
int adam_step_seg(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* map, int32_t G, const float* hyper,
                  void* states, const void* guard, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!p || !g || !m || !v || !hyper || !states || G < 1 || G > 254 || seg_bad_range(n, map, p, g, m, v)) return GDN_ERR_BAD_ARG;
    if (((uintptr_t)hyper & 3) || ((uintptr_t)states & 7) || ((uintptr_t)guard & 7)) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(adam_prep_kernel, dim3(1), adam_prep_block(G), 0, ST(stream), (AdamDevState*)states, hyper, (int)G,
                       (const AdamGuard*)guard);
    hipLaunchKernelGGL((adam_seg_kernel<DECOUPLED>), dim3(stream_rw_blocks(n, true)), dim3(256), 0, ST(stream), (f32x4*)p,
                       (const f32x4*)g, (f32x4*)m, (f32x4*)v, n / 4, map, hyper, (const AdamDevState*)states,
                       (const AdamGuard*)guard);
    return gdn_launch_status();
}

}  // namespace

extern "C" int gdn_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int32_t step, float grad_scale, void* stream) {
    return adam_step_host<false>(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, stream);
}
extern "C" int gdn_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, void* state,
                                 void* stream) {
    return adam_step_dev<false>(p, g, m, v, n, hyper, state, nullptr, false, stream);
}
extern "C" int gdn_adam_step_dev_guarded(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                                         void* state, const void* guard, void* stream) {
    return adam_step_dev<false>(p, g, m, v, n, hyper, state, guard, true, stream);
}
extern "C" int gdn_adam_step_seg(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* map, int32_t G,
                                 const float* hyper, void* states, const void* guard, void* stream) {
    return adam_step_seg<false>(p, g, m, v, n, map, G, hyper, states, guard, stream);
}
extern "C" int gdn_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int32_t step, float grad_scale, void* stream) {
    return adam_step_host<true>(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, stream);
}
extern "C" int gdn_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, void* state,
                                  void* stream) {
    return adam_step_dev<true>(p, g, m, v, n, hyper, state, nullptr, false, stream);
}
extern "C" int gdn_adamw_step_dev_guarded(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                                          void* state, const void* guard, void* stream) {
    return adam_step_dev<true>(p, g, m, v, n, hyper, state, guard, true, stream);
}
extern "C" int gdn_adamw_step_seg(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* map, int32_t G,
                                  const float* hyper, void* states, const void* guard, void* stream) {
    return adam_step_seg<true>(p, g, m, v, n, map, G, hyper, states, guard, stream);
}

extern "C" size_t gdn_grad_sumsq_workspace_bytes(int64_t n) {
    return n > 0 ? (size_t)gradnorm_blocks(n) * sizeof(double) : 0;
}
extern "C" int gdn_grad_sumsq(const float* g, int64_t n, void* guard, int32_t accumulate, void* workspace,
                              size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!g || n <= 0 || !guard || ((uintptr_t)g & 3) || ((uintptr_t)guard & 7) || ((uintptr_t)workspace & 7)) return GDN_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < gdn_grad_sumsq_workspace_bytes(n)) return GDN_ERR_WORKSPACE;
    const int nb = gradnorm_blocks(n);
    hipLaunchKernelGGL(adam_gradnorm_partial_kernel, dim3(nb), dim3(256), 0, ST(stream), g, n, (double*)workspace);
    hipLaunchKernelGGL(adam_gradnorm_final_kernel, dim3(1), dim3(256), 0, ST(stream), (const double*)workspace, nb,
                       (AdamGuard*)guard, accumulate);
    return gdn_launch_status();
}
extern "C" int gdn_grad_guard_finalize(void* guard, const float* hyper, double max_norm, int32_t skip_nonfinite, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!guard || !hyper || ((uintptr_t)guard & 7) || max_norm != max_norm) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(adam_guard_finalize_kernel, dim3(1), dim3(1), 0, ST(stream), (AdamGuard*)guard, hyper, max_norm,
                       skip_nonfinite ? 1 : 0);
    return gdn_launch_status();
}

extern "C" int gdn_ema_update(float* ema, const float* p, int64_t n, double decay, const void* state, const void* guard,
                              void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!ema || !p || n <= 0 || !state || !(decay > 0.0 && decay < 1.0)) return GDN_ERR_BAD_ARG;
    if (((uintptr_t)ema & 3) || ((uintptr_t)p & 3) || ((uintptr_t)state & 7) || ((uintptr_t)guard & 7)) return GDN_ERR_BAD_ARG;
    stream2_launch(ema, p, n, EmaOp{decay, (const AdamDevState*)state, (const AdamGuard*)guard, 0.f}, stream);
    return gdn_launch_status();
}
extern "C" int gdn_swap_f32(float* a, float* b, int64_t n, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!a || !b || n <= 0 || ((uintptr_t)a & 3) || ((uintptr_t)b & 3)) return GDN_ERR_BAD_ARG;
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
    if (ua < ub + bytes && ub < ua + bytes) return GDN_ERR_BAD_ARG;       // overlapping ranges (a == b included)
    stream2_launch(a, b, n, SwapOp{}, stream);
    return gdn_launch_status();
}
extern "C" int gdn_grad_accumulate(float* acc, const float* g, int64_t n, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!acc || !g || n <= 0 || ((uintptr_t)acc & 3) || ((uintptr_t)g & 3)) return GDN_ERR_BAD_ARG;
    const uintptr_t ua = (uintptr_t)acc, ug = (uintptr_t)g, bytes = (uintptr_t)n * sizeof(float);
    if (ua < ug + bytes && ug < ua + bytes) return GDN_ERR_BAD_ARG;       // overlapping ranges (acc == g included)
    stream2_launch(acc, g, n, AccumulateOp{}, stream);
    return gdn_launch_status();
}

extern "C" int gdn_grad_sumsq_seg(const float* g, int64_t n, const uint8_t* map, void* guard, int32_t accumulate, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!g || !guard || seg_bad_range(n, map, g, nullptr, nullptr, nullptr)) return GDN_ERR_BAD_ARG;
    if (((uintptr_t)guard & 7) || ((uintptr_t)workspace & 7)) return GDN_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < gdn_grad_sumsq_workspace_bytes(n)) return GDN_ERR_WORKSPACE;
    const int nb = gradnorm_blocks(n);
    hipLaunchKernelGGL(adam_gradnorm_seg_partial_kernel, dim3(nb), dim3(256), 0, ST(stream), (const f32x4*)g, n / 4, map,
                       (double*)workspace);
    hipLaunchKernelGGL(adam_gradnorm_final_kernel, dim3(1), dim3(256), 0, ST(stream), (const double*)workspace, nb,
                       (AdamGuard*)guard, accumulate);
    return gdn_launch_status();
}
extern "C" int gdn_ema_update_seg(float* ema, const float* p, int64_t n, const uint8_t* map, double decay, const void* states,
                                  const void* guard, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!ema || !p || !states || !(decay > 0.0 && decay < 1.0) || seg_bad_range(n, map, ema, p, nullptr, nullptr)) return GDN_ERR_BAD_ARG;
    if (((uintptr_t)states & 7) || ((uintptr_t)guard & 7)) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(ema_update_seg_kernel, dim3(stream_rw_blocks(n, true)), dim3(256), 0, ST(stream), (f32x4*)ema, (const f32x4*)p,
                       n / 4, map, decay, (const AdamDevState*)states, (const AdamGuard*)guard);
    return gdn_launch_status();
}

extern "C" int gdn_lr_schedule(float* hyper, const double* base_lr, const void* states, int32_t G, int32_t kind, int32_t warmup,
                               int32_t total, double floor, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!hyper || !base_lr || !states || G < 1 || G > 254 || kind < 0 || kind > 2 || warmup < 0 || total < 1) return GDN_ERR_BAD_ARG;
    if (!(floor >= 0.0 && floor <= 1.0)) return GDN_ERR_BAD_ARG;          // (a NaN fails both comparisons)
    if (((uintptr_t)hyper & 3) || ((uintptr_t)base_lr & 7) || ((uintptr_t)states & 7)) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(G <= 64 ? 64 : 256), 0, ST(stream), hyper, base_lr,
                       (const AdamDevState*)states, (int)G, (int)kind, (int)warmup, (int)total, floor);
    return gdn_launch_status();
}

extern "C" int gdn_step_record(void* ring, int32_t cap, const float* const* terms, int32_t n_terms, const float* hyper,
                               const void* state, const void* guard, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!ring || cap < 1 || n_terms < 0 || n_terms > 8 || (n_terms > 0 && !terms)) return GDN_ERR_BAD_ARG;
    if (((uintptr_t)ring & 7) || ((uintptr_t)state & 7) || ((uintptr_t)guard & 7) || ((uintptr_t)hyper & 3)) return GDN_ERR_BAD_ARG;
    StepRecordTerms t;
    for (int j = 0; j < 8; ++j) {
        t.p[j] = j < n_terms ? terms[j] : nullptr;
        if (j < n_terms && (!t.p[j] || ((uintptr_t)t.p[j] & 3))) return GDN_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL(step_record_kernel, dim3(1), dim3(64), 0, ST(stream), (unsigned long long*)ring, (int)cap, t, (int)n_terms,
                       hyper, (const AdamDevState*)state, (const AdamGuard*)guard);
    return gdn_launch_status();
}

// items of the streaming pass: every segment's last slab may be short, so at most cdiv(n, slab) + T of them
static int64_t tss_max_items(int64_t n, int32_t T) { return cdiv64(n, TSS_SLAB) + (int64_t)T; }
extern "C" size_t gdn_tensor_sumsq_workspace_bytes(int64_t n, int32_t T) {
    if (n <= 0 || T < 1) return 0;
    return ((size_t)T + 1) * sizeof(int64_t) + (size_t)tss_max_items(n, T) * 2 * sizeof(double);
}
extern "C" int gdn_tensor_sumsq(const float* p, const float* g, int64_t n, const int64_t* seg, int32_t T, double* out,
                                void* workspace, size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!p || !seg || !out || !workspace || n <= 0 || T < 1) return GDN_ERR_BAD_ARG;
    if ((((uintptr_t)p | (uintptr_t)g) & 15) || (((uintptr_t)seg | (uintptr_t)out | (uintptr_t)workspace) & 7)) return GDN_ERR_BAD_ARG;
    const int64_t max_items = tss_max_items(n, T);
    if (max_items > 0x7fffffff || workspace_bytes < gdn_tensor_sumsq_workspace_bytes(n, T)) return GDN_ERR_BAD_ARG;
    int64_t* first = (int64_t*)workspace;
    double* partial = (double*)(first + T + 1);
    hipLaunchKernelGGL(tss_items_kernel, dim3(1), dim3(256), 0, ST(stream), seg, (int)T, n, first);
    hipLaunchKernelGGL(tss_partial_kernel, dim3((unsigned)max_items), dim3(256), 0, ST(stream), p, g, n, seg, (int)T,
                       (const int64_t*)first, partial);
    hipLaunchKernelGGL(tss_final_kernel, dim3(T), dim3(256), 0, ST(stream), (const int64_t*)first, (const double*)partial,
                       max_items, out);
    return gdn_launch_status();
}
