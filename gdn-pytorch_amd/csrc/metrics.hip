// The reference's three depth-metric protocols (calculate_error.py: compute_errors :10-103 for KITTI, compute_errors_NYU
// :105-150, compute_errors_Make3D :152-182), each as one workgroup per image: min/max normalisation, crop + validity mask,
// lower-median scaling by an 8-bit radix select over the float bit patterns (the selected values are >= +0, so bit order ==
// value order), clamp, and the reductions in fp64.  No host round trips, no sorts, no atomics on global memory.  Every
// pixel value is recomputed from the inputs on each pass (the images stay L2-resident), with correctly rounded divisions
// and no FMA contraction, so that every valid / invalid decision, median and threshold decision equals torch's fp32 one.
// An image without a valid pixel yields NaN metrics (the reference raises there: torch.median of an empty tensor).
// Non-finite inputs follow torch: min / max / median propagate NaN and the clamp keeps it, so a NaN or +-inf pixel in the
// prediction, or a constant prediction (0 / 0), gives NaN sums and a1 = a2 = a3 = 0; a NaN pixel in, or a constant,
// ground truth leaves no valid pixel.
#include "common.h"

namespace {

#define MT 1024   // threads per image

__device__ __forceinline__ double block_sum_d1024(double v, double* sh) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < MT / 64; ++i) s += sh[i];
    return s;
}

// torch.min / torch.max: NaN as soon as one operand is NaN (fminf / fmaxf alone would drop it)
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fminf(a, b); }
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }

// lo[k] = a[k].min(), hi[k] = a[k].max() over the n pixels of K planes of one image as torch gives them: NaN when a pixel
// is NaN, +-inf kept (the normalisation that follows then yields 0 and NaN by plain IEEE arithmetic, as torch's does).
// The pixel loop keeps fminf / fmaxf and only notes, per wave, that a lane saw a NaN (one compare into a lane mask); the
// few steps across lanes and waves carry it.  All MT threads call it; all get the result.
template <int K>
__device__ __forceinline__ void image_minmax(const float* const (&a)[K], int n, float (&lo)[K], float (&hi)[K],
                                             float* shlo, float* shhi) {
    unsigned long long nan[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; nan[k] = 0ull; }
    for (int i = threadIdx.x; i < n; i += MT) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float v = a[k][i];
            lo[k] = fminf(lo[k], v); hi[k] = fmaxf(hi[k], v); nan[k] |= __ballot(v != v);
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (nan[k]) lo[k] = hi[k] = __builtin_nanf("");
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[k] = min_nan(lo[k], __shfl_xor(lo[k], o, 64)); hi[k] = max_nan(hi[k], __shfl_xor(hi[k], o, 64));
        }
        __syncthreads();
        if ((threadIdx.x & 63) == 0) { shlo[threadIdx.x >> 6] = lo[k]; shhi[threadIdx.x >> 6] = hi[k]; }
        __syncthreads();
        for (int i = 0; i < MT / 64; ++i) { lo[k] = min_nan(lo[k], shlo[i]); hi[k] = max_nan(hi[k], shhi[i]); }
    }
}

// k-th smallest (0-based) of { v : f(i, v) is true, 0 <= i < n } by an 8-bit radix select over the float bits.
// Every selected value must be >= +0 and not NaN (bit order == value order): the normalised values are, except that a
// constant or non-finite prediction normalises to NaN -- the kernels count the valid NaN pixels first and, where there
// is one, take the median to be NaN (torch.median) without coming here.  All MT threads call it; all get the result.
template <class F>
__device__ float block_select_kth(F f, int n, int k, int* hist, unsigned* sh_prefix, int* sh_k) {
    const int tid = threadIdx.x;
    unsigned prefix = 0u, mask = 0u;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        __syncthreads();
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += MT) {
            float v;
            if (!f(i, v)) continue;
            const unsigned bits = __float_as_uint(v);
            if ((bits & mask) == prefix) atomicAdd(&hist[(bits >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int cum = 0, sel = 255;
            for (int q = 0; q < 256; ++q) {
                if (cum + hist[q] > k) { sel = q; break; }
                cum += hist[q];
            }
            *sh_k = k - cum;
            *sh_prefix = prefix | ((unsigned)sel << shift);
        }
        __syncthreads();
        k = *sh_k;
        prefix = *sh_prefix;
        mask |= 0xFFu << shift;
    }
    return __uint_as_float(prefix);
}

// (x - mn) / (mx - mn) can only be NaN when mx - mn is not a finite positive number: a NaN or +-inf pixel, or mx == mn.
// Otherwise every x in [mn, mx] normalises to a finite value and nobody has to look for NaN among them.
__device__ __forceinline__ bool may_normalise_to_nan(float mn, float mx) { return !(mx - mn > 0.f && mx - mn < INFINITY); }

// torch.clamp: NaN stays NaN (fminf / fmaxf alone would drop it)
__device__ __forceinline__ float clamp_nan(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

// (x - mn) / (mx - mn) * s as torch evaluates it in fp32: three separately rounded operations
__device__ __forceinline__ float minmax_scale(float x, float mn, float mx, float s) {
#pragma clang fp contract(off)
    return __fdiv_rn(x - mn, mx - mn) * s;
}

// ---- KITTI: compute_errors (calculate_error.py:10-103) ----
struct KittiPx { float g, p; bool valid; };

__device__ __forceinline__ KittiPx kitti_px(const float* gs, const float* g, const float* p, int i, int W, float gmin,
                                            float gmax, float pmin, float pmax, int y1, int y2, int x1, int x2) {
#pragma clang fp contract(off)
    KittiPx v;
    v.p = minmax_scale(p[i], pmin, pmax, 80.f);
    v.g = minmax_scale(g[i], gmin, gmax, 80.f);
    const float s = ((gs[i] + 1.0f) * 0.5f) * 80.f;     // x 0.5 is / 2 exactly; a NaN return fails the comparisons below
    const int y = i / W, x = i - y * W;
    v.valid = (s < 80.f) && (v.g < 80.f) && (s > 1.f) && (v.g > 1.f) && y >= y1 && y < y2 && x >= x1 && x < x2;
    return v;
}

__global__ __launch_bounds__(MT) void depth_metrics_kernel(const float* __restrict__ gt_sparse,
                                                           const float* __restrict__ gt,
                                                           const float* __restrict__ pred, int H, int W, int y1,
                                                           int y2, int x1, int x2, double* __restrict__ per_image) {
#pragma clang fp contract(off)
    __shared__ double shd[MT / 64];
    __shared__ float shf[2][MT / 64];
    __shared__ int hist[256];
    __shared__ unsigned sel_prefix;
    __shared__ int sel_k;
    const int b = blockIdx.x, n = H * W, tid = threadIdx.x;
    const float* gs = gt_sparse + (size_t)b * n;
    const float* g = gt + (size_t)b * n;
    const float* p = pred + (size_t)b * n;

    const float* const planes[2] = {g, p};      // calculate_error.py:38-39
    float lo[2], hi[2];
    image_minmax(planes, n, lo, hi, shf[0], shf[1]);
    const float gmin = lo[0], gmax = hi[0], pmin = lo[1], pmax = hi[1];

    // the valid count; and, for the median of the prediction, whether a valid pixel's normalised prediction is NaN (its
    // ground truth passed two comparisons, so that cannot be)
    const bool p_may_nan = may_normalise_to_nan(pmin, pmax);
    int cnt = 0;
    for (int i = tid; i < n; i += MT) cnt += kitti_px(gs, g, p, i, W, gmin, gmax, pmin, pmax, y1, y2, x1, x2).valid ? 1 : 0;
    const int nvalid = (int)(block_sum_d1024((double)cnt, shd) + 0.5);
    bool med_p_nan = false;     // the same in every thread
    if (p_may_nan) {
        int nan_p = 0;
#pragma nounroll        // hardly ever taken: kept small so that it does not cost the passes around it registers
        for (int i = tid; i < n; i += MT) {
            const KittiPx q = kitti_px(gs, g, p, i, W, gmin, gmax, pmin, pmax, y1, y2, x1, x2);
            nan_p += (q.valid && q.p != q.p) ? 1 : 0;
        }
        med_p_nan = block_sum_d1024((double)nan_p, shd) > 0.5;
    }
    const int kk = nvalid > 0 ? (nvalid - 1) / 2 : 0;

    const float med_g = block_select_kth([&](int i, float& v) {
        const KittiPx q = kitti_px(gs, g, p, i, W, gmin, gmax, pmin, pmax, y1, y2, x1, x2); v = q.g; return q.valid; },
        n, kk, hist, &sel_prefix, &sel_k);
    const float med_p = med_p_nan ? __builtin_nanf("") : block_select_kth([&](int i, float& v) {
        const KittiPx q = kitti_px(gs, g, p, i, W, gmin, gmax, pmin, pmax, y1, y2, x1, x2); v = q.p; return q.valid; },
        n, kk, hist, &sel_prefix, &sel_k);

    double s_abs = 0, s_rel = 0, s_sq = 0, c1 = 0, c2 = 0, c3 = 0, s_d2 = 0, s_log = 0;
    for (int i = tid; i < n; i += MT) {
        const KittiPx v = kitti_px(gs, g, p, i, W, gmin, gmax, pmin, pmax, y1, y2, x1, x2);
        if (!v.valid) continue;
        const float vp = clamp_nan(__fdiv_rn(v.p * med_g, med_p), 1.f, 80.f);
        const float vg = v.g;
        const float th = fmaxf(__fdiv_rn(vg, vp), __fdiv_rn(vp, vg));      // NaN only when both are: vg is finite
        const float d = vg - vp;
        s_abs += (double)fabsf(d);
        s_rel += (double)__fdiv_rn(fabsf(d), vg);
        s_sq += (double)__fdiv_rn(d * d, vg);
        c1 += th < 1.25f ? 1.0 : 0.0;
        c2 += th < 1.5625f ? 1.0 : 0.0;
        c3 += th < 1.953125f ? 1.0 : 0.0;
        s_d2 += (double)(d * d);
        const float lg = logf(vg) - logf(vp);
        s_log += (double)(lg * lg);
    }
    s_abs = block_sum_d1024(s_abs, shd); s_rel = block_sum_d1024(s_rel, shd); s_sq = block_sum_d1024(s_sq, shd);
    c1 = block_sum_d1024(c1, shd); c2 = block_sum_d1024(c2, shd); c3 = block_sum_d1024(c3, shd);
    s_d2 = block_sum_d1024(s_d2, shd); s_log = block_sum_d1024(s_log, shd);
    if (tid == 0) {
        const double nv = nvalid > 0 ? (double)nvalid : __longlong_as_double(0x7ff8000000000000ll);   // none valid: NaN
        double* o = per_image + (size_t)b * 8;
        o[0] = s_abs / nv; o[1] = s_rel / nv; o[2] = s_sq / nv;
        o[3] = c1 / nv; o[4] = c2 / nv; o[5] = c3 / nv;
        o[6] = sqrt(s_d2 / nv); o[7] = sqrt(s_log / nv);
    }
}

// ---- NYU Depth v2: compute_errors_NYU (calculate_error.py:105-150) ----
struct NyuPx { float g, p; bool valid; };

__device__ __forceinline__ NyuPx nyu_px(const float* g, const float* p, int i, int W, float gmin, float gmax, float pmin,
                                        float pmax, int y1, int y2, int x1, int x2) {
    NyuPx v;
    v.g = minmax_scale(g[i], gmin, gmax, 10.f);
    v.p = minmax_scale(p[i], pmin, pmax, 10.f);
    const int y = i / W, x = i - y * W;
    v.valid = (v.g < 10.f) && (v.g > 0.f) && y >= y1 && y < y2 && x >= x1 && x < x2;
    return v;
}

__global__ __launch_bounds__(MT) void depth_metrics_nyu_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                               int H, int W, int y1, int y2, int x1, int x2,
                                                               double* __restrict__ per_image) {
#pragma clang fp contract(off)
    __shared__ double shd[MT / 64];
    __shared__ float shf[2][MT / 64];
    __shared__ int hist[256];
    __shared__ unsigned sel_prefix;
    __shared__ int sel_k;
    const int b = blockIdx.x, n = H * W, tid = threadIdx.x;
    const float* g = gt + (size_t)b * n;
    const float* p = pred + (size_t)b * n;

    const float* const planes[2] = {g, p};
    float lo[2], hi[2];
    image_minmax(planes, n, lo, hi, shf[0], shf[1]);
    const float gmin = lo[0], gmax = hi[0], pmin = lo[1], pmax = hi[1];

    const bool p_may_nan = may_normalise_to_nan(pmin, pmax);
    int cnt = 0;
    for (int i = tid; i < n; i += MT) cnt += nyu_px(g, p, i, W, gmin, gmax, pmin, pmax, y1, y2, x1, x2).valid ? 1 : 0;
    const int nvalid = (int)(block_sum_d1024((double)cnt, shd) + 0.5);
    bool med_p_nan = false;     // the same in every thread
    if (p_may_nan) {
        int nan_p = 0;
#pragma nounroll        // hardly ever taken: kept small so that it does not cost the passes around it registers
        for (int i = tid; i < n; i += MT) {
            const NyuPx q = nyu_px(g, p, i, W, gmin, gmax, pmin, pmax, y1, y2, x1, x2);
            nan_p += (q.valid && q.p != q.p) ? 1 : 0;
        }
        med_p_nan = block_sum_d1024((double)nan_p, shd) > 0.5;
    }
    const int kk = nvalid > 0 ? (nvalid - 1) / 2 : 0;     // torch.median: the lower of the two middle values

    const float med_g = block_select_kth([&](int i, float& v) {
        const NyuPx q = nyu_px(g, p, i, W, gmin, gmax, pmin, pmax, y1, y2, x1, x2); v = q.g; return q.valid; },
        n, kk, hist, &sel_prefix, &sel_k);
    const float med_p = med_p_nan ? __builtin_nanf("") : block_select_kth([&](int i, float& v) {
        const NyuPx q = nyu_px(g, p, i, W, gmin, gmax, pmin, pmax, y1, y2, x1, x2); v = q.p; return q.valid; },
        n, kk, hist, &sel_prefix, &sel_k);

    double s_abs = 0, s_rel = 0, s_l10 = 0, c1 = 0, c2 = 0, c3 = 0, s_d2 = 0, s_log = 0;
    for (int i = tid; i < n; i += MT) {
        const NyuPx v = nyu_px(g, p, i, W, gmin, gmax, pmin, pmax, y1, y2, x1, x2);
        if (!v.valid) continue;
        const float vp = clamp_nan(__fdiv_rn(v.p * med_g, med_p), 1e-3f, 10.f);
        const float vg = v.g;
        const float th = fmaxf(__fdiv_rn(vg, vp), __fdiv_rn(vp, vg));
        const float d = vg - vp;
        s_abs += (double)fabsf(d);
        s_rel += (double)__fdiv_rn(fabsf(d), vg);
        s_l10 += (double)fabsf(log10f(vg) - log10f(vp));
        c1 += th < 1.25f ? 1.0 : 0.0;
        c2 += th < 1.5625f ? 1.0 : 0.0;
        c3 += th < 1.953125f ? 1.0 : 0.0;
        s_d2 += (double)(d * d);
        const float lg = logf(vg) - logf(vp);
        s_log += (double)(lg * lg);
    }
    s_abs = block_sum_d1024(s_abs, shd); s_rel = block_sum_d1024(s_rel, shd); s_l10 = block_sum_d1024(s_l10, shd);
    c1 = block_sum_d1024(c1, shd); c2 = block_sum_d1024(c2, shd); c3 = block_sum_d1024(c3, shd);
    s_d2 = block_sum_d1024(s_d2, shd); s_log = block_sum_d1024(s_log, shd);
    if (tid == 0) {
        const double nv = nvalid > 0 ? (double)nvalid : __longlong_as_double(0x7ff8000000000000ll);   // none valid: NaN
        double* o = per_image + (size_t)b * 8;
        o[0] = s_abs / nv; o[1] = s_rel / nv; o[2] = s_l10 / nv;
        o[3] = c1 / nv; o[4] = c2 / nv; o[5] = c3 / nv;
        o[6] = sqrt(s_d2 / nv); o[7] = sqrt(s_log / nv);
    }
}

// ---- Make3D: compute_errors_Make3D (calculate_error.py:152-182) ----
struct M3Px { float g, p; bool valid; };

__device__ __forceinline__ M3Px m3_px(const float* s, const float* g, const float* p, int i, float smin, float smax,
                                      float gmin, float gmax, float pmin, float pmax) {
    M3Px v;
    const float sn = minmax_scale(s[i], smin, smax, 1.f);      // x 1.f is exact: the normalised value itself
    const float gn = minmax_scale(g[i], gmin, gmax, 1.f);
    const float pn = minmax_scale(p[i], pmin, pmax, 1.f);
    const float s80 = sn * 80.f, g80 = gn * 80.f;
    v.valid = (sn > 1e-2f) && (gn > 1e-2f) && (s80 < 80.f) && (g80 < 80.f);
    v.g = clamp_nan(g80, 1e-2f, 80.f);                         // clamped BEFORE the median scaling, not after
    v.p = clamp_nan(pn * 80.f, 1e-2f, 80.f);
    return v;
}

__global__ __launch_bounds__(MT) void depth_metrics_make3d_kernel(const float* __restrict__ gt_np,
                                                                  const float* __restrict__ gt,
                                                                  const float* __restrict__ pred, int n,
                                                                  double* __restrict__ per_image) {
#pragma clang fp contract(off)
    __shared__ double shd[MT / 64];
    __shared__ float shf[2][MT / 64];
    __shared__ int hist[256];
    __shared__ unsigned sel_prefix;
    __shared__ int sel_k;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* s = gt_np + (size_t)b * n;
    const float* g = gt + (size_t)b * n;
    const float* p = pred + (size_t)b * n;

    const float* const planes[3] = {s, g, p};
    float lo[3], hi[3];
    image_minmax(planes, n, lo, hi, shf[0], shf[1]);
    const float smin = lo[0], smax = hi[0], gmin = lo[1], gmax = hi[1], pmin = lo[2], pmax = hi[2];

    const bool p_may_nan = may_normalise_to_nan(pmin, pmax);
    int cnt = 0;
    for (int i = tid; i < n; i += MT) cnt += m3_px(s, g, p, i, smin, smax, gmin, gmax, pmin, pmax).valid ? 1 : 0;
    const int nvalid = (int)(block_sum_d1024((double)cnt, shd) + 0.5);
    bool med_p_nan = false;     // the same in every thread
    if (p_may_nan) {
        int nan_p = 0;
#pragma nounroll        // hardly ever taken: kept small so that it does not cost the passes around it registers
        for (int i = tid; i < n; i += MT) {
            const M3Px q = m3_px(s, g, p, i, smin, smax, gmin, gmax, pmin, pmax);
            nan_p += (q.valid && q.p != q.p) ? 1 : 0;
        }
        med_p_nan = block_sum_d1024((double)nan_p, shd) > 0.5;
    }
    const int kk = nvalid > 0 ? (nvalid - 1) / 2 : 0;

    const float med_g = block_select_kth([&](int i, float& v) {
        const M3Px q = m3_px(s, g, p, i, smin, smax, gmin, gmax, pmin, pmax); v = q.g; return q.valid; },
        n, kk, hist, &sel_prefix, &sel_k);
    const float med_p = med_p_nan ? __builtin_nanf("") : block_select_kth([&](int i, float& v) {
        const M3Px q = m3_px(s, g, p, i, smin, smax, gmin, gmax, pmin, pmax); v = q.p; return q.valid; },
        n, kk, hist, &sel_prefix, &sel_k);

    double s_abs = 0, s_rel = 0, s_l10 = 0, s_d2 = 0;
    for (int i = tid; i < n; i += MT) {
        const M3Px v = m3_px(s, g, p, i, smin, smax, gmin, gmax, pmin, pmax);
        if (!v.valid) continue;
        const float vp = __fdiv_rn(v.p * med_g, med_p);
        const float vg = v.g;
        const float d = vg - vp;
        s_abs += (double)fabsf(d);
        s_rel += (double)__fdiv_rn(fabsf(d), vg);
        s_l10 += (double)fabsf(log10f(vg) - log10f(vp));
        s_d2 += (double)(d * d);
    }
    s_abs = block_sum_d1024(s_abs, shd); s_rel = block_sum_d1024(s_rel, shd);
    s_l10 = block_sum_d1024(s_l10, shd); s_d2 = block_sum_d1024(s_d2, shd);
    if (tid == 0) {
        const double nv = nvalid > 0 ? (double)nvalid : __longlong_as_double(0x7ff8000000000000ll);
        double* o = per_image + (size_t)b * 4;
        o[0] = s_abs / nv; o[1] = s_rel / nv; o[2] = s_l10 / nv; o[3] = sqrt(s_d2 / nv);
    }
}

// errors[m] = mean over the batch of per_image[b][m], m < M
__global__ void metrics_mean_m_kernel(const double* __restrict__ per_image, int B, int M, float* __restrict__ errors) {
    const int m = threadIdx.x;
    if (m >= M) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += per_image[(size_t)b * M + m];
    errors[m] = (float)(s / (double)B);
}

}  // namespace

extern "C" size_t gdn_depth_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    (void)H; (void)W;
    return (size_t)(B > 0 ? B : 0) * 8 * sizeof(double);
}

extern "C" int gdn_depth_metrics(const float* gt_sparse, const float* gt, const float* pred, int32_t B, int32_t H,
                                 int32_t W, int32_t crop, float* errors, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!gt_sparse || !gt || !pred || !errors || B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > INT32_MAX)
        return GDN_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < gdn_depth_metrics_workspace_bytes(B, H, W)) return GDN_ERR_WORKSPACE;
    int y1 = 0, y2 = H, x1 = 0, x2 = W;
    if (crop) {  // Godard crop, calculate_error.py:28-29
        y1 = (int)(0.3324324 * H); y2 = (int)(0.91351351 * H);
        x1 = (int)(0.0359477 * W); x2 = (int)(0.96405229 * W);
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(depth_metrics_kernel, dim3(B), dim3(MT), 0, st, gt_sparse, gt, pred, H, W, y1, y2, x1, x2,
                       (double*)workspace);
    hipLaunchKernelGGL(metrics_mean_m_kernel, dim3(1), dim3(64), 0, st, (const double*)workspace, B, 8, errors);
    return gdn_launch_status();
}

// the NYU crop (calculate_error.py:109-110) is the Godard x-range on BOTH axes
extern "C" size_t gdn_depth_metrics_nyu_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    (void)H; (void)W;
    return (size_t)(B > 0 ? B : 0) * 8 * sizeof(double);
}

extern "C" int gdn_depth_metrics_nyu(const float* gt, const float* pred, int32_t B, int32_t H, int32_t W, int32_t crop,
                                     float* errors, void* workspace, size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();
    if (!gt || !pred || !errors || B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > INT32_MAX) return GDN_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < gdn_depth_metrics_nyu_workspace_bytes(B, H, W)) return GDN_ERR_WORKSPACE;
    int y1 = 0, y2 = H, x1 = 0, x2 = W;
    if (crop) {
        y1 = (int)(0.0359477 * H); y2 = (int)(0.96405229 * H);
        x1 = (int)(0.0359477 * W); x2 = (int)(0.96405229 * W);
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(depth_metrics_nyu_kernel, dim3(B), dim3(MT), 0, st, gt, pred, H, W, y1, y2, x1, x2,
                       (double*)workspace);
    hipLaunchKernelGGL(metrics_mean_m_kernel, dim3(1), dim3(64), 0, st, (const double*)workspace, B, 8, errors);
    return gdn_launch_status();
}

extern "C" size_t gdn_depth_metrics_make3d_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    (void)H; (void)W;
    return (size_t)(B > 0 ? B : 0) * 4 * sizeof(double);
}

extern "C" int gdn_depth_metrics_make3d(const float* gt_np, const float* gt, const float* pred, int32_t B, int32_t H,
                                        int32_t W, float* errors, void* workspace, size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();
    if (!gt_np || !gt || !pred || !errors || B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > INT32_MAX)
        return GDN_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < gdn_depth_metrics_make3d_workspace_bytes(B, H, W)) return GDN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(depth_metrics_make3d_kernel, dim3(B), dim3(MT), 0, st, gt_np, gt, pred, H * W, (double*)workspace);
    hipLaunchKernelGGL(metrics_mean_m_kernel, dim3(1), dim3(64), 0, st, (const double*)workspace, B, 4, errors);
    return gdn_launch_status();
}
