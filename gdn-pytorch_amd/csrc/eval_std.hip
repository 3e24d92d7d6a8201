// Metric KITTI evaluation under the Eigen-split protocol (--eval_protocol standard) and the two kernels of
// the flip test-time augmentation.  No counterpart in the reference: its compute_errors stretches both maps to their own
// min / max (metrics.hip); this one works in metres, at the ground truth's own resolution.
//
// gdn_depth_metrics_std, per image b (its box {h0, w0, y1, y2, x1, x2} comes from the host):
//   prep      one pass over the h0 x w0 pixels, split over SD_NCH workgroups: ground truth -> metres (float32), validity,
//             the prediction resampled to this pixel (bilinear, half-pixel centres, float64, rounded to float32 once); both
//             values go to the workspace (g == 0 marks an invalid pixel), and the first digit of the radix select is counted.
//   digit 1-3 (median scaling only) one launch per further 8-bit digit of an exact radix select over the float32 bit patterns
//             of the valid g and p (all >= +0: bit order == value order; a NaN prediction is canonicalised to the largest
//             pattern and flagged).  Four selections run side by side -- the lower and the upper middle value of g and of p:
//             numpy's median is their mean -- on per-workgroup LDS histograms added to the image's global ones with INTEGER
//             atomics.  Every workgroup derives the digits chosen so far from the finished global histograms (std_replay).
//   partial   ratio = median(g) / median(p) (1 without median scaling), then the six float64 sums and four counts of each
//             workgroup's chunk, combined in a fixed order (lane stride, xor butterfly, wave order).
//   finalize  one workgroup per image sums the chunk partials in a fixed order and writes the twelve doubles.
// Launches: 1 memset node + 3 kernels without median scaling, 1 memset node + 6 kernels with it.  No floating-point atomic
// anywhere: two calls on the same inputs give the same bytes.  Per-pixel arithmetic is float64 with FMA contraction off, so
// that a float64 numpy restatement (tests/eval_std_numpy.py) decides every threshold the same way.
#include "common.h"

namespace {

#define SD_T 256          // threads per workgroup
#define SD_CHUNK 2048     // pixels per workgroup the chunk count is sized for
#define SD_MAX_NCH 1024   // most workgroups per image
#define SD_HIST_INTS (4 * 4 * 256)   // per image: [digit][selection: g lower, g upper, p lower, p upper][bin]
#define SD_NSUM 6         // abs_rel, sq_rel, (g-p)^2, e^2, e, |log10 g - log10 p|
#define SD_NCNT 4         // a1, a2, a3, n

struct StdLayout {
    int nch;              // workgroups per image
    int64_t chunk;        // pixels per workgroup
    size_t off_flags, off_ratio, off_g, off_p, off_sums, off_cnts, zero_bytes, total;
};

inline size_t sd_align(size_t v) { return (v + 255) & ~(size_t)255; }

inline StdLayout std_layout(int64_t B, int64_t Hmax, int64_t Wmax) {
    StdLayout L;
    const int64_t N = Hmax * Wmax;
    int64_t nch = cdiv64(N, SD_CHUNK);
    nch = nch < 1 ? 1 : (nch > SD_MAX_NCH ? SD_MAX_NCH : nch);
    L.nch = (int)nch;
    L.chunk = cdiv64(N, nch);
    size_t o = 0;
    o = sd_align(o + (size_t)B * SD_HIST_INTS * sizeof(int));         // histograms at offset 0
    L.off_flags = o; o = sd_align(o + (size_t)B * sizeof(int));       // NaN-prediction flags
    L.zero_bytes = o;                                                 // [0, zero_bytes) is zeroed by every call
    L.off_ratio = o; o = sd_align(o + (size_t)B * sizeof(double));
    L.off_g = o; o = sd_align(o + (size_t)B * N * sizeof(float));
    L.off_p = o; o = sd_align(o + (size_t)B * N * sizeof(float));
    L.off_sums = o; o = sd_align(o + (size_t)B * nch * SD_NSUM * sizeof(double));
    L.off_cnts = o; o = sd_align(o + (size_t)B * nch * SD_NCNT * sizeof(int));
    L.total = o;
    return L;
}

struct StdBox { int h0, w0, y1, y2, x1, x2; };

// the image's box; h0 / w0 are held inside the pool so that no index derived from them leaves gt or the workspace
__device__ __forceinline__ StdBox std_box(const int32_t* boxes, int b, int Hmax, int Wmax) {
    const int32_t* q = boxes + (size_t)b * 6;
    StdBox r;
    r.h0 = min(max(q[0], 0), Hmax); r.w0 = min(max(q[1], 0), Wmax);
    r.y1 = q[2]; r.y2 = q[3]; r.x1 = q[4]; r.x2 = q[5];
    return r;
}

// one axis of the bilinear resampling: source index pair and weight of output index i
__device__ __forceinline__ void std_axis(int i, int n_in, int n_out, int& i0, int& i1, double& w) {
#pragma clang fp contract(off)
    const double scale = (double)n_in / (double)n_out;
    double s = ((double)i + 0.5) * scale - 0.5;
    s = s > 0.0 ? s : 0.0;
    i0 = min((int)floor(s), n_in - 1);
    i1 = min(i0 + 1, n_in - 1);
    w = s - (double)i0;
}

// Adds one valid pixel to the four LDS histograms of a digit: selection s counts it iff its higher digits equal prefix[s].
__device__ __forceinline__ void std_count(int* hist, unsigned gbits, unsigned pbits, const unsigned prefix[4], unsigned mask,
                                          int shift) {
    if ((gbits & mask) == prefix[0]) atomicAdd(&hist[0 * 256 + ((gbits >> shift) & 255u)], 1);
    if ((gbits & mask) == prefix[1]) atomicAdd(&hist[1 * 256 + ((gbits >> shift) & 255u)], 1);
    if ((pbits & mask) == prefix[2]) atomicAdd(&hist[2 * 256 + ((pbits >> shift) & 255u)], 1);
    if ((pbits & mask) == prefix[3]) atomicAdd(&hist[3 * 256 + ((pbits >> shift) & 255u)], 1);
}

// LDS histograms of one digit -> the image's global ones (integer atomics: the order of arrival does not change a sum)
__device__ __forceinline__ void std_flush(const int* hist, int* ghist_digit) {
    for (int i = threadIdx.x; i < 4 * 256; i += SD_T) {
        const int v = hist[i];
        if (v) atomicAdd(&ghist_digit[i], v);
    }
}

// The digits the four selections have chosen in the first `ndigits` finished global histograms of an image: prefix[s] holds
// them in place, k[s] is the rank that is left among the values sharing that prefix, n the count of valid pixels.  All SD_T
// threads call it and all get the same result (thread t owns bin t; an inclusive scan over the 256 bins finds the bin that
// holds rank k).  sh: 24 ints.
__device__ void std_replay(const int* ghist, int ndigits, int* sh, unsigned prefix[4], int k[4], int& n) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int s = 0; s < 4; ++s) { prefix[s] = 0u; k[s] = 0; }
    n = 0;
    for (int q = 0; q < ndigits; ++q) {
        int h[4], incl[4];
        for (int s = 0; s < 4; ++s) incl[s] = h[s] = ghist[(q * 4 + s) * 256 + t];
        for (int o = 1; o < 64; o <<= 1) {
            for (int s = 0; s < 4; ++s) {
                const int v = __shfl_up(incl[s], o, 64);
                if (lane >= o) incl[s] += v;
            }
        }
        __syncthreads();
        if (lane == 63) for (int s = 0; s < 4; ++s) sh[wv * 4 + s] = incl[s];
        __syncthreads();
        for (int s = 0; s < 4; ++s) for (int w = 0; w < wv; ++w) incl[s] += sh[w * 4 + s];
        if (q == 0) {
            n = sh[0] + sh[4] + sh[8] + sh[12];
            if (n == 0) return;                       // the same n in every thread: a uniform exit
            k[0] = k[2] = (n - 1) / 2;                // the two middle ranks (equal for an odd count)
            k[1] = k[3] = n / 2;
        }
        for (int s = 0; s < 4; ++s) {
            const int excl = incl[s] - h[s];
            if (excl <= k[s] && k[s] < incl[s]) { sh[16 + s] = t; sh[20 + s] = k[s] - excl; }
        }
        __syncthreads();
        for (int s = 0; s < 4; ++s) { prefix[s] |= (unsigned)sh[16 + s] << (24 - 8 * q); k[s] = sh[20 + s]; }
    }
}

__global__ __launch_bounds__(SD_T) void std_prep_kernel(const void* __restrict__ gt, int gt_kind, int Hmax, int Wmax,
                                                        const int32_t* __restrict__ boxes, const float* __restrict__ pred,
                                                        int H, int W, float depth_scale, float min_depth, float max_depth,
                                                        int64_t chunk, float* __restrict__ wg, float* __restrict__ wp,
                                                        int* __restrict__ ghist, int* __restrict__ nan_flags) {
#pragma clang fp contract(off)
    __shared__ int hist[4 * 256];
    const int b = blockIdx.y, t = threadIdx.x;
    const StdBox bx = std_box(boxes, b, Hmax, Wmax);
    const int64_t npx = (int64_t)bx.h0 * bx.w0, N = (int64_t)Hmax * Wmax;
    const int64_t i0 = (int64_t)blockIdx.x * chunk;
    const int64_t i1 = i0 + chunk < npx ? i0 + chunk : npx;
    if (i0 >= i1) return;                                         // uniform: this chunk lies past the image
    for (int i = t; i < 4 * 256; i += SD_T) hist[i] = 0;
    __syncthreads();
    const size_t gt_base = (size_t)b * (size_t)N;
    const float* pr = pred + (size_t)b * H * W;
    const unsigned zero4[4] = {0u, 0u, 0u, 0u};
    const double dscale = (double)depth_scale;
    bool saw_nan = false;
    for (int64_t i = i0 + t; i < i1; i += SD_T) {
        const int y = (int)(i / bx.w0), x = (int)(i - (int64_t)y * bx.w0);
        const size_t at = gt_base + (size_t)y * Wmax + x;
        float g;
        if (gt_kind == 1) g = (float)reinterpret_cast<const unsigned short*>(gt)[at] / 256.0f;        // exact
        else if (gt_kind == 0) g = reinterpret_cast<const float*>(gt)[at];
        else g = (float)(((double)reinterpret_cast<const float*>(gt)[at] + 1.0) / 2.0 * dscale);
        const bool valid = g > min_depth && g < max_depth && y >= bx.y1 && y < bx.y2 && x >= bx.x1 && x < bx.x2;
        float p = 0.f;
        if (valid) {
            int ya, yb, xa, xb;
            double wy, wx;
            std_axis(y, H, bx.h0, ya, yb, wy);
            std_axis(x, W, bx.w0, xa, xb, wx);
            const double t00 = ((double)pr[(size_t)ya * W + xa] + 1.0) / 2.0, t01 = ((double)pr[(size_t)ya * W + xb] + 1.0) / 2.0;
            const double t10 = ((double)pr[(size_t)yb * W + xa] + 1.0) / 2.0, t11 = ((double)pr[(size_t)yb * W + xb] + 1.0) / 2.0;
            const double top = t00 * (1.0 - wx) + t01 * wx, bot = t10 * (1.0 - wx) + t11 * wx;
            const double tv = top * (1.0 - wy) + bot * wy;
            const float v = (float)(tv * dscale);
            if (v != v) { p = __uint_as_float(0x7fffffffu); saw_nan = true; }       // NaN: the largest pattern, sorts last
            else p = v > 0.f ? v : 0.f;                                             // (-0 becomes +0)
            std_count(hist, __float_as_uint(g), __float_as_uint(p), zero4, 0u, 24);
        }
        wg[gt_base + (size_t)i] = valid ? g : 0.f;
        wp[gt_base + (size_t)i] = p;
    }
    if (saw_nan) atomicOr(&nan_flags[b], 1);
    __syncthreads();
    std_flush(hist, ghist + (size_t)b * SD_HIST_INTS);
}

// digit q (1..3) of the four selections
__global__ __launch_bounds__(SD_T) void std_digit_kernel(const int32_t* __restrict__ boxes, int Hmax, int Wmax, int64_t chunk,
                                                         const float* __restrict__ wg, const float* __restrict__ wp,
                                                         int* __restrict__ ghist, int q) {
    __shared__ int hist[4 * 256];
    __shared__ int sh[24];
    const int b = blockIdx.y, t = threadIdx.x;
    const StdBox bx = std_box(boxes, b, Hmax, Wmax);
    const int64_t npx = (int64_t)bx.h0 * bx.w0;
    const int64_t i0 = (int64_t)blockIdx.x * chunk;
    const int64_t i1 = i0 + chunk < npx ? i0 + chunk : npx;
    if (i0 >= i1) return;
    int* gh = ghist + (size_t)b * SD_HIST_INTS;
    unsigned prefix[4];
    int k[4], n;
    std_replay(gh, q, sh, prefix, k, n);
    if (n == 0) return;
    for (int i = t; i < 4 * 256; i += SD_T) hist[i] = 0;
    __syncthreads();
    const int shift = 24 - 8 * q;
    const unsigned mask = 0xffffffffu << (shift + 8);
    const size_t base = (size_t)b * (size_t)Hmax * Wmax;
    for (int64_t i = i0 + t; i < i1; i += SD_T) {
        const float g = wg[base + (size_t)i];
        if (g == 0.f) continue;
        std_count(hist, __float_as_uint(g), __float_as_uint(wp[base + (size_t)i]), prefix, mask, shift);
    }
    __syncthreads();
    std_flush(hist, gh + (size_t)q * 4 * 256);
}

// sum over the workgroup in a fixed order; every thread gets the result.  sh: SD_T / 64 doubles.
__device__ __forceinline__ double std_block_sum(double v, double* sh) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(SD_T) void std_partial_kernel(const int32_t* __restrict__ boxes, int Hmax, int Wmax, int64_t chunk,
                                                           const float* __restrict__ wg, const float* __restrict__ wp,
                                                           const int* __restrict__ ghist, const int* __restrict__ nan_flags,
                                                           float min_depth, float max_depth, int median_scaling,
                                                           double* __restrict__ ratios, double* __restrict__ sums,
                                                           int* __restrict__ cnts) {
#pragma clang fp contract(off)
    __shared__ int sh[24];
    __shared__ double shd[SD_T / 64];
    const int b = blockIdx.y, t = threadIdx.x;
    const StdBox bx = std_box(boxes, b, Hmax, Wmax);
    const int64_t npx = (int64_t)bx.h0 * bx.w0;
    const int64_t i0 = (int64_t)blockIdx.x * chunk;
    const int64_t i1 = i0 + chunk < npx ? i0 + chunk : npx;
    double ratio = 1.0;
    if (median_scaling) {
        unsigned sel[4];
        int k[4], n;
        std_replay(ghist + (size_t)b * SD_HIST_INTS, 4, sh, sel, k, n);
        if (n > 0) {
            const double med_g = ((double)__uint_as_float(sel[0]) + (double)__uint_as_float(sel[1])) / 2.0;
            const double med_p = ((double)__uint_as_float(sel[2]) + (double)__uint_as_float(sel[3])) / 2.0;
            ratio = med_g / med_p;
            if (nan_flags[b]) ratio = __longlong_as_double(0x7ff8000000000000ll);      // numpy's median of a set with a NaN
        }
    }
    if (blockIdx.x == 0 && t == 0) ratios[b] = ratio;
    const double lo = (double)min_depth, hi = (double)max_depth;
    double s_rel = 0, s_sqrel = 0, s_sq = 0, s_e2 = 0, s_e = 0, s_l10 = 0;
    int c1 = 0, c2 = 0, c3 = 0, cn = 0;
    const size_t base = (size_t)b * (size_t)Hmax * Wmax;
    for (int64_t i = i0 + t; i < i1; i += SD_T) {
        const float g32 = wg[base + (size_t)i];
        if (g32 == 0.f) continue;
        const float p32 = wp[base + (size_t)i];
        const double g = (double)g32;
        double p = (__float_as_uint(p32) == 0x7fffffffu ? __longlong_as_double(0x7ff8000000000000ll) : (double)p32) * ratio;
        if (p == p) p = fmin(fmax(p, lo), hi);
        const double d = g - p;
        s_rel += fabs(d) / g;
        s_sqrel += (d * d) / g;
        s_sq += d * d;
        const double e = log(p) - log(g);
        s_e2 += e * e;
        s_e += e;
        s_l10 += fabs(log10(g) - log10(p));
        const double a = g / p, c = p / g;
        const double th = a > c ? a : c;              // a NaN prediction makes both NaN: no threshold counts it
        c1 += th < 1.25 ? 1 : 0;
        c2 += th < 1.5625 ? 1 : 0;
        c3 += th < 1.953125 ? 1 : 0;
        cn += 1;
    }
    s_rel = std_block_sum(s_rel, shd); s_sqrel = std_block_sum(s_sqrel, shd); s_sq = std_block_sum(s_sq, shd);
    s_e2 = std_block_sum(s_e2, shd); s_e = std_block_sum(s_e, shd); s_l10 = std_block_sum(s_l10, shd);
    const double d1 = std_block_sum((double)c1, shd), d2 = std_block_sum((double)c2, shd);     // < 2^53: exact
    const double d3 = std_block_sum((double)c3, shd), dn = std_block_sum((double)cn, shd);
    if (t == 0) {
        const size_t at = (size_t)b * gridDim.x + blockIdx.x;
        double* s = sums + at * SD_NSUM;
        s[0] = s_rel; s[1] = s_sqrel; s[2] = s_sq; s[3] = s_e2; s[4] = s_e; s[5] = s_l10;
        int* c = cnts + at * SD_NCNT;
        c[0] = (int)d1; c[1] = (int)d2; c[2] = (int)d3; c[3] = (int)dn;
    }
}

__global__ __launch_bounds__(SD_T) void std_finalize_kernel(const double* __restrict__ sums, const int* __restrict__ cnts, int nch,
                                                            const double* __restrict__ ratios, double* __restrict__ per_image) {
#pragma clang fp contract(off)
    __shared__ double shd[SD_T / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    double acc[SD_NSUM] = {0, 0, 0, 0, 0, 0};
    double cnt[SD_NCNT] = {0, 0, 0, 0};
    for (int c = t; c < nch; c += SD_T) {
        const size_t at = (size_t)b * nch + c;
        for (int m = 0; m < SD_NSUM; ++m) acc[m] += sums[at * SD_NSUM + m];
        for (int m = 0; m < SD_NCNT; ++m) cnt[m] += (double)cnts[at * SD_NCNT + m];
    }
    for (int m = 0; m < SD_NSUM; ++m) acc[m] = std_block_sum(acc[m], shd);
    for (int m = 0; m < SD_NCNT; ++m) cnt[m] = std_block_sum(cnt[m], shd);
    if (t != 0) return;
    double* o = per_image + (size_t)b * 12;
    const double n = cnt[3], nan = __longlong_as_double(0x7ff8000000000000ll);
    o[0] = n;
    o[11] = 0.0;
    if (n == 0.0) {
        for (int m = 1; m < 11; ++m) o[m] = nan;
        return;
    }
    const double m1 = acc[4] / n, m2 = acc[3] / n;
    const double var = m2 - m1 * m1;
    o[1] = ratios[b];
    o[2] = acc[0] / n;
    o[3] = acc[1] / n;
    o[4] = sqrt(acc[2] / n);
    o[5] = sqrt(m2);
    o[6] = cnt[0] / n; o[7] = cnt[1] / n; o[8] = cnt[2] / n;
    o[9] = acc[5] / n;
    o[10] = var != var ? var : 100.0 * sqrt(var > 0.0 ? var : 0.0);
}

__global__ __launch_bounds__(256) void flip_w_kernel(const float* __restrict__ src, int64_t total, int W, float* __restrict__ dst) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / W;
        const int x = (int)(i - r * W);
        dst[i] = src[r * W + (W - 1 - x)];
    }
}

// out may be a: each element of a is read by the thread that writes it
__global__ __launch_bounds__(256) void flip_mean_kernel(const float* a, const float* __restrict__ b, int64_t total, int W,
                                                        float* out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / W;
        const int x = (int)(i - r * W);
        out[i] = 0.5f * (a[i] + b[r * W + (W - 1 - x)]);
    }
}

inline int flip_grid(int64_t total) {
    const int64_t g = cdiv64(total, 256);
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

inline bool std_dims_ok(int32_t B, int32_t Hmax, int32_t Wmax) {
    return B > 0 && B <= 65535 && Hmax > 0 && Wmax > 0 && (int64_t)Hmax * Wmax <= INT32_MAX;
}

}  // namespace

extern "C" size_t gdn_depth_metrics_std_workspace_bytes(int32_t B, int32_t Hmax, int32_t Wmax) {
    if (!std_dims_ok(B, Hmax, Wmax)) return 0;
    return std_layout(B, Hmax, Wmax).total;
}

extern "C" int gdn_depth_metrics_std(const void* gt, int32_t gt_kind, int32_t Hmax, int32_t Wmax, const int32_t* boxes,
                                     const float* pred, int32_t B, int32_t H, int32_t W, float depth_scale, float min_depth,
                                     float max_depth, int32_t median_scaling, double* per_image, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();
    if (!gt || !boxes || !pred || !per_image || !std_dims_ok(B, Hmax, Wmax) || H <= 0 || W <= 0 ||
        (int64_t)H * W > INT32_MAX || gt_kind < 0 || gt_kind > 2)
        return GDN_ERR_BAD_ARG;
    if (!(min_depth > 0.f) || !(max_depth > min_depth) || !(depth_scale > 0.f) || !(max_depth < INFINITY) ||
        !(depth_scale < INFINITY))
        return GDN_ERR_BAD_ARG;
    const StdLayout L = std_layout(B, Hmax, Wmax);
    if (!workspace || workspace_bytes < L.total) return GDN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int* ghist = (int*)ws;
    int* flags = (int*)(ws + L.off_flags);
    double* ratios = (double*)(ws + L.off_ratio);
    float* wg = (float*)(ws + L.off_g);
    float* wp = (float*)(ws + L.off_p);
    double* sums = (double*)(ws + L.off_sums);
    int* cnts = (int*)(ws + L.off_cnts);
    if (hipMemsetAsync(ws, 0, L.zero_bytes, st) != hipSuccess) return GDN_ERR_LAUNCH;
    const dim3 grid(L.nch, B), block(SD_T);
    hipLaunchKernelGGL(std_prep_kernel, grid, block, 0, st, gt, gt_kind, Hmax, Wmax, boxes, pred, H, W, depth_scale, min_depth,
                       max_depth, L.chunk, wg, wp, ghist, flags);
    if (median_scaling) {
        for (int q = 1; q < 4; ++q)
            hipLaunchKernelGGL(std_digit_kernel, grid, block, 0, st, boxes, Hmax, Wmax, L.chunk, (const float*)wg,
                               (const float*)wp, ghist, q);
    }
    hipLaunchKernelGGL(std_partial_kernel, grid, block, 0, st, boxes, Hmax, Wmax, L.chunk, (const float*)wg, (const float*)wp,
                       (const int*)ghist, (const int*)flags, min_depth, max_depth, median_scaling ? 1 : 0, ratios, sums, cnts);
    hipLaunchKernelGGL(std_finalize_kernel, dim3(B), block, 0, st, (const double*)sums, (const int*)cnts, L.nch,
                       (const double*)ratios, per_image);
    return gdn_launch_status();
}

extern "C" int gdn_flip_w(const float* src, int64_t rows, int32_t W, float* dst, void* stream) {
    (void)hipGetLastError();
    if (!src || !dst || src == dst || rows <= 0 || W <= 0 || rows > INT64_MAX / W) return GDN_ERR_BAD_ARG;
    const int64_t total = rows * W;
    hipLaunchKernelGGL(flip_w_kernel, dim3(flip_grid(total)), dim3(256), 0, (hipStream_t)stream, src, total, W, dst);
    return gdn_launch_status();
}

extern "C" int gdn_flip_mean(const float* a, const float* b, int64_t rows, int32_t W, float* out, void* stream) {
    (void)hipGetLastError();
    if (!a || !b || !out || b == out || rows <= 0 || W <= 0 || rows > INT64_MAX / W) return GDN_ERR_BAD_ARG;
    const int64_t total = rows * W;
    hipLaunchKernelGGL(flip_mean_kernel, dim3(flip_grid(total)), dim3(256), 0, (hipStream_t)stream, a, b, total, W, out);
    return gdn_launch_status();
}
