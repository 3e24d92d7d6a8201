// NYU Depth v2 training-time augmentation on the device, bit-exact with the reference's host pipeline
// (GDN_main.py:94-129, datasets_list.py:399-430; restated in tests/nyu_augment_numpy.py):
//   imresize (bytescale + Pillow BILINEAR 8 bpc, or Pillow 'F') to img_s x (251, 340) -> depth / scale
//   -> RandomCropNumpy(251, 340) -> RandomRotate (scipy.ndimage.rotate, order 3, mode 'constant', clipped to the input's
//   range) -> imresize by `scale` -> CenterCrop -> RandomHorizontalFlip -> RandomColor (RtoD) -> ArrayToTensor, Normalize.
// Building blocks:
//   * the Pillow resampler as two passes (horizontal into a float scratch, then vertical), each computing only the output
//     window the next stage reads; any scale, 2 * ceil(support) + 1 taps, weights recomputed per output sample in double;
//   * the spline rotation as a prefilter (one lane per column, then per row, sequential float64 recursion) and an
//     interpolation kernel (4 x 4 taps, float32 out, clip);
//   * per-sample min/max reductions (partials over 64 workgroups per sample, then a fold: min and max are exact).
// The last vertical pass carries the epilogue: flip, colour multiply, normalise, written into [B][C][H][W].
// Contraction is off wherever a rounding of the restatement must hold; no atomics, so every run gives the same bits.
#include <math.h>
#include <string.h>

#include "common.h"

namespace {

#define NYU_PREC 22
#define NYU_CH 251
#define NYU_CW 340

enum { RS_UNIFORM = 0, RS_CROP = 1, RS_RGB251 = 2, RS_CENTER = 3 };     // which window a resize computes
enum { EPI_F32 = 0, EPI_U8 = 1, EPI_FINAL = 2 };                         // what its vertical pass stores

struct Win { int oh, ow, wy, wx; };

struct RsArgs {
    const void* src; int src_f32;
    int64_t s_b, s_c, s_y, s_x;            // source element strides
    int in_h, in_w, C;
    int f_mode;                            // 1: Pillow 'F' (double weights, float32 between passes); 0: 8 bpc
    const float* mm;                       // 8 bpc: per-sample bytescale min/max, or nullptr (the source is bytes)
    int win_h, win_w;
    Win uni;                               // RS_UNIFORM: one output size and window for the whole batch
    const gdn_nyu_aug_params* p; int stage;
    int divide;                            // F: the result / (float)p[b].scale
    float* tmp;                            // [B][C][in_h][win_w] horizontal-pass result
    void* dst; int epi; int color;         // color: EPI_FINAL applies p[b].mult
    int64_t d_b, d_c, d_y, d_x;            // destination element strides
};

__device__ Win rs_win(const RsArgs& a, int b) {
    Win w = a.uni;
    if (a.stage != RS_UNIFORM) {
        const gdn_nyu_aug_params& q = a.p[b];
        if (a.stage == RS_CROP) w = Win{q.h1, q.w1, q.y1, q.x1};
        else if (a.stage == RS_RGB251) w = Win{NYU_CH, NYU_CW, q.cy, q.cx};
        else w = Win{q.h2, q.w2, q.cy, q.cx};
    }
    if (w.oh < 1) w.oh = 1;                // the struct lives in device memory: keep every index derived from it bounded
    if (w.ow < 1) w.ow = 1;
    return w;
}

// Pillow precompute_coeffs for one output coordinate of the bilinear filter: taps [x0, x0 + n) of the source axis
struct Axis { int x0, n; double center, ss; };

__device__ Axis axis_of(int in_size, int out_size, int xx) {
#pragma clang fp contract(off)
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    Axis a;
    a.center = (xx + 0.5) * scale;
    a.ss = 1.0 / filterscale;
    int xmin = (int)(a.center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(a.center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    a.x0 = xmin;
    a.n = xmax - xmin;
    return a;
}

__device__ __forceinline__ double tap_w(const Axis& a, int x) {
#pragma clang fp contract(off)
    double t = ((double)(x + a.x0) - a.center + 0.5) * a.ss;
    if (t < 0.0) t = -t;
    return t < 1.0 ? 1.0 - t : 0.0;
}

__device__ __forceinline__ double axis_ww(const Axis& a) {
#pragma clang fp contract(off)
    double ww = 0.0;
    for (int x = 0; x < a.n; ++x) ww += tap_w(a, x);
    return ww;
}

// normalised weight of tap x: double ('F'), or Pillow's 22-bit fixed point (8 bpc)
__device__ __forceinline__ double tap_k(const Axis& a, int x, double ww) {
#pragma clang fp contract(off)
    const double w = tap_w(a, x);
    return ww != 0.0 ? w / ww : w;
}

__device__ __forceinline__ int tap_k8(const Axis& a, int x, double ww) {
#pragma clang fp contract(off)
    return (int)(0.5 + tap_k(a, x, ww) * (double)(1 << NYU_PREC));
}

__device__ __forceinline__ int clip8(long long v) {
    const long long s = v >> NYU_PREC;
    return (int)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

__device__ __forceinline__ float rs_src(const RsArgs& a, int b, int c, int y, int x, float cmin, float bscale) {
#pragma clang fp contract(off)
    const int64_t idx = b * a.s_b + c * a.s_c + y * a.s_y + x * a.s_x;
    const float v = a.src_f32 ? reinterpret_cast<const float*>(a.src)[idx]
                              : (float)reinterpret_cast<const unsigned char*>(a.src)[idx];
    if (a.f_mode || !a.mm) return v;
    float s = (v - cmin) * bscale;                          // scipy bytescale in float32
    s = fminf(fmaxf(s, 0.f), 255.f) + 0.5f;
    return (float)(int)(unsigned char)s;
}

__global__ __launch_bounds__(256) void rs_hpass_kernel(RsArgs a, int B) {
#pragma clang fp contract(off)
    const int64_t total = (int64_t)B * a.C * a.in_h * a.win_w;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int xx = (int)(i % a.win_w);
        const int r = (int)((i / a.win_w) % a.in_h);
        const int c = (int)((i / ((int64_t)a.win_w * a.in_h)) % a.C);
        const int b = (int)(i / ((int64_t)a.win_w * a.in_h * a.C));
        const Win w = rs_win(a, b);
        float cmin = 0.f, bscale = 1.f;
        if (!a.f_mode && a.mm) {
            cmin = a.mm[2 * b];
            float cs = a.mm[2 * b + 1] - cmin;
            if (cs == 0.f) cs = 1.f;
            bscale = (float)(255.0 / (double)cs);
        }
        const int ox = xx + w.wx;
        float v = 0.f;
        if (w.ow == a.in_w) {                               // no horizontal pass (Pillow skips an axis that keeps its size)
            if (ox >= 0 && ox < a.in_w) v = rs_src(a, b, c, r, ox, cmin, bscale);
        } else {
            const Axis ax = axis_of(a.in_w, w.ow, ox);
            const double ww = axis_ww(ax);
            if (a.f_mode) {
                double ss = 0.0;
                for (int x = 0; x < ax.n; ++x) ss += (double)rs_src(a, b, c, r, ax.x0 + x, cmin, bscale) * tap_k(ax, x, ww);
                v = (float)ss;
            } else {
                long long ss = 1ll << (NYU_PREC - 1);
                for (int x = 0; x < ax.n; ++x)
                    ss += (long long)(int)rs_src(a, b, c, r, ax.x0 + x, cmin, bscale) * tap_k8(ax, x, ww);
                v = (float)clip8(ss);
            }
        }
        a.tmp[i] = v;
    }
}

__device__ __forceinline__ float normalize01(float v) {
    return __fdiv_rn(__fdiv_rn(v, 255.0f) - 0.5f, 0.5f);        // ArrayToTensor /255, Normalize (t - 0.5) / 0.5
}

__global__ __launch_bounds__(256) void rs_vpass_kernel(RsArgs a, int B) {
#pragma clang fp contract(off)
    const int64_t total = (int64_t)B * a.C * a.win_h * a.win_w;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % a.win_w);
        const int y = (int)((i / a.win_w) % a.win_h);
        const int c = (int)((i / ((int64_t)a.win_w * a.win_h)) % a.C);
        const int b = (int)(i / ((int64_t)a.win_w * a.win_h * a.C));
        const Win w = rs_win(a, b);
        const float* col = a.tmp + ((int64_t)(b * a.C + c) * a.in_h) * a.win_w + x;
        const int oy = y + w.wy;
        float v = 0.f;
        if (w.oh == a.in_h) {
            if (oy >= 0 && oy < a.in_h) v = col[(int64_t)oy * a.win_w];
        } else {
            const Axis ay = axis_of(a.in_h, w.oh, oy);
            const double ww = axis_ww(ay);
            if (a.f_mode) {
                double ss = 0.0;
                for (int k = 0; k < ay.n; ++k) ss += (double)col[(int64_t)(ay.x0 + k) * a.win_w] * tap_k(ay, k, ww);
                v = (float)ss;
            } else {
                long long ss = 1ll << (NYU_PREC - 1);
                for (int k = 0; k < ay.n; ++k)
                    ss += (long long)(int)col[(int64_t)(ay.x0 + k) * a.win_w] * tap_k8(ay, k, ww);
                v = (float)clip8(ss);
            }
        }
        if (a.f_mode && a.divide) v = __fdiv_rn(v, (float)a.p[b].scale);     // depth / scale, float32 by float32
        int xo = x;
        if (a.epi == EPI_FINAL) {
            if (a.p[b].flip) xo = a.win_w - 1 - x;
            if (a.color) {                                  // RandomColor: clip(u8 * mult, 0, 255) in float64, then .float()
                double t = (double)v * a.p[b].mult;
                v = (float)fmin(fmax(t, 0.0), 255.0);
            }
            v = normalize01(v);
        }
        const int64_t o = b * a.d_b + c * a.d_c + y * a.d_y + xo * a.d_x;
        if (a.epi == EPI_U8) reinterpret_cast<unsigned char*>(a.dst)[o] = (unsigned char)(int)v;
        else reinterpret_cast<float*>(a.dst)[o] = v;
    }
}

// per-sample min / max of `count` consecutive elements at sample stride `stride` (uint8 or float32): MM_PARTS workgroups
// per sample write partial results, then one wave per sample folds them (min and max are exact: the order cannot matter)
#define MM_PARTS 64

__global__ __launch_bounds__(256) void nyu_minmax_part_kernel(const void* __restrict__ src, int f32, int64_t count,
                                                              int64_t stride, float* __restrict__ part) {
    __shared__ float slo[4], shi[4];
    float lo = INFINITY, hi = -INFINITY;
    const int64_t base = (int64_t)blockIdx.y * stride;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)MM_PARTS * 256) {
        const float v = f32 ? reinterpret_cast<const float*>(src)[base + i]
                            : (float)reinterpret_cast<const unsigned char*>(src)[base + i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = part + ((int64_t)blockIdx.y * MM_PARTS + blockIdx.x) * 2;
        o[0] = fminf(fminf(slo[0], slo[1]), fminf(slo[2], slo[3]));
        o[1] = fmaxf(fmaxf(shi[0], shi[1]), fmaxf(shi[2], shi[3]));
    }
}

__global__ __launch_bounds__(64) void nyu_minmax_fold_kernel(const float* __restrict__ part, float* __restrict__ mm) {
    const float* q = part + ((int64_t)blockIdx.x * MM_PARTS + threadIdx.x) * 2;
    float lo = q[0], hi = q[1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    if (threadIdx.x == 0) { mm[blockIdx.x * 2] = lo; mm[blockIdx.x * 2 + 1] = hi; }
}

// Cubic B-spline prefilter along one axis of [planes][H][W] planes, one lane per line of n samples (element stride es,
// line stride ls).  src (float32) is read on the first axis; the second runs in place on the float64 coefficients.
// Mirror boundaries; the causal start is the exact sum, the powers of z are running products (z^(n-1) from the host).
// Each sequential pass loads PF_CHUNK samples ahead into registers, so a lane waits for memory once per chunk rather than
// once per sample; the arithmetic and its order are the restatement's.
#define PF_CHUNK 8

__global__ __launch_bounds__(64) void spline_prefilter_kernel(const float* __restrict__ src, double* __restrict__ coef,
                                                              int planes, int C, int lines, int n, int64_t es, int64_t ls,
                                                              int64_t plane_stride, double z, double gain, double zn1_uni,
                                                              const gdn_nyu_aug_params* p, int axis) {
#pragma clang fp contract(off)
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (int64_t)planes * lines) return;
    const int plane = (int)(t / lines), line = (int)(t % lines);
    const double zn1 = p ? p[plane / C].zn1[axis] : zn1_uni;
    double* l = coef + plane * plane_stride + line * ls;
    const float* s = src ? src + plane * plane_stride + line * ls : nullptr;
    for (int i0 = 0; i0 < n; i0 += PF_CHUNK) {
        double v[PF_CHUNK];
#pragma unroll
        for (int k = 0; k < PF_CHUNK; ++k)
            if (i0 + k < n) v[k] = s ? (double)s[(i0 + k) * es] : l[(i0 + k) * es];
#pragma unroll
        for (int k = 0; k < PF_CHUNK; ++k)
            if (i0 + k < n) l[(i0 + k) * es] = v[k] * gain;
    }
    double c0 = l[0] + zn1 * l[(n - 1) * es];
    double zi = z;
    for (int i0 = 1; i0 < n - 1; i0 += PF_CHUNK) {
        double a[PF_CHUNK], b[PF_CHUNK];
#pragma unroll
        for (int k = 0; k < PF_CHUNK; ++k)
            if (i0 + k < n - 1) { a[k] = l[(i0 + k) * es]; b[k] = l[(n - 1 - i0 - k) * es]; }
#pragma unroll
        for (int k = 0; k < PF_CHUNK; ++k)
            if (i0 + k < n - 1) { c0 = c0 + zi * (a[k] + zn1 * b[k]); zi = zi * z; }
    }
    double prev = c0 / (1.0 - zn1 * zn1);
    l[0] = prev;
    for (int i0 = 1; i0 < n; i0 += PF_CHUNK) {
        double v[PF_CHUNK];
#pragma unroll
        for (int k = 0; k < PF_CHUNK; ++k)
            if (i0 + k < n) v[k] = l[(i0 + k) * es];
#pragma unroll
        for (int k = 0; k < PF_CHUNK; ++k)
            if (i0 + k < n) { prev = v[k] + z * prev; l[(i0 + k) * es] = prev; }
    }
    double next = (z * l[(n - 2) * es] + prev) * z / (z * z - 1.0);
    l[(n - 1) * es] = next;
    for (int i0 = n - 2; i0 >= 0; i0 -= PF_CHUNK) {
        double v[PF_CHUNK];
#pragma unroll
        for (int k = 0; k < PF_CHUNK; ++k)
            if (i0 - k >= 0) v[k] = l[(i0 - k) * es];
#pragma unroll
        for (int k = 0; k < PF_CHUNK; ++k)
            if (i0 - k >= 0) { next = z * (next - v[k]); l[(i0 - k) * es] = next; }
    }
}

struct Affine { double m[4], off[2]; };

__device__ __forceinline__ int mirror_idx(int i, int n) {
    if (i < 0) i = -i;
    if (i > n - 1) i = 2 * (n - 1) - i;
    return i;
}

// Order-3 affine resampling (scipy.ndimage.affine_transform, mode 'constant'): output (y, x) of a plane reads the
// coefficients around (m0 y + m1 x + off0, m2 y + m3 x + off1); 0 where that point leaves the plane; float32 out,
// clipped to [mm[2b], mm[2b+1]] when mm is given.
__global__ __launch_bounds__(256) void spline_interp_kernel(const double* __restrict__ coef, float* __restrict__ dst,
                                                            int planes, int C, int H, int W, Affine uni,
                                                            const gdn_nyu_aug_params* p, const float* __restrict__ mm) {
#pragma clang fp contract(off)
    const int64_t total = (int64_t)planes * H * W;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int plane = (int)(i / ((int64_t)W * H));
        const int b = plane / C;
        const Affine af = p ? Affine{{p[b].m[0], p[b].m[1], p[b].m[2], p[b].m[3]}, {p[b].off[0], p[b].off[1]}} : uni;
        const double c0 = ((double)y * af.m[0] + (double)x * af.m[1]) + af.off[0];
        const double c1 = ((double)y * af.m[2] + (double)x * af.m[3]) + af.off[1];
        float v = 0.f;
        if (c0 >= 0.0 && c0 <= (double)(H - 1) && c1 >= 0.0 && c1 <= (double)(W - 1)) {
            const double f0 = floor(c0), f1 = floor(c1);
            double wy[4], wx[4];
            {
                const double t = c0 - f0, u = 1.0 - t;
                wy[0] = u * u * u / 6.0;
                wy[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
                wy[2] = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0;
                wy[3] = 1.0 - (wy[0] + wy[1] + wy[2]);
            }
            {
                const double t = c1 - f1, u = 1.0 - t;
                wx[0] = u * u * u / 6.0;
                wx[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
                wx[2] = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0;
                wx[3] = 1.0 - (wx[0] + wx[1] + wx[2]);
            }
            const int i0 = (int)f0 - 1, i1 = (int)f1 - 1;
            int xs[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) xs[k] = mirror_idx(i1 + k, W);
            const double* pl = coef + (int64_t)plane * H * W;
            double acc = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double* row = pl + (int64_t)mirror_idx(i0 + r, H) * W;
#pragma unroll
                for (int k = 0; k < 4; ++k) acc = acc + (row[xs[k]] * wy[r]) * wx[k];
            }
            v = (float)acc;
        }
        if (mm) v = fminf(fmaxf(v, mm[2 * b]), mm[2 * b + 1]);
        dst[i] = v;
    }
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

inline int grid_for(int64_t total) { return (int)(cdiv64(total, 256) < 4096 ? cdiv64(total, 256) : 4096); }

void launch_resize(const RsArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(rs_hpass_kernel, dim3(grid_for((int64_t)B * a.C * a.in_h * a.win_w)), dim3(256), 0, st, a, B);
    hipLaunchKernelGGL(rs_vpass_kernel, dim3(grid_for((int64_t)B * a.C * a.win_h * a.win_w)), dim3(256), 0, st, a, B);
}

// mm: float[B][2], followed by the partials float[B][MM_PARTS][2]
inline size_t minmax_bytes(int B) { return align256((size_t)B * 2 * sizeof(float) * (1 + MM_PARTS)); }

void launch_minmax(const void* src, int f32, int B, int64_t count, int64_t stride, float* mm, hipStream_t st) {
    float* part = mm + (size_t)B * 2;
    hipLaunchKernelGGL(nyu_minmax_part_kernel, dim3(MM_PARTS, B), dim3(256), 0, st, src, f32, count, stride, part);
    hipLaunchKernelGGL(nyu_minmax_fold_kernel, dim3(B), dim3(64), 0, st, (const float*)part, mm);
}

double spline_z() { return sqrt(3.0) - 2.0; }

double z_pow(int n) {          // running product, as the restatement computes it
    double p = 1.0;
    for (int i = 0; i < n; ++i) p = p * spline_z();
    return p;
}

// prefilter (both axes) + interpolation of B*C planes of H x W; src and dst may alias (src is read only by the first pass)
void launch_rotate(const float* src, float* dst, double* coef, int B, int C, int H, int W, const Affine& uni,
                   const gdn_nyu_aug_params* p, const float* mm, hipStream_t st) {
    const double z = spline_z(), gain = (1.0 - z) * (1.0 - 1.0 / z);
    const int planes = B * C;
    const int64_t ps = (int64_t)H * W;
    hipLaunchKernelGGL(spline_prefilter_kernel, dim3(cdiv(planes * W, 64)), dim3(64), 0, st, src, coef, planes, C, W, H,
                       (int64_t)W, (int64_t)1, ps, z, gain, z_pow(H - 1), p, 0);
    hipLaunchKernelGGL(spline_prefilter_kernel, dim3(cdiv(planes * H, 64)), dim3(64), 0, st, (const float*)nullptr, coef,
                       planes, C, H, W, (int64_t)1, (int64_t)W, ps, z, gain, z_pow(W - 1), p, 1);
    hipLaunchKernelGGL(spline_interp_kernel, dim3(grid_for((int64_t)planes * ps)), dim3(256), 0, st, (const double*)coef,
                       dst, planes, C, H, W, uni, p, mm);
}

RsArgs rs_base() {
    RsArgs a;
    memset(&a, 0, sizeof(a));
    a.stage = RS_UNIFORM;
    return a;
}

}  // namespace

extern "C" size_t gdn_pil_resize_workspace_bytes(int32_t B, int32_t H0, int32_t C, int32_t win_w) {
    if (B <= 0 || H0 <= 0 || C <= 0 || win_w <= 0) return 0;
    return minmax_bytes(B) + (size_t)B * C * H0 * win_w * sizeof(float);
}

extern "C" int gdn_pil_resize_bilinear(const void* src, int32_t src_is_f32, int32_t B, int32_t H0, int32_t W0, int32_t C,
                                       int32_t f_mode, int32_t bytescale, int32_t out_h, int32_t out_w, int32_t win_y,
                                       int32_t win_x, int32_t win_h, int32_t win_w, void* dst, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!src || !dst || B <= 0 || H0 <= 0 || W0 <= 0 || C <= 0 || C > 4 || out_h <= 0 || out_w <= 0) return GDN_ERR_BAD_ARG;
    if (win_h <= 0 || win_w <= 0 || win_y < 0 || win_x < 0 || (int64_t)win_y + win_h > out_h ||
        (int64_t)win_x + win_w > out_w)
        return GDN_ERR_BAD_ARG;
    if (f_mode ? (!src_is_f32 || bytescale) : (src_is_f32 && !bytescale)) return GDN_ERR_BAD_ARG;
    if ((int64_t)B * H0 * W0 * C > INT32_MAX || (int64_t)B * win_h * win_w * C > INT32_MAX) return GDN_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < gdn_pil_resize_workspace_bytes(B, H0, C, win_w)) return GDN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* mm = (float*)workspace;
    RsArgs a = rs_base();
    a.src = src; a.src_f32 = src_is_f32;
    a.s_b = (int64_t)H0 * W0 * C; a.s_c = 1; a.s_y = (int64_t)W0 * C; a.s_x = C;
    a.in_h = H0; a.in_w = W0; a.C = C; a.f_mode = f_mode;
    a.mm = bytescale ? mm : nullptr;
    a.win_h = win_h; a.win_w = win_w;
    a.uni = Win{out_h, out_w, win_y, win_x};
    a.tmp = (float*)((char*)workspace + minmax_bytes(B));
    a.dst = dst; a.epi = f_mode ? EPI_F32 : EPI_U8;
    a.d_b = (int64_t)win_h * win_w * C; a.d_c = 1; a.d_y = (int64_t)win_w * C; a.d_x = C;
    if (bytescale) launch_minmax(src, src_is_f32, B, (int64_t)H0 * W0 * C, (int64_t)H0 * W0 * C, mm, st);
    launch_resize(a, B, st);
    return gdn_launch_status();
}

extern "C" size_t gdn_spline_rotate3_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return minmax_bytes(B) + (size_t)B * C * H * W * sizeof(double);
}

extern "C" int gdn_spline_rotate3(const float* src, int32_t B, int32_t C, int32_t H, int32_t W, const double* matrix,
                                  const double* offset, int32_t clip, float* dst, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    (void)hipGetLastError();
    if (!src || !dst || !matrix || !offset || B <= 0 || C <= 0 || H < 4 || W < 4) return GDN_ERR_BAD_ARG;
    if ((int64_t)B * C * H * W > INT32_MAX) return GDN_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < gdn_spline_rotate3_workspace_bytes(B, C, H, W)) return GDN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* mm = (float*)workspace;
    double* coef = (double*)((char*)workspace + minmax_bytes(B));
    Affine uni;
    for (int k = 0; k < 4; ++k) uni.m[k] = matrix[k];
    uni.off[0] = offset[0];
    uni.off[1] = offset[1];
    if (clip) launch_minmax(src, 1, B, (int64_t)C * H * W, (int64_t)C * H * W, mm, st);
    launch_rotate(src, dst, coef, B, C, H, W, uni, nullptr, clip ? mm : nullptr, st);
    return gdn_launch_status();
}

namespace {
struct NyuWs { float *mm_src, *mm_rot, *mm_rgb; float* planes; double* coef; float* tmp; size_t bytes; };

NyuWs nyu_ws(char* base, int B, int H0, int rtod) {
    const int C = rtod ? 4 : 1;
    const size_t plane = (size_t)NYU_CH * NYU_CW;
    const size_t rows = (size_t)(H0 > NYU_CH ? H0 : NYU_CH);
    NyuWs w;
    size_t o = 0;
    w.mm_src = (float*)(base + o); o += minmax_bytes(B);
    w.mm_rot = (float*)(base + o); o += minmax_bytes(B);
    w.mm_rgb = (float*)(base + o); o += minmax_bytes(B);
    w.planes = (float*)(base + o); o += align256((size_t)B * C * plane * sizeof(float));
    w.coef = (double*)(base + o); o += align256((size_t)B * C * plane * sizeof(double));
    w.tmp = (float*)(base + o); o += (size_t)B * 3 * rows * NYU_CW * sizeof(float);
    w.bytes = o;
    return w;
}
}  // namespace

extern "C" size_t gdn_nyu_augment_workspace_bytes(int32_t B, int32_t H0, int32_t W0, int32_t rtod) {
    if (B <= 0 || H0 <= 0 || W0 <= 0) return 0;
    return nyu_ws(nullptr, B, H0, rtod).bytes;
}

extern "C" int gdn_nyu_augment(const float* depth, const uint8_t* rgb, int32_t B, int32_t H0, int32_t W0, int32_t rtod,
                               const gdn_nyu_aug_params* params, int32_t H, int32_t W, float* depth_out, float* rgb_out,
                               void* workspace, size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();
    if (!depth || !rgb || !params || !depth_out || !rgb_out || B <= 0 || H0 <= 0 || W0 <= 0) return GDN_ERR_BAD_ARG;
    if (H <= 0 || W <= 0 || H > NYU_CH || W > NYU_CW) return GDN_ERR_BAD_ARG;
    if ((int64_t)B * H0 * W0 * 3 > INT32_MAX || (int64_t)B * 4 * NYU_CH * NYU_CW > INT32_MAX) return GDN_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < gdn_nyu_augment_workspace_bytes(B, H0, W0, rtod)) return GDN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int C = rtod ? 4 : 1;
    const int64_t plane = (int64_t)NYU_CH * NYU_CW;
    const NyuWs w = nyu_ws((char*)workspace, B, H0, rtod);

    // source colour range for imresize's bytescale (over all channels of the decoded image)
    launch_minmax(rgb, 0, B, (int64_t)H0 * W0 * 3, (int64_t)H0 * W0 * 3, w.mm_src, st);

    // depth: 'F' resize to h1 x w1, only the 251 x 340 crop window, / scale -> plane C-1 of each sample
    RsArgs d = rs_base();
    d.src = depth; d.src_f32 = 1;
    d.s_b = (int64_t)H0 * W0; d.s_c = 0; d.s_y = W0; d.s_x = 1;
    d.in_h = H0; d.in_w = W0; d.C = 1; d.f_mode = 1;
    d.win_h = NYU_CH; d.win_w = NYU_CW;
    d.p = params; d.stage = RS_CROP; d.divide = 1;
    d.tmp = w.tmp;
    d.dst = w.planes + (C - 1) * plane; d.epi = EPI_F32;
    d.d_b = C * plane; d.d_c = plane; d.d_y = NYU_CW; d.d_x = 1;
    launch_resize(d, B, st);

    // colour: bytescale + 8-bpc resize of the source.  DtoD: to 251 x 340, only the centre-crop window, straight to the
    // output.  RtoD: to h1 x w1, the crop window, into planes 0..2 beside the depth (Merge)
    RsArgs c = rs_base();
    c.src = rgb; c.src_f32 = 0;
    c.s_b = (int64_t)H0 * W0 * 3; c.s_c = 1; c.s_y = (int64_t)W0 * 3; c.s_x = 3;
    c.in_h = H0; c.in_w = W0; c.C = 3; c.f_mode = 0; c.mm = w.mm_src;
    c.p = params; c.tmp = w.tmp;
    if (rtod) {
        c.stage = RS_CROP; c.win_h = NYU_CH; c.win_w = NYU_CW;
        c.dst = w.planes; c.epi = EPI_F32;
        c.d_b = C * plane; c.d_c = plane; c.d_y = NYU_CW; c.d_x = 1;
    } else {
        c.stage = RS_RGB251; c.win_h = H; c.win_w = W;
        c.dst = rgb_out; c.epi = EPI_FINAL;
        c.d_b = (int64_t)3 * H * W; c.d_c = (int64_t)H * W; c.d_y = W; c.d_x = 1;
    }
    launch_resize(c, B, st);

    // RandomRotate over the merged channels, clipped to their joint range (the rotated planes overwrite the inputs)
    launch_minmax(w.planes, 1, B, C * plane, C * plane, w.mm_rot, st);
    Affine none;
    memset(&none, 0, sizeof(none));
    launch_rotate(w.planes, w.planes, w.coef, B, C, NYU_CH, NYU_CW, none, params, w.mm_rot, st);

    // second resize by `scale`, only the centre-crop window, with the epilogue (flip, colour, normalise)
    if (rtod) {
        launch_minmax(w.planes, 1, B, 3 * plane, C * plane, w.mm_rgb, st);
        RsArgs r = rs_base();
        r.src = w.planes; r.src_f32 = 1;
        r.s_b = C * plane; r.s_c = plane; r.s_y = NYU_CW; r.s_x = 1;
        r.in_h = NYU_CH; r.in_w = NYU_CW; r.C = 3; r.f_mode = 0; r.mm = w.mm_rgb;
        r.win_h = H; r.win_w = W; r.p = params; r.stage = RS_CENTER;
        r.tmp = w.tmp;
        r.dst = rgb_out; r.epi = EPI_FINAL; r.color = 1;
        r.d_b = (int64_t)3 * H * W; r.d_c = (int64_t)H * W; r.d_y = W; r.d_x = 1;
        launch_resize(r, B, st);
    }
    RsArgs e = rs_base();
    e.src = w.planes + (C - 1) * plane; e.src_f32 = 1;
    e.s_b = C * plane; e.s_c = 0; e.s_y = NYU_CW; e.s_x = 1;
    e.in_h = NYU_CH; e.in_w = NYU_CW; e.C = 1; e.f_mode = 1;
    e.win_h = H; e.win_w = W; e.p = params; e.stage = RS_CENTER;
    e.tmp = w.tmp;
    e.dst = depth_out; e.epi = EPI_FINAL;
    e.d_b = (int64_t)H * W; e.d_c = 0; e.d_y = W; e.d_x = 1;
    launch_resize(e, B, st);
    return gdn_launch_status();
}
