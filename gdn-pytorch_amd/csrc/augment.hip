// KITTI training-time augmentation on the device, bit-exact with the reference's host pipeline
// (datasets_list.py:82-101 -> transform_list.py RandomHorizontalFlip :158-166, RandomScaleCrop :185-199,
// ArrayToTensor :100-118, Normalize :84-92).  RandomScaleCrop's scipy.misc.imresize is bytescale (min-max
// stretch of non-uint8 data to 0..255) + Pillow's two-pass bilinear resampler: double-precision triangle
// weights normalised to 1, 22-bit fixed point, horizontal pass rounded to uint8, then the vertical pass.
// For the up-scaling RandomScaleCrop draws (1.0-1.15x) every output sample has <= 3 taps per axis, so one
// thread rebuilds the <= 3 horizontally filtered bytes it needs and filters them vertically: 9 source reads
// per output pixel, no intermediate image.  HBM-bound byte work: 1 B/channel read (L2-resident re-reads),
// 4 B/channel written.
// aug_resident_kernel is the same per-pixel code over a batch picked by index from device-resident pools (three images per
// launch, one set of coefficients per pixel); gather_* copy whole samples out of such pools for the NYU transform.
#include "common.h"

namespace {

#define AUG_PREC 22

struct AxisK { int x0, n; int k[3]; };

// Pillow precompute_coeffs + normalize_coeffs_8bpc for one output coordinate (bilinear filter, support 1).
// Contraction is off: the weights must round exactly as the host's separate multiplies and adds do.
__device__ AxisK axis_coeffs(int in_size, int out_size, int xx) {
#pragma clang fp contract(off)
    AxisK a;
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale, ss = 1.0 / filterscale;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > 3) xmax = 3;          // up-scaling only (host checks scaled >= in)
    double w[3] = {0.0, 0.0, 0.0}, ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        double t = (x + xmin - center + 0.5) * ss;
        if (t < 0.0) t = -t;
        w[x] = t < 1.0 ? 1.0 - t : 0.0;
        ww += w[x];
    }
    for (int x = 0; x < 3; ++x) {
        double v = w[x];
        if (x < xmax && ww != 0.0) v = v / ww;
        a.k[x] = (int)(0.5 + v * (double)(1 << AUG_PREC));
    }
    a.x0 = xmin; a.n = xmax;
    return a;
}

__device__ __forceinline__ int clip8(long long v) {
    const long long s = v >> AUG_PREC;
    return (int)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

// per-image min / max of a float source (bytescale's cmin, cmax)
__global__ __launch_bounds__(256) void aug_minmax_kernel(const float* __restrict__ src, int64_t per_image, float* mm) {
    __shared__ float smin[4], smax[4];
    const float* p = src + (size_t)blockIdx.x * per_image;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = threadIdx.x; i < per_image; i += 256) { const float v = p[i]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mm[blockIdx.x * 2 + 0] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
        mm[blockIdx.x * 2 + 1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    }
}

__device__ __forceinline__ int src_byte(const void* src, int f32, size_t idx, float cmin, float bscale) {
#pragma clang fp contract(off)
    if (!f32) return reinterpret_cast<const unsigned char*>(src)[idx];
    float b = (reinterpret_cast<const float*>(src)[idx] - cmin) * bscale;     // scipy bytescale, float32 arithmetic
    b = fminf(fmaxf(b, 0.f), 255.f) + 0.5f;
    return (int)(unsigned char)b;
}

__device__ __forceinline__ float normalize01(float v) {
    return __fdiv_rn(__fdiv_rn(v, 255.0f) - 0.5f, 0.5f);        // ArrayToTensor /255, Normalize (t - 0.5) / 0.5
}

// Validation transform of one pixel: the C channels at `px` (element offset of the pixel's first channel) normalised.
__device__ __forceinline__ void val_pixel(const void* __restrict__ src, int f32, size_t px, int C, size_t plane,
                                          float* __restrict__ out) {
    for (int c = 0; c < C; ++c) {
        const float v = f32 ? reinterpret_cast<const float*>(src)[px + c]
                            : (float)reinterpret_cast<const unsigned char*>(src)[px + c];
        out[(size_t)c * plane] = normalize01(v);
    }
}

// Training transform of one output pixel of one image: the C channels through the two filter passes with the pixel's
// coefficients ky, kx (which depend on the draws and the pixel only, not on the image).  `img` is the element offset of
// the image in src; `sx0` the source column when the width does not change.
__device__ __forceinline__ void aug_pixel(const void* __restrict__ src, int f32, size_t img, int H, int W, int C, int flip,
                                          int sh, int sw, int sx0, const AxisK& ky, const AxisK& kx, float cmin, float bscale,
                                          float* __restrict__ out) {
    for (int c = 0; c < C; ++c) {
        long long v = 1ll << (AUG_PREC - 1);
        for (int r = 0; r < ky.n; ++r) {
            const int sy = ky.x0 + r;
            int hb;
            if (sw != W) {                      // horizontal pass (only when the width changes, as Pillow does)
                long long hsum = 1ll << (AUG_PREC - 1);
                for (int j = 0; j < kx.n; ++j) {
                    int sx = kx.x0 + j;
                    if (flip) sx = W - 1 - sx;
                    hsum += (long long)src_byte(src, f32, img + ((size_t)sy * W + sx) * C + c, cmin, bscale) * kx.k[j];
                }
                hb = clip8(hsum);
            } else {
                int sx = sx0;
                if (flip) sx = W - 1 - sx;
                hb = src_byte(src, f32, img + ((size_t)sy * W + sx) * C + c, cmin, bscale);
            }
            if (sh == H) { v = (long long)hb << AUG_PREC; break; }
            v += (long long)hb * ky.k[r];
        }
        const int ob = sh == H ? (int)(v >> AUG_PREC) : clip8(v);
        out[(size_t)c * H * W] = normalize01((float)ob);
    }
}

__global__ __launch_bounds__(256) void aug_kernel(const void* __restrict__ src, int f32, int B, int H, int W, int C,
                                                  const int* __restrict__ params, int train,
                                                  const float* __restrict__ mm, float* __restrict__ dst) {
    const int64_t total = (int64_t)B * H * W;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % W);
        const int oy = (int)((i / W) % H);
        const int b = (int)(i / ((int64_t)W * H));
        const size_t img = (size_t)b * H * W * C;
        float* out = dst + (size_t)b * C * H * W + (size_t)oy * W + ox;
        if (!train) {
            val_pixel(src, f32, img + ((size_t)oy * W + ox) * C, C, (size_t)H * W, out);
            continue;
        }
        const int* pr = params + b * 5;
        const int flip = pr[0], sh = pr[1], sw = pr[2], offy = pr[3], offx = pr[4];
        float cmin = 0.f, bscale = 1.f;
        if (f32) {
            cmin = mm[b * 2];
            float cs = mm[b * 2 + 1] - cmin;
            if (cs == 0.f) cs = 1.f;
            bscale = (float)(255.0 / (double)cs);
        }
        const AxisK ky = axis_coeffs(H, sh, oy + offy);
        const AxisK kx = axis_coeffs(W, sw, ox + offx);
        aug_pixel(src, f32, img, H, W, C, flip, sh, sw, ox + offx, ky, kx, cmin, bscale, out);
    }
}

// The same transform for a batch assembled from device-resident uint8 pools: sample sel[b][0] of each of the three pools,
// one launch for the three tensors.  The filter coefficients of a pixel are computed once and serve every channel of the
// three images.  Pool offsets are 64-bit: a colour pool at 128x416 passes 2^32 bytes at 26,888 samples.
__global__ __launch_bounds__(256) void aug_resident_kernel(const unsigned char* __restrict__ p0, int C0,
                                                           const unsigned char* __restrict__ p1, int C1,
                                                           const unsigned char* __restrict__ p2, int C2, int B, int H, int W,
                                                           const int* __restrict__ sel, int train, float* __restrict__ d0,
                                                           float* __restrict__ d1, float* __restrict__ d2) {
    const int64_t total = (int64_t)B * H * W;
    const size_t plane = (size_t)H * W;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % W);
        const int oy = (int)((i / W) % H);
        const int b = (int)(i / ((int64_t)W * H));
        const int* pr = sel + b * 6;
        const size_t smp = (size_t)pr[0] * plane;                 // pixels before the sample in every pool
        const size_t pix = (size_t)oy * W + ox;
        float* o0 = d0 + (size_t)b * C0 * plane + pix;
        float* o1 = d1 + (size_t)b * C1 * plane + pix;
        float* o2 = d2 + (size_t)b * C2 * plane + pix;
        if (!train) {
            val_pixel(p0, 0, (smp + pix) * C0, C0, plane, o0);
            val_pixel(p1, 0, (smp + pix) * C1, C1, plane, o1);
            val_pixel(p2, 0, (smp + pix) * C2, C2, plane, o2);
            continue;
        }
        const int flip = pr[1], sh = pr[2], sw = pr[3], offy = pr[4], offx = pr[5];
        const AxisK ky = axis_coeffs(H, sh, oy + offy);
        const AxisK kx = axis_coeffs(W, sw, ox + offx);
        aug_pixel(p0, 0, smp * C0, H, W, C0, flip, sh, sw, ox + offx, ky, kx, 0.f, 1.f, o0);
        aug_pixel(p1, 0, smp * C1, H, W, C1, flip, sh, sw, ox + offx, ky, kx, 0.f, 1.f, o1);
        aug_pixel(p2, 0, smp * C2, H, W, C2, flip, sh, sw, ox + offx, ky, kx, 0.f, 1.f, o2);
    }
}

// dst[b] = pool[idx[b]] for samples of sample_bytes bytes; `bps` blocks share a sample.  16-byte copies when the sample's
// source and destination are both 16-byte aligned, bytes for the tail (or for the whole sample otherwise).
__global__ __launch_bounds__(256) void gather_copy_kernel(const unsigned char* __restrict__ pool, const int* __restrict__ idx,
                                                          size_t sample_bytes, int bps, unsigned char* __restrict__ dst) {
    const int b = blockIdx.x / bps, blk = blockIdx.x % bps;
    const unsigned char* s = pool + (size_t)idx[b] * sample_bytes;
    unsigned char* d = dst + (size_t)b * sample_bytes;
    const size_t step = (size_t)bps * 256, first = (size_t)blk * 256 + threadIdx.x;
    const bool vec = (((uintptr_t)s | (uintptr_t)d) & 15) == 0;
    const size_t nvec = vec ? sample_bytes / 16 : 0;
    for (size_t i = first; i < nvec; i += step)
        reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
    for (size_t i = nvec * 16 + first; i < sample_bytes; i += step) d[i] = s[i];
}

// the same gather widening uint16 to float32 (exact): 8 elements per 16-byte load, two 16-byte stores
__global__ __launch_bounds__(256) void gather_u16_f32_kernel(const unsigned short* __restrict__ pool,
                                                             const int* __restrict__ idx, size_t per_sample, int bps,
                                                             float* __restrict__ dst) {
    const int b = blockIdx.x / bps, blk = blockIdx.x % bps;
    const unsigned short* s = pool + (size_t)idx[b] * per_sample;
    float* d = dst + (size_t)b * per_sample;
    const size_t step = (size_t)bps * 256, first = (size_t)blk * 256 + threadIdx.x;
    const bool vec = (((uintptr_t)s | (uintptr_t)d) & 15) == 0;
    const size_t nvec = vec ? per_sample / 8 : 0;
    for (size_t i = first; i < nvec; i += step) {
        const uint4 u = reinterpret_cast<const uint4*>(s)[i];
        const f32x4 lo = {(float)(u.x & 0xffffu), (float)(u.x >> 16), (float)(u.y & 0xffffu), (float)(u.y >> 16)};
        const f32x4 hi = {(float)(u.z & 0xffffu), (float)(u.z >> 16), (float)(u.w & 0xffffu), (float)(u.w >> 16)};
        reinterpret_cast<f32x4*>(d)[2 * i] = lo;
        reinterpret_cast<f32x4*>(d)[2 * i + 1] = hi;
    }
    for (size_t i = nvec * 8 + first; i < per_sample; i += step) d[i] = (float)s[i];
}

}  // namespace

extern "C" size_t gdn_kitti_augment_workspace_bytes(int32_t B) { return (size_t)(B > 0 ? B : 0) * 2 * sizeof(float) + 16; }

extern "C" int gdn_kitti_augment(const void* src, int32_t src_is_f32, int32_t B, int32_t H, int32_t W, int32_t C,
                                 const int32_t* params, int32_t train, float* dst, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!src || !dst || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C > 4) return GDN_ERR_BAD_ARG;
    if (train && !params) return GDN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    float* mm = (float*)workspace;
    if (train && src_is_f32) {
        if (!workspace || workspace_bytes < gdn_kitti_augment_workspace_bytes(B)) return GDN_ERR_WORKSPACE;
        hipLaunchKernelGGL(aug_minmax_kernel, dim3(B), dim3(256), 0, st, (const float*)src, (int64_t)H * W * C, mm);
    }
    const int64_t total = (int64_t)B * H * W;
    const int blocks = (int)(cdiv64(total, 256) < 4096 ? cdiv64(total, 256) : 4096);
    hipLaunchKernelGGL(aug_kernel, dim3(blocks), dim3(256), 0, st, src, src_is_f32, B, H, W, C, (const int*)params, train,
                       (const float*)mm, dst);
    return gdn_launch_status();
}

extern "C" int gdn_kitti_augment_resident(const uint8_t* gt_pool, int32_t Cg, const uint8_t* rgb_pool, int32_t Cr,
                                          const uint8_t* sparse_pool, int32_t Cs, int32_t H, int32_t W, const int32_t* sel,
                                          int32_t B, int32_t train, float* gt_out, float* rgb_out, float* sparse_out,
                                          void* stream) {
    (void)hipGetLastError();
    if (!gt_pool || !rgb_pool || !sparse_pool || !sel || !gt_out || !rgb_out || !sparse_out) return GDN_ERR_BAD_ARG;
    if (B <= 0 || H <= 0 || W <= 0 || Cg <= 0 || Cg > 4 || Cr <= 0 || Cr > 4 || Cs <= 0 || Cs > 4) return GDN_ERR_BAD_ARG;
    const int64_t total = (int64_t)B * H * W;
    const int blocks = (int)(cdiv64(total, 256) < 4096 ? cdiv64(total, 256) : 4096);
    hipLaunchKernelGGL(aug_resident_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, gt_pool, Cg, rgb_pool, Cr,
                       sparse_pool, Cs, B, H, W, (const int*)sel, train, gt_out, rgb_out, sparse_out);
    return gdn_launch_status();
}

extern "C" int gdn_gather_samples(const void* pool, int32_t elem_bytes, const int32_t* idx, int32_t B, int64_t per_sample,
                                  int32_t to_f32, void* dst, void* stream) {
    (void)hipGetLastError();
    if (!pool || !idx || !dst || B <= 0 || per_sample <= 0) return GDN_ERR_BAD_ARG;
    if (elem_bytes != 1 && elem_bytes != 2) return GDN_ERR_BAD_ARG;
    if (to_f32 && elem_bytes != 2) return GDN_ERR_BAD_ARG;
    // 4 KiB (256 threads x 16 bytes) per block and pass; at most 64 blocks per sample
    const int64_t chunks = cdiv64(per_sample * elem_bytes, 4096);
    int bps = (int)(chunks < 64 ? chunks : 64);
    if ((int64_t)B * bps > 0x7fffffffll) return GDN_ERR_BAD_ARG;
    if (to_f32)
        hipLaunchKernelGGL(gather_u16_f32_kernel, dim3(B * bps), dim3(256), 0, (hipStream_t)stream,
                           (const unsigned short*)pool, (const int*)idx, (size_t)per_sample, bps, (float*)dst);
    else
        hipLaunchKernelGGL(gather_copy_kernel, dim3(B * bps), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)pool,
                           (const int*)idx, (size_t)per_sample * elem_bytes, bps, (unsigned char*)dst);
    return gdn_launch_status();
}
