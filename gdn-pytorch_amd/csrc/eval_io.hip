// Evaluation-side image kernels.
//   crop_normalize: the NYU validation transform (GDN_main.py:41-47: CenterCrop, ArrayToTensor, Normalize) for a whole
//     batch: an HWC window of the decoded image -> NCHW float32 (v/255 - 0.5)/0.5, both divisions correctly rounded like
//     torch's fp32 `/ 255` and `div_(0.5)`.  No bytescale: this transform has no imresize.
//   bytescale_u8: what scipy.misc.imsave does to an image before writing it (bytescale via toimage): per image, over all
//     channels jointly, (x - min) * (255 / (max - min)) clipped to [0, 255], + 0.5, truncated -- in fp64, because the
//     reference copies the float32 tensor into a float64 array first (GDN_main.py:298-306).  NCHW float -> NHWC uint8.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void crop_normalize_kernel(const void* __restrict__ src, int f32, int B, int H0, int W0,
                                                             int C, int off_y, int off_x, int H, int W,
                                                             float* __restrict__ dst) {
    const int64_t total = (int64_t)B * H * W;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int b = (int)(i / ((int64_t)W * H));
        const size_t in = (((size_t)b * H0 + (y + off_y)) * W0 + (x + off_x)) * C;
        float* out = dst + (size_t)b * C * H * W + (size_t)y * W + x;
        for (int c = 0; c < C; ++c) {
            const float v = f32 ? reinterpret_cast<const float*>(src)[in + c]
                                : (float)reinterpret_cast<const unsigned char*>(src)[in + c];
            out[(size_t)c * H * W] = __fdiv_rn(__fdiv_rn(v, 255.0f) - 0.5f, 0.5f);
        }
    }
}

#define BS_T 1024

// one workgroup per image: min / max over C*H*W, then the conversion
__global__ __launch_bounds__(BS_T) void bytescale_u8_kernel(const float* __restrict__ src, int C, int HW,
                                                            unsigned char* __restrict__ dst) {
#pragma clang fp contract(off)
    __shared__ float shlo[BS_T / 64], shhi[BS_T / 64];
    const int64_t per = (int64_t)C * HW;
    const float* s = src + (size_t)blockIdx.x * per;
    unsigned char* d = dst + (size_t)blockIdx.x * per;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = threadIdx.x; i < per; i += BS_T) { const float v = s[i]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { shlo[threadIdx.x >> 6] = lo; shhi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    for (int w = 0; w < BS_T / 64; ++w) { lo = fminf(lo, shlo[w]); hi = fmaxf(hi, shhi[w]); }
    const double cmin = (double)lo;
    double cscale = (double)hi - cmin;
    if (cscale == 0.0) cscale = 1.0;
    const double scale = 255.0 / cscale;
    for (int64_t i = threadIdx.x; i < per; i += BS_T) {      // i indexes the NHWC output: pixel p, channel c
        const int64_t p = i / C;
        const int c = (int)(i - p * C);
        double v = ((double)s[(size_t)c * HW + p] - cmin) * scale;
        v = fmin(fmax(v, 0.0), 255.0) + 0.5;
        d[i] = (unsigned char)(int)v;
    }
}

}  // namespace

extern "C" int gdn_crop_normalize(const void* src, int32_t src_is_f32, int32_t B, int32_t H0, int32_t W0, int32_t C,
                                  int32_t off_y, int32_t off_x, int32_t H, int32_t W, float* dst, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!src || !dst || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C > 3) return GDN_ERR_BAD_ARG;
    if (off_y < 0 || off_x < 0 || (int64_t)off_y + H > H0 || (int64_t)off_x + W > W0) return GDN_ERR_BAD_ARG;
    const int64_t total = (int64_t)B * H * W;
    const int blocks = (int)(cdiv64(total, 256) < 4096 ? cdiv64(total, 256) : 4096);
    hipLaunchKernelGGL(crop_normalize_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, src_is_f32, B, H0, W0,
                       C, off_y, off_x, H, W, dst);
    return gdn_launch_status();
}

extern "C" int gdn_bytescale_u8(const float* src, int32_t B, int32_t C, int32_t H, int32_t W, uint8_t* dst,
                                void* stream) {
    (void)hipGetLastError();
    if (!src || !dst || B <= 0 || C <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > INT32_MAX) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(bytescale_u8_kernel, dim3(B), dim3(BS_T), 0, (hipStream_t)stream, src, C, H * W, dst);
    return gdn_launch_status();
}
