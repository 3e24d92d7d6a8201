// HBM-bound glue kernels of the GDN hot path for gfx950: BatchNorm finalize /
// apply / backward, x2 bilinear up-sampling, layout transforms, fused Adam.
// All are 16-byte-per-lane streaming kernels (NHWC, channel count % 4 == 0).
#include <type_traits>

#include "common.h"
#include "up2x.h"

namespace {

// log2 of v if v is a power of two, else -1: the channel-quad counts of these networks (16..128) all are, which turns
// the per-element 64-bit division of the flat index into a shift (the division alone cost more than the memory traffic).
inline int pow2_shift(int v) {
    for (int s = 0; s < 31; ++s)
        if ((1 << s) == v) return s;
    return -1;
}
#define SPLIT_PIX_C(i, cq, sh, pix, c)                                       \
    const int64_t pix = (sh) >= 0 ? ((i) >> (sh)) : (i) / (cq);              \
    const int c = (int)((sh) >= 0 ? ((i) & ((cq) - 1)) : ((i) - pix * (cq))) * 4

inline int stream_blocks(int64_t n_items, int threads = 256, int cap = 2048) {
    int64_t b = cdiv64(n_items, threads);
    if (b < 1) b = 1;
    return (int)(b < cap ? b : cap);
}

// ------------------------------------------------------------------ BN forward
__global__ __launch_bounds__(256) void bn_finalize_train_kernel(
    const float* __restrict__ stats, int64_t slots, int C, double count, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* running_mean, float* running_var, float momentum, float eps,
    float* scale, float* shift, float* mean_out, float* invstd_out, long long* num_batches_tracked) {
    __shared__ double sh[8];
    const int c = blockIdx.x;
    if (num_batches_tracked && c == 0 && threadIdx.x == 0) *num_batches_tracked += 1;   // nn.BatchNorm2d bookkeeping
    double s1 = 0.0, s2 = 0.0;
    for (int64_t s = threadIdx.x; s < slots; s += 256) {
        s1 += (double)stats[(s * 2 + 0) * C + c];
        s2 += (double)stats[(s * 2 + 1) * C + c];
    }
    s1 = block_sum_d256(s1, sh);
    s2 = block_sum_d256(s2, sh + 4);
    if (threadIdx.x == 0) {
        const double mean = s1 / count;
        double var = s2 / count - mean * mean;
        if (var < 0.0) var = 0.0;
        const double invstd = 1.0 / sqrt(var + (double)eps);
        const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
        const float sc = (float)((double)g * invstd);
        scale[c] = sc;
        shift[c] = (float)((double)b - mean * (double)g * invstd);
        if (mean_out) mean_out[c] = (float)mean;
        if (invstd_out) invstd_out[c] = (float)invstd;
        if (running_mean) running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * mean);
        if (running_var) {
            const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
            running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * unb);
        }
    }
}

__global__ void bn_eval_coeffs_kernel(const float* gamma, const float* beta, const float* rm, const float* rv,
                                      float eps, int C, float* scale, float* shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    const float inv = 1.0f / sqrtf(rv[c] + eps);
    scale[c] = g * inv;
    shift[c] = b - rm[c] * g * inv;
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const void* __restrict__ y, int ldy,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift,
                                                       const void* __restrict__ res, int ld_res,
                                                       void* __restrict__ out, int ld_out, int64_t npix, int C,
                                                       int relu, int dt, int sh) {
    const int cq = C >> 2;
    const int64_t total = npix * cq;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        SPLIT_PIX_C(i, cq, sh, pix, c);
        const f32x4 v = ld4_any(y, pix * ldy + c, dt & 1);
        const f32x4 s = *reinterpret_cast<const f32x4*>(scale + c);
        const f32x4 t = *reinterpret_cast<const f32x4*>(shift + c);
        f32x4 o = v * s + t;
        if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], 0.f);
        }
        if (res) o += ld4_any(res, pix * ld_res + c, dt & 2);
        st4_any(out, pix * ld_out + c, o, dt & 4);
    }
}

// bf16 tensors: 8 channels per lane (16-byte accesses); same arithmetic
__global__ __launch_bounds__(256) void bn_apply8_kernel(const void* __restrict__ y, int ldy,
                                                        const float* __restrict__ scale,
                                                        const float* __restrict__ shift,
                                                        const void* __restrict__ res, int ld_res,
                                                        void* __restrict__ out, int ld_out, int64_t npix, int C,
                                                        int relu, int dt, int sh) {
    const int co = C >> 3;
    const int64_t total = npix * co;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t pix = sh >= 0 ? (i >> sh) : i / co;
        const int c = (int)(sh >= 0 ? (i & (co - 1)) : (i - pix * co)) * 8;
        f32x4 v0, v1;
        ld8_any(y, pix * ldy + c, dt & 1, v0, v1);
        f32x4 o0 = v0 * *reinterpret_cast<const f32x4*>(scale + c) + *reinterpret_cast<const f32x4*>(shift + c);
        f32x4 o1 = v1 * *reinterpret_cast<const f32x4*>(scale + c + 4) + *reinterpret_cast<const f32x4*>(shift + c + 4);
        if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { o0[e] = fmaxf(o0[e], 0.f); o1[e] = fmaxf(o1[e], 0.f); }
        }
        if (res) {
            f32x4 r0, r1;
            ld8_any(res, pix * ld_res + c, dt & 2, r0, r1);
            o0 += r0; o1 += r1;
        }
        st8_any(out, pix * ld_out + c, o0, o1, dt & 4);
    }
}

// ----------------------------------------------------------------- BN backward
#define BNB_MAXBLK 1024
// pass 1: partial[blk][2][C] = sum over the block's pixels of dz, dz*xhat
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(
    const void* __restrict__ dout, int ld_dout, const void* __restrict__ y, int ldy,
    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
    const float* __restrict__ invstd, float* __restrict__ partial, int64_t npix, int C, int relu, int dt) {
    __shared__ float sh[256 * 8];
    const int cq = C >> 2;
    const int CQ = cq < 256 ? cq : 256;      // channel-quad lanes
    const int PY = 256 / CQ;                 // pixel lanes
    const int tx = threadIdx.x % CQ, ty = threadIdx.x / CQ;
    const int64_t per = cdiv64(npix, gridDim.x);
    const int64_t p0 = blockIdx.x * per, p1 = (p0 + per < npix) ? p0 + per : npix;
    for (int q = tx; q < cq; q += CQ) {
        const int c = q * 4;
        f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f};
        if (ty < PY) {
            const f32x4 s = *reinterpret_cast<const f32x4*>(scale + c);
            const f32x4 t = *reinterpret_cast<const f32x4*>(shift + c);
            const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c);
            const f32x4 is = *reinterpret_cast<const f32x4*>(invstd + c);
            for (int64_t pix = p0 + ty; pix < p1; pix += PY) {
                const f32x4 d = ld4_any(dout, pix * ld_dout + c, dt & 1);
                const f32x4 v = ld4_any(y, pix * ldy + c, dt & 2);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float dz = d[e];
                    if (relu && !(v[e] * s[e] + t[e] > 0.f)) dz = 0.f;
                    a1[e] += dz;
                    a2[e] += dz * ((v[e] - mu[e]) * is[e]);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) { sh[threadIdx.x * 8 + e] = a1[e]; sh[threadIdx.x * 8 + 4 + e] = a2[e]; }
        __syncthreads();
        if (ty == 0) {
            f32x4 r1 = {0.f, 0.f, 0.f, 0.f}, r2 = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < PY; ++j) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { r1[e] += sh[(j * CQ + tx) * 8 + e]; r2[e] += sh[(j * CQ + tx) * 8 + 4 + e]; }
            }
            *reinterpret_cast<f32x4*>(partial + ((size_t)blockIdx.x * 2 + 0) * C + c) = r1;
            *reinterpret_cast<f32x4*>(partial + ((size_t)blockIdx.x * 2 + 1) * C + c) = r2;
        }
    }
}

// pass 2: per-channel totals -> dgamma, dbeta, and the two means used by pass 3
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ partial, int nblk, int C,
                                                              double count, float* dgamma, float* dbeta,
                                                              float* k1, float* k2) {
    __shared__ double sh[8];
    const int c = blockIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) {
        s1 += (double)partial[((size_t)b * 2 + 0) * C + c];
        s2 += (double)partial[((size_t)b * 2 + 1) * C + c];
    }
    s1 = block_sum_d256(s1, sh);
    s2 = block_sum_d256(s2, sh + 4);
    if (threadIdx.x == 0) {
        if (dbeta) dbeta[c] = (float)s1;
        if (dgamma) dgamma[c] = (float)s2;
        k1[c] = (float)(s1 / count);
        k2[c] = (float)(s2 / count);
    }
}

// pass 3: dy = gamma*invstd * (dz - mean(dz) - xhat*mean(dz*xhat))
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(
    const void* __restrict__ dout, int ld_dout, const void* __restrict__ y, int ldy,
    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ k1, const float* __restrict__ k2,
    void* __restrict__ dy, int ld_dy, int64_t npix, int C, int relu, int dt, int sh) {
    const int cq = C >> 2;
    const int64_t total = npix * cq;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        SPLIT_PIX_C(i, cq, sh, pix, c);
        const f32x4 d = ld4_any(dout, pix * ld_dout + c, dt & 1);
        const f32x4 v = ld4_any(y, pix * ldy + c, dt & 2);
        const f32x4 s = *reinterpret_cast<const f32x4*>(scale + c);   // gamma*invstd
        const f32x4 t = *reinterpret_cast<const f32x4*>(shift + c);
        const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c);
        const f32x4 is = *reinterpret_cast<const f32x4*>(invstd + c);
        const f32x4 a = *reinterpret_cast<const f32x4*>(k1 + c);
        const f32x4 b = *reinterpret_cast<const f32x4*>(k2 + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float dz = d[e];
            if (relu && !(v[e] * s[e] + t[e] > 0.f)) dz = 0.f;
            const float xh = (v[e] - mu[e]) * is[e];
            o[e] = s[e] * (dz - a[e] - xh * b[e]);
        }
        st4_any(dy, pix * ld_dy + c, o, dt & 4);
    }
}

__global__ __launch_bounds__(256) void bn_bwd_apply8_kernel(
    const void* __restrict__ dout, int ld_dout, const void* __restrict__ y, int ldy,
    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ k1, const float* __restrict__ k2,
    void* __restrict__ dy, int ld_dy, int64_t npix, int C, int relu, int dt, int sh) {
    const int co = C >> 3;
    const int64_t total = npix * co;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t pix = sh >= 0 ? (i >> sh) : i / co;
        const int c = (int)(sh >= 0 ? (i & (co - 1)) : (i - pix * co)) * 8;
        f32x4 d[2], v[2], o[2];
        ld8_any(dout, pix * ld_dout + c, dt & 1, d[0], d[1]);
        ld8_any(y, pix * ldy + c, dt & 2, v[0], v[1]);
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const f32x4 s = *reinterpret_cast<const f32x4*>(scale + c + 4 * hh);
            const f32x4 t = *reinterpret_cast<const f32x4*>(shift + c + 4 * hh);
            const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c + 4 * hh);
            const f32x4 is = *reinterpret_cast<const f32x4*>(invstd + c + 4 * hh);
            const f32x4 a = *reinterpret_cast<const f32x4*>(k1 + c + 4 * hh);
            const f32x4 b = *reinterpret_cast<const f32x4*>(k2 + c + 4 * hh);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float dz = d[hh][e];
                if (relu && !(v[hh][e] * s[e] + t[e] > 0.f)) dz = 0.f;
                const float xh = (v[hh][e] - mu[e]) * is[e];
                o[hh][e] = s[e] * (dz - a[e] - xh * b[e]);
            }
        }
        st8_any(dy, pix * ld_dy + c, o[0], o[1], dt & 4);
    }
}

// ------------------------------------------------------------------- upsample
// grid.y = output row (b, oy), grid.x covers the Wo * C/4 quads of that row: no per-thread division
__global__ __launch_bounds__(256) void upsample2x_fwd_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                             int B, int H, int W, int C, int align, int dt, int sh) {
    const int cq = C >> 2, Ho = 2 * H, Wo = 2 * W;
    const int row = blockIdx.y, b = row / Ho, oy = row - b * Ho;
    float ly; int y0, y1;
    up_src(oy, H, align, ly, y0, y1);
    const size_t xb = (size_t)b * H * W * C;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < Wo * cq; j += gridDim.x * 256) {
        const int ox = sh >= 0 ? j >> sh : j / cq;
        const int c = (sh >= 0 ? j & (cq - 1) : j - ox * cq) * 4;
        float lx; int x0, x1;
        up_src(ox, W, align, lx, x0, x1);
        const f32x4 v00 = ld4_any(x, xb + ((size_t)y0 * W + x0) * C + c, dt & 1);
        const f32x4 v01 = ld4_any(x, xb + ((size_t)y0 * W + x1) * C + c, dt & 1);
        const f32x4 v10 = ld4_any(x, xb + ((size_t)y1 * W + x0) * C + c, dt & 1);
        const f32x4 v11 = ld4_any(x, xb + ((size_t)y1 * W + x1) * C + c, dt & 1);
        const f32x4 o = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
        st4_any(y, (((size_t)b * Ho + oy) * Wo + ox) * C + c, o, dt & 2);
    }
}

// Round 5 (row N1, bf16 forward half): out = [relu](y * scale + shift) (+ residual) and its x2 bilinear upsampling in ONE pass
// -- a ResidualBlock's output x + bn2(conv2(.)) followed by F.interpolate (AE_model_unet.py:55-57 -> :336-359).  Reads the raw
// convolution output and the residual, writes the block output (low resolution; `low` may be null) and the upsampled tensor; the
// block output is not read back.  Same arithmetic and the same rounding points as bn_apply8_kernel followed by
// upsample2x_fwd_kernel: the four neighbours are rounded to the block output's storage type before they are interpolated, so the
// two forms agree bit for bit.  grid.y = output row (b, oy); the thread at odd (oy, ox) also stores the low-resolution value.
__global__ __launch_bounds__(256) void bn_apply_up2x_kernel(const void* __restrict__ y, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, const void* __restrict__ res,
                                                            void* __restrict__ low, void* __restrict__ up, int B, int H, int W,
                                                            int C, int relu, int align, int dt, int sh) {
    const int cq = C >> 2, Ho = 2 * H, Wo = 2 * W;
    const int row = blockIdx.y, b = row / Ho, oy = row - b * Ho;
    float ly; int y0, y1;
    up_src(oy, H, align, ly, y0, y1);
    const size_t xb = (size_t)b * H * W * C;
    auto act = [&](int yy, int xx, int c, const f32x4& s, const f32x4& t) {
        const size_t at = xb + ((size_t)yy * W + xx) * C + c;
        f32x4 o = ld4_any(y, at, dt & 1) * s + t;
        if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], 0.f);
        }
        if (res) o += ld4_any(res, at, dt & 2);
        if (dt & 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = bf16_h_to_f32(f32_to_bf16_h(o[e]));
        }
        return o;
    };
    for (int j = blockIdx.x * 256 + threadIdx.x; j < Wo * cq; j += gridDim.x * 256) {
        const int ox = sh >= 0 ? j >> sh : j / cq;
        const int c = (sh >= 0 ? j & (cq - 1) : j - ox * cq) * 4;
        float lx; int x0, x1;
        up_src(ox, W, align, lx, x0, x1);
        const f32x4 s = *reinterpret_cast<const f32x4*>(scale + c), t = *reinterpret_cast<const f32x4*>(shift + c);
        const f32x4 v00 = act(y0, x0, c, s, t), v01 = act(y0, x1, c, s, t), v10 = act(y1, x0, c, s, t), v11 = act(y1, x1, c, s, t);
        const f32x4 o = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
        st4_any(up, (((size_t)b * Ho + oy) * Wo + ox) * C + c, o, dt & 8);
        if (low && (oy & 1) && (ox & 1)) {
            const int iy = oy >> 1, ix = ox >> 1;      // (floor(src) of an odd output index is its own source pixel, up to rounding)
            const f32x4 a = (y0 == iy && x0 == ix) ? v00 : act(iy, ix, c, s, t);
            st4_any(low, xb + ((size_t)iy * W + ix) * C + c, a, dt & 4);
        }
    }
}

// The same in tiles (C % 8 == 0, C <= 1024): a workgroup owns TXL low-resolution columns x all channels (8 per lane: 16-byte
// accesses on bf16 tensors) and walks RC low-resolution rows, keeping the last three rows of the block output -- already rounded
// to its storage type -- in LDS with one halo column on either side: every element of y / residual is read once per workgroup
// that needs it (halo rows and columns are the only re-reads), the BatchNorm arithmetic runs once per element, and each lane
// stores the 2 x 2 output pixels of its low-resolution pixel as whole 16-byte pieces of full pixel lines.  Same values as the
// kernel above, bit for bit.
__global__ __launch_bounds__(256) void bn_apply_up2x8_kernel(const void* __restrict__ y, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const void* __restrict__ res,
                                                             void* __restrict__ low, void* __restrict__ up, int B, int H, int W,
                                                             int C, int relu, int align, int dt, int TXL, int RC) {
    extern __shared__ float a_s[];                             // [3 rows][TXL + 2 columns][C]
    const int CG = C >> 3, tid = threadIdx.x;
    const int cg = tid % CG, cl = tid / CG;                    // channel group, local column (>= TXL: only halo duty)
    const int xb0 = blockIdx.x * TXL, b = blockIdx.z, r0 = blockIdx.y * RC, r1 = min(H, r0 + RC);
    const int ix = xb0 + cl, c = cg * 8;
    const bool mine = cl < TXL && ix < W;
    const int rowf = (TXL + 2) * C;                            // floats per LDS row
    const size_t xb = (size_t)b * H * W * C;
    auto act = [&](int yy, int xx, int cc, f32x4& o0, f32x4& o1) {
        const size_t at = xb + ((size_t)yy * W + xx) * C + cc;
        f32x4 v0, v1;
        ld8_any(y, at, dt & 1, v0, v1);
        o0 = v0 * *reinterpret_cast<const f32x4*>(scale + cc) + *reinterpret_cast<const f32x4*>(shift + cc);
        o1 = v1 * *reinterpret_cast<const f32x4*>(scale + cc + 4) + *reinterpret_cast<const f32x4*>(shift + cc + 4);
        if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { o0[e] = fmaxf(o0[e], 0.f); o1[e] = fmaxf(o1[e], 0.f); }
        }
        if (res) {
            f32x4 q0, q1;
            ld8_any(res, at, dt & 2, q0, q1);
            o0 += q0; o1 += q1;
        }
        if (dt & 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { o0[e] = bf16_h_to_f32(f32_to_bf16_h(o0[e])); o1[e] = bf16_h_to_f32(f32_to_bf16_h(o1[e])); }
        }
    };
    auto load_row = [&](int iy) {                              // block output row iy, columns xb0 - 1 .. xb0 + TXL -> slot iy % 3
        if (iy < 0 || iy >= H) return;                         // (never referenced: up_src clamps)
        float* dst = a_s + (iy % 3) * rowf;
        f32x4 o0, o1;
        if (mine) {
            act(iy, ix, c, o0, o1);
            *reinterpret_cast<f32x4*>(dst + (cl + 1) * C + c) = o0;
            *reinterpret_cast<f32x4*>(dst + (cl + 1) * C + c + 4) = o1;
            if (low && iy >= r0 && iy < r1) st8_any(low, xb + ((size_t)iy * W + ix) * C + c, o0, o1, dt & 4);
        }
        if (tid < 2 * CG) {                                    // the two halo columns
            const int side = tid / CG, hx = side ? xb0 + TXL : xb0 - 1;
            if (hx >= 0 && hx < W) {
                act(iy, hx, c, o0, o1);
                *reinterpret_cast<f32x4*>(dst + (side ? TXL + 1 : 0) * C + c) = o0;
                *reinterpret_cast<f32x4*>(dst + (side ? TXL + 1 : 0) * C + c + 4) = o1;
            }
        }
    };
    const int Ho = 2 * H, Wo = 2 * W;
    load_row(r0 - 1);
    load_row(r0);
    for (int iy = r0; iy < r1; ++iy) {
        load_row(iy + 1);
        __syncthreads();
        if (mine) {
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const int oy = 2 * iy + dy;
                float ly; int y0, y1;
                up_src(oy, H, align, ly, y0, y1);
                const float* ra = a_s + (y0 % 3) * rowf + c;
                const float* rb = a_s + (y1 % 3) * rowf + c;
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int ox = 2 * ix + dx;
                    float lx; int x0, x1;
                    up_src(ox, W, align, lx, x0, x1);
                    const int j0 = (x0 - xb0 + 1) * C, j1 = (x1 - xb0 + 1) * C;
                    f32x4 o[2];
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        const f32x4 v00 = *reinterpret_cast<const f32x4*>(ra + j0 + 4 * hh), v01 = *reinterpret_cast<const f32x4*>(ra + j1 + 4 * hh);
                        const f32x4 v10 = *reinterpret_cast<const f32x4*>(rb + j0 + 4 * hh), v11 = *reinterpret_cast<const f32x4*>(rb + j1 + 4 * hh);
                        o[hh] = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
                    }
                    st8_any(up, (((size_t)b * Ho + oy) * Wo + ox) * C + c, o[0], o[1], dt & 8);
                }
            }
        }
        __syncthreads();                                       // (the next row overwrites the slot of row iy - 1)
    }
}

// Gather form of the adjoint (deterministic, no atomics): each input pixel sums
// the <= 6x6 output pixels whose stencil touches it.
__global__ __launch_bounds__(256) void upsample2x_bwd_kernel(const void* __restrict__ dy, void* __restrict__ dx,
                                                             int B, int H, int W, int C, int align, int dt, int sh) {
    const int cq = C >> 2, Ho = 2 * H, Wo = 2 * W;
    const int row = blockIdx.y, b = row / H, iy = row - b * H;
    float wy[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int oy = 2 * iy - 2 + j;
        float l; int a0, a1;
        wy[j] = 0.f;
        if (oy >= 0 && oy < Ho) { up_src(oy, H, align, l, a0, a1); if (a0 == iy) wy[j] += 1.f - l; if (a1 == iy) wy[j] += l; }
    }
    for (int q = blockIdx.x * 256 + threadIdx.x; q < W * cq; q += gridDim.x * 256) {
        const int ix = sh >= 0 ? q >> sh : q / cq;
        const int c = (sh >= 0 ? q & (cq - 1) : q - ix * cq) * 4;
        float wx[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int ox = 2 * ix - 2 + j;
            float l; int a0, a1;
            wx[j] = 0.f;
            if (ox >= 0 && ox < Wo) { up_src(ox, W, align, l, a0, a1); if (a0 == ix) wx[j] += 1.f - l; if (a1 == ix) wx[j] += l; }
        }
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int jy = 0; jy < 6; ++jy) {
            if (wy[jy] == 0.f) continue;
            const int oy = 2 * iy - 2 + jy;
#pragma unroll
            for (int jx = 0; jx < 6; ++jx) {
                if (wx[jx] == 0.f) continue;
                const int ox = 2 * ix - 2 + jx;
                s += (wy[jy] * wx[jx]) * ld4_any(dy, (((size_t)b * Ho + oy) * Wo + ox) * C + c, dt & 1);
            }
        }
        st4_any(dx, (((size_t)b * H + iy) * W + ix) * C + c, s, dt & 2);
    }
}

// --------------------------------------------------------------------- layouts
__global__ void nchw_to_nhwc_kernel(const void* __restrict__ x, void* __restrict__ y, int B, int C, int HW, int dt) {
    const int64_t total = (int64_t)B * HW * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int64_t t = i / C;
        const int hw = (int)(t % HW);
        const int b = (int)(t / HW);
        st1_any(y, i, ld1_any(x, ((size_t)b * C + c) * HW + hw, dt & 1), dt & 2);
    }
}
__global__ void nhwc_to_nchw_kernel(const void* __restrict__ x, void* __restrict__ y, int B, int C, int HW, int dt) {
    const int64_t total = (int64_t)B * HW * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int hw = (int)(i % HW);
        const int64_t t = i / HW;
        const int c = (int)(t % C);
        const int b = (int)(t / C);
        st1_any(y, i, ld1_any(x, ((size_t)b * HW + hw) * C + c, dt & 1), dt & 2);
    }
}

// [ntaps][R][C] -> [ntaps][C][R], 32x32 LDS tiles
__global__ __launch_bounds__(256) void transpose_taps_kernel(const void* __restrict__ w, void* __restrict__ wt,
                                                             int R, int C, int dt) {
    __shared__ float tile[32][33];
    const size_t tb = (size_t)blockIdx.z * R * C;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < R && c0 + tx < C) tile[j][tx] = ld1_any(w, tb + (size_t)(r0 + j) * C + c0 + tx, dt & 1);
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < C && r0 + tx < R) st1_any(wt, tb + (size_t)(c0 + j) * R + r0 + tx, tile[tx][j], dt & 2);
}

// torch [A][Bc][T] <-> tap-major [T][Cout][Cin]
__global__ void weight_tapmajor_kernel(const float* __restrict__ src, float* __restrict__ dst, int Cout, int Cin,
                                       int T, int a_is_cout, int to_tap) {
    const int64_t total = (int64_t)T * Cout * Cin;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ci = (int)(i % Cin);
        const int64_t r = i / Cin;
        const int co = (int)(r % Cout);
        const int t = (int)(r / Cout);
        const size_t ti = a_is_cout ? ((size_t)co * Cin + ci) * T + t : ((size_t)ci * Cout + co) * T + t;
        if (to_tap) dst[i] = src[ti];
        else dst[ti] = src[i];
    }
}

// ------------------------------------------------------------------ elementwise
__global__ void add_kernel(const void* __restrict__ a, const void* __restrict__ b, void* __restrict__ o, int64_t n, int dt) {
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        st4_any(o, i * 4, ld4_any(a, i * 4, dt & 1) + ld4_any(b, i * 4, dt & 2), dt & 4);
    for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        st1_any(o, i, ld1_any(a, i, dt & 1) + ld1_any(b, i, dt & 2), dt & 4);
}
// out[p][c] = a[p][c] (+ b[p][c]); each tensor with its own pixel pitch (channel slices of wider tensors)
__global__ __launch_bounds__(256) void add_pitched_kernel(const void* __restrict__ a, int lda, const void* __restrict__ b, int ldb,
                                                          void* __restrict__ o, int ldo, int64_t npix, int C, int dt, int sh) {
    const int cq = C >> 2;
    const int64_t total = npix * cq;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        SPLIT_PIX_C(i, cq, sh, pix, c);
        f32x4 v = ld4_any(a, pix * lda + c, dt & 1);
        if (b) v += ld4_any(b, pix * ldb + c, dt & 2);
        st4_any(o, pix * ldo + c, v, dt & 4);
    }
}
// out[i] = x[i] * (*s): the chain rule through a scalar loss whose upstream gradient lives on the device
__global__ void scale_dev_kernel(const float* __restrict__ x, const float* __restrict__ s, float* __restrict__ o, int64_t n) {
    const float k = *s;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) o[i] = x[i] * k;
}
__global__ void cast_kernel(const void* __restrict__ a, void* __restrict__ o, int64_t n, int dt) {
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        st4_any(o, i * 4, ld4_any(a, i * 4, dt & 1), dt & 2);
    for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        st1_any(o, i, ld1_any(a, i, dt & 1), dt & 2);
}
__global__ void tanh_bwd_kernel(const float* __restrict__ d, const float* __restrict__ o, float* __restrict__ r, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        r[i] = d[i] * (1.f - o[i] * o[i]);
}
__global__ void fill_kernel(float* __restrict__ p, float v, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

// ------------------------------------------------------------------------ Adam
// torch.optim.Adam: g += wd*p; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
// p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
// The update loop of adam_kernel and adam_dev_kernel: `step` = lr / bc1, `gscale` the gradient's scale (grad_scale, times the guard's coef).
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, int64_t n, float step, float b1, float b2, float eps,
                                            float wd, float bc2s, float gscale) {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float pi = p[i];
        const float gi = g[i] * gscale + wd * pi;
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        p[i] = pi - step * mi / (sqrtf(vi) / bc2s + eps);
    }
}
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                   float b1, float b2, float eps, float wd, float bc1, float bc2s,
                                                   float gscale) {
    adam_update(p, g, m, v, n, lr / bc1, b1, b2, eps, wd, bc2s, gscale);
}

// Capturable Adam: the step counter and the running powers beta^t live in device memory, so a captured training step
// advances them on every replay.  state = { double beta1^t, double beta2^t, int32 t, float bc1, float bc2s }.
struct AdamDevState { double p1, p2; int step; float bc1, bc2s; };
static_assert(sizeof(AdamDevState) == 32, "the step-state table is G x 32 bytes (include/gdn_hip.h)");
// The gradient guard's record (below; include/gdn_hip.h): every capturable kernel takes one, or null for an unguarded update.
struct AdamGuard { double sumsq; float norm, coef; int skip, steps, clipped, skipped; };
static_assert(sizeof(AdamGuard) == 32, "guard record layout is part of the C ABI");
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
    if (guard != nullptr && guard->skip != 0) return;    // a skipped step takes no place in any row's bias corrections
    const int k = (int)threadIdx.x;
    if (k < G) adam_advance(states + k, hyper + 6 * k);
}
inline dim3 adam_prep_block(int G) { return dim3(G <= 64 ? 64 : 256); }       // one wave where it holds every row
// The capturable update of a contiguous range: the gradient's scale is hyper[5], times the guard's coefficient under a guard.
__global__ __launch_bounds__(256) void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                       const float* __restrict__ hyper, const AdamDevState* st,
                                                       const AdamGuard* guard) {
    if (guard != nullptr && guard->skip != 0) return;    // p, m, v are neither read nor written
    adam_update(p, g, m, v, n, hyper[0] / st->bc1, hyper[1], hyper[2], hyper[3], hyper[4], st->bc2s,
                guard != nullptr ? hyper[5] * guard->coef : hyper[5]);
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
// e += w_t (p - e) with w_t = 1 - min(decay, (1 + t) / (10 + t)), t = the step count the Adam update of this store has just
// advanced; every thread computes w_t itself, in double, rounded once.  A skipped step (guard->skip) reads and writes nothing.
struct EmaOp {
    using B = const float;
    double decay; const AdamDevState* st; const AdamGuard* guard; float w;
    __device__ bool begin() {
        if (guard != nullptr && guard->skip != 0) return false;
        const double t = (double)st->step;
        w = (float)(1.0 - fmin(decay, (1.0 + t) / (10.0 + t)));
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
    hipLaunchKernelGGL(kernel, dim3(stream_rw_blocks(n, vec)), dim3(256), 0, (hipStream_t)stream, a, b, n, op);
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
// One element of adam_update with the roundings of that loop's gfx950 code spelled out, so the bits are the same whatever
// the compiler would contract in a four-wide body: there the weight decay is fused into the scaled gradient
// (fma(wd, p, g * gscale)) and every other product and sum is rounded on its own.  tests/test_hip_seg_adam.py holds the two
// forms to bit identity.
__device__ __forceinline__ void adam_update1(float& p, float g, float& m, float& v, float step, float b1, float b2, float eps,
                                             float wd, float bc2s, float gscale) {
#pragma clang fp contract(off)
    const float pi = p;
    const float gi = fmaf(wd, pi, g * gscale);
    const float mi = b1 * m + (1.f - b1) * gi;
    const float vi = b2 * v + (1.f - b2) * gi * gi;
    m = mi; v = vi;
    p = pi - step * mi / (sqrtf(vi) / bc2s + eps);
}
__global__ __launch_bounds__(256) void adam_seg_kernel(f32x4* __restrict__ p, const f32x4* __restrict__ g, f32x4* __restrict__ m,
                                                       f32x4* __restrict__ v, int64_t nvec, const uint8_t* __restrict__ map,
                                                       const float* __restrict__ hyper, const AdamDevState* __restrict__ states,
                                                       const AdamGuard* guard) {
    if (guard != nullptr && guard->skip != 0) return;    // p, m, v are neither read nor written
    const int64_t T = (int64_t)gridDim.x * 256;
    for (int64_t i0 = blockIdx.x * 256ll; i0 < nvec; i0 += T) {      // (block-uniform bound: every lane reaches the shuffle)
        const int64_t i = i0 + threadIdx.x;
        const int k = seg_group(map, i, i < nvec);
        if (k == SEG_SKIP) continue;
        const float* __restrict__ h = hyper + 6 * k;
        const AdamDevState* st = states + k;
        const float gscale = guard != nullptr ? h[5] * guard->coef : h[5];
        const float step = h[0] / st->bc1, b1 = h[1], b2 = h[2], eps = h[3], wd = h[4], bc2s = st->bc2s;
        const f32x4 gi = g[i];
        const f32x4 p4 = p[i], m4 = m[i], v4 = v[i];
        float pe[4] = {p4.x, p4.y, p4.z, p4.w}, me[4] = {m4.x, m4.y, m4.z, m4.w}, ve[4] = {v4.x, v4.y, v4.z, v4.w};
        const float ge[4] = {gi.x, gi.y, gi.z, gi.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) adam_update1(pe[e], ge[e], me[e], ve[e], step, b1, b2, eps, wd, bc2s, gscale);
        m[i] = f32x4{me[0], me[1], me[2], me[3]};
        v[i] = f32x4{ve[0], ve[1], ve[2], ve[3]};
        p[i] = f32x4{pe[0], pe[1], pe[2], pe[3]};
    }
}
// ---- decoupled weight decay (AdamW; include/gdn_hip.h).  The gradient carries no decay term, so the moments
// never see it; the decay dec * p, dec = float(lr * wd) with the product in double, is added to the Adam term q and the sum is
// subtracted from the weight ONCE: p (1 - lr wd) in float32 loses the decay altogether at this project's rates (1 - 1e-8
// rounds to 1).  One element, every product, sum, quotient and root rounded on its own but the one fma: all four adamw kernels
// go through it, so their bits agree, and with dec = 0 it is adam_update1 at wd = 0.
// dec = (float)((double)lr * (double)wd): the double product of two floats is exact (48 bits), so its one rounding to float IS
// the IEEE float product -- written as that, which keeps double-rate instructions out of a loop that streams at HBM speed.
__device__ __forceinline__ float adamw_dec(float lr, float wd) { return lr * wd; }
__device__ __forceinline__ void adamw_update1(float& p, float g, float& m, float& v, float step, float b1, float b2, float eps,
                                              float dec, float bc2s, float gscale) {
#pragma clang fp contract(off)
    const float pi = p;
    const float gi = g * gscale;
    const float mi = b1 * m + (1.f - b1) * gi;
    const float vi = b2 * v + (1.f - b2) * gi * gi;
    m = mi; v = vi;
    const float q = step * mi / (sqrtf(vi) / bc2s + eps);
    p = pi - fmaf(dec, pi, q);
}
// adam_update's loop (a scalar grid-stride loop over any start and n) with the decoupled element
__device__ __forceinline__ void adamw_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, int64_t n, float step, float b1, float b2, float eps,
                                             float dec, float bc2s, float gscale) {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float pi = p[i], mi = m[i], vi = v[i];
        adamw_update1(pi, g[i], mi, vi, step, b1, b2, eps, dec, bc2s, gscale);
        m[i] = mi; v[i] = vi;
        p[i] = pi;
    }
}
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                    float b1, float b2, float eps, float wd, float bc1, float bc2s,
                                                    float gscale) {
    adamw_update(p, g, m, v, n, lr / bc1, b1, b2, eps, adamw_dec(lr, wd), bc2s, gscale);
}
__global__ __launch_bounds__(256) void adamw_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                        const float* __restrict__ hyper, const AdamDevState* st,
                                                        const AdamGuard* guard) {
    if (guard != nullptr && guard->skip != 0) return;    // p, m, v are neither read nor written: a skipped step does not decay
    adamw_update(p, g, m, v, n, hyper[0] / st->bc1, hyper[1], hyper[2], hyper[3], adamw_dec(hyper[0], hyper[4]), st->bc2s,
                 guard != nullptr ? hyper[5] * guard->coef : hyper[5]);
}
// adam_seg_kernel with the decoupled element: the same grid, the same map reads, the same 16 bytes per lane
__global__ __launch_bounds__(256) void adamw_seg_kernel(f32x4* __restrict__ p, const f32x4* __restrict__ g, f32x4* __restrict__ m,
                                                        f32x4* __restrict__ v, int64_t nvec, const uint8_t* __restrict__ map,
                                                        const float* __restrict__ hyper, const AdamDevState* __restrict__ states,
                                                        const AdamGuard* guard) {
    if (guard != nullptr && guard->skip != 0) return;    // p, m, v are neither read nor written
    const int64_t T = (int64_t)gridDim.x * 256;
    for (int64_t i0 = blockIdx.x * 256ll; i0 < nvec; i0 += T) {      // (block-uniform bound: every lane reaches the shuffle)
        const int64_t i = i0 + threadIdx.x;
        const int k = seg_group(map, i, i < nvec);
        if (k == SEG_SKIP) continue;
        const float* __restrict__ h = hyper + 6 * k;
        const AdamDevState* st = states + k;
        const float gscale = guard != nullptr ? h[5] * guard->coef : h[5];
        const float step = h[0] / st->bc1, b1 = h[1], b2 = h[2], eps = h[3], dec = adamw_dec(h[0], h[4]), bc2s = st->bc2s;
        const f32x4 gi = g[i];
        const f32x4 p4 = p[i], m4 = m[i], v4 = v[i];
        float pe[4] = {p4.x, p4.y, p4.z, p4.w}, me[4] = {m4.x, m4.y, m4.z, m4.w}, ve[4] = {v4.x, v4.y, v4.z, v4.w};
        const float ge[4] = {gi.x, gi.y, gi.z, gi.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) adamw_update1(pe[e], ge[e], me[e], ve[e], step, b1, b2, eps, dec, bc2s, gscale);
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
    if (guard != nullptr && guard->skip != 0) return;
    const int64_t T = (int64_t)gridDim.x * 256;
    for (int64_t i0 = blockIdx.x * 256ll; i0 < nvec; i0 += T) {
        const int64_t i = i0 + threadIdx.x;
        const int k = seg_group(map, i, i < nvec);
        if (k == SEG_SKIP) continue;
        const double t = (double)states[k].step;
        const float w = (float)(1.0 - fmin(decay, (1.0 + t) / (10.0 + t)));
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

}  // namespace

#define ST(s) ((hipStream_t)(s))

extern "C" int gdn_bn_finalize_train(const float* stats, int64_t slots, int32_t C, int64_t count, const float* gamma,
                                     const float* beta, float* running_mean, float* running_var, float momentum,
                                     float eps, float* scale, float* shift, float* mean, float* invstd,
                                     int64_t* num_batches_tracked, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!stats || slots <= 0 || C <= 0 || count <= 0 || !scale || !shift) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(bn_finalize_train_kernel, dim3(C), dim3(256), 0, ST(stream), stats, slots, C, (double)count,
                       gamma, beta, running_mean, running_var, momentum, eps, scale, shift, mean, invstd,
                       (long long*)num_batches_tracked);
    return gdn_launch_status();
}

extern "C" int gdn_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                                  const float* running_var, float eps, int32_t C, float* scale, float* shift,
                                  void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!running_mean || !running_var || C <= 0 || !scale || !shift) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3(cdiv(C, 256)), dim3(256), 0, ST(stream), gamma, beta, running_mean,
                       running_var, eps, C, scale, shift);
    return gdn_launch_status();
}

extern "C" int gdn_bn_apply(const void* y, int32_t ldy, const float* scale, const float* shift, const void* residual,
                            int32_t ld_res, void* out, int32_t ld_out, int64_t npix, int32_t C, int32_t relu,
                            int32_t dtypes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!y || !scale || !shift || !out || npix <= 0 || C <= 0) return GDN_ERR_BAD_ARG;
    if ((C % 4) || (ldy % 4) || (ld_out % 4) || (residual && (ld_res % 4))) return GDN_ERR_UNSUPPORTED;
    if (dtypes && (C % 8) == 0 && (ldy % 8) == 0 && (ld_out % 8) == 0 && (!residual || (ld_res % 8) == 0)) {
        hipLaunchKernelGGL(bn_apply8_kernel, dim3(stream_blocks(npix * (C / 8))), dim3(256), 0, ST(stream), y, ldy, scale,
                           shift, residual, ld_res, out, ld_out, npix, C, relu, dtypes, pow2_shift(C / 8));
        return gdn_launch_status();
    }
    hipLaunchKernelGGL(bn_apply_kernel, dim3(stream_blocks(npix * (C / 4))), dim3(256), 0, ST(stream), y, ldy, scale,
                       shift, residual, ld_res, out, ld_out, npix, C, relu, dtypes, pow2_shift(C / 4));
    return gdn_launch_status();
}

static int bnb_blocks(int64_t npix) {
    int64_t b = cdiv64(npix, 64);
    if (b < 1) b = 1;
    return (int)(b < BNB_MAXBLK ? b : BNB_MAXBLK);
}

extern "C" size_t gdn_bn_bwd_workspace_bytes(int64_t npix, int32_t C) {
    return ((size_t)bnb_blocks(npix) * 2 * C + 2 * (size_t)C) * sizeof(float);
}

extern "C" int gdn_bn_bwd(const void* dout, int32_t ld_dout, const void* y, int32_t ldy, const float* gamma,
                          const float* scale, const float* shift, const float* mean, const float* invstd, void* dy,
                          int32_t ld_dy, float* dgamma, float* dbeta, int64_t npix, int32_t C, int32_t relu,
                          const float* ext_partial, int64_t ext_slots,
                          void* workspace, size_t workspace_bytes, int32_t dtypes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    (void)gamma;
    if (!dout || !y || !scale || !shift || !mean || !invstd || !dy || npix <= 0 || C <= 0) return GDN_ERR_BAD_ARG;
    if (ext_partial && (ext_slots <= 0 || ext_slots > 0x7fffffff)) return GDN_ERR_BAD_ARG;
    if ((C % 4) || (ldy % 4) || (ld_dout % 4) || (ld_dy % 4)) return GDN_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < gdn_bn_bwd_workspace_bytes(npix, C)) return GDN_ERR_WORKSPACE;
    const int nblk = bnb_blocks(npix);
    float* partial = (float*)workspace;
    float* k1 = partial + (size_t)nblk * 2 * C;
    float* k2 = k1 + C;
    if (ext_partial) {
        // pass 1 already happened in the epilogue of the kernel that produced dout (gdn_winoconv_bwd / gdn_fftconv_bwd)
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0, ST(stream), ext_partial, (int)ext_slots, C,
                           (double)npix, dgamma, dbeta, k1, k2);
    } else {
        hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(nblk), dim3(256), 0, ST(stream), dout, ld_dout, y, ldy, scale, shift,
                           mean, invstd, partial, npix, C, relu, dtypes);
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0, ST(stream), (const float*)partial, nblk, C,
                           (double)npix, dgamma, dbeta, k1, k2);
    }
    if (dtypes && (C % 8) == 0 && (ldy % 8) == 0 && (ld_dout % 8) == 0 && (ld_dy % 8) == 0)
        hipLaunchKernelGGL(bn_bwd_apply8_kernel, dim3(stream_blocks(npix * (C / 8))), dim3(256), 0, ST(stream), dout,
                           ld_dout, y, ldy, scale, shift, mean, invstd, (const float*)k1, (const float*)k2, dy, ld_dy,
                           npix, C, relu, dtypes, pow2_shift(C / 8));
    else
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(stream_blocks(npix * (C / 4))), dim3(256), 0, ST(stream), dout,
                       ld_dout, y, ldy, scale, shift, mean, invstd, (const float*)k1, (const float*)k2, dy, ld_dy, npix,
                       C, relu, dtypes, pow2_shift(C / 4));
    return gdn_launch_status();
}

// Passes 1 + 2 only: dgamma, dbeta and kk = {k1 = mean(dz), k2 = mean(dz*xhat)}[C] for a consumer that applies pass 3 itself while
// loading (gdn_fftconv_bwd's dyb_* arguments).  ext_partial as in gdn_bn_bwd.
extern "C" int gdn_bn_bwd_coeffs(const void* dout, int32_t ld_dout, const void* y, int32_t ldy, const float* scale,
                                 const float* shift, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                                 float* kk, int64_t npix, int32_t C, int32_t relu, const float* ext_partial,
                                 int64_t ext_slots, void* workspace, size_t workspace_bytes, int32_t dtypes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!scale || !shift || !mean || !invstd || !kk || npix <= 0 || C <= 0) return GDN_ERR_BAD_ARG;
    if (ext_partial && (ext_slots <= 0 || ext_slots > 0x7fffffff)) return GDN_ERR_BAD_ARG;
    if (ext_partial) {
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0, ST(stream), ext_partial, (int)ext_slots, C,
                           (double)npix, dgamma, dbeta, kk, kk + C);
        return gdn_launch_status();
    }
    if (!dout || !y) return GDN_ERR_BAD_ARG;
    if ((C % 4) || (ldy % 4) || (ld_dout % 4)) return GDN_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < gdn_bn_bwd_workspace_bytes(npix, C)) return GDN_ERR_WORKSPACE;
    const int nblk = bnb_blocks(npix);
    float* partial = (float*)workspace;
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(nblk), dim3(256), 0, ST(stream), dout, ld_dout, y, ldy, scale, shift,
                       mean, invstd, partial, npix, C, relu, dtypes);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0, ST(stream), (const float*)partial, nblk, C,
                       (double)npix, dgamma, dbeta, kk, kk + C);
    return gdn_launch_status();
}

// Backward of out = [relu](y*scale + shift) with FIXED per-channel coefficients (eval-mode BatchNorm of a frozen
// network): dy = scale * dout * [z > 0].  No reductions, no parameter gradients.
__global__ __launch_bounds__(256) void bn_eval_bwd_kernel(const void* __restrict__ dout, int ld_dout,
                                                          const void* __restrict__ y, int ldy,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift, void* __restrict__ dy,
                                                          int ld_dy, int64_t npix, int C, int relu, int dt, int sh) {
    const int cq = C >> 2;
    const int64_t total = npix * cq;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        SPLIT_PIX_C(i, cq, sh, pix, c);
        const f32x4 d = ld4_any(dout, pix * ld_dout + c, dt & 1);
        const f32x4 s = *reinterpret_cast<const f32x4*>(scale + c);
        f32x4 o = d * s;
        if (relu) {
            const f32x4 v = ld4_any(y, pix * ldy + c, dt & 2);
            const f32x4 t = *reinterpret_cast<const f32x4*>(shift + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // relu == 2: y already IS the activated output (conv + BN + ReLU fused in the conv epilogue)
                const bool on = relu == 2 ? v[e] > 0.f : v[e] * s[e] + t[e] > 0.f;
                if (!on) o[e] = 0.f;
            }
        }
        st4_any(dy, pix * ld_dy + c, o, dt & 4);
    }
}

extern "C" int gdn_bn_eval_bwd(const void* dout, int32_t ld_dout, const void* y, int32_t ldy, const float* scale,
                               const float* shift, void* dy, int32_t ld_dy, int64_t npix, int32_t C, int32_t relu,
                               int32_t dtypes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!dout || !y || !scale || !shift || !dy || npix <= 0 || C <= 0) return GDN_ERR_BAD_ARG;
    if ((C % 4) || (ldy % 4) || (ld_dout % 4) || (ld_dy % 4)) return GDN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(bn_eval_bwd_kernel, dim3(stream_blocks(npix * (C / 4))), dim3(256), 0, ST(stream), dout, ld_dout,
                       y, ldy, scale, shift, dy, ld_dy, npix, C, relu, dtypes, pow2_shift(C / 4));
    return gdn_launch_status();
}

// ------------------------------------------------ BN backward on FROZEN statistics
// A trained layer whose BatchNorm stays in eval(): out = [relu](y*scale + shift) with scale / shift from the RUNNING statistics.
// dy = scale * dout * [z > 0] depends on no reduction, so one pass reads dout and y once, writes dy and leaves the per-block
// sums of dz and dz*xhat (xhat = (y - running_mean) * invstd) that bn_bwd_finalize_kernel turns into dbeta / dgamma.
__global__ void bn_frozen_coeffs_kernel(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                                        int C, float* scale, float* shift, float* mean, float* invstd) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    // (scale / shift: bn_eval_coeffs_kernel's expressions, letter for letter -- the two must agree to the bit)
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    const float inv = 1.0f / sqrtf(rv[c] + eps);
    scale[c] = g * inv;
    shift[c] = b - rm[c] * g * inv;
    mean[c] = rm[c];
    invstd[c] = inv;
}

#define BNF_MAXBLK 2048
// bn_bwd_reduce_kernel's block layout -- channel-vector lanes x pixel lanes over one contiguous pixel range per block, the same
// 8 KB of LDS -- with the dy store added.  NH: 4-channel halves per lane (1: 16 bytes of fp32; 2: 16 bytes of bf16).
// partial[blk][2][C]: a lane sums its pixels in order, lane 0 of each channel vector adds the pixel lanes in order -- a fixed
// order, no atomics.  DY: dy is written, with bn_eval_bwd_kernel's arithmetic.
template <int NH, bool DY>
__global__ __launch_bounds__(256) void bn_frozen_bwd_kernel(
    const void* __restrict__ dout, int ld_dout, const void* __restrict__ y, int ldy,
    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
    const float* __restrict__ invstd, void* __restrict__ dy, int ld_dy, float* __restrict__ partial, int64_t npix, int C,
    int relu, int dt) {
    __shared__ float sh[256 * 8];
    const int cv = C / (4 * NH);
    const int CQ = cv < 256 ? cv : 256;      // channel-vector lanes
    const int PY = 256 / CQ;                 // pixel lanes
    const int tx = threadIdx.x % CQ, ty = threadIdx.x / CQ;
    const int64_t per = cdiv64(npix, gridDim.x);
    const int64_t p0 = blockIdx.x * per, p1 = (p0 + per < npix) ? p0 + per : npix;
    for (int q0 = 0; q0 < cv; q0 += CQ) {    // (uniform trip count: the barriers below are reached by every lane)
        const int q = q0 + tx;
        const bool lane = ty < PY && q < cv;
        const int c = q * 4 * NH;
        f32x4 a1[NH], a2[NH];
#pragma unroll
        for (int h = 0; h < NH; ++h) { a1[h] = f32x4{0.f, 0.f, 0.f, 0.f}; a2[h] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        if (lane) {
            f32x4 s[NH], t[NH], mu[NH], is[NH];
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                s[h] = *reinterpret_cast<const f32x4*>(scale + c + 4 * h);
                t[h] = *reinterpret_cast<const f32x4*>(shift + c + 4 * h);
                mu[h] = *reinterpret_cast<const f32x4*>(mean + c + 4 * h);
                is[h] = *reinterpret_cast<const f32x4*>(invstd + c + 4 * h);
            }
            for (int64_t pix = p0 + ty; pix < p1; pix += PY) {
                f32x4 d[NH], v[NH], o[NH];
                if (NH == 2) ld8_any(dout, pix * ld_dout + c, dt & 1, d[0], d[NH - 1]);
                else d[0] = ld4_any(dout, pix * ld_dout + c, dt & 1);
                if (NH == 2) ld8_any(y, pix * ldy + c, dt & 2, v[0], v[NH - 1]);
                else v[0] = ld4_any(y, pix * ldy + c, dt & 2);
#pragma unroll
                for (int h = 0; h < NH; ++h) {
                    o[h] = d[h] * s[h];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float dz = d[h][e];
                        if (relu) {
                            const bool on = v[h][e] * s[h][e] + t[h][e] > 0.f;
                            if (!on) { o[h][e] = 0.f; dz = 0.f; }
                        }
                        a1[h][e] += dz;
                        a2[h][e] += dz * ((v[h][e] - mu[h][e]) * is[h][e]);
                    }
                }
                if (DY) {
                    if (NH == 2) st8_any(dy, pix * ld_dy + c, o[0], o[NH - 1], dt & 4);
                    else st4_any(dy, pix * ld_dy + c, o[0], dt & 4);
                }
            }
        }
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 4; ++e) { sh[threadIdx.x * 8 + e] = a1[h][e]; sh[threadIdx.x * 8 + 4 + e] = a2[h][e]; }
            __syncthreads();
            if (ty == 0 && q < cv) {
                f32x4 r1 = {0.f, 0.f, 0.f, 0.f}, r2 = {0.f, 0.f, 0.f, 0.f};
                for (int j = 0; j < PY; ++j) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { r1[e] += sh[(j * CQ + tx) * 8 + e]; r2[e] += sh[(j * CQ + tx) * 8 + 4 + e]; }
                }
                *reinterpret_cast<f32x4*>(partial + ((size_t)blockIdx.x * 2 + 0) * C + c + 4 * h) = r1;
                *reinterpret_cast<f32x4*>(partial + ((size_t)blockIdx.x * 2 + 1) * C + c + 4 * h) = r2;
            }
        }
    }
}

// The dy pass alone (the sums came from the producer of dout): nothing is reduced, so it is the flat grid-stride stream of
// bn_eval_bwd_kernel -- that kernel itself for 4-channel lanes, this one for the 16-byte bf16 lanes; the same arithmetic.
__global__ __launch_bounds__(256) void bn_frozen_apply8_kernel(const void* __restrict__ dout, int ld_dout,
                                                               const void* __restrict__ y, int ldy,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift, void* __restrict__ dy,
                                                               int ld_dy, int64_t npix, int C, int relu, int dt, int sh) {
    const int co = C >> 3;
    const int64_t total = npix * co;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t pix = sh >= 0 ? (i >> sh) : i / co;
        const int c = (int)(sh >= 0 ? (i & (co - 1)) : (i - pix * co)) * 8;
        f32x4 d[2], v[2], o[2];
        ld8_any(dout, pix * ld_dout + c, dt & 1, d[0], d[1]);
        if (relu) ld8_any(y, pix * ldy + c, dt & 2, v[0], v[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 s = *reinterpret_cast<const f32x4*>(scale + c + 4 * h);
            o[h] = d[h] * s;
            if (relu) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(shift + c + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool on = v[h][e] * s[e] + t[e] > 0.f;
                    if (!on) o[h][e] = 0.f;
                }
            }
        }
        st8_any(dy, pix * ld_dy + c, o[0], o[1], dt & 4);
    }
}

static int bnf_blocks(int64_t npix) {
    int64_t b = cdiv64(npix, 64);
    if (b < 1) b = 1;
    return (int)(b < BNF_MAXBLK ? b : BNF_MAXBLK);
}

template <int NH>
static void bnf_launch(bool wdy, int nblk, hipStream_t st, const void* dout, int ld_dout, const void* y, int ldy,
                       const float* scale, const float* shift, const float* mean, const float* invstd, void* dy, int ld_dy,
                       float* partial, int64_t npix, int C, int relu, int dt) {
#define BNF_GO(D)                                                                                                      \
    hipLaunchKernelGGL((bn_frozen_bwd_kernel<NH, D>), dim3(nblk), dim3(256), 0, st, dout, ld_dout, y, ldy, scale, shift, \
                       mean, invstd, dy, ld_dy, partial, npix, C, relu, dt)
    if (wdy) BNF_GO(true);
    else BNF_GO(false);
#undef BNF_GO
}

extern "C" int gdn_bn_frozen_coeffs(const float* gamma, const float* beta, const float* running_mean,
                                    const float* running_var, float eps, int32_t C, float* scale, float* shift,
                                    float* mean, float* invstd, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!running_mean || !running_var || C <= 0 || !scale || !shift || !mean || !invstd) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(bn_frozen_coeffs_kernel, dim3(cdiv(C, 256)), dim3(256), 0, ST(stream), gamma, beta, running_mean,
                       running_var, eps, C, scale, shift, mean, invstd);
    return gdn_launch_status();
}

extern "C" size_t gdn_bn_frozen_bwd_workspace_bytes(int64_t npix, int32_t C) {
    return ((size_t)bnf_blocks(npix) * 2 * C + 2 * (size_t)C) * sizeof(float);   // partials + the finalize kernel's two means
}

extern "C" int gdn_bn_frozen_bwd(const void* dout, int32_t ld_dout, const void* y, int32_t ldy, const float* scale,
                                 const float* shift, const float* mean, const float* invstd, void* dy, int32_t ld_dy,
                                 float* dgamma, float* dbeta, int64_t npix, int32_t C, int32_t relu,
                                 const float* ext_partial, int64_t ext_slots, void* workspace, size_t workspace_bytes,
                                 int32_t dtypes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!scale || !shift || !mean || !invstd || npix <= 0 || C <= 0) return GDN_ERR_BAD_ARG;
    if (ext_partial && (ext_slots <= 0 || ext_slots > 0x7fffffff)) return GDN_ERR_BAD_ARG;
    const bool want_sums = dgamma || dbeta;
    const bool sums = want_sums && !ext_partial;         // this call reduces itself
    if ((dy || sums) && (!dout || !y)) return GDN_ERR_BAD_ARG;
    if ((C % 4) || (ldy % 4) || (ld_dout % 4) || (dy && (ld_dy % 4))) return GDN_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < gdn_bn_frozen_bwd_workspace_bytes(npix, C)) return GDN_ERR_WORKSPACE;
    const int nblk = bnf_blocks(npix);
    float* partial = (float*)workspace;
    float* k1 = partial + (size_t)nblk * 2 * C;
    float* k2 = k1 + C;
    const bool wide = dtypes && (C % 8) == 0 && (ldy % 8) == 0 && (ld_dout % 8) == 0 && (!dy || (ld_dy % 8) == 0);
    if (dy && !sums) {
        if (wide)
            hipLaunchKernelGGL(bn_frozen_apply8_kernel, dim3(stream_blocks(npix * (C / 8))), dim3(256), 0, ST(stream), dout,
                               ld_dout, y, ldy, scale, shift, dy, ld_dy, npix, C, relu ? 1 : 0, dtypes, pow2_shift(C / 8));
        else
            hipLaunchKernelGGL(bn_eval_bwd_kernel, dim3(stream_blocks(npix * (C / 4))), dim3(256), 0, ST(stream), dout,
                               ld_dout, y, ldy, scale, shift, dy, ld_dy, npix, C, relu ? 1 : 0, dtypes, pow2_shift(C / 4));
    } else if (sums) {
        if (wide)
            bnf_launch<2>(dy != nullptr, nblk, ST(stream), dout, ld_dout, y, ldy, scale, shift, mean, invstd, dy, ld_dy,
                          partial, npix, C, relu ? 1 : 0, dtypes);
        else
            bnf_launch<1>(dy != nullptr, nblk, ST(stream), dout, ld_dout, y, ldy, scale, shift, mean, invstd, dy, ld_dy,
                          partial, npix, C, relu ? 1 : 0, dtypes);
    }
    if (want_sums)
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0, ST(stream),
                           ext_partial ? ext_partial : (const float*)partial, ext_partial ? (int)ext_slots : nblk, C,
                           (double)npix, dgamma, dbeta, k1, k2);
    return gdn_launch_status();
}

extern "C" int gdn_upsample2x_fwd(const void* x, void* y, int32_t B, int32_t H, int32_t W, int32_t C,
                                  int32_t align_corners, int32_t dtypes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0) return GDN_ERR_BAD_ARG;
    if (C % 4) return GDN_ERR_UNSUPPORTED;
    if ((int64_t)B * 2 * H > 65535) return GDN_ERR_UNSUPPORTED;      // grid.y limit
    hipLaunchKernelGGL(upsample2x_fwd_kernel, dim3(cdiv(2 * W * (C / 4), 256), B * 2 * H), dim3(256), 0,
                       ST(stream), x, y, B, H, W, C, align_corners, dtypes, pow2_shift(C / 4));
    return gdn_launch_status();
}

extern "C" int gdn_bn_apply_up2x(const void* y, const float* scale, const float* shift, const void* residual, void* low,
                                 void* up, int32_t B, int32_t H, int32_t W, int32_t C, int32_t relu, int32_t align_corners,
                                 int32_t dtypes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!y || !scale || !shift || !up || B <= 0 || H <= 0 || W <= 0 || C <= 0) return GDN_ERR_BAD_ARG;
    if (C % 4) return GDN_ERR_UNSUPPORTED;
    if ((int64_t)B * 2 * H > 65535) return GDN_ERR_UNSUPPORTED;      // grid.y limit
    if ((C % 8) == 0 && C <= 1024 && B <= 65535) {
        // tiles: TXL low-resolution columns x all channels per workgroup, RC rows per workgroup (more where the tensor is large
        // enough to still give every CU several workgroups: a workgroup re-reads one halo row above and below its range)
        const int TXL = 256 / (C / 8), nbx = cdiv(W, TXL);
        int RC = 16;
        while (RC > 2 && (int64_t)B * nbx * cdiv(H, RC) < 2048) RC >>= 1;
        const size_t lds = (size_t)3 * (TXL + 2) * C * sizeof(float);
        hipLaunchKernelGGL(bn_apply_up2x8_kernel, dim3(nbx, cdiv(H, RC), B), dim3(256), lds, ST(stream), y, scale, shift, residual,
                           low, up, B, H, W, C, relu, align_corners, dtypes, TXL, RC);
        return gdn_launch_status();
    }
    hipLaunchKernelGGL(bn_apply_up2x_kernel, dim3(cdiv(2 * W * (C / 4), 256), B * 2 * H), dim3(256), 0, ST(stream), y, scale,
                       shift, residual, low, up, B, H, W, C, relu, align_corners, dtypes, pow2_shift(C / 4));
    return gdn_launch_status();
}

extern "C" int gdn_upsample2x_bwd(const void* dy, void* dx, int32_t B, int32_t H, int32_t W, int32_t C,
                                  int32_t align_corners, int32_t dtypes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!dy || !dx || B <= 0 || H <= 0 || W <= 0 || C <= 0) return GDN_ERR_BAD_ARG;
    if (C % 4) return GDN_ERR_UNSUPPORTED;
    if ((int64_t)B * H > 65535) return GDN_ERR_UNSUPPORTED;          // grid.y limit
    hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3(cdiv(W * (C / 4), 256), B * H), dim3(256), 0,
                       ST(stream), dy, dx, B, H, W, C, align_corners, dtypes, pow2_shift(C / 4));
    return gdn_launch_status();
}

extern "C" int gdn_nchw_to_nhwc(const void* x, void* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t dtypes,
                                void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!x || !y || B <= 0 || C <= 0 || H <= 0 || W <= 0) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(stream_blocks((int64_t)B * C * H * W)), dim3(256), 0, ST(stream), x, y,
                       B, C, H * W, dtypes);
    return gdn_launch_status();
}
extern "C" int gdn_nhwc_to_nchw(const void* x, void* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t dtypes,
                                void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!x || !y || B <= 0 || C <= 0 || H <= 0 || W <= 0) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(stream_blocks((int64_t)B * C * H * W)), dim3(256), 0, ST(stream), x, y,
                       B, C, H * W, dtypes);
    return gdn_launch_status();
}

extern "C" int gdn_transpose_taps(const void* w, void* wt, int32_t ntaps, int32_t R, int32_t C, int32_t dtypes,
                                  void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!w || !wt || ntaps <= 0 || R <= 0 || C <= 0) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(transpose_taps_kernel, dim3(cdiv(C, 32), cdiv(R, 32), ntaps), dim3(256), 0, ST(stream), w, wt, R,
                       C, dtypes);
    return gdn_launch_status();
}

extern "C" int gdn_weight_to_tapmajor(const float* w_torch, float* w_tap, int32_t Cout, int32_t Cin, int32_t ntaps,
                                      int32_t a_is_cout, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!w_torch || !w_tap || Cout <= 0 || Cin <= 0 || ntaps <= 0) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(weight_tapmajor_kernel, dim3(stream_blocks((int64_t)Cout * Cin * ntaps)), dim3(256), 0,
                       ST(stream), w_torch, w_tap, Cout, Cin, ntaps, a_is_cout, 1);
    return gdn_launch_status();
}
extern "C" int gdn_weight_from_tapmajor(const float* w_tap, float* w_torch, int32_t Cout, int32_t Cin, int32_t ntaps,
                                        int32_t a_is_cout, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!w_torch || !w_tap || Cout <= 0 || Cin <= 0 || ntaps <= 0) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(weight_tapmajor_kernel, dim3(stream_blocks((int64_t)Cout * Cin * ntaps)), dim3(256), 0,
                       ST(stream), w_tap, w_torch, Cout, Cin, ntaps, a_is_cout, 0);
    return gdn_launch_status();
}

extern "C" int gdn_add(const void* a, const void* b, void* out, int64_t n, int32_t dtypes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!a || !b || !out || n <= 0) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(add_kernel, dim3(stream_blocks(n / 4 + 1)), dim3(256), 0, ST(stream), a, b, out, n, dtypes);
    return gdn_launch_status();
}
extern "C" int gdn_add_pitched(const void* a, int32_t lda, const void* b, int32_t ldb, void* out, int32_t ld_out,
                               int64_t npix, int32_t C, int32_t dtypes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!a || !out || npix <= 0 || C <= 0) return GDN_ERR_BAD_ARG;
    if ((C % 4) || (lda % 4) || (ld_out % 4) || (b && (ldb % 4))) return GDN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(add_pitched_kernel, dim3(stream_blocks(npix * (C / 4))), dim3(256), 0, ST(stream), a, lda, b, ldb, out,
                       ld_out, npix, C, dtypes, pow2_shift(C / 4));
    return gdn_launch_status();
}

extern "C" int gdn_scale_dev(const float* x, const float* s, float* out, int64_t n, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!x || !s || !out || n <= 0) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(scale_dev_kernel, dim3(stream_blocks(n)), dim3(256), 0, ST(stream), x, s, out, n);
    return gdn_launch_status();
}

extern "C" int gdn_cast(const void* src, void* dst, int64_t n, int32_t dtypes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!src || !dst || n <= 0) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(cast_kernel, dim3(stream_blocks(n / 4 + 1, 256, 4096)), dim3(256), 0, ST(stream), src, dst, n, dtypes);
    return gdn_launch_status();
}
extern "C" int gdn_tanh_bwd(const float* dout, const float* out, float* dpre, int64_t n, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!dout || !out || !dpre || n <= 0) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(tanh_bwd_kernel, dim3(stream_blocks(n)), dim3(256), 0, ST(stream), dout, out, dpre, n);
    return gdn_launch_status();
}
extern "C" int gdn_fill(float* p, float value, int64_t n, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!p || n <= 0) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(fill_kernel, dim3(stream_blocks(n)), dim3(256), 0, ST(stream), p, value, n);
    return gdn_launch_status();
}

extern "C" int gdn_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int32_t step, float grad_scale, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!p || !g || !m || !v || n <= 0 || step < 1) return GDN_ERR_BAD_ARG;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(adam_kernel, dim3(stream_blocks(n, 256, 4096)), dim3(256), 0, ST(stream), p, g, m, v, n, lr,
                       beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), grad_scale);
    return gdn_launch_status();
}

// gdn_adam_step_dev (guard null) and gdn_adam_step_dev_guarded: the prep launch for the one state, then the update
static void adam_dev_launch(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, void* state,
                            const void* guard, void* stream) {
    hipLaunchKernelGGL(adam_prep_kernel, dim3(1), adam_prep_block(1), 0, ST(stream), (AdamDevState*)state, hyper, 1,
                       (const AdamGuard*)guard);
    hipLaunchKernelGGL(adam_dev_kernel, dim3(stream_blocks(n, 256, 4096)), dim3(256), 0, ST(stream), p, g, m, v, n, hyper,
                       (const AdamDevState*)state, (const AdamGuard*)guard);
}
extern "C" int gdn_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, void* state,
                                 void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!p || !g || !m || !v || n <= 0 || !hyper || !state) return GDN_ERR_BAD_ARG;
    adam_dev_launch(p, g, m, v, n, hyper, state, nullptr, stream);
    return gdn_launch_status();
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
extern "C" int gdn_adam_step_dev_guarded(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                                         void* state, const void* guard, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!p || !g || !m || !v || n <= 0 || !hyper || !state || !guard) return GDN_ERR_BAD_ARG;
    adam_dev_launch(p, g, m, v, n, hyper, state, guard, stream);
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

// ---- segmented Adam family (include/gdn_hip.h).  The map's CONTENTS are the caller's: entries < G or 0xFF.
static bool seg_bad_range(int64_t n, const void* map, const void* a, const void* b, const void* c, const void* d) {
    return n <= 0 || (n & 63) != 0 || !map || (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) != 0;
}
extern "C" int gdn_adam_step_seg(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* map, int32_t G,
                                 const float* hyper, void* states, const void* guard, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!p || !g || !m || !v || !hyper || !states || G < 1 || G > 254 || seg_bad_range(n, map, p, g, m, v)) return GDN_ERR_BAD_ARG;
    if (((uintptr_t)hyper & 3) || ((uintptr_t)states & 7) || ((uintptr_t)guard & 7)) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(adam_prep_kernel, dim3(1), adam_prep_block(G), 0, ST(stream), (AdamDevState*)states, hyper, (int)G,
                       (const AdamGuard*)guard);
    hipLaunchKernelGGL(adam_seg_kernel, dim3(stream_rw_blocks(n, true)), dim3(256), 0, ST(stream), (f32x4*)p, (const f32x4*)g,
                       (f32x4*)m, (f32x4*)v, n / 4, map, hyper, (const AdamDevState*)states, (const AdamGuard*)guard);
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

// ---- decoupled weight decay: the four update entry points again, argument lists, checks and launch geometry of their coupled
// counterparts, the prep launch shared with them
extern "C" int gdn_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int32_t step, float grad_scale, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!p || !g || !m || !v || n <= 0 || step < 1) return GDN_ERR_BAD_ARG;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(adamw_kernel, dim3(stream_blocks(n, 256, 4096)), dim3(256), 0, ST(stream), p, g, m, v, n, lr,
                       beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), grad_scale);
    return gdn_launch_status();
}
static void adamw_dev_launch(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, void* state,
                             const void* guard, void* stream) {
    hipLaunchKernelGGL(adam_prep_kernel, dim3(1), adam_prep_block(1), 0, ST(stream), (AdamDevState*)state, hyper, 1,
                       (const AdamGuard*)guard);
    hipLaunchKernelGGL(adamw_dev_kernel, dim3(stream_blocks(n, 256, 4096)), dim3(256), 0, ST(stream), p, g, m, v, n, hyper,
                       (const AdamDevState*)state, (const AdamGuard*)guard);
}
extern "C" int gdn_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, void* state,
                                  void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!p || !g || !m || !v || n <= 0 || !hyper || !state) return GDN_ERR_BAD_ARG;
    adamw_dev_launch(p, g, m, v, n, hyper, state, nullptr, stream);
    return gdn_launch_status();
}
extern "C" int gdn_adamw_step_dev_guarded(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                                          void* state, const void* guard, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!p || !g || !m || !v || n <= 0 || !hyper || !state || !guard) return GDN_ERR_BAD_ARG;
    adamw_dev_launch(p, g, m, v, n, hyper, state, guard, stream);
    return gdn_launch_status();
}
extern "C" int gdn_adamw_step_seg(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* map, int32_t G,
                                  const float* hyper, void* states, const void* guard, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!p || !g || !m || !v || !hyper || !states || G < 1 || G > 254 || seg_bad_range(n, map, p, g, m, v)) return GDN_ERR_BAD_ARG;
    if (((uintptr_t)hyper & 3) || ((uintptr_t)states & 7) || ((uintptr_t)guard & 7)) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(adam_prep_kernel, dim3(1), adam_prep_block(G), 0, ST(stream), (AdamDevState*)states, hyper, (int)G,
                       (const AdamGuard*)guard);
    hipLaunchKernelGGL(adamw_seg_kernel, dim3(stream_rw_blocks(n, true)), dim3(256), 0, ST(stream), (f32x4*)p, (const f32x4*)g,
                       (f32x4*)m, (f32x4*)v, n / 4, map, hyper, (const AdamDevState*)states, (const AdamGuard*)guard);
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

// ---- shader-clock probe (measurement aid; include/gdn_hip.h) -----------------------------------------------------------------
// One wave: reads the shader cycle counter (s_memtime) and the constant 100 MHz counter (s_memrealtime), sleeps until the flag
// word is set by clock_probe_set_kernel on the measured stream (or max_ticks have passed), reads both again.
// buf must be HOST-PINNED memory mapped into the device (hipHostMalloc / a pinned torch tensor): the setter and the watcher
// usually run on different XCDs, whose L2s are not coherent with each other for ordinary device memory inside a kernel -- an
// agent-scope load kept hitting the watcher's own stale line (the r06 full-suite run: the watcher ran into its tick limit) and
// polling with L2 invalidates would disturb the kernels being measured.  Host memory is uncached: every poll reads the flag.
__global__ __launch_bounds__(64) void clock_probe_kernel(unsigned long long* __restrict__ buf, unsigned long long max_ticks) {
    if (threadIdx.x != 0) return;
    const unsigned long long c0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long r1 = r0;
    while (__hip_atomic_load(buf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0ull && r1 - r0 < max_ticks) {
        __builtin_amdgcn_s_sleep(64);
        r1 = __builtin_amdgcn_s_memrealtime();
    }
    const unsigned long long c1 = __builtin_readcyclecounter();
    r1 = __builtin_amdgcn_s_memrealtime();
    buf[1] = c1 - c0;
    buf[2] = r1 - r0;
    buf[3] = __hip_atomic_load(buf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // 1: ended by the flag, 0: by the tick limit
}
__global__ void clock_probe_set_kernel(unsigned long long* buf, unsigned long long v) {
    __hip_atomic_store(buf, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (v == 0ull) { buf[1] = 0ull; buf[2] = 0ull; buf[3] = 0ull; }
}

extern "C" int gdn_clock_probe_arm(uint64_t* buf, void* stream) {
    (void)hipGetLastError();
    if (!buf) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(clock_probe_set_kernel, dim3(1), dim3(1), 0, ST(stream), (unsigned long long*)buf, 0ull);
    return gdn_launch_status();
}
extern "C" int gdn_clock_probe_watch(uint64_t* buf, uint64_t max_ticks, void* side_stream) {
    (void)hipGetLastError();
    if (!buf || max_ticks == 0 || max_ticks > 1000000000ull) return GDN_ERR_BAD_ARG;      // at most 10 s
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, ST(side_stream), (unsigned long long*)buf,
                       (unsigned long long)max_ticks);
    return gdn_launch_status();
}
extern "C" int gdn_clock_probe_stop(uint64_t* buf, void* stream) {
    (void)hipGetLastError();
    if (!buf) return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(clock_probe_set_kernel, dim3(1), dim3(1), 0, ST(stream), (unsigned long long*)buf, 1ull);
    return gdn_launch_status();
}

extern "C" int gdn_version(void) { return 223; }
extern "C" int gdn_hints_supported(void) {
    return GDN_HINT_TRAIN | GDN_HINT_NO_X3 | GDN_HINT_NO_WINO_F4 | GDN_HINT_FFT_NP32 | GDN_HINT_FFT_NP40 | GDN_HINT_FLIP_TAPS |
           GDN_HINT_PLAN_BATCH(0xff) | GDN_HINT_PLAN_CUS(2040);
}

extern "C" const char* gdn_strerror(int status) {
    switch (status) {
        case GDN_OK: return "ok";
        case GDN_ERR_BAD_ARG: return "bad argument";
        case GDN_ERR_UNSUPPORTED: return "unsupported shape/alignment";
        case GDN_ERR_WORKSPACE: return "workspace missing or too small";
        case GDN_ERR_LAUNCH: return "kernel launch failed";
        default: return "unknown error";
    }
}

extern "C" int gdn_device_info(char* name, int name_len) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return GDN_ERR_LAUNCH;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return GDN_ERR_LAUNCH;
    if (name && name_len > 0) {
        int i = 0;
        for (; i < name_len - 1 && prop.gcnArchName[i]; ++i) name[i] = prop.gcnArchName[i];
        name[i] = 0;
    }
    return prop.multiProcessorCount;
}
