// HBM-bound glue kernels of the GDN hot path for gfx950: BatchNorm finalize /
// apply / backward, x2 bilinear up-sampling, layout transforms, elementwise.
// All are 16-byte-per-lane streaming kernels (NHWC, channel count % 4 == 0).
// The optimizer's kernels are in optim.hip.
#include "common.h"
#include "bn_math.h"
#include "up2x.h"

namespace {

// log2 of v if v is a power of two, else -1: the channel-vector counts of these networks (16..128) all are, which turns
// the per-element 64-bit division of the flat index into a shift (bn_split, bn_math.h).
inline int pow2_shift(int v) {
    for (int s = 0; s < 31; ++s)
        if ((1 << s) == v) return s;
    return -1;
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

// scale / shift of a BatchNorm applied with its RUNNING statistics (eval mode, frozen layers); returns invstd
__device__ __forceinline__ float bn_running_coeffs(const float* gamma, const float* beta, const float* rm, const float* rv,
                                                   float eps, int c, float* scale, float* shift) {
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    const float inv = 1.0f / sqrtf(rv[c] + eps);
    scale[c] = g * inv;
    shift[c] = b - rm[c] * g * inv;
    return inv;
}

__global__ void bn_eval_coeffs_kernel(const float* gamma, const float* beta, const float* rm, const float* rv,
                                      float eps, int C, float* scale, float* shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    bn_running_coeffs(gamma, beta, rm, rv, eps, c, scale, shift);
}

// out = [relu](y * scale + shift) (+ residual).  NH = 2 for bf16 tensors: 8 channels per lane, 16-byte accesses.
template <int NH>
__global__ __launch_bounds__(256) void bn_apply_kernel(const void* __restrict__ y, int ldy,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift,
                                                       const void* __restrict__ res, int ld_res,
                                                       void* __restrict__ out, int ld_out, int64_t npix, int C,
                                                       int relu, int dt, int sh) {
    const int cv = C / (4 * NH);
    const int64_t total = npix * cv;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t pix; int c;
        bn_split<NH>(i, cv, sh, pix, c);
        BnLane<NH> s, t, o;
        o.load(y, pix * ldy + c, dt & 1);
        s.coef(scale, c);
        t.coef(shift, c);
        o.act(s, t, relu, res, pix * ld_res + c, dt & 2, 0);
        o.store(out, pix * ld_out + c, dt & 4);
    }
}

// ----------------------------------------------------------------- BN backward
#define BNB_MAXBLK 1024      // blocks of pass 1 on batch statistics (gdn_bn_bwd, gdn_bn_bwd_coeffs)
#define BNF_MAXBLK 2048      // ... on frozen statistics (gdn_bn_frozen_bwd)
// pass 1: partial[blk][2][C] = sum over the block's pixels of dz, dz*xhat; with DY also dy = scale * dz, the whole backward of
// a BatchNorm on FROZEN statistics (no reduction feeds back into dy).  Channel-vector lanes x pixel lanes over one contiguous
// pixel range per block, 8 KB of LDS.  A lane sums its pixels in order, lane 0 of each channel vector adds the pixel lanes in
// order (bn_lane_reduce): a fixed order, no atomics.
template <int NH, bool DY>
__global__ __launch_bounds__(256) void bn_bwd_sums_kernel(
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
    for (int q0 = 0; q0 < cv; q0 += CQ) {    // (uniform trip count: bn_lane_reduce's barriers are reached by every lane)
        const int q = q0 + tx;
        const bool lane = ty < PY && q < cv;
        const int c = q * 4 * NH;
        BnLane<NH> a1, a2;
        a1.zero();
        a2.zero();
        if (lane) {
            BnLane<NH> s, t, mu, is;
            s.coef(scale, c);
            t.coef(shift, c);
            mu.coef(mean, c);
            is.coef(invstd, c);
            for (int64_t pix = p0 + ty; pix < p1; pix += PY) {
                BnLane<NH> d, v, o;
                d.load(dout, pix * ld_dout + c, dt & 1);
                v.load(y, pix * ldy + c, dt & 2);
#pragma unroll
                for (int k = 0; k < NH; ++k) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float dz = bn_dz(d.h[k][e], v.h[k][e], s.h[k][e], t.h[k][e], relu);
                        if constexpr (DY) o.h[k][e] = bn_fixed_dy(d.h[k][e], v.h[k][e], s.h[k][e], t.h[k][e], relu);
                        a1.h[k][e] += dz;
                        a2.h[k][e] += dz * bn_xhat(v.h[k][e], mu.h[k][e], is.h[k][e]);
                    }
                }
                if constexpr (DY) o.store(dy, pix * ld_dy + c, dt & 4);
            }
        }
#pragma unroll
        for (int k = 0; k < NH; ++k) {
            float* dst = ty == 0 && q < cv ? partial + (size_t)blockIdx.x * 2 * C + c + 4 * k : nullptr;
            bn_lane_reduce(sh, a1.h[k], a2.h[k], tx, ty, CQ, PY, dst, dst + C);
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
template <int NH>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(
    const void* __restrict__ dout, int ld_dout, const void* __restrict__ y, int ldy,
    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ k1, const float* __restrict__ k2,
    void* __restrict__ dy, int ld_dy, int64_t npix, int C, int relu, int dt, int sh) {
    const int cv = C / (4 * NH);
    const int64_t total = npix * cv;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t pix; int c;
        bn_split<NH>(i, cv, sh, pix, c);
        BnLane<NH> d, v, s, t, mu, is, a, b, o;
        d.load(dout, pix * ld_dout + c, dt & 1);
        v.load(y, pix * ldy + c, dt & 2);
        s.coef(scale, c);      // gamma*invstd
        t.coef(shift, c);
        mu.coef(mean, c);
        is.coef(invstd, c);
        a.coef(k1, c);
        b.coef(k2, c);
#pragma unroll
        for (int k = 0; k < NH; ++k) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dz = bn_dz(d.h[k][e], v.h[k][e], s.h[k][e], t.h[k][e], relu);
                o.h[k][e] = bn_bwd_dy(dz, bn_xhat(v.h[k][e], mu.h[k][e], is.h[k][e]), s.h[k][e], a.h[k][e], b.h[k][e]);
            }
        }
        o.store(dy, pix * ld_dy + c, dt & 4);
    }
}

// Backward of out = [relu](y*scale + shift) with FIXED per-channel coefficients (eval-mode BatchNorm of a frozen network, or
// a trained layer whose BatchNorm stays in eval() and whose sums came from the producer of dout): dy = scale * dout * [z > 0].
// No reductions, no parameter gradients: a flat grid-stride stream.
template <int NH>
__global__ __launch_bounds__(256) void bn_eval_bwd_kernel(const void* __restrict__ dout, int ld_dout,
                                                          const void* __restrict__ y, int ldy,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift, void* __restrict__ dy,
                                                          int ld_dy, int64_t npix, int C, int relu, int dt, int sh) {
    const int cv = C / (4 * NH);
    const int64_t total = npix * cv;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t pix; int c;
        bn_split<NH>(i, cv, sh, pix, c);
        BnLane<NH> d, s, o;
        d.load(dout, pix * ld_dout + c, dt & 1);
        s.coef(scale, c);
#pragma unroll
        for (int k = 0; k < NH; ++k) o.h[k] = d.h[k] * s.h[k];
        if (relu) {
            BnLane<NH> v, t;
            v.load(y, pix * ldy + c, dt & 2);
            t.coef(shift, c);
#pragma unroll
            for (int k = 0; k < NH; ++k) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // relu == 2: y already IS the activated output (conv + BN + ReLU fused in the conv epilogue)
                    const bool on = relu == 2 ? v.h[k][e] > 0.f : bn_on(v.h[k][e], s.h[k][e], t.h[k][e]);
                    if (!on) o.h[k][e] = 0.f;
                }
            }
        }
        o.store(dy, pix * ld_dy + c, dt & 4);
    }
}

// the coefficients of a trained layer whose BatchNorm stays in eval(): bn_eval_coeffs_kernel's scale / shift plus the
// running mean and invstd that xhat = (y - running_mean) * invstd needs
__global__ void bn_frozen_coeffs_kernel(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                                        int C, float* scale, float* shift, float* mean, float* invstd) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    invstd[c] = bn_running_coeffs(gamma, beta, rm, rv, eps, c, scale, shift);
    mean[c] = rm[c];
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
// block output is not read back.  Same arithmetic and the same rounding points as bn_apply_kernel followed by
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
    auto act = [&](int yy, int xx, int c, const BnLane<1>& s, const BnLane<1>& t) {
        const size_t at = xb + ((size_t)yy * W + xx) * C + c;
        BnLane<1> o;
        o.load(y, at, dt & 1);
        o.act(s, t, relu, res, at, dt & 2, dt & 4);
        return o.h[0];
    };
    for (int j = blockIdx.x * 256 + threadIdx.x; j < Wo * cq; j += gridDim.x * 256) {
        const int ox = sh >= 0 ? j >> sh : j / cq;
        const int c = (sh >= 0 ? j & (cq - 1) : j - ox * cq) * 4;
        float lx; int x0, x1;
        up_src(ox, W, align, lx, x0, x1);
        BnLane<1> s, t;
        s.coef(scale, c);
        t.coef(shift, c);
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
        BnLane<2> s, t, o;
        o.load(y, at, dt & 1);
        s.coef(scale, cc);
        t.coef(shift, cc);
        o.act(s, t, relu, res, at, dt & 2, dt & 4);
        o0 = o.h[0];
        o1 = o.h[1];
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
        int64_t pix; int c;
        bn_split<1>(i, cq, sh, pix, c);
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

}  // namespace

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

// ---- BatchNorm launches.  8-channel lanes (NH = 2) where a tensor is bf16 and the channel count and every pitch in use
// (0 for an absent tensor) are multiples of 8: 16-byte accesses.
static bool bn_wide(int dtypes, int C, int ld0, int ld1, int ld2) {
    return dtypes && (C % 8) == 0 && (ld0 % 8) == 0 && (ld1 % 8) == 0 && (ld2 % 8) == 0;
}

static void bn_apply_launch(bool wide, hipStream_t st, const void* y, int ldy, const float* scale, const float* shift,
                            const void* res, int ld_res, void* out, int ld_out, int64_t npix, int C, int relu, int dt) {
    const int cv = C / (wide ? 8 : 4);
    hipLaunchKernelGGL(wide ? bn_apply_kernel<2> : bn_apply_kernel<1>, dim3(stream_blocks(npix * cv)), dim3(256), 0, st, y, ldy,
                       scale, shift, res, ld_res, out, ld_out, npix, C, relu, dt, pow2_shift(cv));
}

// pass 1 (dy == nullptr), or the whole backward on frozen statistics
static void bn_bwd_sums_launch(bool wide, int nblk, hipStream_t st, const void* dout, int ld_dout, const void* y, int ldy,
                               const float* scale, const float* shift, const float* mean, const float* invstd, void* dy,
                               int ld_dy, float* partial, int64_t npix, int C, int relu, int dt) {
    auto* k = wide ? (dy ? bn_bwd_sums_kernel<2, true> : bn_bwd_sums_kernel<2, false>)
                   : (dy ? bn_bwd_sums_kernel<1, true> : bn_bwd_sums_kernel<1, false>);
    hipLaunchKernelGGL(k, dim3(nblk), dim3(256), 0, st, dout, ld_dout, y, ldy, scale, shift, mean, invstd, dy, ld_dy, partial,
                       npix, C, relu, dt);
}

static void bn_bwd_finalize_launch(hipStream_t st, const float* partial, int slots, int C, int64_t npix, float* dgamma,
                                   float* dbeta, float* k1, float* k2) {
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0, st, partial, slots, C, (double)npix, dgamma, dbeta, k1, k2);
}

static void bn_bwd_apply_launch(bool wide, hipStream_t st, const void* dout, int ld_dout, const void* y, int ldy,
                                const float* scale, const float* shift, const float* mean, const float* invstd,
                                const float* k1, const float* k2, void* dy, int ld_dy, int64_t npix, int C, int relu, int dt) {
    const int cv = C / (wide ? 8 : 4);
    hipLaunchKernelGGL(wide ? bn_bwd_apply_kernel<2> : bn_bwd_apply_kernel<1>, dim3(stream_blocks(npix * cv)), dim3(256), 0, st,
                       dout, ld_dout, y, ldy, scale, shift, mean, invstd, k1, k2, dy, ld_dy, npix, C, relu, dt, pow2_shift(cv));
}

static void bn_eval_bwd_launch(bool wide, hipStream_t st, const void* dout, int ld_dout, const void* y, int ldy,
                               const float* scale, const float* shift, void* dy, int ld_dy, int64_t npix, int C, int relu,
                               int dt) {
    const int cv = C / (wide ? 8 : 4);
    hipLaunchKernelGGL(wide ? bn_eval_bwd_kernel<2> : bn_eval_bwd_kernel<1>, dim3(stream_blocks(npix * cv)), dim3(256), 0, st,
                       dout, ld_dout, y, ldy, scale, shift, dy, ld_dy, npix, C, relu, dt, pow2_shift(cv));
}

static int bn_sums_blocks(int64_t npix, int maxblk) {
    int64_t b = cdiv64(npix, 64);
    if (b < 1) b = 1;
    return (int)(b < maxblk ? b : maxblk);
}
static int bnb_blocks(int64_t npix) { return bn_sums_blocks(npix, BNB_MAXBLK); }
static int bnf_blocks(int64_t npix) { return bn_sums_blocks(npix, BNF_MAXBLK); }

extern "C" int gdn_bn_apply(const void* y, int32_t ldy, const float* scale, const float* shift, const void* residual,
                            int32_t ld_res, void* out, int32_t ld_out, int64_t npix, int32_t C, int32_t relu,
                            int32_t dtypes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!y || !scale || !shift || !out || npix <= 0 || C <= 0) return GDN_ERR_BAD_ARG;
    if ((C % 4) || (ldy % 4) || (ld_out % 4) || (residual && (ld_res % 4))) return GDN_ERR_UNSUPPORTED;
    bn_apply_launch(bn_wide(dtypes, C, ldy, ld_out, residual ? ld_res : 0), ST(stream), y, ldy, scale, shift, residual, ld_res,
                    out, ld_out, npix, C, relu, dtypes);
    return gdn_launch_status();
}

extern "C" size_t gdn_bn_bwd_workspace_bytes(int64_t npix, int32_t C) {
    return ((size_t)bnb_blocks(npix) * 2 * C + 2 * (size_t)C) * sizeof(float);
}

// Pass 1 runs on 4-channel lanes for bf16 tensors too: the order of its sums, and with it dgamma / dbeta to the bit, depends
// on the lane width.  Widening it is a speed change of its own.
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
        bn_bwd_finalize_launch(ST(stream), ext_partial, (int)ext_slots, C, npix, dgamma, dbeta, k1, k2);
    } else {
        bn_bwd_sums_launch(false, nblk, ST(stream), dout, ld_dout, y, ldy, scale, shift, mean, invstd, nullptr, 0, partial, npix,
                           C, relu, dtypes);
        bn_bwd_finalize_launch(ST(stream), partial, nblk, C, npix, dgamma, dbeta, k1, k2);
    }
    bn_bwd_apply_launch(bn_wide(dtypes, C, ldy, ld_dout, ld_dy), ST(stream), dout, ld_dout, y, ldy, scale, shift, mean, invstd,
                        k1, k2, dy, ld_dy, npix, C, relu, dtypes);
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
        bn_bwd_finalize_launch(ST(stream), ext_partial, (int)ext_slots, C, npix, dgamma, dbeta, kk, kk + C);
        return gdn_launch_status();
    }
    if (!dout || !y) return GDN_ERR_BAD_ARG;
    if ((C % 4) || (ldy % 4) || (ld_dout % 4)) return GDN_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < gdn_bn_bwd_workspace_bytes(npix, C)) return GDN_ERR_WORKSPACE;
    const int nblk = bnb_blocks(npix);
    float* partial = (float*)workspace;
    bn_bwd_sums_launch(false, nblk, ST(stream), dout, ld_dout, y, ldy, scale, shift, mean, invstd, nullptr, 0, partial, npix, C,
                       relu, dtypes);
    bn_bwd_finalize_launch(ST(stream), partial, nblk, C, npix, dgamma, dbeta, kk, kk + C);
    return gdn_launch_status();
}

// 4-channel lanes for every dtype, as it always ran; widening it for bf16 is a speed change of its own.
extern "C" int gdn_bn_eval_bwd(const void* dout, int32_t ld_dout, const void* y, int32_t ldy, const float* scale,
                               const float* shift, void* dy, int32_t ld_dy, int64_t npix, int32_t C, int32_t relu,
                               int32_t dtypes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    if (!dout || !y || !scale || !shift || !dy || npix <= 0 || C <= 0) return GDN_ERR_BAD_ARG;
    if ((C % 4) || (ldy % 4) || (ld_dout % 4) || (ld_dy % 4)) return GDN_ERR_UNSUPPORTED;
    bn_eval_bwd_launch(false, ST(stream), dout, ld_dout, y, ldy, scale, shift, dy, ld_dy, npix, C, relu, dtypes);
    return gdn_launch_status();
}

// ------------------------------------------------ BN backward on FROZEN statistics
// A trained layer whose BatchNorm stays in eval(): out = [relu](y*scale + shift) with scale / shift from the RUNNING statistics.
// dy = scale * dout * [z > 0] depends on no reduction, so one pass (bn_bwd_sums_kernel<NH, true>) reads dout and y once, writes
// dy and leaves the per-block sums of dz and dz*xhat (xhat = (y - running_mean) * invstd) that bn_bwd_finalize_kernel turns
// into dbeta / dgamma.  Where the sums came from the producer of dout, the dy pass alone is bn_eval_bwd_kernel.
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
    const bool wide = bn_wide(dtypes, C, ldy, ld_dout, dy ? ld_dy : 0);
    if (sums)
        bn_bwd_sums_launch(wide, nblk, ST(stream), dout, ld_dout, y, ldy, scale, shift, mean, invstd, dy, ld_dy, partial, npix, C,
                           relu ? 1 : 0, dtypes);
    else if (dy)
        bn_eval_bwd_launch(wide, ST(stream), dout, ld_dout, y, ldy, scale, shift, dy, ld_dy, npix, C, relu ? 1 : 0, dtypes);
    if (want_sums)
        bn_bwd_finalize_launch(ST(stream), ext_partial ? ext_partial : partial, ext_partial ? (int)ext_slots : nblk, C, npix,
                               dgamma, dbeta, k1, k2);
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
