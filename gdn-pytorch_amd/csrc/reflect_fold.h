// The mirror rule of ReflectionPad2d(p) read backwards, for every kernel that folds a data gradient computed over the padded
// domain (extent n + 2p per axis) back onto the image: which padded coordinates reflect onto image coordinate o.
#pragma once
#include "common.h"

namespace {

// q[0] = o + p (o itself); then p - o when the low border mirrors o (1 <= o <= p) and 2(n-1) - o + p when the high border
// does (n-1-p <= o <= n-2).  Returns the count, 1..3; the order is the order every fold sums in.
__device__ __forceinline__ int reflect_sources(int o, int n, int p, int (&q)[3]) {
    int c = 0;
    q[c++] = o + p;
    if (o >= 1 && o <= p) q[c++] = p - o;
    if (o <= n - 2 && o >= n - 1 - p) q[c++] = 2 * (n - 1) - o + p;
    return c;
}

// dx[y][x] = sum of the padded-domain gradient dxp [B][H+2p][W+2p][C] over the padded coordinates that reflect onto (y, x)
// (+ addsrc); fp32, thread = 4 channels of a pixel, grid-stride.  Body of fft_reflect_fold_kernel and wino_reflect_fold_kernel.
__device__ __forceinline__ void reflect_fold_f32x4(const float* __restrict__ dxp, float* __restrict__ dx, int ldx,
                                                   const float* __restrict__ addsrc, int ld_add, int B, int H, int W, int C, int p) {
    const int Hp = H + 2 * p, Wp = W + 2 * p, c4n = C / 4;
    const int64_t total = (int64_t)B * H * W * c4n;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(i % c4n);
        int64_t t = i / c4n;
        const int x = (int)(t % W); t /= W;
        const int y = (int)(t % H), b = (int)(t / H);
        int qy[3], qx[3];
        const int ny = reflect_sources(y, H, p, qy), nx = reflect_sources(x, W, p, qx);
        f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
        for (int a = 0; a < ny; ++a)
            for (int e = 0; e < nx; ++e)
                s4 += *reinterpret_cast<const f32x4*>(dxp + ((size_t)(b * Hp + qy[a]) * Wp + qx[e]) * C + c4 * 4);
        const size_t op = (size_t)(b * H + y) * W + x;
        if (addsrc) s4 += *reinterpret_cast<const f32x4*>(addsrc + op * ld_add + c4 * 4);
        *reinterpret_cast<f32x4*>(dx + op * ldx + c4 * 4) = s4;
    }
}

// grid of a fold launch over n lanes' worth of items (all fold kernels are grid-stride, 256 threads per block)
inline unsigned fold_blocks(int64_t n, int cap = 65536 * 8) { return (unsigned)stream_blocks(n, 256, cap); }

}  // namespace
