// The BatchNorm arithmetic, once: the activation out = [relu](y*s + t), the masked gradient dz = dout * [z > 0], xhat and
// pass 3 of the backward, the 4- or 8-channel lane of the streaming kernels and the LDS sum over a block's pixel lanes.
// pointwise.hip's kernels and the conv epilogues that emit backward partial sums (conv_wino.hip, ring_common.h,
// conv_igemm.hip, conv_fft.hip) agree to the bit because they all call these.  The expressions are written plainly: the
// compiler contracts y*s + t into one FMA, and the tests' bars are set for that -- no reassociation, no fmaf by hand.
#pragma once
#include "common.h"

// ---- per element ----
__device__ __forceinline__ bool bn_on(float y, float s, float t) { return y * s + t > 0.f; }
__device__ __forceinline__ bool bn_off(float y, float s, float t, int relu) { return relu && !bn_on(y, s, t); }
// gradient at the BatchNorm output z = y*s + t, behind the optional ReLU (0 AT z == 0, as torch)
__device__ __forceinline__ float bn_dz(float d, float y, float s, float t, int relu) { return bn_off(y, s, t, relu) ? 0.f : d; }
// dy of a BatchNorm with fixed coefficients: s * dz, and an exact +0 where the ReLU is off
__device__ __forceinline__ float bn_fixed_dy(float d, float y, float s, float t, int relu) { return bn_off(y, s, t, relu) ? 0.f : d * s; }
__device__ __forceinline__ float bn_xhat(float y, float mu, float is) { return (y - mu) * is; }
// pass 3: dy = gamma*invstd * (dz - mean(dz) - xhat * mean(dz*xhat))
__device__ __forceinline__ float bn_bwd_dy(float dz, float xhat, float s, float k1, float k2) { return s * (dz - k1 - xhat * k2); }
// the activation before the residual is added
__device__ __forceinline__ float bn_act(float y, float s, float t, int relu) {
    const float o = y * s + t;
    return relu ? fmaxf(o, 0.f) : o;
}

// ---- a lane's channels: NH 4-channel halves (1: 16 bytes of fp32; 2: 16 bytes of bf16) ----
template <int NH>
struct BnLane {
    static_assert(NH == 1 || NH == 2, "a lane holds 4 or 8 channels");
    f32x4 h[NH];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int k = 0; k < NH; ++k) h[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __device__ __forceinline__ void load(const void* p, size_t idx, int bf16) {
        if constexpr (NH == 2) ld8_any(p, idx, bf16, h[0], h[1]);
        else h[0] = ld4_any(p, idx, bf16);
    }
    __device__ __forceinline__ void store(void* p, size_t idx, int bf16) const {
        if constexpr (NH == 2) st8_any(p, idx, h[0], h[1], bf16);
        else st4_any(p, idx, h[0], bf16);
    }
    // per-channel fp32 coefficients of channels c .. c + 4*NH - 1
    __device__ __forceinline__ void coef(const float* __restrict__ p, int c) {
#pragma unroll
        for (int k = 0; k < NH; ++k) h[k] = *reinterpret_cast<const f32x4*>(p + c + 4 * k);
    }
    // this lane holds y: -> [relu](y*s + t) (+ residual), optionally rounded to bf16 storage and back (what a consumer reads)
    __device__ __forceinline__ void act(const BnLane& s, const BnLane& t, int relu, const void* res, size_t at_res, int res_bf16,
                                        int round_bf16) {
#pragma unroll
        for (int k = 0; k < NH; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) h[k][e] = bn_act(h[k][e], s.h[k][e], t.h[k][e], relu);
        if (res) {
            BnLane r;
            r.load(res, at_res, res_bf16);
#pragma unroll
            for (int k = 0; k < NH; ++k) h[k] += r.h[k];
        }
        if (round_bf16) {
#pragma unroll
            for (int k = 0; k < NH; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) h[k][e] = bf16_h_to_f32(f32_to_bf16_h(h[k][e]));
        }
    }
};

// flat lane index i over [pixel][cv channel vectors of 4*NH] -> pixel, first channel.  sh = log2(cv) where cv is a power of
// two (the host's pow2_shift), else -1: the 64-bit division alone cost more than the memory traffic.
template <int NH>
__device__ __forceinline__ void bn_split(int64_t i, int cv, int sh, int64_t& pix, int& c) {
    pix = sh >= 0 ? (i >> sh) : i / cv;
    c = (int)(sh >= 0 ? (i & (cv - 1)) : (i - pix * cv)) * (4 * NH);
}

// Sum of (a1, a2) over the PY pixel lanes of a 256-thread block laid out as thread = ty * CQ + tx, through sh[256 * 8].
// Every thread of the block calls it (two barriers).  Lane ty == 0 adds j = 0 .. PY-1 in order and, where dst1 is not null,
// stores the two sums.
__device__ __forceinline__ void bn_lane_reduce(float* sh, const f32x4& a1, const f32x4& a2, int tx, int ty, int CQ, int PY,
                                               float* dst1, float* dst2) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) { sh[threadIdx.x * 8 + e] = a1[e]; sh[threadIdx.x * 8 + 4 + e] = a2[e]; }
    __syncthreads();
    if (ty == 0 && dst1) {
        f32x4 r1 = {0.f, 0.f, 0.f, 0.f}, r2 = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < PY; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { r1[e] += sh[(j * CQ + tx) * 8 + e]; r2[e] += sh[(j * CQ + tx) * 8 + 4 + e]; }
        }
        *reinterpret_cast<f32x4*>(dst1) = r1;
        *reinterpret_cast<f32x4*>(dst2) = r2;
    }
}
