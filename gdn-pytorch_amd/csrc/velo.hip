// Raw Velodyne scans -> the sparse ground-truth maps of the Eigen split, on the device (--eval_velodyne).
// No counterpart in the reference: the published host routine projects one scan at a time and resolves the pixels that
// several points hit in a Python loop; this one takes a ragged batch of scans and leaves float32 metres in the padded pool
// that gdn_depth_metrics_std reads as gt_kind 0.
//
// gdn_velo_project, per point (x, y, z, .) of image b (the fourth float is taken as 1), all in float64 with FMA contraction
// off, so that a float64 numpy restatement (tests/velo_numpy.py) rounds and compares the same way:
//   keep iff x >= 0;  r_i = ((P[i][0] x + P[i][1] y) + P[i][2] z) + P[i][3];  u = rint(r_0 / r_2) - 1, v = rint(r_1 / r_2) - 1
//   (half to even; the -1 is the devkit's 1-based pixel);  keep iff 0 <= u < w0 and 0 <= v < h0, compared in double (NaN and
//   +-inf fail);  d = (float)(depth_kind ? x : r_2).  A pixel takes the MINIMUM d of the points on it; a minimum that is not
//   > 0, or no point at all, reads +0.
// No workspace: between the launches the output cells hold an order-preserving 32-bit key of d (vp_key), 0xFFFFFFFF = empty.
//   memset    the pool to 0xFF
//   scatter   grid (points / VP_PPW, B), grid-stride inside an image: one 16-byte load per point, one no-return unsigned
//             atomicMin per kept point
//   finalise  the whole pool in place, padding included: key -> metres, 16 bytes per lane where a quad of cells lies inside
//             the workgroup's range; with `hits`, one integer atomic per workgroup adds its count of > 0 pixels
// Only integer atomics: the result does not depend on the order of arrival, two calls give the same bytes.
#include "common.h"

namespace {

#define VP_T 256            // threads per workgroup
#define VP_PPW 2048         // points per workgroup the scatter grid is sized for
#define VP_MAX_GX 4096      // most scatter workgroups per image (grid-stride beyond)
#define VP_CHUNK 4096       // cells per finalise workgroup the chunk count is sized for
#define VP_MAX_NCH 1024     // most finalise workgroups per image
#define VP_EMPTY 0xFFFFFFFFu

// float32 -> a key whose unsigned order is the float order (-inf < ... < -0 < +0 < ... < +inf); no depth maps to VP_EMPTY
// (that would be the NaN 0x7fffffff, and a kept point's depth is never NaN)
__device__ __forceinline__ unsigned vp_key(float d) {
    const unsigned bits = __float_as_uint(d);
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// key -> the cell's final value: the depth if it is > 0, else +0 (VP_EMPTY decodes to a NaN, which is not > 0)
__device__ __forceinline__ float vp_metres(unsigned key) {
    const float d = __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
    return d > 0.f ? d : 0.f;
}

__global__ __launch_bounds__(VP_T) void velo_scatter_kernel(const float4* __restrict__ points, const int64_t* __restrict__ offsets,
                                                            const double* __restrict__ proj, const int32_t* __restrict__ sizes,
                                                            int Hmax, int Wmax, int depth_kind, unsigned* __restrict__ cells) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int64_t first = offsets[b], n = offsets[b + 1] - first;
    const int64_t stride = (int64_t)gridDim.x * VP_T;
    int64_t i = (int64_t)blockIdx.x * VP_T + threadIdx.x;
    if (i >= n) return;
    // h0 / w0 are held inside the pool so that no pixel derived from them leaves this image's cells
    const int h0 = min(max(sizes[2 * b], 0), Hmax), w0 = min(max(sizes[2 * b + 1], 0), Wmax);
    const double dh = (double)h0, dw = (double)w0;
    double P[12];
    for (int k = 0; k < 12; ++k) P[k] = proj[(size_t)b * 12 + k];
    unsigned* img = cells + (size_t)b * (size_t)Hmax * Wmax;
    for (; i < n; i += stride) {
        const float4 q = points[first + i];
        const double x = (double)q.x, y = (double)q.y, z = (double)q.z;
        if (!(x >= 0.0)) continue;
        const double r0 = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
        const double r1 = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
        const double r2 = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
        const double u = rint(r0 / r2) - 1.0, v = rint(r1 / r2) - 1.0;
        if (!(u >= 0.0 && v >= 0.0 && u < dw && v < dh)) continue;
        const float d = (float)(depth_kind ? x : r2);
        atomicMin(&img[(size_t)(int)v * Wmax + (int)u], vp_key(d));
    }
}

// Workgroup (c, b) finalises cells [b N + c chunk, b N + min((c + 1) chunk, N)) of the flat pool.  Lanes walk the 16-byte
// quads that overlap the range: a quad inside it moves as one uint4, a quad the range cuts (an image boundary when N is no
// multiple of 4) cell by cell -- the neighbouring workgroup does the other cells of that quad.
__global__ __launch_bounds__(VP_T) void velo_finalise_kernel(unsigned* cells, int64_t N, int64_t chunk, int32_t* __restrict__ hits) {
    __shared__ int sh[VP_T / 64];
    const int b = blockIdx.y, t = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * chunk;
    if (c0 >= N) return;                                              // uniform: this chunk lies past the image
    const int64_t lo = (int64_t)b * N + c0, hi = (int64_t)b * N + (c0 + chunk < N ? c0 + chunk : N);
    int count = 0;
    for (int64_t q = (lo >> 2) + t; q * 4 < hi; q += VP_T) {
        const int64_t at = q * 4;
        if (at >= lo && at + 4 <= hi) {
            const uint4 k = *reinterpret_cast<const uint4*>(cells + at);
            float4 o;
            o.x = vp_metres(k.x); o.y = vp_metres(k.y); o.z = vp_metres(k.z); o.w = vp_metres(k.w);
            count += (o.x > 0.f) + (o.y > 0.f) + (o.z > 0.f) + (o.w > 0.f);
            *reinterpret_cast<float4*>(cells + at) = o;
        } else {
            for (int j = 0; j < 4; ++j) {
                if (at + j < lo || at + j >= hi) continue;
                const float o = vp_metres(cells[at + j]);
                count += o > 0.f;
                cells[at + j] = __float_as_uint(o);
            }
        }
    }
    if (!hits) return;
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
    if ((t & 63) == 0) sh[t >> 6] = count;
    __syncthreads();
    if (t == 0) {
        const int total = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        if (total) atomicAdd(&hits[b], total);
    }
}

}  // namespace

extern "C" int gdn_velo_project(const float* points, const int64_t* offsets, const double* proj, const int32_t* sizes, int32_t B,
                                int64_t max_points, int32_t Hmax, int32_t Wmax, int32_t depth_kind, float* depth, int32_t* hits,
                                void* stream) {
    (void)hipGetLastError();
    if (!offsets || !proj || !sizes || !depth || B < 1 || B > 65535 || Hmax <= 0 || Wmax <= 0 ||
        (int64_t)Hmax * Wmax > INT32_MAX || depth_kind < 0 || depth_kind > 1 || max_points < 0 || (max_points > 0 && !points))
        return GDN_ERR_BAD_ARG;
    if (((uintptr_t)points & 15) || ((uintptr_t)depth & 15) || ((uintptr_t)offsets & 7) || ((uintptr_t)proj & 7) ||
        ((uintptr_t)sizes & 3) || ((uintptr_t)hits & 3))
        return GDN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)Hmax * Wmax;
    if (hipMemsetAsync(depth, 0xFF, (size_t)B * (size_t)N * sizeof(float), st) != hipSuccess) return GDN_ERR_LAUNCH;
    if (hits && hipMemsetAsync(hits, 0, (size_t)B * sizeof(int32_t), st) != hipSuccess) return GDN_ERR_LAUNCH;
    if (max_points > 0) {
        int64_t gx = cdiv64(max_points, VP_PPW);
        gx = gx > VP_MAX_GX ? VP_MAX_GX : gx;
        hipLaunchKernelGGL(velo_scatter_kernel, dim3((unsigned)gx, B), dim3(VP_T), 0, st, (const float4*)points, offsets, proj,
                           sizes, Hmax, Wmax, depth_kind, (unsigned*)depth);
    }
    int64_t nch = cdiv64(N, VP_CHUNK);
    nch = nch > VP_MAX_NCH ? VP_MAX_NCH : nch;
    const int64_t chunk = (cdiv64(N, nch) + 3) & ~(int64_t)3;
    hipLaunchKernelGGL(velo_finalise_kernel, dim3((unsigned)nch, B), dim3(VP_T), 0, st, (unsigned*)depth, N, chunk, hits);
    return gdn_launch_status();
}
