// Sparse LiDAR depth -> dense depth on the device, and the byte encoder of the training files (gdn_amd.prepare_kitti,
// DESIGN.md 3.16).  No counterpart in the reference, which trains on dense maps somebody else's script made.  The chain is the
// classical morphological completion of Ku, Harakeh and Waslander ("In Defense of Classical Image Processing", 2018), restated
// in numpy by tests/densify_numpy.py, which the pools are compared with bit for bit: every step is a selection (max, min,
// median) or a fixed-order chain of single float32 operations with contraction off.
//
// gdn_depth_densify, per image b of the padded pool (h0 x w0 = sizes[b], held inside Hmax x Wmax), empty(v) := !(v > 0.1f):
//   1  v = D > 0.1f ? max_depth - D : 0, then 0 where empty(v)           (larger = nearer; NaN, +-inf and far returns drop out)
//   2  max over the 5 x 5 diamond, out-of-image cells read 0
//   3  max over the 5 x 5 box (out-of-image 0), then min over the 5 x 5 box (out-of-image ignored)
//   4  where empty(v): v = max over the 7 x 7 box
//   5  every row above a column's topmost non-empty row takes that row's value
//   6  where empty(v): v = max over the 31 x 31 box
//   7  where !empty(v): v = the 13th smallest of the 5 x 5 window, borders replicated
//   8  where !empty(v): v = the [1 4 6 4 1] / 16 blur, rows then columns, borders reflected without the edge sample;
//      out = empty(v) ? +0 : max_depth - v
// Four launches, tiles of DZ_TH x DZ_TW outputs, the stages of a launch ping-ponged between two LDS images:
//   fill     steps 1-4, halo 9                       in   -> out
//   extend   step 5, one lane per column, in place   out
//   holes    step 6, halo 15, rows then columns      out  -> work  (a tile without an empty cell is copied through)
//   smooth   steps 7-8 and the inversion, halo 4     work -> out   (every cell of the pool, the padding as +0)
// No atomics; every cell has one writer per launch, so two calls give the same bytes.  Between the launches only cells inside
// an image are read, so neither `out` nor the workspace needs clearing.
#ifndef GDN_DENSIFY_HOST            // tests/diag/densify_host.cpp compiles this file's kernels as serial host code
#include "common.h"
#endif

namespace {

#ifndef DZ_T
#define DZ_T 256            // threads per workgroup
#endif
#define DZ_TW 64            // tile width: one wave reads one row of it
#define DZ_TH 32            // tile height
#define DZ_EMPTY 0.1f

__device__ __forceinline__ bool dz_empty(float v) { return !(v > DZ_EMPTY); }

// A tile's place: the image, its size held inside the pool, the tile's first cell; false when the tile lies outside the image.
struct dz_tile { int h0, w0, y0, x0; size_t base; };

__device__ __forceinline__ dz_tile dz_place(const int32_t* sizes, int Hmax, int Wmax, int ntx) {
    dz_tile t;
    const int b = blockIdx.y;
    t.h0 = min(max(sizes[2 * b], 0), Hmax);
    t.w0 = min(max(sizes[2 * b + 1], 0), Wmax);
    t.y0 = (int)(blockIdx.x / ntx) * DZ_TH;
    t.x0 = (int)(blockIdx.x % ntx) * DZ_TW;
    t.base = (size_t)b * (size_t)Hmax * Wmax;
    return t;
}

// ---- fill: steps 1-4.  Every stage keeps the coordinates of the first one: region cell (ry, rx) is image cell
// (y0 - 9 + ry, x0 - 9 + rx), and stage k is computed on the region shrunk by its margin.
#define F_HALO 9
#define F_RW (DZ_TW + 2 * F_HALO)
#define F_RH (DZ_TH + 2 * F_HALO)

__global__ __launch_bounds__(DZ_T) void densify_fill_kernel(const float* __restrict__ in, const int32_t* __restrict__ sizes,
                                                            int Hmax, int Wmax, int ntx, float max_depth, float* __restrict__ out) {
    __shared__ float sa[F_RH * F_RW], sb[F_RH * F_RW];
    const dz_tile t = dz_place(sizes, Hmax, Wmax, ntx);
    if (t.y0 >= t.h0 || t.x0 >= t.w0) return;
    const int tid = threadIdx.x;
    const int oy = t.y0 - F_HALO, ox = t.x0 - F_HALO;
    const float* img = in + t.base;
    // 1: invert
    for (int i = tid; i < F_RH * F_RW; i += DZ_T) {
        const int ry = i / F_RW, rx = i % F_RW, y = oy + ry, x = ox + rx;
        float v = 0.f;
        if (y >= 0 && y < t.h0 && x >= 0 && x < t.w0) {
            const float d = img[(size_t)y * Wmax + x];
            v = d > DZ_EMPTY ? max_depth - d : 0.f;
            if (dz_empty(v)) v = 0.f;
        }
        sa[i] = v;
    }
    __syncthreads();
    // 2: diamond dilation, margin 2
    for (int i = tid; i < (F_RH - 4) * (F_RW - 4); i += DZ_T) {
        const int ry = 2 + i / (F_RW - 4), rx = 2 + i % (F_RW - 4), y = oy + ry, x = ox + rx;
        float m = 0.f;
        if (y >= 0 && y < t.h0 && x >= 0 && x < t.w0) {
            const float* c = sa + ry * F_RW + rx;
            m = fmaxf(c[-2 * F_RW], c[2 * F_RW]);
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) m = fmaxf(m, fmaxf(c[-F_RW + dx], c[F_RW + dx]));
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) m = fmaxf(m, c[dx]);
        }
        sb[ry * F_RW + rx] = m;
    }
    __syncthreads();
    // 3a: box dilation, margin 4 (a cell outside the image keeps what the maximum gives: the erosion does not read it)
    for (int i = tid; i < (F_RH - 8) * (F_RW - 8); i += DZ_T) {
        const int ry = 4 + i / (F_RW - 8), rx = 4 + i % (F_RW - 8);
        const float* c = sb + ry * F_RW + rx;
        float m = 0.f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) m = fmaxf(m, c[dy * F_RW + dx]);
        sa[ry * F_RW + rx] = m;
    }
    __syncthreads();
    // 3b: box erosion over the cells inside the image, margin 6
    for (int i = tid; i < (F_RH - 12) * (F_RW - 12); i += DZ_T) {
        const int ry = 6 + i / (F_RW - 12), rx = 6 + i % (F_RW - 12), y = oy + ry, x = ox + rx;
        float m = 0.f;
        if (y >= 0 && y < t.h0 && x >= 0 && x < t.w0) {
            const float* c = sa + ry * F_RW + rx;
            m = c[0];
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx)
                    if (y + dy >= 0 && y + dy < t.h0 && x + dx >= 0 && x + dx < t.w0) m = fminf(m, c[dy * F_RW + dx]);
        }
        sb[ry * F_RW + rx] = m;
    }
    __syncthreads();
    // 4: small holes take the 7 x 7 maximum
    float* dst = out + t.base;
    for (int i = tid; i < DZ_TH * DZ_TW; i += DZ_T) {
        const int ty = i / DZ_TW, tx = i % DZ_TW, y = t.y0 + ty, x = t.x0 + tx;
        if (y >= t.h0 || x >= t.w0) continue;
        const float* c = sb + (ty + F_HALO) * F_RW + tx + F_HALO;
        float v = c[0];
        if (dz_empty(v)) {
            v = 0.f;
#pragma unroll
            for (int dy = -3; dy <= 3; ++dy)
#pragma unroll
                for (int dx = -3; dx <= 3; ++dx) v = fmaxf(v, c[dy * F_RW + dx]);
        }
        dst[(size_t)y * Wmax + x] = v;
    }
}

// ---- extend: step 5.  One lane per column, rows read eight at a time so that the loads of a group do not wait for each other.
#ifndef E_T
#define E_T 64
#endif
#define E_ROWS 8

__global__ __launch_bounds__(E_T) void densify_extend_kernel(float* __restrict__ pool, const int32_t* __restrict__ sizes, int Hmax,
                                                             int Wmax) {
    const int b = blockIdx.y, x = blockIdx.x * E_T + threadIdx.x;
    const int h0 = min(max(sizes[2 * b], 0), Hmax), w0 = min(max(sizes[2 * b + 1], 0), Wmax);
    if (x >= w0) return;
    float* col = pool + (size_t)b * (size_t)Hmax * Wmax + x;
    int top = -1;
    float value = 0.f;
    for (int r = 0; r < h0 && top < 0; r += E_ROWS) {
        float v[E_ROWS];
#pragma unroll
        for (int k = 0; k < E_ROWS; ++k) v[k] = r + k < h0 ? col[(size_t)(r + k) * Wmax] : 0.f;
#pragma unroll
        for (int k = E_ROWS - 1; k >= 0; --k)
            if (!dz_empty(v[k])) { top = r + k; value = v[k]; }
    }
    for (int r = 0; r < top; ++r) col[(size_t)r * Wmax] = value;
}

// ---- holes: step 6, the 31 x 31 maximum as a row pass and a column pass in LDS.
#define G_HALO 15
#define G_RW (DZ_TW + 2 * G_HALO)
#define G_RH (DZ_TH + 2 * G_HALO)

__global__ __launch_bounds__(DZ_T) void densify_holes_kernel(const float* __restrict__ in, const int32_t* __restrict__ sizes,
                                                             int Hmax, int Wmax, int ntx, float* __restrict__ out) {
    __shared__ float sa[G_RH * G_RW], sb[G_RH * DZ_TW];
    const dz_tile t = dz_place(sizes, Hmax, Wmax, ntx);
    if (t.y0 >= t.h0 || t.x0 >= t.w0) return;
    const int tid = threadIdx.x;
    const int oy = t.y0 - G_HALO, ox = t.x0 - G_HALO;
    const float* img = in + t.base;
    float* dst = out + t.base;
    // a tile without an empty cell (most tiles of a LiDAR map after step 5) passes through: no halo, no LDS
    int holes = 0;
    for (int i = tid; i < DZ_TH * DZ_TW; i += DZ_T) {
        const int y = t.y0 + i / DZ_TW, x = t.x0 + i % DZ_TW;
        if (y < t.h0 && x < t.w0) holes |= dz_empty(img[(size_t)y * Wmax + x]);
    }
    if (!__syncthreads_or(holes)) {
        for (int i = tid; i < DZ_TH * DZ_TW; i += DZ_T) {
            const int y = t.y0 + i / DZ_TW, x = t.x0 + i % DZ_TW;
            if (y < t.h0 && x < t.w0) dst[(size_t)y * Wmax + x] = img[(size_t)y * Wmax + x];
        }
        return;
    }
    for (int i = tid; i < G_RH * G_RW; i += DZ_T) {
        const int ry = i / G_RW, rx = i % G_RW, y = oy + ry, x = ox + rx;
        sa[i] = (y >= 0 && y < t.h0 && x >= 0 && x < t.w0) ? img[(size_t)y * Wmax + x] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < G_RH * DZ_TW; i += DZ_T) {
        const int ry = i / DZ_TW, tx = i % DZ_TW;
        const float* c = sa + ry * G_RW + tx;
        float m = 0.f;
#pragma unroll
        for (int dx = 0; dx <= 2 * G_HALO; ++dx) m = fmaxf(m, c[dx]);
        sb[i] = m;
    }
    __syncthreads();
    for (int i = tid; i < DZ_TH * DZ_TW; i += DZ_T) {
        const int ty = i / DZ_TW, tx = i % DZ_TW, y = t.y0 + ty, x = t.x0 + tx;
        if (y >= t.h0 || x >= t.w0) continue;
        float v = sa[(ty + G_HALO) * G_RW + tx + G_HALO];
        if (dz_empty(v)) {
            v = 0.f;
#pragma unroll
            for (int dy = 0; dy <= 2 * G_HALO; ++dy) v = fmaxf(v, sb[(ty + dy) * DZ_TW + tx]);
        }
        dst[(size_t)y * Wmax + x] = v;
    }
}

// ---- smooth: steps 7-8 and the inversion.
#define S_HALO 4
#define S_RW (DZ_TW + 2 * S_HALO)
#define S_RH (DZ_TH + 2 * S_HALO)

#define DZ_CX(a, b) { const float lo_ = fminf(a, b); b = fmaxf(a, b); a = lo_; }

// The 13th smallest of 25 by forgetful selection: of 14 values neither the smallest nor the largest can be the median of the
// 25, so both leave and the next value joins, down to three (165 compare-exchanges).  Every loop unrolls, so every index is
// a constant and the values stay in registers: no dynamically indexed private array, no scratch.
__device__ __forceinline__ float dz_median25(const float (&w)[25]) {
    float p[14];
#pragma unroll
    for (int i = 0; i < 14; ++i) p[i] = w[i];
    int next = 14;
#pragma unroll
    for (int n = 14; n > 3; --n) {
        // minimum to p[0], maximum to p[n - 1]
#pragma unroll
        for (int i = 1; i < n; ++i) DZ_CX(p[0], p[i]);
#pragma unroll
        for (int i = 1; i < n - 1; ++i) DZ_CX(p[i], p[n - 1]);
        // forget both: the next value takes the minimum's place, the last place closes
        p[0] = w[next++];
    }
    DZ_CX(p[0], p[1]);
    DZ_CX(p[1], p[2]);
    return fmaxf(p[0], p[1]);
}

// reflect-101 of index i into [0, n): the period is 2 (n - 1); a single row or column reads itself
__device__ __forceinline__ int dz_reflect(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    m = m < 0 ? m + p : m;
    return m >= n ? p - m : m;
}

__global__ __launch_bounds__(DZ_T) void densify_smooth_kernel(const float* __restrict__ in, const int32_t* __restrict__ sizes,
                                                              int Hmax, int Wmax, int ntx, float max_depth, float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ float sa[S_RH * S_RW], sb[S_RH * S_RW];
    const dz_tile t = dz_place(sizes, Hmax, Wmax, ntx);
    const int tid = threadIdx.x;
    float* dst = out + t.base;
    if (t.y0 >= t.h0 || t.x0 >= t.w0) {                               // a tile of padding: +0
        for (int i = tid; i < DZ_TH * DZ_TW; i += DZ_T) {
            const int y = t.y0 + i / DZ_TW, x = t.x0 + i % DZ_TW;
            if (y < Hmax && x < Wmax) dst[(size_t)y * Wmax + x] = 0.f;
        }
        return;
    }
    const int oy = t.y0 - S_HALO, ox = t.x0 - S_HALO;
    const float* img = in + t.base;
    for (int i = tid; i < S_RH * S_RW; i += DZ_T) {
        const int ry = i / S_RW, rx = i % S_RW, y = oy + ry, x = ox + rx;
        sa[i] = (y >= 0 && y < t.h0 && x >= 0 && x < t.w0) ? img[(size_t)y * Wmax + x] : 0.f;
    }
    __syncthreads();
    // 7: median of the replicated 5 x 5 window, margin 2, cells inside the image
    for (int i = tid; i < (S_RH - 4) * (S_RW - 4); i += DZ_T) {
        const int ry = 2 + i / (S_RW - 4), rx = 2 + i % (S_RW - 4), y = oy + ry, x = ox + rx;
        if (y < 0 || y >= t.h0 || x < 0 || x >= t.w0) continue;
        float v = sa[ry * S_RW + rx];
        if (!dz_empty(v)) {
            float w[25];
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy) {
                const int row = (min(max(y + dy, 0), t.h0 - 1) - oy) * S_RW;
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) w[(dy + 2) * 5 + dx + 2] = sa[row + min(max(x + dx, 0), t.w0 - 1) - ox];
            }
            v = dz_median25(w);
        }
        sb[ry * S_RW + rx] = v;
    }
    __syncthreads();
    // 8a: the row pass of the blur on the tile's columns, rows with margin 2; sa is free again
    for (int i = tid; i < (S_RH - 4) * DZ_TW; i += DZ_T) {
        const int ry = 2 + i / DZ_TW, tx = i % DZ_TW, y = oy + ry, x = t.x0 + tx;
        if (y < 0 || y >= t.h0 || x >= t.w0) continue;
        const float* row = sb + ry * S_RW;
        const float p0 = row[dz_reflect(x - 2, t.w0) - ox], p1 = row[dz_reflect(x - 1, t.w0) - ox], p2 = row[x - ox],
                    p3 = row[dz_reflect(x + 1, t.w0) - ox], p4 = row[dz_reflect(x + 2, t.w0) - ox];
        sa[ry * S_RW + tx] = ((((p0 + 4.f * p1) + 6.f * p2) + 4.f * p3) + p4) * 0.0625f;
    }
    __syncthreads();
    // 8b: the column pass, the mask of step 8 and the inversion; every cell of the tile inside the pool is written
    for (int i = tid; i < DZ_TH * DZ_TW; i += DZ_T) {
        const int ty = i / DZ_TW, tx = i % DZ_TW, y = t.y0 + ty, x = t.x0 + tx;
        if (y >= Hmax || x >= Wmax) continue;
        float o = 0.f;
        if (y < t.h0 && x < t.w0) {
            float v = sb[(ty + S_HALO) * S_RW + tx + S_HALO];
            if (!dz_empty(v)) {
                const float* col = sa + tx;
                const float p0 = col[(dz_reflect(y - 2, t.h0) - oy) * S_RW], p1 = col[(dz_reflect(y - 1, t.h0) - oy) * S_RW],
                            p2 = col[(y - oy) * S_RW], p3 = col[(dz_reflect(y + 1, t.h0) - oy) * S_RW],
                            p4 = col[(dz_reflect(y + 2, t.h0) - oy) * S_RW];
                v = ((((p0 + 4.f * p1) + 6.f * p2) + 4.f * p3) + p4) * 0.0625f;
            }
            o = dz_empty(v) ? 0.f : max_depth - v;
        }
        dst[(size_t)y * Wmax + x] = o;
    }
}

// ---- the byte encoder: q = rint(clamp(d, 0, scale) / scale * 255) in double, half to even; NaN -> 0.
__device__ __forceinline__ unsigned dz_byte(float d, double scale, int keep_valid) {
    double c = (double)d;
    c = c > 0.0 ? c : 0.0;                                            // NaN and negatives
    c = c > scale ? scale : c;
    unsigned q = (unsigned)rint(c / scale * 255.0);
    if (keep_valid && d > 0.f && q == 0u) q = 1u;
    return q;
}

__global__ __launch_bounds__(256) void depth_encode_u8_kernel(const float* __restrict__ x, int64_t n, double scale, int keep_valid,
                                                              uint8_t* __restrict__ out) {
    const int64_t quads = n >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[q];
        reinterpret_cast<unsigned*>(out)[q] = dz_byte(v.x, scale, keep_valid) | (dz_byte(v.y, scale, keep_valid) << 8) |
                                              (dz_byte(v.z, scale, keep_valid) << 16) | (dz_byte(v.w, scale, keep_valid) << 24);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (quads << 2) + threadIdx.x;
        out[i] = (uint8_t)dz_byte(x[i], scale, keep_valid);
    }
}

#ifndef GDN_DENSIFY_HOST
static bool dz_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + bytes && q < p + bytes;
}

#endif

}  // namespace

#ifndef GDN_DENSIFY_HOST
extern "C" size_t gdn_depth_densify_workspace_bytes(int32_t B, int32_t Hmax, int32_t Wmax) {
    if (B < 1 || Hmax < 1 || Wmax < 1) return 0;
    return (size_t)B * (size_t)Hmax * (size_t)Wmax * sizeof(float);
}

extern "C" int gdn_depth_densify(const float* depth, const int32_t* sizes, int32_t B, int32_t Hmax, int32_t Wmax, float max_depth,
                                 float* out, void* workspace, size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();
    if (!depth || !sizes || !out || !workspace || B < 1 || B > 65535 || Hmax < 1 || Wmax < 1 ||
        (int64_t)Hmax * Wmax > INT32_MAX || !(max_depth > 0.2f) || !(max_depth < INFINITY))
        return GDN_ERR_BAD_ARG;
    if (((uintptr_t)depth & 15) || ((uintptr_t)out & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)sizes & 3))
        return GDN_ERR_BAD_ARG;
    const size_t bytes = gdn_depth_densify_workspace_bytes(B, Hmax, Wmax);
    if (workspace_bytes < bytes || dz_overlap(depth, out, bytes) || dz_overlap(workspace, out, bytes) ||
        dz_overlap(workspace, depth, bytes))
        return GDN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int ntx = cdiv(Wmax, DZ_TW);
    const dim3 tiles((unsigned)((int64_t)ntx * cdiv(Hmax, DZ_TH)), B);
    float* work = (float*)workspace;
    hipLaunchKernelGGL(densify_fill_kernel, tiles, dim3(DZ_T), 0, st, depth, sizes, Hmax, Wmax, ntx, max_depth, out);
    hipLaunchKernelGGL(densify_extend_kernel, dim3(cdiv(Wmax, E_T), B), dim3(E_T), 0, st, out, sizes, Hmax, Wmax);
    hipLaunchKernelGGL(densify_holes_kernel, tiles, dim3(DZ_T), 0, st, (const float*)out, sizes, Hmax, Wmax, ntx, work);
    hipLaunchKernelGGL(densify_smooth_kernel, tiles, dim3(DZ_T), 0, st, (const float*)work, sizes, Hmax, Wmax, ntx, max_depth, out);
    return gdn_launch_status();
}

extern "C" int gdn_depth_encode_u8(const float* x, int64_t n, double scale, int32_t keep_valid, uint8_t* out, void* stream) {
    (void)hipGetLastError();
    if (!x || !out || n < 1 || !(scale > 0.0) || !(scale < (double)INFINITY) || keep_valid < 0 || keep_valid > 1 ||
        ((uintptr_t)x & 15) || ((uintptr_t)out & 3))
        return GDN_ERR_BAD_ARG;
    hipLaunchKernelGGL(depth_encode_u8_kernel, dim3(stream_blocks(cdiv64(n, 4))), dim3(256), 0, (hipStream_t)stream, x, n, scale,
                       (int)keep_valid, out);
    return gdn_launch_status();
}
#endif
