// Winograd F(2x2, 3x3) convolution for the 512-channel 3x3 residual layers (levels 3 and 4 of G and R: after the
// frequency-domain path took the large windows they are the biggest share of the fp32 step).
//
// A 3x3 stride-1 convolution costs 9 MACs per (pixel, cin, cout); F(2x2,3x3) costs 16 per 2x2 outputs = 4, a 2.25x
// cut with transforms that only add and halve -- the fp32 error stays at the level of the direct sum (rms 1.6x,
// DESIGN.md 2.5), unlike F(4x4,3x3).  The frequency-domain path of conv_fft.hip does not apply here: with 512 channels
// its weight spectrum would be 1.7 GB per layer.
//
//   input     x  -> V [16][tile][Cin]     V = B^T d B of every 4x4 patch (stride 2, zero border)
//   weights   w  -> U [16][Cout][Cin]     U = G g G^T   (data gradient: taps flipped, channel roles swapped)
//   gemm      Mo[bin] = V[bin] * U[bin]^T           16 real GEMMs, M = tiles, K = Cin, N = Cout (fp32 MFMA)
//   output    Mo -> y                                y = A^T m A (2x2 per tile) + the conv_igemm epilogue (BN partials,
//                                                    affine / ReLU / residual)
// Backward: the data gradient is the same pipeline on dy with the flipped / transposed weights; the weight gradient is
// dW = G^T [ sum_tiles (B^T d B) (.) (A dy A^T) ] G: V is kept from the forward, dy gets the 2x2 -> 4x4 transform, the sum
// over tiles is a reduction GEMM per bin on the MFMA, and a last small kernel folds the 16 bins into the 9 taps.
#include "common.h"
#include "bn_math.h"
#include "wino_gemm.h"
#include "up2x.h"
#include "gemm_x3.h"

namespace {

struct WinoGeom {
    int B, H, W, C, N;            // input [B,H,W,C] -> output [B,Ho,Wo,N]
    int Ho, Wo;                   // output extent (= H, W except for the padded-domain data gradient of a reflection layer)
    int pad_off;                  // output (oy, ox) reads input rows oy - pad_off .. oy - pad_off + 2
    int reflect;                  // input border: 0 zeros, 1 mirror (ReflectionPad2d(1) + conv)
    int tiles_y, tiles_x, M;      // 2x2 output tiles; M = B * tiles_y * tiles_x
    int cq_shift, nq_shift;       // log2(C / 64), log2(N / 64)
    int x3;                       // per-bin GEMMs as bf16 x 3 split products (gemm_x3.h) unless the caller set GDN_HINT_NO_X3
    int flip;                     // 0, or WINO_FLIP: a stride-1 ConvTranspose2d given as the convolution it is (GDN_HINT_FLIP_TAPS)
    int T, bins;                  // outputs per tile side and transform bins: F(2x2,3x3) T = 2, 16 bins; F(4x4,3x3) T = 4, 36 bins
};

// V = B^T d B of the 4x4 patch whose top-left corner is (2a - pad_off, 2b - pad_off)
// in_scale != NULL: x is the RAW output of the producer convolution and the layer input is
// [relu](x * in_scale[c] + in_shift[c]) -- the producer's train-mode BatchNorm (+ReLU) applied on load, so that
// activation is never written to memory (ResidualBlock AE_model_unet.py:49-54).  Padding stays zero.
__global__ __launch_bounds__(256) void wino_input_kernel(const float* __restrict__ x, int ldx, float* __restrict__ V, WinoGeom g,
                                                         const float* __restrict__ in_scale, const float* __restrict__ in_shift,
                                                         int in_relu, int up2x) {
    int t, c;
    if (!wino_decode(g.M, g.cq_shift, t, c)) return;
    const float is = in_scale ? in_scale[c] : 1.f, it = in_scale ? in_shift[c] : 0.f;
    const float lo = in_relu ? 0.f : -3.402823466e38f;
    const int b2 = t % g.tiles_x, a2 = (t / g.tiles_x) % g.tiles_y, img = t / (g.tiles_x * g.tiles_y);
    float d[4][4];
    const int lim = g.reflect ? 1 : 0;      // mirrored border rows / columns -1 and H (W); anything further out reads zero
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int iy = 2 * a2 - g.pad_off + i;
        const bool row_ok = iy >= -lim && iy < g.H + lim;
        const int iyr = iy < 0 ? -iy : (iy >= g.H ? 2 * g.H - 2 - iy : iy);
        if (up2x) {
            // x is the LOW-resolution tensor [B][H/2][W/2][ldx]: the x2 bilinear upsampling happens here (up2x.h)
            const int Hl = g.H >> 1, Wl = g.W >> 1;
            float ly; int y0, y1;
            up_src(row_ok ? iyr : 0, Hl, up2x - 1, ly, y0, y1);
            const float* r0 = x + ((size_t)(img * Hl + y0) * Wl) * ldx + c;
            const float* r1 = x + ((size_t)(img * Hl + y1) * Wl) * ldx + c;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ix = 2 * b2 - g.pad_off + j;
                const int ixr = ix < 0 ? -ix : (ix >= g.W ? 2 * g.W - 2 - ix : ix);
                const bool ok = row_ok && ix >= -lim && ix < g.W + lim;
                float v = 0.f;
                if (ok) {
                    float lx; int x0, x1;
                    up_src(ixr, Wl, up2x - 1, lx, x0, x1);
                    v = up2x_at(r0, r1, ldx, ly, x0, x1, lx);
                }
                d[i][j] = v;
            }
            continue;
        }
        const float* row = x + ((size_t)(img * g.H + (row_ok ? iyr : 0)) * g.W) * ldx + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ix = 2 * b2 - g.pad_off + j;
            const int ixr = ix < 0 ? -ix : (ix >= g.W ? 2 * g.W - 2 - ix : ix);
            const bool ok = row_ok && ix >= -lim && ix < g.W + lim;
            float v = ok ? row[(size_t)ixr * ldx] : 0.f;
            if (in_scale) v = ok ? fmaxf(v * is + it, lo) : 0.f;
            d[i][j] = v;
        }
    }
    float r[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {          // B^T along rows
        r[0][j] = d[0][j] - d[2][j];
        r[1][j] = d[1][j] + d[2][j];
        r[2][j] = d[2][j] - d[1][j];
        r[3][j] = d[1][j] - d[3][j];
    }
    float* dst = V + (size_t)t * g.C + c;
    const size_t bs = (size_t)g.M * g.C;
#pragma unroll
    for (int i = 0; i < 4; ++i) {          // ... and along columns
        dst[0] = r[i][0] - r[i][2]; dst += bs; GDN_KEEP(dst);
        dst[0] = r[i][1] + r[i][2]; dst += bs; GDN_KEEP(dst);
        dst[0] = r[i][2] - r[i][1]; dst += bs; GDN_KEEP(dst);
        dst[0] = r[i][1] - r[i][3]; dst += bs; GDN_KEEP(dst);
    }
}

// Dv = A dy A^T of the 2x2 output tile (weight gradient)
__global__ __launch_bounds__(256) void wino_dy_kernel(const float* __restrict__ dy, int ldy, float* __restrict__ Dv, WinoGeom g) {
    int t, n;
    if (!wino_decode(g.M, g.nq_shift, t, n)) return;
    const int b2 = t % g.tiles_x, a2 = (t / g.tiles_x) % g.tiles_y, img = t / (g.tiles_x * g.tiles_y);
    float y[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int oy = 2 * a2 + i, ox = 2 * b2 + j;
            y[i][j] = (oy < g.Ho && ox < g.Wo) ? dy[((size_t)(img * g.Ho + oy) * g.Wo + ox) * ldy + n] : 0.f;
        }
    float s[4][2];                          // A along rows: (y0, y0 + y1, y0 - y1, -y1)
#pragma unroll
    for (int j = 0; j < 2; ++j) { s[0][j] = y[0][j]; s[1][j] = y[0][j] + y[1][j]; s[2][j] = y[0][j] - y[1][j]; s[3][j] = -y[1][j]; }
    float* dst = Dv + (size_t)t * g.N + n;
    const size_t bs = (size_t)g.M * g.N;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        dst[0] = s[i][0]; dst += bs; GDN_KEEP(dst);
        dst[0] = s[i][0] + s[i][1]; dst += bs; GDN_KEEP(dst);
        dst[0] = s[i][0] - s[i][1]; dst += bs; GDN_KEEP(dst);
        dst[0] = -s[i][1]; dst += bs; GDN_KEEP(dst);
    }
}

constexpr int WINO_FLIP = 2;      // bit 1 of the weight kernels' `swap` arguments: a flipped-tap layer (GDN_HINT_FLIP_TAPS)

// U = G g G^T.  swap = 0: U[bin][n][c] from w[tap][n][c] (forward);  swap = 1: U[bin][c][n] from the flipped taps
// (data gradient: correlation of dy with w[n][c][2 - ty][2 - tx], output channel c)
// Uswap != NULL (forward of a layer that will run backward): the data gradient's set (taps flipped: bins permuted
// (3,1,2,0) per axis; channel roles swapped) is written by the same launch from the same nine reads -- the weights do not
// change between a step's forward and backward, so the backward needs no weight transform of its own.
__global__ __launch_bounds__(256) void wino_weights_kernel(const float* __restrict__ w, float* __restrict__ U, int N, int C, int swap,
                                                           float* __restrict__ Uswap) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * C) return;
    const int c = i % C, n = i / C;
    const int rev = (swap & 1) ^ (swap >> 1);       // WINO_FLIP: the layer correlates with the stored taps in reverse order
    swap &= 1;
    float gk[3][3];
#pragma unroll
    for (int ty = 0; ty < 3; ++ty)
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
            const int tap = rev ? (2 - ty) * 3 + (2 - tx) : ty * 3 + tx;
            gk[ty][tx] = w[((size_t)tap * N + n) * C + c];
        }
    float r[4][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        r[0][j] = gk[0][j];
        r[1][j] = 0.5f * (gk[0][j] + gk[1][j] + gk[2][j]);
        r[2][j] = 0.5f * (gk[0][j] - gk[1][j] + gk[2][j]);
        r[3][j] = gk[2][j];
    }
    float* dst = U ? U + (swap ? (size_t)c * N + n : (size_t)n * C + c) : nullptr;      // (U == NULL: only the swapped set)
    const size_t bs = (size_t)N * C;
    float u[4][4];
#pragma unroll
    for (int i2 = 0; i2 < 4; ++i2) {
        u[i2][0] = r[i2][0];
        u[i2][1] = 0.5f * (r[i2][0] + r[i2][1] + r[i2][2]);
        u[i2][2] = 0.5f * (r[i2][0] - r[i2][1] + r[i2][2]);
        u[i2][3] = r[i2][2];
    }
    if (dst) {
#pragma unroll
        for (int i2 = 0; i2 < 4; ++i2)
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) { dst[0] = u[i2][j2]; dst += bs; GDN_KEEP(dst); }
    }
    if (Uswap) {
        // G flip(g) G^T = P (G g G^T) P with P the permutation (3,1,2,0): flipping the taps swaps rows 0 <-> 3 of G g
        float* d2 = Uswap + (size_t)c * N + n;
#pragma unroll
        for (int i2 = 0; i2 < 4; ++i2)
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) {
                const int pi = i2 == 0 ? 3 : (i2 == 3 ? 0 : i2), pj = j2 == 0 ? 3 : (j2 == 3 ? 0 : j2);
                d2[0] = u[pi][pj]; d2 += bs; GDN_KEEP(d2);
            }
    }
}

// The same transform written as bf16 x 3 packed panels (gemm_x3.h) for the GEMMs that run on the bf16 matrix pipe.
// swap = 0: rows = n (output channel), k = c -- the forward's B operand U[bin][n][c];  swap = 1: rows = c, k = n from the
// flipped taps -- the data gradient's.  thread = (row, 8 consecutive k): 9 taps x 8 values in, 16 bins x 3 planes x 16 bytes out.
// grid.y selects the set: y = 0 -> (Up, swap), y = 1 -> (Up1, swap1): a forward that will run backward writes both in one launch.
__global__ __launch_bounds__(256) void wino_weights_x3_kernel(const float* __restrict__ w, unsigned char* __restrict__ Up0, int N, int C,
                                                              int swap0, unsigned char* __restrict__ Up1, int swap1) {
    unsigned char* __restrict__ Up = blockIdx.y ? Up1 : Up0;
    const int swapf = blockIdx.y ? swap1 : swap0;
    const int swap = swapf & 1, rev = swap ^ (swapf >> 1);       // WINO_FLIP, as in wino_weights_kernel
    const int rows = swap ? C : N, K = swap ? N : C, k8n = K / 8;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * k8n) return;
    // a wave = 16 consecutive rows x the 4 chunks of ONE k block: 1 KB contiguous per (bin, plane) store in the packed layout;
    // its loads are 16 runs of 128 B (k = c contiguous) or 8 x 4 runs of 64 B (swap: k = n, stride C)
    const int row = (i >> 2) % rows, k8 = (i & 3) + 4 * ((i >> 2) / rows);
    float gk[8][3][3];
#pragma unroll
    for (int ty = 0; ty < 3; ++ty)
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
            const int tap = rev ? (2 - ty) * 3 + (2 - tx) : ty * 3 + tx;
            if (swap) {
#pragma unroll
                for (int e = 0; e < 8; ++e) gk[e][ty][tx] = w[((size_t)tap * N + k8 * 8 + e) * C + row];
            } else {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(w + ((size_t)tap * N + row) * C + k8 * 8);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(w + ((size_t)tap * N + row) * C + k8 * 8 + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { gk[e][ty][tx] = lo[e]; gk[4 + e][ty][tx] = hi[e]; }
            }
        }
    const int KB = K / X3_BK;
    const size_t per_bin = x3_packed_bytes(rows, K);
    unsigned char* dst = Up + x3_off(row, k8 * 8, 0, KB);
#pragma unroll
    for (int i2 = 0; i2 < 4; ++i2)
#pragma unroll
        for (int j2 = 0; j2 < 4; ++j2) {
            unsigned h[3][4];
            float uu[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // (G g G^T)[i2][j2]: rows of G = (1,0,0), (.5,.5,.5), (.5,-.5,.5), (0,0,1)
                float r[3];
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    r[j] = i2 == 0 ? gk[e][0][j] : i2 == 3 ? gk[e][2][j]
                         : 0.5f * (i2 == 1 ? gk[e][0][j] + gk[e][1][j] + gk[e][2][j] : gk[e][0][j] - gk[e][1][j] + gk[e][2][j]);
                uu[e] = j2 == 0 ? r[0] : j2 == 3 ? r[2] : 0.5f * (j2 == 1 ? r[0] + r[1] + r[2] : r[0] - r[1] + r[2]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) x3_split2(uu[2 * q], uu[2 * q + 1], h[0][q], h[1][q], h[2][q]);
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const uint4 v = {h[p][0], h[p][1], h[p][2], h[p][3]};
                *reinterpret_cast<uint4*>(dst + (size_t)(i2 * 4 + j2) * per_bin + (size_t)p * 128 * 64) = v;
            }
        }
}

// epilogue of the two output kernels: the conv_igemm one (residual, BatchNorm partials, affine / activation) and, for a data
// gradient, the BatchNorm-backward partials
// bnb_y != NULL (data gradient): y is the gradient of a train-mode BatchNorm's output z = [relu](BN(bnb_y)); `stats` then
// receives that layer's backward partials (sum dz, sum dz*xhat per slot; bnb_co = [scale, shift, mean, invstd][Nout])
// instead of sum / sum of squares, so the stand-alone reduce pass over (dy, y) disappears.
struct WinoEp {
    const float* addsrc; int ld_add;
    float* stats;
    const float* ep_scale; const float* ep_shift;
    int act;
    const float* bnb_y; int ld_bnb;
    const float* bnb_co; int bnb_relu;
};

// y = A^T m A (2x2 outputs per tile) with the epilogue above; stats slot = group of 4 tiles
__global__ __launch_bounds__(256) void wino_output_kernel(const float* __restrict__ Mo, float* __restrict__ y, int ldy, WinoEp ep,
                                                          WinoGeom g, int Nout, int q_shift) {
    int t, n;
    const bool live = wino_decode(g.M, q_shift, t, n);
    float s1 = 0.f, s2 = 0.f;
    if (live) {
        const int b2 = t % g.tiles_x, a2 = (t / g.tiles_x) % g.tiles_y, img = t / (g.tiles_x * g.tiles_y);
        float m[4][4];
        const float* src = Mo + (size_t)t * Nout + n;
        const size_t bs = (size_t)g.M * Nout;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) { m[i][j] = *src; src += bs; GDN_KEEP(src); }
        float r[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { r[0][j] = m[0][j] + m[1][j] + m[2][j]; r[1][j] = m[1][j] - m[2][j] - m[3][j]; }
        const float es = ep.ep_scale ? ep.ep_scale[n] : 1.f, et = ep.ep_shift ? ep.ep_shift[n] : 0.f;
        float bsc = 0.f, bt = 0.f, bmu = 0.f, bis = 0.f;
        if (ep.bnb_y) { bsc = ep.bnb_co[n]; bt = ep.bnb_co[Nout + n]; bmu = ep.bnb_co[2 * Nout + n]; bis = ep.bnb_co[3 * Nout + n]; }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float o[2] = {r[i][0] + r[i][1] + r[i][2], r[i][1] - r[i][2] - r[i][3]};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int oy = 2 * a2 + i, ox = 2 * b2 + j;
                if (oy < g.Ho && ox < g.Wo) {
                    float val = o[j];
                    if (!ep.bnb_y) { s1 += val; s2 += val * val; }
                    if (ep.ep_scale) val = val * es + et;
                    if (ep.act & GDN_ACT_RELU) val = fmaxf(val, 0.f);
                    const size_t px = (size_t)(img * g.Ho + oy) * g.Wo + ox;
                    if (ep.addsrc) val += ep.addsrc[px * ep.ld_add + n];
                    if (ep.act & GDN_ACT_TANH) val = tanhf(val);
                    y[px * ldy + n] = val;
                    if (ep.bnb_y) {
                        const float yv = ep.bnb_y[px * ep.ld_bnb + n];
                        const float dz = bn_dz(val, yv, bsc, bt, ep.bnb_relu);
                        s1 += dz; s2 += dz * bn_xhat(yv, bmu, bis);
                    }
                }
            }
        }
    }
    if (ep.stats) wino_stats_store(s1, s2, ep.stats, q_shift, Nout);
}

// dW[tap][n][c] = (G^T P G)[ty][tx]
// flip (a flipped-tap layer): tap t is the gradient of stored tap 8 - t
__global__ __launch_bounds__(256) void wino_wgrad_output_kernel(const float* __restrict__ P, float* __restrict__ dw, int N, int C,
                                                                int nsplit, int flip) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * C) return;
    float p[4][4];
    const float* src = P + i;
    const size_t bs = (size_t)N * C;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            float v = *src;
            for (int sp = 1; sp < nsplit; ++sp) v += src[(size_t)sp * WINO_BINS * bs];      // split reduction, fixed order
            p[a][b] = v; src += bs; GDN_KEEP(src);
        }
    float r[3][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        r[0][b] = p[0][b] + 0.5f * (p[1][b] + p[2][b]);
        r[1][b] = 0.5f * (p[1][b] - p[2][b]);
        r[2][b] = 0.5f * (p[1][b] + p[2][b]) + p[3][b];
    }
#pragma unroll
    for (int ty = 0; ty < 3; ++ty) {
        const int t0 = ty * 3;
        dw[(size_t)(flip ? 8 - t0 : t0) * bs + i] = r[ty][0] + 0.5f * (r[ty][1] + r[ty][2]);
        dw[(size_t)(flip ? 7 - t0 : t0 + 1) * bs + i] = 0.5f * (r[ty][1] - r[ty][2]);
        dw[(size_t)(flip ? 6 - t0 : t0 + 2) * bs + i] = 0.5f * (r[ty][1] + r[ty][2]) + r[ty][3];
    }
}


// ---- F(4x4, 3x3): 6x6 patches, 36 bins, 2.25 multiplications per output instead of 4 (and 2.25 transformed values per pixel
// instead of 4).  Interpolation points 0, +-a, +-b, inf with a = 5/8, b = 3/2 -- NOT the textbook 0, +-1, +-2: in fp32 (transforms
// rounded, products exact: what the bf16 x 3 GEMMs deliver) the textbook set has 2.0x the rms and 4x the worst-case error of this
// one, whose rms is 1.25x the direct fp32 sum's (numpy model, tests/test_winoconv_model_cpu.py; a scan of dyadic pairs is flat
// around a ~ 0.6-0.7, b ~ 1.5, i.e. a b ~ 1).  Both values are dyadic, so every power and every entry of B^T is exact in fp32.
// With M(x) = x (x^2 - a^2)(x^2 - b^2):  B^T rows = coefficients of M(x) / (x - p) (row inf: M itself),  G rows = (1, p, p^2) / N_p
// with N_p = prod_{q != p} (p - q) (row inf: (0, 0, 1)),  A^T columns = (1, p, p^2, p^3) (column inf: (0, 0, 0, 1)).
// The weight gradient is F(3x3,4x4) on the same points: the saved B^T d B is reused, dy takes G_w (6x4: rows (1, p, p^2, p^3) / N_p),
// the reduction over tiles is the TN GEMM, and A_w^T (3x6: columns (1, p, p^2), column inf (0, 0, 1)) folds the 36 bins into 9 taps.
// F(2x2,3x3) stays for reflection-padded layers, small images and the fp32-matrix-pipe fallback.
#define W4_A 0.625f
#define W4_B 1.5f
constexpr float W4_A2 = W4_A * W4_A, W4_B2 = W4_B * W4_B, W4_A3 = W4_A2 * W4_A, W4_B3 = W4_B2 * W4_B;
constexpr float W4_P = W4_A2 * W4_B2, W4_S = W4_A2 + W4_B2;                                       // a^2 b^2, a^2 + b^2
constexpr float W4_I0 = (float)(1.0 / ((double)W4_A2 * W4_B2));                                  // 1 / N_0
constexpr float W4_IA = (float)(1.0 / (2.0 * W4_A2 * ((double)W4_A2 - W4_B2)));                  // 1 / N_a = 1 / N_-a
constexpr float W4_IB = (float)(1.0 / (2.0 * W4_B2 * ((double)W4_B2 - W4_A2)));                  // 1 / N_b = 1 / N_-b
// B^T (6x6) and A^T (4x6) are PINNED: no contraction by the compiler, a fused multiply-add exactly where it is written.  Left to
// the compiler, which products fuse depends on the code around the call (a select next to a load is enough to move one), and
// every rescheduling of a transform kernel would change what training computes.  The forms below are the ones the compiler
// had chosen for the input / output transforms when they were pinned (recovered by matching candidate forms against the
// kernels' output bits) -- they were not the same in every instance, hence the switches:
//   W4_FP / W4_FS / W4_F0   rows 0 and 5,  P x - S y + z :  fma(P, x, -(S y)) + z  /  fma(-S, y, P x) + z  /  (P x - S y) + z
//   fodd                    rows 1..4,  e +- k i :  fma(+-k, i, e)  or  e +- (k i)        (e and i are always fused)
// w4_g, w4_gw and w4_awt (weight and weight-gradient transforms) are still the compiler's choice, each in its own kernel(s).
enum { W4_FP = 0, W4_FS = 1, W4_F0 = 2 };
__device__ __forceinline__ float w4_bt_edge(int f, float x, float y, float z) {
#pragma clang fp contract(off)
    if (f == W4_FP) return __builtin_fmaf(W4_P, x, -(W4_S * y)) + z;
    if (f == W4_FS) return __builtin_fmaf(-W4_S, y, W4_P * x) + z;
    return (W4_P * x - W4_S * y) + z;
}
// (f0, fodd, f5 are constants at every call once the loops around it are unrolled)
__device__ __forceinline__ void w4_bt(const float (&d)[6], float (&o)[6], int f0, bool fodd, int f5) {
#pragma clang fp contract(off)
    const float ea = __builtin_fmaf(-W4_B2, d[2], d[4]), ia = __builtin_fmaf(-W4_B2, d[1], d[3]);      // d4 - b^2 d2,  d3 - b^2 d1
    const float eb = __builtin_fmaf(-W4_A2, d[2], d[4]), ib = __builtin_fmaf(-W4_A2, d[1], d[3]);
    o[0] = w4_bt_edge(f0, d[0], d[2], d[4]);
    if (fodd) {
        o[1] = __builtin_fmaf(W4_A, ia, ea);
        o[2] = __builtin_fmaf(-W4_A, ia, ea);
        o[3] = __builtin_fmaf(W4_B, ib, eb);
        o[4] = __builtin_fmaf(-W4_B, ib, eb);
    } else {
        const float oa = W4_A * ia, ob = W4_B * ib;
        o[1] = ea + oa;
        o[2] = ea - oa;
        o[3] = eb + ob;
        o[4] = eb - ob;
    }
    o[5] = w4_bt_edge(f5, d[1], d[3], d[5]);
}
// the two passes of V = B^T d B as the input transform runs them: along the rows of patch column j, then along the columns of
// row i of the result
__device__ __forceinline__ void w4_bt_rows(int j, const float (&d)[6], float (&o)[6]) { w4_bt(d, o, W4_FP, j != 5, W4_FP); }
__device__ __forceinline__ void w4_bt_cols(int i, const float (&r)[6], float (&o)[6]) {
    w4_bt(r, o, W4_F0, true, (i == 0 || i == 5) ? W4_FP : W4_FS);
}
__device__ __forceinline__ void w4_g(const float (&g)[3], float (&o)[6]) {        // G (6x3)
    const float ea = W4_IA * (g[0] + W4_A2 * g[2]), oa = (W4_IA * W4_A) * g[1];
    const float eb = W4_IB * (g[0] + W4_B2 * g[2]), ob = (W4_IB * W4_B) * g[1];
    o[0] = W4_I0 * g[0];
    o[1] = ea + oa;
    o[2] = ea - oa;
    o[3] = eb + ob;
    o[4] = eb - ob;
    o[5] = g[2];
}
__device__ __forceinline__ void w4_gw(const float (&y)[4], float (&o)[6]) {       // G_w (6x4)
    const float ea = W4_IA * (y[0] + W4_A2 * y[2]), oa = (W4_IA * W4_A) * (y[1] + W4_A2 * y[3]);
    const float eb = W4_IB * (y[0] + W4_B2 * y[2]), ob = (W4_IB * W4_B) * (y[1] + W4_B2 * y[3]);
    o[0] = W4_I0 * y[0];
    o[1] = ea + oa;
    o[2] = ea - oa;
    o[3] = eb + ob;
    o[4] = eb - ob;
    o[5] = y[3];
}
__device__ __forceinline__ void w4_at(const float (&m)[6], float (&o)[4]) {       // A^T (4x6)
#pragma clang fp contract(off)
    const float s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
    o[0] = m[0] + s12 + s34;
    o[1] = __builtin_fmaf(W4_A, d12, W4_B * d34);
    o[2] = __builtin_fmaf(W4_A2, s12, W4_B2 * s34);
    o[3] = __builtin_fmaf(W4_A3, d12, W4_B3 * d34) + m[5];
}
// a product that is rounded on its own, never contracted into the sum it feeds (the partial sums of wino4_output_kernel)
__device__ __forceinline__ float w4_mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ void w4_awt(const float (&p)[6], float (&o)[3]) {      // A_w^T (3x6)
    const float s12 = p[1] + p[2], d12 = p[1] - p[2], s34 = p[3] + p[4], d34 = p[3] - p[4];
    o[0] = p[0] + s12 + s34;
    o[1] = W4_A * d12 + W4_B * d34;
    o[2] = W4_A2 * s12 + W4_B2 * s34 + p[5];
}

// A wave of the transform kernels is one tile (wino_decode: 64 channels of tile t), so everything derived from t -- the tile's
// image and position, which patch rows / columns lie in the image, the row bases -- is uniform over the wave.  Computed from
// threadIdx the compiler keeps it in vector registers; WINO_UNI moves t to a scalar register once, which makes the bounds
// logic scalar arithmetic and every access a scalar base + the lane's channel.
#define WINO_UNI(v) __builtin_amdgcn_readfirstlane(v)

// V = B^T d B of the 6x6 patch whose top-left corner is (4a - pad_off, 4b - pad_off); in_scale as wino_input_kernel, a
// compile-time switch here (zero padding only: reflection-padded layers stay on F(2x2,3x3)).
// Branch-free loader: a patch element outside the image is read from the nearest pixel inside it (clamped row / column: 6 + 6
// predicates and bases per wave, not 36 pairs) and replaced by zero with one select, so all 36 loads of a thread are in flight
// before the first use -- per-element `if (ok)` regions made them 36 memory round trips one after another.
template <bool INSC>
__global__ __launch_bounds__(256) void wino4_input_kernel(const float* __restrict__ x, int ldx, float* __restrict__ V, WinoGeom g,
                                                          const float* __restrict__ in_scale, const float* __restrict__ in_shift,
                                                          int in_relu) {
    int tv, c;
    if (!wino_decode(g.M, g.cq_shift, tv, c)) return;
    const int t = WINO_UNI(tv);
    float is = 1.f, it = 0.f;
    if (INSC) { is = in_scale[c]; it = in_shift[c]; }
    const float lo = in_relu ? 0.f : -3.402823466e38f;
    const int b2 = t % g.tiles_x, a2 = (t / g.tiles_x) % g.tiles_y, img = t / (g.tiles_x * g.tiles_y);
    const float* rowp[6];                    // patch row i (clamped into the image), column 0, channel 0
    size_t colo[6];                          // patch column j (clamped): element offset within a row
    bool row_ok[6], col_ok[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int iy = 4 * a2 - g.pad_off + k, ix = 4 * b2 - g.pad_off + k;
        row_ok[k] = iy >= 0 && iy < g.H;
        col_ok[k] = ix >= 0 && ix < g.W;
        const int iyc = iy < 0 ? 0 : (iy < g.H ? iy : g.H - 1), ixc = ix < 0 ? 0 : (ix < g.W ? ix : g.W - 1);
        rowp[k] = x + ((size_t)(img * g.H + iyc) * g.W) * ldx;
        colo[k] = (size_t)ixc * ldx;
    }
    float d[6][6];                           // d[j][i]: patch column j, row i
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int i = 0; i < 6; ++i) d[j][i] = (rowp[i] + colo[j])[(unsigned)c];
    float r[6][6];                           // B^T along rows, one patch column at a time
#pragma unroll
    for (int j = 0; j < 6; ++j) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            float v = d[j][i];
            if (INSC) v = fmaxf(v * is + it, lo);
            d[j][i] = (row_ok[i] && col_ok[j]) ? v : 0.f;
        }
        float o[6];
        w4_bt_rows(j, d[j], o);
#pragma unroll
        for (int i = 0; i < 6; ++i) r[i][j] = o[i];
    }
    float* dst = V + (size_t)t * g.C + c;
    const size_t bs = (size_t)g.M * g.C;
#pragma unroll
    for (int i = 0; i < 6; ++i) {            // ... and along columns
        float o[6];
        w4_bt_cols(i, r[i], o);
#pragma unroll
        for (int j = 0; j < 6; ++j) { dst[0] = o[j]; dst += bs; GDN_KEEP(dst); }
    }
}

// The same on a LOW-resolution x [B][H/2][W/2][ldx]: the x2 bilinear upsampling happens on load (up2x.h; up2x - 1 =
// align_corners).  Only the legacy network's flipped-tap layer runs it, so it keeps the per-element loader; no BatchNorm-on-load
// here (gdn_winoconv_fwd refuses the combination).
__global__ __launch_bounds__(256) void wino4_input_up2x_kernel(const float* __restrict__ x, int ldx, float* __restrict__ V, WinoGeom g,
                                                               int up2x) {
    int t, c;
    if (!wino_decode(g.M, g.cq_shift, t, c)) return;
    const int b2 = t % g.tiles_x, a2 = (t / g.tiles_x) % g.tiles_y, img = t / (g.tiles_x * g.tiles_y);
    float r[6][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int ix = 4 * b2 - g.pad_off + j;
        const bool col_ok = ix >= 0 && ix < g.W;
        float d[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int iy = 4 * a2 - g.pad_off + i;
            const bool ok = col_ok && iy >= 0 && iy < g.H;
            float v = 0.f;
            if (ok) {
                const int Hl = g.H >> 1, Wl = g.W >> 1;
                float ly, lx; int y0, y1, x0, x1;
                up_src(iy, Hl, up2x - 1, ly, y0, y1);
                up_src(ix, Wl, up2x - 1, lx, x0, x1);
                v = up2x_at(x + ((size_t)(img * Hl + y0) * Wl) * ldx + c, x + ((size_t)(img * Hl + y1) * Wl) * ldx + c, ldx, ly, x0, x1, lx);
            }
            d[i] = v;
        }
        float o[6];
        w4_bt_rows(j, d, o);
#pragma unroll
        for (int i = 0; i < 6; ++i) r[i][j] = o[i];
    }
    float* dst = V + (size_t)t * g.C + c;
    const size_t bs = (size_t)g.M * g.C;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float o[6];
        w4_bt_cols(i, r[i], o);
#pragma unroll
        for (int j = 0; j < 6; ++j) { dst[0] = o[j]; dst += bs; GDN_KEEP(dst); }
    }
}

// Dv = G_w dy G_w^T of the 4x4 output tile (weight gradient)
__global__ __launch_bounds__(256) void wino4_dy_kernel(const float* __restrict__ dy, int ldy, float* __restrict__ Dv, WinoGeom g) {
    int t, n;
    if (!wino_decode(g.M, g.nq_shift, t, n)) return;
    const int b2 = t % g.tiles_x, a2 = (t / g.tiles_x) % g.tiles_y, img = t / (g.tiles_x * g.tiles_y);
    float s[6][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ox = 4 * b2 + j;
        float y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int oy = 4 * a2 + i;
            y[i] = (oy < g.Ho && ox < g.Wo) ? dy[((size_t)(img * g.Ho + oy) * g.Wo + ox) * ldy + n] : 0.f;
        }
        float o[6];
        w4_gw(y, o);
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i][j] = o[i];
    }
    float* dst = Dv + (size_t)t * g.N + n;
    const size_t bs = (size_t)g.M * g.N;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float o[6];
        w4_gw(s[i], o);
#pragma unroll
        for (int j = 0; j < 6; ++j) { dst[0] = o[j]; dst += bs; GDN_KEEP(dst); }
    }
}

// U = G g G^T as bf16 x 3 packed panels, 36 bins (arguments as wino_weights_x3_kernel)
__global__ __launch_bounds__(256) void wino4_weights_x3_kernel(const float* __restrict__ w, unsigned char* __restrict__ Up0, int N, int C,
                                                               int swap0, unsigned char* __restrict__ Up1, int swap1) {
    unsigned char* __restrict__ Up = blockIdx.y ? Up1 : Up0;
    const int swapf = blockIdx.y ? swap1 : swap0;
    const int swap = swapf & 1, rev = swap ^ (swapf >> 1);       // WINO_FLIP, as in wino_weights_kernel
    const int rows = swap ? C : N, K = swap ? N : C, k8n = K / 8;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * k8n) return;
    // a wave = 16 consecutive rows x the 4 chunks of ONE k block: 1 KB contiguous per (bin, plane) store in the packed layout
    // (thread = (row, consecutive k8) wrote sixteen 64-byte pieces 24 KB apart per store: 54 us for 113 MB at 512 channels)
    const int row = (i >> 2) % rows, k8 = (i & 3) + 4 * ((i >> 2) / rows);
    float r[8][6][3];                        // G along the tap rows, per k value
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
        float gk[8][3];
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) {
            const int tap = rev ? (2 - ty) * 3 + (2 - tx) : ty * 3 + tx;
            if (swap) {
#pragma unroll
                for (int e = 0; e < 8; ++e) gk[e][ty] = w[((size_t)tap * N + k8 * 8 + e) * C + row];
            } else {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(w + ((size_t)tap * N + row) * C + k8 * 8);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(w + ((size_t)tap * N + row) * C + k8 * 8 + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { gk[e][ty] = lo[e]; gk[4 + e][ty] = hi[e]; }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float o[6];
            w4_g(gk[e], o);
#pragma unroll
            for (int i2 = 0; i2 < 6; ++i2) r[e][i2][tx] = o[i2];
        }
    }
    const int KB = K / X3_BK;
    const size_t per_bin = x3_packed_bytes(rows, K);
    unsigned char* dst = Up + x3_off(row, k8 * 8, 0, KB);
#pragma unroll
    for (int i2 = 0; i2 < 6; ++i2) {
        float uu[8][6];
#pragma unroll
        for (int e = 0; e < 8; ++e) w4_g(r[e][i2], uu[e]);
#pragma unroll
        for (int j2 = 0; j2 < 6; ++j2) {
            unsigned h[3][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) x3_split2(uu[2 * q][j2], uu[2 * q + 1][j2], h[0][q], h[1][q], h[2][q]);
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const uint4 v = {h[p][0], h[p][1], h[p][2], h[p][3]};
                *reinterpret_cast<uint4*>(dst + (size_t)(i2 * 6 + j2) * per_bin + (size_t)p * 128 * 64) = v;
            }
        }
    }
}

// y = A^T m A (4x4 outputs per tile); epilogue, BatchNorm partials and the data gradient's BatchNorm-backward partials exactly as
// wino_output_kernel (stats slot = group of 4 tiles).  ADD / BNB: addsrc / bnb_y given, as compile-time switches, so that the
// tile's 16 addsrc and 16 bnb_y values are loaded next to the 36 bins (pixels outside the image from the nearest one inside it,
// never used) and all of them are in flight together; the 16 outputs are computed, then stored under the tile's 4 + 4 row /
// column predicates, which are scalar (WINO_UNI).
template <bool ADD, bool BNB>
__global__ __launch_bounds__(256) void wino4_output_kernel(const float* __restrict__ Mo, float* __restrict__ y, int ldy, WinoEp ep,
                                                           WinoGeom g, int Nout, int q_shift) {
    int tv, n;
    const bool live = wino_decode(g.M, q_shift, tv, n);
    float s1 = 0.f, s2 = 0.f;
    if (live) {
        const int t = WINO_UNI(tv);
        const int b2 = t % g.tiles_x, a2 = (t / g.tiles_x) % g.tiles_y, img = t / (g.tiles_x * g.tiles_y);
        size_t rowpx[4];                     // first pixel of output row i (clamped into the image)
        int colpx[4];
        bool row_ok[4], col_ok[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int oy = 4 * a2 + k, ox = 4 * b2 + k;
            row_ok[k] = oy < g.Ho;
            col_ok[k] = ox < g.Wo;
            rowpx[k] = (size_t)(img * g.Ho + (oy < g.Ho ? oy : g.Ho - 1)) * g.Wo;
            colpx[k] = ox < g.Wo ? ox : g.Wo - 1;
        }
        float av[4][4], yv[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t px = rowpx[i] + colpx[j];
                av[i][j] = ADD ? (ep.addsrc + px * ep.ld_add)[(unsigned)n] : 0.f;
                yv[i][j] = BNB ? (ep.bnb_y + px * ep.ld_bnb)[(unsigned)n] : 0.f;
            }
        // (no branch around these two loads either -- the join would wait for everything issued above: without an affine they
        // read Mo[n], which exists, and the value is dropped)
        const float esl = (ep.ep_scale ? ep.ep_scale : Mo)[(unsigned)n], etl = (ep.ep_shift ? ep.ep_shift : Mo)[(unsigned)n];
        const float es = ep.ep_scale ? esl : 1.f, et = ep.ep_shift ? etl : 0.f;
        float bsc = 0.f, bt = 0.f, bmu = 0.f, bis = 0.f;
        if (BNB) { bsc = ep.bnb_co[n]; bt = ep.bnb_co[Nout + n]; bmu = ep.bnb_co[2 * Nout + n]; bis = ep.bnb_co[3 * Nout + n]; }
        float r[4][6];                       // A^T along rows, one bin column at a time
        const float* src = Mo + (size_t)t * Nout + n;
        const size_t bs = (size_t)g.M * Nout;
        {
            float m[6][6];
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = 0; j < 6; ++j) { m[i][j] = *src; src += bs; GDN_KEEP(src); }
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const float col[6] = {m[0][j], m[1][j], m[2][j], m[3][j], m[4][j], m[5][j]};
                float o[4];
                w4_at(col, o);
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i][j] = o[i];
            }
        }
        float out[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float o[4];
            w4_at(r[i], o);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = row_ok[i] && col_ok[j];
                float val = o[j];
                if (!BNB) { s1 = ok ? s1 + val : s1; s2 = ok ? s2 + w4_mul_rn(val, val) : s2; }
                if (ep.ep_scale) val = val * es + et;
                if (ep.act & GDN_ACT_RELU) val = fmaxf(val, 0.f);
                if (ADD) val += av[i][j];
                if (ep.act & GDN_ACT_TANH) val = tanhf(val);
                out[i][j] = val;
                if (BNB) {
                    const float dz = bn_dz(val, yv[i][j], bsc, bt, ep.bnb_relu);
                    s1 = ok ? s1 + dz : s1; s2 = ok ? s2 + w4_mul_rn(dz, bn_xhat(yv[i][j], bmu, bis)) : s2;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (row_ok[i] && col_ok[j]) (y + (rowpx[i] + colpx[j]) * ldy)[(unsigned)n] = out[i][j];
    }
    if (ep.stats) wino_stats_store(s1, s2, ep.stats, q_shift, Nout);
}

// dW[tap][n][c] = (A_w^T P A_w)[ty][tx], the split partial products summed in order
__global__ __launch_bounds__(256) void wino4_wgrad_output_kernel(const float* __restrict__ P, float* __restrict__ dw, int N, int C,
                                                                 int nsplit, int flip) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * C) return;
    const float* src = P + i;
    const size_t bs = (size_t)N * C;
    float r[3][6];
    {
        float p[6][6];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                float v = *src;
                for (int sp = 1; sp < nsplit; ++sp) v += src[(size_t)sp * 36 * bs];
                p[a][b] = v; src += bs; GDN_KEEP(src);
            }
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const float col[6] = {p[0][b], p[1][b], p[2][b], p[3][b], p[4][b], p[5][b]};
            float o[3];
            w4_awt(col, o);
#pragma unroll
            for (int a = 0; a < 3; ++a) r[a][b] = o[a];
        }
    }
#pragma unroll
    for (int ty = 0; ty < 3; ++ty) {
        float o[3];
        w4_awt(r[ty], o);
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) dw[(size_t)(flip ? 8 - (ty * 3 + tx) : ty * 3 + tx) * bs + i] = o[tx];
    }
}

bool wino_geom(const gdn_conv_geom* g, WinoGeom& f) {
    if (!g || g->transposed || g->stride != 1 || g->k != 3 || g->pad != 1) return false;
    if ((g->hints & GDN_HINT_FLIP_TAPS) && g->pad_mode != 0) return false;
    f.flip = (g->hints & GDN_HINT_FLIP_TAPS) ? WINO_FLIP : 0;
    if (g->pad_mode == 1 && (g->H < 4 || g->W < 4)) return false;        // mirrored rows 1 and H-2 must be distinct interior rows
    if ((g->Cin % 64) || (g->Cout % 64) || g->Cin > 512 || g->Cout > 512) return false;
    auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
    if (!pow2(g->Cin / 64) || !pow2(g->Cout / 64)) return false;
    f.B = g->B; f.H = g->H; f.W = g->W; f.C = g->Cin; f.N = g->Cout;
    f.Ho = g->H; f.Wo = g->W; f.pad_off = 1; f.reflect = g->pad_mode == 1;
    f.tiles_y = cdiv(g->H, 2); f.tiles_x = cdiv(g->W, 2);
    f.M = g->B * f.tiles_y * f.tiles_x;
    f.cq_shift = 0; while ((64 << f.cq_shift) < f.C) ++f.cq_shift;
    f.nq_shift = 0; while ((64 << f.nq_shift) < f.N) ++f.nq_shift;
    f.x3 = (g->hints & GDN_HINT_NO_X3) ? 0 : 1;
    f.T = 2; f.bins = WINO_BINS;
    // F(4x4,3x3) where every GEMM of the layer runs as bf16 x 3 split products (the transformed weights exist as panels only),
    // the border is zero padding, and rounding the image up to whole 4 x 4 tiles computes at most 15 % more pixels.
    // GDN_HINT_NO_WINO_F4 in the geometry keeps F(2x2,3x3) (A/B measurements, accuracy studies; gdn_amd/ops.py: set_wino_f4).  Like
    // the bf16 x 3 switch it is part of the geometry -- no environment read -- so the forward that lays out the saved state and the
    // backward that reads it agree on the plan by construction.
    if (f.x3 && !f.reflect && g->H >= 4 && g->W >= 4 && !(g->hints & GDN_HINT_NO_WINO_F4)) {
        const int ty = cdiv(g->H, 4), tx = cdiv(g->W, 4), M4 = g->B * ty * tx;
        const bool fits = (int64_t)ty * tx * 16 * 100 <= (int64_t)g->H * g->W * 115;
        if (fits && gemm_x3_ok(M4, f.N, f.C) && gemm_x3_ok(M4, f.C, f.N) && gemm_x3_tn_ok(M4, f.N, f.C)) {
            f.T = 4; f.bins = 36; f.tiles_y = ty; f.tiles_x = tx; f.M = M4;
        }
    }
    return true;
}

inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }
inline size_t v_bytes(const WinoGeom& f) { return al256((size_t)f.bins * f.M * f.C * 4); }
// transformed weights: fp32 [16][N][C], or the bf16 x 3 panels of either orientation (rows padded to whole 128-row tiles)
inline size_t u_bytes(const WinoGeom& f) {
    size_t b = (size_t)f.bins * f.N * f.C * 4;
    const size_t p1 = (size_t)f.bins * x3_packed_bytes(f.N, f.C), p2 = (size_t)f.bins * x3_packed_bytes(f.C, f.N);
    if (p1 > b) b = p1;
    if (p2 > b) b = p2;
    return al256(b);
}
// GDN_HINT_NO_X3 in the geometry keeps every per-bin GEMM on the fp32 MFMA (ranks that share a GPU, A/B measurements, accuracy
// studies).  It is part of the layer's geometry, so the forward that writes the saved weight set and the backward that reads
// it agree on its form by construction.
inline size_t m_bytes(const WinoGeom& f) { return al256((size_t)f.bins * f.M * f.N * 4); }
inline bool tn_x3(const WinoGeom& f) { return f.x3 && gemm_x3_tn_ok(f.M, f.N, f.C); }
inline int tn_splits(const WinoGeom& f) { return tn_x3(f) ? gemm_x3_tn_splits(f.bins, f.M, f.N, f.C) : wino_tn_splits(f.M, f.N, f.C); }
// (workspace sizing: the larger of the two kernels' split counts)
inline int tn_splits_max(const WinoGeom& f) {
    const int a = wino_tn_splits(f.M, f.N, f.C), b = gemm_x3_tn_ok(f.M, f.N, f.C) ? gemm_x3_tn_splits(f.bins, f.M, f.N, f.C) : 1;
    return a > b ? a : b;
}
inline size_t p_bytes(const WinoGeom& f) { return (size_t)tn_splits_max(f) * al256((size_t)f.bins * f.N * f.C * 4); }   // one set per split
// The NT GEMM Cm[bin] = A[bin] * U[bin]^T of geometry f (M tiles, N outputs, K = C) runs as bf16 x 3 split products where the
// shape allows, and its weight set is then written as panels.  True for every GEMM of an F(4x4,3x3) plan (wino_geom).  The tile
// count does not enter, so the padded-domain data gradient of a reflection layer reads the form the forward saved.
inline bool nt_x3(const WinoGeom& f) { return f.x3 && gemm_x3_ok(f.M, f.N, f.C); }

// The data gradient of a 3x3 layer is the same kind of convolution of dy with flipped, role-swapped taps: pad 1 onto the H x W
// input for a zero-padded layer; pad 2 onto the (H+2) x (W+2) padded domain for a reflection-padded one (always F(2x2,3x3)),
// whose border rows / columns are then folded back onto the rows they mirror.
inline WinoGeom dgrad_geom(const WinoGeom& f) {
    WinoGeom fd = f;
    fd.C = f.N; fd.N = f.C; fd.cq_shift = f.nq_shift; fd.nq_shift = f.cq_shift; fd.reflect = 0;
    if (f.reflect) {
        fd.Ho = f.H + 2; fd.Wo = f.W + 2; fd.pad_off = 2;
        fd.tiles_y = cdiv(fd.Ho, f.T); fd.tiles_x = cdiv(fd.Wo, f.T); fd.M = f.B * fd.tiles_y * fd.tiles_x;
    }
    return fd;
}

// ---- stages: each reads the plan from the geometry and issues the launch that plan calls for ----

// V = B^T d B (f: the geometry whose INPUT is x)
void wino_input(const WinoGeom& f, const float* x, int ldx, float* V, const float* in_scale, const float* in_shift, int in_relu,
                int up2x, hipStream_t st) {
    const dim3 grid(cdiv(f.M, 4) << f.cq_shift), blk(256);
    if (f.T != 4) hipLaunchKernelGGL(wino_input_kernel, grid, blk, 0, st, x, ldx, V, f, in_scale, in_shift, in_relu, up2x);
    // F(4x4,3x3): the instantiation that holds exactly what the call uses
    else if (up2x) hipLaunchKernelGGL(wino4_input_up2x_kernel, grid, blk, 0, st, x, ldx, V, f, up2x);
    else if (in_scale) hipLaunchKernelGGL(wino4_input_kernel<true>, grid, blk, 0, st, x, ldx, V, f, in_scale, in_shift, in_relu);
    else hipLaunchKernelGGL(wino4_input_kernel<false>, grid, blk, 0, st, x, ldx, V, f, in_scale, in_shift, in_relu);
}

// U = G g G^T of the forward layer f: the forward's set into Uf and / or the data gradient's (taps flipped, roles swapped) into
// Ud, each in the form its GEMM reads (nt_x3).  Both panel sets come from one launch (grid.y = 2).  Of the fp32 sets, the
// swapped one rides along with the forward's from the same nine reads (Uswap); asked for alone -- a backward without saved
// state -- it is transformed from the flipped taps directly.
void wino_weights(const WinoGeom& f, const float* w, float* Uf, float* Ud, hipStream_t st) {
    const bool pf = Uf && nt_x3(f), pd = Ud && nt_x3(dgrad_geom(f));
    float* const ff = pf ? nullptr : Uf;
    float* const fs = pd ? nullptr : Ud;
    const dim3 blk(256);
    if (ff || fs) {
        const dim3 grid(cdiv(f.N * f.C, 256));
        if (Uf) hipLaunchKernelGGL(wino_weights_kernel, grid, blk, 0, st, w, ff, f.N, f.C, f.flip, fs);
        else hipLaunchKernelGGL(wino_weights_kernel, grid, blk, 0, st, w, fs, f.N, f.C, 1 | f.flip, (float*)nullptr);
    }
    if (pf || pd) {
        unsigned char* const U0 = (unsigned char*)(pf ? Uf : Ud);
        unsigned char* const U1 = (unsigned char*)(pf && pd ? Ud : nullptr);
        const int swap0 = pf ? f.flip : 1 | f.flip, swap1 = U1 ? 1 | f.flip : 0;
        const dim3 grid(cdiv(f.N * f.C / 8, 256), U1 ? 2 : 1);
        if (f.T == 4) hipLaunchKernelGGL(wino4_weights_x3_kernel, grid, blk, 0, st, w, U0, f.N, f.C, swap0, U1, swap1);
        else hipLaunchKernelGGL(wino_weights_x3_kernel, grid, blk, 0, st, w, U0, f.N, f.C, swap0, U1, swap1);
    }
}

// Cm[bin] = A[bin] * U[bin]^T (f: M tiles, N outputs, K = C).  nt_cfg: the bf16 x 3 kernel form (gemm_x3.h)
void wino_gemm_nt(const WinoGeom& f, const float* A, const void* U, float* Cm, int nt_cfg, hipStream_t st) {
    if (nt_x3(f)) launch_gemm_x3_nt_cfg(A, U, Cm, f.bins, f.M, f.N, f.C, nt_cfg, 0, st);
    else launch_wino_gemm(A, (const float*)U, Cm, f.M, f.N, f.C, st);
}

// y = A^T m A + epilogue (f: the geometry whose OUTPUT is y)
void wino_output(const WinoGeom& f, const float* Mo, float* y, int ldy, const WinoEp& ep, hipStream_t st) {
    const dim3 grid(cdiv(f.M, 4) << f.nq_shift), blk(256);
#define W4_OUT(A, Bn) hipLaunchKernelGGL((wino4_output_kernel<A, Bn>), grid, blk, 0, st, Mo, y, ldy, ep, f, f.N, f.nq_shift)
    if (f.T != 4) hipLaunchKernelGGL(wino_output_kernel, grid, blk, 0, st, Mo, y, ldy, ep, f, f.N, f.nq_shift);
    else if (ep.addsrc) { if (ep.bnb_y) W4_OUT(true, true); else W4_OUT(true, false); }
    else { if (ep.bnb_y) W4_OUT(false, true); else W4_OUT(false, false); }
#undef W4_OUT
}

// Dv = the weight gradient's transform of dy
void wino_dy(const WinoGeom& f, const float* dy, int ldy, float* Dv, hipStream_t st) {
    const dim3 grid(cdiv(f.M, 4) << f.nq_shift), blk(256);
    if (f.T == 4) hipLaunchKernelGGL(wino4_dy_kernel, grid, blk, 0, st, dy, ldy, Dv, f);
    else hipLaunchKernelGGL(wino_dy_kernel, grid, blk, 0, st, dy, ldy, Dv, f);
}

// P[split][bin] = sum over the split's tiles of Dv[bin]^T V[bin]
void wino_gemm_tn(const WinoGeom& f, const float* Dv, const float* V, float* P, int ns, hipStream_t st) {
    if (tn_x3(f)) launch_gemm_x3_tn(Dv, V, P, f.bins, f.M, f.N, f.C, ns, st);
    else launch_wino_gemm_tn(Dv, V, P, f.M, f.N, f.C, ns, st);
}

// dw = the bins of P folded into the 9 taps, the ns partial sets summed in order
void wino_tap_fold(const WinoGeom& f, const float* P, float* dw, int ns, hipStream_t st) {
    const dim3 grid(cdiv(f.N * f.C, 256)), blk(256);
    if (f.T == 4) hipLaunchKernelGGL(wino4_wgrad_output_kernel, grid, blk, 0, st, P, dw, f.N, f.C, ns, f.flip ? 1 : 0);
    else hipLaunchKernelGGL(wino_wgrad_output_kernel, grid, blk, 0, st, P, dw, f.N, f.C, ns, f.flip ? 1 : 0);
}

// ---- the two chains of the backward.  Each starts with a transform of dy (wino_dy; wino_input on dgrad_geom), which the
// two-stream form runs ahead of both; what follows touches disjoint memory when Dv / Vd and P / Eo are separate regions. ----

// weight gradient, after wino_dy: Dv -> P -> dw   (V: the forward's saved input transform)
void wgrad_chain(const WinoGeom& f, const float* Dv, const float* V, float* P, float* dw, hipStream_t st) {
    const int ns = tn_splits(f);
    wino_gemm_tn(f, Dv, V, P, ns, st);
    wino_tap_fold(f, P, dw, ns, st);
}

// data gradient, after wino_input(fd, dy): Vd -> Eo -> dx (+ addsrc, BatchNorm-backward partials).  A reflection layer writes
// the padded-domain gradient to `padded` and folds it onto dx, with the adjoint of the x2 upsampling when dx_up2x.
void dgrad_chain(const WinoGeom& f, const WinoGeom& fd, const float* Vd, const void* Ud, float* Eo, float* padded, float* dx, int ldx,
                 const float* addsrc, int ld_add, const float* bnb_y, int ld_bnb, const float* bnb_co, int bnb_relu,
                 float* bnb_partial, int dx_up2x, int nt_cfg, hipStream_t st) {
    wino_gemm_nt(fd, Vd, Ud, Eo, nt_cfg, st);
    const WinoEp ep = {f.reflect ? nullptr : addsrc, ld_add, bnb_y ? bnb_partial : nullptr, nullptr, nullptr, 0,
                       bnb_y, ld_bnb, bnb_co, bnb_relu};
    wino_output(fd, Eo, f.reflect ? padded : dx, f.reflect ? f.C : ldx, ep, st);
    if (f.reflect && dx_up2x)
        // dx is the gradient of the LOW-resolution tensor the forward upsampled on load: fold + adjoint interpolation
        hipLaunchKernelGGL(reflect_fold_up2x_kernel, dim3(fold_blocks((int64_t)f.B * (f.H / 2) * (f.W / 2) * (f.C / 4))), dim3(256), 0, st,
                           (const void*)padded, (void*)dx, ldx, (const void*)addsrc, ld_add, f.B, f.H, f.W, f.C, 1, dx_up2x - 1, 0);
    else if (f.reflect)
        launch_wino_reflect_fold(padded, dx, ldx, addsrc, ld_add, f.B, f.H, f.W, f.C, st);
}

// ---- workspace layouts, one per entry point: byte offsets of the regions -- V (forward V / data gradient Vd), Dv, U, Mo (NT GEMM
// output: forward Mo / data gradient Eo), P, the padded-domain gradient of a reflection layer -- and the total ----
struct WinoWs { size_t V, Dv, U, Mo, P, padded, total; };
inline size_t max2(size_t a, size_t b) { return a > b ? a : b; }
inline float* ws_at(const void* base, size_t off) { return (float*)((char*)base + off); }

inline WinoWs fwd_ws(const WinoGeom& f) {                  // V, U, Mo
    WinoWs L = {};
    L.U = v_bytes(f); L.Mo = L.U + u_bytes(f); L.total = L.Mo + m_bytes(f);
    return L;
}
// single stream: Vd / Dv share, U', Eo / P share; a reflection layer's data gradient runs over the padded domain (more tiles)
// and writes the padded gradient directly behind Eo's [bins][Md][C]
inline WinoWs bwd_ws(const WinoGeom& f) {
    const WinoGeom fd = dgrad_geom(f);
    WinoWs L = {};
    L.U = max2(v_bytes(fd), m_bytes(f)); L.Mo = L.P = L.U + u_bytes(f); L.padded = L.Mo + (size_t)f.bins * fd.M * f.C * 4;
    L.total = L.Mo + max2(m_bytes(fd), p_bytes(f)) + (f.reflect ? al256((size_t)f.B * (f.H + 2) * (f.W + 2) * f.C * 4) : 0);
    return L;
}
// two chains: Vd, Dv, P, Eo -- four SEPARATE regions, so that the weight-gradient chain (Dv -> P -> dw) and the data-gradient
// chain (Vd -> Eo -> dx) touch disjoint memory once both transforms of dy have run
inline WinoWs pair_ws(const WinoGeom& f) {
    WinoWs L = {};
    L.Dv = m_bytes(f); L.P = L.Dv + m_bytes(f); L.Mo = L.P + p_bytes(f); L.total = L.Mo + v_bytes(f);
    return L;
}
// the layers the two-chain form is for: F(4x4,3x3) plans (zero padding, every GEMM bf16 x 3)
inline bool pair_geom(const gdn_conv_geom* g, WinoGeom& f) { return wino_geom(g, f) && f.T == 4; }

}  // namespace

// saved state of one forward for its backward: the transformed input V, then the data gradient's transformed weights
extern "C" size_t gdn_winoconv_state_bytes(const gdn_conv_geom* g) {
    WinoGeom f;
    return wino_geom(g, f) ? v_bytes(f) + u_bytes(f) : 0;
}

extern "C" size_t gdn_winoconv_fwd_workspace_bytes(const gdn_conv_geom* g) {
    WinoGeom f;
    return wino_geom(g, f) ? fwd_ws(f).total : 0;
}

extern "C" int64_t gdn_winoconv_stats_slots(const gdn_conv_geom* g) {
    WinoGeom f;
    if (!wino_geom(g, f)) return GDN_ERR_UNSUPPORTED;
    return cdiv(f.M, 4);
}

extern "C" int gdn_winoconv_fwd(const gdn_conv_geom* g, const float* x, int32_t ldx, const float* w, float* y, int32_t ldy,
                                const float* addsrc, int32_t ld_add, float* stats, const float* ep_scale,
                                const float* ep_shift, int32_t act, const float* in_scale, const float* in_shift,
                                int32_t in_relu, int32_t in_up2x, void* state_out, void* workspace,
                                size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other HIP users of this thread
    WinoGeom f;
    if (!wino_geom(g, f)) return GDN_ERR_UNSUPPORTED;
    if (!x || !w || !y || (!ep_scale) != (!ep_shift) || (!in_scale) != (!in_shift)) return GDN_ERR_BAD_ARG;
    if (in_up2x < 0 || in_up2x > 2 || (in_up2x && (in_scale || (g->H & 1) || (g->W & 1)))) return GDN_ERR_BAD_ARG;
    const WinoWs L = fwd_ws(f);
    if (!workspace || workspace_bytes < L.total) return GDN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    // a forward that will run backward writes V into the state and, behind it, the data gradient's weight set: the weights
    // do not change between a step's forward and backward
    float* V = state_out ? (float*)state_out : ws_at(workspace, L.V);
    float* Usw = state_out ? ws_at(state_out, v_bytes(f)) : nullptr;
    float* U = ws_at(workspace, L.U);
    float* Mo = ws_at(workspace, L.Mo);
    wino_input(f, x, ldx, V, in_scale, in_shift, in_relu, in_up2x, st);
    wino_weights(f, w, U, Usw, st);
    wino_gemm_nt(f, V, U, Mo, X3_NT_AUTO, st);
    wino_output(f, Mo, y, ldy, WinoEp{addsrc, ld_add, stats, ep_scale, ep_shift, act, nullptr, 0, nullptr, 0}, st);
    return gdn_launch_status();
}

extern "C" size_t gdn_winoconv_bwd_workspace_bytes(const gdn_conv_geom* g) {
    WinoGeom f;
    return wino_geom(g, f) ? bwd_ws(f).total : 0;
}

// slots of the BatchNorm-backward partials the data-gradient epilogue can emit (0: not available for this layer)
extern "C" int64_t gdn_winoconv_bnb_slots(const gdn_conv_geom* g) {
    WinoGeom f;
    if (!wino_geom(g, f) || f.reflect) return 0;
    return cdiv(f.M, 4);
}

extern "C" int gdn_winoconv_bwd(const gdn_conv_geom* g, const float* dy, int32_t ldy, const float* w, const void* state,
                                float* dx, int32_t ldx, const float* addsrc, int32_t ld_add, float* dw,
                                const float* bnb_y, int32_t ld_bnb, const float* bnb_co, int32_t bnb_relu,
                                float* bnb_partial, int32_t dx_up2x, void* workspace, size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();
    WinoGeom f;
    if (!wino_geom(g, f)) return GDN_ERR_UNSUPPORTED;
    if (!dy || (!dx && !dw) || (dx && !w && !state) || (dw && !state)) return GDN_ERR_BAD_ARG;
    if (bnb_y && (!dx || !bnb_co || !bnb_partial)) return GDN_ERR_BAD_ARG;
    if (bnb_y && f.reflect) return GDN_ERR_UNSUPPORTED;
    if (dx && f.reflect && ((ldx % 4) || (addsrc && (ld_add % 4)))) return GDN_ERR_UNSUPPORTED;
    if (dx_up2x < 0 || dx_up2x > 2 || (dx_up2x && ((g->H & 1) || (g->W & 1)))) return GDN_ERR_BAD_ARG;
    if (dx && dx_up2x && !f.reflect) return GDN_ERR_UNSUPPORTED;   // (the fold pass of a reflection layer carries the adjoint)
    const WinoWs L = bwd_ws(f);
    if (!workspace || workspace_bytes < L.total) return GDN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (dw) {
        wino_dy(f, dy, ldy, ws_at(workspace, L.Dv), st);
        wgrad_chain(f, ws_at(workspace, L.Dv), (const float*)state, ws_at(workspace, L.P), dw, st);
    }
    if (dx) {
        const WinoGeom fd = dgrad_geom(f);
        wino_input(fd, dy, ldy, ws_at(workspace, L.V), nullptr, nullptr, 0, 0, st);
        if (!state) wino_weights(f, w, nullptr, ws_at(workspace, L.U), st);
        const float* Ud = state ? ws_at(state, v_bytes(f)) : ws_at(workspace, L.U);      // state: transformed by the forward's launch
        dgrad_chain(f, fd, ws_at(workspace, L.V), Ud, ws_at(workspace, L.Mo), ws_at(workspace, L.padded), dx, ldx, addsrc, ld_add,
                    bnb_y, ld_bnb, bnb_co, bnb_relu, bnb_partial, dx_up2x, X3_NT_AUTO, st);
    }
    return gdn_launch_status();
}

// ---- F(4x4,3x3) backward with both gradients, in phases a caller can put on two streams ----
extern "C" size_t gdn_winoconv_bwd_pair_workspace_bytes(const gdn_conv_geom* g) {
    WinoGeom f;
    return pair_geom(g, f) ? pair_ws(f).total : 0;
}

extern "C" int gdn_winoconv_bwd_pair(const gdn_conv_geom* g, const float* dy, int32_t ldy, const float* w, const void* state,
                                     float* dx, int32_t ldx, const float* addsrc, int32_t ld_add, float* dw,
                                     const float* bnb_y, int32_t ld_bnb, const float* bnb_co, int32_t bnb_relu,
                                     float* bnb_partial, int32_t dx_up2x, int32_t phases, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    (void)hipGetLastError();
    (void)w;                                   // (the data gradient's weight set comes with the forward's state)
    WinoGeom f;
    if (!pair_geom(g, f)) return GDN_ERR_UNSUPPORTED;
    if (!dy || !dx || !dw || !state) return GDN_ERR_BAD_ARG;
    if (bnb_y && (!bnb_co || !bnb_partial)) return GDN_ERR_BAD_ARG;
    if (dx_up2x < 0 || dx_up2x > 2) return GDN_ERR_BAD_ARG;
    if (dx_up2x) return GDN_ERR_UNSUPPORTED;   // (as gdn_winoconv_bwd: only the fold pass of a reflection layer carries the adjoint)
    if (phases < 0 || phases > 7) return GDN_ERR_BAD_ARG;
    const WinoWs L = pair_ws(f);
    if (!workspace || workspace_bytes < L.total) return GDN_ERR_WORKSPACE;
    if (!phases) phases = 7;
    hipStream_t st = (hipStream_t)stream;
    const WinoGeom fd = dgrad_geom(f);
    if (phases & 1) {
        wino_input(fd, dy, ldy, ws_at(workspace, L.V), nullptr, nullptr, 0, 0, st);
        wino_dy(f, dy, ldy, ws_at(workspace, L.Dv), st);
    }
    if (phases & 2) wgrad_chain(f, ws_at(workspace, L.Dv), (const float*)state, ws_at(workspace, L.P), dw, st);
    if (phases & 4)
        // phase 4 without phase 2 is the forked form: the weight-gradient chain runs beside this GEMM on another stream
        dgrad_chain(f, fd, ws_at(workspace, L.V), ws_at(state, v_bytes(f)), ws_at(workspace, L.Mo), nullptr, dx, ldx, addsrc, ld_add,
                    bnb_y, ld_bnb, bnb_co, bnb_relu, bnb_partial, 0, X3_NT_AUTO | ((phases & 2) ? 0 : X3_NT_SHARED), st);
    return gdn_launch_status();
}

// Measurement hook (bench.py roofline, tools/): the 16 per-bin GEMMs of one forward alone, on already transformed operands
// V [16][M][Cin] and U [16][Cout][Cin]  ->  Mo [16][M][Cout].
extern "C" int gdn_winoconv_gemm(const gdn_conv_geom* g, const float* V, const float* U, float* Mo, void* stream) {
    (void)hipGetLastError();
    WinoGeom f;
    if (!wino_geom(g, f)) return GDN_ERR_UNSUPPORTED;
    if (!V || !U || !Mo) return GDN_ERR_BAD_ARG;
    launch_wino_gemm(V, U, Mo, f.B * cdiv(f.H, 2) * cdiv(f.W, 2), f.N, f.C, (hipStream_t)stream);      // (F(2x2,3x3) tiles whatever the layer's plan)
    return gdn_launch_status();
}

