// The kernels of csrc/densify.hip compiled as serial HOST code: one thread per workgroup (DZ_T = E_T = 1), so every stage
// loop of a kernel runs to its end before the next begins and the barriers are no-ops.  A stand-alone program for a CPU
// build with -fsanitize=address,undefined and -ffp-contract=off: the LDS images become static arrays and the pools heap
// blocks, so an index outside either is reported, and the arithmetic is the kernels' own.  tests/test_densify_cpu.py builds
// it, feeds it pools and compares what it writes with the numpy restatement bit for bit.
//
//   densify_host IN OUT
//   IN:  int32 B, Hmax, Wmax; float32 max_depth; int32 sizes[B][2]; float32 pool[B][Hmax][Wmax]
//   OUT: float32 dense[B][Hmax][Wmax]; uint8 code[n - 1] without and uint8 code[n - 1] with keep_valid, of the first n - 1
//        cells of `dense` at scale 80 (n - 1 so that the encoder's tail lanes run)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
using std::max;
using std::min;

#define GDN_DENSIFY_HOST
#define DZ_T 1
#define E_T 1
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
struct dim3_ { unsigned x, y, z; };
static dim3_ threadIdx, blockIdx, blockDim, gridDim;
static void __syncthreads() {}
static int __syncthreads_or(int v) { return v; }
struct float4 { float x, y, z, w; };
#include "../../gdn-pytorch_amd/csrc/densify.hip"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    float md;
    if (fread(hdr, 4, 3, f) != 3 || fread(&md, 4, 1, f) != 1) return 2;
    const int B = hdr[0], Hm = hdr[1], Wm = hdr[2];
    const size_t n = (size_t)B * Hm * Wm;
    std::vector<int32_t> sizes(2 * B);
    std::vector<float> in(n), out(n), work(n);
    if (fread(sizes.data(), 4, 2 * B, f) != (size_t)2 * B || fread(in.data(), 4, n, f) != n) return 2;
    fclose(f);
    memset(out.data(), 0x7f, n * 4);              // NaN bits: a cell read before it is written shows
    memset(work.data(), 0x7f, n * 4);
    const int ntx = (Wm + DZ_TW - 1) / DZ_TW, nty = (Hm + DZ_TH - 1) / DZ_TH;
    threadIdx = {0, 0, 0};
    blockDim = {1, 1, 1};
    for (int launch = 0; launch < 4; ++launch)
        for (unsigned b = 0; b < (unsigned)B; ++b)
            for (unsigned t = 0; t < (launch == 1 ? (unsigned)Wm : (unsigned)(ntx * nty)); ++t) {
                blockIdx = {t, b, 0};
                if (launch == 0) densify_fill_kernel(in.data(), sizes.data(), Hm, Wm, ntx, md, out.data());
                if (launch == 1) densify_extend_kernel(out.data(), sizes.data(), Hm, Wm);
                if (launch == 2) densify_holes_kernel(out.data(), sizes.data(), Hm, Wm, ntx, work.data());
                if (launch == 3) densify_smooth_kernel(work.data(), sizes.data(), Hm, Wm, ntx, md, out.data());
            }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.data(), 4, n, f);
    gridDim = {1, 1, 1};
    blockIdx = {0, 0, 0};
    for (int keep = 0; keep < 2; ++keep) {
        std::vector<uint8_t> code((n - 1 + 3) / 4 * 4, 0xAA);
        for (unsigned t = 0; t < 4; ++t) {        // lane 0 walks every quad; lanes 0 .. 2 the tail
            threadIdx = {t, 0, 0};
            depth_encode_u8_kernel(out.data(), (int64_t)n - 1, 80.0, keep, code.data());
        }
        fwrite(code.data(), 1, n - 1, f);
    }
    fclose(f);
    return 0;
}
