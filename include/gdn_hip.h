/*
 * gdn_hip.h -- C ABI of libgdn_hip.so, the MI355X (gfx950) kernels behind the
 * GDN-Pytorch hot path.
 *
 * The reference (tjqansthd/GDN-Pytorch) has no FFI: its boundary is Python
 * (nn.Module.forward + loss helpers) and every device op is a PyTorch/cuDNN
 * call.  Each entry point below therefore replaces one *PyTorch call site* of
 * the reference; the file:line cited is that call site (paths relative to
 * /root/reference/src).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions (all entry points):
 *   - return 0 on success, negative gdn_status on error (gdn_strerror());
 *   - never allocate, never synchronise, never read device memory on the host:
 *     every call is stream-ordered on `stream` (a hipStream_t passed as void*)
 *     and is hipGraph-capture safe; the caller owns every buffer, including
 *     workspaces sized by the matching *_workspace_bytes() query;
 *   - activations are fp32 NHWC: pixel p of an image batch [B,H,W] with C
 *     channels lives at base + p*ld (ld >= C floats, lets a tensor be a channel
 *     slice of a wider one); weights are fp32 in "tap-major" layout
 *     [kh*kw][Cout][Cin] (Cin contiguous) for both Conv2d and ConvTranspose2d;
 *   - stateless and thread-safe: the library owns no stream, event, buffer or cache.
 *     Work that profits from a second stream (gdn_fftconv_bwd's two chains) is split
 *     into phases the CALLER places on streams of its own.
 */
#ifndef GDN_HIP_H
#define GDN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    GDN_OK = 0,
    GDN_ERR_BAD_ARG = -1,
    GDN_ERR_UNSUPPORTED = -2,
    GDN_ERR_WORKSPACE = -3,
    GDN_ERR_LAUNCH = -4
} gdn_status;

/* Revision of this header (argument lists, struct layouts).  223: gdn_depth_metrics_nyu*, gdn_depth_metrics_make3d*, gdn_crop_normalize, gdn_bytescale_u8 (evaluation); added later without a bump (purely additive: a library without them fails at load on the missing symbol): gdn_nyu_aug_params, gdn_nyu_augment*, gdn_pil_resize*, gdn_spline_rotate3* (NYU training); gdn_grad_sumsq*, gdn_grad_guard_finalize, gdn_adam_step_dev_guarded (gradient guard of the capturable Adam); gdn_hints_supported with GDN_HINT_FLIP_TAPS (a library that would ignore the bit lacks the symbol); gdn_bn_frozen_coeffs, gdn_bn_frozen_bwd* (--freeze_bn); gdn_silog_masked (--loss silog; gdn_loss_workspace_bytes grows by a third partial array, which every caller queries); gdn_depth_metrics_std*, gdn_flip_w, gdn_flip_mean (--eval_protocol standard, --flip_test); gdn_velo_project (--eval_velodyne).  222: gdn_fftconv_bwd bnb_*, gdn_fftconv_bnb_slots.  221: gdn_clock_probe_*.  220: gdn_conv_dgrad dx_up2x; gdn_bn_apply_up2x; bf16 tile id 12 (conv_ring2_bf16).  219: gdn_conv_wgrad_bf16 cfg 4 (wgrad_ring_bf16); gdn_fftconv_cgemm* measurement hooks; plan overrides in gdn_conv_geom.hints; gdn_gemm_x3_nt_packed / gdn_gemm_x3_ring_workspace_bytes removed (the measured-and-not-wired kernel now lives under tests/diag/).  218: gdn_gemm_x3_tn_splits.  217: gdn_conv_dgrad bnb_*.  216: gdn_conv_c1_fwd Cin.  215: GDN_HINT_NO_WINO_F4.  214: gdn_gemm_x3_nt_packed.  213: gdn_conv_c1_fwd dtypes / gdn_conv_c1_wgrad gw_bf16.  212: GDN_HINT_NO_X3 (replaces the GDN_X3 environment read).  211: gdn_gemm_x3_*.  210: gdn_conv_geom.hints, in_up2x / dx_up2x.  A binding checks it
 * for equality at load time (gdn_amd/_lib.py: ABI_VERSION). */
int gdn_version(void);
/* The GDN_HINT_* bits (below) this library acts on.  A binding that sets a bit that CHANGES WHAT IS COMPUTED (GDN_HINT_FLIP_TAPS)
 * checks it here first: a library that predates the bit would silently ignore it. */
int gdn_hints_supported(void);
const char* gdn_strerror(int status);
/* Fills name[] with the HIP device name of the current device; returns CU count (<0 on error). */
int gdn_device_info(char* name, int name_len);

/* ------------------------------------------------------------------------
 * Convolution geometry, in torch.nn semantics.
 *   transposed == 0 : nn.Conv2d(Cin, Cout, k, stride, pad), optionally preceded
 *                     by nn.ReflectionPad2d(pad) (pad_mode 1, conv pad 0) --
 *                     ConvBlock AE_model_unet.py:65-69, ResidualBlock :49-54.
 *   transposed == 1 : nn.ConvTranspose2d(Cin, Cout, k, stride, pad) --
 *                     ConvTBlock AE_model_unet.py:84-87, upconv4 :521.
 * H, W are the spatial dims of the layer INPUT.
 * ---------------------------------------------------------------------- */
typedef struct {
    int32_t B, H, W;
    int32_t Cin, Cout;
    int32_t k, stride, pad;
    int32_t pad_mode;   /* 0 zero padding, 1 reflection padding (Conv2d only) */
    int32_t transposed; /* 0 Conv2d, 1 ConvTranspose2d */
    int32_t hints;      /* GDN_HINT_* bits; 0 = none.  A hint never changes results beyond rounding, only which internal
                         * plan a transform-domain path picks; every call of one layer instance (workspace / state queries,
                         * forward, backward) must carry the same hints. */
} gdn_conv_geom;

/* GDN_HINT_TRAIN: the layer runs forward AND backward with a weight gradient (a trained layer in train mode).  The
 * frequency-domain path then tiles for the sum of both passes: 40-point tiles (32 valid outputs of a 9x9 window: 128 x 416
 * is exactly 4 x 13 of them, 26 % fewer transformed points) shorten the three per-bin GEMM chains of a training step by a
 * quarter but make the forward's single-pass transforms slower, so inference / frozen layers keep the 32-point tiles. */
enum { GDN_HINT_TRAIN = 1, GDN_HINT_NO_X3 = 2, GDN_HINT_NO_WINO_F4 = 4, GDN_HINT_FFT_NP32 = 8, GDN_HINT_FFT_NP40 = 16,
       GDN_HINT_FLIP_TAPS = 32 };
/* GDN_HINT_FLIP_TAPS (transposed == 0, zero padding, stride 1, odd k, pad == k / 2; gdn_fftconv_* and gdn_winoconv_* only):
 * the layer is a stride-1 nn.ConvTranspose2d(Cin, Cout, k, 1, k / 2) written as the convolution it is -- the correlation with
 * the stored taps in reverse order.  `w` is that module's tap-major buffer [k*k][Cout][Cin] as stored, and `dw` receives the
 * gradient of the STORED taps (the weight-gradient output pass writes tap t to slot k*k - 1 - t), so the caller hands in
 * the module's own weight and gradient slices.  Unlike the other hints this one changes what is computed, not how: it is
 * part of the layer's definition.  The direct entry points (gdn_conv_fwd / _dgrad / _wgrad / _wgrad_bf16) refuse it with
 * GDN_ERR_UNSUPPORTED rather than compute the un-flipped layer; they take the same layer as a transposed == 1 geometry, for which the transform-domain paths remain forward-only (fft) or refuse (wino). */
/* Plan overrides (tests, measurements; 0 = none), fields of `hints`: the library itself reads no environment variable.
 *   GDN_HINT_PLAN_BATCH(n), bits 8..15: every plan that depends on the batch size is made as if the batch were n (1..255), so
 *                           a batch-1 call takes the plans of a batch-n call and an image compares bitwise across batch sizes;
 *   GDN_HINT_PLAN_CUS(n),   bits 16..23: the persistent kernels (conv_ring_bf16, wgrad_ring_bf16) are planned as for a chip
 *                           with n CUs (a multiple of 8, <= 2040): small test shapes reach the multi-round / split paths;
 *   GDN_HINT_FFT_NP32 / _NP40: gdn_fftconv_* plans 32- / 40-point tiles where it would choose the other. */
#define GDN_HINT_PLAN_BATCH(n) (((n) & 0xff) << 8)
#define GDN_HINT_PLAN_CUS(n) ((((n) / 8) & 0xff) << 16)
/* GDN_HINT_NO_X3: the Winograd paths (gdn_winoconv_*, gdn_wino2conv_*) run their per-bin GEMMs on the fp32 matrix
 * instruction instead of as bf16 x 3 split products (gdn_gemm_x3_*).  Same results to rounding.  The library reads no
 * environment variable for this: the caller decides once (gdn_amd/ops.py: set_x3; ranks that share one GPU switch it off,
 * DESIGN.md 2.10) and the form of a forward's saved weight set follows the geometry its backward is called with.
 * GDN_HINT_NO_WINO_F4: gdn_winoconv_* plans F(2x2,3x3) where it would plan F(4x4,3x3) (zero-padded 3x3 layers whose GEMMs are
 * bf16 x 3 eligible); results differ by rounding only, the layout of the saved state follows the plan. */

enum { GDN_ACT_NONE = 0, GDN_ACT_TANH = 1, GDN_ACT_RELU = 2 };   /* bit flags */

/* tile_cfg flag bits shared by the conv entry points (low byte: tile id, 0 = automatic).
 * GDN_CFG_BF16: x/x2/w/y/addsrc (dy/wt/dx for dgrad) hold bfloat16 instead of float
 * (BASELINE configs[2]); accumulation, BatchNorm statistics and split-K partials stay fp32.
 * Needs Cin, C1 (dgrad: Cout) multiples of 64 and pixel pitches multiples of 8.
 * Exception: the 1-channel 9x9 heads (Cout == 1) take a bf16 x but fp32 weights and write an
 * fp32 depth map; their backward runs through the fp32 entry points.
 * The workspace/slot queries must be given the same tile_cfg as the launch.
 * bf16 tile ids (tests, A/B measurements): 1-3 tap-major tiles, 8/9 the round-1 row-patch kernel, 10/11 conv_ring_bf16 (256 x 64 /
 * 256 x 128: the LDS-DMA ring kernel of the stride-1 layers with a 3/5/7/9 window, the automatic choice for them; its persistent
 * workgroups may cut the last round of tiles into stage ranges, whose fp32 slabs live in `workspace`: the forward and the
 * data-gradient workspace queries include them; bit 0x800, "single stage", keeps every unit whole, as it keeps the other
 * kernels from splitting over the filter taps), 12 conv_ring2_bf16 (the same kernel on 512 x 64 tiles and 32-channel slabs:
 * the automatic choice for 64-output-channel layers with a 7 / 9 window that fill the chip twice).  For ids 10..12 bits 12..15
 * are measurement knobs of that kernel (timing-only variants that drop an operand's LDS-DMA traffic or skip the tap loop; 0 in
 * production). */
enum { GDN_CFG_KC64 = 0x200, GDN_CFG_NO_SPLITK = 0x800, GDN_CFG_BF16 = 0x10000 };

/* Output spatial dims of the layer. */
int gdn_conv_out_dims(const gdn_conv_geom* g, int32_t* Ho, int32_t* Wo);

/* Number of per-block partial-statistics slots gdn_conv_fwd writes when
 * `stats` is non-NULL, for the same tile_cfg; the stats buffer must hold
 * slots*2*Cout floats laid out [slot][2][Cout]. */
int64_t gdn_conv_stats_slots(const gdn_conv_geom* g, int32_t tile_cfg);

/* Forward convolution.  Replaces nn.Conv2d / nn.ConvTranspose2d forward
 * (AE_model_unet.py:50,53,67,85,300,521) and, through x2, the
 * torch.cat(...)+1x1 ConvBlock pair (:338-339,:345-346,:351-352,:357-358)
 * without materialising the concat: reduction channels [0,C1) come from x,
 * [C1,Cin) from x2 (x2 may be NULL when C1 == Cin).
 *   y[pixel][c] = tanh?( relu?( conv(x)[c] * ep_scale[c] + ep_shift[c] ) + addsrc[pixel][c] )
 *                 ep_scale/ep_shift (both or neither; NULL = identity) fold an eval-mode BatchNorm
 *                 (gdn_bn_eval_coeffs) into the epilogue: conv + BN + ReLU (+ residual) in one pass --
 *                 the frozen guide network and the inference path (depth_extract.py); act is a bit mask
 *                 of GDN_ACT_RELU (before the add) and GDN_ACT_TANH (after it)
 *   stats[slot][0][c], [1][c] = per-block sum / sum of squares of the raw conv
 *                               output (feeds train-mode BatchNorm, K7).
 * Launches that cannot fill the chip are split over the filter taps (split-K);
 * their partial sums live in `workspace` (gdn_conv_fwd_workspace_bytes, 0 when
 * no split is planned) and are combined -- with the same fusions -- by a second
 * kernel inside the call.
 * tile_cfg: 0 = automatic; low byte >0 forces a tile configuration (tuning/testing);
 * flag bits above.  x, x2, w, y, addsrc: float (default) or bfloat16 (GDN_CFG_BF16). */
size_t gdn_conv_fwd_workspace_bytes(const gdn_conv_geom* g, int32_t tile_cfg);
int gdn_conv_fwd(const gdn_conv_geom* g,
                 const void* x, int32_t ldx, const void* x2, int32_t ldx2, int32_t C1,
                 const void* w, void* y, int32_t ldy,
                 const void* addsrc, int32_t ld_add,
                 float* stats, const float* ep_scale, const float* ep_shift, int32_t act, int32_t tile_cfg,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Data gradient.  Replaces autograd's conv backward-data for the call sites
 * above (loss.backward(), trainer.py:467,767).  wt is the tap-major TRANSPOSED
 * weight [kh*kw][Cin][Cout] (see gdn_transpose_taps).  dx = dgrad(dy) (+ addsrc).
 * Reflection-padded layers need a workspace for the gradient on the padded
 * domain, folded back onto dx inside the call. */
size_t gdn_conv_dgrad_workspace_bytes(const gdn_conv_geom* g, int32_t tile_cfg);
/* bnb_y != NULL: dx (+ addsrc) is the FINAL gradient of z = [relu](BN_train(bnb_y)) -- the layer's input is the output of a
 * train-mode BatchNorm (+ReLU) and this call comes from its first consumer -- and bnb_partial [slots][2][Cin] receives that
 * BatchNorm's backward partial sums (sum dz, sum dz * xhat per slot; bnb_co = [scale, shift, mean, invstd][Cin]) computed from
 * the values as they are stored, so gdn_bn_bwd can skip its reduce pass.  slots = gdn_conv_dgrad_bnb_slots(g, tile_cfg);
 * 0 = not available for this layer (today: the bf16 stride-1 layers of the LDS-DMA ring kernel, zero padding).
 * dx_up2x (0 none, 1 align_corners False, 2 True): the layer's input was F.interpolate(t, scale_factor=2, mode='bilinear') and
 * nothing else reads the upsampled tensor (AE_model_unet.py:336-359: every upconvN); dx and addsrc are then dL/dt,
 * [B, H/2, W/2, Cin] -- the fold pass of a reflection-padded layer applies the adjoint of the interpolation while it folds, so
 * the full-resolution gradient is neither written nor read back.  Reflection-padded layers with Cin % 4 == 0 and even H, W
 * only (GDN_ERR_UNSUPPORTED otherwise); fp32 and bf16. */
int64_t gdn_conv_dgrad_bnb_slots(const gdn_conv_geom* g, int32_t tile_cfg);
int gdn_conv_dgrad(const gdn_conv_geom* g, const void* dy, int32_t ldy,
                   const void* wt, void* dx, int32_t ldx,
                   const void* addsrc, int32_t ld_add,
                   const void* bnb_y, int32_t ld_bnb, const float* bnb_co, int32_t bnb_relu, float* bnb_partial,
                   int32_t dx_up2x, void* workspace, size_t workspace_bytes, int32_t tile_cfg, void* stream);

/* Weight gradient (same call sites).  x is the layer input ([B,H,W], channel
 * slice [0,Cx) of width ldx), dy the output gradient.  Writes
 * dw[tap][co][ci_off + ci] for ci in [0,Cx), with row stride ld_dw (= total
 * Cin), so the two halves of a concat 1x1 conv are two calls.  Deterministic:
 * split-K partial slabs in `workspace` are summed in a fixed order.
 * dtypes (bit0 x, bit1 dy): 0 = fp32.  On the mixed-precision path the layers with a 1-3 channel
 * tensor (image-input conv, 64->1 heads) keep that tensor in fp32 and may pass the wide one as bf16. */
size_t gdn_conv_wgrad_workspace_bytes(const gdn_conv_geom* g, int32_t Cx);
int gdn_conv_wgrad(const gdn_conv_geom* g, const void* x, int32_t ldx, int32_t Cx,
                   const void* dy, int32_t ldy,
                   float* dw, int32_t ld_dw, int32_t ci_off,
                   void* workspace, size_t workspace_bytes, int32_t dtypes, void* stream);

/* FFT-domain convolution for the large-window stride-1 layers (AE_model_unet.py ResidualBlock: 9x9 on
 * 64 channels, 7x7 on 128, 5x5 on 256; ConvBlock with ReflectionPad2d in R's decoder; the legacy
 * network's stride-1 ConvTranspose2d): stride 1, pad k/2 (zeros or reflection), odd k in 3..9, Cin and
 * Cout multiples of 64 up to 256, fp32.  Overlap-save on 32x32 tiles: real FFT of the input patches,
 * one complex (real-embedded, MFMA) GEMM per frequency bin, inverse FFT of the valid outputs.
 * Same contract as gdn_conv_fwd for y / addsrc / stats / ep_scale / ep_shift / act (slots:
 * gdn_fftconv_stats_slots).
 * in_scale / in_shift (nullable pair, Cin floats) + in_relu: x is the RAW output of the producer
 * convolution and the layer input is [relu](x*in_scale[c] + in_shift[c]) -- the producer's train-mode
 * BatchNorm (+ReLU) applied while the patch is loaded, so `a = relu(bn1(conv1 x))` of a ResidualBlock
 * (AE_model_unet.py:49-54) is never written to memory.  Padding stays zero.
 * in_up2x (0 = off, 1 = align_corners False, 2 = True; not together with in_scale): x is the LOW-resolution
 * tensor [B][H/2][W/2][Cin] and the layer input is its x2 bilinear upsampling (F.interpolate(scale_factor=2,
 * mode='bilinear') + ConvBlock, AE_model_unet.py:336-359; the legacy decoder :214-230), interpolated from the four
 * neighbours of every element while the patch is loaded -- border rule (zeros / reflection) first, on the upsampled
 * coordinates -- so the upsampled tensor is never written to memory.  g->H, g->W stay the convolution's (upsampled, even)
 * input extent.
 * xf_out (nullable, gdn_fftconv_spectrum_bytes) receives the input and weight spectra, which
 * gdn_fftconv_bwd reuses (weight gradient; data gradient without a second weight transform).
 * GDN_ERR_UNSUPPORTED for other geometries; transposed (stride-1) layers are forward-only
 * (gdn_fftconv_bwd_workspace_bytes == 0). */
size_t gdn_fftconv_fwd_workspace_bytes(const gdn_conv_geom* g);
size_t gdn_fftconv_spectrum_bytes(const gdn_conv_geom* g);
int64_t gdn_fftconv_stats_slots(const gdn_conv_geom* g);
int gdn_fftconv_fwd(const gdn_conv_geom* g, const float* x, int32_t ldx, const float* w,
                    float* y, int32_t ldy, const float* addsrc, int32_t ld_add, float* stats,
                    const float* ep_scale, const float* ep_shift, int32_t act,
                    const float* in_scale, const float* in_shift, int32_t in_relu, int32_t in_up2x,
                    void* xf_out, void* workspace, size_t workspace_bytes, void* stream);
/* Backward of the same layer from one transform of dy: dx = dgrad (+ addsrc) when dx != NULL,
 * dw[tap][Cout][Cin] = wgrad when dw != NULL (needs xf, the state saved by the forward; with
 * xf == NULL the data gradient transforms w itself).
 * phases: 0 / GDN_FFT_BWD_ALL = everything on `stream`.  The weight-gradient chain and the
 * data-gradient chain only share the spectrum of dy and use disjoint parts of the workspace, so a
 * caller may issue GDN_FFT_BWD_TRANSFORM on stream A, let stream B wait for it, issue GDN_FFT_BWD_DW
 * on B and GDN_FFT_BWD_DX on A (same arguments, same workspace) and join B into A: the two
 * latency-bound chains then overlap.  The library creates no stream or event itself.
 * dyb_* (nullable; replaces pass 3 of gdn_bn_bwd for THIS layer's own BatchNorm): `dy` is dout, the
 * gradient of z = [relu](BN_train(dyb_y)) with dyb_y this layer's raw conv output, dyb_co = {scale, shift,
 * mean, invstd}[Cout] and dyb_kk = {k1, k2}[Cout] from gdn_bn_bwd_coeffs; the dy transform computes
 * dy = scale*(dz - k1 - xhat*k2) while loading, so dy itself is never written to memory.
 * bnb_* (nullable; zero-padded layers, gdn_fftconv_bnb_slots(g) > 0 slots): dx is the final gradient of this layer's INPUT
 * z = [relu](BN_train(bnb_y)) (bnb_y: the producer's raw conv output [B][H][W][Cin], pitch ld_bnb; bnb_co = {scale, shift,
 * mean, invstd}[Cin]); the pass that writes dx also writes that BatchNorm's backward partial sums (sum dz, sum dz * xhat) to
 * bnb_partial[slots][2][Cin] -- gdn_bn_bwd / gdn_bn_bwd_coeffs take them as ext_partial, and the stand-alone reduce pass
 * over (dx, y) disappears (AE_model_unet.py:51,54 as consumed by the next conv of :50,53).
 * dx_up2x (as in_up2x of the forward; reflection-padded layers only, else GDN_ERR_UNSUPPORTED): dx, addsrc are
 * [B][H/2][W/2][Cin], the gradient of the LOW-resolution tensor the forward upsampled on load -- the pass that folds the
 * padded-domain gradient back onto the image also applies the adjoint of the interpolation (gather form, deterministic). */
enum { GDN_FFT_BWD_TRANSFORM = 1, GDN_FFT_BWD_DW = 2, GDN_FFT_BWD_DX = 4, GDN_FFT_BWD_ALL = 7 };
size_t gdn_fftconv_bwd_workspace_bytes(const gdn_conv_geom* g);
int gdn_fftconv_bwd(const gdn_conv_geom* g, const float* dy, int32_t ldy, const float* w,
                    const void* xf, float* dx, int32_t ldx, const float* addsrc, int32_t ld_add,
                    float* dw, const float* dyb_y, int32_t ld_dyb, const float* dyb_co,
                    const float* dyb_kk, int32_t dyb_relu,
                    const float* bnb_y, int32_t ld_bnb, const float* bnb_co, int32_t bnb_relu, float* bnb_partial,
                    int32_t dx_up2x, int32_t phases,
                    void* workspace, size_t workspace_bytes, void* stream);
int64_t gdn_fftconv_bnb_slots(const gdn_conv_geom* g);
/* Measurement hooks (bench.py roofline_cgemm): launch ONLY the per-bin complex GEMMs of the frequency-domain layer `g` on
 * whatever the workspace holds -- which: 0 forward (Y = X W), 1 data gradient, 2 the weight gradient's reduction over the
 * tiles; 1 and 2 use disjoint outputs and may run on two streams like gdn_fftconv_bwd's chains.  gdn_fftconv_cgemm_shape:
 * host query of {frequency bins, tiles M, transform points}: per bin the GEMM is [M x Cin] x [Cin x Cout] complex, executed
 * as three real products (Gauss) on v_mfma_f32_32x32x2_f32.  Replace nothing of the reference: the product path reaches these
 * kernels through gdn_fftconv_fwd / _bwd (AE_model_unet.py:50,53: the 5x5 ... 9x9 ResidualBlock convolutions). */
size_t gdn_fftconv_cgemm_workspace_bytes(const gdn_conv_geom* g);
int gdn_fftconv_cgemm(const gdn_conv_geom* g, int32_t which, void* workspace, size_t workspace_bytes, void* stream);
int gdn_fftconv_cgemm_shape(const gdn_conv_geom* g, int32_t* bins, int32_t* M, int32_t* np);

/* Winograd F(2x2,3x3) convolution for the 3x3 stride-1 layers (zero or reflection padding 1) on
 * 64..512 channels (the 512-channel ResidualBlocks of levels 3 and 4, AE_model_unet.py:45-57; R's
 * decoder ConvBlocks upconv0 / upconv1, :60-77), fp32: 2.25x fewer
 * multiplies than the direct kernel, transforms that only add and halve.  Same contract as
 * gdn_conv_fwd for y / addsrc / stats / ep_scale / ep_shift / act (slots: gdn_winoconv_stats_slots).
 * in_scale / in_shift / in_relu: as for gdn_fftconv_fwd (the producer's train-mode BatchNorm + ReLU
 * applied while the 4x4 patches are loaded).  in_up2x: as for gdn_fftconv_fwd (x2 bilinear upsampling of a
 * low-resolution x while the 4x4 patches are loaded: R's upconv0 / upconv1).
 * state_out (nullable, gdn_winoconv_state_bytes) receives the transformed input, which
 * gdn_winoconv_bwd needs for the weight gradient, followed by the data gradient's transformed weights (written by the same
 * weight-transform launch: the backward of that step then runs no weight transform).  Cin/64 and Cout/64 must be powers of two. */
size_t gdn_winoconv_fwd_workspace_bytes(const gdn_conv_geom* g);
size_t gdn_winoconv_state_bytes(const gdn_conv_geom* g);
int64_t gdn_winoconv_stats_slots(const gdn_conv_geom* g);
int gdn_winoconv_fwd(const gdn_conv_geom* g, const float* x, int32_t ldx, const float* w,
                     float* y, int32_t ldy, const float* addsrc, int32_t ld_add, float* stats,
                     const float* ep_scale, const float* ep_shift, int32_t act,
                     const float* in_scale, const float* in_shift, int32_t in_relu, int32_t in_up2x,
                     void* state_out, void* workspace, size_t workspace_bytes, void* stream);
/* dx = dgrad (+ addsrc) when dx != NULL (needs state, or w when state is NULL), dw[tap][Cout][Cin] = wgrad when
 * dw != NULL (needs state).
 * bnb_* (nullable; replaces the reduce pass of gdn_bn_bwd, AE_model_unet.py:51,54,68): dx is the gradient of
 * z = [relu](BN_train(bnb_y)), bnb_y [B,H,W,Cin] with pitch ld_bnb being that BatchNorm's input and
 * bnb_co = {scale, shift, mean, invstd}[Cin]; the output transform that writes dx (+ addsrc) also writes
 * bnb_partial[slot][2][Cin] = per-slot sum(dz), sum(dz*xhat), dz = dx*[z>0 if bnb_relu], slots =
 * gdn_winoconv_bnb_slots(g) (0: not available -- reflection-padded layers).  (The frequency-domain layers do
 * not offer this: their inverse transforms are VALU-bound and the fused sums measured slower than the reduce pass.)
 * dx_up2x: as for gdn_fftconv_bwd (reflection-padded layers: dx is the gradient of the low-resolution tensor). */
size_t gdn_winoconv_bwd_workspace_bytes(const gdn_conv_geom* g);
int64_t gdn_winoconv_bnb_slots(const gdn_conv_geom* g);
/* Measurement hook: only the 16 per-bin MFMA GEMMs of one forward, V [16][tiles][Cin] x U [16][Cout][Cin]
 * -> Mo [16][tiles][Cout] (tiles = B * ceil(H/2) * ceil(W/2)). */
int gdn_winoconv_gemm(const gdn_conv_geom* g, const float* V, const float* U, float* Mo, void* stream);
int gdn_winoconv_bwd(const gdn_conv_geom* g, const float* dy, int32_t ldy, const float* w,
                     const void* state, float* dx, int32_t ldx, const float* addsrc, int32_t ld_add,
                     float* dw, const float* bnb_y, int32_t ld_bnb, const float* bnb_co, int32_t bnb_relu,
                     float* bnb_partial, int32_t dx_up2x, void* workspace, size_t workspace_bytes, void* stream);
/* The F(4x4,3x3) backward with BOTH gradients, in phases a caller can issue on two streams of its own.  Arguments as
 * gdn_winoconv_bwd; dx, dw and state are all required (w is not read).  The workspace query returns 0 unless the layer plans
 * F(4x4,3x3): F(2x2,3x3) and reflection-padded layers, and calls that want one gradient only, stay with gdn_winoconv_bwd
 * (GDN_ERR_UNSUPPORTED / GDN_ERR_BAD_ARG here).  phases is a mask:
 *   1  both transforms of dy: Vd = B^T d B of the 6x6 patches (data gradient) and Dv = G_w y G_w^T of their inner 4x4 (weight gradient)
 *   2  weight gradient: the reduction GEMM over tiles, then the fold of the 36 bins into dw
 *   4  data gradient: the per-bin GEMMs, then the output transform into dx (+ addsrc, bnb_* partials)
 *   0  all three, in that order, on `stream`
 * Phases 2 and 4 only read what phase 1 wrote and touch disjoint memory otherwise, so they may run on two streams once
 * phase 1 is complete; both must be complete before the workspace, dx or dw is used again.  Workspace layout (every
 * region rounded up to 256 bytes; tiles = B * ceil(H/4) * ceil(W/4)): Vd [36][tiles][Cout], Dv [36][tiles][Cout], the
 * reduction's partial product sets (splits x [36][Cout][Cin]), the data gradient's GEMM output [36][tiles][Cin].
 * Results are bit-identical to gdn_winoconv_bwd's. */
size_t gdn_winoconv_bwd_pair_workspace_bytes(const gdn_conv_geom* g);
int gdn_winoconv_bwd_pair(const gdn_conv_geom* g, const float* dy, int32_t ldy, const float* w,
                          const void* state, float* dx, int32_t ldx, const float* addsrc, int32_t ld_add,
                          float* dw, const float* bnb_y, int32_t ld_bnb, const float* bnb_co, int32_t bnb_relu,
                          float* bnb_partial, int32_t dx_up2x, int32_t phases, void* workspace, size_t workspace_bytes,
                          void* stream);

/* Winograd F(3x3,2x2) for the 4x4 stride-2 pad-1 layers of G (ConvBlock(k4,s2,p1) AE_model_unet.py:497-500 with
 * ReflectionPad2d(1) or zero padding; ConvTBlock = ConvTranspose2d(k4,s2,p1) :517-520), fp32: the layer is a 2x2
 * stride-1 convolution over the four polyphase images of its input, computed with 16 instead of 36 multiplies per 3x3
 * output tile (2.25x fewer than the direct kernel; same interpolation points as F(2x2,3x3)).  Cin, Cout in
 * {64,128,256,512}; Conv2d needs even H, W.  y / addsrc / stats / ep_scale / ep_shift / act as for gdn_conv_fwd (no tanh;
 * slots: gdn_wino2conv_stats_slots).  state_out (Conv2d only, gdn_wino2conv_state_bytes) receives the transformed input
 * for the weight gradient.
 * Backward: dx = dgrad (+ addsrc) when dx != NULL (needs w); dw[tap][Cout][Cin] when dw != NULL -- a Conv2d needs `state`,
 * a ConvTranspose2d needs x (its forward input, pitch ldx_in): its weight gradient shares the transform of dy with the
 * data gradient. */
size_t gdn_wino2conv_fwd_workspace_bytes(const gdn_conv_geom* g);
size_t gdn_wino2conv_state_bytes(const gdn_conv_geom* g);
int64_t gdn_wino2conv_stats_slots(const gdn_conv_geom* g);
int gdn_wino2conv_fwd(const gdn_conv_geom* g, const float* x, int32_t ldx, const float* w,
                      float* y, int32_t ldy, const float* addsrc, int32_t ld_add, float* stats,
                      const float* ep_scale, const float* ep_shift, int32_t act,
                      void* state_out, void* workspace, size_t workspace_bytes, void* stream);
size_t gdn_wino2conv_bwd_workspace_bytes(const gdn_conv_geom* g);
int gdn_wino2conv_bwd(const gdn_conv_geom* g, const float* dy, int32_t ldy, const float* w,
                      const float* x, int32_t ldx_in, const void* state,
                      float* dx, int32_t ldx, const float* addsrc, int32_t ld_add, float* dw,
                      void* workspace, size_t workspace_bytes, void* stream);

/* The 1 <-> 64 channel 9x9 stride-1 pad-4 layers on the matrix cores (G's first convolution AE_model_unet.py:496, the
 * data and weight gradients of the 64 -> 1 heads :362 / :521), fp32.  x1 is a dense single-channel image [B,H,W].
 *   gdn_conv_c1_fwd:   y[p][n] = sum_tap x1[p + tap - 4] * w[tap][n]   (N = 64; taps flipped when flip != 0; zero or reflection
 *                      padding of x1); y / addsrc / stats / ep_scale / ep_shift / act as for gdn_conv_fwd (no tanh), slots =
 *                      gdn_conv_c1_stats_slots.  The first convolution forward, and -- with x1 = d(pre-tanh) -- a head's data gradient.
 *   gdn_conv_c1_wgrad: dw[tap][n] = sum_p gw[p][n] * x1[p + tap - 4]   (gw [B,H,W,64], pitch ldg; result written at the flipped
 *                      tap when flip != 0).  The first convolution's weight gradient (x1 = input, gw = dy) and a head's
 *                      (x1 = d(pre-tanh), gw = the head's input; flip for a Conv2d head, none for a ConvTranspose2d one).
 *   gdn_conv_c1_fwd also takes Cin = 3 (x1 [B,H,W,3], w [tap][64][3]): R's first convolution Conv2d(3, 64, 9) after
 *   ReflectionPad2d(4), AE_model_unet.py:273 (its weight gradient stays on gdn_conv_wgrad).
 *   x1, w, stats, dw stay fp32.  dtypes of gdn_conv_c1_fwd: bit 0 = y is bf16, bit 1 = addsrc is bf16 (a bf16 model's head
 *   data gradient, rounded once after the fp32 add); gw_bf16 != 0: gw is bf16 (the head's bf16 input), ldg % 4 == 0 either way. */
int64_t gdn_conv_c1_stats_slots(int32_t B, int32_t H, int32_t W);
int gdn_conv_c1_fwd(const float* x1, int32_t Cin, int32_t B, int32_t H, int32_t W, int32_t N, int32_t k, int32_t pad, int32_t reflect,
                    int32_t flip, const float* w, void* y, int32_t ldy, const void* addsrc, int32_t ld_add,
                    float* stats, const float* ep_scale, const float* ep_shift, int32_t act, int32_t dtypes, void* stream);
size_t gdn_conv_c1_wgrad_workspace_bytes(void);
int gdn_conv_c1_wgrad(const float* x1, const void* gw, int32_t ldg, int32_t gw_bf16, int32_t B, int32_t H, int32_t W, int32_t N,
                      int32_t k, int32_t pad, int32_t reflect, int32_t flip, float* dw,
                      void* workspace, size_t workspace_bytes, void* stream);

/* fp32 per-bin GEMMs on the bf16 matrix pipe ("bf16 x 3": an fp32 operand is exactly the sum of three bf16 terms; six bf16
 * products, accumulated in fp32, reproduce the fp32 product to its own rounding level at 6/16 of the matrix-pipe cycles) --
 * the core behind the Winograd layers' per-bin GEMMs (torch / cuDNN conv2d of the 512-channel ResidualBlocks,
 * AE_model_unet.py:45-57).  Measurement / test hooks: the product path reaches the same kernels through gdn_winoconv_*.
 *   gdn_gemm_x3_pack : B fp32 row-major [bins][rows][K] -> packed bf16 panels (gdn_gemm_x3_packed_bytes), split once
 *   gdn_gemm_x3_nt   : C[bin][m][n] = sum_k A[bin][m][k] * B[bin][n][k];  A fp32 row-major [bins][M][K] (split while it is
 *                      staged), Bp the packed panels of B [bins][N][K], C fp32 row-major [bins][M][N].
 *   gdn_gemm_x3_tn   : P[split][bin][i][j] = sum_t A[bin][t][i] * B[bin][t][j] over the split's chunk of the T rows (the weight
 *                      gradients' reduction over tiles); A [bins][T][NI], B [bins][T][NJ] fp32 row-major, both split while staged;
 *                      P fp32 [nsplit][bins][NI][NJ], partial sets to be summed by the caller.  NI, NJ multiples of 128.
 * N a multiple of 128, K a multiple of 32 (GDN_ERR_UNSUPPORTED otherwise). */
size_t gdn_gemm_x3_packed_bytes(int32_t bins, int32_t rows, int32_t K);
int gdn_gemm_x3_pack(const float* src, void* dst, int32_t bins, int32_t rows, int32_t K, void* stream);
int gdn_gemm_x3_nt(const float* A, const void* Bp, float* C, int32_t bins, int32_t M, int32_t N, int32_t K, void* stream);
int gdn_gemm_x3_tn(const float* A, const float* B, float* P, int32_t bins, int32_t T, int32_t NI, int32_t NJ, int32_t nsplit,
                   void* stream);
/* gdn_gemm_x3_nt with the kernel form chosen by the caller (tests and measurements; every form gives the same bits).
 * cfg & 0xff: GDN_X3_NT_AUTO = what gdn_gemm_x3_nt and the Winograd layers run; the one-shot launches (one workgroup per 128-
 * or 64-row output block) and the persistent ones (a resident grid, every workgroup walking a static list of output blocks).
 * Flags of the persistent forms: GDN_X3_NT_KEEP_BINS (an XCD keeps whole bins instead of a contiguous range of (bin, row tile)
 * pairs), GDN_X3_NT_NO_HALVES (a ragged last round is not cut into half-height blocks).  GDN_X3_NT_SHARED, with GDN_X3_NT_AUTO
 * only: the launch shares the chip with another stream's GEMM chain, as in the forked Winograd backward.  grid: workgroups of a persistent form,
 * a multiple of 8 up to 8192; 0 = two per CU.  GDN_ERR_BAD_ARG for anything else.
 * Added WITHOUT a new ABI revision, like gdn_grad_accumulate and for the same reason. */
#define GDN_X3_NT_AUTO 0
#define GDN_X3_NT_ONESHOT_128 1
#define GDN_X3_NT_ONESHOT_64 2
#define GDN_X3_NT_UNITS_128 3
#define GDN_X3_NT_UNITS_64 4
#define GDN_X3_NT_KEEP_BINS 0x100
#define GDN_X3_NT_NO_HALVES 0x200
#define GDN_X3_NT_SHARED 0x400
int gdn_gemm_x3_nt_cfg(const float* A, const void* Bp, float* C, int32_t bins, int32_t M, int32_t N, int32_t K, int32_t cfg,
                       int32_t grid, void* stream);
/* host query: the number of reduction splits gdn_winoconv_bwd / gdn_wino2conv_bwd give gdn_gemm_x3_tn for a shape (0: shape not
 * eligible): rounds of the chip per split plus the partial-product sets read back, DESIGN.md 2.10 */
int64_t gdn_gemm_x3_tn_splits(int32_t bins, int32_t T, int32_t NI, int32_t NJ);

/* bf16 weight gradient (BASELINE configs[2]): x and dy hold bfloat16, dw is fp32 (the master
 * gradient arena).  Same contract as gdn_conv_wgrad otherwise.  Needs Cx and Cout multiples of
 * 64, pixel pitches multiples of 8 and 16-byte aligned bases.  v_mfma_f32_32x32x16_bf16 fed by
 * ds_read_b64_tr_b16.  cfg (low 3 bits): 0 automatic; 1 / 3 / 2 force the small / medium / large
 * staging class of the round-1 kernel (tuning, tests); 4 forces wgrad_ring_bf16 (csrc/wgrad_ring.h,
 * round 5: persistent workgroups, LDS-DMA staged row images, one filter-row pair per workgroup,
 * the taps of a row as register shifts of one transposed window -- stride-1 Conv2d with a 3 / 5 / 7 / 9
 * window; GDN_ERR_UNSUPPORTED otherwise), the automatic choice for 5x5 ... 9x9 windows.  Bits 12..15:
 * measurement knobs of that kernel (timing-only variants that drop its DMA traffic or its MFMA
 * loop; 0 in production).  The workspace query takes the same cfg.  Results are bitwise reproducible
 * for a given geometry and cfg (fixed-order split-K). */
size_t gdn_conv_wgrad_bf16_workspace_bytes(const gdn_conv_geom* g, int32_t Cx, int32_t cfg);
int gdn_conv_wgrad_bf16(const gdn_conv_geom* g, const void* x, int32_t ldx, int32_t Cx,
                        const void* dy, int32_t ldy,
                        float* dw, int32_t ld_dw, int32_t ci_off,
                        void* workspace, size_t workspace_bytes, int32_t cfg, void* stream);

/* `dtypes` of the element-wise entry points below: bit i set = the i-th ACTIVATION-type tensor argument
 * (in argument order, NULL-able ones included) holds bfloat16 instead of float; 0 = all fp32.
 * Per-channel coefficient vectors, statistics, parameter gradients and scalars are always fp32. */

/* [ntaps][R][C] -> [ntaps][C][R].  dtypes: bit0 w, bit1 wt (fp32 -> bf16 transposed copy in one pass). */
int gdn_transpose_taps(const void* w, void* wt, int32_t ntaps, int32_t R, int32_t C, int32_t dtypes, void* stream);
/* dst[i] = src[i] with dtype conversion.  dtypes: bit0 src, bit1 dst. */
int gdn_cast(const void* src, void* dst, int64_t n, int32_t dtypes, void* stream);
/* torch layout [A][Bc][ntaps] (Conv2d weight [Cout][Cin][kh][kw], or ConvTranspose2d
 * weight [Cin][Cout][kh][kw]) <-> tap-major [ntaps][Cout][Cin].  a_is_cout selects
 * which of the two leading torch dims is Cout. */
int gdn_weight_to_tapmajor(const float* w_torch, float* w_tap, int32_t Cout, int32_t Cin, int32_t ntaps,
                           int32_t a_is_cout, void* stream);
int gdn_weight_from_tapmajor(const float* w_tap, float* w_torch, int32_t Cout, int32_t Cin, int32_t ntaps,
                             int32_t a_is_cout, void* stream);

/* ------------------------------------------------------------------------
 * BatchNorm2d (AE_model_unet.py:51,54,68,86), ReLU (:52,69,87), residual add (:57).
 * ---------------------------------------------------------------------- */
/* Train mode: reduce the conv kernel's partial statistics (fp64), update the
 * running stats (momentum, unbiased variance), and emit the per-channel
 * affine  scale = gamma*invstd,  shift = beta - mean*scale  plus mean/invstd
 * for backward.  num_batches_tracked (nullable, device int64): += 1, nn.BatchNorm2d's counter. */
int gdn_bn_finalize_train(const float* stats, int64_t slots, int32_t C, int64_t count,
                          const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float momentum, float eps,
                          float* scale, float* shift, float* mean, float* invstd,
                          int64_t* num_batches_tracked, void* stream);
/* Eval mode: scale/shift from the running statistics. */
int gdn_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, int32_t C,
                       float* scale, float* shift, void* stream);
/* out = [relu](y*scale[c] + shift[c]) (+ residual).  npix pixels of C channels.
 * dtypes: bit0 y, bit1 residual, bit2 out. */
int gdn_bn_apply(const void* y, int32_t ldy, const float* scale, const float* shift,
                 const void* residual, int32_t ld_res, void* out, int32_t ld_out,
                 int64_t npix, int32_t C, int32_t relu, int32_t dtypes, void* stream);
/* low = [relu](y*scale[c] + shift[c]) (+ residual), up = F.interpolate(low, scale_factor=2, mode='bilinear', align_corners) in ONE
 * pass over dense NHWC tensors [B,H,W,C] -> [B,2H,2W,C]: a ResidualBlock's output followed by the decoder's upsampling
 * (AE_model_unet.py:55-57 -> :336-359, north_star "bilinear-interp + residual-add fused").  low may be NULL (the block output has
 * no other reader).  Bit-identical to gdn_bn_apply followed by gdn_upsample2x_fwd: the interpolated values are rounded to low's
 * storage type first.  dtypes: bit0 y, bit1 residual, bit2 low, bit3 up (1 = bfloat16).  C % 4 == 0, B * 2H <= 65535. */
int gdn_bn_apply_up2x(const void* y, const float* scale, const float* shift, const void* residual, void* low, void* up,
                      int32_t B, int32_t H, int32_t W, int32_t C, int32_t relu, int32_t align_corners, int32_t dtypes,
                      void* stream);
/* Backward of out = [relu](BN_train(y)):
 *   pass 1 (reduce): per-channel sum(dz), sum(dz*xhat) with dz = dout*[z>0];
 *   pass 2 (apply) : dy = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)),
 *                    dgamma = sum(dz*xhat), dbeta = sum(dz).
 * Both passes inside one call; workspace from gdn_bn_bwd_workspace_bytes.
 * ext_partial (nullable, [ext_slots][2][C]): pass 1 was already done by the epilogue of the kernel that wrote
 * dout (bnb_partial of gdn_winoconv_bwd / gdn_fftconv_bwd) and is skipped.
 * dtypes: bit0 dout, bit1 y, bit2 dy. */
size_t gdn_bn_bwd_workspace_bytes(int64_t npix, int32_t C);
int gdn_bn_bwd(const void* dout, int32_t ld_dout, const void* y, int32_t ldy,
               const float* gamma, const float* scale, const float* shift,
               const float* mean, const float* invstd,
               void* dy, int32_t ld_dy, float* dgamma, float* dbeta,
               int64_t npix, int32_t C, int32_t relu,
               const float* ext_partial, int64_t ext_slots,
               void* workspace, size_t workspace_bytes, int32_t dtypes, void* stream);

/* Passes 1 + 2 of gdn_bn_bwd only: dgamma, dbeta (nullable) and kk = {mean(dz), mean(dz*xhat)}[C] for a consumer that
 * applies pass 3 while loading (gdn_fftconv_bwd dyb_*).  With ext_partial, dout / y / workspace may be NULL. */
int gdn_bn_bwd_coeffs(const void* dout, int32_t ld_dout, const void* y, int32_t ldy,
                      const float* scale, const float* shift, const float* mean, const float* invstd,
                      float* dgamma, float* dbeta, float* kk, int64_t npix, int32_t C, int32_t relu,
                      const float* ext_partial, int64_t ext_slots,
                      void* workspace, size_t workspace_bytes, int32_t dtypes, void* stream);

/* Backward of out = [relu](y*scale + shift) through an EVAL-mode BatchNorm (fixed coefficients from
 * gdn_bn_eval_coeffs): dy = scale*dout*[z>0].  Used when a gradient crosses the frozen guide network
 * (--latent_grad, the guided training of trainer.py:699-703 without the no_grad).  relu: 0 none, 1 y is the raw conv
 * output (mask = y*scale+shift > 0), 2 y is the activated output of a fused conv+BN+ReLU epilogue (mask = y > 0).
 * dtypes: bit0 dout, bit1 y, bit2 dy. */
int gdn_bn_eval_bwd(const void* dout, int32_t ld_dout, const void* y, int32_t ldy,
                    const float* scale, const float* shift, void* dy, int32_t ld_dy,
                    int64_t npix, int32_t C, int32_t relu, int32_t dtypes, void* stream);

/* A TRAINED layer whose BatchNorm stays in eval mode (--freeze_bn: fine-tuning on the stored running statistics).
 * gdn_bn_frozen_coeffs fills the four rows gdn_bn_finalize_train leaves for a train-mode layer from the running
 * statistics: scale / shift exactly as gdn_bn_eval_coeffs (same bits), mean = running_mean, invstd = 1/sqrtf(running_var + eps);
 * nothing is updated. */
int gdn_bn_frozen_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                         float eps, int32_t C, float* scale, float* shift, float* mean, float* invstd, void* stream);
/* Backward of out = [relu](y*scale + shift) with those coefficients, parameter gradients included:
 *   dy = scale*dout*[z>0] (the bits of gdn_bn_eval_bwd, relu 0 / 1), dbeta = sum(dz), dgamma = sum(dz*xhat) with
 *   dz = dout*[z>0], xhat = (y - mean)*invstd.
 * dy depends on no reduction: ONE kernel reads dout and y once, writes dy and per-block partial sums (a grid that is a
 * function of (npix, C) only, a fixed summation order, no atomics), and the finalize kernel of gdn_bn_bwd turns those into
 * dgamma / dbeta (overwritten; either may be NULL, both NULL: no sums at all).  Operands, pitches, C % 4 and `dtypes`
 * (bit0 dout, bit1 y, bit2 dy) as in gdn_bn_bwd; workspace from gdn_bn_frozen_bwd_workspace_bytes.
 * dy == NULL: the sums only (a consumer applies scale and mask itself: gdn_fftconv_bwd dyb_* with kk = 0).
 * ext_partial (nullable, [ext_slots][2][C]): the sums were emitted by the epilogue of the kernel that wrote dout; only the
 * finalize kernel and the dy pass run (with dy == NULL as well, dout / y may be NULL). */
size_t gdn_bn_frozen_bwd_workspace_bytes(int64_t npix, int32_t C);
int gdn_bn_frozen_bwd(const void* dout, int32_t ld_dout, const void* y, int32_t ldy,
                      const float* scale, const float* shift, const float* mean, const float* invstd,
                      void* dy, int32_t ld_dy, float* dgamma, float* dbeta,
                      int64_t npix, int32_t C, int32_t relu,
                      const float* ext_partial, int64_t ext_slots,
                      void* workspace, size_t workspace_bytes, int32_t dtypes, void* stream);

/* ------------------------------------------------------------------------
 * x2 bilinear up-sampling: F.interpolate(align_corners=False) AE_model_unet.py:336,343,349,355
 * and nn.Upsample(align_corners=True) :135,203,215,227.  NHWC, C channels.
 * ---------------------------------------------------------------------- */
/* dtypes: bit0 input, bit1 output. */
int gdn_upsample2x_fwd(const void* x, void* y, int32_t B, int32_t H, int32_t W, int32_t C,
                       int32_t align_corners, int32_t dtypes, void* stream);
int gdn_upsample2x_bwd(const void* dy, void* dx, int32_t B, int32_t H, int32_t W, int32_t C,
                       int32_t align_corners, int32_t dtypes, void* stream);

/* Layout and small element-wise helpers.  dtypes: bit0 x, bit1 y (gdn_add: bit0 a, bit1 b, bit2 out). */
int gdn_nchw_to_nhwc(const void* x, void* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t dtypes, void* stream);
int gdn_nhwc_to_nchw(const void* x, void* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t dtypes, void* stream);
int gdn_add(const void* a, const void* b, void* out, int64_t n, int32_t dtypes, void* stream);
/* out[p][c] = a[p][c] (+ b[p][c], b nullable): npix pixels of C channels, each tensor with its own pixel pitch -- the
 * gradient of a torch.cat half (AE_model_unet.py:340,346,352,358) is a channel slice of the 1x1 conv's data gradient.
 * dtypes: bit0 a, bit1 b, bit2 out. */
int gdn_add_pitched(const void* a, int32_t lda, const void* b, int32_t ldb, void* out, int32_t ld_out,
                    int64_t npix, int32_t C, int32_t dtypes, void* stream);
/* out[i] = x[i] * (*s), s a device scalar: d(loss)/d(pred) times the upstream gradient of the loss node. */
int gdn_scale_dev(const float* x, const float* s, float* out, int64_t n, void* stream);
/* dpre = dout * (1 - out^2): backward of x15.tanh() (AE_model_unet.py:363,571). */
int gdn_tanh_bwd(const float* dout, const float* out, float* dpre, int64_t n, void* stream);
int gdn_fill(float* p, float value, int64_t n, void* stream);

/* ------------------------------------------------------------------------
 * Training losses, forward value and gradient in one call, sync-free (F6).
 * Each writes its scalar to *loss (device) and ADDS its gradient into dout
 * (caller zero-fills dout once per step); `w` scales both.
 * ---------------------------------------------------------------------- */
/* Masked BerHu, trainer.py:433-448 == :705-720.  out/gt [B,1,H,W];
 * sparse [B,Cs,H,W] NCHW (channel 0 used) or NULL; box = {y1,y2,x1,x2}.
 * loss = 3*mean(w*rho).  workspace >= gdn_loss_workspace_bytes().
 * ext_max: NULL = the threshold c = 0.2*max|out-gt| is taken over THIS batch (one reference run, and what
 * each rank of the data-parallel build does); a device float = use that maximum instead -- the value of
 * gdn_absdiff_max after a 4-byte all-reduce(MAX), which reproduces nn.DataParallel's threshold over the
 * gathered batch (--global_berhu). */
size_t gdn_loss_workspace_bytes(int64_t npix);
int gdn_absdiff_max(const float* a, const float* b, int64_t n, float* max_out, void* stream);
int gdn_berhu_masked(const float* out, const float* gt, const float* sparse, int32_t Cs,
                     int32_t B, int32_t H, int32_t W, const int32_t box[4], const float* ext_max,
                     float* loss, float* dout, void* workspace, size_t workspace_bytes, void* stream);
/* Sobel L1, utils.py:105-131 with the factor 3 of trainer.py:453 passed as `weight`.
 * total (nullable): *total = *loss + *plus (plus nullable) -- the step's loss sum, trainer.py:456. */
int gdn_sobel_l1(const float* pred, const float* gt, int32_t B, int32_t H, int32_t W, float weight,
                 float* loss, float* dpred, const float* plus, float* total,
                 void* workspace, size_t workspace_bytes, void* stream);
/* Edge-aware smoothness, utils.py:139-178 + trainer.py:753-754.
 * depth [B,1,H,W], img [B,Ci,H,W] NCHW.  loss = mean|0.1*smooth|.
 * total (nullable): *total = (*loss + *plus) + *plus2 (both nullable) -- trainer.py:757. */
int gdn_smoothness(const float* depth, const float* img, int32_t Ci, int32_t B, int32_t H, int32_t W,
                   float* loss, float* ddepth, const float* plus, const float* plus2, float* total,
                   void* workspace, size_t workspace_bytes, void* stream);
/* loss_accum (+)= weight * mean((a-b)^2): the latent MSE terms, trainer.py:728-733
 * (value only, F3).  accumulate != 0 adds to the existing *loss.  dtypes: bit0 a, bit1 b. */
int gdn_mse(const void* a, const void* b, int64_t n, float weight, int32_t accumulate,
            float* loss, void* workspace, size_t workspace_bytes, int32_t dtypes, void* stream);
/* Gradient of weight*mean((a-b)^2) w.r.t. a, times the device scalar *gscale (NULL = 1):
 * da = gscale * 2*weight/n * (a-b).  dtypes: bit0 a, bit1 b, bit2 da.  (--latent_grad) */
int gdn_mse_grad(const void* a, const void* b, int64_t n, float weight, const float* gscale,
                 void* da, int32_t dtypes, void* stream);
/* Scale-invariant log loss (Eigen et al. 2014, with the variance-focus weight lambda), --loss silog: replaces the BerHu
 * term of trainer.py:433-448 == :705-720 where the user asks for it; the reference has no counterpart.  out / gt / sparse /
 * box as for gdn_berhu_masked (a NULL box with a NULL sparse: every pixel).  With t(x) = (x + 1) / 2 and
 * u(x) = max(t(x), floor):
 *   a pixel is VALID iff t(gt) > floor and, when sparse is given, it lies inside box with sparse > -1;
 *   d_i = log u(out_i) - log u(gt_i) over the n valid pixels, m1 = sum d / n, m2 = sum d^2 / n, D = m2 - lambda * m1^2;
 *   *loss = weight * sqrt(D);  dout_i += weight / (sqrt(D) * n) * (d_i - lambda * m1) / (out_i + 1) at every valid pixel
 *   whose prediction is not clamped (t(out_i) <= floor: no gradient).
 * n == 0 or D <= 0: *loss = 0 and dout is not touched.  A NaN / +Inf prediction at a valid pixel makes *loss and the
 * gradient of every valid pixel non-finite (the gradient guard's business); an invalid pixel's prediction is never read
 * into the sums.  All per-pixel arithmetic and the sums are float64; *loss and each gradient term are rounded to float32
 * once.  Three launches (two when dout is NULL): block partials in a fixed order, a one-workgroup finalize that leaves the
 * two gradient coefficients in the workspace, the gradient pass -- no atomics, bitwise reproducible.
 * stats (nullable, 4 device doubles): n, m1, m2, D.  lambda in [0, 1), floor in (0, 1), weight > 0 (GDN_ERR_BAD_ARG). */
int gdn_silog_masked(const float* out, const float* gt, const float* sparse, int32_t Cs,
                     int32_t B, int32_t H, int32_t W, const int32_t box[4],
                     float lambda, float weight, float floor,
                     float* loss, float* dout, double* stats,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Depth metrics, calculate_error.py:10-103: per image min-max -> x80, Godard
 * crop, validity mask, median scaling (lower median), clamp, 8 reductions.
 * gt_sparse/gt/pred are [B,1,H,W]; errors[8] = batch means, device memory.
 * H * W > INT32_MAX is GDN_ERR_BAD_ARG (here and in the two variants below).
 * Non-finite inputs give torch's results, in all three: min / max / median
 * propagate NaN and the clamp keeps it.  A NaN or +-inf pixel in pred, or a
 * constant pred (0 / 0), gives NaN for every sum and a1 = a2 = a3 = 0; a NaN
 * pixel in gt, or a constant gt, leaves no valid pixel, which like any image
 * without one gives NaN throughout (the reference raises: torch.median of an
 * empty tensor).  A NaN in gt_sparse only drops that pixel here; in the
 * Make3D variant, which min-max normalises gt_np too, it leaves none.
 * ---------------------------------------------------------------------- */
size_t gdn_depth_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W);
int gdn_depth_metrics(const float* gt_sparse, const float* gt, const float* pred,
                      int32_t B, int32_t H, int32_t W, int32_t crop,
                      float* errors, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * NYU Depth v2 depth metrics, calculate_error.py:105-150 (compute_errors_NYU):
 * per image min-max -> x10, valid = (gt < 10) & (gt > 0), with crop the rows AND
 * columns [int(0.0359477 n), int(0.96405229 n)), median scaling (lower median),
 * clamp to [1e-3, 10], 8 reductions in fp64.  gt/pred are [B,1,H,W];
 * errors[8] = batch means of [abs_diff, abs_rel, log10, a1, a2, a3, rmse, rmse_log],
 * device memory.  An image with no valid pixel gives NaN (the reference raises:
 * torch.median of an empty tensor).
 * ---------------------------------------------------------------------- */
size_t gdn_depth_metrics_nyu_workspace_bytes(int32_t B, int32_t H, int32_t W);
int gdn_depth_metrics_nyu(const float* gt, const float* pred, int32_t B, int32_t H, int32_t W, int32_t crop,
                          float* errors, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Make3D depth metrics, calculate_error.py:152-182 (compute_errors_Make3D):
 * gt_np, gt and pred min-max normalised per image; valid = normalised gt_np and
 * gt > 1e-2 and their x80 values < 80; gt and pred x80 clamped to [1e-2, 80]
 * BEFORE the median scaling (none after).  gt_np/gt/pred are [B,1,H,W];
 * errors[4] = batch means of [abs_diff, abs_rel, ave_log10, rmse].  No valid
 * pixel: NaN, as above.
 * ---------------------------------------------------------------------- */
size_t gdn_depth_metrics_make3d_workspace_bytes(int32_t B, int32_t H, int32_t W);
int gdn_depth_metrics_make3d(const float* gt_np, const float* gt, const float* pred, int32_t B, int32_t H, int32_t W,
                             float* errors, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Metric KITTI evaluation under the Eigen-split protocol (--eval_protocol standard).  No counterpart in
 * the reference, whose compute_errors (gdn_depth_metrics above) stretches both maps to their own min / max; its intent is
 * the commented-out block of calculate_error.py:59-76.
 *   gt     [B][Hmax][Wmax]; image b is the top-left h0 x w0 corner, the padding is never read.  gt_kind 0: float32 metres;
 *          1: uint16, metres = v / 256 (the official KITTI PNG, 0 = no return); 2: float32 in [-1, 1] as the loaders
 *          yield it, metres = (float)(((double)v + 1) / 2 * depth_scale)
 *   boxes  device int32 [B][6] = {h0, w0, y1, y2, x1, x2}: size and crop box of each image, from the host, taken as
 *          given (0 <= y1 <= y2 <= h0, likewise in x); h0 / w0 beyond the pool are held to Hmax / Wmax
 *   pred   [B][1][H][W] float32 in [-1, 1]
 * Per pixel (y, x) of the h0 x w0 image, float64 without FMA contraction unless stated: g = ground truth in metres (a
 * float32 value, widened); valid iff g > min_depth, g < max_depth, y1 <= y < y2, x1 <= x < x2.  The prediction at the
 * ground truth's resolution is bilinear with half-pixel centres and edge clamping -- per axis
 * s = max((i + 0.5) * ((double)n_in / n_out) - 0.5, 0), i0 = min(floor(s), n_in - 1), i1 = min(i0 + 1, n_in - 1),
 * w = s - i0; t = (top0 * (1 - wx) + top1 * wx) * (1 - wy) + (bot0 * (1 - wx) + bot1 * wx) * wy over ((double)pred + 1) / 2
 * of the four neighbours -- then p = max((float)(t * depth_scale), 0), rounded to float32 once (NaN propagates; the
 * identity when h0 x w0 == H x W).  median_scaling: ratio = median(valid g) / median(valid p) with numpy's median (the mean
 * of the two middle values of an even count; an exact selection over the float32 bit patterns), else ratio = 1;
 * p <- min(max(p * ratio, min_depth), max_depth), NaN stays NaN.  Over the n valid pixels: abs_rel = mean(|g-p|/g),
 * sq_rel = mean((g-p)^2/g), rmse = sqrt(mean((g-p)^2)), rmse_log = sqrt(mean((ln g - ln p)^2)),
 * a_k = count(max(g/p, p/g) < 1.25^k) / n, log10 = mean(|log10 g - log10 p|),
 * silog = 100 sqrt(max(mean(e^2) - mean(e)^2, 0)) with e = ln p - ln g.
 *   per_image  device [B][12] doubles = {n, ratio, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, log10, silog, 0};
 *              n == 0: {0, NaN x 10, 0}
 * An image is split over several workgroups; partial sums are float64 and combined in a fixed order, the select's
 * histograms are summed with integer atomics, there is no floating-point atomic: two calls on the same inputs give the same
 * 96 B bytes.  One memset node and 3 kernel launches, 6 with median scaling.  min_depth > 0, max_depth > min_depth,
 * depth_scale > 0, all finite, gt_kind in 0..2, Hmax x Wmax and H x W below 2^31, B <= 65535 (GDN_ERR_BAD_ARG).
 * ---------------------------------------------------------------------- */
size_t gdn_depth_metrics_std_workspace_bytes(int32_t B, int32_t Hmax, int32_t Wmax);
int gdn_depth_metrics_std(const void* gt, int32_t gt_kind, int32_t Hmax, int32_t Wmax,
                          const int32_t* boxes, const float* pred, int32_t B, int32_t H, int32_t W,
                          float depth_scale, float min_depth, float max_depth, int32_t median_scaling,
                          double* per_image, void* workspace, size_t workspace_bytes, void* stream);

/* Flip test-time augmentation (--flip_test), float32 rows of W elements, rows = B * C * H:
 * gdn_flip_w: dst[r][x] = src[r][W-1-x] (dst must not be src);
 * gdn_flip_mean: out[r][x] = 0.5f * (a[r][x] + b[r][W-1-x]), bitwise (a + b.flip(-1)) * 0.5; out may be a, not b. */
int gdn_flip_w(const float* src, int64_t rows, int32_t W, float* dst, void* stream);
int gdn_flip_mean(const float* a, const float* b, int64_t rows, int32_t W, float* out, void* stream);

/* ------------------------------------------------------------------------
 * NYU validation transform (GDN_main.py:41-47: CenterCrop, ArrayToTensor,
 * Normalize) for a batch, bit-exact with torch's fp32 arithmetic.
 *   src  [B][H0][W0][C] as decoded: uint8, or float32 when src_is_f32 (NOT
 *        bytescaled: this transform has no imresize); 1 <= C <= 3
 *   the window (off_y, off_x, H, W) must lie inside H0 x W0; CenterCrop's offsets
 *   are round((H0-H)/2), round((W0-W)/2) with Python's round-half-even (the
 *   caller computes them, transform_list.py:260-261)
 *   dst  [B][C][H][W] float32 = (v/255 - 0.5)/0.5
 * ---------------------------------------------------------------------- */
int gdn_crop_normalize(const void* src, int32_t src_is_f32, int32_t B, int32_t H0, int32_t W0, int32_t C,
                       int32_t off_y, int32_t off_x, int32_t H, int32_t W, float* dst, void* stream);

/* ------------------------------------------------------------------------
 * --img_save's image conversion (GDN_main.py:285-307: scipy.misc.imsave ->
 * toimage -> bytescale): src [B][C][H][W] float32 -> dst [B][H][W][C] uint8,
 * per image over all channels jointly, in fp64: cscale = max - min (1 when 0),
 * u8 = trunc(clip((x - min) * (255 / cscale), 0, 255) + 0.5).
 * ---------------------------------------------------------------------- */
int gdn_bytescale_u8(const float* src, int32_t B, int32_t C, int32_t H, int32_t W, uint8_t* dst, void* stream);

/* ------------------------------------------------------------------------
 * KITTI training-time augmentation on the device.  Replaces the host pipeline
 * datasets_list.py:82-101 -> transform_list.py RandomHorizontalFlip :158-166, RandomScaleCrop :185-199
 * (scipy.misc.imresize = bytescale + Pillow bilinear), ArrayToTensor :100-118, Normalize :84-92,
 * bit-exactly (uint8 resampling in Pillow's 22-bit fixed point, IEEE float32 normalisation).
 *   src    [B][H][W][C] as decoded from the image files: uint8, or float32 when src_is_f32 (then the
 *          per-image min/max stretch of scipy's bytescale is applied first); C <= 4
 *   params device int32 [B][5] = {flip, scaled_h, scaled_w, off_y, off_x}: the sample is flipped, resized to
 *          scaled_h x scaled_w (>= H x W) and cropped back to H x W at (off_y, off_x); ignored when train == 0
 *   train  0: validation transform (GDN_main.py:49-52): ArrayToTensor + Normalize only
 *   dst    [B][C][H][W] float32 = (v/255 - 0.5)/0.5
 * ---------------------------------------------------------------------- */
size_t gdn_kitti_augment_workspace_bytes(int32_t B);
int gdn_kitti_augment(const void* src, int32_t src_is_f32, int32_t B, int32_t H, int32_t W, int32_t C,
                      const int32_t* params, int32_t train, float* dst,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Batch assembly from a device-resident training set (no reference counterpart: the reference decodes every file of
 * every batch on the host).  The decoded uint8 images of ALL samples stay in three device pools; one launch picks the
 * batch's samples by index and applies gdn_kitti_augment's transform (the same device code: bit-identical results) to
 * the three images of each, computing a pixel's filter coefficients once for all their channels.
 *   gt_pool [N][H][W][Cg], rgb_pool [N][H][W][Cr], sparse_pool [N][H][W][Cs]  uint8, each C <= 4
 *   sel     device int32 [B][6] = {sample index, flip, scaled_h, scaled_w, off_y, off_x}; when train == 0 only the
 *           index is read.  0 <= index < N is the CALLER's check, made on the host before the rows are uploaded.
 *   gt_out [B][Cg][H][W], rgb_out [B][Cr][H][W], sparse_out [B][Cs][H][W]  float32 = (v/255 - 0.5)/0.5
 * Offsets into the pools are 64-bit.
 * ---------------------------------------------------------------------- */
int gdn_kitti_augment_resident(const uint8_t* gt_pool, int32_t Cg, const uint8_t* rgb_pool, int32_t Cr,
                               const uint8_t* sparse_pool, int32_t Cs, int32_t H, int32_t W, const int32_t* sel,
                               int32_t B, int32_t train, float* gt_out, float* rgb_out, float* sparse_out,
                               void* stream);

/* Indexed copy of whole samples: dst[b] = pool[idx[b]], b < B, samples of per_sample elements of elem_bytes (1 or 2)
 * bytes; idx is a device int32 [B] the caller has range-checked.  to_f32 (elem_bytes 2 only): dst is float32 and every
 * uint16 is widened on the way (exact) -- what decoding a 16-bit PNG to float32 gives.  16-byte accesses where a
 * sample's source and destination are both 16-byte aligned, element-wise for the tail and otherwise; 64-bit offsets. */
int gdn_gather_samples(const void* pool, int32_t elem_bytes, const int32_t* idx, int32_t B, int64_t per_sample,
                       int32_t to_f32, void* dst, void* stream);

/* ------------------------------------------------------------------------
 * NYU Depth v2 training-time augmentation on the device (GDN_main.py:94-129, datasets_list.py:399-430), bit-exact with
 * the host pipeline: imresize (bytescale + Pillow BILINEAR, or Pillow 'F' for depth) to img_s x (251, 340), depth /
 * scale, RandomCropNumpy(251, 340), RandomRotate (scipy.ndimage.rotate, order 3, mode 'constant', reshape=False, clipped
 * to the input's range over all channels), imresize by `scale`, CenterCrop (offsets from the colour image), flip,
 * RandomColor (RtoD), ArrayToTensor, Normalize.  DtoD rotates the depth alone and resizes the colour image once, to
 * 251 x 340; RtoD rotates colour and depth together (Merge) and resizes both again.
 * One struct per sample, in DEVICE memory, filled by the host from the reference's random draws.
 * ---------------------------------------------------------------------- */
typedef struct {
    int32_t h1, w1;       /* first resize: int(img_s * 251) x int(img_s * 340) */
    int32_t y1, x1;       /* RandomCropNumpy: the 251 x 340 window inside h1 x w1 */
    int32_t h2, w2;       /* second resize: int(251 * scale) x int(340 * scale) */
    int32_t cy, cx;       /* CenterCrop offsets: round-half-even of ((251 - H) / 2, (340 - W) / 2) in DtoD, of
                             ((h2 - H) / 2, (w2 - W) / 2) in RtoD; the same window is cut from every image */
    int32_t flip;         /* RandomHorizontalFlip */
    int32_t reserved;     /* 0 */
    double scale;         /* the depth is divided by (float)scale after the first resize */
    double mult;          /* RandomColor multiplier (RtoD; unused in DtoD) */
    double m[4];          /* rotation, as scipy computes it: input (r, c) = (m0 y + m1 x + off0, m2 y + m3 x + off1) */
    double off[2];
    double zn1[2];        /* z^250, z^339 for the spline pole z = sqrt(3) - 2, as running products */
} gdn_nyu_aug_params;

/*   depth      [B][H0][W0] float32 (16-bit depth as decoded);  rgb [B][H0][W0][3] uint8
 *   rtod       0: DtoD (angle range +-4, no RandomColor), 1: RtoD
 *   H, W       output size, H <= 251, W <= 340
 *   depth_out  [B][1][H][W] float32,  rgb_out [B][3][H][W] float32, both (v/255 - 0.5)/0.5 */
size_t gdn_nyu_augment_workspace_bytes(int32_t B, int32_t H0, int32_t W0, int32_t rtod);
int gdn_nyu_augment(const float* depth, const uint8_t* rgb, int32_t B, int32_t H0, int32_t W0, int32_t rtod,
                    const gdn_nyu_aug_params* params, int32_t H, int32_t W, float* depth_out, float* rgb_out,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Building block: Pillow's bilinear resampler (Image.resize(..., BILINEAR)) for any scale, batched.
 *   src        [B][H0][W0][C] uint8, or float32 when src_is_f32; 1 <= C <= 4, channels resized independently
 *   f_mode     1: Pillow 'F' (float32 source, double weights normalised to 1, double sums, float32 between the passes);
 *              0: 8 bpc (22-bit fixed point, horizontal pass rounded to uint8)
 *   bytescale  8 bpc only: scipy's bytescale with each sample's min/max over all channels first (required for float32)
 *   out_h x out_w  the size resized to; only the window (win_y, win_x, win_h, win_w), which must lie inside it, is computed
 *   dst        [B][win_h][win_w][C]: float32 ('F') or uint8 (8 bpc) */
size_t gdn_pil_resize_workspace_bytes(int32_t B, int32_t H0, int32_t C, int32_t win_w);
int gdn_pil_resize_bilinear(const void* src, int32_t src_is_f32, int32_t B, int32_t H0, int32_t W0, int32_t C,
                            int32_t f_mode, int32_t bytescale, int32_t out_h, int32_t out_w, int32_t win_y,
                            int32_t win_x, int32_t win_h, int32_t win_w, void* dst, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Building block: scipy.ndimage.rotate / affine_transform of order 3, mode 'constant', on float32 planes.
 *   src, dst   [B][C][H][W] float32, H, W >= 4; every plane gets the same HOST matrix[4] and offset[2]:
 *              output (y, x) reads the input at (m0 y + m1 x + off0, m2 y + m3 x + off1), 0 outside the plane
 *   clip       1: clip each sample to the min/max of its C input planes (RandomRotate), 0: no clip */
size_t gdn_spline_rotate3_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int gdn_spline_rotate3(const float* src, int32_t B, int32_t C, int32_t H, int32_t W, const double* matrix,
                       const double* offset, int32_t clip, float* dst, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------------
 * Fused Adam with coupled L2 weight decay over one flat arena
 * (torch.optim.Adam(..., weight_decay=5e-4), GDN_main.py:157,173; step at
 * trainer.py:468,768).  grad_scale multiplies the gradient first (1/world
 * after an RCCL sum all-reduce).
 * ---------------------------------------------------------------------- */
int gdn_adam_step(float* p, const float* g, float* m, float* v, int64_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay,
                  int32_t step, float grad_scale, void* stream);
/* The same update with every step-dependent scalar in DEVICE memory, so the launch can be captured in a hipGraph and
 * replayed: hyper = float[6] {lr, beta1, beta2, eps, weight_decay, grad_scale} (the host rewrites it when the schedule
 * changes the learning rate); state = 32 bytes {double beta1^t, double beta2^t, int32 t, float bc1, float bc2s},
 * initialised to {1.0, 1.0, 0, 0, 0} and advanced by the call itself. */
int gdn_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n,
                      const float* hyper, void* state, void* stream);

/* Gradient guard of the capturable update: the global gradient norm, torch.nn.utils.clip_grad_norm_'s coefficient and the
 * decision to skip a step whose gradient holds a NaN or an Inf, all taken on the device (no host read, capturable).
 * guard = 32 bytes of device memory, 8-byte aligned, zero-initialised by the caller:
 *   { double sumsq; float norm; float coef; int32 skip; int32 steps; int32 clipped; int32 skipped; }
 *
 * gdn_grad_sumsq: guard->sumsq = (accumulate ? guard->sumsq : 0) + sum g[i]^2 over n floats (any 4-byte aligned base, n >= 1).
 *   Each element is squared and summed in double (1e30f does not overflow); a NaN or an Inf anywhere makes sumsq non-finite,
 *   which IS the detection.  Two launches: per-block partial sums into `workspace` (gdn_grad_sumsq_workspace_bytes(n); the
 *   grid is a function of n alone), then one block that adds them in a fixed order -- no floating-point atomics: the same
 *   buffer at the same address gives the same bits every time.
 * gdn_grad_guard_finalize (one launch, after the last gdn_grad_sumsq of a step; hyper as for gdn_adam_step_dev), in double:
 *   norm = sqrt(sumsq) * |hyper[5]|, the norm of the gradient as the update sees it;
 *   norm finite:      skip = 0, coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1;
 *   norm not finite:  skip_nonfinite ? (skip = 1, coef = 0) : (skip = 0, coef = 1 -- clipping alone changes nothing there);
 *   norm and coef are stored rounded once to float; steps += 1; clipped += (coef < 1 as stored, and not skipped);
 *   skipped += skip.
 * gdn_adam_step_dev_guarded: gdn_adam_step_dev with grad_scale * coef in the place of grad_scale (bit-identical to it for
 *   coef == 1); with skip != 0 neither the step state nor p, m, v are touched. */
size_t gdn_grad_sumsq_workspace_bytes(int64_t n);
int gdn_grad_sumsq(const float* g, int64_t n, void* guard, int32_t accumulate, void* workspace, size_t workspace_bytes,
                   void* stream);
int gdn_grad_guard_finalize(void* guard, const float* hyper, double max_norm, int32_t skip_nonfinite, void* stream);
int gdn_adam_step_dev_guarded(float* p, const float* g, float* m, float* v, int64_t n,
                              const float* hyper, void* state, const void* guard, void* stream);

/* Exponential moving average of the weights, kept beside the moments (no reference counterpart).
 * gdn_ema_update runs directly after the Adam update of the same store, on the same stream: `state` is the step state that
 *   update has just advanced (gdn_adam_step_dev / gdn_adam_step_dev_guarded), `guard` the record the guarded update read, or
 *   NULL after the unguarded one.  guard != NULL and guard->skip != 0: ema is neither read nor written.  Otherwise, with
 *   t = state->step (1 after the first applied update):
 *     w_t = (float)(1.0 - min(decay, (1.0 + t) / (10.0 + t)))     in double, rounded once -- every thread computes it itself
 *     ema[i] = fmaf(w_t, p[i] - ema[i], ema[i])                    in float32
 *   so the warm-up averages over the steps taken so far until (1 + t) / (10 + t) reaches `decay`.  The state is only read.
 *   One launch; 0 < decay < 1, n >= 1, ema and p 4-byte aligned (GDN_ERR_BAD_ARG otherwise).
 * gdn_swap_f32 exchanges two non-overlapping ranges of n floats in place (one launch); a NULL pointer, n <= 0 or overlapping
 *   ranges return GDN_ERR_BAD_ARG before any launch.
 * Both move 16 bytes per lane where the two bases agree modulo 16 (scalar head and tail around the aligned body) and one float
 * per lane where they do not. */
int gdn_ema_update(float* ema, const float* p, int64_t n, double decay, const void* state, const void* guard, void* stream);
int gdn_swap_f32(float* a, float* b, int64_t n, void* stream);

/* Gradient accumulation (no reference counterpart): acc[i] = acc[i] + g[i] over n floats, one IEEE float32
 * add per element (no FMA, subnormals kept, no atomics), `g` only read: the sum of a group of micro-batch gradients, whose
 * mean the optimizer takes through its gradient scale.  One launch, 16 bytes per lane where the two bases agree modulo 16
 * (scalar head and tail around the aligned body), one float per lane where they do not.  A NULL pointer, n <= 0, a base that
 * is not 4-byte aligned or overlapping ranges return GDN_ERR_BAD_ARG before any launch.
 * Added WITHOUT a new ABI revision: no existing signature or record changed, and the Python loader binds every name it
 * declares when it opens the library, so a revision-223 library built before this symbol existed still fails loudly at load
 * (a missing symbol), never silently at the first accumulating backward. */
int gdn_grad_accumulate(float* acc, const float* g, int64_t n, void* stream);

/* Segmented forms of the capturable update, the gradient norm and the weight average (no reference counterpart; DESIGN.md
 * 3.8): ONE launch over an arena whose parameters belong to several parameter groups, some of them frozen.  Arena slices
 * are 64-float aligned, so a 64-float chunk belongs to one parameter or to padding:
 *   map     uint8[n / 64] in device memory: the group 0 .. G-1 of each chunk, or 0xFF for a chunk to skip (a frozen
 *           parameter, padding after the last parameter).  The padding floats inside a live parameter's last chunk are
 *           updated like its elements (they are zero and stay zero).  The CONTENTS of the map are the caller's to check.
 *   hyper   float[G][6], per group the fields of gdn_adam_step_dev's hyper;
 *   states  G x 32 bytes, per group the step state of gdn_adam_step_dev (8-byte aligned);
 *   guard   the record of gdn_grad_guard_finalize, or NULL (gdn_adam_step_seg, gdn_ema_update_seg).
 * gdn_adam_step_seg: a one-block launch advances each of the G step states as gdn_adam_step_dev advances its own (none of
 *   them when guard->skip != 0), then ONE launch updates every element of a chunk mapped to group k with hyper[k], states[k]
 *   and the gradient scale hyper[k][5] (times guard->coef): bit-identical to gdn_adam_step_dev[_guarded] on that slice with
 *   those records.  p, g, m, v of a skipped chunk are neither read nor written.
 * gdn_grad_sumsq_seg: gdn_grad_sumsq over the chunks that are not skipped (a NaN in a skipped chunk does not reach the sum);
 *   same workspace, a grid that is a function of n alone, double partial sums in a fixed order, no floating-point atomics.
 * gdn_ema_update_seg: gdn_ema_update with the warm-up weight of the chunk's own group's step count; skipped chunks untouched.
 * All move 16 bytes per lane; the 16 lanes of a chunk read its map byte once.  A NULL pointer (guard excepted), n <= 0,
 * n % 64 != 0, G outside 1 .. 254 or a buffer base that is not 16-byte aligned return GDN_ERR_BAD_ARG before any launch.
 * Added WITHOUT a new ABI revision, like gdn_grad_accumulate and for the same reason. */
int gdn_adam_step_seg(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* map, int32_t G,
                      const float* hyper, void* states, const void* guard, void* stream);
int gdn_grad_sumsq_seg(const float* g, int64_t n, const uint8_t* map, void* guard, int32_t accumulate, void* workspace,
                       size_t workspace_bytes, void* stream);
int gdn_ema_update_seg(float* ema, const float* p, int64_t n, const uint8_t* map, double decay, const void* states,
                       const void* guard, void* stream);

/* Learning-rate schedule on the device (no reference counterpart): turns each group's update count into the
 * rate of the update about to run, in front of gdn_adam_step_dev[_guarded] / gdn_adam_step_seg on the same stream.
 *   hyper    float[G][6], the table of gdn_adam_step_dev (G = 1) / gdn_adam_step_seg; only hyper[k][0] is written;
 *   base_lr  double[G] in device memory: per group lr * lr_mult;
 *   states   G x 32 bytes, the step states (8-byte aligned); only read.  u = states[k].t is the number of updates applied so
 *            far, i.e. the 0-based index of the update about to run (a skipped step leaves it where it was);
 *   hyper[k][0] = (float)(base_lr[k] * s(u)), everything in double and rounded to float32 once, s(u) = w(u) * d(u):
 *     w(u) = (u + 1) / warmup for u < warmup, else 1;
 *     d(u) = 1 for u < warmup and for kind 0 (constant); otherwise, with x = min(1, (u - warmup) / max(1, total - warmup)),
 *     kind 1 (linear):  d = floor + (1 - floor) * (1 - x)
 *     kind 2 (cosine):  d = floor + (1 - floor) * (0.5 * (1 + cos(pi * x)))
 *   Warm-up, the linear decay and the product are IEEE double operations without contraction: a host that evaluates the same
 *   expressions in plain double gets the same bits.  cos is the device library's (within double ulps of the host's).
 * One launch of one workgroup, lane k < G does group k; no allocation, no sync, no host read: capturable.  A NULL pointer, G
 * outside 1 .. 254, kind outside 0 .. 2, warmup < 0, total < 1, floor outside [0, 1] or NaN, base_lr or states not 8-byte
 * aligned or hyper not 4-byte aligned return GDN_ERR_BAD_ARG before any launch.
 * Added WITHOUT a new ABI revision, like gdn_grad_accumulate and for the same reason. */
int gdn_lr_schedule(float* hyper, const double* base_lr, const void* states, int32_t G, int32_t kind, int32_t warmup,
                    int32_t total, double floor, void* stream);

/* Decoupled weight decay (AdamW; no reference counterpart): the four update entry points once more, each with
 * the argument list, the return codes, the checks, the records (hyper row of 6 floats, step state, guard, chunk map), the prep
 * launch and the launch geometry of the entry point it is named after -- only the element differs.  weight_decay / hyper[4]
 * is the DECOUPLED rate: it does not enter the gradient, so the moments never see it.  With lr = this update's rate (the
 * launch argument, hyper[0] after a gdn_lr_schedule), step = lr / bc1 and gscale as in the coupled update, in float32:
 *     dec = (float)((double)lr * (double)wd)           computed by the update kernel from the row it reads (the double product of
 *                                                      two floats is exact: this is the float32 product, rounded once)
 *     gi  = g * gscale
 *     mi  = b1 * m + (1 - b1) * gi
 *     vi  = b2 * v + (1 - b2) * gi * gi
 *     q   = step * mi / (sqrtf(vi) / bc2s + eps)
 *     p   = pi - fmaf(dec, pi, q)
 *   every product, sum, quotient and root rounded on its own, the one fmaf the only fused operation, in all four entry points:
 *   on the same slice with the same records they give the same bits, and with wd = 0 the bits of the coupled entry point at
 *   wd = 0.  (The decay is ADDED to the Adam term and subtracted once: p * (1 - lr * wd) loses it in float32 as soon as
 *   lr * wd < 2^-25.)  Mathematically torch.optim.AdamW.  A step the guard skips touches neither p, m, v nor the step state:
 *   it does not decay.  A skipped chunk (0xFF) of gdn_adamw_step_seg is neither read nor written.
 * Added WITHOUT a new ABI revision, like gdn_grad_accumulate and for the same reason. */
int gdn_adamw_step(float* p, const float* g, float* m, float* v, int64_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay,
                   int32_t step, float grad_scale, void* stream);
int gdn_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n,
                       const float* hyper, void* state, void* stream);
int gdn_adamw_step_dev_guarded(float* p, const float* g, float* m, float* v, int64_t n,
                               const float* hyper, void* state, const void* guard, void* stream);
int gdn_adamw_step_seg(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* map, int32_t G,
                       const float* hyper, void* states, const void* guard, void* stream);

/* Training record kept on the device (no reference counterpart).  Both entry points follow this header's
 * contract: no allocation, no sync, no host read, stream-ordered, capturable, every argument checked before any launch.
 *
 * gdn_step_record: one row per training step into a ring in device memory, from records that already live there.
 *   ring     64 + 64 * cap bytes, 8-byte aligned, zeroed ONCE by the caller: a 64-byte header whose first 8 bytes are
 *            uint64 count (the rest is reserved), then cap rows of 64 bytes;
 *   terms    a HOST array of n_terms (0 .. 8) device pointers to float32 scalars (the step's loss terms).  The pointers travel
 *            by value in the kernel's argument block: under capture the addresses of the capture are what replays read;
 *   hyper, state, guard   one row of the Adam hyper table, one step state and the guard record, as gdn_adam_step_dev_guarded
 *            takes them; any of them may be NULL.
 *   One launch of one workgroup writes row count % cap and then count += 1 (calls on one stream are ordered: no atomic):
 *     bytes  0- 7  uint64 seq      count as found
 *            8-11  int32  t        state->t as found; -1 if state is NULL
 *           12-15  int32  skip     guard->skip; -1 if guard is NULL
 *           16-19  float  lr       hyper[0]; quiet NaN (0x7fc00000) if hyper is NULL
 *           20-23  float  norm     guard->norm; quiet NaN if guard is NULL
 *           24-27  float  coef     guard->coef; quiet NaN if guard is NULL
 *           28-31  int32  n_terms
 *           32-63  float  terms[8] *terms[j] for j < n_terms, quiet NaN beyond
 *   Every float is copied as its BIT PATTERN: a NaN loss stays the NaN it is, -0 stays -0.
 *   A NULL ring, cap < 1, n_terms outside 0 .. 8, a NULL term pointer (or array), a ring, state or guard that is not 8-byte
 *   aligned or a hyper or term pointer that is not 4-byte aligned return GDN_ERR_BAD_ARG before any launch.
 *
 * gdn_tensor_sumsq: out[k] = { sum p[i]^2, sum g[i]^2 } over segment k of an arena of n floats, for T segments in one call.
 *   seg      int64[T][2] = {offset, length} in device memory: the slices of a parameter arena -- offsets multiples of 64,
 *            ascending, non-overlapping, offset + length <= n.  The CONTENTS of the table are the caller's to check, like the
 *            chunk map of the segmented Adam (an entry that leaves [0, n) is cut to it: nothing outside the arena is read);
 *   g        may be NULL: the second value of every pair is 0 and g is never read;
 *   out      double[T][2] in device memory.
 *   Each element is widened to double, squared (exact) and summed in double.  Floats outside every segment -- the padding -- are
 *   NOT read; a NaN or an Inf makes its own segment's sum non-finite and no other's.  No floating-point atomics and a fixed
 *   order of additions: the same buffers at the same addresses give the same bytes on every call.
 *   Three launches: the segment table becomes a list of (segment, slab of 16384 floats) items; one workgroup per item streams
 *   its slab with 16-byte loads and leaves one double pair in `workspace`; one workgroup per segment adds its pairs in order.
 *   A NULL p, seg, out or workspace, n <= 0, T < 1, p or g not 16-byte aligned, seg, out or workspace not 8-byte aligned or
 *   workspace_bytes < gdn_tensor_sumsq_workspace_bytes(n, T) return GDN_ERR_BAD_ARG before any launch.
 * Added WITHOUT a new ABI revision, like gdn_grad_accumulate and for the same reason. */
int gdn_step_record(void* ring, int32_t cap, const float* const* terms, int32_t n_terms, const float* hyper,
                    const void* state, const void* guard, void* stream);
size_t gdn_tensor_sumsq_workspace_bytes(int64_t n, int32_t T);
int gdn_tensor_sumsq(const float* p, const float* g, int64_t n, const int64_t* seg, int32_t T, double* out, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Raw Velodyne scans -> sparse ground-truth maps (no reference counterpart): a ragged batch of B scans is
 * projected into the padded pool that gdn_depth_metrics_std reads as gt_kind 0.  All pointers are device memory.
 *   points   float[total][4] as the .bin files store them (x, y, z, reflectance), the scans one after the other, 16-byte
 *            aligned; the fourth float is never used (the homogeneous coordinate is 1);
 *   offsets  int64[B + 1]: image b owns points offsets[b] .. offsets[b + 1] - 1.  The CONTENTS of the table are the caller's
 *            to check, like the chunk map of the segmented Adam;
 *   proj     double[B][12]: the row-major 3 x 4 matrix P = P_rect . R_rect . T_velo_to_cam of each image;
 *   sizes    int32[B][2] = {h0, w0} of each image (held inside Hmax x Wmax);
 *   max_points  at least the largest scan of the batch: it sizes the grid and nothing else (a longer scan is still
 *            projected whole, by the grid stride);
 *   depth    float[B][Hmax][Wmax], 16-byte aligned: every cell is written, the padding and an image without points as +0;
 *   hits     int32[B] or NULL: the number of pixels of each image that come out > 0.
 * Per point, in double without contraction:  drop it unless x >= 0;  r_i = ((P[i][0] x + P[i][1] y) + P[i][2] z) + P[i][3];
 *   u = rint(r_0 / r_2) - 1, v = rint(r_1 / r_2) - 1 (half to even; the -1 is the KITTI devkit's 1-based pixel); keep it iff
 *   u >= 0, v >= 0, u < w0, v < h0, compared in double (NaN and +-inf fail);  d = (float)(depth_kind ? x : r_2): 0 is the
 *   depth along the camera's axis, 1 the scanner's forward distance.  The pixel takes the MINIMUM d of the points on it; a
 *   minimum that is not > 0 reads +0, like a pixel no point hits.
 * One memset node (two with hits), a scatter launch (one no-return 32-bit unsigned atomic min per kept point on an
 * order-preserving key kept in the output cell) and a finalise launch over the whole pool: no workspace, no allocation, no
 * sync, no host read, capturable; integer atomics only, so two calls give the same bytes.  A NULL pointer (hits excepted;
 * points only when max_points is 0), B outside 1 .. 65535, Hmax or Wmax < 1, Hmax * Wmax >= 2^31, depth_kind outside 0 .. 1,
 * max_points < 0 or a misaligned buffer return GDN_ERR_BAD_ARG before any launch.
 * Added WITHOUT a new ABI revision, like gdn_grad_accumulate and for the same reason. */
int gdn_velo_project(const float* points, const int64_t* offsets, const double* proj, const int32_t* sizes, int32_t B,
                     int64_t max_points, int32_t Hmax, int32_t Wmax, int32_t depth_kind, float* depth, int32_t* hits,
                     void* stream);

/* Sparse LiDAR depth -> dense depth, and the bytes of the training files (no reference counterpart).  All
 * pointers are device memory.
 *   depth    float[B][Hmax][Wmax] metres, 16-byte aligned, what gdn_velo_project leaves: 0 = no return.  Cells outside an
 *            image's h0 x w0 are never read;
 *   sizes    int32[B][2] = {h0, w0} of each image (held inside Hmax x Wmax); the CONTENTS are the caller's to check, as in
 *            gdn_velo_project;
 *   out      float[B][Hmax][Wmax], 16-byte aligned, not overlapping depth: every cell is written, the padding as +0;
 *   workspace  gdn_depth_densify_workspace_bytes(B, Hmax, Wmax) bytes (one pool), 16-byte aligned, overlapping neither.
 * The morphological completion of Ku, Harakeh and Waslander (2018), in float32, one IEEE operation per written operation,
 * no contraction; empty(v) := !(v > 0.1f):
 *   1 v = D > 0.1f ? max_depth - D : 0, then 0 where empty(v);  2 max over the 5 x 5 diamond (out-of-image 0);  3 max over
 *   the 5 x 5 box (out-of-image 0), then min over it (out-of-image ignored);  4 where empty(v): the 7 x 7 box max;  5 rows
 *   above a column's topmost non-empty row take its value;  6 where empty(v): the 31 x 31 box max;  7 where !empty(v): the
 *   13th smallest of the 5 x 5 window, borders replicated;  8 where !empty(v): the [1 4 6 4 1] / 16 blur, rows then columns,
 *   each ((((p0 + 4 p1) + 6 p2) + 4 p3) + p4) * 0.0625f, borders reflected without the edge sample (period 2 (n - 1); a
 *   single row or column reads itself);  out = empty(v) ? +0 : max_depth - v.
 * Four launches (steps 1-4, 5, 6, 7-8), no atomics, no allocation, no sync, no host read, capturable; two calls give the
 * same bytes.  A NULL pointer, B outside 1 .. 65535, Hmax or Wmax < 1, Hmax * Wmax >= 2^31, a misaligned buffer, overlapping
 * buffers, a short workspace, or a max_depth that is not finite or is <= 0.2 return GDN_ERR_BAD_ARG before any launch.
 *
 * gdn_depth_encode_u8: x float[n] metres (16-byte aligned) -> out uint8[n] (4-byte aligned),
 *   q = rint(clamp(d, 0, scale) / scale * 255) in double, half to even, NaN -> 0; with keep_valid a d > 0 that rounds to 0
 *   becomes 1 (byte 0 of a sparse map means no return).  One launch.  A NULL pointer, n < 1, a scale that is not finite or
 *   not > 0, keep_valid outside 0 .. 1 or a misaligned buffer return GDN_ERR_BAD_ARG before the launch.
 * Added WITHOUT a new ABI revision, like gdn_grad_accumulate and for the same reason. */
size_t gdn_depth_densify_workspace_bytes(int32_t B, int32_t Hmax, int32_t Wmax);
int gdn_depth_densify(const float* depth, const int32_t* sizes, int32_t B, int32_t Hmax, int32_t Wmax, float max_depth,
                      float* out, void* workspace, size_t workspace_bytes, void* stream);
int gdn_depth_encode_u8(const float* x, int64_t n, double scale, int32_t keep_valid, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------
 * Measurement aid (no reference counterpart): the shader clock the chip holds WHILE a window of launches runs, so a
 * roofline fraction can be read against the clock of the box it was measured on (bench.py `clock_ghz`, `frac_at_clock`).
 *   buf    HOST-PINNED memory mapped into the device (hipHostMalloc; not device memory: the setter and the watcher run on
 *          different XCDs, whose L2s are not coherent inside a kernel), uint64[4]:
 *          {flag, shader cycles (s_memtime), 100 MHz ticks (s_memrealtime), ended_by_flag}
 *   gdn_clock_probe_arm(buf, stream)            clears buf, stream-ordered BEFORE the measured launches;
 *   gdn_clock_probe_watch(buf, max_ticks, side) one wave on a SECOND stream of the caller's (which must wait for the arm):
 *                                               reads both counters, sleeps until the flag is set or max_ticks (<= 1e9 =
 *                                               10 s) have passed, reads them again: clock = cycles / ticks x 100 MHz;
 *   gdn_clock_probe_stop(buf, stream)           sets the flag, stream-ordered AFTER the measured launches.
 * One sleeping wave: no LDS, 16 registers -- it fits beside any kernel of this library.
 * ---------------------------------------------------------------------- */
int gdn_clock_probe_arm(uint64_t* buf, void* stream);
int gdn_clock_probe_watch(uint64_t* buf, uint64_t max_ticks, void* side_stream);
int gdn_clock_probe_stop(uint64_t* buf, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GDN_HIP_H */
