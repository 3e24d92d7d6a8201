"""Thin tensor-level wrappers over the C ABI (one Python function per entry point).

Activations are torch tensors used purely as device buffers: shape [B,H,W,C],
fp32, channel stride 1; a channel slice of a wider tensor is allowed (pixel
pitch ``ld`` = stride(2)).  Everything launches on torch's current stream.
"""
import ctypes
import math
import os

import numpy as np
import torch

from ._lib import ConvGeom, GdnError, lib

ACT_NONE, ACT_TANH, ACT_RELU = 0, 1, 2       # bit flags
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _is_bf16(t):
    return 1 if t is not None and t.dtype == torch.bfloat16 else 0


def _ld(t):
    if t.shape[-1] == 1:          # single channel: the pixel pitch is all that matters
        return t.stride(-2) if t.shape[-2] > 1 else 1
    if t.stride(-1) != 1:
        raise GdnError("activation must have channel stride 1, got strides %s" % (t.stride(),))
    return t.stride(-2)


def _chk(t, name="tensor", bf16_ok=False):
    ok = t.dtype == torch.float32 or (bf16_ok and t.dtype == torch.bfloat16)
    if not ok or not t.is_cuda:
        raise GdnError("%s must be a CUDA/HIP float32 tensor (got %s on %s); the HIP path has no CPU fallback"
                       % (name, t.dtype, t.device))
    return t


CFG_BF16 = 0x10000      # GDN_CFG_BF16
HINT_TRAIN, HINT_NO_X3, HINT_NO_WINO_F4, HINT_FFT_NP32, HINT_FFT_NP40 = 1, 2, 4, 8, 16      # GDN_HINT_* bits of gdn_conv_geom.hints
HINT_FLIP_TAPS = 32


def plan_override_hints():
    """Test / measurement hooks of THIS BINDING (the C library reads no environment variable): GDN_PLAN_BATCH=<n>,
    GDN_RING_CUS=<n>, GDN_FFT_NP=<32|40> become the plan-override fields of gdn_conv_geom.hints of every geometry built while
    they are set."""
    h = 0
    e = os.environ
    if e.get("GDN_PLAN_BATCH"):
        n = int(e["GDN_PLAN_BATCH"])
        if not 1 <= n <= 255:           # an 8-bit field: masking would silently plan for another batch
            raise GdnError("GDN_PLAN_BATCH=%d is outside 1..255" % n)
        h |= n << 8
    if e.get("GDN_RING_CUS"):
        n = int(e["GDN_RING_CUS"])
        if not 8 <= n <= 2040 or n % 8:
            raise GdnError("GDN_RING_CUS=%d must be a multiple of 8 in 8..2040" % n)
        h |= (n // 8) << 16
    if e.get("GDN_FFT_NP") in ("32", "40"):
        h |= HINT_FFT_NP32 if e["GDN_FFT_NP"] == "32" else HINT_FFT_NP40
    return h

# bf16 x 3 split products for the Winograd per-bin GEMMs.  The switch lives HERE, not in the library: the
# environment variable GDN_X3 is read once, at import; distributed._guard_shared_gpu (ranks sharing one GPU), tests and
# measurements call set_x3().  Every geometry handed to the C ABI carries the decision as GDN_HINT_NO_X3, and a forward's
# saved state remembers the hints it was written with, so its backward reads the weight set in the form it was written in
# even if the switch moved in between.
_x3 = os.environ.get("GDN_X3", "1")[:1] != "0"
_x3_explicit = "GDN_X3" in os.environ


def x3_enabled():
    return _x3


def x3_explicit():
    """True when the user chose (GDN_X3 in the environment at import, or set_x3(explicit=True))."""
    return _x3_explicit


def set_x3(on, explicit=False):
    """Switch the bf16 x 3 GEMMs on / off for every layer planned from now on; returns the previous setting."""
    global _x3, _x3_explicit
    prev, _x3 = _x3, bool(on)
    _x3_explicit = _x3_explicit or explicit
    return prev


def _state_x3(state):
    """The switch a forward wrote `state` under (None: stateless call, use the current one)."""
    return getattr(state, "_gdn_x3", None) if state is not None else None


# Winograd F(4x4,3x3) for the zero-padded 3x3 layers: GDN_WINO_F4=0 in the environment at import, or
# set_wino_f4(False), keeps F(2x2,3x3) -- carried to the library as GDN_HINT_NO_WINO_F4 in every geometry, like the switch above
# (the saved state of a forward is laid out for the plan it was written under; its backward passes the same hint).
_f4 = os.environ.get("GDN_WINO_F4", "1")[:1] != "0"


def wino_f4_enabled():
    return _f4


def set_wino_f4(on):
    """Switch the F(4x4,3x3) plan on / off for every layer planned from now on; returns the previous setting."""
    global _f4
    prev, _f4 = _f4, bool(on)
    return prev


def _state_f4(state):
    return getattr(state, "_gdn_f4", None) if state is not None else None


def _bf(t):
    """dtype-mask bit of a tensor argument: 1 for bfloat16, 0 for float32 / None."""
    if t is None or t.dtype == torch.float32:
        return 0
    if t.dtype == torch.bfloat16:
        return 1
    raise GdnError("unsupported dtype %s (float32 or bfloat16)" % t.dtype)


def _mask(*ts):
    m = 0
    for i, t in enumerate(ts):
        m |= _bf(t) << i
    return m


def _same_dtype(ref, *others):
    for o in others:
        if o is not None and o.dtype != ref.dtype:
            raise GdnError("mixed dtypes in one conv call: %s vs %s" % (ref.dtype, o.dtype))


_ws_cache = {}


def workspace(nbytes, device, tag="ws"):
    """Grow-only scratch buffer per (device, tag, current stream): calls on one stream are ordered, so they may share
    scratch memory; two streams (or threads driving their own streams) never do.  Inside a hipGraph capture a missing or
    too small buffer is allocated as a plain temporary instead (it lives in the graph's private pool and must not be
    handed to later eager calls)."""
    key = (device, tag, torch.cuda.current_stream(device).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        if not torch.cuda.is_current_stream_capturing():
            _ws_cache[key] = buf
    return buf


_side_streams = {}


def side_stream(device):
    """The caller-owned second stream gdn_fftconv_bwd's weight-gradient chain runs on (one per device; every use is a
    fork from / join into the caller's current stream, so sharing it only serialises)."""
    st = _side_streams.get(device)
    if st is None:
        st = torch.cuda.Stream(device=device)
        _side_streams[device] = st
    return st


class ShaderClock:
    """Measurement aid: the shader clock the chip holds while the launches inside the `with` block run on the current stream
    (gdn_clock_probe_*: one sleeping wave on a second stream reads s_memtime / s_memrealtime at both ends of the window).

        with ops.ShaderClock(dev) as clk:
            for _ in range(reps): launch()
        torch.cuda.synchronize(); clk.ghz()      # None if no stream was found that runs beside the current one

    The watcher only works on a stream whose hardware queue is not the current stream's: HIP deals its streams onto a handful
    of hardware queues, and a watcher that shares the queue of the stream it watches sits IN FRONT of the launches it is
    meant to bracket (the r06 full-suite runs: the watcher ran into its tick limit after earlier tests had created a few
    dozen streams).  So the side stream is chosen by trial -- a 1 ms watcher that must see a stop issued right behind it --
    among a high-priority stream and up to eight fresh ones, once per (device, current stream)."""

    _side = {}            # (device index, current stream handle) -> torch.cuda.Stream or None

    def __init__(self, device, max_s=2.0):
        # host-pinned, device-mapped: the flag is polled across XCDs whose L2s are not coherent for device memory (gdn_hip.h)
        self.buf = torch.zeros(4, dtype=torch.int64).pin_memory()
        self.max_ticks = int(min(max_s, 10.0) * 1e8)
        self.device = torch.device(device)
        self.side = self._find_side()

    def _trial(self, side, ticks):
        main = torch.cuda.current_stream(self.device)
        self.buf.zero_()
        lib.gdn_clock_probe_arm(self.buf.data_ptr(), main.cuda_stream)
        side.wait_stream(main)
        lib.gdn_clock_probe_watch(self.buf.data_ptr(), ticks, side.cuda_stream)
        lib.gdn_clock_probe_stop(self.buf.data_ptr(), main.cuda_stream)
        main.wait_stream(side)
        torch.cuda.synchronize(self.device)
        return bool(self.buf[3].item())

    def _find_side(self):
        main = torch.cuda.current_stream(self.device)
        key = (self.device.index or 0, main.cuda_stream)
        if key not in ShaderClock._side:
            found = None
            for i in range(9):
                cand = torch.cuda.Stream(device=self.device, priority=-1 if i == 0 else 0)
                if self._trial(cand, 100000):            # 1 ms: ended by the flag only if it ran beside the stop
                    found = cand
                    break
            ShaderClock._side[key] = found
        return ShaderClock._side[key]

    def __enter__(self):
        self.buf.zero_()
        if self.side is not None:
            main = torch.cuda.current_stream(self.device)
            lib.gdn_clock_probe_arm(self.buf.data_ptr(), main.cuda_stream)
            self.side.wait_stream(main)
            lib.gdn_clock_probe_watch(self.buf.data_ptr(), self.max_ticks, self.side.cuda_stream)
        return self

    def __exit__(self, *exc):
        if self.side is not None:
            main = torch.cuda.current_stream(self.device)
            lib.gdn_clock_probe_stop(self.buf.data_ptr(), main.cuda_stream)
            main.wait_stream(self.side)
        return False

    def read(self):
        """(shader cycles, 100 MHz ticks, ended_by_flag) of the window; call after a synchronize."""
        _, cyc, ticks, ended = [int(v) for v in self.buf.tolist()]
        return cyc, ticks, bool(ended)

    def ghz(self, min_ticks=1000):
        cyc, ticks, ended = self.read()
        if not ended or ticks < min_ticks or cyc <= 0:
            return None
        return cyc / ticks * 0.1


class Conv:
    """Geometry + launch helper for one Conv2d / ConvTranspose2d layer.

    Weights are tap-major [k*k, Cout, Cin] (see AE_model_unet._tap_view).

    flip_taps: a stride-1 ConvTranspose2d(cin, cout, k, 1, k // 2) given as the convolution it is (GDN_HINT_FLIP_TAPS: the
    correlation with the stored taps in reverse order) -- the form in which the transform-domain paths (fft_* / wino_*) run it
    forward AND backward; w_tap / dw_tap are the module's own tap-major weight and gradient.  The direct entry points (fwd /
    dgrad / wgrad) take the same layer as transposed=True."""

    def __init__(self, cin, cout, k, stride=1, pad=0, reflect=False, transposed=False, flip_taps=False):
        if flip_taps:
            if transposed or reflect or stride != 1 or k % 2 == 0 or pad != k // 2:
                raise GdnError("flip_taps describes a stride-1 ConvTranspose2d with odd k and padding k // 2 as a plain "
                               "convolution: transposed / reflect must be off")
            if not int(lib.gdn_hints_supported()) & HINT_FLIP_TAPS:
                raise GdnError("libgdn_hip.so does not implement GDN_HINT_FLIP_TAPS; rebuild it")
        self.cin, self.cout, self.k, self.stride, self.pad = cin, cout, k, stride, pad
        self.reflect, self.transposed, self.flip_taps = bool(reflect and pad > 0), transposed, bool(flip_taps)
        self._geom = {}
        self._fwd_ws = {}
        self._slots = {}

    def geom(self, B, H, W, hints=0, x3=None, f4=None):
        """x3 / f4: None = the current switch; a saved state's backward passes what its forward used."""
        if not (_x3 if x3 is None else x3):
            hints |= HINT_NO_X3
        if not (_f4 if f4 is None else f4):
            hints |= HINT_NO_WINO_F4
        hints |= plan_override_hints()
        if self.flip_taps:
            hints |= HINT_FLIP_TAPS
        key = (B, H, W, hints)
        g = self._geom.get(key)
        if g is None:
            cg = ConvGeom(B, H, W, self.cin, self.cout, self.k, self.stride, self.pad,
                          1 if self.reflect else 0, 1 if self.transposed else 0, hints)
            ho, wo = ctypes.c_int32(), ctypes.c_int32()
            lib.gdn_conv_out_dims(ctypes.byref(cg), ctypes.byref(ho), ctypes.byref(wo))
            g = (cg, ctypes.byref(cg), ho.value, wo.value)
            self._geom[key] = g
        return g

    def stats_slots(self, B, H, W, tile_cfg=0):
        _, ref, _, _ = self.geom(B, H, W)
        return int(lib.gdn_conv_stats_slots(ref, tile_cfg))

    def fwd(self, x, w_tap, x2=None, stats=False, act=ACT_NONE, addsrc=None, tile_cfg=0, out=None, stats_out=None,
            affine=None):
        """y = tanh?(relu?(conv(cat(x, x2)) * scale + shift) + addsrc); returns y, or (y, stats_partials) when stats.
        affine = (scale, shift) per output channel (an eval-mode BatchNorm folded into the epilogue) or None."""
        _chk(x, "x", bf16_ok=True)
        bf = x.dtype == torch.bfloat16
        head_mixed = bf and self.cout == 1       # 1-channel heads: bf16 x, fp32 weights and depth map
        if head_mixed:
            _chk(w_tap, "head weight")
            if x2 is not None or addsrc is not None or stats or affine is not None:
                raise GdnError("the bf16 head takes no concat / addsrc / stats / affine")
        else:
            _same_dtype(x, x2, w_tap, addsrc, out)
        if bf:
            tile_cfg |= CFG_BF16
        B, H, W, C1 = x.shape
        _, ref, Ho, Wo = self.geom(B, H, W)
        ph = plan_override_hints()       # part of every cache key below: an override changes the plan, hence slot count and workspace
        c2 = 0 if x2 is None else x2.shape[3]
        if C1 + c2 != self.cin:
            raise GdnError("conv expects %d input channels, got %d" % (self.cin, C1 + c2))
        y = out if out is not None else torch.empty((B, Ho, Wo, self.cout),
                                                    dtype=torch.float32 if head_mixed else x.dtype, device=x.device)
        st = None
        if stats:
            st = stats_out
            slots = self._slots.get((B, H, W, tile_cfg, ph))
            if slots is None:
                slots = int(lib.gdn_conv_stats_slots(ref, tile_cfg))
                self._slots[(B, H, W, tile_cfg, ph)] = slots
            if st is None:
                st = torch.empty((slots, 2, self.cout), dtype=torch.float32, device=x.device)
            elif (st.dtype != torch.float32 or not st.is_contiguous() or st.dim() != 3 or st.shape[0] != slots
                  or tuple(st.shape[1:]) != (2, self.cout)):
                # the kernel writes one slot per tile of the configuration it picks: a buffer sized for another tile_cfg is
                # overrun (or leaves slots unwritten that the finalize pass then sums)
                raise GdnError("conv fwd: stats_out must be a dense float32 [%d, 2, %d] for this geometry and tile_cfg, got %s"
                               % (slots, self.cout, tuple(st.shape)))
        nb = self._fwd_ws.get((B, H, W, tile_cfg, ph))
        if nb is None:
            nb = int(lib.gdn_conv_fwd_workspace_bytes(ref, tile_cfg))
            self._fwd_ws[(B, H, W, tile_cfg, ph)] = nb
        ws = workspace(nb, x.device, "splitk") if nb else None
        try:
            lib.gdn_conv_fwd(ref, _p(x), _ld(x), _p(x2), 0 if x2 is None else _ld(x2), C1, _p(w_tap), _p(y), _ld(y),
                             _p(addsrc), 0 if addsrc is None else _ld(addsrc), _p(st),
                             None if affine is None else _p(affine[0]), None if affine is None else _p(affine[1]),
                             act, tile_cfg, _p(ws), nb, stream())
        except GdnError as e:
            raise GdnError("%s [conv %d->%d k%d s%d p%d reflect=%s transposed=%s, x %s ld %d, x2 %s]" % (
                e, self.cin, self.cout, self.k, self.stride, self.pad, self.reflect, self.transposed,
                tuple(x.shape), _ld(x), None if x2 is None else tuple(x2.shape))) from None
        return (y, st) if stats else y

    def dgrad_bnb_slots(self, B, H, W, dtype, tile_cfg=0):
        """Slots of the BatchNorm-backward partials dgrad's epilogue can emit for this layer (0: it cannot)."""
        _, ref, _, _ = self.geom(B, H, W)
        return int(lib.gdn_conv_dgrad_bnb_slots(ref, tile_cfg | (CFG_BF16 if dtype == torch.bfloat16 else 0)))

    def dgrad(self, dy, wt_tap, in_hw, addsrc=None, tile_cfg=0, bnb=None, up2x=0):
        """dx = dgrad(dy) (+ addsrc).  wt_tap: [k*k, Cin, Cout]; in_hw: layer input (H, W).
        bnb = (y, co, relu, partial): dx is the final gradient of [relu](BN_train(y)); `partial` [dgrad_bnb_slots, 2, Cin]
        receives that BatchNorm's backward partial sums (as wino_bwd's bnb).
        up2x (1: align_corners False, 2: True): the layer's input was the x2 bilinear upsampling of a tensor t; dx (and addsrc)
        are dL/dt [B, H/2, W/2, Cin] (reflection-padded layers: the fold pass applies the adjoint interpolation)."""
        _chk(dy, "dy", bf16_ok=True)
        _same_dtype(dy, wt_tap, addsrc)
        if dy.dtype == torch.bfloat16:
            tile_cfg |= CFG_BF16
        B = dy.shape[0]
        H, W = in_hw
        _, ref, Ho, Wo = self.geom(B, H, W)
        if tuple(dy.shape[1:]) != (Ho, Wo, self.cout):
            raise GdnError("dgrad: dy shape %s does not match layer output (%d,%d,%d)" % (tuple(dy.shape), Ho, Wo, self.cout))
        dx = torch.empty((B, H // 2, W // 2, self.cin) if up2x else (B, H, W, self.cin), dtype=dy.dtype, device=dy.device)
        if up2x and addsrc is not None and tuple(addsrc.shape) != tuple(dx.shape):
            raise GdnError("dgrad(up2x): addsrc must be the low-resolution gradient %s" % (tuple(dx.shape),))
        nb = int(lib.gdn_conv_dgrad_workspace_bytes(ref, tile_cfg))
        ws = workspace(nb, dy.device, "dgrad") if nb else None
        by, bco, brelu, bpart = bnb if bnb is not None else (None, None, False, None)
        if by is not None and by.dtype != dy.dtype:
            raise GdnError("dgrad: the BatchNorm input of the fused backward reduction must have the gradient's dtype")
        lib.gdn_conv_dgrad(ref, _p(dy), _ld(dy), _p(wt_tap), _p(dx), _ld(dx), _p(addsrc),
                           0 if addsrc is None else _ld(addsrc), _p(by), 0 if by is None else _ld(by), _p(bco),
                           1 if brelu else 0, _p(bpart), int(up2x), _p(ws), nb, tile_cfg, stream())
        return dx

    # ---- FFT-domain path (csrc/conv_fft.hip): stride-1 zero-padded fp32 layers with 64..256 channels ----
    def fft_ok(self, B, H, W, backward=False, train=False):
        """True when gdn_fftconv_fwd (and, with `backward`, gdn_fftconv_bwd) supports this layer at this input size.
        Stride-1 ConvTranspose2d layers are forward-only as transposed=True and have the backward as flip_taps=True.  train (here and in fft_fwd / fft_bwd, the same value for one
        layer instance): GDN_HINT_TRAIN -- forward + backward of a trained layer, tiled for the sum of both."""
        _, ref, _, _ = self.geom(B, H, W, 1 if train else 0)
        if backward:
            return int(lib.gdn_fftconv_bwd_workspace_bytes(ref)) > 0
        return int(lib.gdn_fftconv_spectrum_bytes(ref)) > 0

    def fft_stats_slots(self, B, H, W, train=False):
        _, ref, _, _ = self.geom(B, H, W, 1 if train else 0)
        return int(lib.gdn_fftconv_stats_slots(ref))

    def fft_fwd(self, x, w_tap, stats=False, addsrc=None, spectrum=False, out=None, stats_out=None, affine=None,
                act=ACT_NONE, in_affine=None, in_relu=False, up2x=0, train=False):
        """y = conv(x) (+ addsrc) through the frequency domain; returns y, then the BatchNorm partials when `stats`,
        then the input spectrum (opaque uint8 buffer for fft_bwd) when `spectrum`.
        in_affine = (scale, shift): x is a raw conv output and the layer input is [relu](x*scale + shift), applied on load.
        up2x (1: align_corners False, 2: True): x is the low-resolution tensor, upsampled x2 (bilinear) on load."""
        _chk(x, "x"); _chk(w_tap, "w")
        B, H, W, C1 = x.shape
        if up2x:
            H, W = 2 * H, 2 * W
        _, ref, Ho, Wo = self.geom(B, H, W, 1 if train else 0)
        nb = int(lib.gdn_fftconv_fwd_workspace_bytes(ref))
        if nb == 0 or C1 != self.cin:
            raise GdnError("fftconv: unsupported layer k=%d stride=%d Cin=%d Cout=%d" % (self.k, self.stride, C1, self.cout))
        y = out if out is not None else torch.empty((B, Ho, Wo, self.cout), dtype=torch.float32, device=x.device)
        st = None
        if stats:
            st = stats_out if stats_out is not None else torch.empty(
                (int(lib.gdn_fftconv_stats_slots(ref)), 2, self.cout), dtype=torch.float32, device=x.device)
        xf = torch.empty(int(lib.gdn_fftconv_spectrum_bytes(ref)), dtype=torch.uint8, device=x.device) if spectrum else None
        ws = workspace(nb, x.device, "fft")
        lib.gdn_fftconv_fwd(ref, _p(x), _ld(x), _p(w_tap), _p(y), _ld(y), _p(addsrc), 0 if addsrc is None else _ld(addsrc),
                            _p(st), _p(affine[0]) if affine else None, _p(affine[1]) if affine else None, int(act),
                            _p(in_affine[0]) if in_affine else None, _p(in_affine[1]) if in_affine else None,
                            1 if in_relu else 0, int(up2x), _p(xf), _p(ws), nb, stream())
        res = (y,) + ((st,) if stats else ()) + ((xf,) if spectrum else ())
        return res if len(res) > 1 else y

    def wino_bnb_slots(self, B, H, W):
        _, ref, _, _ = self.geom(B, H, W)
        return int(lib.gdn_winoconv_bnb_slots(ref))

    def fft_bnb_slots(self, B, H, W, train=False):
        """Slots of the BatchNorm-backward partial sums fft_bwd's data-gradient gather can emit (`bnb`); 0: not available."""
        _, ref, _, _ = self.geom(B, H, W, 1 if train else 0)
        return int(lib.gdn_fftconv_bnb_slots(ref))

    def fft_bwd(self, dy, w_tap, in_hw, xf=None, dw_tap=None, need_dx=True, addsrc=None, dyb=None, up2x=0, train=False,
                bnb=None):
        """Data gradient (returned; + addsrc) and / or weight gradient (into dw_tap, needs the forward's saved state xf:
        input + weight spectra) from one transform of dy.  w_tap is the FORWARD tap-major weight [k*k, Cout, Cin]; it is
        only read when xf is None.
        dyb = (y_raw, coeffs[4,Cout], kk[2,Cout], relu): `dy` is dout of THIS layer's train-mode BatchNorm; the dy transform
        applies scale*(dz - k1 - xhat*k2) while loading (kk from bn_bwd_coeffs).
        up2x: the forward upsampled a low-resolution x on load; dx (and addsrc) are that tensor's gradient [B,H/2,W/2,Cin]
        (in_hw stays the convolution's input extent).
        bnb = (y_in, coeffs[4,Cin], relu, partial[fft_bnb_slots,2,Cin]): dx is the final gradient of this layer's input
        [relu](BN_train(y_in)); the pass that writes dx fills `partial` with that BatchNorm's backward sums (bn_bwd `partial`);
        it needs need_dx."""
        _chk(dy, "dy")
        B = dy.shape[0]
        H, W = in_hw
        _, ref, Ho, Wo = self.geom(B, H, W, 1 if train else 0)
        nb = int(lib.gdn_fftconv_bwd_workspace_bytes(ref))
        if nb == 0:
            raise GdnError("fftconv: unsupported layer k=%d stride=%d" % (self.k, self.stride))
        if bnb is not None and not need_dx:
            raise GdnError("fft_bwd: bnb needs the data gradient (need_dx)")
        by, bco, brelu, bpart = bnb if bnb is not None else (None, None, False, None)
        if bpart is not None and (bpart.dtype != torch.float32 or not bpart.is_contiguous()
                                  or tuple(bpart.shape) != (int(lib.gdn_fftconv_bnb_slots(ref)), 2, self.cin)):
            raise GdnError("fft_bwd: bnb partial must be a dense float32 [%d, 2, %d]" % (int(lib.gdn_fftconv_bnb_slots(ref)), self.cin))
        if tuple(dy.shape[1:]) != (Ho, Wo, self.cout):
            raise GdnError("fft_bwd: dy shape %s does not match layer output" % (tuple(dy.shape),))
        dx = torch.empty((B, H // 2, W // 2, self.cin) if up2x else (B, H, W, self.cin), dtype=torch.float32,
                         device=dy.device) if need_dx else None
        ws = workspace(nb, dy.device, "fft")
        yy, yco, ykk, yrelu = dyb if dyb is not None else (None, None, None, False)

        def call(phases, st):
            lib.gdn_fftconv_bwd(ref, _p(dy), _ld(dy), _p(w_tap), _p(xf), _p(dx),
                                0 if dx is None else _ld(dx), _p(addsrc), 0 if addsrc is None else _ld(addsrc),
                                _p(dw_tap), _p(yy), 0 if yy is None else _ld(yy), _p(yco), _p(ykk), 1 if yrelu else 0,
                                _p(by), 0 if by is None else _ld(by), _p(bco), 1 if brelu else 0, _p(bpart),
                                int(up2x), phases, _p(ws), nb, st)
        if dw_tap is not None and need_dx:
            # the two chains only share the spectrum of dy and are each latency-bound: the weight-gradient chain runs on a
            # second stream of OURS next to the data-gradient chain (fork after the transform, join before returning)
            main = torch.cuda.current_stream(dy.device)
            side = side_stream(dy.device)
            call(1, main.cuda_stream)
            side.wait_stream(main)
            call(2, side.cuda_stream)
            call(4, main.cuda_stream)
            main.wait_stream(side)
        else:
            call(0, stream())
        return dx

    # ---- Winograd F(2x2,3x3) path (csrc/conv_wino.hip): 3x3 stride-1 zero-padded fp32 layers with 64..512 channels ----
    def fft_cgemm_only(self, B, H, W, which, ws=None, train=False, st=None):
        """Measurement hook: only the per-bin complex GEMMs of this layer's frequency-domain plan (which: 0 forward, 1 data
        gradient, 2 weight-gradient reduction) on a scratch workspace; returns (workspace, bins, tiles, points)."""
        _, ref, _, _ = self.geom(B, H, W, hints=HINT_TRAIN if train else 0)
        nb = int(lib.gdn_fftconv_cgemm_workspace_bytes(ref))
        if nb == 0:
            raise GdnError("fftconv: unsupported layer k=%d stride=%d" % (self.k, self.stride))
        if ws is None:
            ws = torch.empty(nb // 4, dtype=torch.float32, device="cuda").normal_()
        lib.gdn_fftconv_cgemm(ref, int(which), _p(ws), nb, stream() if st is None else st)
        bins, M, npnt = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        lib.gdn_fftconv_cgemm_shape(ref, ctypes.byref(bins), ctypes.byref(M), ctypes.byref(npnt))
        return ws, bins.value, M.value, npnt.value

    def wino_ok(self, B, H, W, backward=False):
        """True when gdn_winoconv_fwd (and, with `backward`, gdn_winoconv_bwd) supports this layer at this input size."""
        _, ref, _, _ = self.geom(B, H, W)
        if backward:
            return int(lib.gdn_winoconv_bwd_workspace_bytes(ref)) > 0
        return int(lib.gdn_winoconv_state_bytes(ref)) > 0

    def wino_fwd(self, x, w_tap, stats=False, addsrc=None, state=False, affine=None, act=ACT_NONE, in_affine=None,
                 in_relu=False, up2x=0):
        """y = conv3x3(x) (+ epilogue) by Winograd F(2x2,3x3); returns y, then the BatchNorm partials when `stats`, then
        the transformed input (opaque buffer for wino_bwd) when `state`.  up2x: as for fft_fwd."""
        _chk(x, "x"); _chk(w_tap, "w")
        B, H, W, C1 = x.shape
        if up2x:
            H, W = 2 * H, 2 * W
        _, ref, Ho, Wo = self.geom(B, H, W)
        nb = int(lib.gdn_winoconv_fwd_workspace_bytes(ref))
        if nb == 0 or C1 != self.cin:
            raise GdnError("winoconv: unsupported layer k=%d stride=%d Cin=%d Cout=%d" % (self.k, self.stride, C1, self.cout))
        y = torch.empty((B, Ho, Wo, self.cout), dtype=torch.float32, device=x.device)
        st = torch.empty((int(lib.gdn_winoconv_stats_slots(ref)), 2, self.cout), dtype=torch.float32,
                         device=x.device) if stats else None
        sv = torch.empty(int(lib.gdn_winoconv_state_bytes(ref)), dtype=torch.uint8, device=x.device) if state else None
        if sv is not None:
            sv._gdn_x3 = _x3                 # the form of the saved weight set (fp32 / bf16 x 3 panels) follows the switch
            sv._gdn_f4 = _f4                 # ... and the layout of the saved input transform (16 / 36 bins) the plan
        ws = workspace(nb, x.device, "fft")
        lib.gdn_winoconv_fwd(ref, _p(x), _ld(x), _p(w_tap), _p(y), _ld(y), _p(addsrc), 0 if addsrc is None else _ld(addsrc),
                             _p(st), _p(affine[0]) if affine else None, _p(affine[1]) if affine else None, int(act),
                             _p(in_affine[0]) if in_affine else None, _p(in_affine[1]) if in_affine else None,
                             1 if in_relu else 0, int(up2x), _p(sv), _p(ws), nb, stream())
        res = (y,) + ((st,) if stats else ()) + ((sv,) if state else ())
        return res if len(res) > 1 else y

    def wino_gemm_only(self, V, U, Mo, B, H, W):
        """Measurement hook: the 16 per-bin GEMMs of one forward on already transformed operands."""
        _, ref, _, _ = self.geom(B, H, W)
        lib.gdn_winoconv_gemm(ref, _p(V), _p(U), _p(Mo), stream())

    def wino_bwd(self, dy, w_tap, in_hw, state=None, dw_tap=None, need_dx=True, addsrc=None, bnb=None, up2x=0):
        """Data gradient (returned; + addsrc) and / or weight gradient (into dw_tap, needs the forward's `state`).
        w_tap is the FORWARD tap-major weight [9, Cout, Cin]."""
        _chk(dy, "dy")
        B = dy.shape[0]
        H, W = in_hw
        _, ref, Ho, Wo = self.geom(B, H, W, x3=_state_x3(state), f4=_state_f4(state))
        nb = int(lib.gdn_winoconv_bwd_workspace_bytes(ref))
        if nb == 0:
            raise GdnError("winoconv: unsupported layer k=%d stride=%d" % (self.k, self.stride))
        if tuple(dy.shape[1:]) != (Ho, Wo, self.cout):
            raise GdnError("wino_bwd: dy shape %s does not match layer output" % (tuple(dy.shape),))
        if bnb is not None and not need_dx:
            raise GdnError("wino_bwd: bnb needs the data gradient (need_dx)")
        dx = torch.empty((B, H // 2, W // 2, self.cin) if up2x else (B, H, W, self.cin), dtype=torch.float32,
                         device=dy.device) if need_dx else None
        by, bco, brelu, bpart = bnb if bnb is not None else (None, None, False, None)
        npair = int(lib.gdn_winoconv_bwd_pair_workspace_bytes(ref)) if dw_tap is not None and need_dx and not up2x else 0
        if npair and state is not None:
            # F(4x4,3x3) with both gradients: the weight-gradient chain and the data-gradient chain share only the read of
            # dy, and each GEMM leaves part of the chip idle in its last round of workgroups -- the weight-gradient chain runs
            # on the second stream of OURS next to the data-gradient chain, as in fft_bwd.  The join before returning keeps a
            # 16-bit-matrix kernel from running beside the next layer's kernels and makes the shared workspace safe.
            ws = workspace(npair, dy.device, "fft")

            def call(phases, st):
                lib.gdn_winoconv_bwd_pair(ref, _p(dy), _ld(dy), _p(w_tap), _p(state), _p(dx), _ld(dx), _p(addsrc),
                                          0 if addsrc is None else _ld(addsrc), _p(dw_tap), _p(by), 0 if by is None else _ld(by),
                                          _p(bco), 1 if brelu else 0, _p(bpart), 0, phases, _p(ws), npair, st)
            main = torch.cuda.current_stream(dy.device)
            side = side_stream(dy.device)
            call(1, main.cuda_stream)
            side.wait_stream(main)
            call(2, side.cuda_stream)
            call(4, main.cuda_stream)
            main.wait_stream(side)
            return dx
        ws = workspace(nb, dy.device, "fft")
        lib.gdn_winoconv_bwd(ref, _p(dy), _ld(dy), _p(w_tap), _p(state), _p(dx), 0 if dx is None else _ld(dx), _p(addsrc),
                             0 if addsrc is None else _ld(addsrc), _p(dw_tap), _p(by), 0 if by is None else _ld(by), _p(bco),
                             1 if brelu else 0, _p(bpart), int(up2x), _p(ws), nb, stream())
        return dx

    # ---- Winograd F(3x3,2x2) path (csrc/conv_wino2.hip): 4x4 stride-2 pad-1 Conv2d / ConvTranspose2d, fp32, 64..512 channels ----
    def wino2_ok(self, B, H, W):
        _, ref, _, _ = self.geom(B, H, W)
        return int(lib.gdn_wino2conv_fwd_workspace_bytes(ref)) > 0

    def wino2_fwd(self, x, w_tap, stats=False, addsrc=None, state=False, affine=None, act=ACT_NONE):
        """y = conv / conv-transpose (k4, s2, p1) (+ epilogue) by Winograd F(3x3,2x2) over the polyphase images; returns y,
        then the BatchNorm partials when `stats`, then the saved state for wino2_bwd when `state` (the transformed input of a
        Conv2d; the input tensor itself for a ConvTranspose2d, whose backward transforms dy instead)."""
        _chk(x, "x"); _chk(w_tap, "w")
        B, H, W, C1 = x.shape
        _, ref, Ho, Wo = self.geom(B, H, W)
        nb = int(lib.gdn_wino2conv_fwd_workspace_bytes(ref))
        if nb == 0 or C1 != self.cin:
            raise GdnError("wino2conv: unsupported layer k=%d stride=%d Cin=%d Cout=%d" % (self.k, self.stride, C1, self.cout))
        y = torch.empty((B, Ho, Wo, self.cout), dtype=torch.float32, device=x.device)
        st = torch.empty((int(lib.gdn_wino2conv_stats_slots(ref)), 2, self.cout), dtype=torch.float32,
                         device=x.device) if stats else None
        sv = None
        if state:
            sb = int(lib.gdn_wino2conv_state_bytes(ref))
            sv = torch.empty(sb, dtype=torch.uint8, device=x.device) if sb else x
        ws = workspace(nb, x.device, "fft")
        lib.gdn_wino2conv_fwd(ref, _p(x), _ld(x), _p(w_tap), _p(y), _ld(y), _p(addsrc), 0 if addsrc is None else _ld(addsrc),
                              _p(st), _p(affine[0]) if affine else None, _p(affine[1]) if affine else None, int(act),
                              _p(sv) if (sv is not None and sv is not x) else None, _p(ws), nb, stream())
        res = (y,) + ((st,) if stats else ()) + ((sv,) if state else ())
        return res if len(res) > 1 else y

    def wino2_bwd(self, dy, w_tap, in_hw, state=None, dw_tap=None, need_dx=True, addsrc=None, bnb=None):
        """Data gradient (returned; + addsrc) and / or weight gradient (into dw_tap, needs the forward's `state`).
        bnb: as wino_bwd's, for the callers that treat the paths alike -- but this path emits no BatchNorm-backward partials
        (gdn_wino2conv_bwd has no such output), so anything but None is an error, not a partial buffer left unwritten."""
        _chk(dy, "dy")
        if bnb is not None:
            raise GdnError("wino2_bwd: this path emits no BatchNorm-backward partials (bnb)")
        B = dy.shape[0]
        H, W = in_hw
        _, ref, Ho, Wo = self.geom(B, H, W)
        nb = int(lib.gdn_wino2conv_bwd_workspace_bytes(ref))
        if nb == 0:
            raise GdnError("wino2conv: unsupported layer k=%d stride=%d" % (self.k, self.stride))
        if tuple(dy.shape[1:]) != (Ho, Wo, self.cout):
            raise GdnError("wino2_bwd: dy shape %s does not match layer output" % (tuple(dy.shape),))
        dx = torch.empty((B, H, W, self.cin), dtype=torch.float32, device=dy.device) if need_dx else None
        ws = workspace(nb, dy.device, "fft")
        xin = state if self.transposed else None
        sv = None if self.transposed else state
        lib.gdn_wino2conv_bwd(ref, _p(dy), _ld(dy), _p(w_tap), _p(xin), 0 if xin is None else _ld(xin), _p(sv), _p(dx),
                              0 if dx is None else _ld(dx), _p(addsrc), 0 if addsrc is None else _ld(addsrc), _p(dw_tap),
                              _p(ws), nb, stream())
        return dx

    def wgrad(self, x, dy, dw_tap, ci_off=0, cfg=0):
        """dw_tap[tap][co][ci_off + ci] = wgrad over the channel slice x (Cx = x.shape[3]).
        bf16 x/dy take the bf16 MFMA kernel; dw_tap is fp32 either way."""
        _chk(x, "x", bf16_ok=True)
        _chk(dy, "dy", bf16_ok=True)
        _chk(dw_tap, "dw")
        B, H, W, Cx = x.shape
        _, ref, _, _ = self.geom(B, H, W)
        if x.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16:
            nb = int(lib.gdn_conv_wgrad_bf16_workspace_bytes(ref, Cx, cfg))
            if nb == 0:
                raise GdnError("bf16 wgrad: unsupported geometry k=%d stride=%d Cx=%d Cout=%d" % (self.k, self.stride, Cx, self.cout))
            ws = workspace(nb, x.device, "wgrad")
            lib.gdn_conv_wgrad_bf16(ref, _p(x), _ld(x), Cx, _p(dy), _ld(dy), _p(dw_tap), self.cin, ci_off, _p(ws), nb, cfg,
                                    stream())
            return
        nb = int(lib.gdn_conv_wgrad_workspace_bytes(ref, Cx))
        if nb == 0:
            raise GdnError("wgrad: unsupported geometry k=%d stride=%d Cx=%d" % (self.k, self.stride, Cx))
        ws = workspace(nb, x.device, "wgrad")
        lib.gdn_conv_wgrad(ref, _p(x), _ld(x), Cx, _p(dy), _ld(dy), _p(dw_tap), self.cin, ci_off, _p(ws), nb,
                           _mask(x, dy), stream())


def c1_ok(x1, n, k, stride, pad, rgb=False):
    """The 1 <-> 64 channel 9x9 layers of csrc/conv_c1.hip: a dense fp32 single-channel image against 64 channels
    (rgb: the forward also takes a 3-channel image, R's first layer)."""
    return (x1.dtype == torch.float32 and x1.dim() == 4 and (x1.shape[3] == 1 or (rgb and x1.shape[3] == 3)) and x1.is_contiguous()
            and n == 64 and k == 9 and stride == 1 and pad == 4)


def conv_c1_fwd(x1, w81, reflect=False, flip=False, stats=False, addsrc=None, affine=None, act=ACT_NONE, out_dtype=torch.float32):
    """y[B,H,W,64] = sum_{tap,c} x1[p + tap - 4][c] * w81[tap][:][c]; x1 [B,H,W,Cin], Cin = 1 or 3, w81 any tensor of 81*64*Cin
    floats in [tap][64][Cin] order.  y (out_dtype) and addsrc may be bf16: a bf16 model's head data gradient."""
    _chk(x1, "x1"); _chk(w81, "w")
    if x1.dtype != torch.float32 or w81.dtype != torch.float32:
        raise GdnError("conv_c1_fwd: the image and the weights are fp32")
    B, H, W, cin = x1.shape
    if cin not in (1, 3) or w81.numel() != 81 * 64 * cin or not w81.is_contiguous() or not x1.is_contiguous():
        raise GdnError("conv_c1_fwd: dense [B,H,W,1|3] image and 81 x 64 x Cin contiguous weights expected")
    y = torch.empty((B, H, W, 64), dtype=out_dtype, device=x1.device)
    st = torch.empty((int(lib.gdn_conv_c1_stats_slots(B, H, W)), 2, 64), dtype=torch.float32, device=x1.device) if stats else None
    dtypes = _is_bf16(y) | (_is_bf16(addsrc) << 1)
    lib.gdn_conv_c1_fwd(_p(x1), cin, B, H, W, 64, 9, 4, 1 if reflect else 0, 1 if flip else 0, _p(w81), _p(y), 64, _p(addsrc),
                        0 if addsrc is None else _ld(addsrc), _p(st), _p(affine[0]) if affine else None,
                        _p(affine[1]) if affine else None, int(act), dtypes, stream())
    return (y, st) if stats else y


def conv_c1_wgrad(x1, gw, dw81, reflect=False, flip=False):
    """dw81[tap][:] = sum_p gw[p][:] * x1[p + tap - 4] (written at the flipped tap when flip); gw [B,H,W,64], fp32 or bf16."""
    _chk(x1, "x1"); _chk(gw, "gw", bf16_ok=True); _chk(dw81, "dw")
    B, H, W, _ = x1.shape
    if dw81.numel() != 81 * 64 or not dw81.is_contiguous() or tuple(gw.shape) != (B, H, W, 64):
        raise GdnError("conv_c1_wgrad: bad shapes")
    nb = int(lib.gdn_conv_c1_wgrad_workspace_bytes())
    ws = workspace(nb, x1.device, "wgrad")
    lib.gdn_conv_c1_wgrad(_p(x1), _p(gw), _ld(gw), _is_bf16(gw), B, H, W, 64, 9, 4, 1 if reflect else 0, 1 if flip else 0, _p(dw81),
                          _p(ws), nb, stream())


def gemm_x3_pack(Bm):
    """fp32 [bins, rows, K] -> packed bf16 x 3 panels (opaque uint8 buffer for gemm_x3_nt)."""
    _chk(Bm, "B")
    bins, rows, K = Bm.shape
    nb = int(lib.gdn_gemm_x3_packed_bytes(bins, rows, K))
    if nb == 0 or not Bm.is_contiguous():
        raise GdnError("gemm_x3_pack: needs a dense [bins, rows, K] tensor with K a multiple of 32")
    out = torch.empty(nb, dtype=torch.uint8, device=Bm.device)
    lib.gdn_gemm_x3_pack(_p(Bm), _p(out), bins, rows, K, stream())
    return out


# kernel forms of gemm_x3_nt (GDN_X3_NT_* of gdn_hip.h): the one-shot launches, the persistent unit walks, and the flags of the latter
X3_NT_AUTO, X3_NT_ONESHOT_128, X3_NT_ONESHOT_64, X3_NT_UNITS_128, X3_NT_UNITS_64 = 0, 1, 2, 3, 4
X3_NT_KEEP_BINS, X3_NT_NO_HALVES, X3_NT_SHARED = 0x100, 0x200, 0x400


def gemm_x3_nt(A, Bp, N, out=None, tile_cfg=X3_NT_AUTO, grid=0):
    """C[bin] = A[bin] @ B[bin]^T with fp32 A [bins, M, K], packed B (gemm_x3_pack of [bins, N, K]); fp32 C [bins, M, N].
    tile_cfg (tests, measurements): the kernel form, X3_NT_*; grid: workgroups of a persistent form (a multiple of 8, 0 = two
    per CU).  Every form gives the same bits."""
    _chk(A, "A")
    bins, M, K = A.shape
    C = out if out is not None else torch.empty((bins, M, N), dtype=torch.float32, device=A.device)
    if tile_cfg == X3_NT_AUTO and grid == 0:
        lib.gdn_gemm_x3_nt(_p(A), _p(Bp), _p(C), bins, M, N, K, stream())
    else:
        lib.gdn_gemm_x3_nt_cfg(_p(A), _p(Bp), _p(C), bins, M, N, K, tile_cfg, grid, stream())
    return C


def gemm_x3_tn(A, Bm, nsplit=1):
    """P[split, bin] = A[bin]^T @ B[bin] over the split's rows; A [bins, T, NI], B [bins, T, NJ] fp32 -> [nsplit, bins, NI, NJ]."""
    _chk(A, "A"); _chk(Bm, "B")
    bins, T, NI = A.shape
    NJ = Bm.shape[2]
    P = torch.empty((nsplit, bins, NI, NJ), dtype=torch.float32, device=A.device)
    lib.gdn_gemm_x3_tn(_p(A), _p(Bm), _p(P), bins, T, NI, NJ, nsplit, stream())
    return P


def transpose_taps(w_tap, out=None, dtype=None):
    """[T, R, C] -> [T, C, R]; dtype (or out.dtype) may differ from w_tap's: fp32 master -> bf16 copy."""
    T, R, C = w_tap.shape
    wt = out if out is not None else torch.empty((T, C, R), dtype=dtype or w_tap.dtype, device=w_tap.device)
    lib.gdn_transpose_taps(_p(w_tap), _p(wt), T, R, C, _mask(w_tap, wt), stream())
    return wt


def cast(src, dtype=None, out=None):
    """Dense dtype conversion fp32 <-> bf16 (one streaming kernel)."""
    if not src.is_contiguous():
        raise GdnError("cast needs a dense tensor")
    dst = out if out is not None else torch.empty(src.shape, dtype=dtype, device=src.device)
    lib.gdn_cast(_p(src), _p(dst), src.numel(), _mask(src, dst), stream())
    return dst


def weight_to_tapmajor(w, transposed):
    """torch-layout conv weight -> tap-major [k*k, Cout, Cin] (w contiguous)."""
    A, Bc, kh, kw = w.shape
    cout, cin = (Bc, A) if transposed else (A, Bc)
    out = torch.empty((kh * kw, cout, cin), dtype=torch.float32, device=w.device)
    lib.gdn_weight_to_tapmajor(_p(w.contiguous()), _p(out), cout, cin, kh * kw, 0 if transposed else 1, stream())
    return out


def weight_from_tapmajor(w_tap, k, transposed):
    T, cout, cin = w_tap.shape
    shape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    out = torch.empty(shape, dtype=torch.float32, device=w_tap.device)
    lib.gdn_weight_from_tapmajor(_p(w_tap), _p(out), cout, cin, T, 0 if transposed else 1, stream())
    return out


def bn_finalize_train(stats, count, gamma, beta, running_mean, running_var, momentum=BN_MOMENTUM, eps=BN_EPS,
                      num_batches_tracked=None):
    slots, _, C = stats.shape
    co = torch.empty((4, C), dtype=torch.float32, device=stats.device)   # scale, shift, mean, invstd
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or not num_batches_tracked.is_cuda):
        raise GdnError("num_batches_tracked must be a device int64 tensor")
    lib.gdn_bn_finalize_train(_p(stats), slots, C, int(count), _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                              momentum, eps, _p(co[0]), _p(co[1]), _p(co[2]), _p(co[3]), _p(num_batches_tracked), stream())
    return co


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps=BN_EPS):
    C = running_mean.numel()
    co = torch.empty((2, C), dtype=torch.float32, device=running_mean.device)
    lib.gdn_bn_eval_coeffs(_p(gamma), _p(beta), _p(running_mean), _p(running_var), eps, C, _p(co[0]), _p(co[1]), stream())
    return co


def bn_apply(y, scale, shift, relu, residual=None, out=None, out_dtype=None):
    B, H, W, C = y.shape
    o = out if out is not None else torch.empty((B, H, W, C), dtype=out_dtype or y.dtype, device=y.device)
    lib.gdn_bn_apply(_p(y), _ld(y), _p(scale), _p(shift), _p(residual), 0 if residual is None else _ld(residual),
                     _p(o), _ld(o), B * H * W, C, 1 if relu else 0, _mask(y, residual, o), stream())
    return o


def bn_bwd(dout, y, gamma, coeffs, relu, dgamma, dbeta, out_dtype=None, partial=None):
    """coeffs = [scale, shift, mean, invstd] from bn_finalize_train. Returns dy.
    partial [slots,2,C]: the reduce pass was done by the epilogue that wrote dout (wino_bwd `bnb`)."""
    B, H, W, C = y.shape
    npix = B * H * W
    dy = torch.empty((B, H, W, C), dtype=out_dtype or y.dtype, device=y.device)
    nb = int(lib.gdn_bn_bwd_workspace_bytes(npix, C))
    ws = workspace(nb, y.device, "bnbwd")
    lib.gdn_bn_bwd(_p(dout), _ld(dout), _p(y), _ld(y), _p(gamma), _p(coeffs[0]), _p(coeffs[1]), _p(coeffs[2]),
                   _p(coeffs[3]), _p(dy), _ld(dy), _p(dgamma), _p(dbeta), npix, C, 1 if relu else 0,
                   _p(partial), 0 if partial is None else partial.shape[0], _p(ws), nb, _mask(dout, y, dy), stream())
    return dy


def bn_bwd_coeffs(dout, y, coeffs, relu, dgamma, dbeta, partial=None):
    """Passes 1 + 2 of the BatchNorm backward: writes dgamma / dbeta (may be None), returns kk [2,C] = mean(dz), mean(dz*xhat)
    for a consumer that applies pass 3 in its loader (Conv.fft_bwd dyb)."""
    B, H, W, C = y.shape
    npix = B * H * W
    kk = torch.empty((2, C), dtype=torch.float32, device=y.device)
    nb = int(lib.gdn_bn_bwd_workspace_bytes(npix, C))
    ws = workspace(nb, y.device, "bnbwd")
    lib.gdn_bn_bwd_coeffs(_p(dout), _ld(dout), _p(y), _ld(y), _p(coeffs[0]), _p(coeffs[1]), _p(coeffs[2]), _p(coeffs[3]),
                          _p(dgamma), _p(dbeta), _p(kk), npix, C, 1 if relu else 0, _p(partial),
                          0 if partial is None else partial.shape[0], _p(ws), nb, _mask(dout, y), stream())
    return kk


def bn_eval_bwd(dout, y, coeffs, relu, out_dtype=None):
    """Backward through an eval-mode BN (+ReLU): coeffs = [scale, shift] from bn_eval_coeffs. Returns dy.
    relu: False/0 none, True/1 y is the raw conv output, 2 y is the activated output of a fused epilogue."""
    B, H, W, C = y.shape
    dy = torch.empty((B, H, W, C), dtype=out_dtype or y.dtype, device=y.device)
    lib.gdn_bn_eval_bwd(_p(dout), _ld(dout), _p(y), _ld(y), _p(coeffs[0]), _p(coeffs[1]), _p(dy), _ld(dy), B * H * W, C,
                        int(relu), _mask(dout, y, dy), stream())
    return dy


def bn_frozen_coeffs(gamma, beta, running_mean, running_var, eps=BN_EPS):
    """[scale, shift, mean, invstd] of a TRAINED layer whose BatchNorm stays in eval mode: bn_finalize_train's block, from the
    running statistics (scale / shift: the bits of bn_eval_coeffs).  Updates nothing."""
    C = running_mean.numel()
    co = torch.empty((4, C), dtype=torch.float32, device=running_mean.device)
    lib.gdn_bn_frozen_coeffs(_p(gamma), _p(beta), _p(running_mean), _p(running_var), eps, C, _p(co[0]), _p(co[1]), _p(co[2]),
                             _p(co[3]), stream())
    return co


def bn_frozen_bwd(dout, y, coeffs, relu, dgamma, dbeta, out_dtype=None, partial=None, need_dy=True, out=None):
    """Backward through an eval-mode BatchNorm (+ReLU) of a trained layer, coeffs from bn_frozen_coeffs: one pass writes
    dy = scale*dout*[z>0] (returned; the bits of bn_eval_bwd) and the sums behind dgamma / dbeta (overwritten; may be None).
    need_dy=False: the sums only, returns None.  partial [slots,2,C]: the sums were emitted by the kernel that wrote dout.
    out: the dy buffer (a channel slice of a wider one works)."""
    B, H, W, C = y.shape
    npix = B * H * W
    dy = None
    if need_dy:
        dy = out if out is not None else torch.empty((B, H, W, C), dtype=out_dtype or y.dtype, device=y.device)
    nb = int(lib.gdn_bn_frozen_bwd_workspace_bytes(npix, C))
    ws = workspace(nb, y.device, "bnbwd")
    lib.gdn_bn_frozen_bwd(_p(dout), 0 if dout is None else _ld(dout), _p(y), _ld(y), _p(coeffs[0]), _p(coeffs[1]), _p(coeffs[2]), _p(coeffs[3]),
                          _p(dy), 0 if dy is None else _ld(dy), _p(dgamma), _p(dbeta), npix, C, 1 if relu else 0,
                          _p(partial), 0 if partial is None else partial.shape[0], _p(ws), nb, _mask(dout, y, dy), stream())
    return dy


def upsample2x(x, align_corners=False):
    B, H, W, C = x.shape
    if not x.is_contiguous():
        raise GdnError("upsample2x needs a dense NHWC tensor")
    y = torch.empty((B, 2 * H, 2 * W, C), dtype=x.dtype, device=x.device)
    lib.gdn_upsample2x_fwd(_p(x), _p(y), B, H, W, C, 1 if align_corners else 0, _mask(x, y), stream())
    return y


def bn_apply_up2x(y, scale, shift, relu, residual, align_corners=False, out_dtype=None, need_low=True):
    """(low, up): low = [relu](y * scale + shift) (+ residual) and up = its x2 bilinear upsampling, one pass (gdn_bn_apply_up2x);
    low is None when need_low is False."""
    B, H, W, C = y.shape
    if not y.is_contiguous() or (residual is not None and not residual.is_contiguous()):
        raise GdnError("bn_apply_up2x needs dense NHWC tensors")
    odt = out_dtype or y.dtype
    low = torch.empty((B, H, W, C), dtype=odt, device=y.device) if need_low else None
    up = torch.empty((B, 2 * H, 2 * W, C), dtype=odt, device=y.device)
    dt = _mask(y, residual, up, up)              # (low is stored in up's type, also when it is not written)
    lib.gdn_bn_apply_up2x(_p(y), _p(scale), _p(shift), _p(residual), _p(low), _p(up), B, H, W, C, 1 if relu else 0,
                          1 if align_corners else 0, dt, stream())
    return low, up


def upsample2x_bwd(dy, align_corners=False):
    B, H2, W2, C = dy.shape
    if not dy.is_contiguous():
        raise GdnError("upsample2x_bwd needs a dense NHWC tensor")
    dx = torch.empty((B, H2 // 2, W2 // 2, C), dtype=dy.dtype, device=dy.device)
    lib.gdn_upsample2x_bwd(_p(dy), _p(dx), B, H2 // 2, W2 // 2, C, 1 if align_corners else 0, _mask(dy, dx), stream())
    return dx


def nchw_to_nhwc(x, dtype=None):
    B, C, H, W = x.shape
    y = torch.empty((B, H, W, C), dtype=dtype or x.dtype, device=x.device)
    lib.gdn_nchw_to_nhwc(_p(x), _p(y), B, C, H, W, _mask(x, y), stream())
    return y


def nhwc_to_nchw(x, dtype=None):
    B, H, W, C = x.shape
    y = torch.empty((B, C, H, W), dtype=dtype or x.dtype, device=x.device)
    lib.gdn_nhwc_to_nchw(_p(x), _p(y), B, C, H, W, _mask(x, y), stream())
    return y


def add(a, b, out_dtype=None):
    if not (a.is_contiguous() and b.is_contiguous()):
        raise GdnError("add needs dense tensors")
    o = torch.empty(a.shape, dtype=out_dtype or a.dtype, device=a.device)
    lib.gdn_add(_p(a), _p(b), _p(o), a.numel(), _mask(a, b, o), stream())
    return o


def add_pitched(a, b=None, out_dtype=None):
    """Dense a (+ b) of [B,H,W,C] tensors that may be channel slices of wider ones (b None: compacting copy)."""
    B, H, W, C = a.shape
    o = torch.empty((B, H, W, C), dtype=out_dtype or a.dtype, device=a.device)
    lib.gdn_add_pitched(_p(a), _ld(a), _p(b), 0 if b is None else _ld(b), _p(o), C, B * H * W, C, _mask(a, b, o), stream())
    return o


def copy_rows(src, dst):
    """dst[...] = src for two dense fp32 tensors of equal size whose last dimension is a multiple of 4 (gdn_add_pitched as a copy)."""
    n = src.numel()
    w = src.shape[-1]
    lib.gdn_add_pitched(_p(src), w, None, 0, _p(dst), w, n // w, w, 0, stream())
    return dst


def scale_dev(x, s):
    """x * s with s a 0-dim device tensor (no host sync, no torch kernel)."""
    o = torch.empty_like(x)
    lib.gdn_scale_dev(_p(x), _p(s), _p(o), x.numel(), stream())
    return o


def tanh_bwd(dout, out):
    r = torch.empty_like(out)
    lib.gdn_tanh_bwd(_p(dout), _p(out), _p(r), out.numel(), stream())
    return r


def fill_(t, value):
    lib.gdn_fill(_p(t), float(value), t.numel(), stream())
    return t


def zeros(shape, device):
    return fill_(torch.empty(shape, dtype=torch.float32, device=device), 0.0)


def _loss_ws(npix, device):
    nb = int(lib.gdn_loss_workspace_bytes(npix))
    return workspace(nb, device, "loss"), nb


def absdiff_max(a, b):
    """max|a-b| as a device scalar (the BerHu threshold's maximum; all-reduce it for --global_berhu)."""
    m = torch.empty((), dtype=torch.float32, device=a.device)
    lib.gdn_absdiff_max(_p(a), _p(b), a.numel(), _p(m), stream())
    return m


def berhu_masked(out, gt, sparse, box, dout, loss, ext_max=None):
    """out/gt [B,1,H,W]; sparse [B,Cs,H,W] or None; adds the gradient into dout; writes loss[()]."""
    B, _, H, W = out.shape
    ws, nb = _loss_ws(B * H * W, out.device)
    cbox = (ctypes.c_int32 * 4)(*box) if box is not None else None
    lib.gdn_berhu_masked(_p(out), _p(gt), _p(sparse), 0 if sparse is None else sparse.shape[1], B, H, W, cbox,
                         _p(ext_max), _p(loss), _p(dout), _p(ws), nb, stream())


def silog_masked(out, gt, sparse, box, dout, loss, lam, weight, floor, stats=None):
    """Scale-invariant log loss (gdn_silog_masked): out/gt [B,1,H,W]; sparse [B,Cs,H,W] with its box, or None = every pixel
    whose ground truth is above the floor; adds the gradient into dout (None: value only); writes loss[()] and, when given,
    stats = (n, m1, m2, D) into a float64 device tensor of 4."""
    B, _, H, W = out.shape
    ws, nb = _loss_ws(B * H * W, out.device)
    cbox = (ctypes.c_int32 * 4)(*box) if box is not None else None
    if stats is not None and (stats.dtype != torch.float64 or stats.numel() != 4 or not stats.is_contiguous()):
        raise GdnError("silog_masked: stats must be a dense float64 tensor of 4")
    lib.gdn_silog_masked(_p(out), _p(gt), _p(sparse), 0 if sparse is None else sparse.shape[1], B, H, W, cbox,
                         float(lam), float(weight), float(floor), _p(loss), _p(dout), _p(stats), _p(ws), nb, stream())


def sobel_l1(pred, gt, weight, dpred, loss, plus=None, total=None):
    """total (0-dim device tensor) = loss + plus: the step's loss sum comes out of the same kernel."""
    B, _, H, W = pred.shape
    ws, nb = _loss_ws(B * H * W, pred.device)
    lib.gdn_sobel_l1(_p(pred), _p(gt), B, H, W, float(weight), _p(loss), _p(dpred), _p(plus), _p(total), _p(ws), nb, stream())


def smoothness(depth, img, ddepth, loss, plus=None, plus2=None, total=None):
    B, _, H, W = depth.shape
    ws, nb = _loss_ws(B * H * W, depth.device)
    lib.gdn_smoothness(_p(depth), _p(img), img.shape[1], B, H, W, _p(loss), _p(ddepth), _p(plus), _p(plus2), _p(total),
                       _p(ws), nb, stream())


def mse_accum(a, b, weight, loss, accumulate):
    ws, nb = _loss_ws(0, a.device)
    lib.gdn_mse(_p(a), _p(b), a.numel(), float(weight), 1 if accumulate else 0, _p(loss), _p(ws), nb, _mask(a, b), stream())


def mse_grad(a, b, weight, gscale, out_dtype=None):
    """d/da of weight*mean((a-b)^2), times the device scalar gscale (or None)."""
    da = torch.empty_like(a, dtype=out_dtype or a.dtype)       # preserves a's (dense) memory order
    if da.stride() != a.stride():
        raise GdnError("mse_grad needs a dense tensor")
    lib.gdn_mse_grad(_p(a), _p(b), a.numel(), float(weight), _p(gscale), _p(da), _mask(a, b, da), stream())
    return da


def depth_metrics(gt_sparse, gt, pred, crop=True):
    B, _, H, W = pred.shape
    nb = int(lib.gdn_depth_metrics_workspace_bytes(B, H, W))
    ws = workspace(nb, pred.device, "metrics")
    err = torch.empty(8, dtype=torch.float32, device=pred.device)
    lib.gdn_depth_metrics(_p(gt_sparse), _p(gt), _p(pred), B, H, W, 1 if crop else 0, _p(err), _p(ws), nb, stream())
    return err


def depth_metrics_nyu(gt, pred, crop=True):
    """compute_errors_NYU on [B,1,H,W] float32 device tensors -> device [8] batch means (no sync)."""
    B, _, H, W = pred.shape
    nb = int(lib.gdn_depth_metrics_nyu_workspace_bytes(B, H, W))
    ws = workspace(nb, pred.device, "metrics")
    err = torch.empty(8, dtype=torch.float32, device=pred.device)
    lib.gdn_depth_metrics_nyu(_p(gt), _p(pred), B, H, W, 1 if crop else 0, _p(err), _p(ws), nb, stream())
    return err


def depth_metrics_make3d(gt_np, gt, pred):
    """compute_errors_Make3D on [B,1,H,W] float32 device tensors -> device [4] batch means (no sync)."""
    B, _, H, W = pred.shape
    nb = int(lib.gdn_depth_metrics_make3d_workspace_bytes(B, H, W))
    ws = workspace(nb, pred.device, "metrics")
    err = torch.empty(4, dtype=torch.float32, device=pred.device)
    lib.gdn_depth_metrics_make3d(_p(gt_np), _p(gt), _p(pred), B, H, W, _p(err), _p(ws), nb, stream())
    return err


GT_METRES, GT_U16, GT_UNIT = 0, 1, 2        # gt_kind of gdn_depth_metrics_std


def depth_metrics_std(gt, gt_kind, boxes, pred, depth_scale=80.0, min_depth=1e-3, max_depth=80.0, median_scaling=False):
    """gdn_depth_metrics_std: gt [B,Hmax,Wmax] (float32 for kind 0 / 2, uint16 for kind 1), boxes int32 [B,6] =
    (h0, w0, y1, y2, x1, x2) and pred [B,1,H,W] float32, all dense and on the GPU -> device float64 [B,12] =
    (n, ratio, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, log10, silog, 0) per image.  No sync."""
    want = torch.uint16 if gt_kind == GT_U16 else torch.float32
    if gt_kind not in (GT_METRES, GT_U16, GT_UNIT):
        raise GdnError("depth_metrics_std: gt_kind %r is not 0 (metres), 1 (uint16 / 256) or 2 ([-1, 1])" % (gt_kind,))
    if not (gt.is_cuda and gt.dim() == 3 and gt.dtype == want and gt.is_contiguous()):
        raise GdnError("depth_metrics_std: gt of kind %d must be a dense [B,Hmax,Wmax] %s tensor on the GPU" % (gt_kind, want))
    if not (pred.is_cuda and pred.dim() == 4 and pred.shape[1] == 1 and pred.dtype == torch.float32 and pred.is_contiguous()):
        raise GdnError("depth_metrics_std: pred must be a dense [B,1,H,W] float32 tensor on the GPU")
    B, _, H, W = pred.shape
    if gt.shape[0] != B or not (boxes.is_cuda and boxes.dtype == torch.int32 and tuple(boxes.shape) == (B, 6) and
                                boxes.is_contiguous()):
        raise GdnError("depth_metrics_std: gt and boxes (int32 [B,6] on the GPU) must hold pred's %d images" % B)
    Hmax, Wmax = gt.shape[1], gt.shape[2]
    nb = int(lib.gdn_depth_metrics_std_workspace_bytes(B, Hmax, Wmax))
    ws = workspace(nb, pred.device, "metrics_std")
    rows = torch.empty((B, 12), dtype=torch.float64, device=pred.device)
    lib.gdn_depth_metrics_std(_p(gt), int(gt_kind), Hmax, Wmax, _p(boxes), _p(pred), B, H, W, float(depth_scale),
                              float(min_depth), float(max_depth), 1 if median_scaling else 0, _p(rows), _p(ws), nb, stream())
    return rows


def _flip_rows(what, *ts):
    a = ts[0]
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() >= 1 and t.shape == a.shape):
            raise GdnError("%s: dense float32 tensors of one shape on the GPU" % what)
    W = a.shape[-1]
    return a.numel() // W, W


def flip_w(src):
    """src[..., ::-1] of a dense float32 device tensor (gdn_flip_w), as a new tensor."""
    rows, W = _flip_rows("flip_w", src)
    dst = torch.empty_like(src)
    lib.gdn_flip_w(_p(src), rows, W, _p(dst), stream())
    return dst


def flip_mean(a, b, out=None):
    """(a + b.flip(-1)) * 0.5 bitwise (gdn_flip_mean): the merge of the flip test-time augmentation.  out: a new tensor, or
    a itself."""
    out = torch.empty_like(a) if out is None else out
    rows, W = _flip_rows("flip_mean", a, b, out)
    if out.data_ptr() == b.data_ptr():
        raise GdnError("flip_mean: out may be a, not b")
    lib.gdn_flip_mean(_p(a), _p(b), rows, W, _p(out), stream())
    return out


VELO_DEPTHS = {'camera': 0, 'forward': 1}   # depth_kind of gdn_velo_project


def velo_project(points, offsets, proj, sizes, Hmax, Wmax, depth='camera', hits=False, max_points=None):
    """gdn_velo_project: points float32 [N,4] (the scans of B images, one after the other), offsets int64 [B+1], proj
    float64 [B,12] (or [B,3,4]) and sizes int32 [B,2] = (h0, w0), all dense and on the GPU -> float32 [B,Hmax,Wmax] metres
    (0 where no point lands, and in the padding), and with hits=True also int32 [B], the > 0 pixels of each image.
    depth: 'camera' (along the optical axis) or 'forward' (the scanner's x).  max_points: at least the largest scan (it
    sizes the grid; when not given: N).  No sync, nothing is read on the host."""
    if depth not in VELO_DEPTHS:
        raise GdnError("velo_project: depth %r is not one of camera / forward" % (depth,))
    if not (points.is_cuda and points.dim() == 2 and points.shape[1] == 4 and points.dtype == torch.float32 and
            points.is_contiguous()):
        raise GdnError("velo_project: points must be a dense [N,4] float32 tensor on the GPU")
    if not (offsets.is_cuda and offsets.dim() == 1 and offsets.dtype == torch.int64 and offsets.is_contiguous() and
            offsets.numel() >= 2):
        raise GdnError("velo_project: offsets must be a dense int64 [B+1] tensor on the GPU")
    B = offsets.numel() - 1
    if not (proj.is_cuda and proj.dtype == torch.float64 and proj.is_contiguous() and proj.numel() == 12 * B and
            proj.shape[0] == B):
        raise GdnError("velo_project: proj must be a dense float64 [B,12] tensor on the GPU for the %d images of offsets" % B)
    if not (sizes.is_cuda and sizes.dtype == torch.int32 and sizes.is_contiguous() and tuple(sizes.shape) == (B, 2)):
        raise GdnError("velo_project: sizes must be a dense int32 [B,2] tensor on the GPU for the %d images of offsets" % B)
    Hmax, Wmax = int(Hmax), int(Wmax)
    if Hmax < 1 or Wmax < 1:
        raise GdnError("velo_project: a pool of %d x %d" % (Hmax, Wmax))
    n = int(points.shape[0]) if max_points is None else int(max_points)
    out = torch.empty((B, Hmax, Wmax), dtype=torch.float32, device=points.device)
    count = torch.empty((B,), dtype=torch.int32, device=points.device) if hits else None
    lib.gdn_velo_project(_p(points) if points.shape[0] else None, _p(offsets), _p(proj), _p(sizes), B, n, Hmax, Wmax,
                         VELO_DEPTHS[depth], _p(out), _p(count) if hits else None, stream())
    return (out, count) if hits else out


def depth_densify(pool, sizes, max_depth=100.0, out=None):
    """gdn_depth_densify: pool float32 [B,Hmax,Wmax] metres (0 = no return; what velo_project returns) and sizes int32 [B,2]
    = (h0, w0), dense and on the GPU -> the dense maps in a float32 pool of the same shape, the padding +0 (DESIGN.md
    3.16).  out: a pool of that shape to write into (not the input), or None for a new one.  No sync, nothing is read on
    the host."""
    if not (pool.is_cuda and pool.dim() == 3 and pool.dtype == torch.float32 and pool.is_contiguous() and pool.numel() > 0):
        raise GdnError("depth_densify: pool must be a dense [B,Hmax,Wmax] float32 tensor on the GPU")
    B, Hmax, Wmax = (int(v) for v in pool.shape)
    if not (sizes.is_cuda and sizes.dtype == torch.int32 and sizes.is_contiguous() and tuple(sizes.shape) == (B, 2)):
        raise GdnError("depth_densify: sizes must be a dense int32 [B,2] tensor on the GPU for the %d images of the pool" % B)
    max_depth = float(max_depth)
    if not (0.2 < max_depth < float("inf")):
        raise GdnError("depth_densify: max_depth %r is not a finite number above 0.2" % (max_depth,))
    if out is None:
        out = torch.empty_like(pool)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == pool.shape and
              out.device == pool.device and out.data_ptr() != pool.data_ptr()):
        raise GdnError("depth_densify: out must be another dense float32 tensor of the pool's shape on its device")
    nb = int(lib.gdn_depth_densify_workspace_bytes(B, Hmax, Wmax))
    ws = workspace(nb, pool.device, "densify")
    lib.gdn_depth_densify(_p(pool), _p(sizes), B, Hmax, Wmax, max_depth, _p(out), _p(ws), nb, stream())
    return out


def depth_encode_u8(x, scale=80.0, keep_valid=False):
    """gdn_depth_encode_u8: a dense float32 device tensor of metres -> uint8 of the same shape, rint(clamp(x, 0, scale) /
    scale * 255) in double, half to even, NaN -> 0; keep_valid: an x > 0 that rounds to 0 becomes 1 (the sparse map, where
    byte 0 means no LiDAR return)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0):
        raise GdnError("depth_encode_u8: x must be a dense, non-empty float32 tensor on the GPU")
    scale = float(scale)
    if not (0.0 < scale < float("inf")):
        raise GdnError("depth_encode_u8: scale %r is not a finite positive number" % (scale,))
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    lib.gdn_depth_encode_u8(_p(x), x.numel(), scale, 1 if keep_valid else 0, _p(out), stream())
    return out


def center_crop_offsets(in_h, in_w, out_h, out_w):
    """CenterCrop.get_params (transform_list.py:260-261): Python's round, i.e. half to even."""
    return int(round((in_h - out_h) / 2.)), int(round((in_w - out_w) / 2.))


def crop_normalize(src, H, W, offsets=None):
    """src [B,H0,W0,C] uint8/float32 as decoded, on the device -> [B,C,H,W] float32 (v/255 - 0.5)/0.5 of the window at
    `offsets` (default: the centre crop).  Float sources are not bytescaled (the NYU validation transform has no imresize)."""
    if not src.is_cuda or src.dtype not in (torch.uint8, torch.float32) or src.dim() != 4 or not src.is_contiguous():
        raise GdnError("crop_normalize: src must be a dense [B,H,W,C] uint8/float32 tensor on the GPU")
    B, H0, W0, C = src.shape
    oy, ox = center_crop_offsets(H0, W0, H, W) if offsets is None else offsets
    if not (0 <= oy and oy + H <= H0 and 0 <= ox and ox + W <= W0):
        raise GdnError("crop_normalize: window %dx%d at (%d, %d) does not fit a %dx%d image" % (H, W, oy, ox, H0, W0))
    dst = torch.empty((B, C, H, W), dtype=torch.float32, device=src.device)
    lib.gdn_crop_normalize(_p(src), 1 if src.dtype == torch.float32 else 0, B, H0, W0, C, int(oy), int(ox), H, W,
                           _p(dst), stream())
    return dst


def bytescale_u8(x):
    """[B,C,H,W] float32 device tensor -> [B,H,W,C] uint8 as scipy.misc.imsave bytescales an image (per image, fp64)."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise GdnError("bytescale_u8: x must be a [B,C,H,W] float32 tensor on the GPU")
    x = x.contiguous()
    B, C, H, W = x.shape
    dst = torch.empty((B, H, W, C), dtype=torch.uint8, device=x.device)
    lib.gdn_bytescale_u8(_p(x), B, C, H, W, _p(dst), stream())
    return dst


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    lib.gdn_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, int(step),
                      float(grad_scale), stream())


def _check_out(what, out, shape, device):
    """A caller-owned output: a dense float32 tensor of exactly the shape and device the kernel writes."""
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != tuple(shape) or \
            out.device != device or not out.is_contiguous():
        raise GdnError("%s: out must be a dense float32 %s tensor on %s, got %s" %
                       (what, tuple(shape), device, "%s %s on %s" % (out.dtype, tuple(out.shape), out.device)
                        if isinstance(out, torch.Tensor) else type(out).__name__))
    return out


def kitti_augment(src, params, train=True, out=None):
    """src [B,H,W,C] uint8/float32 as decoded; params int32 [B,5] on the device (or None when not train).
    Returns the normalised NCHW float32 batch: a new tensor, or `out` (dense float32 [B,C,H,W] on src's device, checked)."""
    if not src.is_cuda or src.dtype not in (torch.uint8, torch.float32) or src.dim() != 4 or not src.is_contiguous():
        raise GdnError("kitti_augment: src must be a dense [B,H,W,C] uint8/float32 tensor on the GPU")
    B, H, W, C = src.shape
    if train and (params is None or params.dtype != torch.int32 or tuple(params.shape) != (B, 5) or not params.is_cuda):
        raise GdnError("kitti_augment: params must be a device int32 [B,5] tensor")
    if out is None:
        dst = torch.empty((B, C, H, W), dtype=torch.float32, device=src.device)
    else:
        dst = _check_out("kitti_augment", out, (B, C, H, W), src.device)
    nb = int(lib.gdn_kitti_augment_workspace_bytes(B))
    ws = workspace(nb, src.device, "augment")
    lib.gdn_kitti_augment(_p(src), 1 if src.dtype == torch.float32 else 0, B, H, W, C, _p(params), 1 if train else 0,
                          _p(dst), _p(ws), nb, stream())
    return dst


def check_sel(rows, n, H, W, train=True):
    """Host-side check of batch-assembly rows before they are uploaded (the device does not check): `rows` is an integer
    [B,6] array {sample index, flip, scaled_h, scaled_w, off_y, off_x}; every index must address one of the n resident
    samples and, for training, the draws must describe a crop window inside the scaled image.  Returns int32 rows."""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    if rows.ndim != 2 or rows.shape[1] != 6 or rows.shape[0] == 0:
        raise GdnError("check_sel: rows must be a non-empty [B,6] integer array, got shape %s" % (rows.shape,))
    idx = rows[:, 0]
    if int(idx.min()) < 0 or int(idx.max()) >= n:
        raise GdnError("check_sel: sample index %d is outside the %d resident samples" %
                       (int(idx.min()) if idx.min() < 0 else int(idx.max()), n))
    if train:
        flip, sh, sw, oy, ox = (rows[:, k] for k in range(1, 6))
        ok = ((flip == 0) | (flip == 1)) & (sh >= H) & (sw >= W) & (oy >= 0) & (oy <= sh - H) & (ox >= 0) & (ox <= sw - W)
        if not ok.all():
            b = int(np.argmin(ok))
            raise GdnError("check_sel: row %d %s is not a flip / scale-up / crop of a %dx%d image" % (b, rows[b, 1:].tolist(), H, W))
    return rows


def kitti_augment_resident(pools, sel, train=True, out=None):
    """Assemble a batch from device-resident pools in one launch: pools = (gt, rgb, sparse), dense uint8 [N,H,W,C] device
    tensors of one N, H, W; sel = int32 [B,6] {sample index, flip, scaled_h, scaled_w, off_y, off_x} -- a device tensor
    whose rows the caller has passed through check_sel, or a host array / CPU tensor, checked and copied here.
    Returns the three normalised NCHW float32 tensors (bit-identical to kitti_augment on the gathered samples): new ones, or
    the three of `out` (dense float32 [B,C,H,W] each on the pools' device, checked)."""
    if len(pools) != 3 or any(not isinstance(p, torch.Tensor) or not p.is_cuda or p.dtype != torch.uint8 or p.dim() != 4 or
                              not p.is_contiguous() or not 1 <= p.shape[3] <= 4 for p in pools):
        raise GdnError("kitti_augment_resident: pools must be three dense [N,H,W,C<=4] uint8 tensors on the GPU")
    N, H, W = pools[0].shape[:3]
    if N == 0 or any(tuple(p.shape[:3]) != (N, H, W) or p.device != pools[0].device for p in pools):
        raise GdnError("kitti_augment_resident: the pools must hold the same samples at one size on one device, got %s" %
                       ([tuple(p.shape) for p in pools],))
    dev = pools[0].device
    if not (isinstance(sel, torch.Tensor) and sel.is_cuda):
        host = check_sel(sel.numpy() if isinstance(sel, torch.Tensor) else sel, N, H, W, train)
        sel = torch.from_numpy(host).to(dev)
    if sel.dtype != torch.int32 or sel.dim() != 2 or sel.shape[1] != 6 or sel.shape[0] == 0 or not sel.is_contiguous() or \
            sel.device != dev:
        raise GdnError("kitti_augment_resident: sel must be a dense int32 [B,6] tensor on the pools' device")
    B = sel.shape[0]
    if out is None:
        outs = tuple(torch.empty((B, p.shape[3], H, W), dtype=torch.float32, device=dev) for p in pools)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 3:
            raise GdnError("kitti_augment_resident: out must be three tensors (gt, rgb, sparse)")
        outs = tuple(_check_out("kitti_augment_resident", o, (B, p.shape[3], H, W), dev) for o, p in zip(out, pools))
        if len({o.data_ptr() for o in outs}) != 3:
            raise GdnError("kitti_augment_resident: the three out tensors must be distinct")
    lib.gdn_kitti_augment_resident(_p(pools[0]), pools[0].shape[3], _p(pools[1]), pools[1].shape[3], _p(pools[2]),
                                   pools[2].shape[3], H, W, _p(sel), B, 1 if train else 0, _p(outs[0]), _p(outs[1]),
                                   _p(outs[2]), stream())
    return outs


def gather_samples(pool, idx, to_f32=False):
    """pool[idx] for a dense uint8 / uint16 device pool [N, ...]: idx is an int32 [B] device tensor the caller has
    range-checked, or a host array / CPU tensor / list, checked and copied here.  to_f32 (uint16 pools): the result is
    float32, every value widened exactly.  Returns [B, ...]."""
    if not isinstance(pool, torch.Tensor) or not pool.is_cuda or pool.dtype not in (torch.uint8, torch.uint16) or \
            pool.dim() < 1 or not pool.is_contiguous() or pool.shape[0] == 0:
        raise GdnError("gather_samples: pool must be a dense uint8/uint16 [N,...] tensor on the GPU")
    if to_f32 and pool.dtype != torch.uint16:
        raise GdnError("gather_samples: to_f32 widens uint16 pools only, got %s" % (pool.dtype,))
    N = pool.shape[0]
    if not (isinstance(idx, torch.Tensor) and idx.is_cuda):
        host = np.ascontiguousarray(idx.numpy() if isinstance(idx, torch.Tensor) else idx)
        if host.ndim != 1 or host.size == 0 or host.dtype.kind not in "iu":
            raise GdnError("gather_samples: idx must be a non-empty 1-D integer array")
        if int(host.min()) < 0 or int(host.max()) >= N:
            raise GdnError("gather_samples: index outside the %d resident samples" % N)
        idx = torch.from_numpy(host.astype(np.int32)).to(pool.device)
    if idx.dtype != torch.int32 or idx.dim() != 1 or idx.numel() == 0 or not idx.is_contiguous() or idx.device != pool.device:
        raise GdnError("gather_samples: idx must be a dense int32 [B] tensor on the pool's device")
    B = idx.numel()
    per_sample = pool[0].numel()
    if per_sample == 0:
        raise GdnError("gather_samples: empty samples")
    dst = torch.empty((B,) + tuple(pool.shape[1:]), dtype=torch.float32 if to_f32 else pool.dtype, device=pool.device)
    lib.gdn_gather_samples(_p(pool), pool.element_size(), _p(idx), B, per_sample, 1 if to_f32 else 0, _p(dst), stream())
    return dst


NYU_CROP = (251, 340)          # RandomCropNumpy's window (GDN_main.py:99, :110)

# gdn_nyu_aug_params (include/gdn_hip.h)
NYU_PARAMS_DTYPE = np.dtype([("h1", "<i4"), ("w1", "<i4"), ("y1", "<i4"), ("x1", "<i4"), ("h2", "<i4"), ("w2", "<i4"),
                             ("cy", "<i4"), ("cx", "<i4"), ("flip", "<i4"), ("reserved", "<i4"), ("scale", "<f8"),
                             ("mult", "<f8"), ("m", "<f8", (4,)), ("off", "<f8", (2,)), ("zn1", "<f8", (2,))])
assert NYU_PARAMS_DTYPE.itemsize == 120


def spline_z_pow(n):
    """z**n for the cubic B-spline pole z = sqrt(3) - 2, as the running product the device uses."""
    z, p = math.sqrt(3.0) - 2.0, 1.0
    for _ in range(n):
        p = p * z
    return p


def rotate_matrix(angle, n0, n1):
    """(matrix [4], offset [2]) that scipy.ndimage.rotate(reshape=False, axes=(0, 1)) computes for an n0 x n1 plane:
    cosdg / sindg of the angle in degrees, and the offset that keeps the centre in place."""
    try:
        from scipy import special
    except ImportError as e:
        raise GdnError("rotate_matrix: scipy.special (cosdg / sindg) is required to reproduce scipy.ndimage.rotate") from e
    c, s = special.cosdg(angle), special.sindg(angle)
    rot = np.array([[c, s], [-s, c]])
    shape = np.array([n0, n1])
    out_center = rot @ ((shape - 1) / 2)
    in_center = (shape - 1) / 2
    offset = in_center - out_center
    return [float(v) for v in rot.ravel()], [float(v) for v in offset]


def nyu_params(draws, H, W, mode):
    """The per-sample gdn_nyu_aug_params (host numpy array) of draws made by datasets.draw_params_nyu."""
    ch, cw = NYU_CROP
    p = np.zeros(len(draws), NYU_PARAMS_DTYPE)
    for b, d in enumerate(draws):
        w2, h2 = (np.array([cw, ch]) * d["scale"]).astype(int)     # imresize(a, scale): (array(im.size) * scale).astype(int)
        h1, w1, y1, x1 = (int(d[k]) for k in ("h1", "w1", "y1", "x1"))
        if not (h1 >= ch and w1 >= cw and 0 <= y1 <= h1 - ch and 0 <= x1 <= w1 - cw and h2 >= ch and w2 >= cw):
            raise GdnError("nyu_params: sample %d: inconsistent draws %s" % (b, d))
        cy, cx = center_crop_offsets(ch, cw, H, W) if mode == "DtoD" else center_crop_offsets(int(h2), int(w2), H, W)
        m, off = rotate_matrix(d["angle"], ch, cw)
        p[b] = (h1, w1, y1, x1, h2, w2, cy, cx, 1 if d["flip"] else 0, 0, d["scale"], d.get("mult", 1.0), m, off,
                (spline_z_pow(ch - 1), spline_z_pow(cw - 1)))
    return p


def nyu_augment(depth, rgb, draws, H, W, mode):
    """The NYU training transform (GDN_main.py:94-129) of a batch on the device.
    depth [B,H0,W0] or [B,H0,W0,1] float32, rgb [B,H0,W0,3] uint8, both on the GPU; draws: one dict per sample from
    datasets.draw_params_nyu, or those draws already packed by nyu_params and copied to the device (a uint8 tensor).
    Returns (depth [B,1,H,W], rgb [B,3,H,W]) float32, normalised."""
    if mode not in ("DtoD", "RtoD"):
        raise GdnError("nyu_augment: mode must be DtoD or RtoD, got %r" % (mode,))
    if depth.dim() == 4 and depth.shape[3] == 1:
        depth = depth[..., 0]
    if not (depth.is_cuda and rgb.is_cuda and depth.dtype == torch.float32 and rgb.dtype == torch.uint8 and
            depth.dim() == 3 and rgb.dim() == 4 and rgb.shape[3] == 3 and tuple(rgb.shape[:3]) == tuple(depth.shape)):
        raise GdnError("nyu_augment: depth must be [B,H0,W0] float32 and rgb [B,H0,W0,3] uint8, on the GPU")
    B, H0, W0 = depth.shape
    if not (0 < H <= NYU_CROP[0] and 0 < W <= NYU_CROP[1]):
        raise GdnError("nyu_augment: output %dx%d must fit the %dx%d crop" % ((H, W) + NYU_CROP))
    if isinstance(draws, torch.Tensor):
        if not (draws.is_cuda and draws.dtype == torch.uint8 and draws.numel() == B * NYU_PARAMS_DTYPE.itemsize):
            raise GdnError("nyu_augment: packed params must be a device uint8 tensor of %d bytes" %
                           (B * NYU_PARAMS_DTYPE.itemsize))
        params = draws.contiguous()
    else:
        if len(draws) != B:
            raise GdnError("nyu_augment: %d draws for a batch of %d" % (len(draws), B))
        host = torch.from_numpy(nyu_params(draws, H, W, mode).view(np.uint8))
        params = host.pin_memory().to(depth.device, non_blocking=True)
    depth, rgb = depth.contiguous(), rgb.contiguous()
    d_out = torch.empty((B, 1, H, W), dtype=torch.float32, device=depth.device)
    c_out = torch.empty((B, 3, H, W), dtype=torch.float32, device=depth.device)
    rtod = 1 if mode == "RtoD" else 0
    nb = int(lib.gdn_nyu_augment_workspace_bytes(B, H0, W0, rtod))
    ws = workspace(nb, depth.device, "nyu_augment")
    lib.gdn_nyu_augment(_p(depth), _p(rgb), B, H0, W0, rtod, _p(params), H, W, _p(d_out), _p(c_out), _p(ws), nb, stream())
    return d_out, c_out


def pil_resize(src, out_h, out_w, window=None, f_mode=False, bytescale=None):
    """Pillow BILINEAR resize of a [B,H0,W0,C] uint8/float32 device batch to out_h x out_w, computing only `window`
    (y, x, h, w; default the whole output).  f_mode: Pillow 'F' on float32 data; else 8 bpc, with scipy's bytescale first
    when `bytescale` (default: for float32 sources).  Returns [B,h,w,C] float32 ('F') or uint8."""
    if not src.is_cuda or src.dtype not in (torch.uint8, torch.float32) or src.dim() != 4:
        raise GdnError("pil_resize: src must be a [B,H0,W0,C] uint8/float32 tensor on the GPU")
    src = src.contiguous()
    B, H0, W0, C = src.shape
    f32 = src.dtype == torch.float32
    if bytescale is None:
        bytescale = f32 and not f_mode
    wy, wx, wh, ww = (0, 0, out_h, out_w) if window is None else window
    dst = torch.empty((B, wh, ww, C), dtype=torch.float32 if f_mode else torch.uint8, device=src.device)
    nb = int(lib.gdn_pil_resize_workspace_bytes(B, H0, C, ww))
    ws = workspace(max(nb, 1), src.device, "pil_resize")
    lib.gdn_pil_resize_bilinear(_p(src), 1 if f32 else 0, B, H0, W0, C, 1 if f_mode else 0, 1 if bytescale else 0,
                                int(out_h), int(out_w), int(wy), int(wx), int(wh), int(ww), _p(dst), _p(ws), nb, stream())
    return dst


def spline_rotate(src, angle=None, matrix=None, offset=None, clip=True):
    """scipy.ndimage.rotate(plane, angle, reshape=False, order=3, mode='constant') of every plane of a [B,C,H,W] float32
    device batch (or the affine map `matrix`, `offset` given directly); clip: to each sample's input min/max."""
    if not src.is_cuda or src.dtype != torch.float32 or src.dim() != 4:
        raise GdnError("spline_rotate: src must be a [B,C,H,W] float32 tensor on the GPU")
    src = src.contiguous()
    B, C, H, W = src.shape
    if matrix is None:
        matrix, offset = rotate_matrix(angle, H, W)
    m = (ctypes.c_double * 4)(*[float(v) for v in matrix])
    o = (ctypes.c_double * 2)(*[float(v) for v in offset])
    dst = torch.empty_like(src)
    nb = int(lib.gdn_spline_rotate3_workspace_bytes(B, C, H, W))
    ws = workspace(max(nb, 1), src.device, "spline_rotate")
    lib.gdn_spline_rotate3(_p(src), B, C, H, W, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(o, ctypes.c_void_p),
                           1 if clip else 0, _p(dst), _p(ws), nb, stream())
    return dst


def adam_step_dev(p, g, m, v, hyper, state):
    """Capturable Adam: hyper float32[6] and the 28-byte step state {double beta1^t, beta2^t; int32 t; float bc1, bc2s} (a
    uint8[28] tensor; the kernels never touch the C struct's 4 bytes of tail padding) live on the device (see
    gdn_adam_step_dev)."""
    lib.gdn_adam_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), _p(state), stream())


def grad_sumsq(g, guard, accumulate=False):
    """guard.sumsq (+)= sum of squares of the float32 buffer `g` in double, in a fixed order (see gdn_grad_sumsq); guard is
    the 32-byte device record of the gradient guard."""
    n = g.numel()
    nb = int(lib.gdn_grad_sumsq_workspace_bytes(n))
    ws = workspace(nb, g.device, "gradnorm")
    lib.gdn_grad_sumsq(_p(g), n, _p(guard), 1 if accumulate else 0, _p(ws), nb, stream())


def grad_guard_finalize(guard, hyper, max_norm=0.0, skip_nonfinite=False):
    """Norm, clipping coefficient, skip decision and counters of the guard record from its sumsq (gdn_grad_guard_finalize);
    max_norm <= 0: no clipping."""
    lib.gdn_grad_guard_finalize(_p(guard), _p(hyper), float(max_norm), 1 if skip_nonfinite else 0, stream())


def adam_step_dev_guarded(p, g, m, v, hyper, state, guard):
    """adam_step_dev under the guard record's coefficient and skip decision (gdn_adam_step_dev_guarded)."""
    lib.gdn_adam_step_dev_guarded(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), _p(state), _p(guard), stream())


def ema_update(ema, p, decay, state, guard=None):
    """ema += w_t (p - ema) with the warm-up weight of the step count in `state`, the device step state the Adam update of
    the same store has just advanced; `guard` is the record a guarded update read (a skipped step leaves ema alone), None
    after an unguarded one (gdn_ema_update)."""
    lib.gdn_ema_update(_p(ema), _p(p), p.numel(), float(decay), _p(state), _p(guard), stream())


def _seg_groups(n, chunk_map, hyper, states):
    """G of a segmented call, after the checks the library leaves to its caller: one map byte per 64-float chunk, one hyper
    row and one 32-byte step state per group.  (The map's contents are checked where it is built: optim._Plan.)"""
    if chunk_map.dtype != torch.uint8 or chunk_map.numel() * 64 != n:
        raise GdnError("segmented Adam: a chunk map of %d %s entries for %d floats" % (chunk_map.numel(), chunk_map.dtype, n))
    G = states.numel() // 32
    if states.dtype != torch.uint8 or states.numel() != 32 * G or (hyper is not None and hyper.numel() != 6 * G):
        raise GdnError("segmented Adam: %d bytes of step states beside %s hyper-parameters" %
                       (states.numel(), "no" if hyper is None else hyper.numel()))
    return G


def adam_step_seg(p, g, m, v, chunk_map, hyper, states, guard=None):
    """The capturable Adam update of every parameter group of an arena in ONE update launch: chunk_map uint8[n / 64] gives the
    group of each 64-float chunk (0xFF: skip it), hyper float32[G, 6], states uint8[G * 32]; guard None for the unguarded
    update (gdn_adam_step_seg)."""
    n = p.numel()
    G = _seg_groups(n, chunk_map, hyper, states)
    lib.gdn_adam_step_seg(_p(p), _p(g), _p(m), _p(v), n, _p(chunk_map), G, _p(hyper), _p(states), _p(guard), stream())


def grad_sumsq_seg(g, chunk_map, guard, accumulate=False):
    """grad_sumsq over the chunks of `g` that chunk_map does not skip (gdn_grad_sumsq_seg)."""
    n = g.numel()
    if chunk_map.dtype != torch.uint8 or chunk_map.numel() * 64 != n:
        raise GdnError("segmented Adam: a chunk map of %d %s entries for %d floats" % (chunk_map.numel(), chunk_map.dtype, n))
    nb = int(lib.gdn_grad_sumsq_workspace_bytes(n))
    ws = workspace(nb, g.device, "gradnorm")
    lib.gdn_grad_sumsq_seg(_p(g), n, _p(chunk_map), _p(guard), 1 if accumulate else 0, _p(ws), nb, stream())


def ema_update_seg(ema, p, chunk_map, decay, states, guard=None):
    """ema_update per chunk, with the warm-up weight of the chunk's own group's step count (gdn_ema_update_seg)."""
    n = p.numel()
    _seg_groups(n, chunk_map, None, states)
    lib.gdn_ema_update_seg(_p(ema), _p(p), n, _p(chunk_map), float(decay), _p(states), _p(guard), stream())


# Decoupled weight decay (AdamW): the four updates again, the arguments and the checks of their siblings, with
# weight_decay / hyper[4] the decoupled rate -- p -= fma(float32(lr * wd), p, adam term), the moments never see the decay.
def adamw_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    lib.gdn_adamw_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, int(step),
                       float(grad_scale), stream())


def adamw_step_dev(p, g, m, v, hyper, state):
    """adam_step_dev with decoupled weight decay (gdn_adamw_step_dev)."""
    lib.gdn_adamw_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), _p(state), stream())


def adamw_step_dev_guarded(p, g, m, v, hyper, state, guard):
    """adam_step_dev_guarded with decoupled weight decay: a skipped step does not decay (gdn_adamw_step_dev_guarded)."""
    lib.gdn_adamw_step_dev_guarded(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), _p(state), _p(guard), stream())


def adamw_step_seg(p, g, m, v, chunk_map, hyper, states, guard=None):
    """adam_step_seg with decoupled weight decay, each chunk at its own group's rate and decay; a skipped chunk does not decay
    (gdn_adamw_step_seg)."""
    n = p.numel()
    G = _seg_groups(n, chunk_map, hyper, states)
    lib.gdn_adamw_step_seg(_p(p), _p(g), _p(m), _p(v), n, _p(chunk_map), G, _p(hyper), _p(states), _p(guard), stream())


LR_SCHEDULE_KINDS = ("constant", "linear", "cosine")        # the `kind` argument of gdn_lr_schedule: 0, 1, 2


def lr_schedule(hyper, base_lr, states, kind, warmup, total, floor):
    """hyper[k][0] = float32(base_lr[k] * s(t_k)) for every group k, t_k the update count in group k's step state: warm-up
    over `warmup` updates, then constant / linear / cosine decay to `floor` at update `total` (gdn_lr_schedule).  hyper
    float32[G, 6] (or [6]), base_lr float64[G], states the 28-byte step state of a plain store (G = 1) or uint8[G * 32].
    One launch, no sync, capturable."""
    G = base_lr.numel()
    if base_lr.dtype != torch.float64 or hyper.dtype != torch.float32 or hyper.numel() != 6 * G or states.dtype != torch.uint8 \
            or states.numel() < 32 * (G - 1) + 28:
        raise GdnError("lr_schedule: %d %s base rates beside %d %s hyper-parameters and %d bytes of step states" %
                       (G, base_lr.dtype, hyper.numel(), hyper.dtype, states.numel()))
    if not (hyper.is_contiguous() and base_lr.is_contiguous() and states.is_contiguous()):
        raise GdnError("lr_schedule: hyper, base_lr and states must be dense")
    k = LR_SCHEDULE_KINDS.index(kind) if isinstance(kind, str) else int(kind)
    lib.gdn_lr_schedule(_p(hyper), _p(base_lr), _p(states), G, k, int(warmup), int(total), float(floor), stream())


def swap_(a, b):
    """Exchange the contents of two non-overlapping dense float32 buffers in place (gdn_swap_f32)."""
    lib.gdn_swap_f32(_p(a), _p(b), a.numel(), stream())


def grad_accumulate(acc, g):
    """acc += g for two non-overlapping dense float32 buffers of one size, one float32 add per element
    (gdn_grad_accumulate): the running sum of a gradient-accumulation group.  No host sync, no allocation."""
    if acc.numel() != g.numel():
        raise GdnError("grad_accumulate: %d and %d elements" % (acc.numel(), g.numel()))
    lib.gdn_grad_accumulate(_p(acc), _p(g), acc.numel(), stream())


STEP_RECORD_ROW = 64          # bytes of a ring row and of the ring's header (gdn_step_record)
STEP_RECORD_TERMS = 8         # loss terms a row holds


def step_record(ring, cap, terms, hyper=None, state=None, guard=None):
    """One row of the training log's device ring (gdn_step_record): row count % cap takes the bit patterns of the 0-dim float32
    device tensors `terms` (at most 8), the rate in hyper[0], the update count of the step state and the guard's norm,
    coefficient and skip decision -- each of the three records may be None -- and the ring's counter advances.  ring: uint8
    [64 + 64 * cap] on the device, zeroed once.  One launch, no sync, capturable."""
    n = len(terms)
    if ring.dtype != torch.uint8 or ring.numel() != STEP_RECORD_ROW * (1 + int(cap)) or not ring.is_contiguous():
        raise GdnError("step_record: a ring of %d %s elements for %d rows" % (ring.numel(), ring.dtype, cap))
    if n > STEP_RECORD_TERMS or any(t is not None and (t.dtype != torch.float32 or t.numel() != 1 or not t.is_cuda) for t in terms):
        raise GdnError("step_record: the terms must be at most %d float32 scalars on the GPU" % STEP_RECORD_TERMS)
    ptrs = (ctypes.c_void_p * STEP_RECORD_TERMS)(*[_p(t) for t in terms])
    lib.gdn_step_record(_p(ring), int(cap), ptrs, n, _p(hyper), _p(state), _p(guard), stream())


def tensor_sumsq(p, g, seg, out=None):
    """out[k] = (sum p[i]^2, sum g[i]^2) in double over segment k = seg[k] = (offset, length) of the float32 buffers p and g
    (g may be None: zeros), in a fixed order, padding between segments not read (gdn_tensor_sumsq).  seg: int64 [T, 2] on the
    device, offsets multiples of 64, ascending, inside the buffer -- the caller's to check.  Returns out, float64 [T, 2]."""
    n, T = p.numel(), seg.shape[0]
    if seg.dtype != torch.int64 or seg.dim() != 2 or seg.shape[1] != 2 or not seg.is_contiguous() or not seg.is_cuda:
        raise GdnError("tensor_sumsq: seg must be a dense int64 [T, 2] tensor on the GPU")
    if p.dtype != torch.float32 or not p.is_contiguous() or (g is not None and (g.dtype != torch.float32 or g.numel() != n or
                                                                                 not g.is_contiguous())):
        raise GdnError("tensor_sumsq: p and g must be dense float32 buffers of one size")
    if out is None:
        out = torch.empty((T, 2), dtype=torch.float64, device=p.device)
    elif out.dtype != torch.float64 or out.numel() != 2 * T or not out.is_contiguous():
        raise GdnError("tensor_sumsq: out must be a dense float64 [T, 2] tensor")
    nb = int(lib.gdn_tensor_sumsq_workspace_bytes(n, T))
    ws = workspace(nb, p.device, "tensor_sumsq")
    lib.gdn_tensor_sumsq(_p(p), _p(g), n, _p(seg), T, _p(out), _p(ws), nb, stream())
    return out
