"""Host-side execution engine: explicit forward/backward over the HIP kernels.

The reference relies on torch autograd + cuDNN for every layer.  Here each
block's forward launches the HIP kernels directly and, when gradients are
needed, pushes one closure on a tape; ``backward`` replays the tape in reverse.
Parameters keep the reference's names/shapes but live, tap-major, in one flat
arena per model (so Adam and the RCCL all-reduce see a single buffer).
"""
import collections
import functools

import torch

from . import ops
from ._lib import GdnError

_ALIGN = 64  # floats
# fp32 stride-1 zero-padded layers with a window of at least this size run in the frequency domain (csrc/conv_fft.hip):
# 5x5 on 256 channels is the break-even neighbourhood
_FFT_MIN_K = 5
# fp32 4x4 stride-2 pad-1 Conv2d / ConvTranspose2d layers run as Winograd F(3x3,2x2) over the polyphase images
# (csrc/conv_wino2.hip) when both channel counts reach this value: the transforms move ~1.8x the layer's
# activations (measured: a gain on every such layer of G, the smallest at 64 channels, tests/diag/wino2_time.py)
_WINO2_MIN_C = 64
# window sizes of the stride-1 ConvTranspose2d layers that train in a transform domain as flipped-tap convolutions (_flip_op):
# the three the legacy AutoEncoder has, each measured against the direct kernels (tests/diag/legacy_layer_time.py, DESIGN.md
# 2.16).  The kernels also take 9x9; no network here has such a layer, so it is not measured and not selected.
_FLIP_TAPS_K = (3, 5, 7)
# The three fusions below are on; the tests switch them off to compare against the unfused form, which is also what a
# layer that cannot fuse runs.
# train-mode BatchNorm: scale/shift/ReLU of a ResidualBlock's first half applied in the consumer's loader, BatchNorm-backward
# reductions emitted by the data-gradient epilogues
_FUSE_TRAIN_BN = True
# No backward work below the lowest trainable layer (Ctx.is_live).  False: every activation counts as live, the
# backward of a partly frozen network runs as it did before -- the A/B switch of tests/test_hip_partial_finetune.py.
_PRUNE_FROZEN = True
# x2 bilinear upsampling folded into the consumer convolution's loader and its backward's fold pass (north_star "bilinear-interp
# ... fused"; csrc/up2x.h)
_FUSE_UP2X = True
# bf16 form of the same fusion (round 5, row N1): LDS-DMA operands cannot be interpolated on load, so the PRODUCER writes the
# upsampled tensor -- BatchNorm-apply (+ residual) and the interpolation are one pass (gdn_bn_apply_up2x) -- and the consumer's
# reflection fold applies the adjoint (gdn_conv_dgrad dx_up2x): no stand-alone upsample2x kernel in either direction
_FUSE_UP2X_BF16 = True
_GRAPH_EPOCH = 0


def bump_graph_epoch():
    """A graph replay changed parameters / BN buffers without touching torch's version counters: drop derived caches."""
    global _GRAPH_EPOCH
    _GRAPH_EPOCH += 1


# ----------------------------------------------------------------------------
# Parameter layout: logical torch shape, physical tap-major [kh*kw, Cout, Cin]
# ----------------------------------------------------------------------------
def _perm(transposed):
    # logical -> physical permutation and its inverse
    return ((2, 3, 1, 0), (3, 2, 0, 1)) if transposed else ((2, 3, 0, 1), (2, 3, 0, 1))


def tap_view(t, transposed):
    """[kh*kw, Cout, Cin] view of a conv weight (or its grad) stored tap-major; None if it is not."""
    fwd, _ = _perm(transposed)
    v = t.permute(*fwd)
    if not v.is_contiguous():
        return None
    kh, kw, co, ci = v.shape
    return v.view(kh * kw, co, ci)


class ParamArena:
    """Flat fp32 storage for all parameters of a model (+ a matching gradient arena)."""

    def __init__(self, module, device):
        self.items = []      # (param, offset, numel, transposed or None)
        convt = {id(m.weight) for m in module.modules() if isinstance(m, torch.nn.ConvTranspose2d)}
        off = 0
        for p in module.parameters():
            tr = None
            if p.dim() == 4:
                tr = id(p) in convt
            self.items.append((p, off, p.numel(), tr))
            off += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.numel = off
        self._slot = {id(p): (o, tr) for p, o, _, tr in self.items}      # (items keeps every parameter alive: the ids stay its own)
        self.device = device
        self.data = torch.zeros(off, dtype=torch.float32, device=device)
        self.grad = torch.zeros(off, dtype=torch.float32, device=device)
        for p, o, n, tr in self.items:
            src = p.data.to(device=device, dtype=torch.float32)
            p.data = self._view(self.data, o, src.shape, tr)
            p.data.copy_(src)
            p._gdn_arena = self
        self.ptr0 = self.items[0][0].data_ptr() if self.items else 0
        self.generation = 0
        self.data16, self._key16, self._v16 = None, None, {}
        # data parallelism (distributed.py): `reduced` -- the gradient arena holds sums over the ranks (an all-reduce ran
        # since the last fresh backward) rather than this rank's local gradients; `carry_reduced` -- an already reduced
        # gradient carried across a further backward (accumulation without zero_grad), kept OUT of the arena until the new
        # local contribution has been reduced too (sync_gradients adds it back), so nothing is summed over the ranks twice
        # gradient accumulation: `_grad_alt` -- a second gradient arena, made by the first accumulating
        # backward that qualifies (bind_grads) and kept; `_pinned` -- a graph capture has recorded this arena's gradient
        # address, so the two buffers never exchange roles again
        self._grad_alt = None
        self._pinned = False
        self.reduced = False
        self.reduced_scale = 1.0       # 1: the reduced arena holds sums over the ranks; 1/world: means (sync_gradients without an optimizer)
        self.carry_reduced = None      # always kept as a SUM over the ranks

    @staticmethod
    def _view(flat, off, shape, tr):
        n = 1
        for s in shape:
            n *= s
        sl = flat[off:off + n]
        if tr is None:
            return sl.view(shape)
        fwd, inv = _perm(tr)
        phys = [shape[i] for i in fwd]
        return sl.view(phys).permute(*inv)

    def touch(self):
        """Called by writers that bypass torch (the fused Adam kernel): parameters changed."""
        self.generation += 1

    def versions(self):
        """Sum of the parameters' own torch version counters: `p.data = view` gives every parameter a counter of its own,
        so load_state_dict / p.copy_() / a stock torch optimizer bump THESE and not the arena tensor's."""
        return sum(p._version for p, _, _, _ in self.items)

    def bf16_data(self):
        """bf16 shadow of the parameter arena (same offsets/layout), re-cast when the master changed."""
        key = (self.generation, self.data._version, self.versions(), _GRAPH_EPOCH)
        if self.data16 is None:
            self.data16 = torch.empty(self.numel, dtype=torch.bfloat16, device=self.device)
            self._key16 = None
        if self._key16 != key or torch.cuda.is_current_stream_capturing():
            ops.cast(self.data, out=self.data16)
            self._key16 = key
        return self.data16

    def _view_of(self, flat, p):
        if id(p) not in self._slot:
            raise KeyError("parameter not in arena")
        o, tr = self._slot[id(p)]
        return self._view(flat, o, p.shape, tr)

    def bf16_view(self, p):
        v = self._v16.get(id(p))
        if v is None:
            v = self._v16[id(p)] = self._view_of(self.bf16_data(), p)
        return v

    def intact(self):
        return all(p.data_ptr() == self.data.data_ptr() + 4 * o and p.device == self.data.device
                   for p, o, _, _ in self.items)

    def grad_view(self, p):
        return self._view_of(self.grad, p)

    def _exchange_ok(self):
        """An accumulating backward may make its sum in the second gradient arena: a GPU arena outside a stream capture
        whose gradient address no captured graph holds, every parameter's .grad already its arena slice, and no all-reduced
        gradient involved (that one takes the carry_reduced detour of finish_grads)."""
        if self.device.type != "cuda" or self._pinned or self.reduced or self.carry_reduced is not None:
            return False
        base = self.grad.data_ptr()
        return all(p.grad is not None and p.grad.data_ptr() == base + 4 * o for p, o, _, _ in self.items)

    def bind_grads(self):
        """Point every .grad at its arena slice for one backward.  Returns the params whose existing, caller-owned grad
        must be accumulated afterwards.  A .grad that already IS the arena slice (a second backward without zero_grad:
        gradient accumulation) is carried over: the kernels overwrite their slices, finish_grads() adds the carry back.

        Where every parameter is carried (_exchange_ok) nothing is copied: the two gradient arenas exchange roles -- the
        old sum becomes the carry, the tape writes into the other buffer, which every .grad now views -- and finish_grads()
        adds the carry with one launch of gdn_grad_accumulate.  Every other case clones the arena as it always did."""
        self._gv = {}
        self._written = set()
        self._bound_before = set()
        self._carry = None
        self._carry_kept = False
        capturing = self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        if capturing:
            self._pinned = True
        elif self.items and self._exchange_ok():
            if self._grad_alt is None:
                self._grad_alt = ops.zeros((self.numel,), self.device)       # (the padding between slices stays zero)
            self._carry, self.grad, self._grad_alt = self.grad, self._grad_alt, self.grad
            self._carry_kept = True
            for p, o, n, tr in self.items:
                gv = self._view(self.grad, o, p.shape, tr)
                p.grad = gv
                self._gv[id(p)] = gv
                self._bound_before.add(id(p))
            return []
        accumulate = []
        for p, o, n, tr in self.items:
            gv = self._view(self.grad, o, p.shape, tr)
            if p.grad is not None:
                if p.grad.data_ptr() == gv.data_ptr():
                    self._bound_before.add(id(p))
                else:
                    accumulate.append((p, p.grad))
            p.grad = gv
            self._gv[id(p)] = gv
        if self._bound_before:
            self._carry = self.grad.clone()
            for p, o, n, tr in self.items:
                if id(p) not in self._bound_before:
                    self._carry[o:o + n].zero_()
        else:
            self.reduced = False               # a fresh backward overwrites the arena with this rank's local gradients
            self.carry_reduced = None
        return accumulate

    def mark_written(self, params):
        self._written.update(id(p) for p in params)

    def finish_grads(self):
        """After the tape ran: parameters no kernel wrote a gradient for (requires_grad False, an unused branch) get the
        state autograd would leave -- their previous gradient, or None -- instead of whatever an earlier step left in the
        arena; a carried gradient (see bind_grads) is added back."""
        for p, o, n, tr in self.items:
            if id(p) in self._written:
                continue
            if id(p) in self._bound_before:
                self.grad[o:o + n].zero_()            # the carry holds the old value
            else:
                p.grad = None
        if self._carry is not None:
            if self.reduced:
                # the carry is a sum over the ranks, what the tape just wrote is local: they meet after the next all-reduce
                if self.reduced_scale != 1.0:
                    self._carry.mul_(1.0 / self.reduced_scale)
                self.carry_reduced = self._carry if self.carry_reduced is None else self.carry_reduced.add_(self._carry)
                self.reduced = False
            elif self._carry_kept:
                ops.grad_accumulate(self.grad, self._carry)       # written + carry, what grad.add_(carry) gives
            else:
                self.grad.add_(self._carry)
            self._carry = None


def begin_backward(module, arena, ctx, trainable=True):
    """Gradient bookkeeping before a model's tape replays (the bridge's backward; also driven directly by the CPU tests of
    the data-parallel accumulation semantics).  Returns the caller-owned gradients to accumulate afterwards."""
    red = getattr(module, "_gdn_reducer", None)
    mine = red is not None and red.arena is arena
    if mine and red.active:
        # a previous backward's overlapped all-reduces are still in flight (backward, backward, ... without a
        # sync_gradients in between): wait for them before bind_grads() reads the arena; it then holds reduced sums
        red.finish()
        arena.reduced, arena.reduced_scale = True, 1.0
    pending = arena.bind_grads() if trainable else []      # a frozen network (the guide) only passes dx through
    # the overlapped reducer hands buckets to async all-reduces while the tape is still running; a carried gradient
    # (backward without zero_grad: finish_grads adds it AFTER the tape) or a caller-owned .grad would be added behind
    # those reductions' backs -- such a backward leaves its local gradients in the arena and sync_gradients reduces the
    # whole arena afterwards (an already REDUCED carry is kept aside until then: ParamArena.carry_reduced)
    # a model whose step is captured (graph.GraphedDataParallelStep) never overlaps: a collective issued from inside a
    # capture, or by a tape that a replay does not run, is no collective at all -- its arena is reduced whole afterwards
    if mine and trainable and not pending and not arena._bound_before and \
            not getattr(module, "_gdn_whole_arena_sync", False) and \
            not (arena.device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
        red.begin()
        ctx.reducer = red
    return pending


def end_backward(arena, pending, trainable=True):
    if trainable:
        arena.finish_grads()
    for p, old in pending:       # a caller-owned .grad existed: accumulate like autograd would
        if p.grad is None:
            p.grad = old
        else:
            p.grad.add_(old)


def ensure_arena(module, device):
    ar = getattr(module, "_gdn_param_arena", None)
    if ar is None or ar.device != device or not ar.intact():
        ar = ParamArena(module, device)
        module._gdn_param_arena = ar
    return ar


# ----------------------------------------------------------------------------
# Tape
# ----------------------------------------------------------------------------
class Ctx:
    def __init__(self, record, arena=None, input_needs_grad=False, dtype=torch.float32, module_training=True):
        self.record = record
        self.module_training = module_training  # the called module is in train(): its eval-mode norm layers are frozen on purpose
        self.dtype = dtype                     # storage dtype of activations / activation gradients
        self.tape = []
        self.arena = arena
        self.grads = {}
        self.input = None                      # the model's NHWC input buffer
        self.input_needs_grad = input_needs_grad
        self.reducer = None                    # distributed.GradReducer while a backward is running
        self.bn_src = {}                       # id(activation) -> BnOut of the train-mode BatchNorm that produced it
        self.up_src = {}                       # id(upsampled tensor) -> (its low-resolution source, up2x mode): conv_bn_act(up_out=)
        self.live = {}                         # id(activation) -> the activation, for every live one (is_live)

    def grads_done(self, *params):
        """Parameters whose gradient has just been written (lets the all-reduce start early)."""
        if self.arena is not None:
            self.arena.mark_written(params)
        if self.reducer is not None:
            self.reducer.mark(params)

    def claim(self, x):
        """Called by whatever consumes activation x FIRST in the forward.  That consumer's backward runs after every other
        consumer's, so its data gradient (with the accumulated `addsrc`) is the final value of dL/dx: if x came out of a
        train-mode BatchNorm, the kernel writing it can also emit that BatchNorm's backward reduction (BnOut.partial).
        Returns the BnOut (once), or None."""
        if isinstance(x, BnOut):
            return x if x.claim() else None
        info = self.bn_src.pop(id(x), None)
        return info if info is not None and info.claim() else None

    def wants_dx(self, x):
        """Data gradients stop at the network input unless the caller asked for them -- and at every activation that is not
        live: nothing it descends from trains (a frozen encoder), so no gradient below it is ever read."""
        return (x is not self.input or self.input_needs_grad) and self.is_live(x)

    # liveness: an activation is live when it descends from a trainable parameter or from an input that needs
    # a gradient.  Nothing adds a gradient into an activation that is not live, so the layer that produced it finds none and
    # its backward returns at once: no backward work below the lowest trainable layer.
    def _descends(self, x):
        return id(x) in self.live or (x is self.input and self.input_needs_grad)

    def is_live(self, x):
        return not _PRUNE_FROZEN or self._descends(x)

    def mark_live(self, out, inputs=(), params=()):
        """Called by every tape op while it records: `out` (a tensor, a BnOut or an Up2x) is live if one of `inputs` is, or
        one of `params` trains.  Returns `out`."""
        if not self.record:
            return out
        if any(p is not None and p.requires_grad for p in params) or any(x is not None and self._descends(x) for x in inputs):
            self.live[id(out)] = out
        return out

    # gradient slots are keyed by tensor identity
    def add_grad(self, t, g):
        k = id(t)
        old = self.grads.get(k)
        if old is None:
            self.grads[k] = (t, g)
        else:
            self.grads[k] = (t, _add(old[1], g, t.dtype))

    def pop_grad_as(self, t, dtype):
        """pop_grad, converted to `dtype` (the head's fp32 input gradient meeting a bf16 consumer)."""
        g = self.pop_grad(t)
        if g is not None and g.dtype != dtype:
            g = ops.cast(_dense(g), dtype)
        return g

    def pop_grad(self, t):
        e = self.grads.pop(id(t), None)
        return None if e is None else e[1]

    def backward(self):
        if self.tape is None:
            raise GdnError("this forward's tape was already consumed (retain_graph is not supported on the HIP path)")
        for fn in reversed(self.tape):
            fn()
        self.tape = None      # drop the saved activations
        self.live = {}


def _chan_slice(t):
    """True for a pure channel slice of a dense NHWC buffer: channel stride 1, one pixel pitch, rows and images laid out
    back to back at that pitch -- the only non-contiguous shape gdn_add_pitched addresses correctly (a spatial crop or a
    strided batch view has other row / image strides and takes the generic copy)."""
    return (t.dim() == 4 and t.shape[3] % 4 == 0 and t.stride(3) == 1 and t.stride(1) == t.shape[2] * t.stride(2)
            and t.stride(0) == t.shape[1] * t.stride(1))


def _dense(t):
    """Dense copy of a channel-slice view (the gradient of a torch.cat half); contiguous tensors pass through."""
    if t.is_contiguous():
        return t
    if _chan_slice(t):
        return ops.add_pitched(t)
    out = torch.empty(t.shape, dtype=t.dtype, device=t.device)
    out.copy_(t)
    return out


def _add(a, b, out_dtype):
    if a.is_contiguous() and b.is_contiguous():
        return ops.add(a, b, out_dtype=out_dtype)
    if _chan_slice(a) and _chan_slice(b):
        return ops.add_pitched(a, b, out_dtype=out_dtype)
    return ops.add(_dense(a), _dense(b), out_dtype=out_dtype)


class BnOut:
    """What a train-mode conv + BatchNorm (+ReLU) layer leaves behind for its backward: the raw conv output y, the
    coefficients co = [scale, shift, mean, invstd] and, once the kernel that writes the final dL/d(output) has run, that
    kernel's per-slot partial sums of the BatchNorm backward reduction (`partial`, or None: run the reduce pass).

    It doubles as the DEFERRED activation of a ResidualBlock's first half: `a = relu(bn1(conv1 x))` has exactly one
    consumer (conv2), whose patch loader applies scale / shift / ReLU on the fly, so `a` is never written to memory
    (AE_model_unet.py:49-54; north_star "conv+BN+ReLU fused").  A consumer that cannot do that calls dense()."""

    def __init__(self, y, co, relu):
        self.y, self.co, self.relu = y, co, relu
        self.partial = None
        self._claimed = False
        self._dense = None
        self.shape, self.dtype = y.shape, y.dtype

    def claim(self):
        first, self._claimed = not self._claimed, True
        return first

    def dense(self, out_dtype=None):
        if self._dense is None:
            self._dense = ops.bn_apply(self.y, self.co[0], self.co[1], self.relu, None, out_dtype=out_dtype)
        return self._dense


class Up2x:
    """Deferred x2 bilinear upsampling of `src` (F.interpolate(scale_factor=2, mode='bilinear'), AE_model_unet.py:336-359):
    the one consumer -- a ConvBlock -- interpolates while its transform kernel gathers the patches and its backward's fold
    pass applies the adjoint, so the upsampled tensor (4x src) and its gradient are never written.  A consumer whose path
    has no such loader calls dense(ctx): the stand-alone kernels, with their tape entry."""

    def __init__(self, src, align_corners):
        self.src, self.align = src, bool(align_corners)
        B, H, W, C = src.shape
        self.shape, self.dtype = torch.Size((B, 2 * H, 2 * W, C)), src.dtype
        self.mode = 2 if align_corners else 1          # in_up2x / dx_up2x of the C ABI

    def dense(self, ctx):
        x, align = self.src, self.align
        y = ops.upsample2x(x, align)
        if ctx.record:
            ctx.mark_live(y, (x, self))

            def bwd():
                dy = ctx.pop_grad(y)
                if dy is None or not ctx.is_live(x):
                    return
                ctx.add_grad(x, ops.upsample2x_bwd(_dense(dy), align))
            ctx.tape.append(bwd)
        return y


def _conv_op(mod, reflect):
    op = getattr(mod, "_gdn_op", None)
    if op is None:
        tr = isinstance(mod, torch.nn.ConvTranspose2d)
        op = ops.Conv(mod.in_channels, mod.out_channels, mod.kernel_size[0], mod.stride[0],
                      mod.padding[0] if not reflect else reflect, reflect=bool(reflect), transposed=tr)
        mod._gdn_op = op
    return op


def _flip_op(ctx, conv, bn, ldt, x2):
    """A stride-1 ConvTranspose2d(k, padding=k // 2) with odd k IS a convolution: the correlation with its stored taps in
    reverse order, and its tap-major buffer [k*k][Cout][Cin] is already laid out like a Conv2d's.  Written that way
    (ops.Conv(flip_taps=True): a transposed = 0 geometry carrying GDN_HINT_FLIP_TAPS) the frequency-domain and Winograd paths
    run it forward and backward.  Returns that op for a layer whose backward is being recorded -- the legacy
    AutoEncoder's three decoder layers under training -- or None: without a tape (inference), in bf16, with a concatenated
    input or in front of a train-mode InstanceNorm the layer stays the transposed op it always was.  conv_bn_act keeps the op
    only where _conv_path then picks a transform-domain path for it."""
    if not (ctx.record and isinstance(conv, torch.nn.ConvTranspose2d) and x2 is None
            and ldt == torch.float32 and ctx.dtype == torch.float32):
        return None
    k = conv.kernel_size[0]
    if (conv.stride[0] != 1 or k not in _FLIP_TAPS_K or conv.padding[0] != k // 2 or conv.output_padding[0] != 0
            or conv.dilation[0] != 1 or conv.groups != 1 or conv.kernel_size[1] != k):
        return None
    if bn.training and isinstance(bn, torch.nn.InstanceNorm2d):
        return None
    op = getattr(conv, "_gdn_op_flip", None)
    if op is None:
        op = ops.Conv(conv.in_channels, conv.out_channels, k, 1, k // 2, flip_taps=True)
        conv._gdn_op_flip = op
    return op


def _w_tap(mod):
    tr = isinstance(mod, torch.nn.ConvTranspose2d)
    v = tap_view(mod.weight.data, tr)
    if v is None:
        raise GdnError("conv weight is not in tap-major layout; call the model once on its device first")
    return v, tr


def _w_for(ctx, mod, dtype):
    """Tap-major weight in the layer's compute dtype (bf16: view into the arena's bf16 shadow)."""
    w, tr = _w_tap(mod)
    if dtype == torch.float32:
        return w, tr
    if ctx.arena is None:
        raise GdnError("bf16 compute needs the parameter arena")
    ctx.arena.bf16_data()                       # refresh the shadow if the master changed
    v = tap_view(ctx.arena.bf16_view(mod.weight), tr)
    return v, tr


def _layer_dtype(ctx, conv):
    """bf16 layers need 64-channel reduction slabs; the image-input conv stays fp32."""
    if ctx.dtype == torch.bfloat16 and conv.in_channels % 64 == 0 and conv.out_channels % 64 == 0:
        return torch.bfloat16
    return torch.float32


def _grad_tap(mod):
    gv = tap_view(mod.weight.grad, isinstance(mod, torch.nn.ConvTranspose2d))
    if gv is None:
        raise GdnError("weight.grad is not tap-major")
    return gv


def _wgrad_into(ctx, mod, x, dy, x2=None):
    """Weight gradient of a conv module straight into its arena slice."""
    op = mod._gdn_op
    gv = _grad_tap(mod)
    op.wgrad(x, dy, gv, 0)
    if x2 is not None:
        op.wgrad(x2, dy, gv, x.shape[3])


def _eval_key(bn):
    ar = getattr(bn.weight, "_gdn_arena", None)       # the fused Adam writes gamma / beta behind torch's version counters
    return (_GRAPH_EPOCH, getattr(bn, "_gdn_stats_ver", 0), bn.running_mean._version, bn.running_var._version,
            bn.weight._version, bn.bias._version, bn.running_mean.data_ptr(), bn.weight.data_ptr(),
            None if ar is None else ar.generation)


def _stored_coeffs(bn, frozen):
    """Coefficients of a norm layer that normalises by its running statistics, cached until its tensors change (the key follows
    the arena generation, so a gamma / beta update by the fused Adam invalidates it): [scale, shift] of an eval-mode layer
    (ops.bn_eval_coeffs), or with `frozen` the [scale, shift, mean, invstd] block of a train-mode layer for one that is being
    trained on frozen statistics (ops.bn_frozen_coeffs)."""
    attr, fn = ("_gdn_frozen_cache", ops.bn_frozen_coeffs) if frozen else ("_gdn_eval_cache", ops.bn_eval_coeffs)
    key = _eval_key(bn)
    c = getattr(bn, attr, None)
    if c is None or c[0] != key:
        c = (key, fn(bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, bn.eps))
        setattr(bn, attr, c)
    return c[1]


def _frozen_stats(ctx, conv, bn):
    """A frozen-statistics trained layer (--freeze_bn): the tape is recording, the called module is in train()
    while this norm layer stays in eval(), and the layer has something to train.  It normalises by the running statistics and
    updates none of them, but keeps its raw conv output and trains conv weight, gamma and beta like a train-mode layer.  (A
    module that is in eval() as a whole is inference: its layers keep the fused epilogue, and a backward reaches only layers
    with nothing trainable.)"""
    return bool(ctx.record and ctx.module_training and not bn.training
                and (conv.weight.requires_grad or bn.weight.requires_grad or bn.bias.requires_grad))


# The kernels one conv_bn_act call runs (_conv_path).  fused_in: the loader applies a deferred train-mode BatchNorm
# (in_affine / in_relu) or x2 upsampling (up2x); dyb: the backward applies this layer's BatchNorm backward while it transforms
# dy; bnb_slots(): slots of the BatchNorm-backward partials of x's producer that the data gradient can emit; fwd(x, w, stats=,
# [loader / epilogue keywords]) -> (y, stats or None, saved state or None) (_fwd3); bwd(dy, w, in_hw, saved state, ...) -> dx
# (transform paths only); c1_wgrad: the weight gradient runs on conv_c1_wgrad; up_fold: the direct data gradient may fold the
# producer's x2 upsampling (gdn_conv_dgrad dx_up2x); epilogue: the forward takes an eval-mode BatchNorm epilogue.
ConvPath = collections.namedtuple("ConvPath", "name fused_in dyb bnb_slots fwd bwd c1_wgrad up_fold epilogue")


def _fwd3(fwd, **fixed):
    """One return shape for every path's forward: ops.*_fwd return y alone, (y, stats), (y, state) or (y, stats, state),
    depending on what was asked for; this returns (y, stats or None, state or None)."""
    def run(x, w, stats=False, **kw):
        r = fwd(x, w, stats=stats, **fixed, **kw)
        if not isinstance(r, tuple):
            return r, None, None
        if stats:
            return r[0], r[1], (r[2] if len(r) > 2 else None)
        return r[0], None, r[1]
    return run


def _conv_path(ctx, x, conv, bn, op, ldt, x2, reflect):
    """Which kernels run layer `conv` on input x (a tensor, a BnOut or an Up2x), first match wins:
      fft     frequency domain (csrc/conv_fft.hip): fp32, window >= _FFT_MIN_K, stride 1
      wino    Winograd F(4x4 / 2x2, 3x3) (csrc/conv_wino.hip): fp32, 3x3, stride 1 (64..512 channels)
      wino2   Winograd F(3x3,2x2) (csrc/conv_wino2.hip): fp32, 4x4, stride 2, both channel counts >= _WINO2_MIN_C
      c1      1 <-> 64 channel 9x9 kernels (csrc/conv_c1.hip): fp32 1- or 3-channel image into a Conv2d
      direct  op.fwd / op.dgrad (the C library picks igemm / ring / ring2)
    the transform paths and c1 only where the C library supports the geometry, never with a concatenated x2, and never in front
    of a train-mode InstanceNorm, which runs image by image on the direct kernels (_instance_fwd)."""
    k, s = conv.kernel_size[0], conv.stride[0]
    B, H, W = x.shape[0], x.shape[1], x.shape[2]
    lazy = isinstance(x, BnOut)
    fp32 = ldt == torch.float32 and x2 is None and not (bn.training and isinstance(bn, torch.nn.InstanceNorm2d))
    # GDN_HINT_TRAIN: a layer whose weight is trained (forward + backward + weight gradient), on batch statistics or on frozen
    # ones -- the frequency-domain path then tiles for the sum of both passes (40-point tiles on the 9x9 layers); layers with a
    # fixed weight and inference keep the forward-optimal plan.  Only such a layer keeps the transform-domain state of its forward.
    train = bool(ctx.record and conv.weight.requires_grad and (bn.training or _frozen_stats(ctx, conv, bn)))
    path = functools.partial(ConvPath, c1_wgrad=False, up_fold=False, epilogue=conv.out_channels > 1)
    if fp32 and k >= _FFT_MIN_K and s == 1 and op.fft_ok(B, H, W, backward=ctx.record, train=train):
        if ctx.dtype == torch.bfloat16:
            # A model that computes in bf16 runs barrier-paced 16-bit matrix kernels (conv_*_bf16) and must never have a
            # frequency-domain kernel in flight beside them (measured interference on this hardware; the
            # frequency-domain backward uses a second stream).  No layer of a bf16 model qualifies today (ldt is fp32 only for
            # the 3-channel input conv); this keeps it that way by construction (tools/check_no_mfma16_beside_fft.py checks traces).
            raise GdnError("internal: a bf16 model selected a frequency-domain layer")
        return path("fft", True, True, functools.partial(op.fft_bnb_slots, B, H, W, train=train),
                    _fwd3(op.fft_fwd, spectrum=train, train=train), functools.partial(op.fft_bwd, train=train))
    if fp32 and k == 3 and s == 1 and op.wino_ok(B, H, W):
        return path("wino", True, False, functools.partial(op.wino_bnb_slots, B, H, W), _fwd3(op.wino_fwd, state=train), op.wino_bwd)
    if (fp32 and k == 4 and s == 2 and not lazy and min(conv.in_channels, conv.out_channels) >= _WINO2_MIN_C
            and op.wino2_ok(B, H, W)):
        return path("wino2", False, False, lambda: 0, _fwd3(op.wino2_fwd, state=train), op.wino2_bwd)
    # (an Up2x input reaches c1 materialised: c1_ok reads dtype, channels and layout, which its source shares)
    if (fp32 and not lazy and conv.in_channels in (1, 3) and not isinstance(conv, torch.nn.ConvTranspose2d)
            and ops.c1_ok(x.src if isinstance(x, Up2x) else x, conv.out_channels, k, s, reflect or conv.padding[0], rgb=True)):
        return path("c1", False, False, None, _fwd3(ops.conv_c1_fwd, reflect=bool(reflect)), None, c1_wgrad=conv.in_channels == 1)
    return path("direct", False, False, None, _fwd3(op.fwd, x2=x2), None,
                up_fold=bool(reflect and not lazy and x2 is None and conv.in_channels % 4 == 0 and H % 2 == 0 and W % 2 == 0))


# ----------------------------------------------------------------------------
# conv_bn_act: one layer call = a layer record (_layer_call), a norm record (_norm_call) and the helpers below
# ----------------------------------------------------------------------------
# What the norm layer does in one conv_bn_act call, decided once in the forward:
BATCH, FROZEN, FOLDED, EVAL, INSTANCE = "batch", "frozen", "folded", "eval", "instance"
#   BATCH     train-mode BatchNorm: batch statistics from the conv epilogue, running statistics updated
#   FROZEN    eval-mode norm layer of a module being trained (_frozen_stats): running statistics, raw conv output kept
#   FOLDED    eval-mode norm layer folded into the conv epilogue: conv + scale / shift + ReLU (+ residual) in one pass
#   EVAL      eval-mode norm layer applied by a pass of its own (the epilogue cannot take it)
#   INSTANCE  train-mode InstanceNorm2d: per-image statistics, the BatchNorm kernels on one image at a time


class NormCall:
    """The norm layer of one conv_bn_act call.  The forward fills it: `mode`; `co`, the coefficient block ([scale, shift] for
    FOLDED / EVAL, [scale, shift, mean, invstd] for BATCH / FROZEN, one such block per image for INSTANCE); `y`, the raw conv
    output (per image for INSTANCE); `out`, the BnOut of a BATCH / FROZEN layer (it carries the backward's partial sums).
    dyb: the layer's path applies the last pass of the BatchNorm backward while it transforms dy; ldt: the dtype of dy."""
    __slots__ = ("mode", "bn", "relu", "dyb", "ldt", "co", "y", "out")

    def __init__(self, mode, bn, relu, dyb, ldt):
        self.mode, self.bn, self.relu, self.dyb, self.ldt = mode, bn, relu, dyb, ldt
        self.co = self.y = self.out = None


class LayerCall:
    """What _layer_call resolved for one conv_bn_act call and what its backward needs: conv, bn, op, path, ldt, w, reflect;
    x (an Up2x only while `up` is set), x2, xin (ConvPath / Ctx.claim), up (the Up2x whose interpolation the loader applies);
    residual, need_dx; xt (the tensor the conv kernels read), state (what a trained transform-domain layer's forward keeps),
    up_in (the low-resolution source of an upsampled x and its mode, where the data gradient may fold the upsampling)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _layer_call(ctx, x, conv, bn, x2, reflect):
    op = _conv_op(conv, reflect)
    ldt = _layer_dtype(ctx, conv)
    if x.dtype != ldt:
        raise GdnError("layer %d->%d computes in %s but its input is %s" % (conv.in_channels, conv.out_channels, ldt, x.dtype))
    fop = _flip_op(ctx, conv, bn, ldt, x2)
    path = _conv_path(ctx, x, conv, bn, fop or op, ldt, x2, reflect)
    if fop is not None:
        if path.name in ("fft", "wino"):
            op = fop
        else:                            # no transform-domain path takes this geometry: the transposed op, as ever
            path = _conv_path(ctx, x, conv, bn, op, ldt, x2, reflect)
    up = None
    if isinstance(x, Up2x):
        # training needs the fold pass of a reflection-padded layer for the adjoint of the interpolation
        if path.fused_in and (not ctx.record or reflect):
            up = x
        else:
            x = x.dense(ctx)
    xin = ctx.claim(x)                   # BnOut of the train-mode BatchNorm that produced x, if we are its first consumer
    if x2 is not None:
        ctx.claim(x2)
    w, _ = _w_for(ctx, conv, ldt)
    return LayerCall(conv=conv, bn=bn, op=op, path=path, ldt=ldt, w=w, reflect=reflect, x=x, x2=x2, xin=xin, up=up, state=None)


def _norm_call(ctx, L, relu):
    """The NormCall of layer call L with its mode: the one place that reads bn.training and, through _frozen_stats, the
    requires_grad flags the forward goes by."""
    bn, residual = L.bn, L.residual
    if bn.training:
        mode = INSTANCE if isinstance(bn, torch.nn.InstanceNorm2d) else BATCH
    elif _frozen_stats(ctx, L.conv, bn):
        # the running statistics normalise, nothing updates them, and the raw conv output is kept (no epilogue fold) with a
        # train-mode layer's coefficient block, so everything downstream of a train-mode layer -- deferred activation, apply
        # passes, the consumers' BatchNorm-backward partials -- works on it unchanged
        mode = FROZEN
    elif (L.path.epilogue and L.ldt == ctx.dtype and not (relu and residual is not None)
            and (residual is None or residual.dtype == L.ldt)):
        mode = FOLDED
    else:
        mode = EVAL
    if mode == INSTANCE and (L.x2 is not None or residual is not None or L.ldt != torch.float32):
        raise GdnError("train-mode InstanceNorm is implemented for the standalone fp32 ConvBlock / ConvTBlock only")
    return NormCall(mode, bn, relu, L.path.dyb, L.ldt)


def _loader_input(ctx, L):
    """(the tensor the conv kernels read, the forward's loader keywords): a deferred upsampling or BatchNorm is applied by the
    loader where the path has one (fft / wino); the other loaders go straight to LDS, so a deferred activation is written."""
    x = L.x
    if L.up is not None:
        return L.up.src, dict(up2x=L.up.mode)
    if not isinstance(x, BnOut):
        return x, {}
    if L.path.fused_in and _FUSE_TRAIN_BN:
        return x.y, dict(in_affine=(x.co[0], x.co[1]), in_relu=x.relu)
    return x.dense(ctx.dtype), {}


def _conv_fwd(L, norm, kw):
    """The convolution with what the norm mode asks of it: statistics (BATCH) or the folded epilogue (FOLDED).  Fills
    norm.co / y / out and L.state."""
    bn, mode = norm.bn, norm.mode
    if mode != BATCH:
        co = norm.co = _stored_coeffs(bn, mode == FROZEN)
    if mode == FOLDED:
        kw.update(affine=(co[0], co[1]), act=ops.ACT_RELU if norm.relu else ops.ACT_NONE, addsrc=L.residual)
    y, st, L.state = L.path.fwd(L.xt, L.w, stats=mode == BATCH, **kw)
    if mode == BATCH:
        mom = 0.1 if bn.momentum is None else bn.momentum
        norm.co = ops.bn_finalize_train(st, y.shape[0] * y.shape[1] * y.shape[2], bn.weight.data, bn.bias.data, bn.running_mean,
                                        bn.running_var, mom, bn.eps, num_batches_tracked=bn.num_batches_tracked)
        bn._gdn_stats_ver = getattr(bn, "_gdn_stats_ver", 0) + 1
    norm.y = y
    if mode in (BATCH, FROZEN):
        norm.out = BnOut(y, norm.co, norm.relu)


def _norm_apply(ctx, L, norm, defer, up_out):
    """The layer's output from the raw conv output: (a, a upsampled x2 or None).  a is y itself (FOLDED), the BnOut (a deferred
    train-mode fp32 layer without a residual: scale / shift / ReLU happen in the consumer's loader) or what the apply pass
    writes -- on the bf16 path together with the upsampled tensor the caller asked for (up_out), in one kernel."""
    y, co, residual, a_up = norm.y, norm.co, L.residual, None
    if norm.mode == FOLDED:
        return y, None
    if (defer and norm.out is not None and residual is None and _FUSE_TRAIN_BN and L.ldt == torch.float32
            and ctx.dtype == torch.float32):
        return norm.out, None
    if (up_out is not None and _FUSE_UP2X_BF16 and ctx.dtype == torch.bfloat16 and y.is_contiguous()
            and (residual is None or residual.is_contiguous()) and y.shape[0] * 2 * y.shape[1] <= 65535
            and y.shape[3] % 4 == 0):             # (the fused kernel's channel-vector width; other shapes take the two-pass form)
        a, a_up = ops.bn_apply_up2x(y, co[0], co[1], norm.relu, residual, align_corners=bool(up_out), out_dtype=ctx.dtype)
    else:
        a = ops.bn_apply(y, co[0], co[1], norm.relu, residual, out_dtype=ctx.dtype)
    if norm.out is not None and ctx.record and _FUSE_TRAIN_BN:
        ctx.bn_src[id(a)] = norm.out
    return a, a_up


def _instance_fwd(ctx, L, norm):
    """Conv -> train-mode InstanceNorm2d(affine=True, track_running_stats=True) -> [ReLU]: the standalone
    ConvBlock / ConvTBlock(norm='Instance') of the reference (AE_model_unet.py:70-75, :88-92; R and G never build one).
    Per-instance statistics are batch statistics of a batch of one, so the BatchNorm kernels run once per image on that
    image's slice: the convolution writes image b's output with its sum / sum-of-squares partials, finalize (momentum 1 into
    scratch buffers) yields that image's coefficients, mean and unbiased variance, apply / backward (_instance_bwd) use them;
    the running statistics take the batch mean of the per-instance values (what F.instance_norm does).  A rarely used path:
    direct kernels, B small launches."""
    x, inorm = L.xt, norm.bn
    B, C = x.shape[0], L.conv.out_channels
    mom = 0.1 if inorm.momentum is None else inorm.momentum
    norm.y, norm.co, outs = [], [], []
    rm = torch.zeros((B, C), dtype=torch.float32, device=x.device)
    rv = torch.ones((B, C), dtype=torch.float32, device=x.device)
    for b in range(B):
        yb, st, _ = L.path.fwd(x[b:b + 1], L.w, stats=True)
        co = ops.bn_finalize_train(st, yb.shape[1] * yb.shape[2], inorm.weight.data, inorm.bias.data, rm[b], rv[b], 1.0, inorm.eps)
        norm.y.append(yb)
        norm.co.append(co)
        outs.append(ops.bn_apply(yb, co[0], co[1], norm.relu, None, out_dtype=ctx.dtype))
    if inorm.track_running_stats:
        inorm.running_mean.mul_(1.0 - mom).add_(rm.mean(0), alpha=mom)
        inorm.running_var.mul_(1.0 - mom).add_(rv.mean(0), alpha=mom)
        # (torch's InstanceNorm2d leaves num_batches_tracked untouched: F.instance_norm does not take it)
        inorm._gdn_stats_ver = getattr(inorm, "_gdn_stats_ver", 0) + 1
    return torch.cat(outs, 0)


def _instance_bwd(norm, da, dgamma, dbeta):
    da = _dense(da)
    dg = torch.zeros(da.shape[3], dtype=torch.float32, device=da.device)
    db = torch.zeros_like(dg)
    dys = []
    for b, (yb, co) in enumerate(zip(norm.y, norm.co)):
        dgb, dbb = torch.empty_like(dg), torch.empty_like(db)
        dys.append(ops.bn_bwd(da[b:b + 1], yb, norm.bn.weight.data, co, norm.relu, dgb, dbb))
        dg += dgb
        db += dbb
    if dgamma is not None:
        dgamma.copy_(dg)
        dbeta.copy_(db)
    return torch.cat(dys, 0)


def _trained(L, norm):
    """(dgamma, dbeta, whether the conv weight gets a gradient, the parameters to report to ctx.grads_done) of a layer's
    backward: the one place that decides which parameter gradients the layer writes.

    When requires_grad is read.  The FORWARD reads it twice: _frozen_stats (is this eval-mode layer being trained: the norm
    mode) and _conv_path's GDN_HINT_TRAIN (does the layer keep transform-domain state).  Everything here is read when the TAPE
    REPLAYS, so a flag changed between forward and backward acts on the gradients written but not on the mode.  A FROZEN layer
    writes exactly the gradients that are asked for (NULL pointers for the rest); every other layer with anything trainable
    writes all three, as a train-mode layer always did, and one with nothing trainable writes none."""
    params = (norm.bn.weight, norm.bn.bias, L.conv.weight)
    rg = [p.requires_grad for p in params]
    if norm.mode != FROZEN:
        rg = [any(rg)] * 3
    if rg[0] and norm.mode in (FOLDED, EVAL):
        raise GdnError("backward through an eval-mode BatchNorm of a module in eval() is only implemented for layers "
                       "with nothing to train (requires_grad False on the conv and BN parameters: the guide network of "
                       "--latent_grad); to train on frozen statistics keep the module in train() and its norm layers in "
                       "eval() (freeze_bn())")
    return (params[0].grad if rg[0] else None, params[1].grad if rg[1] else None, rg[2],
            tuple(p for p, r in zip(params, rg) if r))


def _norm_bwd(norm, da, dgamma, dbeta):
    """da -> (dy, extra keywords for the path's backward), by norm mode; dgamma / dbeta (or None) receive their gradients."""
    mode, y, co, relu = norm.mode, norm.y, norm.co, norm.relu
    if mode == INSTANCE:
        return _instance_bwd(norm, da, dgamma, dbeta), {}
    if mode in (FOLDED, EVAL):
        return ops.bn_eval_bwd(da, y, co, (2 if mode == FOLDED else 1) if relu else 0, out_dtype=norm.ldt), {}
    partial, norm.out.partial = norm.out.partial, None
    # frequency-domain layer: dy has one reader (the dy transform), which applies the last pass of the BatchNorm backward
    # while loading -- dy is never written
    on_load = norm.dyb and _FUSE_TRAIN_BN and da.is_contiguous() and da.dtype == torch.float32
    if mode == FROZEN and on_load:
        # the sums only; pass 3 of the BatchNorm backward with k1 = k2 = 0 IS scale * dz: the transform applies scale and mask
        ops.bn_frozen_bwd(da, y, co, relu, dgamma, dbeta, partial=partial, need_dy=False)
        return da, dict(dyb=(y, co, ops.zeros((2, y.shape[3]), y.device), relu))
    if mode == FROZEN:
        return ops.bn_frozen_bwd(da, y, co, relu, dgamma, dbeta, out_dtype=norm.ldt, partial=partial), {}
    if on_load:
        return da, dict(dyb=(y, co, ops.bn_bwd_coeffs(da, y, co, relu, dgamma, dbeta, partial=partial), relu))
    return ops.bn_bwd(da, y, norm.bn.weight.data, co, relu, dgamma, dbeta, out_dtype=norm.ldt, partial=partial), {}


def _bnb(xin, slots, device):
    """The `bnb` argument of a data gradient that is the final gradient of x = [relu](BN_train(xin.y)): (y, co, relu, partial),
    with the [slots, 2, C] buffer the kernel's epilogue fills with the producer's BatchNorm-backward partial sums; None
    where the kernel has no such epilogue (slots 0).  The caller stores bnb[3] as xin.partial once the kernel has run."""
    if slots <= 0:
        return None
    return (xin.y, xin.co, xin.relu, torch.empty((slots, 2, xin.y.shape[3]), dtype=torch.float32, device=device))


def _dgrad_into(ctx, op, dy, wt, x, x2=None, **kw):
    """Direct data gradient of a convolution of x (or of cat(x, x2)) into ctx.grads.  A single input's pending gradient rides
    along as addsrc and the result replaces it; the halves of a concatenated one are added to their inputs' gradients, each
    only where it is live (the skip connection of a frozen encoder is not).  kw: in_hw (default: x's), bnb, up2x of op.dgrad."""
    in_hw = kw.pop("in_hw", (x.shape[1], x.shape[2]))
    if x2 is None:
        ctx.grads[id(x)] = (x, op.dgrad(dy, wt, in_hw, addsrc=ctx.pop_grad_as(x, dy.dtype), **kw))
        return
    dcat = op.dgrad(dy, wt, in_hw)
    c1 = x.shape[3]
    if ctx.is_live(x):
        ctx.add_grad(x, dcat[..., :c1])
    if ctx.is_live(x2):
        ctx.add_grad(x2, dcat[..., c1:])


def _want_dx(ctx, L):
    return L.need_dx and (ctx.wants_dx(L.x) or (L.x2 is not None and ctx.wants_dx(L.x2)))


def _transform_grads(ctx, L, dy, extra, wtrain):
    """Transform-domain backward: one transform of dy feeds both gradients; the forward's transformed input is reused for dw."""
    gv = _grad_tap(L.conv) if wtrain else None
    want_dx = _want_dx(ctx, L)
    if gv is None and not want_dx:
        return
    xin, bnb, gx = L.xin, None, L.x                      # gx: the tensor whose gradient this layer's dx is
    if xin is not None and want_dx and xin.y.dtype == torch.float32:
        # this data gradient is the final gradient of x: emit the producer's BatchNorm-backward partial sums from the epilogue
        bnb = _bnb(xin, L.path.bnb_slots(), dy.device)
    if L.up is not None:
        extra["up2x"] = L.up.mode                        # ... the low-resolution source of the deferred upsampling
        gx = L.up.src
    dx = L.path.bwd(dy, L.w, (L.x.shape[1], L.x.shape[2]), L.state, dw_tap=gv, need_dx=want_dx,
                    addsrc=ctx.pop_grad_as(gx, L.ldt) if want_dx else None, bnb=bnb, **extra)
    if want_dx:
        ctx.grads[id(gx)] = (gx, dx)
        if bnb is not None:
            xin.partial = bnb[3]


def _direct_dgrad(ctx, L, dy):
    """Data gradient on the direct kernels.  bf16: the LDS-DMA ring kernel's epilogue emits the BatchNorm-backward partial sums
    of x's producer when this is x's final gradient (we are its first consumer; the other consumers' gradients arrive as
    addsrc), as the transform paths do for the fp32 layers.  up_in: x is an upsampled tensor whose producer kept the
    low-resolution source -- a reflection-padded layer's fold pass writes dL/d(source) directly."""
    op, x, xin, ldt = L.op, L.x, L.xin, L.ldt
    wt = ops.transpose_taps(_w_tap(L.conv)[0], dtype=ldt)
    if L.x2 is not None:
        return _dgrad_into(ctx, op, dy, wt, x, L.x2)
    bnb = None
    if xin is not None and ldt == torch.bfloat16 and xin.y.dtype == ldt and _FUSE_TRAIN_BN and xin.y.is_contiguous():
        bnb = _bnb(xin, op.dgrad_bnb_slots(x.shape[0], x.shape[1], x.shape[2], ldt), dy.device)
    if L.up_in is not None and bnb is None and id(x) not in ctx.grads:
        lo, mode = L.up_in
        return _dgrad_into(ctx, op, dy, wt, lo, in_hw=(x.shape[1], x.shape[2]), up2x=mode)
    _dgrad_into(ctx, op, dy, wt, x, bnb=bnb)
    if bnb is not None:
        xin.partial = bnb[3]


def _layer_bwd(ctx, L, norm, da):
    """The tape entry of one conv_bn_act call: norm backward, then both gradients of the convolution."""
    dgamma, dbeta, wtrain, done = _trained(L, norm)
    if L.residual is not None and ctx.is_live(L.residual):
        ctx.add_grad(L.residual, da)
    dy, extra = _norm_bwd(norm, da, dgamma, dbeta)
    if L.path.bwd is not None:
        _transform_grads(ctx, L, dy, extra, wtrain)
    elif wtrain and L.path.c1_wgrad and dy.is_contiguous():
        ops.conv_c1_wgrad(L.xt, dy, tap_view(L.conv.weight.grad, False), reflect=bool(L.reflect))
    elif wtrain:
        _wgrad_into(ctx, L.conv, L.xt, dy, L.x2)
    if done:
        ctx.grads_done(*done)
    if L.path.bwd is None and _want_dx(ctx, L):
        _direct_dgrad(ctx, L, dy)


def _also_upsampled(ctx, a, a_up, align):
    """(a, its x2 upsampling) for conv_bn_act(up_out=): a_up from the fused bf16 apply pass, with its tape entry, or upsample()."""
    if a_up is None:
        return a, upsample(ctx, a, align)
    ctx.claim(a)                         # (as upsample() does: the interpolation is this activation's first consumer)
    if ctx.record:
        ctx.up_src[id(a_up)] = (a, 2 if align else 1)
        ctx.mark_live(a_up, (a,))

        def up_bwd():                    # (after this tape entry in the forward = before the layer's own backward)
            dup = ctx.pop_grad(a_up)     # None when the consumer's fold pass already wrote dL/da (the usual case)
            if dup is not None:
                ctx.add_grad(a, ops.upsample2x_bwd(_dense(dup), align))
        ctx.tape.append(up_bwd)
    return a, a_up


def conv_bn_act(ctx, x, conv, bn, relu, residual=None, x2=None, reflect=0, need_dx=True, defer=False, up_out=None):
    """[relu](BN(conv(cat(x, x2)))) (+ residual): ConvBlock / ResidualBlock halves / ConvTBlock.

    up_out (None, or the align_corners flag): the caller also wants F.interpolate(output, scale_factor=2, mode='bilinear') and
    gets (output, upsampled) back -- on the bf16 path the BatchNorm-apply pass writes both (one kernel), on the fp32 path the
    upsampled one is the deferred Up2x of upsample().

    x may be a BnOut (the deferred activation of the previous layer) or an Up2x (a deferred upsampling): the fft / wino loaders
    apply its scale / shift / ReLU or interpolate while loading; any other path materialises it first.  defer=True (the
    caller guarantees a single consumer) returns this layer's output as a BnOut instead of running the BatchNorm-apply pass,
    when the layer is a train-mode fp32 one without a residual."""
    L = _layer_call(ctx, x, conv, bn, x2, reflect)
    L.residual, L.need_dx = residual, need_dx
    norm = _norm_call(ctx, L, relu)
    L.xt, kw = _loader_input(ctx, L)
    if norm.mode == INSTANCE:
        a, a_up = _instance_fwd(ctx, L, norm), None
    else:
        _conv_fwd(L, norm, kw)
        a, a_up = _norm_apply(ctx, L, norm, defer, up_out)
    # the layer's input is an upsampled tensor whose producer kept the low-resolution source (up_out of that call)
    L.up_in = ctx.up_src.get(id(L.x)) if L.path.up_fold else None
    if ctx.record:
        ctx.mark_live(a, (L.x, x2, residual), (conv.weight, bn.weight, bn.bias))

        def bwd():
            da = ctx.pop_grad(a)
            if da is not None:
                _layer_bwd(ctx, L, norm, da)
        ctx.tape.append(bwd)
    return a if up_out is None else _also_upsampled(ctx, a, a_up, bool(up_out))


def conv_head_tanh(ctx, x, conv):
    """Final 9x9 (transposed) conv to one channel + tanh (AE_model_unet.py:362-363, :570-571).
    On the bf16 path only x is bf16: weights, the depth map and this layer's backward results are fp32 (the 1 <-> 64 channel
    kernels read the bf16 x / the bf16 gradient already accumulated for x directly)."""
    op = _conv_op(conv, 0)
    ctx.claim(x)
    w, tr = _w_tap(conv)
    out = op.fwd(x, w, act=ops.ACT_TANH)
    if ctx.record:
        ctx.mark_live(out, (x,), (conv.weight,))

        def bwd():
            do = ctx.pop_grad(out)
            if do is None:
                return
            dpre = ops.tanh_bwd(do.contiguous(), out)
            # 64 -> 1 heads: both gradients are 1 <-> 64 channel correlations with the single-channel d(pre-tanh) as the
            # staged image (csrc/conv_c1.hip); a Conv2d head flips the taps, a ConvTranspose2d head does not
            c1 = (x.is_contiguous() and conv.out_channels == 1
                  and ops.c1_ok(dpre, conv.in_channels, conv.kernel_size[0], conv.stride[0], conv.padding[0]))
            if conv.weight.requires_grad:
                if c1:
                    ops.conv_c1_wgrad(dpre, x, tap_view(conv.weight.grad, tr), flip=not tr)
                else:
                    _wgrad_into(ctx, conv, x, dpre)
                ctx.grads_done(conv.weight)
            if not ctx.is_live(x):
                return                   # only the head trains: nothing below it needs a gradient
            if c1:
                ctx.grads[id(x)] = (x, ops.conv_c1_fwd(dpre, w, flip=not tr, addsrc=ctx.pop_grad(x)))
            else:                        # (fp32 like dpre, also for a bf16 x)
                _dgrad_into(ctx, op, dpre, ops.transpose_taps(w), x)
        ctx.tape.append(bwd)
    return out


def conv_plain(ctx, x, conv, x2=None):
    """Bare convolution without norm/activation (legacy AutoEncoder 1x1 after cat, :210)."""
    op = _conv_op(conv, 0)
    ctx.claim(x)
    if x2 is not None:
        ctx.claim(x2)
    ldt = _layer_dtype(ctx, conv)
    w, tr = _w_for(ctx, conv, ldt)
    y = op.fwd(x, w, x2=x2)
    if ctx.record:
        ctx.mark_live(y, (x, x2), (conv.weight,))

        def bwd():
            dy = ctx.pop_grad(y)
            if dy is None:
                return
            dy = _dense(dy)
            if dy.dtype != ldt:
                dy = ops.cast(dy, ldt)
            if conv.weight.requires_grad:
                _wgrad_into(ctx, conv, x, dy, x2)
                ctx.grads_done(conv.weight)
            wt = ops.transpose_taps(_w_tap(conv)[0], dtype=ldt)
            if ctx.wants_dx(x) if x2 is None else (ctx.is_live(x) or ctx.is_live(x2)):
                _dgrad_into(ctx, op, dy, wt, x, x2)
        ctx.tape.append(bwd)
    return y


def upsample(ctx, x, align_corners=False):
    """F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=...).  fp32: returned DEFERRED (Up2x) -- the consumer
    ConvBlock's loader interpolates; see conv_bn_act."""
    ctx.claim(x)
    if isinstance(x, BnOut):
        x = ctx.mark_live(x.dense(ctx.dtype), (x,))
    up = ctx.mark_live(Up2x(x, align_corners), (x,))
    if _FUSE_UP2X and ctx.dtype == torch.float32 and x.dtype == torch.float32 and x.is_contiguous():
        return up
    return up.dense(ctx)


# ----------------------------------------------------------------------------
# Boundary: NCHW torch tensors <-> NHWC device buffers
# ----------------------------------------------------------------------------
def to_nhwc(x):
    if x.dim() != 4:
        raise GdnError("expected a 4-D NCHW tensor")
    if not x.is_cuda:
        raise GdnError("input must live on the GPU: the HIP path has no CPU fallback")
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    B, C, H, W = x.shape
    if C == 1 and x.is_contiguous():
        return x.view(B, H, W, 1)
    p = x.permute(0, 2, 3, 1)
    if p.is_contiguous():       # already channels_last in memory
        return p
    return ops.nchw_to_nhwc(x.contiguous())


def to_nchw_view(t):
    """Logical NCHW view (channels_last strides) of an NHWC buffer -- zero copy."""
    return t.permute(0, 3, 1, 2)


def grad_to_nhwc(g):
    """Incoming NCHW-shaped gradient -> dense NHWC buffer (copy only if the memory order differs)."""
    g = g.detach()
    if g.dtype not in (torch.float32, torch.bfloat16):
        g = g.float()
    B, C, H, W = g.shape
    if C == 1:
        return g.contiguous().view(B, H, W, 1)
    p = g.permute(0, 2, 3, 1)
    if p.is_contiguous():
        return p
    return ops.nchw_to_nhwc(g.contiguous())
