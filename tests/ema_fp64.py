"""Float64 restatement of the weight average of the fused Adam (gdn_ema_update, include/gdn_hip.h), numpy only; the
yardstick of test_ema_cpu.py and test_hip_ema.py.

    w_t  = float32(1.0 - min(decay, (1.0 + t) / (10.0 + t)))       computed in double, rounded once
    e   <- e + w_t (p - e)                                          the kernel: fmaf(w_t, p - e, e) in float32

The bar.  One float32 update rounds p - e by at most 2^-24 |p - e| <= 2^-23 max(|p|, |e|), which w_t < 1 scales down, and
rounds the fma's result by at most 2^-24 |e'| <= 2^-24 max(|p|, |e|) (e' lies between e and p): together at most
3 2^-24 M < 2^-22 M per step, M the running maximum of |p| and |e| of that element.  The errors of earlier steps are
carried on with the factor 1 - w_t <= 1, so k steps stay within k 2^-22 M.
"""
import struct

import numpy as np

STATE_FMT = "<ddiff"          # AdamDevState: { double beta1^t, beta2^t; int32 t; float bc1, bc2s; } + 4 bytes of padding


def weight(decay, t):
    """The float32 w_t of applied update t = 1, 2, ..."""
    return np.float32(1.0 - min(float(decay), (1.0 + float(t)) / (10.0 + float(t))))


def update(e64, p32, decay, t):
    """One update in float64 from the float32 weights `p32` and the float32 w_t."""
    e64 = np.asarray(e64, np.float64)
    return e64 + np.float64(weight(decay, t)) * (np.asarray(p32, np.float32).astype(np.float64) - e64)


def update32(e32, p32, w32):
    """The kernel's own arithmetic in numpy: the float32 difference, then one fused multiply-add (the product and the sum
    are exact in float64 for float32 operands up to one rounding far below float32's, then rounded to float32)."""
    e32, p32 = np.asarray(e32, np.float32), np.asarray(p32, np.float32)
    d = (p32 - e32).astype(np.float32)
    return (np.float64(w32) * d.astype(np.float64) + e32.astype(np.float64)).astype(np.float32)


def bound(k, M):
    """What k float32 updates may differ from the float64 restatement by; M = running max of |p| and |e| per element."""
    return k * 2.0 ** -22 * np.asarray(M, np.float64)


def state_record(t, beta1=0.9, beta2=0.999):
    """The 32 bytes of an AdamDevState after t updates (only t matters to the average)."""
    p1, p2 = beta1 ** t, beta2 ** t
    return struct.pack(STATE_FMT, p1, p2, int(t), np.float32(1.0 - p1), np.float32(np.sqrt(1.0 - p2))) + bytes(4)
