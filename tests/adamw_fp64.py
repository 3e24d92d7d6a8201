"""The decoupled update of the gdn_adamw_step* entry points (include/gdn_hip.h) restated twice: in float64, as
the mathematics (torch.optim.AdamW up to the order of two additions), and in float32 with the header's roundings -- every
product, sum, quotient and root rounded on its own, the one fma evaluated exactly (fractions.Fraction) and rounded once -- so
a kernel that keeps those roundings gives these bits.  The float32 form also restates the coupled update of gdn_adam_step*
(coupled=True): both families go through one element of csrc/optim.hip, which differs in where the one fma sits."""
import fractions
import struct

import numpy as np

STATE_FMT = "<ddiff"          # AdamDevState: { double beta1^t, beta2^t; int32 t; float bc1, bc2s; } + 4 bytes of padding
f32 = np.float32


def dec32(lr, wd):
    """float32(double(lr) * double(wd)) of the float32 values the kernel reads."""
    return f32(float(f32(lr)) * float(f32(wd)))


def corrections(b1, b2, t):
    """(bc1, bc2s) after t updates as adam_prep_kernel leaves them: the powers of the float32 betas as running double
    products, 1 - p1 and sqrt(1 - p2) in double, rounded to float32 once."""
    p1 = p2 = 1.0
    for _ in range(int(t)):
        p1 *= float(f32(b1))
        p2 *= float(f32(b2))
    return f32(1.0 - p1), f32(np.sqrt(1.0 - p2))


def state_bytes(b1, b2, t):
    """The 32 bytes of a step state after t updates."""
    p1 = p2 = 1.0
    for _ in range(int(t)):
        p1 *= float(f32(b1))
        p2 *= float(f32(b2))
    bc1, bc2s = corrections(b1, b2, t) if t else (f32(0), f32(0))
    return struct.pack(STATE_FMT, p1, p2, int(t), float(bc1), float(bc2s)) + b"\0" * 4


def round32(x):
    """A Fraction rounded to the nearest float32, ties to even (normal range)."""
    c = f32(float(x))                       # within one float32 step of the answer: pick among it and its neighbours
    best = None
    for cand in (np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))):
        d = abs(fractions.Fraction(float(cand)) - x)
        even = (int(np.array(cand, f32).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, cand, even)
    return f32(best[1])


def fma32(a, b, c):
    """fmaf(a, b, c) per element of float32 arrays: the exact a * b + c, rounded once."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    out = np.empty(a.shape, f32)
    F = fractions.Fraction
    for i in np.ndindex(a.shape):
        out[i] = round32(F(float(a[i])) * F(float(b[i])) + F(float(c[i])))
    return out


def step32(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2s, gscale, coupled=False):
    """One update of float32 arrays with the header's roundings; returns (p, m, v).  coupled: the gdn_adam_step* element,
    whose one fma puts the decay into the scaled gradient, gi = fma32(wd, p, round32(g * gscale)), and whose final
    subtraction carries no decay."""
    p, g, m, v = (np.asarray(a, f32) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, bc1, bc2s, gscale = (f32(x) for x in (lr, b1, b2, eps, wd, bc1, bc2s, gscale))
    with np.errstate(all="ignore"):
        step = lr / bc1
        gi = fma32(wd, p, g * gscale) if coupled else g * gscale
        mi = b1 * m + (f32(1) - b1) * gi
        vi = b2 * v + ((f32(1) - b2) * gi) * gi
        q = (step * mi) / (np.sqrt(vi) / bc2s + eps)
        assert all(a.dtype == f32 for a in (gi, mi, vi, q))
        return (p - q if coupled else p - fma32(dec32(lr, wd), p, q)), mi, vi


def run32(p, g, m, v, hyper, steps, coef=None, t0=0, coupled=False):
    """`steps` updates from update count t0 with one gradient; hyper = (lr, b1, b2, eps, wd, grad_scale); under a guard the
    gradient scale is float32(grad_scale * coef)."""
    lr, b1, b2, eps, wd, gs = hyper
    gscale = f32(gs) if coef is None else f32(gs) * f32(coef)
    for t in range(t0 + 1, t0 + steps + 1):
        bc1, bc2s = corrections(b1, b2, t)
        p, m, v = step32(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2s, gscale, coupled=coupled)
    return p, m, v


def step64(p, g, m, v, lr, b1, b2, eps, wd, t, gscale=1.0):
    """The same element in float64 (numpy arrays), t = 1, 2, ... the index of this update; returns (p, m, v)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    bc1, bc2s = 1.0 - b1 ** t, np.sqrt(1.0 - b2 ** t)
    gi = g * gscale
    mi = b1 * m + (1.0 - b1) * gi
    vi = b2 * v + (1.0 - b2) * gi * gi
    q = (lr / bc1) * mi / (np.sqrt(vi) / bc2s + eps)
    return p - ((lr * wd) * p + q), mi, vi


def ulps32(a, b):
    """Distance of two float32 arrays in units in the last place (same-sign finite values)."""
    ia = np.asarray(a, f32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, f32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)
