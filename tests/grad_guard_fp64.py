"""numpy float64 restatement of the gradient guard's device record (include/gdn_hip.h: gdn_grad_sumsq,
gdn_grad_guard_finalize), written from the specification and independent of the kernels.  The GPU tests
(test_hip_grad_guard.py) compare the kernels against it; test_grad_guard_cpu.py checks the restatement itself.

Record: { double sumsq; float norm; float coef; int32 skip; int32 steps; int32 clipped; int32 skipped; } -- 32 bytes."""
import struct

import numpy as np

RECORD_FMT = "<dffiiii"
RECORD_BYTES = struct.calcsize(RECORD_FMT)
U23 = 2.0 ** -23          # one float32 ulp relative to 1: the bar for a double result rounded once to float


def new_record():
    return {"sumsq": 0.0, "norm": np.float32(0.0), "coef": np.float32(0.0), "skip": 0, "steps": 0, "clipped": 0, "skipped": 0}


def unpack(raw):
    """The record's fields from its 32 bytes."""
    sumsq, norm, coef, skip, steps, clipped, skipped = struct.unpack(RECORD_FMT, bytes(raw))
    return {"sumsq": sumsq, "norm": np.float32(norm), "coef": np.float32(coef), "skip": skip, "steps": steps,
            "clipped": clipped, "skipped": skipped}


def sumsq(g):
    """Sum of squares of float32 values, each converted to float64 before squaring (1e30 squared is finite), summed in
    float64 (pairwise: its error is far below the 2^-53 n bound the tests allow for the device's order).  A NaN or an Inf
    anywhere makes it non-finite."""
    g = np.asarray(g, dtype=np.float32).astype(np.float64).ravel()
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sum(g * g))


def accumulate(rec, g, accumulate=False):
    with np.errstate(over="ignore", invalid="ignore"):
        rec["sumsq"] = (rec["sumsq"] if accumulate else 0.0) + sumsq(g)
    return rec


def norm64(total_sumsq, grad_scale=1.0):
    """The float64 norm of the gradient as the update sees it: sqrt(sumsq) * |float32(grad_scale)|."""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sqrt(np.float64(total_sumsq)) * abs(np.float64(np.float32(grad_scale))))


def coef64(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient for a FINITE norm, in float64; max_norm <= 0: no clipping."""
    return min(1.0, float(max_norm) / (float(norm) + 1e-6)) if max_norm > 0 else 1.0


def finalize(rec, grad_scale=1.0, max_norm=0.0, skip_nonfinite=False):
    """The four branches and the counters; norm and coef are rounded once to float32."""
    norm = norm64(rec["sumsq"], grad_scale)
    skip, coef = 0, 1.0
    if np.isfinite(norm):
        coef = coef64(norm, max_norm)
    elif skip_nonfinite:
        skip, coef = 1, 0.0
    with np.errstate(over="ignore"):
        rec["norm"] = np.float32(norm)
    rec["coef"] = np.float32(coef)
    rec["skip"] = skip
    rec["steps"] += 1
    if rec["coef"] < np.float32(1.0) and not skip:
        rec["clipped"] += 1
    rec["skipped"] += skip
    return rec
