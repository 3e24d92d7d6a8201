"""The learning-rate schedule of gdn_lr_schedule (include/gdn_hip.h) restated in plain Python double: the
expressions of the header in the header's order, one IEEE operation each, so the kernel's warm-up, linear decay and final
product are these bits exactly; only cos() is another library's."""
import math
import struct

import numpy as np

KINDS = ("constant", "linear", "cosine")
STATE_FMT = "<ddiff"          # AdamDevState: { double beta1^t, beta2^t; int32 t; float bc1, bc2s; } + 4 bytes of padding
STATE_BYTES = 32


def s(u, kind, warmup, total, floor):
    """The factor on lr * lr_mult for the update with 0-based index u (= the number of updates applied so far)."""
    kind = KINDS.index(kind) if isinstance(kind, str) else int(kind)
    u, warmup, total, floor = int(u), int(warmup), int(total), float(floor)
    if u < warmup:
        return (float(u) + 1.0) / float(warmup)                     # w(u); d(u) = 1
    if kind == 0:
        return 1.0
    x = min(1.0, (float(u) - float(warmup)) / float(max(1, total - warmup)))
    shape = 1.0 - x if kind == 1 else 0.5 * (1.0 + math.cos(math.pi * x))
    return floor + (1.0 - floor) * shape


def rate32(base, u, kind, warmup, total, floor):
    """What the kernel stores: base * s(u) in double, rounded to float32 once."""
    return np.float32(float(base) * s(u, kind, warmup, total, floor))


def ulp32(x):
    """The spacing of float32 at |x| (of the smallest normal below it)."""
    return float(np.spacing(np.float32(max(abs(float(x)), float(np.finfo(np.float32).tiny)))))


def state_bytes(t, beta1=0.9, beta2=0.999):
    """The 32 bytes of a step state after t updates, as optim._step_state packs the first 28."""
    return struct.pack(STATE_FMT, float(beta1) ** t, float(beta2) ** t, int(t), 0.0, 0.0) + b"\0" * (STATE_BYTES - struct.calcsize(STATE_FMT))
