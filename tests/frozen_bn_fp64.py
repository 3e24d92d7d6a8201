"""Float64 restatement of a BatchNorm layer that is TRAINED on frozen statistics (--freeze_bn): out = [relu](y*scale + shift)
with scale / shift from the running statistics, and its backward with parameter gradients.  numpy only; the references of
tests/test_frozen_bn_cpu.py (checked there against torch's float64 autograd) and tests/test_hip_frozen_bn.py."""
import numpy as np

from pointwise_fp64 import bn_preact, f64


def coeffs(gamma, beta, running_mean, running_var, eps=1e-5):
    """[scale, shift, mean, invstd]: scale = gamma * invstd, shift = beta - running_mean * scale, mean = running_mean,
    invstd = 1 / sqrt(running_var + eps)."""
    invstd = 1.0 / np.sqrt(f64(running_var) + eps)
    scale = f64(gamma) * invstd
    return np.stack((scale, f64(beta) - f64(running_mean) * scale, f64(running_mean), invstd))


def bwd(dout, y, scale, shift, mean, invstd, relu=False):
    """dz = dout * [y*scale + shift > 0] (gradient 0 AT 0, as torch), xhat = (y - mean) * invstd:
    dy = scale * dz, dbeta = sum dz, dgamma = sum dz * xhat (sums over every axis but the last).
    Also abs1 = sum |dz| and abs2 = sum |dz * xhat|, the scale of the sums' rounding error."""
    dz = f64(dout).copy()
    yy = f64(y)
    C = yy.shape[-1]
    if relu:
        dz[~(bn_preact(yy, scale, shift) > 0.0)] = 0.0
    xh = (yy - f64(mean)) * f64(invstd)
    t2 = dz * xh
    return {"dz": dz, "xhat": xh, "dy": f64(scale) * dz, "dbeta": dz.reshape(-1, C).sum(0), "dgamma": t2.reshape(-1, C).sum(0),
            "abs1": np.abs(dz).reshape(-1, C).sum(0), "abs2": np.abs(t2).reshape(-1, C).sum(0), "n": yy.size // C}
