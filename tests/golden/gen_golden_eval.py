#!/usr/bin/env python3
"""Generate tests/golden/metrics_eval.npz: the reference's compute_errors_NYU (crop on and off) and
compute_errors_Make3D on seeded inputs, run on torch CPU.

Like gen_golden.py this runs only where the reference sources are available; it imports the reference's
calculate_error with cv2 stubbed (gen_golden.py's recipe) and stores data only.

    python -B tests/golden/gen_golden_eval.py          # writes tests/golden/metrics_eval.npz

The inputs are not stored: tests/eval_numpy.py::golden_inputs rebuilds them bit for bit from a seed, and
``<case>_digest`` pins them.  Stored per case: ``<case>_nyu_crop`` [8], ``<case>_nyu_nocrop`` [8], ``<case>_make3d`` [4]
for the whole batch and ``..._per`` [B,n] image by image (so a test may check any sub-batch).
"""
import pathlib
import sys

sys.dont_write_bytecode = True
HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from eval_numpy import GOLDEN_CASES, golden_inputs, inputs_digest  # noqa: E402
from gen_golden import REF, _stub  # noqa: E402


def import_calculate_error():
    _stub("cv2")
    sys.path.insert(0, REF)
    import calculate_error
    return calculate_error


def main():
    ce = import_calculate_error()
    out = {}
    for name, B, H, W, levels in GOLDEN_CASES:
        arrays = golden_inputs(name)
        s, g, p = (torch.from_numpy(a) for a in arrays)
        out[name + "_digest"] = np.array(inputs_digest(arrays))
        out[name + "_nyu_crop"] = np.array(ce.compute_errors_NYU(g, p, crop=True), np.float64)
        out[name + "_nyu_nocrop"] = np.array(ce.compute_errors_NYU(g, p, crop=False), np.float64)
        out[name + "_make3d"] = np.array(ce.compute_errors_Make3D(s, g, p), np.float64)
        out[name + "_nyu_crop_per"] = np.array([ce.compute_errors_NYU(g[b:b + 1], p[b:b + 1], crop=True)
                                                for b in range(B)], np.float64)
        out[name + "_nyu_nocrop_per"] = np.array([ce.compute_errors_NYU(g[b:b + 1], p[b:b + 1], crop=False)
                                                  for b in range(B)], np.float64)
        out[name + "_make3d_per"] = np.array([ce.compute_errors_Make3D(s[b:b + 1], g[b:b + 1], p[b:b + 1])
                                              for b in range(B)], np.float64)
        print(name, out[name + "_nyu_crop"].round(4), out[name + "_make3d"].round(4))
    out["cases"] = np.array([c[0] for c in GOLDEN_CASES])
    np.savez_compressed(HERE / "metrics_eval.npz", **out)
    print("wrote", HERE / "metrics_eval.npz", (HERE / "metrics_eval.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
