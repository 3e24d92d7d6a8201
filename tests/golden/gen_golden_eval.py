#!/usr/bin/env python3
"""Generate tests/golden/metrics_eval.npz: the reference's compute_errors_NYU (crop on and off) and
compute_errors_Make3D on seeded inputs, run on torch CPU; and tests/golden/metrics_edges.npz: the reference's
compute_errors, compute_errors_NYU (both crop on and off) and compute_errors_Make3D, image by image, on the edge inputs
of tests/eval_numpy.py::EDGE_CASES, plus compute_errors on the inputs of metrics_eval.npz.

Like gen_golden.py this runs only where the reference sources are available; it imports the reference's
calculate_error with cv2 stubbed (gen_golden.py's recipe) and stores data only.

    python -B tests/golden/gen_golden_eval.py          # writes both files
    python -B tests/golden/gen_golden_eval.py edges    # writes tests/golden/metrics_edges.npz only (or: eval)

The inputs are not stored: tests/eval_numpy.py::golden_inputs rebuilds them bit for bit from a seed, and
``<case>_digest`` pins them.  Stored per case: ``<case>_nyu_crop`` [8], ``<case>_nyu_nocrop`` [8], ``<case>_make3d`` [4]
for the whole batch and ``..._per`` [B,n] image by image (so a test may check any sub-batch).

metrics_edges.npz stores per edge case ``<case>_digest`` and ``<case>_kitti_crop_per``, ``_kitti_nocrop_per``,
``_nyu_crop_per``, ``_nyu_nocrop_per`` [B,8] and ``_make3d_per`` [B,4]: one call per image, a row of NaN where the
reference raises (no valid pixel: torch.median of an empty tensor).  For the cases of metrics_eval.npz it stores
``<case>_kitti_crop``, ``_kitti_nocrop`` [8] and their ``_per`` [B,8].
"""
import pathlib
import sys

sys.dont_write_bytecode = True
HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from eval_numpy import EDGE_CASES, GOLDEN_CASES, edge_inputs, golden_inputs, inputs_digest  # noqa: E402
from gen_golden import REF, _stub  # noqa: E402


def import_calculate_error():
    _stub("cv2")
    sys.path.insert(0, REF)
    import calculate_error
    return calculate_error


def _rows(fn, n, B):
    """fn(b) -> the reference's metrics of image b alone; NaN where it raises."""
    rows = []
    for b in range(B):
        try:
            rows.append(fn(slice(b, b + 1)))
        except (RuntimeError, IndexError) as e:
            print("   image %d: the reference raises (%s)" % (b, str(e).splitlines()[0][:60]))
            rows.append([float("nan")] * n)
    return np.array(rows, np.float64)


def write_edges(ce):
    out = {}
    for case in [c[0] for c in EDGE_CASES]:
        arrays = edge_inputs(case)
        s, g, p = (torch.from_numpy(a) for a in arrays)
        B = g.shape[0]
        out[case + "_digest"] = np.array(inputs_digest(arrays))
        for crop, tag in ((True, "crop"), (False, "nocrop")):
            out["%s_kitti_%s_per" % (case, tag)] = _rows(lambda i: ce.compute_errors(s[i], g[i], p[i], crop=crop), 8, B)
            out["%s_nyu_%s_per" % (case, tag)] = _rows(lambda i: ce.compute_errors_NYU(g[i], p[i], crop=crop), 8, B)
        out[case + "_make3d_per"] = _rows(lambda i: ce.compute_errors_Make3D(s[i], g[i], p[i]), 4, B)
        print(case, out[case + "_kitti_crop_per"][0].round(4))
    for name, B, H, W, levels in GOLDEN_CASES:
        s, g, p = (torch.from_numpy(a) for a in golden_inputs(name))
        for crop, tag in ((True, "crop"), (False, "nocrop")):
            out["%s_kitti_%s" % (name, tag)] = np.array(ce.compute_errors(s, g, p, crop=crop), np.float64)
            out["%s_kitti_%s_per" % (name, tag)] = _rows(lambda i: ce.compute_errors(s[i], g[i], p[i], crop=crop), 8, B)
    out["cases"] = np.array([c[0] for c in EDGE_CASES])
    np.savez_compressed(HERE / "metrics_edges.npz", **out)
    print("wrote", HERE / "metrics_edges.npz", (HERE / "metrics_edges.npz").stat().st_size, "bytes")


def main():
    ce = import_calculate_error()
    which = sys.argv[1:] or ["eval", "edges"]
    if "edges" in which:
        write_edges(ce)
    if "eval" not in which:
        return
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
