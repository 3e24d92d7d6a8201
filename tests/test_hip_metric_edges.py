"""GPU tests of the three reference-protocol metric kernels (csrc/metrics.hip: compute_errors, compute_errors_NYU,
compute_errors_Make3D) at the edges: images smaller than, equal to and just above the 1024-thread workgroup, one and two
valid pixels, medians on ties and across a radix bucket, thresholds hit exactly, non-finite and constant inputs.

The yardstick is the float64 numpy restatement (eval_numpy.py), which test_eval_cpu.py pins to the reference's own
results on these very inputs (metrics_edges.npz).  The bars (eval_numpy.row_mismatch):
  * NaN positions identical;
  * a1, a2, a3 bit-equal to float32(count / nvalid): every decision is float32, operation by operation;
  * abs_diff, abs_rel, sq_rel, rmse within one float32 step: the terms are the same float32 numbers, the float64 sums
    differ only in order (n 2^-53), the result is rounded to float32 once;
  * rmse_log, log10, ave_log10 within LOG_BAR, relative: they rest on the device's logf / log10f against numpy's."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eval_numpy as E

pytestmark = pytest.mark.gpu

EDGE_NAMES = [c[0] for c in E.EDGE_CASES]
# Largest relative deviation of a log metric from the restatement over the edge set, measured on an MI355X: 3.54e-7
# (ave_log10 of `thresh` under Make3D: 0.23914360 for 0.23914368).  The bar is four times that, 1.416e-6, which stays
# below the cap of 1e-5 that the restatement itself is held to against the reference.
LOG_MEASURED = 3.54e-7
LOG_BAR = min(4 * LOG_MEASURED, 1e-5)
COMBOS = [("kitti", True), ("kitti", False), ("nyu", True), ("nyu", False), ("make3d", None)]


def _restated(kind, crop, s, g, p):
    if kind == "kitti":
        return E.kitti_per_image(s, g, p, crop)
    if kind == "nyu":
        return E.nyu_per_image(g, p, crop)
    return E.make3d_per_image(s, g, p)


def _kernel(kind, crop, s, g, p):
    """float32 row of batch means straight from the device."""
    from gdn_amd import calculate_error as C
    if kind == "kitti":
        t = C.compute_errors_device(s, g, p, crop)
    elif kind == "nyu":
        t = C.compute_errors_NYU_device(g, p, crop)
    else:
        t = C.compute_errors_Make3D_device(s, g, p)
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _rows(case):
    """{(kind, crop): (want [B,n] float64 from the restatement, got [B,n] float32 from B launches of one image)}; computed
    once per case and shared by the tests below."""
    arrays = E.edge_inputs(case)
    dev = [torch.from_numpy(a).to("cuda:0") for a in arrays]
    out = {}
    for kind, crop in COMBOS:
        want = _restated(kind, crop, *arrays)
        got = np.stack([_kernel(kind, crop, *(t[b:b + 1] for t in dev)) for b in range(want.shape[0])])
        out[kind, crop] = (want, got)
    return out


@pytest.mark.parametrize("case", EDGE_NAMES)
def test_edge_case_image_by_image(gpu, golden, case):
    assert E.inputs_digest(E.edge_inputs(case)) == str(golden["metrics_edges"][case + "_digest"])
    bad = []
    for (kind, crop), (want, got) in _rows(case).items():
        assert got.dtype == np.float32 and got.shape == want.shape
        for b in range(want.shape[0]):
            bad += ["%s crop=%s image %d %s" % (kind, crop, b, m) for m in E.row_mismatch(got[b], want[b], kind, LOG_BAR)]
    assert not bad, "\n".join(bad)


def test_non_finite_rows_are_the_references(gpu, golden):
    """Spelled out against the reference's own rows: a diverged or constant prediction gives NaN sums and a1..a3 = 0, a NaN
    or constant ground truth NaN throughout, a NaN in the sparse map costs one pixel."""
    g = golden["metrics_edges"]
    for case in ("pred_nan", "pred_inf", "pred_all_nan", "pred_const", "gt_nan", "gt_const", "sparse_nan"):
        for (kind, crop), (_, got) in _rows(case).items():
            ref = g["%s_%s%s_per" % (case, kind, {True: "_crop", False: "_nocrop", None: ""}[crop])]
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (case, kind, crop, got, ref)
            if case.startswith("pred") and kind != "make3d":
                assert np.isnan(got[0, [0, 1, 2, 6, 7]]).all() and (got[0, 3:6] == 0).all(), (case, kind, got)
            if case.startswith("gt"):
                assert np.isnan(got).all(), (case, kind, got)
    assert np.isfinite(_rows("sparse_nan")["kitti", True][1]).all()


def test_log_metrics_deviation(gpu):
    """The largest relative deviation of rmse_log / log10 / ave_log10 from the restatement over the whole edge set, printed
    so that it can be measured again, and held to LOG_BAR = min(4 x LOG_MEASURED, 1e-5) = 1.416e-6 (measured on an MI355X:
    3.54e-7; a log metric that is exactly 0 must come out as 0)."""
    worst, where = 0.0, None
    for case in EDGE_NAMES:
        for (kind, crop), (want, got) in _rows(case).items():
            for c in E.COLUMNS[kind]["log"]:
                for b in range(want.shape[0]):
                    w, v = want[b, c], float(got[b, c])
                    if np.isnan(w) or w == v:
                        continue
                    dev = abs(v - w) / abs(w) if w != 0 else float("inf")
                    if dev > worst:
                        worst, where = dev, (case, kind, crop, b, c, v, w)
    print("largest relative deviation of a log metric: %.3e at %s; bar %.3e" % (worst, where, LOG_BAR))
    assert LOG_BAR == min(4 * LOG_MEASURED, 1e-5) < 1e-5
    assert worst <= LOG_BAR, (worst, where)


FINITE_16x24 = ["s16x24", "two", "tie5_16x24", "tie7_16x24", "bucket_g", "bucket_p", "sparse_nan"]


@pytest.mark.parametrize("name", ["s32x104", "mixed", "finite_16x24"])
def test_edge_batches(gpu, name):
    """One launch over a batch: the float32 of the float64 mean of the per-image rows, NaN where one of them is NaN."""
    names = FINITE_16x24 if name == "finite_16x24" else [name]
    arrays = [np.concatenate(a) for a in zip(*(E.edge_inputs(n) for n in names))]
    dev = [torch.from_numpy(a).to(gpu) for a in arrays]
    assert arrays[0].shape[0] >= 2
    bad = []
    for kind, crop in COMBOS:
        want = _restated(kind, crop, *arrays).mean(0)
        got = _kernel(kind, crop, *dev)
        if name == "mixed":
            assert np.isnan(want).all()                     # image 3 has no valid pixel
        bad += ["%s crop=%s %s" % (kind, crop, m) for m in E.row_mismatch(got, want, kind, LOG_BAR, count_ulps=1)]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", ["kitti_tie", "nyu_tie"])
def test_kitti_kernel_on_tie_goldens(gpu, golden, case):
    """The 5- and 7-level inputs of metrics_eval.npz through the KITTI kernel: against the reference's compute_errors (whose
    float32 means carry their own rounding: the file's rtol 1e-5) and against the restatement at the bars above."""
    g = golden["metrics_edges"]
    arrays = E.golden_inputs(case)
    assert E.inputs_digest(arrays) == str(golden["metrics_eval"][case + "_digest"])
    dev = [torch.from_numpy(a).to(gpu) for a in arrays]
    for crop, tag in ((True, "crop"), (False, "nocrop")):
        want = E.kitti_per_image(*arrays, crop)
        got = _kernel("kitti", crop, *dev)
        np.testing.assert_allclose(got, g["%s_kitti_%s" % (case, tag)], rtol=1e-5)
        assert not E.row_mismatch(got, want.mean(0), "kitti", LOG_BAR, count_ulps=1)
        for b in range(want.shape[0]):
            one = _kernel("kitti", crop, *(t[b:b + 1] for t in dev))
            np.testing.assert_allclose(one, g["%s_kitti_%s_per" % (case, tag)][b], rtol=1e-5)
            assert not E.row_mismatch(one, want[b], "kitti", LOG_BAR), (case, crop, b)


@pytest.mark.parametrize("name", ["gdn_depth_metrics", "gdn_depth_metrics_nyu", "gdn_depth_metrics_make3d"])
def test_metrics_refuse_images_beyond_int32(gpu, name):
    """H * W > INT32_MAX is GDN_ERR_BAD_ARG before anything else is looked at: the pointers are dummies, nothing of that size
    exists, and the workspace size of 0 would stop a library without the guard short of a launch as well."""
    from gdn_amd import _lib as L
    P = ctypes.c_void_p(16)
    ptrs = (P, P) if name.endswith("nyu") else (P, P, P)
    crop = () if name.endswith("make3d") else (1,)
    for H, W in ((65536, 65536), (46341, 46341), (2 ** 31 - 1, 2), (1, 2 ** 31 - 1)):
        rc = L.lib.raw(name)(*ptrs, 1, H, W, *crop, P, P, 0, None)
        assert rc == (-1 if H * W > 2 ** 31 - 1 else -3), (name, H, W, rc)     # BAD_ARG, else (at INT32_MAX) WORKSPACE
