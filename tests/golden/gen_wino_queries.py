#!/usr/bin/env python3
"""Recorded results of the host-side queries of the 3x3 Winograd layer (csrc/conv_wino.hip), for
tests/test_winoconv_queries_cpu.py: gdn_winoconv_state_bytes, _fwd_workspace_bytes, _bwd_workspace_bytes,
_bwd_pair_workspace_bytes, _stats_slots and _bnb_slots over a grid of geometries and hints.

The queries size buffers that callers allocate and the entry points carve, so a change of the host code must keep every
number.  Run it against the library whose numbers are the reference (the parent of the change under test); no GPU needed:

    GDN_HIP_LIB=/path/to/parent/libgdn_hip.so python tests/golden/gen_wino_queries.py [OUT.npz]

The file holds `geoms` (int32 [rows, 11]: the fields of gdn_conv_geom in order) and `results` (int64 [rows, 6]: the queries
in the order of QUERIES).  The test imports the grid from here, so both sides ask the same questions.
"""
import ctypes
import itertools
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
DEFAULT_OUT = HERE / "wino_queries.npz"

QUERIES = ["gdn_winoconv_state_bytes", "gdn_winoconv_fwd_workspace_bytes", "gdn_winoconv_bwd_workspace_bytes",
           "gdn_winoconv_bwd_pair_workspace_bytes", "gdn_winoconv_stats_slots", "gdn_winoconv_bnb_slots"]
NO_X3, NO_WINO_F4, FLIP_TAPS = 2, 4, 32          # GDN_HINT_* (include/gdn_hip.h)
BATCHES = [1, 2, 3, 20]
CHANNELS = [64, 128, 256, 512]
SIZES = [(1, 7), (2, 2), (3, 16), (4, 4), (5, 6), (8, 12), (9, 13), (8, 26), (16, 52), (32, 104)]
HINTS = [0, NO_X3, NO_WINO_F4, FLIP_TAPS, NO_X3 | NO_WINO_F4]
# (B, H, W, Cin, Cout, k, stride, pad, pad_mode, transposed, hints) that the layer refuses: 5x5, stride 2, 192 channels (no
# power-of-two multiple of 64) on either side, a transposed layer, pad 0, 1024 channels
REJECTED = [(2, 8, 12, 128, 128, 5, 1, 2, 0, 0, 0), (2, 8, 12, 128, 128, 3, 2, 1, 0, 0, 0), (2, 8, 12, 192, 128, 3, 1, 1, 0, 0, 0),
            (2, 8, 12, 128, 192, 3, 1, 1, 1, 0, 0), (2, 8, 12, 128, 128, 3, 1, 1, 0, 1, 0), (2, 8, 12, 128, 128, 3, 1, 0, 0, 0, 0),
            (2, 8, 12, 1024, 128, 3, 1, 1, 0, 0, 0)]


def grid():
    """Every geometry of the grid as the 11 fields of gdn_conv_geom."""
    rows = [(B, H, W, ci, co, 3, 1, 1, pm, 0, h)
            for B, ci, co, (H, W), pm, h in itertools.product(BATCHES, CHANNELS, CHANNELS, SIZES, (0, 1), HINTS)]
    return np.array(rows + REJECTED, dtype=np.int32)


def ask(geoms):
    """The six queries for every row, from the library gdn_amd._lib loads (GDN_HIP_LIB, or the tree's own)."""
    from gdn_amd._lib import ConvGeom, lib
    fns = [getattr(lib, q) for q in QUERIES]
    out = np.empty((len(geoms), len(QUERIES)), dtype=np.int64)
    for i, row in enumerate(geoms):
        g = ConvGeom(*[int(v) for v in row])
        out[i] = [int(fn(ctypes.byref(g))) for fn in fns]
    return out


def main():
    sys.path.insert(0, str(HERE.parent.parent / "gdn-pytorch_amd"))
    geoms = grid()
    results = ask(geoms)
    out = pathlib.Path(sys.argv[1]) if len(sys.argv) > 1 else DEFAULT_OUT
    np.savez_compressed(out, geoms=geoms, results=results)
    print("wrote %s: %d rows (%d supported), %d bytes" % (out, len(geoms), int((results[:, 0] > 0).sum()), out.stat().st_size))


if __name__ == "__main__":
    main()
