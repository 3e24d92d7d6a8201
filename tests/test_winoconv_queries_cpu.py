"""CPU-side check of the 3x3 Winograd layer's host queries (csrc/conv_wino.hip): state, forward / backward / two-chain
backward workspace bytes, BatchNorm and BatchNorm-backward partial slots return, for every geometry and hint of the grid in
tests/golden/gen_wino_queries.py, the numbers recorded there from the library before the host side was rebuilt around one
workspace layout per entry point.  Callers allocate by these numbers and the entry points carve by the same layouts."""
import importlib.util
import pathlib

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("gen_wino_queries", REPO / "tests" / "golden" / "gen_wino_queries.py")
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def asked():
    spec = importlib.util.spec_from_file_location("gdn_build", REPO / "gdn-pytorch_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    rec = np.load(G.DEFAULT_OUT, allow_pickle=False)
    return rec["geoms"], rec["results"], G.ask(G.grid())


def test_recorded_grid_is_the_generators(asked):
    geoms, results, _ = asked
    assert np.array_equal(geoms, G.grid())
    assert results.shape == (len(geoms), len(G.QUERIES))
    # the record is not vacuous: most of the grid is supported, F(4x4,3x3) and reflection plans are in it, the refused rows are refused
    assert (results[:, 0] > 0).sum() > len(geoms) // 2
    assert (results[:, 3] > 0).any() and (results[(geoms[:, 8] == 1) & (results[:, 0] > 0), 5] == 0).all()
    assert (results[-len(G.REJECTED):, :4] == 0).all()


@pytest.mark.parametrize("q", range(len(G.QUERIES)), ids=G.QUERIES)
def test_query_returns_the_recorded_numbers(asked, q):
    geoms, results, got = asked
    bad = np.nonzero(got[:, q] != results[:, q])[0]
    assert bad.size == 0, "%s: %d of %d rows differ, first %s: %d, recorded %d" % (
        G.QUERIES[q], bad.size, len(geoms), geoms[bad[0]].tolist(), got[bad[0], q], results[bad[0], q])
