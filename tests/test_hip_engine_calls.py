"""engine.py against tests/golden/engine_calls.json: in every configuration of tests/golden/gen_engine_calls.py one forward and
one backward make the recorded calls into the C library -- the same entry points in the same order with the same geometries,
sizes, flags and null / non-null pointers.  The recording was written by the commit before conv_bn_act was split up."""
import importlib.util
import pathlib

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


def _load():
    spec = importlib.util.spec_from_file_location("gen_engine_calls", GOLDEN / "gen_engine_calls.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load()


@pytest.fixture(scope="module")
def recorded():
    return G.decode((GOLDEN / "engine_calls.json").read_text())


def test_recording_lists_every_configuration(recorded):
    assert list(recorded) == list(G.CONFIGS)


@pytest.mark.parametrize("name", list(G.CONFIGS))
def test_calls_match_the_recording(gpu, recorded, name):
    got = G.run_config(name, gpu)
    for part in ("fwd", "bwd"):
        want, have = recorded[name][part], got[part]
        for i, (w, h) in enumerate(zip(want, have)):
            if w != h:
                print("%s %s: first difference at call %d\n  recorded %s\n  now      %s" % (name, part, i, w, h))
                assert w == h, "%s %s: call %d differs" % (name, part, i)
        if len(want) != len(have):
            longer = want if len(want) > len(have) else have
            print("%s %s: %d calls recorded, %d now; the first extra one (%s): %s" % (
                name, part, len(want), len(have), "recorded" if longer is want else "now", longer[min(len(want), len(have))]))
        assert len(want) == len(have), "%s %s: %d calls recorded, %d now" % (name, part, len(want), len(have))
