"""The training loops' cadence (trainer.train_AE_DtoD / train_AE_RtoD) against a recording of it: tests/golden/loop_cadence.json,
written by tests/golden/gen_loop_cadence.py at the commit before the two loop bodies became one driver.  Each scenario runs
a loop on the CPU with its heavy parts replaced (see the generator) and compares, in this order, the printed lines, the
sparse events -- learning-rate writes, checkpoint paths, state-file progress dicts, validations, each with its position in
the stream -- and the sha256 of the whole stream of zero_grad / backward / sync / step(micro_batches) and sparse events.
The long scenarios reach every constant of the cadence: print 50 / 100, checkpoint 3000 / 700, decay at 1900 / 2200."""
import importlib.util
import pathlib

import pytest

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


def _load_gen():
    spec = importlib.util.spec_from_file_location("gen_loop_cadence", GOLDEN / "gen_loop_cadence.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _load_gen()
_ran = {}


def _run(name):
    if name not in _ran:
        _ran[name] = GEN.run_scenario(name)
    return _ran[name]


@pytest.fixture(scope="module")
def recorded():
    return GEN.parse(GEN.PATH.read_text())


def test_the_recording_holds_every_scenario(recorded):
    assert list(recorded) == list(GEN.SCENARIOS)


@pytest.mark.parametrize("name", list(GEN.SCENARIOS))
def test_loop_matches_the_recording(name, recorded):
    want, got = recorded[name], _run(name)
    assert got["error"] == want["error"]
    assert got["stdout"] == want["stdout"]
    assert got["events"] == want["events"]
    assert (got["dense_len"], got["dense_sha256"]) == (want["dense_len"], want["dense_sha256"])
    assert got["returns"] == want["returns"] and got["micro_batches"] == want["micro_batches"]


@pytest.mark.parametrize("name", ["refuse_graph_with_accum", "refuse_resume_other_k"])
def test_refusals_come_before_any_event(name):
    got = _run(name)
    assert got["error"][0] == "GdnError"
    assert [e for e in got["events"] if e[1] != "print"] == [] and got["dense_len"] == len(got["stdout"]) == 1
    assert got["stdout"] == ["Training for 2 epochs..."]


def test_the_long_scenarios_reach_every_cadence_constant():
    """What the sizes were chosen for, read off the runs themselves."""
    def kinds(name, kind):
        return [e for e in _run(name)["events"] if e[1] == kind]
    d, r = "dtod_cadence", "rtod_single_accum3"
    out = _run(d)["stdout"]
    assert "epoch: 1,  50/3800" in out and "epoch: 8,  3750/3800" in out
    assert len(kinds(d, "ckpt")) == 8 * 2 and len(kinds(d, "lr")) == 2 and len(kinds(d, "validate")) == 8
    states = [e[2] for e in kinds(d, "state")]
    assert {"epoch": 0, "i": 999, "model_num": 0, "seen": 2000, "step": 1000, "lr": 2e-5} in states        # every 1000 steps
    assert any(s["i"] == 2999 and s["model_num"] == 1 for s in states)                                   # on a checkpoint
    assert any(s["i"] == -1 and s["epoch"] == 8 for s in states)                                         # the epoch's end
    out = _run(r)["stdout"]
    assert "epoch: 1,  100/4400" in out and "epoch: 1,  50/4400" not in out
    assert len(kinds(r, "ckpt")) == 4 * 6 and len(kinds(r, "lr")) == 1
    states = [e[2] for e in kinds(r, "state")]
    assert [s["i"] for s in states if s["epoch"] == 0][:2] == [701, 1001]       # fell due inside a group: written at its end
    assert all(s["accum_steps"] == 3 for s in states)
    steps = _run(r)["dense_len"]
    assert steps > 4 * 4400 * 2
    assert [e[2] for e in kinds("rtod_single_short", "ckpt")] != [] and kinds("rtod_single_short", "state")[-1][2]["i"] == -1


def test_regenerating_reproduces_the_file_byte_for_byte():
    assert GEN.render({name: _run(name) for name in GEN.SCENARIOS}) == GEN.PATH.read_text()
