"""The fused Adam against a state its own earlier revision left on an MI355X (tests/golden/optim_state_v1.pt, written by
tests/golden/gen_optim_state.py at the commit before the state stores became one type): weights, moments, averages, host
counts, device step states and guard counts after five steps -- one-launch, clipped, per-tensor, skipped, with a
caller-owned gradient -- bit for bit, for the guarded + averaged optimizer and for the host-path one.  The update is
elementwise and the norm's reduction order is a function of n alone, so the tiny arena is the whole case."""
import importlib.util

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _load_gen():
    spec = importlib.util.spec_from_file_location("gen_optim_state", GOLDEN / "gen_optim_state.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load_gen()


@pytest.fixture(scope="module")
def stored():
    return torch.load(G.PATH, weights_only=True)


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _same(got, want, where):
    """Recursive and bitwise: the same types, keys and lengths, equal numbers, tensors of one dtype, shape and content."""
    assert type(got) is type(want), "%s: %s / %s" % (where, type(got).__name__, type(want).__name__)
    if torch.is_tensor(want):
        assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s / %s %s" % (
            where, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
        assert torch.equal(_bits(got), _bits(want)), "%s: %d of %d elements differ" % (where, int((got != want).sum()), want.numel())
    elif isinstance(want, dict):
        assert list(got) == list(want), "%s: keys %s / %s" % (where, list(got), list(want))
        for k in want:
            _same(got[k], want[k], "%s[%r]" % (where, k))
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), "%s: %d / %d entries" % (where, len(got), len(want))
        for k, (a, b) in enumerate(zip(got, want)):
            _same(a, b, "%s[%d]" % (where, k))
    else:
        assert got == want, "%s: %r / %r" % (where, got, want)


@pytest.mark.parametrize("form", list(G.FORMS))
def test_from_scratch(gpu, stored, form):
    """All steps from the seeded start: the state, weights and averages stored after step 3 and after step 5."""
    params, ar, opt = G.make(gpu, form)
    _same([p.detach().cpu() for p in params], stored[form]["initial"], form + " initial weights")
    got = G.run(form, params, ar, opt, G.STEPS[form])
    for when in ("after3", "after5"):
        _same(got[when], stored[form][when], "%s %s" % (form, when))


@pytest.mark.parametrize("form", list(G.FORMS))
def test_resumed_from_the_stored_state(gpu, stored, form):
    """New objects take the stored step-3 weights and state, then the remaining steps: the stored step-5 snapshot."""
    at3 = stored[form]["after3"]
    params, ar, opt = G.make(gpu, form, weights=at3["weights"])
    opt.load_state_dict(at3["state"])
    got = G.run(form, params, ar, opt, [k for k in G.STEPS[form] if k > 3])
    _same(got["after5"], stored[form]["after5"], form + " resumed, after5")


@pytest.mark.parametrize("form", list(G.FORMS))
def test_stored_state_loads_and_comes_back_before_any_step(gpu, stored, form):
    at5 = stored[form]["after5"]
    params, ar, opt = G.make(gpu, form, weights=at5["weights"])
    opt.load_state_dict(at5["state"])
    _same(G.to_cpu(opt.state_dict()), at5["state"], form + " state_dict() of a fresh optimizer after load_state_dict()")
