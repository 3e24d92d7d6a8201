"""The one streaming skeleton under gdn_ema_update, gdn_swap_f32 and gdn_grad_accumulate (stream2_kernel in optim.hip),
at the sizes where its head / 16-byte body / tail split can go wrong and at every pair of base offsets: bit for bit against
the restatement each kernel's own test uses (tests/ema_fp64.py's float32 difference and one fused multiply-add; numpy's exact
exchange and float32 add), and the elements on both sides of both ranges keep their old bits."""
import numpy as np
import pytest
import torch

import ema_fp64 as R

pytestmark = pytest.mark.gpu

# one element, fewer than a body lane's four, exactly four, one past; head + body + tail inside one wave and inside two blocks;
# two full blocks of 16-byte lanes plus a tail (the grid then has three blocks on the 16-byte form, nine on the scalar one)
SIZES = [1, 3, 4, 5, 67, 259, 2 * 256 * 4 + 7]
PAD = 8                       # canary floats on either side of an operand (a multiple of 4: the offset decides the alignment)
DECAY, T = 0.999, 3
PAIRS = [(a, b) for a in range(4) for b in range(4)]          # equal: the 16-byte form; different: the scalar form


@pytest.fixture(scope="module")
def pool():
    """Two seeded host buffers every size and offset is a slice of, made once and never written."""
    rng = np.random.default_rng(20261020)
    n = max(SIZES) + 3 + 2 * PAD
    return tuple((rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)).astype(np.float32) for _ in range(2))


def _fma32(w, d, e):
    """float32(w * d + e) with ONE rounding, for float32 operands: the product is exact in float64, the sum is rounded to odd
    there (Knuth's two-sum gives what the float64 addition lost), which the final rounding to float32 cannot tell from the
    exact sum.  R.update32 is this without the round-to-odd step."""
    prod = np.float64(w) * d.astype(np.float64)
    e = e.astype(np.float64)
    s = prod + e
    bb = s - prod
    lost = (prod - (s - bb)) + (e - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((lost != 0.0) & even, np.nextafter(s, np.where(lost > 0.0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _expected(op, a, b):
    if op == "ema":
        return _fma32(R.weight(DECAY, T), (b - a).astype(np.float32), a), b
    if op == "swap":
        return b, a
    return (a + b).astype(np.float32), b


def _launch(op, a, b):
    from gdn_amd import ops
    if op == "ema":
        state = torch.frombuffer(bytearray(R.state_record(T)), dtype=torch.uint8).to(a.device)
        ops.ema_update(a, b, DECAY, state)
    elif op == "swap":
        ops.swap_(a, b)
    else:
        ops.grad_accumulate(a, b)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", ["ema", "swap", "accumulate"])
def test_every_size_and_offset_bit_for_bit(gpu, pool, op, n):
    ha, hb = pool
    m = n + 3 + 2 * PAD
    a0, b0 = torch.from_numpy(ha[:m]).to(gpu), torch.from_numpy(hb[:m]).to(gpu)
    for oa, ob in PAIRS:
        abuf, bbuf = a0.clone(), b0.clone()
        a, b = abuf[PAD + oa:PAD + oa + n], bbuf[PAD + ob:PAD + ob + n]
        assert a.data_ptr() % 16 == 4 * oa and b.data_ptr() % 16 == 4 * ob
        _launch(op, a, b)
        want_a, want_b = _expected(op, ha[PAD + oa:PAD + oa + n], hb[PAD + ob:PAD + ob + n])
        what = "%s n=%d offsets (%d, %d)" % (op, n, oa, ob)
        for name, buf, orig, off, want in (("a", abuf, a0, oa, want_a), ("b", bbuf, b0, ob, want_b)):
            got = buf.cpu().numpy().view(np.int32)
            assert np.array_equal(got[PAD + off:PAD + off + n], want.view(np.int32)), "%s: %s differs" % (what, name)
            old = orig.cpu().numpy().view(np.int32)
            assert np.array_equal(got[:PAD + off], old[:PAD + off]), "%s: elements before %s changed" % (what, name)
            assert np.array_equal(got[PAD + off + n:], old[PAD + off + n:]), "%s: elements after %s changed" % (what, name)
