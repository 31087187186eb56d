"""tools/mul192_model.py chain(), the walk of fthe_gprod192 with the lazy remainder in [0, 2N) as the next multiplier
and the bounds re-derived for that range asserted, against Python's product mod N.  No GPU."""
from math import gcd

import pytest

import n2_edges as ne
from test_mul192_model import MODULI, mm          # the six edge moduli; tools/ on the path

TOP = (1 << 6144) - 1


@pytest.mark.parametrize("n", MODULI, ids=range(len(MODULI)))
def test_chain_reduces_exactly(n):
    """chains of 8 hostile rows that are units mod N (rows >= N among them), so that every step's bounds are asserted on
    a full-size remainder, from every offset, one lane by lane; chain() checks the result"""
    H = [x for x in ne.hostile_rows(n * n, bits=6144, nrand=2) if gcd(x, n * n) == 1]
    for j in range(len(H)):
        assert mm.chain((H + H)[j:j + 8], n, lanes=j == 9) > 0
    assert mm.chain([TOP] * 8, n) == pow(TOP, 8, n * n)
    assert mm.chain([], n) == 1 and mm.chain([TOP], n, lanes=True) == TOP % (n * n) and mm.chain([n * n, 5], n) == 0


@pytest.mark.parametrize("name, bad", [("SHIFT_A", mm.SHIFT_A - 1), ("mu_of", lambda N: (1 << 12312) // N - (1 << 30))])
def test_bounds_are_live(monkeypatch, name, bad):
    """a cut point one limb lower: z1 outgrows its bound; a mu 2^30 too small: q falls below floor(z / N) - 1"""
    monkeypatch.setattr(mm, name, bad)
    with pytest.raises(AssertionError):
        mm.chain([TOP - 1, TOP, TOP], MODULI[1])
