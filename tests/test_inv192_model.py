"""tools/mul192_model.py inverse(), the radix-8 walk of fthe_inv192_up / fthe_inv192_down with the Barrett bounds
asserted at every product, against Python's pow(x, -1, N).  No GPU."""
from math import gcd

import pytest

import n2_edges as ne
from test_mul192_model import MODULI, mm          # the six edge moduli; tools/ on the path


def _units(N, count):
    H = [x for x in ne.hostile_rows(N, bits=6144, nrand=count, seed=count) if gcd(x, N) == 1]
    return (H[-count // 2:] + H)[:count]          # random rows below N, then 1, 2, N - 1 and the rows >= N


@pytest.mark.parametrize("count", [1, 9, 65])
@pytest.mark.parametrize("n", MODULI, ids=range(len(MODULI)))
def test_inverse_is_exact(n, count):
    """the top alone, a last group of one, three levels; with and without a and an offset; the products counted"""
    N = n * n
    x, ran = _units(N, count), []
    assert mm.inverse(N, x, count=ran) == [pow(v, -1, N) for v in x]
    a = x[::-1]
    assert mm.inverse(N, x, a=a, offset=1 << 3071, n=n, count=ran) == [
        s * pow(t, -1, N) * (1 + (n << 3071)) % N for s, t in zip(a, x)]
    assert ran == [mm.inverse_products(count, False), mm.inverse_products(count, True)]


def test_inverse_lane_by_lane():
    N = MODULI[0] ** 2
    x = _units(N, 9)
    assert mm.inverse(N, x, a=x[1:] + x[:1], lanes=True) == [s * pow(t, -1, N) % N for s, t in zip(x[1:] + x[:1], x)]


def test_formulas():
    assert [mm.inverse_levels(c) for c in (1, 8, 9, 64, 65, 513)] == [[1], [8], [9, 2], [64, 8], [65, 9, 2], [513, 65, 9, 2]]
    assert mm.inverse_products(65, True) == 21 * 11 + 8 * 9 and mm.inverse_products(8, True) == 8
    assert mm.inverse_ws_bytes(65, 1) == 11 * 768 + 11 * 7 * 1024 + 64 * 1024 and mm.inverse_ws_bytes(8, 0) == 8 * 768
    assert [mm.inverse_blocks(c, 256) for c in (8, 9, 512, 513, 1 << 20)] == [0, 1, 1, 2, 256]


def test_bounds_are_live(monkeypatch):
    """a cut point one limb lower: z1 outgrows its bound at a product of the tree"""
    monkeypatch.setattr(mm, "SHIFT_A", mm.SHIFT_A - 1)
    N = MODULI[1] ** 2
    with pytest.raises(AssertionError):
        mm.inverse(N, [((1 << 6144) - 1) // N * N - 1] * 9)          # the largest row congruent to -1
