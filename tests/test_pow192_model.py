"""The model of fthe_pow192 (tools/mul192_model.py power()): x^e t mod N against Python's pow over the six edge moduli,
on hostile bases that are units mod N (every step then works on a full-size remainder), with every bound of
DESIGN.md 24 asserted at every product, and the schedule builder's product count against the products that ran."""
import os
import random
import sys
from math import gcd

import pytest

import n2_edges as ne

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import mul192_model as mm  # noqa: E402

MODULI = mm.edge_moduli()


def _all_windows(w):
    """an exponent whose width-w walk uses every table entry and squares: each odd v < 2^w, then w zero bits"""
    return int("".join(bin(v)[2:] + "0" * w for v in range((1 << w) - 1, 0, -2)), 2)


@pytest.mark.parametrize("ni", range(len(MODULI)))
def test_power_at_the_modulus_edges(ni):
    n = MODULI[ni]
    N, rng = n * n, random.Random(ni)
    units = [x for x in ne.hostile_rows(N, bits=32 * mm.WORDS, nrand=2, seed=ni) if gcd(x, N) == 1]
    assert len(units) >= 10
    for e in (2, 3, (1 << 64) - 1, rng.getrandbits(200) | 1 << 199, n):
        xs = units if e < n else units[-2:]              # the 3,600 products of e = n: on two bases, with and without t
        for x, t in zip(xs, [None, units[-1]] + units[:-2]):
            ran = []
            assert mm.power(x, e, n, t=t, count=ran) == pow(x, e, N) * (1 if t is None else t) % N
            assert ran == [mm.products(mm.plan(e, t is not None)[1], t is not None)]


@pytest.mark.parametrize("w", range(1, mm.MAX_WINDOW + 1))
def test_every_window_width(w):
    """each width forced once, lane by lane: every schedule byte and every table entry is used"""
    n, e = MODULI[w], _all_windows(w)
    N, sched, ran = n * n, mm.schedule(e, w), []
    assert set(sched) == set(range((1 << (w - 1)) + 1)) and sched[0] == 1 << (w - 1)
    x = ne.hostile_rows(N, bits=32 * mm.WORDS)[13]                   # the all-ones row, >= N
    assert mm.power(x, e, n, t=N - 2, w=w, lanes=w in (1, 3), count=ran) == pow(x, e, N) * (N - 2) % N
    assert ran == [mm.products(sched, True)] == [1 + (1 << (w - 1)) * (w > 1) + len(sched)]


def test_plan_counts_exactly():
    """short exponents get a small table, a 3072-bit one the widest; ties go to the smaller width"""
    assert mm.plan(2)[0] == 1 and mm.plan(3) == (1, bytes([1, 0, 1])) and mm.plan(MODULI[0])[0] == 5
    for e in (5, 255, (1 << 64) - 1, MODULI[5]):
        w, sched = mm.plan(e)
        costs = [mm.products(mm.schedule(e, v), False) for v in range(1, mm.MAX_WINDOW + 1)]
        assert costs.index(min(costs)) + 1 == w and mm.products(sched, False) == min(costs)
