"""The model of fthe_horner192 (tools/mul192_model.py horner()): prod_j x_j^(2^(j sq)) mod N against Python's pow over
the six edge moduli on hostile rows (rows >= N included), with every bound of DESIGN.md 24 asserted at every product
and the product count against the products that ran."""
import os
import sys

import pytest

import n2_edges as ne

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import mul192_model as mm  # noqa: E402

MODULI = mm.edge_moduli()


@pytest.mark.parametrize("sq", [1, 224])
@pytest.mark.parametrize("ni", range(len(MODULI)))
def test_horner_at_the_modulus_edges(ni, sq):
    n = MODULI[ni]
    N = n * n
    E = ne.hostile_rows(N, bits=32 * mm.WORDS, nrand=2, seed=ni)
    for J in (1, 2, 3):
        for i in range(0, len(E), 1 if sq == 1 else 5):          # every row as the seed; sq = 224: every fifth
            xs, ran = [E[(i + 7 * j) % len(E)] for j in range(J)][::-1], []
            want = xs[0] if J == 1 else mm.reduce_mod([pow(x, 1 << (j * sq), N) for j, x in enumerate(xs)], N)
            assert mm.horner(xs, sq, n, lanes=sq == 1 and i == 13, count=ran) == want
            assert ran == [mm.horner_products(J, sq) if J > 1 else 0]
