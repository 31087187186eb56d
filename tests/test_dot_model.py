"""The per-row power and the bucket (Pippenger) dot product on Python integers (tools/dot_model.py; include/fthe.h
fthe_scalar_mul_rows / fthe_dot_segments), no device.

The model runs the engine's order of operations and counts its products.  Its results must equal the direct
prod pow(x_t, e_t, n^2) for both window widths on 512-, 1,023- and 2,048-bit moduli; its counts must equal the
closed forms the GPU tests compare with fthe_last_montmuls; and dot_plan must send short segments to the composed
form and a million terms in 28 segments to a bucket width."""
import pytest

from conftest import GOLDEN_KEYS, golden_key, load_golden
from dot_cases import (DOT_CASES, EDGE_EXPONENTS, dot_case, rand_exponents, rand_rows, seg_ptr_of, want_dot, want_rows)

import dot_model

X_ROWS = 40
_WANT = {}


def _modulus(name):
    p, q = golden_key(load_golden(name))
    return p * q


@pytest.fixture(scope="module")
def moduli():
    out = {name: _modulus(name) for name in GOLDEN_KEYS}
    assert sorted(n.bit_length() for n in out.values()) == [512, 1023, 2048]
    return out


@pytest.mark.parametrize("name", GOLDEN_KEYS)
@pytest.mark.parametrize("w", (4, 8))
def test_buckets_equal_direct_product(moduli, name, w):
    n = moduli[name]
    n2 = n * n
    xs = rand_rows(n, X_ROWS, 11)
    for case in DOT_CASES:
        for bits in (20, 64) if case in ("mixed", "digits") else (64,):
            seg, idx, es = dot_case(case, bits, X_ROWS, 3)
            if (name, case, bits) not in _WANT:              # the reference, once for both widths
                _WANT[name, case, bits] = want_dot(n, xs, es, seg, idx)
                assert _WANT[name, case, bits] == dot_model.dot_direct(xs, es, seg, idx, n2)
            got, parts = dot_model.dot_buckets(xs, es, seg, idx, n2, w)
            assert got == _WANT[name, case, bits], (case, bits)
            # the counted products are the closed form's
            top = max(e.bit_length() for e in es)
            assert parts["total"] == dot_model.bucket_products(parts["sizes"], len(seg) - 1, top, w), (case, bits)
            nwin = dot_model.windows(top, w)
            assert parts["weights"] == (len(seg) - 1) * nwin * dot_model.digit_weight_products(w)
            assert parts["horner"] == (len(seg) - 1) * dot_model.horner_products(nwin, w)
            assert parts["buckets"] == dot_model.bucket_pass_products(parts["sizes"])
            assert len(parts["sizes"]) == (len(seg) - 1) * nwin * ((1 << w) - 1)
            assert sum(parts["sizes"]) == sum(1 for e in es for j in range(nwin) if dot_model.digit(e, j, w))


def test_case_shapes():
    """What the cases promise: the segment sizes, repeated idx entries, a zero segment, every digit of a window."""
    seg, idx, es = dot_case("mixed", 64, X_ROWS, 3)
    assert [b - a for a, b in zip(seg, seg[1:])] == [0, 1, 2, 7, 8, 9, 300]
    assert idx[0] == idx[1] == idx[-1] and len(set(idx)) < len(idx)
    assert set(EDGE_EXPONENTS) <= set(es)
    assert dot_case("identity", 64, X_ROWS, 3)[1] is None
    seg, idx, es = dot_case("zeros", 20, X_ROWS, 3)
    assert es[seg[1]:seg[2]] == [0] * 5 and any(es[:3]) and any(es[8:])
    seg, idx, es = dot_case("digits", 20, X_ROWS, 3)
    assert {e & 15 for e in es[:17]} >= set(range(1, 16)) and 255 in {e & 255 for e in es}
    assert dot_case("big", 64, X_ROWS, 3)[0] == [0, 300]


def test_zero_weights_and_empty_segments(moduli):
    n = moduli[GOLDEN_KEYS[0]]
    xs = rand_rows(n, 8, 1)
    for w in (4, 8):
        got, parts = dot_model.dot_buckets(xs, [0] * 8, seg_ptr_of((0, 3, 5)), None, n * n, w)
        assert got == [1, 1, 1] and parts["total"] == 0
        got, _ = dot_model.dot_buckets(xs, [0, 0, 0, 5, 0, 0, 0, 0], seg_ptr_of((0, 3, 5)), None, n * n, w)
        assert got == [1, 1, pow(xs[3], 5, n * n)]


@pytest.mark.parametrize("name", GOLDEN_KEYS)
def test_row_powers(moduli, name):
    n = moduli[name]
    for count, bits in ((17, 64), (9, 96), (5, 5), (3, n.bit_length())):
        xs, es = rand_rows(n, count, count), rand_exponents(count, bits, count + 1)
        got, products = dot_model.scalar_mul_rows(xs, es, n * n)
        assert got == want_rows(n, xs, es)
        assert products == count * dot_model.rows_products(max(e.bit_length() for e in es))
    got, products = dot_model.scalar_mul_rows([0, 1, 7], [0, 0, 0], n * n)
    assert got == [1, 1, 1] and products == 0               # x^0 = 1, 0^0 included, with no product


def test_row_power_counts():
    assert dot_model.rows_products(0) == 0
    assert dot_model.rows_products(1) == dot_model.rows_products(4) == 14
    assert dot_model.rows_products(5) == 19                  # a second window: four squarings and a product
    assert dot_model.rows_products(64) == 89 and dot_model.rows_products(96) == 129


def test_dot_plan():
    for nseg in (1, 9, 1000, 10**6):
        for bits in (8, 20, 64, 192):
            assert dot_model.dot_plan(bits, nseg, nseg) == 0  # one-member segments: composed
    assert dot_model.dot_plan(64, 10**6, 28) in (4, 8)
    assert dot_model.dot_plan(20, 10**6, 28) in (4, 8)
    assert dot_model.dot_plan(0, 10**6, 28) == 0 and dot_model.dot_plan(64, 0, 28) == 0
    # the choice is the cheapest form by the model's own costs
    for bits, terms, nseg in ((64, 10**6, 28), (64, 10**6, 125000), (20, 4096, 16), (192, 300, 1)):
        costs = {w: dot_model.dot_cost(bits, terms, nseg, w) for w in (0, 4, 8)}
        assert costs[dot_model.dot_plan(bits, terms, nseg)] == min(costs.values())
