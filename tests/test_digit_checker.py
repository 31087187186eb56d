"""The crafted digit cases (tests/digit_cases.py) and the checker of what the kernels return for them, on the CPU.

Every listed case runs through the bit-exact model of every body it is meant for, under every test key: the models
assert each bound of the kernels' arithmetic (int32 column sums, 64-bit accumulators, the quotient estimate's window,
the digit bounds), so a case they take lies within the kernel's contract, and one on which they fire would not
belong in the list.  The checker is then shown the models' outputs, which it must accept, and the same outputs
spoiled in the two ways that matter: one limb off by one, and one multiple of the modulus moved from x1 to x0 (the
same residue).  The second is wrong for fthe_nadic_b76, whose digits are compared with the model's; for the P-adic
bodies, which may differ from each other by one in a quotient, it is wrong exactly when it breaks the digit bound
that the next product relies on.
"""
import pytest

import digit_cases as dc

PROGS_PADIC, PROGS_NADICB = dc.PADIC_PROGS, dc.NADICB_PROGS

_vetted = set()


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("name", dc.PADIC_KEYS)
def test_models_admit_every_padic_case(name, side):
    """one SQR per squaring pair, one MUL per operand pair, one LOADP per plain value, and LOADX; STOREX through the
    model of every body that can run for this prime; the checker accepts each result"""
    P = dc.padic_prime_pairs()[name][side]
    for variant in dc.BODIES:
        body = dc.padic_body_for(P, variant)
        if (P, body) in _vetted:
            continue
        _vetted.add((P, body))
        for pair in dc.padic_sqr_pairs(P, body):
            for prog in (PROGS_PADIC["sqr_storep"], PROGS_PADIC["io"]):
                out = dc.padic_model_run(P, body, prog, {0: pair})
                dc.check_padic(P, body, prog, {0: pair}, out)
        for a, b in dc.padic_mul_pairs(P, body):
            out = dc.padic_model_run(P, body, PROGS_PADIC["mul"], {0: a, 1: b})
            dc.check_padic(P, body, PROGS_PADIC["mul"], {0: a, 1: b}, out)
        vals = dc.padic_plain_values(P, body)
        assert max(vals) == dc.padic_plain_limit(P, body) - 1
        for X in vals:
            out = dc.padic_model_run(P, body, PROGS_PADIC["loadp"], {0: X})
            dc.check_padic(P, body, PROGS_PADIC["loadp"], {0: X}, out)


@pytest.mark.parametrize("name", dc.NADICB_KEYS)
def test_model_admits_every_nadicb_case(name):
    """every pair through CANON and SQR and every operand pair through MUL on nadicb_model.Digits (the VALU pass and
    the tile path of both reductions, every assertion live); the shortcut the GPU test's reference takes (integer
    products, reductions on convolved column sums) gives the same digits"""
    import nadicb_model as nm
    n = dc.nadicb_moduli()[name][0]
    key = nm.Key(n)
    for pair in dc.nadicb_pairs(n):
        assert max(pair) < 3 * n
        for pn in ("io", "canon", "sqr"):
            slow = dc.nadicb_model_run(key, PROGS_NADICB[pn], {0: pair}, fast=False)
            assert slow == dc.nadicb_model_run(key, PROGS_NADICB[pn], {0: pair}, fast=True)
            dc.check_nadicb(n, PROGS_NADICB[pn], {0: pair}, dc.nadicb_row(slow), model=slow)
    for a, b in dc.nadicb_mul_pairs(n):
        slow = dc.nadicb_model_run(key, PROGS_NADICB["mul"], {0: a, 1: b}, fast=False)
        assert slow == dc.nadicb_model_run(key, PROGS_NADICB["mul"], {0: a, 1: b}, fast=True)
        dc.check_nadicb(n, PROGS_NADICB["mul"], {0: a, 1: b}, dc.nadicb_row(slow), model=slow)


def test_case_lists_hold_what_they_promise():
    P = dc.padic_prime_pairs()["golden"][0]
    for body in dc.BODIES:
        nd = 3 if body in dc.FOUR_TILE else 5
        assert dc.padic_nd(body) == nd
        digits = {d for pair in dc.padic_sqr_pairs(P, body) for d in pair}
        assert {P - 1, P, P + 1, 2 * P - 1, 2 * P, nd * P - 1} <= digits
        assert any(a[0] * b[0] < P for a, b in dc.padic_mul_pairs(P, body))
        assert any(a[0] * b[0] >= P for a, b in dc.padic_mul_pairs(P, body))
        assert {0, 1, P - 1, P, P * P - 1, P * P, P * P + 1} <= set(dc.padic_plain_values(P, body))
    n = dc.nadicb_moduli()["2048"][0]
    t = 3 * n - 1
    assert {(0, 0), (1, 0), (0, 1), (n, n - 1), (t, t), (t, 0), (0, t)} <= set(dc.nadicb_pairs(n))
    assert any(all(v == dc.NMASK for v in dc.nlimbs(a)[:75]) for a, _ in dc.nadicb_pairs(n))
    assert any(a[0] * b[0] < n for a, b in dc.nadicb_mul_pairs(n))


@pytest.mark.parametrize("count,ncases,wave,wg", [(1100, 61, 64, 256), (1536, 23, 16, 192), (1536, 39, 16, 192)])
def test_rotated_layout_reaches_both_halves_another_wave_and_another_workgroup(count, ncases, wave, wg):
    lay = dc.rotated_layout(ncases, count, wave, wg)
    assert len(lay) == count and None in lay
    for i in range(ncases):
        pos = [j for j, c in enumerate(lay) if c == i]
        assert any(j % wave < wave // 2 for j in pos) and any(j % wave >= wave // 2 for j in pos), i
        assert any((j % wg) // wave > 0 and j // wg > 0 for j in pos), i
    assert lay[count - 1] == 0                                   # and the partial wave at the end
    for small in (1, 15, 16, 17, 63, 64, 65, 192, 193):          # small launches: cases in turn, none out of range
        lay = dc.rotated_layout(ncases, small, wave, wg)
        assert len(lay) == small and lay[0] == small % ncases


def _bump(out, radix_mask):
    bad = list(out)
    j = len(bad) // 3
    bad[j] = bad[j] + 1 if bad[j] < radix_mask else bad[j] - 1
    return bad


@pytest.mark.parametrize("body", dc.BODIES)
def test_checker_on_padic_model_outputs(body):
    pp = dc.padic_prime_pairs()
    P = pp["1009-1030"][1] if body in ("m37", "k37") else pp["golden"][0]
    nd = dc.padic_nd(body)
    rng = dc.make_rng("checker", body)
    pairs = dc.padic_sqr_pairs(P, body)[::7] + [dc.filler(rng, nd * P) for _ in range(3)]
    others = [b for _, b in dc.padic_mul_pairs(P, body)[::5]]
    for i, pair in enumerate(pairs):
        for pn, prog in PROGS_PADIC.items():
            slots = {0: pair, 1: others[i % len(others)]}
            if pn == "loadp":
                slots = {0: dc.padic_plain_values(P, body)[i % 10]}
            out = dc.padic_model_run(P, body, prog, slots)
            dc.check_padic(P, body, prog, slots, out)                          # the model's output passes
            with pytest.raises(dc.Mismatch):                                   # one limb off by one
                dc.check_padic(P, body, prog, slots, _bump(out, dc.PMASK))
            with pytest.raises(dc.Mismatch):                                   # a limb of 2^28
                dc.check_padic(P, body, prog, slots, [1 << 28] + list(out[1:]))
            if pn != "sqr2":
                continue
            # the same residue with multiples of P moved from x1 to x0: still the contract while both digits stay
            # below the bound (the bodies differ so), a failure from the first one that breaks it
            x0 = sum(v << (28 * j) for j, v in enumerate(out[:37]))
            x1 = sum(v << (28 * j) for j, v in enumerate(out[37:]))
            k = 1
            while x0 + k * P < nd * P:
                k += 1
            if x1 < k:
                continue
            if k > 1:
                dc.check_padic(P, body, prog, slots, dc.padic_row((x0 + P, x1 - 1)))
            with pytest.raises(dc.Mismatch, match="digit at or above"):
                dc.check_padic(P, body, prog, slots, dc.padic_row((x0 + k * P, x1 - k)))
    # LOADX; STOREX of the top digit: x0 += P, x1 -= 1 is another pair and beyond the bound
    top = nd * P - 1
    with pytest.raises(dc.Mismatch):
        dc.check_padic(P, body, PROGS_PADIC["io"], {0: (top, top)}, dc.plimbs(top + P) + dc.plimbs(top - 1))
    # a STOREP value that is the residue but not below 6 P^2
    out = dc.padic_model_run(P, body, PROGS_PADIC["sqr_storep"], {0: (1, 1)})
    big = sum(v << (28 * j) for j, v in enumerate(out)) + 6 * P * P
    with pytest.raises(dc.Mismatch, match="6 P"):
        dc.check_padic(P, body, PROGS_PADIC["sqr_storep"], {0: (1, 1)}, dc.plimbs(big, 74))


@pytest.mark.parametrize("name", ["2048", "2^2040+1"])
def test_checker_on_nadicb_model_outputs(name):
    import nadicb_model as nm
    n = dc.nadicb_moduli()[name][0]
    key = nm.Key(n)
    rng = dc.make_rng("checker", name)
    pairs = dc.nadicb_pairs(n)[::4] + [dc.filler(rng, 3 * n) for _ in range(4)]
    moved = 0
    for i, pair in enumerate(pairs):
        for pn, prog in PROGS_NADICB.items():
            slots = {0: pair, 1: pairs[(i + 3) % len(pairs)]}
            want = dc.nadicb_model_run(key, prog, slots)
            out = dc.nadicb_row(want)
            dc.check_nadicb(n, prog, slots, out, model=want)
            with pytest.raises(dc.Mismatch):
                dc.check_nadicb(n, prog, slots, _bump(out, dc.NMASK), model=want)
            with pytest.raises(dc.Mismatch):
                dc.check_nadicb(n, prog, slots, _bump(out, dc.NMASK))          # the residue alone tells as well
            x0, x1 = want
            if x1 >= 1 and x0 + n < (1 << (27 * 76)):                          # x0 += n, x1 -= 1: the same residue
                with pytest.raises(dc.Mismatch):
                    dc.check_nadicb(n, prog, slots, dc.nadicb_row((x0 + n, x1 - 1)), model=want)
                moved += 1
    assert moved >= len(pairs)


@pytest.mark.parametrize("variant", ["m37", "m37t", "m37s", "m37l"])
def test_emulator_takes_the_edge_pairs_too(variant):
    """the wave emulator's digit self-test draws its special pairs from the shared list (as before); here it runs the
    rest of what the GPU tests run, the pairs next to multiples of P and the small squares, on the kernel text"""
    import wave_emu
    pp = dc.padic_prime_pairs()
    P = pp["1009-1030"][1] if variant == "m37" else pp["1009-1027"][1]
    pairs0 = dc.padic_edge_pairs(P, variant)
    assert wave_emu.m37_digits_selftest(seed=9, variant=variant, P=P, pairs0=pairs0) == 0
