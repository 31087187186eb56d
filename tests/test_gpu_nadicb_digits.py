"""Single products of fthe_nadic_b76 (the parties' r^n mod n^2 on base-n digits, Barrett on the matrix cores) on
crafted digits, on the GPU.

fthe_debug_nadicb_prog runs the five bring-up programs (LOADX; STOREX -- CANON -- one SQR -- one MUL -- SQR x3 + MUL)
on the crafted pairs of tests/digit_cases.py (0, 1, n next to n - 1, the largest digit 3n - 1 alone and on both sides,
all-ones limbs, products below n whose quotient estimate is clamped) and on random digits in [0, 3n), under n of 2048
and 2041 bits from primes and the model's extreme moduli 2^2048 - 1 and 2^2040 + 1 as public keys, at 1, 15, 16, 17
(one wave holds 16 ciphertexts), 192, 193 (one workgroup of 12 waves) and 1,536 ciphertexts (eight workgroups' worth:
the persistent waves draw batches).  The crafted cases and the first 200 random ones are compared digit for digit with
tools/nadicb_model.py; every ciphertext of every launch is checked for limbs below 2^27, digits below 3n (below n
after CANON) and the exact residue.  Integer work: no tolerance.
"""
import functools

import numpy as np
import pytest

import digit_cases as dc

pytestmark = pytest.mark.gpu

COUNTS = (1, 15, 16, 17, 192, 193, 1536)
NPOOL = max(COUNTS)
NEXACT = 200                                     # random ciphertexts compared digit for digit (the model is Python)
WAVE, WG = 16, 192


@pytest.fixture(scope="module", params=dc.NADICB_KEYS)
def keyed(request):
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    n, primes = dc.nadicb_moduli()[request.param]
    pl = Paillier.from_primes(*primes, dev) if primes else Paillier.from_public(n, dev)
    assert pl.modulus == n
    return pl, n, request.param


@functools.lru_cache(maxsize=None)
def _pool(n):
    rng = dc.make_rng("nadicb", n)
    rows = lambda vs: np.array([dc.nadicb_row(v) for v in vs], dtype=np.uint32)      # noqa: E731
    sq = dc.nadicb_pairs(n)
    mu = dc.nadicb_mul_pairs(n)
    rx = [dc.filler(rng, 3 * n) for _ in range(NPOOL)]
    ry = [dc.filler(rng, 3 * n) for _ in range(NPOOL)]
    return {"one": (sq, rows(sq), rx, rows(rx)), "mula": ([a for a, _ in mu], rows([a for a, _ in mu]), rx, rows(rx)),
            "mulb": ([b for _, b in mu], rows([b for _, b in mu]), ry, rows(ry))}


@functools.lru_cache(maxsize=None)
def _model(n, pn, x, y):
    return dc.nadicb_model_run(_key(n), dc.NADICB_PROGS[pn], {0: x, 1: y})


@functools.lru_cache(maxsize=None)
def _key(n):
    import nadicb_model as nm
    return nm.Key(n)


@pytest.mark.parametrize("pn", list(dc.NADICB_PROGS))
def test_program_on_crafted_digits(keyed, pn):
    pl, n, name = keyed
    prog = dc.NADICB_PROGS[pn]
    pool = _pool(n)
    kinds = ("mula", "mulb") if dc.MUL in prog[::2] else ("one", "mulb")
    out_slot = 1 if pn in ("io", "canon") else 2
    gap, exact, total = 0, 0, 0
    for count in COUNTS:
        lay = dc.rotated_layout(len(pool[kinds[0]][0]), count, WAVE, WG)
        slots = np.zeros((4, count, 2 * dc.NS), dtype=np.uint32)
        vals = []
        for s, k in enumerate(kinds):
            cases, crows, rnd, rrows = pool[k]
            vals.append([cases[c] if c is not None else rnd[j] for j, c in enumerate(lay)])
            slots[s] = np.stack([crows[c] if c is not None else rrows[j] for j, c in enumerate(lay)])
        out = pl.debug_nadicb_prog(prog, slots, out_slot)
        assert out.shape == (count, 2 * dc.NS)
        for g in range(count):                               # every ciphertext
            x, y = vals[0][g], vals[1][g]
            model = _model(n, pn, x, y) if lay[g] is not None or g < NEXACT else None
            try:
                d = dc.check_nadicb(n, prog, {0: x, 1: y}, out[g], model=model)
            except dc.Mismatch as e:
                raise AssertionError(f"{pn} count {count} ciphertext {g} (case {lay[g]}): {e}; x {[hex(v) for v in x]} "
                                     f"y {[hex(v) for v in y]} got {[hex(v) for v in dc.nadicb_digits(out[g])]}")
            exact += model is not None
            total += 1
            if pn in ("sqr", "mul", "sqr3_mul"):
                gap = max(gap, *d)
    assert total == sum(COUNTS) and exact >= NEXACT
    # a digit r = z - q3 n lies q - q3 multiples of n above z mod n: the model's bound on the estimate is 2
    print(f"nadic_b76 n = {name} {pn}: {total} ciphertexts, {exact} digit-exact, largest q - q3 = {gap}")
    assert gap <= 2
