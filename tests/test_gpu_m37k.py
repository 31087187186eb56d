"""fthe_padic_m37k (fthe_padic_m37l with MUL's cross term x0 y1 + x1 y0 by one level of Karatsuba; the default
wherever m37l is admitted) through the engine: the same ciphertexts and
plaintexts, bit for bit, as fthe_padic_m37l (FTHE_NO_M37K=1) for primes at both ends of the admitted range and one past
it (1028 bits: that side falls back to fthe_padic_m37), at injected-r batches of 1, 63, 64, 65 and 1,000 -- r = 1, 2,
n - 1, n - 2 among the lanes -- and one direct-y batch of 16,385; the profiling ids tell which body ran (1537, also
counted under 1437, 1337, 1237 and 1137).  Through fthe_debug_padic_prog, on the real matrix cores: single products on
the crafted operands of the Karatsuba cross term (tools/barrett_cases.py padic_kara_mul_pairs) and squarings on the
crafted pairs every body is run on, 65 lanes (one wave and one lane), every lane checked by digit_cases.check_padic
against Python integers; the digits a product leaves (MUL; STOREX) are m37l's own, limb for limb, and below P + 2^1015,
the four-tile bodies' promise (at P just above 2^1008 two operands at the digit bound leave x1 = 3P under m37l too, so
the checker's 3P is asked of the squarings only, as in tests/test_gpu_padic_digits.py).  Integer work: exact
equality."""
import ctypes
import os

import numpy as np
import pytest

import digit_cases as dc
import pyoracle

pytestmark = pytest.mark.gpu

SEED = 20261023
COUNTS = (1, 63, 64, 65, 1000)
NDEC = 16385                                     # the smallest direct-y batch that takes the P-adic kernel
IDS = (1037, 1137, 1237, 1337, 1437, 1537)
LANES = 65


def _key_with(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", params=["1009-1027", "1027-1009", "1020-1028"])
def duo(request):
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    p, q = dc.padic_prime_pairs()[request.param]
    kk = _key_with(dc.BODY_ENV["m37k"], lambda: Paillier.from_primes(p, q, dev))
    kl = _key_with(dc.BODY_ENV["m37l"], lambda: Paillier.from_primes(p, q, dev))
    return request.param, dev, kk, kl, (p, q)


def _launches(dev, fn):
    """launches per profiling variant while fn runs"""
    lib = dev.lib
    lib.fthe_prof_enable(dev.ctx, 1)
    try:
        fn()
        vals = [ctypes.c_double() for _ in range(7)]
        assert lib.fthe_prof_read(dev.ctx, *[ctypes.byref(v) for v in vals]) == 0
        got = {}
        for S in IDS:
            ms, nl = ctypes.c_double(), ctypes.c_double()
            assert lib.fthe_prof_variant(dev.ctx, S, ctypes.byref(ms), ctypes.byref(nl)) == 0
            got[S] = nl.value
    finally:
        lib.fthe_prof_enable(dev.ctx, 0)
    return got


def test_encrypts_and_decrypt_identical_to_m37l(duo):
    name, dev, kk, kl, _ = duo
    rng = np.random.default_rng(SEED)
    m = rng.integers(0, 2**64 - 1, NDEC, dtype=np.uint64)    # seeded direct-y CRT encrypt on the P-adic kernel
    c = kk.encrypt_u64(m, seed=SEED + NDEC)
    assert np.array_equal(c, kl.encrypt_u64(m, seed=SEED + NDEC))
    d = kk.decrypt_u64(c)
    assert np.array_equal(d, m)
    assert np.array_equal(d, kl.decrypt_u64(c))
    n = kk.modulus                                           # injected r: the P-adic kernel at every count
    rs = [1, 2, n - 1, n - 2] + [int.from_bytes(rng.bytes(kk.n_words * 4), "little") % (n - 1) + 1 for _ in range(996)]
    m = rng.integers(0, 2**64 - 1, 1000, dtype=np.uint64)
    rw = pyoracle.ints_to_words(rs, kk.n_words)
    n2 = n * n
    for cnt in COUNTS:
        c = kk.encrypt_u64(m[:cnt], r=rw[:cnt])
        assert np.array_equal(c, kl.encrypt_u64(m[:cnt], r=rw[:cnt])), cnt
        for i in {0, min(1, cnt - 1), min(2, cnt - 1), min(3, cnt - 1), cnt - 1}:
            assert pyoracle.from_words(c[i]) == (1 + int(m[i]) * n) * pow(rs[i], n, n2) % n2, (cnt, i)
        d = kk.decrypt_u64(c)
        assert np.array_equal(d, m[:cnt]) and np.array_equal(d, kl.decrypt_u64(c)), cnt


def test_profiling_ids_tell_the_body(duo):
    name, dev, kk, kl, _ = duo
    m = np.arange(NDEC, dtype=np.uint64)
    c = kl.encrypt_u64(m, seed=5)
    rw = pyoracle.ints_to_words([3 + i for i in range(65)], kk.n_words)
    narrow = float(1 if name == "1020-1028" else 2)          # exponentiations on a four-tile body: p's and q's
    for what, run in (("injected r", lambda k: k.encrypt_u64(m[:65], r=rw)),
                      ("direct y", lambda k: k.encrypt_u64(m, seed=3)), ("decrypt", lambda k: k.decrypt_u64(c))):
        got = _launches(dev, lambda: run(kk))
        assert got == {1037: 0.0, 1137: 2.0, 1237: narrow, 1337: narrow, 1437: narrow, 1537: narrow}, (what, got)
        got = _launches(dev, lambda: run(kl))
        assert got == {1037: 0.0, 1137: 2.0, 1237: narrow, 1337: narrow, 1437: narrow, 1537: 0.0}, (what, got)


def _rows(vals):
    return np.array([dc.padic_row(v) for v in vals], dtype=np.uint32)


def test_crafted_products_and_squarings_on_the_matrix_cores(duo):
    name, dev, kk, kl, primes = duo
    for side, P in enumerate(primes):
        ran = dc.padic_body_for(P, "m37k")                   # the 1028-bit side falls to m37
        rng = dc.make_rng("m37k", P)
        nd = dc.padic_nd(ran)
        mul = dc.padic_kara_mul_pairs(P, ran)
        sqr = dc.padic_sqr_pairs(P, ran)
        assert len(mul) <= LANES and len(sqr) <= LANES
        a = [x for x, _ in mul] + [dc.filler(rng, nd * P) for _ in range(LANES - len(mul))]
        b = [y for _, y in mul] + [dc.filler(rng, nd * P) for _ in range(LANES - len(mul))]
        s = sqr + [dc.filler(rng, nd * P) for _ in range(LANES - len(sqr))]
        mulx = dc.PADIC_PROGS["mul"][:4] + [dc.STOREX, 2, 0, 0]           # the digits a MUL leaves
        runs = [(dc.PADIC_PROGS["mul"], [a, b], 2), (dc.PADIC_PROGS["sqr3_mul"], [a, b], 2),
                (dc.PADIC_PROGS["sqr2"], [s], 1), (dc.PADIC_WITNESS, [s], 1)]
        outs = []

        def slots_of(vals):
            slots = np.zeros((3, LANES, 2 * dc.PK), dtype=np.uint32)
            for i, v in enumerate(vals):
                slots[i] = _rows(v)
            return slots

        def run():
            for prog, vals, out_slot in runs:
                outs.append(kk.debug_padic_prog(side, prog, slots_of(vals), out_slot))
            outs.append(kk.debug_padic_prog(side, mulx, slots_of([a, b]), 2))
        got = _launches(dev, run)                            # the witness's 64 squarings are what the counters see
        want = {1037: 0.0, 1137: 1.0}
        want.update({S: 0.0 if ran == "m37" else 1.0 for S in IDS[2:]})
        assert got == want, (side, ran, got)
        digits = outs.pop()                                  # MUL; STOREX: m37l's digits, within its promise
        assert np.array_equal(digits, kl.debug_padic_prog(side, mulx, slots_of([a, b]), 2))
        for lane in range(LANES):
            x = [sum(int(v) << (dc.PB * i) for i, v in enumerate(h)) for h in (digits[lane][:dc.PK], digits[lane][dc.PK:])]
            assert int(digits[lane].max()) <= dc.PMASK and max(x) < (P + (1 << 1015) if ran == "m37k" else 5 * P), lane
            assert (x[0] + x[1] * P) % (P * P) == (a[lane][0] + a[lane][1] * P) * (b[lane][0] + b[lane][1] * P) % (P * P)
        for (prog, vals, _), out in zip(runs, outs):
            assert out.shape == (LANES, 2 * dc.PK)
            for lane in range(LANES):
                try:
                    dc.check_padic(P, ran, prog, {i: v[lane] for i, v in enumerate(vals)}, out[lane])
                except dc.Mismatch as e:
                    raise AssertionError(f"side {side} ({ran}) lane {lane} of {prog}: {e}; inputs "
                                         f"{[hex(x) for v in vals for x in v[lane]]}")
