"""fthe_padic_m37l (the four-tile body whose product 1 is fed q1's limbs as they lie, no repack; the default for a
modulus of at most 1027 bits) through the engine: the same ciphertexts and plaintexts, bit for bit, as
fthe_padic_m37s (FTHE_NO_M37L=1) and as fthe_padic_m37 (FTHE_NO_M37T=1), for primes at both ends of the admitted
range and one past it, and the profiling ids tell which body ran (1437, also counted under 1337, 1237 and 1137).
Integer work: exact equality.  Direct-y encrypts and decrypts of at most 16,384 ciphertexts take the four-lane kernel,
so the batches that reach the P-adic kernel at one wave and its edges are the injected-r ones (1, 63, 64, 65, 1,000)
and everything from 16,385.  r = 1, 2, n - 1, n - 2 start their squarings with q1 = 0 (the clamped quotient)."""
import ctypes
import os

import numpy as np
import pytest

import pyoracle
from conftest import golden_key, load_golden

pytestmark = pytest.mark.gpu

SEED = 20261022
L = 1027                                         # the widest P of the four-tile bodies
COUNTS = (1, 63, 64, 65, 1000)
NDEC = 16385                                     # the smallest batch that takes the P-adic decrypt
IDS = (1037, 1137, 1237, 1337, 1437)


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


def _primes(name):
    from test_gpu_parity import _next_prime
    if name == "golden":
        return golden_key(load_golden("ref_gmp_L4096.json"))
    lo, hi = {"1009-1027": (1009, L), "1027-1009": (1009, L), "1020-1028": (1020, L + 1)}[name]
    p, q = _next_prime((1 << (lo - 1)) + (1 << 500)), _next_prime((1 << hi) - (1 << 600))
    assert p.bit_length() == lo and q.bit_length() == hi
    return (q, p) if name == "1027-1009" else (p, q)


@pytest.fixture(scope="module", params=["golden", "1009-1027", "1027-1009", "1020-1028"])
def trio(request):
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    p, q = _primes(request.param)
    kl = _key_with({}, lambda: Paillier.from_primes(p, q, dev))
    ks = _key_with({"FTHE_NO_M37L": "1"}, lambda: Paillier.from_primes(p, q, dev))
    km = _key_with({"FTHE_NO_M37T": "1"}, lambda: Paillier.from_primes(p, q, dev))
    return request.param, dev, kl, ks, km


def _launches(dev, fn):
    """launches per profiling variant while fn runs"""
    lib = dev.lib
    lib.fthe_prof_enable(dev.ctx, 1)
    fn()
    vals = [ctypes.c_double() for _ in range(7)]
    assert lib.fthe_prof_read(dev.ctx, *[ctypes.byref(v) for v in vals]) == 0
    got = {}
    for S in IDS:
        ms, nl = ctypes.c_double(), ctypes.c_double()
        assert lib.fthe_prof_variant(dev.ctx, S, ctypes.byref(ms), ctypes.byref(nl)) == 0
        got[S] = nl.value
    lib.fthe_prof_enable(dev.ctx, 0)
    return got


def test_encrypts_and_decrypt_identical_across_bodies(trio):
    name, dev, kl, ks, km = trio
    rng = np.random.default_rng(SEED)
    m = rng.integers(0, 2**64 - 1, NDEC, dtype=np.uint64)    # seeded direct-y CRT encrypt on the P-adic kernel
    c = kl.encrypt_u64(m, seed=SEED + NDEC)
    assert np.array_equal(c, ks.encrypt_u64(m, seed=SEED + NDEC))
    assert np.array_equal(c, km.encrypt_u64(m, seed=SEED + NDEC))
    d = kl.decrypt_u64(c)
    assert np.array_equal(d, m)                              # round trip
    assert np.array_equal(d, ks.decrypt_u64(c))
    assert np.array_equal(d, km.decrypt_u64(c))
    n = kl.modulus                                           # injected r: the P-adic kernel at every count
    rs = [1, 2, n - 1, n - 2] + [int.from_bytes(rng.bytes(kl.n_words * 4), "little") % (n - 1) + 1 for _ in range(996)]
    m = rng.integers(0, 2**64 - 1, 1000, dtype=np.uint64)
    rw = pyoracle.ints_to_words(rs, kl.n_words)
    n2 = n * n
    for cnt in COUNTS:
        c = kl.encrypt_u64(m[:cnt], r=rw[:cnt])
        assert np.array_equal(c, ks.encrypt_u64(m[:cnt], r=rw[:cnt])), cnt
        assert np.array_equal(c, km.encrypt_u64(m[:cnt], r=rw[:cnt])), cnt
        for i in {0, min(1, cnt - 1), min(2, cnt - 1), min(3, cnt - 1), cnt - 1}:
            assert pyoracle.from_words(c[i]) == (1 + int(m[i]) * n) * pow(rs[i], n, n2) % n2, (cnt, i)
        assert np.array_equal(kl.decrypt_u64(c), m[:cnt]), cnt


def test_profiling_ids_tell_the_body(trio):
    name, dev, kl, ks, km = trio
    m = np.arange(NDEC, dtype=np.uint64)
    c = km.encrypt_u64(m, seed=5)
    rw = pyoracle.ints_to_words([3 + i for i in range(65)], kl.n_words)
    narrow = float(1 if name == "1020-1028" else 2)          # exponentiations on a four-tile body: p's and q's
    for what, run in (("injected r", lambda k: k.encrypt_u64(m[:65], r=rw)),
                      ("direct y", lambda k: k.encrypt_u64(m, seed=3)), ("decrypt", lambda k: k.decrypt_u64(c))):
        got = _launches(dev, lambda: run(kl))
        assert got == {1037: 0.0, 1137: 2.0, 1237: narrow, 1337: narrow, 1437: narrow}, (what, got)
        got = _launches(dev, lambda: run(ks))
        assert got == {1037: 0.0, 1137: 2.0, 1237: narrow, 1337: narrow, 1437: 0.0}, (what, got)
        got = _launches(dev, lambda: run(km))
        assert got == {1037: 0.0, 1137: 2.0, 1237: 0.0, 1337: 0.0, 1437: 0.0}, (what, got)


def test_public_paillier1024_p_equals_n():
    """the public path r^n mod n^2 with P = n (1024 bits) reaches the new body and matches the FTHE_NO_M37L key"""
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    kl = _key_with({}, lambda: Paillier(dev).keygen(1024, seed=SEED + 2))
    ks = _key_with({"FTHE_NO_M37L": "1"}, lambda: Paillier.from_primes(kl.p, kl.q, dev))
    rng = np.random.default_rng(SEED + 3)
    n = kl.modulus
    rs = [1, 2, n - 1, n - 2] + [int.from_bytes(rng.bytes(128), "little") % (n - 1) + 1 for _ in range(996)]
    m = rng.integers(0, 2**63, 1000, dtype=np.uint64)
    rw = pyoracle.ints_to_words(rs, kl.n_words)
    got = _launches(dev, lambda: kl.encrypt_u64(m, r=rw, public=True))
    assert got[1437] >= 1.0 and got[1137] == got[1237] == got[1337] == got[1437], got
    c = kl.encrypt_u64(m, r=rw, public=True)
    got = _launches(dev, lambda: ks.encrypt_u64(m, r=rw, public=True))
    assert got[1437] == 0.0 and got[1337] >= 1.0 and got[1137] == got[1337], got
    assert np.array_equal(c, ks.encrypt_u64(m, r=rw, public=True))
    n2 = n * n
    for i in (0, 1, 2, 3, 999):
        assert pyoracle.from_words(c[i]) == (1 + int(m[i]) * n) * pow(rs[i], n, n2) % n2, i
    assert np.array_equal(kl.decrypt_u64(c), m)
