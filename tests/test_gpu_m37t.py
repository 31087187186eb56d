"""fthe_padic_m37t (the four-tile body of the matrix-core P-adic kernel, the default for a modulus of at most 1027
bits) through the engine: the same ciphertexts and plaintexts, bit for bit, as fthe_padic_m37
(FTHE_NO_M37T=1) and as the Montgomery programs (FTHE_NO_PADIC=1) at one wave and its edges, for primes at both ends
of the admitted range and one past it, and the profiling id 1237 tells which body ran.  Integer work: exact equality.
Direct-y encrypts and decrypts of at most 16,384 ciphertexts take the four-lane kernel, so the batches that reach the
P-adic kernel at one wave and its edges are the injected-r ones (1, 63, 64, 65, 1,000) and everything from 16,385."""
import ctypes
import os

import numpy as np
import pytest

import pyoracle
from conftest import golden_key, load_golden

pytestmark = pytest.mark.gpu

SEED = 20261020
L = 1027                                         # the widest P of fthe_padic_m37t
COUNTS = (1, 63, 64, 65, 1000)
NDEC = 16385                                     # the smallest batch that takes the P-adic decrypt


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
    lo = {"1009-L": 1009, "L-1009": 1009, "L+1": 1020}[name]
    hi = L + 1 if name == "L+1" else L
    p, q = _next_prime((1 << (lo - 1)) + (1 << 500)), _next_prime((1 << hi) - (1 << 600))
    assert p.bit_length() == lo and q.bit_length() == hi
    return (q, p) if name == "L-1009" else (p, q)


@pytest.fixture(scope="module", params=["golden", "1009-L", "L-1009", "L+1"])
def trio(request):
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    p, q = _primes(request.param)
    pt = _key_with({}, lambda: Paillier.from_primes(p, q, dev))
    pm = _key_with({"FTHE_NO_M37T": "1"}, lambda: Paillier.from_primes(p, q, dev))
    ps = _key_with({"FTHE_NO_PADIC": "1"}, lambda: Paillier.from_primes(p, q, dev))
    return request.param, dev, pt, pm, ps


def _launches(dev, fn):
    """launches per profiling variant while fn runs"""
    lib = dev.lib
    lib.fthe_prof_enable(dev.ctx, 1)
    fn()
    vals = [ctypes.c_double() for _ in range(7)]
    assert lib.fthe_prof_read(dev.ctx, *[ctypes.byref(v) for v in vals]) == 0
    got = {}
    for S in (1037, 1137, 1237):
        ms, nl = ctypes.c_double(), ctypes.c_double()
        assert lib.fthe_prof_variant(dev.ctx, S, ctypes.byref(ms), ctypes.byref(nl)) == 0
        got[S] = nl.value
    lib.fthe_prof_enable(dev.ctx, 0)
    return got


def test_encrypts_and_decrypt_identical_across_bodies(trio):
    name, dev, pt, pm, ps = trio
    rng = np.random.default_rng(SEED)
    for cnt in COUNTS + (NDEC,):                 # seeded direct-y CRT encrypts (the P-adic kernel from NDEC on)
        m = rng.integers(0, 2**64 - 1, cnt, dtype=np.uint64)
        c = pt.encrypt_u64(m, seed=SEED + cnt)
        assert np.array_equal(c, pm.encrypt_u64(m, seed=SEED + cnt)), cnt
        assert np.array_equal(c, ps.encrypt_u64(m, seed=SEED + cnt)), cnt
    n = pt.modulus                               # injected r: the P-adic kernel at every count
    rs = [1, 2, n - 1, n - 2] + [int.from_bytes(rng.bytes(pt.n_words * 4), "little") % (n - 1) + 1 for _ in range(996)]
    m = rng.integers(0, 2**64 - 1, 1000, dtype=np.uint64)
    rw = pyoracle.ints_to_words(rs, pt.n_words)
    n2 = n * n
    for cnt in COUNTS:
        c = pt.encrypt_u64(m[:cnt], r=rw[:cnt])
        assert np.array_equal(c, pm.encrypt_u64(m[:cnt], r=rw[:cnt])), cnt
        assert np.array_equal(c, ps.encrypt_u64(m[:cnt], r=rw[:cnt])), cnt
        for i in {0, min(2, cnt - 1), cnt - 1}:
            assert pyoracle.from_words(c[i]) == (1 + int(m[i]) * n) * pow(rs[i], n, n2) % n2, (cnt, i)
    m = rng.integers(0, 2**64 - 1, NDEC, dtype=np.uint64)
    c = ps.encrypt_u64(m, seed=SEED + 7)
    d = pt.decrypt_u64(c)
    assert np.array_equal(d, m)
    assert np.array_equal(d, pm.decrypt_u64(c))
    assert np.array_equal(d, ps.decrypt_u64(c))


def test_profiling_id_tells_the_body(trio):
    name, dev, pt, pm, ps = trio
    m = np.arange(NDEC, dtype=np.uint64)
    c = ps.encrypt_u64(m, seed=5)
    rw = pyoracle.ints_to_words([3 + i for i in range(65)], pt.n_words)
    narrow = {"golden": 2, "1009-L": 2, "L-1009": 2, "L+1": 1}[name]      # exponentiations on m37t: p's and q's
    for what, run in (("injected r", lambda k: k.encrypt_u64(m[:65], r=rw)),
                      ("direct y", lambda k: k.encrypt_u64(m, seed=3)), ("decrypt", lambda k: k.decrypt_u64(c))):
        got = _launches(dev, lambda: run(pt))
        assert got == {1037: 0.0, 1137: 2.0, 1237: float(narrow)}, (what, got)   # 1137 counts both bodies
        got = _launches(dev, lambda: run(pm))
        assert got == {1037: 0.0, 1137: 2.0, 1237: 0.0}, (what, got)
        got = _launches(dev, lambda: run(ps))
        assert got[1137] == 0.0 and got[1237] == 0.0, (what, got)


def test_public_paillier1024_p_equals_n():
    """the public path r^n mod n^2 with P = n (1024 bits: the four-tile body) against the FTHE_NO_M37T key"""
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    pt = _key_with({}, lambda: Paillier(dev).keygen(1024, seed=SEED + 2))
    pm = _key_with({"FTHE_NO_M37T": "1"}, lambda: Paillier.from_primes(pt.p, pt.q, dev))
    rng = np.random.default_rng(SEED + 3)
    n = pt.modulus
    rs = [1, 2, n - 1, n - 2] + [int.from_bytes(rng.bytes(128), "little") % (n - 1) + 1 for _ in range(996)]
    m = rng.integers(0, 2**63, 1000, dtype=np.uint64)
    rw = pyoracle.ints_to_words(rs, pt.n_words)
    got = _launches(dev, lambda: pt.encrypt_u64(m, r=rw, public=True))
    assert got[1237] >= 1.0 and got[1137] == got[1237], got
    c = pt.encrypt_u64(m, r=rw, public=True)
    got = _launches(dev, lambda: pm.encrypt_u64(m, r=rw, public=True))
    assert got[1237] == 0.0 and got[1137] >= 1.0, got
    assert np.array_equal(c, pm.encrypt_u64(m, r=rw, public=True))
    n2 = n * n
    for i in (0, 1, 2, 3, 999):
        assert pyoracle.from_words(c[i]) == (1 + int(m[i]) * n) * pow(rs[i], n, n2) % n2, i
    assert np.array_equal(pt.decrypt_u64(c), m)
