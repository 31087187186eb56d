"""fthe_padic_m37 after the round-7 cuts in its reduction (product 1's window from column 128 with a 2^1046
bias, the second quotient folded straight into operand dwords) against the VALU kernel
fthe_padic_k37 (the same key set up with FTHE_NO_PADIC_MFMA=1), whose Barrett keeps every column: device-randomness
encrypts and CRT decrypts of 16,640 ciphertexts (m37 serves batches above 16,384), with the bench's key and with
primes at both ends of the kernel's range -- at P near 2^1030 the numerator of a small nonzero q1 goes negative
(the clamp / the r = T + P path), which the decrypt rows 0, 1, 2 and n^2 - 1 reach through LOADP.
Integer work: exact equality."""
import os
import random

import numpy as np
import pytest

import pyoracle

pytestmark = pytest.mark.gpu

BENCH_SEED = 20261015            # bench.py's key
COUNT = 16640


def _with_env(env, fn):
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


def _primes(kind):
    from test_gpu_parity import _next_prime
    if kind == "ends":                           # the largest and the smallest P the kernel takes
        return _next_prime((1 << 1030) - (1 << 600)), _next_prime((1 << 1008) + (1 << 500))
    rng = random.Random(1030)                    # random primes of exactly 1030 and 1009 bits
    return (_next_prime(rng.getrandbits(1030) | (1 << 1029)), _next_prime(rng.getrandbits(1009) | (1 << 1008)))


@pytest.fixture(scope="module", params=["bench", "ends", "random-1030-1009"])
def pair(request):
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    if request.param == "bench":
        pa = _with_env({}, lambda: Paillier(dev).keygen(2048, seed=BENCH_SEED))
        p, q = pa.p, pa.q
    else:
        p, q = _primes(request.param)
        assert {p.bit_length(), q.bit_length()} == {1030, 1009}
        pa = _with_env({}, lambda: Paillier.from_primes(p, q, dev))
    pk = _with_env({"FTHE_NO_PADIC_MFMA": "1"}, lambda: Paillier.from_primes(p, q, dev))
    return dev, pa, pk


def _runs_on(dev, fn):
    """launches of fthe_padic_k37 (1037) and fthe_padic_m37 (1137) during fn()"""
    import ctypes
    lib = dev.lib
    lib.fthe_prof_enable(dev.ctx, 1)
    out = fn()
    vals = [ctypes.c_double() for _ in range(7)]
    assert lib.fthe_prof_read(dev.ctx, *[ctypes.byref(v) for v in vals]) == 0
    got = {}
    for S in (1037, 1137):
        ms, nl = ctypes.c_double(), ctypes.c_double()
        assert lib.fthe_prof_variant(dev.ctx, S, ctypes.byref(ms), ctypes.byref(nl)) == 0
        got[S] = nl.value
    lib.fthe_prof_enable(dev.ctx, 0)
    return out, got


def test_encrypts_and_decrypts_identical_to_the_valu_kernel(pair):
    dev, pa, pk = pair
    rng = np.random.default_rng(BENCH_SEED + 7)
    m = rng.integers(0, 2**64 - 1, COUNT, dtype=np.uint64)
    ca, runs = _runs_on(dev, lambda: pa.encrypt_u64(m, seed=BENCH_SEED + 8))
    assert runs[1137] > 0 and runs[1037] == 0, runs          # the matrix-core kernel did the work
    ck, runs = _runs_on(dev, lambda: pk.encrypt_u64(m, seed=BENCH_SEED + 8))
    assert runs[1137] == 0 and runs[1037] > 0, runs
    assert np.array_equal(ca, ck)
    # decrypt: the ciphertexts, with rows 0, 1, 2 and n^2 - 1 in front (LOADP with q1 tiny or zero)
    n = pa.modulus
    cw = 2 * pa.n_words
    rows = ca.copy()
    rows[:4] = pyoracle.ints_to_words([0, 1, 2, n * n - 1], cw)
    (low_a, full_a), runs = _runs_on(dev, lambda: pa.decrypt_u64(rows, full=True))
    assert runs[1137] > 0 and runs[1037] == 0, runs
    low_k, full_k = pk.decrypt_u64(rows, full=True)
    assert np.array_equal(full_a, full_k) and np.array_equal(low_a, low_k)
    assert np.array_equal(low_a[4:], m[4:])
    assert pyoracle.from_words(full_a[1]) == 0 and pyoracle.from_words(full_a[3]) == 0    # 1 and n^2 - 1 = -1: m = 0
