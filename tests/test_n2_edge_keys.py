"""The edge keys of tests/golden/n2_edge_keys.json (made by tests/golden/make_n2_edge_keys.py) are what
they claim: primes, N = n^2 on the stated side of each dispatch threshold and close to it, and the regime
the host logic picks (addb::build through fthe_debug_addb_image; the bit length of n^2 for
MontMod::classical_ok, bn_host.hpp) matches the table in tests/n2_edges.py.  Runs on the CPU."""
import ctypes
import math

import numpy as np
import pytest

import n2_edges as ne
import pyoracle
from fedtree_amd import _lib

KEYS = ne.load_keys()


def _next_prime(x):
    nw = (x.bit_length() + 31) // 32
    w = np.asarray(pyoracle.to_words(x, nw), dtype=np.uint32)
    out = np.zeros(nw + 1, dtype=np.uint32)
    assert _lib.load().fthe_next_prime(w.ctypes.data, nw, out.ctypes.data, nw + 1) == 0
    return pyoracle.from_words(out)


@pytest.mark.parametrize("name", ne.KEYS_2048 + ne.KEYS_1024)
def test_primes(name):
    p, q = KEYS[name]
    hb = 1024 if name in ne.KEYS_2048 else 512
    assert p != q and p.bit_length() == hb and q.bit_length() == hb
    for x in (p, q):
        assert x % 2 == 1 and _next_prime(x - 2) == x          # x - 1 is even: x is the next prime after x - 2


# name -> (threshold T on n, side): n >= T ("above") or n < T ("below"), within 2^(prime bits + 12) of T
EDGE = {
    "addb_lo": (1 << 2047, "above"),
    "addb_hi": (1 << 2048, "below"),
    "addb_mid_hi": (math.isqrt(1 << 4095) + 1, "above"),      # n^2 > 2^4095 (not a square) <=> n > isqrt
    "addb_mid_lo": (math.isqrt(1 << 4095) + 1, "below"),
    "cls_hi": (1 << 2047, "below"),
    "cls_lo": (math.isqrt(1 << 4093) + 1, "above"),
    "mont_hi": (math.isqrt(1 << 4093) + 1, "below"),
    "p1024_lo": (1 << 1023, "above"),
    "p1024_hi": (1 << 1024, "below"),
}


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_property(name):
    p, q = KEYS[name]
    n = p * q
    T, side = EDGE[name]
    slack = 1 << (p.bit_length() + 12)
    if side == "above":
        assert T <= n < T + slack
    else:
        assert T - slack < n < T
    N = n * n
    if name in ("addb_lo", "addb_mid_hi", "cls_lo", "p1024_lo"):   # the top of N: 1 then a long run of zeros
        assert (N >> (N.bit_length() - 900 * p.bit_length() // 1024)) == 1 << (900 * p.bit_length() // 1024 - 1)
    # the thresholds on N themselves
    want_bits = {"addb_lo": 4095, "addb_hi": 4096, "addb_mid_hi": 4096, "addb_mid_lo": 4095, "cls_hi": 4094,
                 "cls_lo": 4094, "mont_hi": 4093, "p1024_lo": 2047, "p1024_hi": 2048}[name]
    assert N.bit_length() == want_bits


@pytest.mark.parametrize("name", ne.KEYS_2048)
def test_host_regime(name):
    """addb::build admits exactly the addb keys; classical_ok (N of at least 27 * 152 - 10 = 4094 bits,
    i.e. N >= 2^4093) admits the addb and cls keys; mont_hi is left to the Montgomery pair"""
    p, q = KEYS[name]
    n = p * q
    N = n * n
    assert ne.regime_of(N) == ne.REGIME[name]
    lib = _lib.load()
    nw = np.frombuffer(n.to_bytes(256, "little"), dtype=np.uint32).copy()
    ln = ctypes.c_size_t()
    rc = lib.fthe_debug_addb_image(ctypes.c_void_p(nw.ctypes.data), 64, None, ctypes.c_size_t(0), ctypes.byref(ln))
    assert rc == (0 if ne.REGIME[name] == "addb" else _lib.FTHE_ERR_UNSUPPORTED)
    assert (N.bit_length() >= 27 * 152 - 10) == (ne.REGIME[name] in ("addb", "cls"))
