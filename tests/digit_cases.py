"""The crafted digit cases, programs, layout and checker of tools/barrett_cases.py (one list for the emulator, the models
and the GPU: see there) under this module's name for the tests, and the keys the tests run them under."""
import os
import random
import sys

_TOOLS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)
from barrett_cases import *  # noqa: E402,F401,F403


# ---- the keys ----------------------------------------------------------------------------------------------------
def next_prime(x):
    """the smallest prime above x (fthe_next_prime: host code, no device)"""
    import numpy as np
    from fedtree_amd import _lib
    lib = _lib.load()
    words = (x.bit_length() + 31) // 32
    w = np.array([(x >> (32 * i)) & 0xFFFFFFFF for i in range(words)], dtype=np.uint32)
    out = np.zeros(words + 1, dtype=np.uint32)
    assert lib.fthe_next_prime(w.ctypes.data, words, out.ctypes.data, words + 1) == 0
    return sum(int(v) << (32 * i) for i, v in enumerate(out))


_CACHE = {}


def padic_prime_pairs():
    """the prime pairs (p, q) the P-adic cases run under: a reference key, both ends of the four-tile bodies' range
    either way round, a q past it (1028 bits: q falls to m37), the ends of the K = 37 range, and primes next to
    0x80.. / 0x7f.. byte runs (the balanced-digit tiles carry in every byte)"""
    if "padic" not in _CACHE:
        from conftest import golden_key, load_golden
        lo = next_prime((1 << 1008) + (1 << 500))
        p27, p28 = next_prime((1 << 1027) - (1 << 600)), next_prime((1 << 1028) - (1 << 600))
        p20, p30 = next_prime((1 << 1019) + (1 << 500)), next_prime((1 << 1030) - (1 << 600))
        assert [x.bit_length() for x in (lo, p27, p28, p20, p30)] == [1009, 1027, 1028, 1020, 1030]
        _CACHE["padic"] = {
            "golden": golden_key(load_golden("ref_gmp_L4096.json")),
            "1009-1027": (lo, p27), "1027-1009": (p27, lo), "1020-1028": (p20, p28), "1009-1030": (lo, p30),
            "x80-x7f": (next_prime(int("80" * 128, 16)), next_prime(int("7f" * 128, 16) | (1 << 1023))),
        }
    return _CACHE["padic"]


PADIC_KEYS = ("golden", "1009-1027", "1027-1009", "1020-1028", "1009-1030", "x80-x7f")


def nadicb_moduli():
    """name -> (n, (p, q) or None): n of 2048 and of 2041 bits from primes, and the model's extreme moduli 2^2048 - 1
    and 2^2040 + 1, which are no products of two primes and exist as public keys only"""
    if "nadicb" not in _CACHE:
        rng = random.Random(76)
        p = next_prime(rng.getrandbits(1024) | (3 << 1022))
        q = next_prime(rng.getrandbits(1024) | (3 << 1022))
        p41 = next_prime(rng.getrandbits(1021) | (3 << 1019))
        q41 = next_prime((rng.getrandbits(1020) | (1 << 1019)) & ~(1 << 1018))
        assert (p * q).bit_length() == 2048 and (p41 * q41).bit_length() == 2041
        _CACHE["nadicb"] = {"2048": (p * q, (p, q)), "2041": (p41 * q41, (p41, q41)),
                            "2^2048-1": ((1 << 2048) - 1, None), "2^2040+1": ((1 << 2040) + 1, None)}
    return _CACHE["nadicb"]


NADICB_KEYS = ("2048", "2041", "2^2048-1", "2^2040+1")
