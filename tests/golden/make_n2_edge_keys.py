"""Make tests/golden/n2_edge_keys.json: Paillier keys whose N = n^2 sits at the ends of the ranges that
pick the kernel of every product mod n^2 (add, sub, scalar mul, k-way merge, segmented product / scan).

For a Paillier-2048 key (two 1024-bit primes, n of 2047 or 2048 bits) the library picks by N:
  N >= 2^4094            fthe_addb_q152, the matrix-core Barrett add (addb::build, addb_image.hpp)
  2^4093 <= N < 2^4094   MULWC / MULWGC, the classical MSB-first product (MontMod::classical_ok, bn_host.hpp)
  N < 2^4093             a Montgomery product plus the R^2 correction

  addb_lo      n >= 2^2047, as close above as the search gives (N just above 2^4094, mu just below 2^4106)
  addb_hi      the two largest primes below 2^1024 (n just below 2^2048)
  addb_mid_hi  n^2 just above 2^4095
  addb_mid_lo  n^2 just below 2^4095
  cls_hi       n < 2^2047, as close below as possible (N just below 2^4094: classical, not addb)
  cls_lo       n^2 >= 2^4093, as close above as possible (the smallest N classical_ok admits)
  mont_hi      n^2 < 2^4093, as close below as possible (the largest N on the Montgomery pair)
and two Paillier-1024 keys (512-bit primes) for the one-lane kernels:
  p1024_lo     n just above 2^1023
  p1024_hi     the two largest primes below 2^512 (n just below 2^1024)

"Just above T" (n >= T):  p = next_prime(isqrt(T) - 2^(hb-24)),  q = the smallest prime >= ceil(T / p);
"just below T" (n < T):   p = next_prime(isqrt(T) - 2^(hb/2+8)), q = the largest prime <= (T - 1) // p
(hb: bits of a prime).  n - T stays below about 2^(hb+11), so the top ~hb-11 bits of n (and of N) are
100...0 or 011...1: long 0x00 / 0xff runs that no random key has.

Primes come from the library's host prime search (fthe_next_prime, pinned to "the smallest prime above
the start" by tests/test_next_prime.py); only the primes are stored, as hex.

  python tests/golden/make_n2_edge_keys.py        (a few seconds)
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def make_keys(next_prime):
    """next_prime(x) -> the smallest prime > x.  Returns {name: (prime bits, p, q)}."""
    def prev_prime(x):
        """the largest prime <= x"""
        span = 1 << 12
        while True:
            y, best = x - span, None
            while True:
                y = next_prime(y)
                if y > x:
                    break
                best = y
            if best:
                return best
            span <<= 1

    def above(T, hb):
        p = next_prime(math.isqrt(T) - (1 << (hb - 24)))
        q = next_prime(-(-T // p) - 1)
        assert p != q and p * q >= T
        return hb, p, q

    def below(T, hb):
        p = next_prime(math.isqrt(T) - (1 << (hb // 2 + 8)))
        q = prev_prime((T - 1) // p)
        assert p != q and p * q < T
        return hb, p, q

    def largest(hb):
        q = prev_prime((1 << hb) - 1)
        return hb, prev_prime(q - 1), q

    return {
        "addb_lo": above(1 << 2047, 1024),
        "addb_hi": largest(1024),
        "addb_mid_hi": above(math.isqrt(1 << 4095) + 1, 1024),
        "addb_mid_lo": below(math.isqrt(1 << 4095) + 1, 1024),
        "cls_hi": below(1 << 2047, 1024),
        "cls_lo": above(math.isqrt(1 << 4093) + 1, 1024),
        "mont_hi": below(math.isqrt(1 << 4093) + 1, 1024),
        "p1024_lo": above(1 << 1023, 512),
        "p1024_hi": largest(512),
    }


def main():
    import numpy as np
    import pyoracle
    from fedtree_amd import _lib
    lib = _lib.load()

    def next_prime(x):
        nw = (x.bit_length() + 31) // 32
        w = np.asarray(pyoracle.to_words(x, nw), dtype=np.uint32)
        out = np.zeros(nw + 1, dtype=np.uint32)
        assert lib.fthe_next_prime(w.ctypes.data, nw, out.ctypes.data, nw + 1) == 0
        return pyoracle.from_words(out)

    keys = make_keys(next_prime)
    for name, (hb, p, q) in keys.items():
        assert p.bit_length() == hb and q.bit_length() == hb, name
    out = {
        "what": "edge keys of the mod-n^2 product kernels' dispatch (make_n2_edge_keys.py): primes as hex",
        "keys": {name: {"prime_bits": hb, "p": hex(p), "q": hex(q)} for name, (hb, p, q) in keys.items()},
    }
    with open(os.path.join(HERE, "n2_edge_keys.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for name, (hb, p, q) in keys.items():
        n = p * q
        print(f"{name:12s} n {n.bit_length()} bits, n^2 {(n * n).bit_length()} bits")


if __name__ == "__main__":
    main()
