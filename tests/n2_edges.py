"""Shared helpers of the mod-n^2 edge tests (tests/golden/n2_edge_keys.json, made by
tests/golden/make_n2_edge_keys.py): the keys, the regime each one must land in, and the hostile operand rows."""
import json
import os
import random

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# regime by N = n^2 of a Paillier-2048 key: "addb" N >= 2^4094 (fthe_addb_q152), "cls" 2^4093 <= N < 2^4094
# (MULWC / MULWGC on the four-lane kernel), "mont" N < 2^4093 (Montgomery product + R^2 correction)
REGIME = {"addb_lo": "addb", "addb_hi": "addb", "addb_mid_hi": "addb", "addb_mid_lo": "addb",
          "cls_hi": "cls", "cls_lo": "cls", "mont_hi": "mont"}
KEYS_2048 = list(REGIME)
KEYS_1024 = ["p1024_lo", "p1024_hi"]
ADDB_KEYS = [k for k in KEYS_2048 if REGIME[k] == "addb"]


def load_keys():
    """{name: (p, q)}"""
    with open(os.path.join(GOLDEN, "n2_edge_keys.json")) as f:
        g = json.load(f)
    return {name: (int(v["p"], 16), int(v["q"], 16)) for name, v in g["keys"].items()}


def modulus(name):
    p, q = load_keys()[name]
    return (p * q) ** 2


def regime_of(N):
    """the regime the table above gives a 4093..4096-bit N"""
    return "addb" if N >= 1 << 4094 else "cls" if N >= 1 << 4093 else "mont"


def hostile_rows(N, bits=4096, nrand=0, seed=1):
    """The operand set E for modulus N in rows of `bits` bits: canonical extremes, rows >= N (not ciphertexts;
    the reference's x y mod n^2 reduces them all the same), the largest rows congruent to -1 and 0, then
    nrand random rows below N."""
    top = (1 << bits) - 1
    kN = top // N * N
    e = [0, 1, 2, N - 1, N - 2, N // 2, N - (1 << 64), 1 << (bits - 96), (1 << 27) - 1, N, N + 12345,
         (1 << (bits - 24)) - 1, 1 << (bits - 24), top, kN - 1, kN]
    assert all(0 <= x <= top for x in e)
    rng = random.Random(seed)
    return e + [rng.randrange(N) for _ in range(nrand)]
