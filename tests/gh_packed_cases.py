"""Shared cases and the plain-integer model of the packed gradient pairs (include/fthe.h FTHE_GH_*):
one plaintext M = code(g) + code(h) 2^96 mod 2^192 per pair.  Everything here is Python integers, the
yardstick the numpy mirror (fedtree_amd.paillier.pack_gh / unpack_gh) and the device kernels are held to."""
import json
import os

import numpy as np

S, W = 96, 192
I64_MIN, I64_MAX = -2**63, 2**63 - 1
EDGE_CODES = [0, 1, -1, I64_MAX, I64_MIN]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def code(x):
    """(int64)((double)x * 1e6) of a float32 x (common.h:81-86), for x whose code fits."""
    return int(float(np.float32(x)) * 1e6)          # int(): truncation toward zero


def wrap64(v):
    """The int64 a two's-complement 64-bit register holds for the integer v."""
    v &= 2**64 - 1
    return v - 2**64 if v >= 2**63 else v


def pack_int(cg, ch):
    return (cg + ch * 2**S) % 2**W


def unpack_int(t):
    """The issue's decode rule on a plaintext integer t -> (g64, h64)."""
    t %= 2**W
    lo = t % 2**S
    g_s = lo - 2**S if lo >= 2**(S - 1) else lo
    hi = ((t - g_s) >> S) % 2**S
    return wrap64(g_s), wrap64(hi)


def codec_floats():
    """Every float of tests/golden/codec.json."""
    with open(os.path.join(GOLDEN, "codec.json")) as f:
        bits = json.load(f)["floats_f32_bits"]
    return np.array(bits, dtype=np.uint32).view(np.float32)


def float_pairs():
    """(g, h) float32 arrays: every codec.json value as g and as h, FedTree's hessian floor 1e-16 (code 0),
    the four sign combinations (a negative g borrows from the h field), codes of +-1 and codes next to
    +-2^63 (the largest floats whose code fits)."""
    v = codec_floats()
    g = list(v) + list(v[::-1]) + [0.5, -0.5, 0.5, -0.5, 0.0, 1.5e-6, -1.5e-6, 9.2e12, -9.2e12, 9.2e12, 0.25]
    h = list(v[::-1]) + list(v) + [0.25, 0.25, -0.25, -0.25, 1e-16, -1.5e-6, 1.5e-6, -9.2e12, 9.2e12, 9.2e12, 1e-16]
    return np.array(g, dtype=np.float32), np.array(h, dtype=np.float32)


def padded_float_pairs(count, seed=5):
    """float_pairs() padded with random gradients to `count` pairs."""
    g, h = float_pairs()
    rng = np.random.default_rng(seed)
    k = count - len(g)
    assert k >= 0
    return (np.concatenate([g, rng.normal(0, 1, k).astype(np.float32)]),
            np.concatenate([h, rng.uniform(1e-16, 0.25, k).astype(np.float32)]))


def words_of(values, nw):
    """Python integers -> (count, nw) little-endian uint32 words."""
    out = np.zeros((len(values), nw), dtype=np.uint32)
    for i, v in enumerate(values):
        out[i] = [(v >> (32 * j)) & 0xFFFFFFFF for j in range(nw)]
    return out


def int_of(row):
    v = 0
    for x in np.asarray(row, dtype=np.uint64)[::-1]:
        v = (v << 32) | int(x)
    return v
