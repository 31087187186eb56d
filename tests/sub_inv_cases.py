"""Shared cases of the batched-inverse tests (include/fthe.h fthe_invert / fthe_sub_inv): keys, operand rows and
the Python reference a * pow(b, -1, n^2) * (1 + offset n) % n^2.  Used by tests/test_gpu_sub_inv.py and by the
child process it starts with FTHE_INV_CHUNK set (this file run as a script)."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0x5A5A5A5A


def key_2041():
    """Primes of a key whose n has 2,041 bits (tests/golden/n2_edge_keys.json holds none):
    tests/golden/sub_inv_key_2041.json."""
    import json
    with open(os.path.join(HERE, "golden", "sub_inv_key_2041.json")) as f:
        g = json.load(f)
    p, q = int(g["p"], 16), int(g["q"], 16)
    assert (p * q).bit_length() == 2041
    return p, q


def unit_rows(n, count, seed):
    """count random units mod n^2 (Python integers)."""
    rng = np.random.default_rng(seed)
    n2, nb = n * n, (2 * n.bit_length() + 7) // 8 + 8
    out = []
    while len(out) < count:
        x = int.from_bytes(rng.bytes(nb), "little") % n2
        if math.gcd(x, n) == 1:
            out.append(x)
    return out


def operands(n, count, seed):
    """(a, b) of `count` rows: random units, with b's first rows the integer 1, n + 1 and n^2 - 1 (its own
    inverse) and, from five rows on, a last row with b == a."""
    a, b = unit_rows(n, count, seed), unit_rows(n, count, seed + 1000)
    for j, special in enumerate((1, n + 1, n * n - 1)):
        if j < count:
            b[j] = special
    if count >= 5:
        a[-1] = b[-1]
    return a, b


def want_sub_inv(n, a, b, offset=0):
    n2 = n * n
    c = (1 + offset * n) % n2
    return [x * pow(y, -1, n2) * c % n2 for x, y in zip(a, b)]


def offsets(n_words, seed):
    """No offset, a one-word offset, and one of n_words words."""
    rng = np.random.default_rng(seed)
    return [None, 0xDEADBEEF, int.from_bytes(rng.bytes(4 * n_words), "little") | 1 << (32 * n_words - 1)]


def non_units(n, p, seed):
    """Rows that are no units mod n^2: n, p times a unit, and 0."""
    return [n, p * unit_rows(n, 1, seed)[0] % (n * n), 0]


def _chunk_child():
    """Run with FTHE_INV_CHUNK=8: counts on both sides of the chunk boundaries against Python at the 2,048- and
    512-bit golden keys, aliased outputs across chunks, and a non-unit in the last chunk that must leave `out`
    as it was."""
    sys.path.insert(0, HERE)
    import torch
    import conftest                                      # noqa: F401  (puts the package and the oracle on the path)
    import pyoracle
    from conftest import GOLDEN_KEYS, golden_key, load_golden
    from fedtree_amd import _lib
    from fedtree_amd.paillier import Device, Paillier
    assert os.environ.get("FTHE_INV_CHUNK") == "8"
    dev = Device(0)

    def t(ints, cw):
        return torch.from_numpy(pyoracle.ints_to_words(ints, cw).view(np.int32)).cuda()

    def ints(x):
        return pyoracle.words_to_ints(x.cpu().numpy().view(np.uint32))

    for name in (GOLDEN_KEYS[2], GOLDEN_KEYS[0]):
        p, q = golden_key(load_golden(name))
        pl = Paillier.from_primes(p, q, dev)
        n, cw = pl.modulus, 2 * pl.n_words
        off = offsets(pl.n_words, 3)[2]
        for count in (8, 9, 19, 24):
            a, b = operands(n, count, count)
            want, winv = want_sub_inv(n, a, b, off), want_sub_inv(n, [1] * count, b)
            assert pyoracle.words_to_ints(pl.sub_inv_batch(pyoracle.ints_to_words(a, cw),
                                                           pyoracle.ints_to_words(b, cw), off)) == want, (name, count)
            assert pyoracle.words_to_ints(pl.invert_batch(pyoracle.ints_to_words(b, cw))) == winv, (name, count)
            for alias in (None, 0, 1):
                ad, bd = t(a, cw), t(b, cw)
                out = torch.zeros_like(ad) if alias is None else (ad, bd)[alias]
                pl.sub_inv_dev(ad, bd, out, off)
                dev.sync()
                assert ints(out) == want, (name, count, alias)
            xd = t(b, cw)
            pl.invert_dev(xd, xd)
            dev.sync()
            assert ints(xd) == winv, (name, count)
        # a non-unit in the last chunk: nothing is written, not even the chunks before it
        a, b = operands(n, 19, 77)
        for bad in non_units(n, p, 5):
            bb = list(b)
            bb[17] = bad
            ad, bd = t(a, cw), t(bb, cw)
            out = torch.full_like(ad, SENTINEL)
            for call in (lambda: pl.sub_inv_dev(ad, bd, out, off), lambda: pl.invert_dev(bd, out),
                         lambda: pl.sub_inv_dev(ad, bd, bd, off)):
                try:
                    call()
                    raise AssertionError("a non-unit row was accepted")
                except _lib.FtheError as e:
                    assert e.status == _lib.FTHE_ERR_ARG
            dev.sync()
            assert bool((out == SENTINEL).all()) and ints(bd) == bb and ints(ad) == a, (name, bad == 0)
            pl.sub_inv_dev(ad, t(b, cw), out, off)       # the context goes on working
            dev.sync()
            assert ints(out) == want_sub_inv(n, a, b, off)
    print("sub_inv chunk child OK")


if __name__ == "__main__":
    _chunk_child()
