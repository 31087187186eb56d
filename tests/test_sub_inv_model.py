"""Subtraction by the modular inverse (include/fthe.h fthe_sub_inv) on Python integers, no device.

The plaintext of a * b^-1 * (1 + offset n) mod n^2 is (m_a - m_b + offset) mod n.  With offset = 2^bits_b, where
T_b < 2^bits_b, the packed plaintext T = T_a - T_b + 2^bits_b lies in [0, 2^(max(bits_a, bits_b) + 1)), equals
T_a - T_b mod 2^W and so decodes by the packed rule; in a slot-packed plaintext the same holds slot by slot.  The
rule is checked at the three golden keys on sums of 1, 8 and 4,096 full-range codes, once and chained, together
with packed_bits_after("sub_inv"), the bound logic of GHPairs.sub_inv, and the presence of the C ABI."""
import ctypes

import numpy as np
import pytest

from conftest import GOLDEN_KEYS, golden_key, load_golden
from gh_packed_cases import EDGE_CODES, I64_MAX, I64_MIN, W, pack_int, unpack_int, wrap64

from fedtree_amd import _lib
from fedtree_amd.paillier import (GH_PACKED_BITS, GHPairs, gh_slot_count, gh_slot_rows, packed_bits_after)

ADDENDS = (1, 8, 4096)
NEW_SYMBOLS = ("fthe_invert_dev", "fthe_invert", "fthe_sub_inv_dev", "fthe_sub_inv")


def _modulus(name):
    p, q = golden_key(load_golden(name))
    return p * q


def _sum_of_codes(k, seed, extreme=None):
    """A packed sum of k codes drawn from EDGE_CODES (extreme: every addend that (g, h) pair): the plaintext
    integer, its bound in bits, and the true sums of the g and h codes."""
    rng = np.random.default_rng(seed)
    if extreme is None:
        gi, hi = rng.integers(0, len(EDGE_CODES), k), rng.integers(0, len(EDGE_CODES), k)
        cg, ch = [EDGE_CODES[i] for i in gi], [EDGE_CODES[i] for i in hi]
    else:
        cg, ch = [extreme[0]] * k, [extreme[1]] * k
    t = sum(pack_int(a, b) for a, b in zip(cg, ch))
    bits = packed_bits_after("sum", GH_PACKED_BITS, k=k)
    assert t.bit_length() <= bits
    return t, bits, sum(cg), sum(ch)


def _operands(count):
    """count operands (T, bits, sum_g, sum_h) over the three addend counts, the all-extreme sums first."""
    ext = [(I64_MIN, I64_MIN), (I64_MAX, I64_MAX), (I64_MIN, I64_MAX), (I64_MAX, I64_MIN), (-1, -1), (0, 0)]
    out = []
    for i in range(count):
        k = ADDENDS[i % len(ADDENDS)]
        out.append(_sum_of_codes(k, seed=i, extreme=ext[i // 3] if i // 3 < len(ext) else None))
    return out


def _sub_inv_plain(n, ta, tb, offset):
    """The plaintext the ciphertext a * b^-1 * (1 + offset n) decrypts to."""
    return (ta - tb + offset) % n


def test_packed_bits_after_sub_inv():
    assert packed_bits_after("sub_inv", 192, 192) == 193
    assert packed_bits_after("sub_inv", 204, 192) == 205 == packed_bits_after("sub_inv", 192, 204)
    assert packed_bits_after("sub", 192, 192) == 385        # the rule of `-` is untouched
    # two subtractions of the vertical flow: 194 bits where `-` needs 578, so 224-bit slots still hold them
    one = packed_bits_after("sub_inv", 192, 192)
    assert packed_bits_after("sub_inv", one, one) == 194 <= 224
    assert packed_bits_after("sub", packed_bits_after("sub", 192, 192), packed_bits_after("sub", 192, 192)) == 578


@pytest.mark.parametrize("name", GOLDEN_KEYS)
def test_offset_rule_on_packed_sums(name):
    n = _modulus(name)
    ops = _operands(30)
    for i, (ta, ba, ga, ha) in enumerate(ops):
        tb, bb, gb, hb = ops[(i + 7) % len(ops)]
        tc, bc, gc, hc = ops[(i + 13) % len(ops)]
        # one subtraction
        t1 = _sub_inv_plain(n, ta, tb, 1 << bb)
        b1 = packed_bits_after("sub_inv", ba, bb)
        assert t1 == ta - tb + (1 << bb) and 0 <= t1 < 1 << b1 < n
        assert t1 % 2**W == (ta - tb) % 2**W
        assert unpack_int(t1) == (wrap64(ga - gb), wrap64(ha - hb))
        # chained: (a - b) - c
        t2 = _sub_inv_plain(n, t1, tc, 1 << bc)
        b2 = packed_bits_after("sub_inv", b1, bc)
        assert 0 <= t2 == t1 - tc + (1 << bc) < 1 << b2 < n
        assert unpack_int(t2) == (wrap64(ga - gb - gc), wrap64(ha - hb - hc))
        # a difference as the right-hand side: a - (b - c)
        t3 = _sub_inv_plain(n, ta, _sub_inv_plain(n, tb, tc, 1 << bc), 1 << packed_bits_after("sub_inv", bb, bc))
        assert 0 <= t3 < 1 << packed_bits_after("sub_inv", ba, packed_bits_after("sub_inv", bb, bc))
        assert unpack_int(t3) == (wrap64(ga - gb + gc), wrap64(ha - hb + hc))
        # no offset: a negative difference wraps mod n and no longer decodes -- the offset is needed
        if ta < tb:
            assert _sub_inv_plain(n, ta, tb, 0) == n + ta - tb >= 1 << b1


@pytest.mark.parametrize("name", GOLDEN_KEYS)
@pytest.mark.parametrize("slot_bits", [224, 256])
def test_offset_rule_in_every_slot(name, slot_bits):
    n = _modulus(name)
    slots = gh_slot_count(n.bit_length(), slot_bits)
    assert slots >= 1
    count = 3 * slots + 1
    rows = gh_slot_rows(count, slots)
    a, b, c = _operands(count), _operands(2 * count)[count:], _operands(3 * count)[2 * count:]

    def layout(ts):
        out = [0] * rows
        for i, t in enumerate(ts):
            out[i % rows] += t << ((i // rows) * slot_bits)
        return out

    def slot(row, j):
        return (row >> (j * slot_bits)) % 2**slot_bits

    ba, bb, bc = (max(x[1] for x in s) for s in (a, b, c))
    b1 = packed_bits_after("sub_inv", ba, bb)
    b2 = packed_bits_after("sub_inv", b1, bc)
    assert b2 <= slot_bits
    ra, rb, rc = layout([x[0] for x in a]), layout([x[0] for x in b]), layout([x[0] for x in c])
    off1 = sum(1 << (j * slot_bits + bb) for j in range(slots))
    off2 = sum(1 << (j * slot_bits + bc) for j in range(slots))
    r1 = [_sub_inv_plain(n, x, y, off1) for x, y in zip(ra, rb)]
    r2 = [_sub_inv_plain(n, x, y, off2) for x, y in zip(r1, rc)]
    assert max(r1 + r2) < 2**(n.bit_length() - 1)
    for i in range(count):
        t1, t2 = slot(r1[i % rows], i // rows), slot(r2[i % rows], i // rows)
        assert t1 == a[i][0] - b[i][0] + (1 << bb) < 1 << b1
        assert t2 == t1 - c[i][0] + (1 << bc) < 1 << b2
        assert unpack_int(t1) == (wrap64(a[i][2] - b[i][2]), wrap64(a[i][3] - b[i][3]))
        assert unpack_int(t2) == (wrap64(a[i][2] - b[i][2] - c[i][2]), wrap64(a[i][3] - b[i][3] - c[i][3]))
    # slots past the last bin hold the bare offsets and nothing else
    for i in range(count, slots * rows):
        assert slot(r1[i % rows], i // rows) == 1 << bb


class _Key:
    """What GHPairs.sub_inv reads of a Paillier object; records the offsets it is asked for."""

    def __init__(self, name):
        p, q = golden_key(load_golden(name))
        self.p, self.modulus = p, p * q
        self.offsets = []

    def sub_inv_batch(self, a, b, offset=None):
        self.offsets.append(offset)
        return a


def _encrypted(key, count, pt_bits, slot_bits=0, slots=0, packed=True):
    t = GHPairs(np.zeros(count, np.float32), paillier=key, packed=packed)
    t.g_enc = np.zeros((gh_slot_rows(count, slots) if slot_bits else count, 2), np.uint32)
    t.h_enc = None if packed else t.g_enc
    t.encrypted, t.pt_bits, t.slot_bits, t.slots = True, pt_bits, slot_bits, slots
    return t


def test_ghpairs_sub_inv_bounds_without_a_device():
    key = _Key(GOLDEN_KEYS[2])
    d = _encrypted(key, 19, 204).sub_inv(_encrypted(key, 19, 192))
    assert (d.pt_bits, d.slot_bits, d.packed, d.encrypted, len(d)) == (205, 0, True, True, 19)
    assert key.offsets == [1 << 192]
    d = _encrypted(key, 19, 192).sub_inv(_encrypted(key, 19, 204))
    assert d.pt_bits == 205 and key.offsets[-1] == 1 << 204
    # slot-packed: the offset in every slot; the result keeps its layout
    key.offsets.clear()
    s = _encrypted(key, 19, 200, 224, 9).sub_inv(_encrypted(key, 19, 193, 224, 9))
    assert (s.pt_bits, s.slot_bits, s.slots, len(s)) == (201, 224, 9, 19)
    assert key.offsets == [sum(1 << (224 * j + 193) for j in range(9))]
    # refused before any device work
    key.offsets.clear()
    with pytest.raises(ValueError, match="225 bits"):
        _encrypted(key, 19, 224, 224, 9).sub_inv(_encrypted(key, 19, 192, 224, 9))
    for other in (_encrypted(key, 19, 192, 256, 7), _encrypted(key, 18, 192, 224, 9), _encrypted(key, 19, 192, 224, 8)):
        with pytest.raises(ValueError, match="differ"):
            _encrypted(key, 19, 192, 224, 9).sub_inv(other)
    with pytest.raises(ValueError, match="slot-packed"):
        _encrypted(key, 19, 192, 224, 9).sub_inv(_encrypted(key, 19, 192))
    with pytest.raises(ValueError, match="slot-packed"):
        _encrypted(key, 19, 192).sub_inv(_encrypted(key, 19, 192, 224, 9))
    with pytest.raises(ValueError, match="packed"):
        _encrypted(key, 19, 64, packed=False).sub_inv(_encrypted(key, 19, 64, packed=False))
    with pytest.raises(ValueError, match="packed"):
        _encrypted(key, 19, 64, packed=False).sub_inv(GHPairs(np.zeros(19, np.float32)))
    assert key.offsets == []
    # neither side encrypted: plain floats, as `-`
    p = GHPairs(np.array([1.5, 2.0], np.float32)).sub_inv(GHPairs(np.array([0.5, 3.0], np.float32)))
    assert p.g.tolist() == [1.0, -1.0] and not p.encrypted


def test_abi_symbols_and_null_arguments():
    lib = _lib.load()
    P, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    want = {"fthe_invert_dev": [P, P, P, SZ, P], "fthe_invert": [P, P, P, SZ, P],
            "fthe_sub_inv_dev": [P, P, P, P, SZ, P, I, P], "fthe_sub_inv": [P, P, P, P, SZ, P, I, P]}
    assert set(NEW_SYMBOLS) <= set(_lib.header_symbols())
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[name], name
    buf = (ctypes.c_uint32 * 64)()
    for count in (0, 3):
        assert lib.fthe_invert_dev(None, None, buf, count, buf) == _lib.FTHE_ERR_ARG
        assert lib.fthe_invert(None, None, buf, count, buf) == _lib.FTHE_ERR_ARG
        assert lib.fthe_sub_inv_dev(None, None, buf, buf, count, None, 0, buf) == _lib.FTHE_ERR_ARG
        assert lib.fthe_sub_inv(None, None, buf, buf, count, None, 0, buf) == _lib.FTHE_ERR_ARG
    assert all(v == 0 for v in buf)
