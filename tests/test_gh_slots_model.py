"""Slot-packed pairs (include/fthe.h FTHE_GH_SLOT_*) against Python integers, no device.

The numpy statement of the layout (fedtree_amd.paillier.pack_gh_slots / split_gh_slots / unpack_gh_slots) is
held to the integer form sum_j T_{j rows + i} 2^(j slot_bits) at the three golden key sizes, the Horner
identity of the compress is checked on plaintexts that carry a subtraction's residue, and the bound logic of
GHPairs is exercised on objects built by hand.  Every comparison is exact."""
import numpy as np
import pytest

from conftest import GOLDEN_KEYS, golden_key, load_golden
from gh_packed_cases import EDGE_CODES, I64_MAX, I64_MIN, W, int_of, pack_int, unpack_int, words_of, wrap64

from fedtree_amd.paillier import (GH_PACKED_BITS, GH_SLOT_BITS_MIN, GHPairs, gh_slot_count, gh_slot_rows,
                                  pack_codes, pack_gh_slots, packed_bits_after, split_gh_slots, unpack_gh_slots)

SLOT_BITS = (224, 256, 416)


def _n_bits(name):
    p, q = golden_key(load_golden(name))
    return (p * q).bit_length(), p.bit_length()


def _codes(count, seed):
    """count (g, h) code pairs: every pair of edge codes first, then full-range random codes."""
    rng = np.random.default_rng(seed)
    pairs = [(a, b) for a in EDGE_CODES for b in EDGE_CODES]
    g = [p[0] for p in pairs] + rng.integers(I64_MIN, I64_MAX, count, dtype=np.int64, endpoint=True).tolist()
    h = [p[1] for p in pairs] + rng.integers(I64_MIN, I64_MAX, count, dtype=np.int64, endpoint=True).tolist()
    off = (seed * 7) % len(pairs)                        # rotate, so short counts see different edge pairs
    return (g[off:] + g[:off])[:count], (h[off:] + h[:off])[:count]


def _row_ints(ts, slot_bits, slots):
    """The normative layout on integers: row i = sum_j T_{j rows + i} 2^(j slot_bits)."""
    rows = gh_slot_rows(len(ts), slots)
    out = [0] * rows
    for b, t in enumerate(ts):
        assert 0 <= t < 2**slot_bits
        out[b % rows] += t << ((b // rows) * slot_bits)
    return out


def test_slot_counts():
    assert GH_SLOT_BITS_MIN == GH_PACKED_BITS + 32 == 224
    bits = [_n_bits(name) for name in GOLDEN_KEYS]
    assert [b[0] for b in bits] == [512, 1023, 2048]
    assert [gh_slot_count(b[0], 224) for b in bits] == [2, 4, 9]
    assert gh_slot_count(bits[2][1], 224) == 4           # the short decrypt of Paillier-2048
    assert gh_slot_count(224, 224) == 0 and gh_slot_count(225, 224) == 1
    assert gh_slot_count(512, 608) == 0
    for bad in (192, 200, 230, 0, -32):
        with pytest.raises(ValueError):
            gh_slot_count(2048, bad)


@pytest.mark.parametrize("name", GOLDEN_KEYS)
@pytest.mark.parametrize("slot_bits", SLOT_BITS)
def test_pack_unpack_vs_integers(name, slot_bits):
    n_bits, _ = _n_bits(name)
    slots = gh_slot_count(n_bits, slot_bits)
    assert slots == (n_bits - 1) // slot_bits and slots >= 1
    sw = slot_bits // 32
    for count in sorted({0, 1, max(slots - 1, 0), slots, slots + 1, 3 * slots + 1}):
        cg, ch = _codes(count, seed=count + slot_bits)
        ts = [pack_int(a, b) for a, b in zip(cg, ch)]
        words = pack_codes(np.array(cg, np.int64), np.array(ch, np.int64))
        rows = pack_gh_slots(words, slot_bits, slots)
        nrows = gh_slot_rows(count, slots)
        assert rows.shape == (nrows, slots * sw) and rows.dtype == np.uint32
        want = _row_ints(ts, slot_bits, slots)
        assert [int_of(r) for r in rows] == want
        assert all(v < 2**(n_bits - 1) for v in want)    # below the modulus
        # decode: every bin from its slot, at the row width and from rows as wide as a plaintext of n
        for width in (slots * sw, (n_bits + 31) // 32):
            wide = words_of(want, width)
            assert [int_of(r) for r in split_gh_slots(wide, count, slot_bits, slots)] == ts
            g, h, dg, dh = unpack_gh_slots(wide, count, slot_bits, slots, codes=True)
            assert (dg.tolist(), dh.tolist()) == (list(cg), list(ch))
            assert len(g) == len(h) == count


@pytest.mark.parametrize("parties", [8, 4096])
def test_sums_of_parties_stay_in_their_slots(parties):
    """Adding slot-packed plaintexts adds slot by slot: sums of full-range codes of 8 and 4,096 parties (well
    within the 2^32 addends a 224-bit slot leaves room for) decode to the wrapped sums of the codes."""
    n_bits, slot_bits = 2048, 224
    slots = gh_slot_count(n_bits, slot_bits)
    count = 3 * slots + 1
    rng = np.random.default_rng(parties)
    sum_g, sum_h, total = [0] * count, [0] * count, [0] * gh_slot_rows(count, slots)
    extreme = {0: (I64_MIN, I64_MIN), 1: (I64_MAX, I64_MAX), 2: (I64_MIN, I64_MAX), 3: (-1, -1)}
    for k in range(parties):
        cg = rng.integers(I64_MIN, I64_MAX, count, dtype=np.int64, endpoint=True)
        ch = rng.integers(I64_MIN, I64_MAX, count, dtype=np.int64, endpoint=True)
        for b, (a, c) in extreme.items():                # bins whose every addend is an extreme
            cg[b], ch[b] = a, c
        rows = pack_gh_slots(pack_codes(cg, ch), slot_bits, slots)
        total = [t + int_of(r) for t, r in zip(total, rows)]
        sum_g = [s + int(v) for s, v in zip(sum_g, cg)]
        sum_h = [s + int(v) for s, v in zip(sum_h, ch)]
    assert max(total) < 2**(n_bits - 1)
    wide = words_of(total, n_bits // 32)
    _, _, dg, dh = unpack_gh_slots(wide, count, slot_bits, slots, codes=True)
    assert dg.tolist() == [wrap64(s) for s in sum_g]
    assert dh.tolist() == [wrap64(s) for s in sum_h]
    ts = [int_of(r) for r in split_gh_slots(wide, count, slot_bits, slots)]
    assert max(t.bit_length() for t in ts) <= packed_bits_after("sum", GH_PACKED_BITS, k=parties) <= slot_bits
    assert [unpack_int(t) for t in ts] == [(wrap64(a), wrap64(b)) for a, b in zip(sum_g, sum_h)]


@pytest.mark.parametrize("name", GOLDEN_KEYS)
def test_horner_identity_with_subtraction_residue(name):
    """The compress on the plaintext side: T = a + b (2^W - 1), what fthe_sub_bits leaves for a - b, is up to
    2 W bits wide; in slots of 416 bits Horner's x <- x 2^slot_bits + T_j rebuilds the layout, and every slot
    decodes to the difference of the codes, residue and all."""
    n_bits, _ = _n_bits(name)
    slot_bits = 416
    slots = gh_slot_count(n_bits, slot_bits)
    assert slots == {512: 1, 1023: 2, 2048: 4}[n_bits]
    count = 3 * slots + 1
    ag, ah = _codes(count, seed=1)
    bg, bh = _codes(count, seed=2)
    ts = [pack_int(a, c) + pack_int(b, d) * (2**W - 1) for a, c, b, d in zip(ag, ah, bg, bh)]
    assert max(t.bit_length() for t in ts) <= packed_bits_after("sub", W, W) <= slot_bits
    assert any(t >= 2**W for t in ts)                    # the residue is there
    rows = gh_slot_rows(count, slots)
    horner = []
    for i in range(rows):
        planes = [ts[j * rows + i] for j in range(slots) if j * rows + i < count]
        acc = planes[-1]
        for t in reversed(planes[:-1]):
            acc = (acc << slot_bits) + t                 # slot_bits squarings, then one product
        horner.append(acc)
    assert horner == _row_ints(ts, slot_bits, slots)
    assert max(horner) < 2**(n_bits - 1)
    wide = words_of(horner, (n_bits + 31) // 32)
    assert [int_of(r) for r in split_gh_slots(wide, count, slot_bits, slots)] == ts
    _, _, dg, dh = unpack_gh_slots(wide, count, slot_bits, slots, codes=True)
    assert dg.tolist() == [wrap64(a - b) for a, b in zip(ag, bg)]
    assert dh.tolist() == [wrap64(a - b) for a, b in zip(ah, bh)]
    # the numpy pack takes such grown plaintexts too
    assert [int_of(r) for r in pack_gh_slots(words_of(ts, slot_bits // 32), slot_bits, slots)] == horner
    with pytest.raises(ValueError):
        pack_gh_slots(words_of(ts, slot_bits // 32), 224, 1)


class _Key:
    """What GHPairs' bound logic reads of a Paillier object."""

    def __init__(self, name):
        p, q = golden_key(load_golden(name))
        self.p, self.modulus = p, p * q

    def add_batch(self, a, b):                           # the rows do not matter to the bound logic
        return a


def _encrypted(key, count, pt_bits, slot_bits=0, slots=0):
    t = GHPairs(np.zeros(count, np.float32), paillier=key, packed=True)
    rows = gh_slot_rows(count, slots) if slot_bits else count
    t.g_enc = np.zeros((rows, 2), np.uint32)
    t.encrypted, t.pt_bits, t.slot_bits, t.slots = True, pt_bits, slot_bits, slots
    return t


def test_ghpairs_bounds_without_a_device():
    k512, k2048 = _Key(GOLDEN_KEYS[0]), _Key(GOLDEN_KEYS[2])
    assert GHPairs(np.zeros(3, np.float32)).slot_bits == 0
    # + : the add rule, refused once the bound passes the slot
    a, b = _encrypted(k2048, 19, 223, 224, 9), _encrypted(k2048, 19, 224, 224, 9)
    with pytest.raises(ValueError, match="225 bits"):
        a + b
    s = _encrypted(k2048, 19, 192, 224, 9) + _encrypted(k2048, 19, 200, 224, 9)
    assert (s.pt_bits, s.slot_bits, s.slots, len(s), s.encrypted, s.packed) == (201, 224, 9, 19, True, True)
    assert (a + a).pt_bits == 224                        # exactly the slot: still allowed
    with pytest.raises(ValueError, match="differ"):
        a + _encrypted(k2048, 19, 192, 256, 8)
    with pytest.raises(ValueError, match="differ"):
        a + _encrypted(k2048, 18, 192, 224, 9)
    with pytest.raises(ValueError, match="slot-packed"):
        a + _encrypted(k2048, 19, 192)                   # a pair-packed batch
    with pytest.raises(ValueError, match="slot-packed"):
        _encrypted(k2048, 19, 192) + a
    with pytest.raises(ValueError, match="slot-packed"):
        a + GHPairs(np.zeros(19, np.float32))
    # - and the histogram methods
    from fedtree_amd.paillier import HEParty
    for lhs, rhs in ((a, b), (a, _encrypted(k2048, 19, 192)), (_encrypted(k2048, 19, 192), a),
                     (a, GHPairs(np.zeros(19, np.float32)))):
        with pytest.raises(ValueError, match="not defined on slot-packed"):
            lhs - rhs
    with pytest.raises(ValueError, match="not defined on slot-packed"):
        HEParty.sibling_histogram(a, b)
    with pytest.raises(ValueError, match="not defined on slot-packed"):
        HEParty(k2048).prefix_histogram(a, np.array([0, 19]))
    with pytest.raises(ValueError, match="not defined on slot-packed"):
        HEParty(k2048).compute_histogram(a, np.zeros(19, np.uint8), np.array([0, 4]), 16)
    # compress: the default width, and a key too small for it
    missing = _encrypted(k512, 5, packed_bits_after("sub", 393, 393))       # ~586 bits: no slot below a 512-bit n
    with pytest.raises(ValueError, match="do not fit below n"):
        missing.compress()
    with pytest.raises(ValueError, match="do not fit slots"):
        _encrypted(k2048, 5, 400).compress(slot_bits=384)
    with pytest.raises(ValueError):
        _encrypted(k2048, 5, 192).compress(slot_bits=200)
    with pytest.raises(ValueError, match="pair-packed"):
        a.compress()
    with pytest.raises(ValueError, match="do not fit below n"):
        _encrypted(k2048, 5, 192).compress(slots=10)
    # homo_encrypt: slot_bits needs a packed batch, and a key with room
    with pytest.raises(ValueError, match="packed"):
        GHPairs(np.zeros(3, np.float32)).homo_encrypt(k2048, slot_bits=224)
    with pytest.raises(ValueError, match="do not fit below n"):
        GHPairs(np.zeros(3, np.float32), packed=True).homo_encrypt(k512, slot_bits=512)
    # homo_decrypt: a layout built for the full decrypt does not go through the short one
    with pytest.raises(ValueError, match="do not fit below p"):
        a.homo_decrypt(k2048, short=True)
    grown = _encrypted(k2048, 19, 230, 224, 4)
    with pytest.raises(ValueError, match="230"):
        grown.homo_decrypt(k2048)
