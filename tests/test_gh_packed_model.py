"""Packed gradient pairs on the host: the numpy codec (pack_gh / unpack_gh) against Python integers, and
the plaintext flow model -- sums and differences of packed plaintexts mod n decode to exactly the codes
the two-ciphertext flow (64-bit plaintexts, exponent 2^64 - 1 for a subtraction) decrypts, while
packed_bits_after bounds every plaintext.  GHPairs refuses, before any device call, to decrypt plaintexts
that outgrew the key."""
import numpy as np
import pytest

from conftest import golden_key, load_golden
from gh_packed_cases import (EDGE_CODES, I64_MAX, I64_MIN, W, code, codec_floats, float_pairs, int_of, pack_int,
                             unpack_int, wrap64)


def test_pack_unpack_codes_vs_integers():
    from fedtree_amd.paillier import decode_fixed, pack_codes, unpack_codes, unpack_gh
    rng = np.random.default_rng(11)
    pairs = [(a, b) for a in EDGE_CODES for b in EDGE_CODES]
    pairs += [(int(a), int(b)) for a, b in rng.integers(I64_MIN, I64_MAX, (200, 2), dtype=np.int64, endpoint=True)]
    cg = np.array([a for a, _ in pairs], dtype=np.int64)
    ch = np.array([b for _, b in pairs], dtype=np.int64)
    w = pack_codes(cg, ch)
    assert w.shape == (len(pairs), 6) and w.dtype == np.uint32
    assert [int_of(r) for r in w] == [pack_int(a, b) for a, b in pairs]
    assert [unpack_int(int_of(r)) for r in w] == pairs
    ug, uh = unpack_codes(w)
    assert np.array_equal(ug, cg) and np.array_equal(uh, ch)
    # rows wider than six words (a decrypted plaintext of n_words words): only the low six count
    wide = np.concatenate([w, rng.integers(0, 2**32, (len(w), 10), dtype=np.uint64).astype(np.uint32)], axis=1)
    g, h, ug, uh = unpack_gh(wide, codes=True)
    assert np.array_equal(ug, cg) and np.array_equal(uh, ch)
    assert g.tobytes() == decode_fixed(cg.view(np.uint64)).tobytes()
    assert h.tobytes() == decode_fixed(ch.view(np.uint64)).tobytes()


def test_pack_gh_floats_vs_integers():
    from fedtree_amd.paillier import decode_fixed, encode_fixed, pack_gh, unpack_gh
    g, h = float_pairs()
    assert len(g) >= 2 * len(codec_floats()) + 8
    w = pack_gh(g, h)
    want = [(code(a), code(b)) for a, b in zip(g, h)]
    assert code(np.float32(1e-16)) == 0 and (code(np.float32(1.5e-6)), code(np.float32(-1.5e-6))) == (1, -1)
    assert {(a < 0, b < 0) for a, b in want} == {(False, False), (False, True), (True, False), (True, True)}
    assert [int_of(r) for r in w] == [pack_int(a, b) for a, b in want]
    dg, dh, cg, ch = unpack_gh(w, codes=True)
    assert list(zip(cg.tolist(), ch.tolist())) == want
    # the floats GHPair::homo_decrypt would hand back from the two 64-bit plaintexts
    assert dg.tobytes() == decode_fixed(encode_fixed(g)).tobytes()
    assert dh.tobytes() == decode_fixed(encode_fixed(h)).tobytes()


# ---- the flow model: plaintext integers mod n ------------------------------------------------------------
class Pt:
    """A packed plaintext beside the two 64-bit plaintexts of the reference flow, all reduced mod n, with the
    packed_bits_after bound of the packed one."""

    def __init__(self, n, m, mg, mh, bits):
        self.n, self.m, self.mg, self.mh, self.bits = n, m % n, mg % n, mh % n, bits

    @classmethod
    def fresh(cls, n, cg, ch):
        return cls(n, pack_int(cg, ch), cg % 2**64, ch % 2**64, W)

    @classmethod
    def total(cls, n, pairs):
        """The product of k fresh ciphertexts: a segment sum."""
        from fedtree_amd.paillier import packed_bits_after
        ps = [cls.fresh(n, a, b) for a, b in pairs]
        return cls(n, sum(p.m for p in ps), sum(p.mg for p in ps), sum(p.mh for p in ps),
                   packed_bits_after("sum", W, k=len(ps)))

    def __add__(self, o):
        from fedtree_amd.paillier import packed_bits_after
        return Pt(self.n, self.m + o.m, self.mg + o.mg, self.mh + o.mh, packed_bits_after("add", self.bits, o.bits))

    def __sub__(self, o):
        from fedtree_amd.paillier import packed_bits_after
        e64 = 2**64 - 1             # fthe_sub, GHPair::operator-
        return Pt(self.n, self.m + o.m * (2**W - 1), self.mg + o.mg * e64, self.mh + o.mh * e64,
                  packed_bits_after("sub", self.bits, o.bits))

    def check(self, what):
        assert self.bits < self.n.bit_length(), what            # every case here must fit the key
        assert self.m.bit_length() <= self.bits, (what, self.m.bit_length(), self.bits)
        assert unpack_int(self.m) == (wrap64(self.mg), wrap64(self.mh)), what


def _moduli():
    ns = []
    for name, bits in (("ref_gmp_L4096.json", 2048), ("ref_gmp_L2048.json", 1023)):   # L: the bits of n^2
        p, q = golden_key(load_golden(name))
        assert (p * q).bit_length() == bits
        ns.append(p * q)
    return ns


@pytest.mark.parametrize("n", _moduli(), ids=["n2048", "n1023"])
def test_flow_model_matches_two_ciphertext_flow(n):
    rng = np.random.default_rng(n.bit_length())

    def rand_pairs(k):
        return [(int(a), int(b)) for a, b in rng.integers(I64_MIN, I64_MAX, (k, 2), dtype=np.int64, endpoint=True)]

    sums = []
    for k in (1, 2, 3, 1024):
        for rep in range(3):
            t = Pt.total(n, rand_pairs(k))
            t.check(f"sum of {k}")
            sums.append(t)
    worst = Pt.total(n, [(I64_MIN, I64_MAX)] * 1024)
    worst.check("1024 x (-2^63, 2^63 - 1)")
    assert unpack_int(worst.m) == (wrap64(1024 * I64_MIN), wrap64(1024 * I64_MAX))
    sums += [worst, Pt.total(n, [(I64_MAX, I64_MIN)] * 1024), Pt.total(n, [(-1, -1)] * 3)]
    for i, A in enumerate(sums):
        for B in (sums[(i + 1) % len(sums)], sums[(i + 5) % len(sums)], A):
            (A - B).check("A - B")
            ((A - B) - B).check("(A - B) - B")
            (A - (A - B)).check("A - (A - B)")
            ((A - B) + B).check("sub then add")
            ((A - B) + A).check("sub then add")
    # FedTree's deepest flow: father - computed, its prefix over up to 256 bins, sum - last prefix
    A, B = sums[9], sums[10]                                # sums of 1,024 pairs
    sib = A - B
    pre = sib + sib
    for _ in range(7):
        pre = pre + pre                                     # 256 addends
    (sums[11] - pre).check("missing_gh")


def test_bits_rule():
    from fedtree_amd.paillier import packed_bits_after
    assert packed_bits_after("add", 192, 192) == 193
    assert packed_bits_after("sub", 192, 192) == 385
    assert packed_bits_after("sum", 192, k=1) == 192 and packed_bits_after("sum", 192, k=2) == 193
    assert packed_bits_after("sum", 192, k=1024) == 202 and packed_bits_after("sum", 192, k=1025) == 203
    father = packed_bits_after("sum", 192, k=512)
    sib = packed_bits_after("sub", father, father)
    assert sib <= 400                                       # "~385" of the design note, plus the sums
    missing = packed_bits_after("sub", father, packed_bits_after("sum", sib, k=256))
    assert 512 <= missing <= 610                            # fits below p of Paillier-2048, not below a 512-bit n
    with pytest.raises(ValueError):
        packed_bits_after("mul", 1, 1)


class _HostOnlyKey:
    """Stands in for a Paillier key on a host without a device: any engine call is an error."""

    class DeviceTouched(Exception):
        pass

    def __init__(self, n_bits):
        self.modulus = 2**n_bits - 1
        self.p = 2**(n_bits // 2) - 1
        self.n_words = n_bits // 32

    def _rows(self, a, *_, **__):
        return np.zeros_like(a)

    add_batch = sub_bits_batch = _rows

    def decrypt_gh_packed(self, *a, **k):
        raise self.DeviceTouched

    decrypt_u64 = decrypt_u64_shared = sub_batch = decrypt_gh_packed


def _enc(pl, count, pt_bits, packed=True):
    from fedtree_amd.paillier import GHPairs
    gh = GHPairs(np.zeros(count, np.float32), packed=packed)
    gh.g_enc = np.zeros((count, 2 * pl.n_words), np.uint32)
    gh.h_enc = None if packed else gh.g_enc
    gh.encrypted, gh.paillier, gh.pt_bits = True, pl, pt_bits
    return gh


def test_ghpairs_refuses_plaintexts_that_outgrew_the_key():
    pl = _HostOnlyKey(512)
    for bits, short in ((512, False), (595, False), (256, True), (300, True)):
        with pytest.raises(ValueError, match="pt_bits"):
            _enc(pl, 3, bits).homo_decrypt(pl, short=short)
    # the largest bounds that fit pass the check and go on to the engine
    for bits, short in ((511, False), (255, True)):
        with pytest.raises(_HostOnlyKey.DeviceTouched):
            _enc(pl, 3, bits).homo_decrypt(pl, short=short)


def test_ghpairs_tracks_pt_bits_and_rejects_mixed_operands():
    from fedtree_amd.paillier import HEParty
    pl = _HostOnlyKey(512)
    a, b = _enc(pl, 4, 201), _enc(pl, 4, 201)
    s = a + b
    assert s.packed and s.h_enc is None and s.pt_bits == 202
    d = HEParty.sibling_histogram(a, b)
    assert d.packed and d.h_enc is None and d.pt_bits == 394
    assert (d - b).pt_bits == 395 and (a - d).pt_bits == 587
    with pytest.raises(ValueError, match="pt_bits"):
        (a - d).homo_decrypt(pl)
    for op in (lambda x, y: x + y, lambda x, y: x - y):
        with pytest.raises(ValueError, match="packed"):
            op(a, _enc(pl, 4, 0, packed=False))
        with pytest.raises(ValueError, match="packed"):
            op(_enc(pl, 4, 0, packed=False), a)
