"""Packed gradient pairs on the device (include/fthe.h FTHE_GH_*): one ciphertext per (g, h).

Every comparison is exact: the codec kernels against the numpy mirror (itself held to Python integers in
test_gh_packed_model.py), the packed encrypt against the encrypt of general plaintexts and the oracle,
fthe_sub_bits against Python's pow, and every decoded float and code of the packed flow against the
two-ciphertext flow (encrypt_u64 + decrypt_u64 + decode_fixed) on the same gradients."""
import os

import numpy as np
import pytest

import pyoracle
from conftest import GOLDEN_KEYS, golden_key, load_golden
from gh_packed_cases import I64_MAX, I64_MIN, float_pairs, int_of, pack_int, padded_float_pairs, wrap64

pytestmark = pytest.mark.gpu

KEY_512, KEY_1023, KEY_2048 = GOLDEN_KEYS          # ref_gmp_L<bits of n^2>
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "credit_bins.npz")


@pytest.fixture(scope="module")
def dev():
    from fedtree_amd.paillier import Device
    return Device(0)


@pytest.fixture(scope="module")
def keys(dev):
    from fedtree_amd.paillier import Paillier
    out = {}
    for name in GOLDEN_KEYS:
        p, q = golden_key(load_golden(name))
        out[name] = (Paillier.from_primes(p, q, dev), pyoracle.keygen_from_primes(p, q))
    return out


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. the codec kernels ------------------------------------------------------------------------------
def test_pack_unpack_kernels_vs_numpy(dev, keys):
    import torch
    from fedtree_amd.paillier import pack_gh, unpack_gh
    pl = keys[KEY_2048][0]
    g, h = padded_float_pairs(257)                      # one full 256-thread block plus one
    m = torch.zeros((257, 6), dtype=torch.int32, device="cuda")
    pl.pack_gh_dev(_t(g), _t(h), m)
    dev.sync()
    want = pack_gh(g, h)
    assert _same(m.cpu().numpy().view(np.uint32), want)
    # unpack: fresh plaintexts, and arbitrary 192-bit values (sums and differences), rows 6 and n_words apart
    rng = np.random.default_rng(3)
    anyw = rng.integers(0, 2**32, (257, 6), dtype=np.uint64).astype(np.uint32)
    for words in (want, anyw):
        for stride in (6, pl.n_words):
            rows = rng.integers(0, 2**32, (257, stride), dtype=np.uint64).astype(np.uint32)
            rows[:, :6] = words
            dg = torch.zeros(257, dtype=torch.float32, device="cuda")
            dh = torch.zeros_like(dg)
            cg = torch.zeros(257, dtype=torch.int64, device="cuda")
            ch = torch.zeros_like(cg)
            pl.unpack_gh_dev(_t(rows.view(np.int32)), 257, dg, dh, cg, ch, stride_words=stride)
            dev.sync()
            wg, wh, wcg, wch = unpack_gh(words, codes=True)
            assert _same(dg.cpu().numpy(), wg) and _same(dh.cpu().numpy(), wh), stride
            assert _same(cg.cpu().numpy(), wcg) and _same(ch.cpu().numpy(), wch), stride
    # nullable outputs; a stride below six words is an argument error
    only_h = torch.zeros(257, dtype=torch.float32, device="cuda")
    pl.unpack_gh_dev(_t(want.view(np.int32)), 257, h=only_h)
    dev.sync()
    assert _same(only_h.cpu().numpy(), unpack_gh(want)[1])
    from fedtree_amd import _lib
    with pytest.raises(_lib.FtheError) as e:
        pl.unpack_gh_dev(_t(want.view(np.int32)), 257, h=only_h, stride_words=5)
    assert e.value.status == _lib.FTHE_ERR_ARG


# ---- 2. encrypt --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_KEYS)
def test_encrypt_vs_encrypt_words_and_oracle(dev, keys, name):
    import torch
    from fedtree_amd.paillier import pack_gh
    pl, key = keys[name]
    n = pl.modulus
    g, h = float_pairs()
    g, h = np.concatenate([g[-11:], g[:6]]), np.concatenate([h[-11:], h[:6]])   # signs, +-1, next to +-2^63, codec.json
    assert len(g) == 17
    rng = np.random.default_rng(len(name))
    rs = [int.from_bytes(rng.bytes(pl.n_words * 4), "little") % (n - 1) + 1 for _ in g]
    words = pack_gh(g, h)
    ms = [int_of(w) for w in words]
    want = [pyoracle.encrypt(key, m, r) for m, r in zip(ms, rs)]
    forms = [False] + ([True] if pl.lib.fthe_kernel_limbs(2 * pl.keyLength) else [])
    for public in forms:
        c = pl.encrypt_gh_packed(g, h, r=rs, public=public)
        assert _same(c, pl.encrypt_words(words, r=rs, public=public)), f"public={public}"
        assert pyoracle.words_to_ints(c) == want, f"public={public}"
    # device randomness: two contiguous shards through index0 are the one-call batch, host and device forms
    whole = pl.encrypt_gh_packed(g, h, seed=77)
    parts = np.concatenate([pl.encrypt_gh_packed(g[:7], h[:7], seed=77),
                            pl.encrypt_gh_packed(g[7:], h[7:], seed=77, index0=7)])
    assert _same(whole, parts)
    assert not _same(whole, pl.encrypt_gh_packed(g, h, seed=78))
    out = torch.zeros((17, 2 * pl.n_words), dtype=torch.int32, device="cuda")
    pl.encrypt_gh_packed_dev(_t(g[:7]), _t(h[:7]), out[:7], seed=77)
    pl.encrypt_gh_packed_dev(_t(g[7:]), _t(h[7:]), out[7:], seed=77, index0=7)
    dev.sync()
    assert _same(out.cpu().numpy().view(np.uint32), whole)
    _, full = pl.decrypt_u64(whole, full=True)
    assert [int_of(w) for w in full] == ms


# ---- 3. round trip against the two-ciphertext flow -----------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_KEYS)
def test_round_trip_equals_two_ciphertext_flow(dev, keys, name):
    import torch
    from fedtree_amd.paillier import GH_PACKED_BITS, decode_fixed, encode_fixed
    pl, _ = keys[name]
    cnt = 273                                           # 256 + 17
    g, h = padded_float_pairs(cnt)
    low = pl.decrypt_u64(pl.encrypt_u64(np.concatenate([encode_fixed(g), encode_fixed(h)]), seed=6))
    wcg, wch = low[:cnt].view(np.int64), low[cnt:].view(np.int64)
    wg, wh = decode_fixed(low[:cnt]), decode_fixed(low[cnt:])
    c = pl.encrypt_gh_packed(g, h, seed=5)
    assert c.shape == (cnt, 2 * pl.n_words)             # half the ciphertexts of the flow above
    assert GH_PACKED_BITS < pl.p.bit_length()           # a fresh plaintext fits below p at all three keys
    cd = _t(c.view(np.int32))
    for short in (False, True):
        dg, dh, cg, ch = pl.decrypt_gh_packed(c, short=short, codes=True)
        assert _same(dg, wg) and _same(dh, wh), short
        assert _same(cg, wcg) and _same(ch, wch), short
        dg, dh = pl.decrypt_gh_packed(c, short=short)
        assert _same(dg, wg) and _same(dh, wh), short
        tg = torch.zeros(cnt, dtype=torch.float32, device="cuda")
        th = torch.zeros_like(tg)
        tcg = torch.zeros(cnt, dtype=torch.int64, device="cuda")
        tch = torch.zeros_like(tcg)
        pl.decrypt_gh_packed_dev(cd, tg, th, tcg, tch, short=short)
        dev.sync()
        assert _same(tg.cpu().numpy(), wg) and _same(th.cpu().numpy(), wh), short
        assert _same(tcg.cpu().numpy(), wcg) and _same(tch.cpu().numpy(), wch), short
    # nullable outputs on the device form
    th2 = torch.zeros(cnt, dtype=torch.float32, device="cuda")
    pl.decrypt_gh_packed_dev(cd, h=th2)
    dev.sync()
    assert _same(th2.cpu().numpy(), wh)


# ---- 4. fthe_sub_bits ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_KEYS)
def test_sub_bits(dev, keys, name):
    import torch
    from fedtree_amd import _lib
    from fedtree_amd.paillier import _ptr
    pl, _ = keys[name]
    cnt = 273 if name == KEY_2048 else 33
    n2 = pl.n2
    rng = np.random.default_rng(cnt)
    ct = pl.encrypt_u64(rng.integers(0, 2**64, 2 * cnt, dtype=np.uint64), seed=9)
    a, b = ct[:cnt], ct[cnt:]
    ai, bi = pyoracle.words_to_ints(a), pyoracle.words_to_ints(b)
    assert _same(pl.sub_bits_batch(a, b, 64), pl.sub_batch(a, b))
    ad, bd = _t(a.view(np.int32)), _t(b.view(np.int32))
    for bits in (192, 8, 64):
        want = [x * pow(y, 2**bits - 1, n2) % n2 for x, y in zip(ai, bi)]
        assert pyoracle.words_to_ints(pl.sub_bits_batch(a, b, bits)) == want, bits
        out = torch.zeros_like(ad)
        pl.sub_bits_dev(ad, bd, out, bits)
        dev.sync()
        assert pyoracle.words_to_ints(out.cpu().numpy().view(np.uint32)) == want, bits
        for alias in (0, 1):                            # out aliasing a, then b
            x, y = ad.clone(), bd.clone()
            pl.sub_bits_dev(x, y, (x, y)[alias], bits)
            dev.sync()
            assert pyoracle.words_to_ints((x, y)[alias].cpu().numpy().view(np.uint32)) == want, (bits, alias)
            assert _same((y, x)[alias].cpu().numpy(), (bd, ad)[alias].cpu().numpy())     # the other is untouched
    out = np.zeros_like(a)
    for bits in (7, 0, -5, 32 * pl.n_words + 1):
        assert pl.lib.fthe_sub_bits(pl._key, dev.ctx, _ptr(a), _ptr(b), cnt, bits, _ptr(out)) == _lib.FTHE_ERR_ARG
        assert pl.lib.fthe_sub_bits_dev(pl._key, dev.ctx, ad.data_ptr(), bd.data_ptr(), cnt, bits,
                                        ad.data_ptr()) == _lib.FTHE_ERR_ARG
    dev.sync()
    assert _same(ad.cpu().numpy().view(np.uint32), a)   # a rejected call wrote nothing
    # the widest exponent the call takes
    bits = 32 * pl.n_words
    want = [x * pow(y, 2**bits - 1, n2) % n2 for x, y in zip(ai[:3], bi[:3])]
    assert pyoracle.words_to_ints(pl.sub_bits_batch(a[:3], b[:3], bits)) == want


# ---- 5. carries through the fields -----------------------------------------------------------------------
@pytest.mark.parametrize("name", [KEY_512, KEY_2048])
def test_carry_through_the_fields(keys, name):
    from fedtree_amd.paillier import pack_codes
    pl, _ = keys[name]
    words = pack_codes(np.full(1024, I64_MIN, np.int64), np.full(1024, I64_MAX, np.int64))
    assert int_of(words[0]) == pack_int(I64_MIN, I64_MAX)
    c = pl.encrypt_words(words, seed=3)
    seg = np.array([0, 1, 3, 1024, 1024], dtype=np.int64)      # lengths 1, 2, 1,021 and an empty segment
    s = pl.reduce_segments(c, seg)
    for short in (False, True):
        _, _, cg, ch = pl.decrypt_gh_packed(s, short=short, codes=True)
        assert cg.tolist() == [wrap64(k * I64_MIN) for k in (1, 2, 1021)] + [0]
        assert ch.tolist() == [wrap64(k * I64_MAX) for k in (1, 2, 1021)] + [0]
    whole = pl.reduce_segments(c, np.array([0, 1024], dtype=np.int64))
    _, _, cg, ch = pl.decrypt_gh_packed(whole, codes=True)
    assert (int(cg[0]), int(ch[0])) == (wrap64(1024 * I64_MIN), wrap64(1024 * I64_MAX))


# ---- 6. one tree level, packed beside unpacked ---------------------------------------------------------
STAGES = ("father", "child", "sib", "pre", "missing")


def _rows_of(gh, idx):
    """The pairs idx of an encrypted batch, as a batch of their own."""
    from fedtree_amd.paillier import GHPairs
    t = GHPairs(np.zeros(len(idx), np.float32), paillier=gh.paillier, packed=gh.packed)
    t.g_enc = gh.g_enc[idx]
    t.h_enc = None if gh.packed else gh.h_enc[idx]
    t.encrypted, t.pt_bits = True, gh.pt_bits
    return t


def _level(pl, packed):
    """compute_histogram of a node and of its smaller child, the sibling as father - child, its prefix, and a
    missing_gh-style sum - last prefix (hist_tree_builder.cpp:565-595, 640-680, 695-724) on 512 instances.
    Returns the encrypted stages, the ciphertext rows each holds, and the child's empty bins."""
    from fedtree_amd.paillier import GHPairs, HEParty, HEServer, histogram_segments
    d = np.load(FIX)
    n = 512
    y, nb = d["y"][:n], d["nbins_p1"].astype(np.int64)
    bins = d["bins_p1"][:n].copy()
    max_num_bin = 16
    bins[::7, 4] = max_num_bin                          # missing values: feature 4's bins do not sum to the node
    cut = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    server, party = HEServer(pl.dev), HEParty(pl)
    server.paillier = pl
    prob = np.full(n, 0.5, np.float32)
    g = (prob - y.astype(np.float32)).astype(np.float32) * np.linspace(0.5, 1.5, n, dtype=np.float32)
    h = np.maximum(prob * (1 - prob), 1e-16).astype(np.float32)
    enc = server.encrypt_gh_pairs(GHPairs(g, h), seed=4, packed=packed)
    assert enc.packed == packed and (enc.h_enc is None) == packed
    left = bins[:, 0] < 3
    small = np.nonzero(left if left.sum() <= (~left).sum() else ~left)[0]
    father = party.compute_histogram(enc, bins.reshape(-1), cut, max_num_bin)
    child = party.compute_histogram(_rows_of(enc, small), bins[small].reshape(-1), cut, max_num_bin)
    sib = party.sibling_histogram(father, child)
    pre = party.prefix_histogram(sib, cut)
    last = cut[1:] - 1
    node_sum = _rows_of(pre, np.full(len(last), last[0]))       # feature 0 has no missing value: the node's sum
    missing = node_sum - _rows_of(pre, last)
    stages = dict(father=father, child=child, sib=sib, pre=pre, missing=missing)
    nrows = {k: len(v.g_enc) + (0 if v.h_enc is None else len(v.h_enc)) for k, v in stages.items()}
    nrows["enc"] = len(enc.g_enc) + (0 if enc.h_enc is None else len(enc.h_enc))
    empty = np.diff(histogram_segments(bins[small].reshape(-1), cut, max_num_bin)[0]) == 0
    return server, stages, nrows, empty


def _decode(server, gh, short=False):
    t = _rows_of(gh, np.arange(len(gh.g_enc)))
    server.decrypt_gh_pairs(t, short=short)
    assert not t.encrypted
    return t.g, t.h


def test_tree_level_packed_equals_unpacked(keys):
    pl, _ = keys[KEY_2048]
    server, got, rows, empty = _level(pl, True)
    _, want, wrows, wempty = _level(pl, False)
    assert got["missing"].pt_bits < pl.p.bit_length()           # the deepest stage still fits the short decrypt
    assert all(2 * rows[k] == wrows[k] for k in wrows) and len(rows) == 6, (rows, wrows)
    assert empty.any() and np.array_equal(empty, wempty)
    assert np.array_equal(got["child"].bin_encrypted, ~empty)
    for k in STAGES:
        for short in (False, True):
            g, h = _decode(server, got[k], short)
            wg, wh = _decode(server, want[k], short)
            assert _same(g, wg) and _same(h, wh), (k, short)
            if k == "child":
                assert not g[empty].any() and not h[empty].any()        # an empty bin, the ciphertext 1, is (0, 0)
                assert h[~empty].all()
            if k == "missing":                                          # only feature 4 has missing values
                assert not np.delete(g, 4).any() and not np.delete(h, 4).any() and h[4] > 0


def test_tree_level_512_bit_key_refuses_missing_gh(keys):
    pl, _ = keys[KEY_512]
    server, got, _, _ = _level(pl, True)
    _, want, _, _ = _level(pl, False)
    for k in STAGES[:-1]:                               # the shallower stages fit a 512-bit n
        g, h = _decode(server, got[k])
        wg, wh = _decode(server, want[k])
        assert _same(g, wg) and _same(h, wh), k
    assert got["missing"].pt_bits >= pl.modulus.bit_length()
    with pytest.raises(ValueError, match="pt_bits"):    # sum - last prefix does not: an error, not wrong floats
        _decode(server, got["missing"])
    for k in ("sib", "pre"):                            # nor do they fit below p
        with pytest.raises(ValueError, match="pt_bits"):
            _decode(server, got[k], short=True)


# ---- 7. keys too small for a packed plaintext ------------------------------------------------------------
def test_small_key_is_rejected(dev):
    import torch
    from fedtree_amd import _lib
    from fedtree_amd.paillier import Paillier
    n = (2**159 + 2**100 + 12345) | 1                   # a public key of five words
    pl = Paillier.from_public(n, dev)
    assert pl.n_words == 5
    g = np.array([0.5, -0.25], np.float32)
    with pytest.raises(_lib.FtheError) as e:
        pl.encrypt_gh_packed(g, g, seed=1)
    assert e.value.status == _lib.FTHE_ERR_ARG
    out = torch.zeros((2, 10), dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.FtheError) as e:
        pl.encrypt_gh_packed_dev(_t(g), _t(g), out, seed=1)
    assert e.value.status == _lib.FTHE_ERR_ARG
    dev.sync()
    assert not out.cpu().numpy().any()
