"""Negate and subtract by one batched modular inverse on the device (include/fthe.h fthe_invert / fthe_sub_inv;
DESIGN.md 20).

Every comparison is exact: the rows against Python's a * pow(b, -1, n^2) * (1 + offset n) % n^2 at every product
path (the matrix-core add at the 2,048-bit golden key, the four-lane row-I/O programs in their classical and
Montgomery forms at a 2,047-bit edge key and a 2,041-bit key, the slot programs at the 512- and 1,023-bit keys),
and every decoded float and code of GHPairs.sub_inv against `-` and against the two-ciphertext flow."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle
from conftest import GOLDEN_KEYS, golden_key, load_golden
from gh_packed_cases import padded_float_pairs
from n2_edges import load_keys
from sub_inv_cases import SENTINEL, key_2041, non_units, offsets, operands, want_sub_inv

pytestmark = pytest.mark.gpu

KEY_512, KEY_1023, KEY_2048 = GOLDEN_KEYS          # ref_gmp_L<bits of n^2>
ALL_KEYS = GOLDEN_KEYS + ["n2041", "cls_hi"]
COUNTS = (1, 2, 3, 5, 8, 9, 17, 257)               # root only, odd pass-through at several levels, a block plus one
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    from fedtree_amd.paillier import Device
    return Device(0)


@pytest.fixture(scope="module")
def keys(dev):
    """name -> (Paillier, p): made on first use."""
    from fedtree_amd.paillier import Paillier
    made = {}

    def get(name):
        if name not in made:
            if name == "n2041":
                p, q = key_2041()
            elif name in GOLDEN_KEYS:
                p, q = golden_key(load_golden(name))
            else:
                p, q = load_keys()[name]
            made[name] = (Paillier.from_primes(p, q, dev), p)
        return made[name]
    return get


def _t(ints, cw):
    import torch
    return torch.from_numpy(pyoracle.ints_to_words(ints, cw).view(np.int32)).cuda()


def _ints(x):
    return pyoracle.words_to_ints(x.cpu().numpy().view(np.uint32))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. exactness ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_KEYS)
def test_rows_equal_python(dev, keys, name):
    import torch
    pl, _ = keys(name)
    n, n2, cw = pl.modulus, pl.n2, 2 * pl.n_words
    assert n.bit_length() == {KEY_512: 512, KEY_1023: 1023, KEY_2048: 2048, "n2041": 2041, "cls_hi": 2047}[name]
    for count in COUNTS:
        a, b = operands(n, count, count)
        aw, bw = pyoracle.ints_to_words(a, cw), pyoracle.ints_to_words(b, cw)
        ad, bd = _t(a, cw), _t(b, cw)
        # the inverse alone
        winv = [pow(y, -1, n2) for y in b]
        inv = pl.invert_batch(bw)
        got = pyoracle.words_to_ints(inv)
        assert got == winv, count
        assert all(x * y % n2 == 1 for x, y in zip(b, got)), count
        out = torch.zeros_like(bd)
        pl.invert_dev(bd, out)
        dev.sync()
        assert _same(out.cpu().numpy().view(np.uint32), inv), count
        # a - b without an offset, with a one-word offset and with one of n_words words
        for off in offsets(pl.n_words, count):
            want = want_sub_inv(n, a, b, off or 0)
            host = pl.sub_inv_batch(aw, bw, off)
            assert pyoracle.words_to_ints(host) == want, (count, off)
            out = torch.zeros_like(ad)
            pl.sub_inv_dev(ad, bd, out, off)
            dev.sync()
            assert _same(out.cpu().numpy().view(np.uint32), host), (count, off)
        assert _ints(ad) == a and _ints(bd) == b, count     # the inputs are read only
    # products mod n^2 as the call accounts for them, exactly the tree's: for 257 rows (levels of 257, 129, 65,
    # 33, 17, 9, 5 and a top of 3) 254 up, 252 down to level 1, 256 at level 0 = 762 for the inverse, and 257
    # more for a: 2.96 and 3.96 per row.  The unit is what one add of this key accounts for (1 on the matrix-core
    # and classical paths, 2 where a Montgomery product needs its R^2 correction).
    pl.add_dev(ad, bd, out)
    per = dev.last_montmuls() / 257
    assert per in (1, 2) and (per == 1 or name not in (KEY_2048, "cls_hi"))
    pl.invert_dev(bd, out)
    assert dev.last_montmuls() == 762 * per
    pl.sub_inv_dev(ad, bd, out)
    assert dev.last_montmuls() == 1019 * per
    dev.sync()
    # a one-word offset reaches the C ABI as one word, and as n_words words with zeroes above it
    one = np.array([0xDEADBEEF] + [0] * (pl.n_words - 1), np.uint32)
    for words in (1, pl.n_words):
        got = np.zeros_like(aw)
        assert pl.lib.fthe_sub_inv(pl._key, dev.ctx, aw.ctypes.data, bw.ctypes.data, 257, one.ctypes.data, words,
                                   got.ctypes.data) == 0
        assert _same(got, pl.sub_inv_batch(aw, bw, 0xDEADBEEF)), words
    # count == 0 and an offset of too many words
    assert pl.sub_inv_batch(aw[:0], bw[:0]).shape == (0, cw) and pl.invert_batch(bw[:0]).shape == (0, cw)
    with pytest.raises(ValueError):
        pl.sub_inv_batch(aw, bw, 1 << (32 * pl.n_words))
    w = np.ones(pl.n_words + 1, np.uint32)
    from fedtree_amd import _lib
    assert pl.lib.fthe_sub_inv(pl._key, dev.ctx, aw.ctypes.data, bw.ctypes.data, 257, w.ctypes.data, pl.n_words + 1,
                               aw.ctypes.data) == _lib.FTHE_ERR_ARG
    assert pyoracle.words_to_ints(aw) == a


def test_public_key_needs_no_private_key(dev, keys):
    from fedtree_amd.paillier import Paillier
    pl, _ = keys(KEY_2048)
    pub = Paillier.from_public(pl.modulus, dev)
    assert not pub.has_private
    a, b = operands(pl.modulus, 9, 4)
    cw = 2 * pl.n_words
    got = pub.sub_inv_batch(pyoracle.ints_to_words(a, cw), pyoracle.ints_to_words(b, cw), 1 << 192)
    assert pyoracle.words_to_ints(got) == want_sub_inv(pl.modulus, a, b, 1 << 192)


# ---- 2. aliasing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [KEY_512, KEY_2048, "cls_hi"])
def test_out_may_alias_an_input(dev, keys, name):
    pl, _ = keys(name)
    n, cw = pl.modulus, 2 * pl.n_words
    off = offsets(pl.n_words, 1)[2]
    for count in (1, 17, 257):
        a, b = operands(n, count, 50 + count)
        want = want_sub_inv(n, a, b, off)
        for alias in (0, 1):                             # out is a, then out is b
            ad, bd = _t(a, cw), _t(b, cw)
            pl.sub_inv_dev(ad, bd, (ad, bd)[alias], off)
            dev.sync()
            assert _ints((ad, bd)[alias]) == want, (count, alias)
            assert _ints((bd, ad)[alias]) == (b, a)[alias], (count, alias)     # the other is untouched
        xd = _t(b, cw)                                   # out is x
        pl.invert_dev(xd, xd)
        dev.sync()
        assert _ints(xd) == want_sub_inv(n, [1] * count, b), count
        ad = _t(a, cw)                                   # a - a, all three the same rows
        pl.sub_inv_dev(ad, ad, ad)
        dev.sync()
        assert _ints(ad) == [1] * count


# ---- 3. non-units ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [KEY_512, KEY_2048])
def test_a_non_unit_fails_the_batch_and_writes_nothing(dev, keys, name):
    import torch
    from fedtree_amd import _lib
    pl, p = keys(name)
    n, cw = pl.modulus, 2 * pl.n_words
    a, b = operands(n, 17, 9)
    aw = pyoracle.ints_to_words(a, cw)
    good = want_sub_inv(n, a, b, 1 << 192)
    for bad in non_units(n, p, 3):
        for pos in (8, 16):                              # the middle, then the last row
            bb = list(b)
            bb[pos] = bad
            bw = pyoracle.ints_to_words(bb, cw)
            ad, bd = _t(a, cw), _t(bb, cw)
            out = torch.full_like(ad, SENTINEL)
            hout = np.full_like(aw, SENTINEL)
            calls = [lambda: pl.sub_inv_dev(ad, bd, out, 1 << 192), lambda: pl.invert_dev(bd, out),
                     lambda: pl.sub_inv_dev(ad, bd, bd), lambda: pl.invert_dev(bd, bd)]
            for call in calls:
                with pytest.raises(_lib.FtheError) as e:
                    call()
                assert e.value.status == _lib.FTHE_ERR_ARG
            for fn, args in ((pl.lib.fthe_sub_inv, (aw.ctypes.data, bw.ctypes.data, 17, None, 0, hout.ctypes.data)),
                             (pl.lib.fthe_invert, (bw.ctypes.data, 17, hout.ctypes.data)),
                             (pl.lib.fthe_invert, (bw.ctypes.data, 17, bw.ctypes.data))):
                assert fn(pl._key, dev.ctx, *args) == _lib.FTHE_ERR_ARG
            dev.sync()
            assert bool((out == SENTINEL).all()) and bool((hout == SENTINEL).all()), (bad == 0, pos)
            assert _ints(bd) == bb and pyoracle.words_to_ints(bw) == bb and _ints(ad) == a, (bad == 0, pos)
            # the next valid call on the same context succeeds
            pl.sub_inv_dev(ad, _t(b, cw), out, 1 << 192)
            dev.sync()
            assert _ints(out) == good, (bad == 0, pos)


# ---- 4. chunk boundaries -----------------------------------------------------------------------------------
@pytest.mark.parametrize("no_pair", ["", "1"])
def test_chunk_boundaries_in_a_fresh_process(no_pair):
    """FTHE_INV_CHUNK is read once per process: a child with chunks of 8 rows (tests/sub_inv_cases.py), with the
    paired down step of the 2,048-bit key and, FTHE_INV_NO_PAIR=1, with the two adds in its place."""
    env = dict(os.environ, FTHE_INV_CHUNK="8")
    env.pop("FTHE_INV_NO_PAIR", None)
    if no_pair:
        env["FTHE_INV_NO_PAIR"] = no_pair
    r = subprocess.run([sys.executable, os.path.join(HERE, "sub_inv_cases.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "sub_inv chunk child OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_memory_limit_shrinks_the_chunk(dev, keys):
    """fthe_ctx_set_mem_limit on a fresh context: 8,192 rows need 8.4 MB of workspace, a 2 MiB limit admits chunks
    of 2,012 rows (five trees), and the rows are those of the unlimited call; a limit below one row's workspace is
    FTHE_ERR_NOMEM."""
    import torch
    from fedtree_amd import _lib
    from fedtree_amd.paillier import Device, Paillier
    pl, p = keys(KEY_2048)
    n, n2, cw, count = pl.modulus, pl.n2, 2 * pl.n_words, 8192
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 2**32, (2 * count, cw), dtype=np.uint64).astype(np.uint32)
    rows[:, -1] = 0                                      # below 2^4064 < n^2
    ad, bd = (torch.from_numpy(x.view(np.int32)).cuda() for x in (rows[:count], rows[count:]))
    want = torch.zeros_like(ad)
    pl.sub_inv_dev(ad, bd, want, 1 << 192)
    dev.sync()
    sample = [0, 2011, 2012, 4023, 4024, 8191]           # both sides of the limited call's chunk boundaries
    a, b = pyoracle.words_to_ints(rows[sample]), pyoracle.words_to_ints(rows[count:][sample])
    assert _ints(want[sample]) == want_sub_inv(n, a, b, 1 << 192)
    small = Device(0)
    pls = Paillier.from_primes(p, n // p, small)
    small.set_mem_limit(2 << 20)
    out = torch.zeros_like(ad)
    pls.sub_inv_dev(ad, bd, out, 1 << 192)
    small.sync()
    assert torch.equal(out, want)
    assert 4.9 * count <= small.last_montmuls() <= 5.1 * count       # several chunks: the up-sweep runs twice
    small.set_mem_limit(16 << 10)
    with pytest.raises(_lib.FtheError) as e:
        pls.sub_inv_dev(ad, bd, out, 1 << 192)
    assert e.value.status == _lib.FTHE_ERR_NOMEM
    small.sync()
    assert torch.equal(out, want)


# ---- 5. the packed and slot-packed flows -------------------------------------------------------------------
FLOW_COUNT = 96            # every pair of gh_packed_cases.float_pairs (71), padded with random gradients


def _batches(pl, packed):
    """Four encrypted batches a, a2, b, b2 of the same gradients in either mode."""
    from fedtree_amd.paillier import GHPairs
    out = []
    for seed in (5, 6, 7, 8):
        g, h = padded_float_pairs(FLOW_COUNT, seed=seed)
        if seed > 5:                                     # the edge pairs meet other edge pairs
            g, h = np.roll(g, 3 * seed), np.roll(h, 5 * seed)
        out.append(GHPairs(g, h, packed=packed).homo_encrypt(pl, seed=seed))
    return out


def _two_ct_codes(pl, gh):
    low = pl.decrypt_u64(np.concatenate([gh.g_enc, gh.h_enc]))
    return low[:len(gh)].view(np.int64), low[len(gh):].view(np.int64)


def _decoded(pl, gh, short=False):
    """(g, h, g_code, h_code) of an encrypted packed or slot-packed batch."""
    if gh.slot_bits:
        return pl.decrypt_gh_slots(gh.g_enc, len(gh), gh.slot_bits, short=short, codes=True, slots=gh.slots)
    return pl.decrypt_gh_packed(gh.g_enc, short=short, codes=True)


@pytest.mark.parametrize("name", GOLDEN_KEYS)
def test_packed_flow_equals_minus_and_the_two_ciphertext_flow(keys, name):
    from fedtree_amd.paillier import decode_fixed, packed_bits_after
    pl, _ = keys(name)
    a, a2, b, b2 = _batches(pl, True)
    ua, ua2, ub, ub2 = _batches(pl, False)
    d = a.sub_inv(b)
    assert d.packed and d.encrypted and d.pt_bits == packed_bits_after("sub_inv", 192, 192) == 193
    wcg, wch = _two_ct_codes(pl, ua - ub)
    wg, wh = decode_fixed(wcg.view(np.uint64)), decode_fixed(wch.view(np.uint64))
    minus = _decoded(pl, a - b)
    for short in (False, True):
        assert d.pt_bits < pl.p.bit_length()
        got = _decoded(pl, d, short=short)
        for x, y, z in zip(got, (wg, wh, wcg, wch), minus):
            assert _same(x, y) and _same(x, z), short
    dec = a.sub_inv(b).homo_decrypt(pl)                  # the GHPairs route to the same floats
    assert _same(dec.g, wg) and _same(dec.h, wh)
    # chained, on a sum
    c = (a + a2).sub_inv(b).sub_inv(b2)
    assert c.pt_bits == 195
    wcg, wch = _two_ct_codes(pl, ((ua + ua2) - ub) - ub2)
    for short in (False, True):
        got = _decoded(pl, c, short=short)
        assert _same(got[2], wcg) and _same(got[3], wch), short
        assert _same(got[0], decode_fixed(wcg.view(np.uint64))) and _same(got[1], decode_fixed(wch.view(np.uint64)))
    # an unencrypted right-hand side, as `-` handles it
    plain = padded_float_pairs(FLOW_COUNT, seed=11)
    from fedtree_amd.paillier import GHPairs
    e = a.sub_inv(GHPairs(*plain))
    f = a - GHPairs(*plain)
    assert e.pt_bits == f.pt_bits == 193
    assert all(_same(x, y) for x, y in zip(_decoded(pl, e), _decoded(pl, f)))


@pytest.mark.parametrize("name", GOLDEN_KEYS)
def test_slot_packed_batches_subtract(keys, name):
    pl, _ = keys(name)
    a, _, b, b2 = _batches(pl, True)
    want = _decoded(pl, a - b)
    sa, sb = a.compress(224), b.compress(224)
    d = sa.sub_inv(sb)
    assert (d.slot_bits, d.slots, d.pt_bits, len(d)) == (224, sa.slots, 193, FLOW_COUNT)
    assert len(d.g_enc) == -(-FLOW_COUNT // sa.slots)
    assert all(_same(x, y) for x, y in zip(_decoded(pl, d), want))
    # twice: still within the 224-bit slots
    d2 = d.sub_inv(b2.compress(224))
    assert d2.pt_bits == 194
    want2 = _decoded(pl, (a - b) - b2) if name != KEY_512 else None     # 578 bits: `-` cannot at a 512-bit n
    got2 = _decoded(pl, d2)
    if want2 is not None:
        assert all(_same(x, y) for x, y in zip(got2, want2))
    assert all(_same(x, y) for x, y in zip(got2, _decoded(pl, a.sub_inv(b).sub_inv(b2))))
    # subtract first, compress after: the slots a difference needs
    assert a.sub_inv(b).compress().slot_bits == 224
    assert (a - b).compress().slot_bits == 416
    assert all(_same(x, y) for x, y in zip(_decoded(pl, a.sub_inv(b).compress()), want))


def test_refusals(keys):
    pl, _ = keys(KEY_2048)
    a, _, b, _ = _batches(pl, True)
    sa = a.compress(224)
    with pytest.raises(ValueError, match="differ"):
        sa.sub_inv(b.compress(256))
    with pytest.raises(ValueError, match="differ"):
        sa.sub_inv(b.compress(224, slots=8))
    with pytest.raises(ValueError, match="slot-packed"):
        sa.sub_inv(b)
    grown = b.compress(224)
    grown.pt_bits = 224                                  # a bound above slot_bits: refused before any device work
    rows = grown.g_enc.copy()
    with pytest.raises(ValueError, match="225 bits"):
        sa.sub_inv(grown)
    assert _same(grown.g_enc, rows)
    ua, _, ub, _ = _batches(pl, False)
    with pytest.raises(ValueError, match="packed"):
        ua.sub_inv(ub)
    with pytest.raises(ValueError):
        a.sub_inv(ub)
    d = ua - ub                                          # `-` itself is as it was
    assert not d.packed and d.h_enc is not None
