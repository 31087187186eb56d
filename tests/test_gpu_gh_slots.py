"""Slot-packed pairs on the device (include/fthe.h FTHE_GH_SLOT_*): several (g, h) bins in one ciphertext.

Every comparison is exact: the codec kernels against the numpy statement of the layout (itself held to Python
integers in test_gh_slots_model.py), the encrypt against the oracle on the packed integers, the compress
against Python's pow, and every decoded float and code against the pair-packed flow on the same pairs."""
import numpy as np
import pytest

import pyoracle
from conftest import GOLDEN_KEYS, golden_key, load_golden
from gh_packed_cases import float_pairs, int_of, padded_float_pairs

pytestmark = pytest.mark.gpu

KEY_512, KEY_1023, KEY_2048 = GOLDEN_KEYS          # ref_gmp_L<bits of n^2>
CHUNK = 393216                                     # lanes of one launch chunk (one per ciphertext at a 512-bit n)


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


def _dev_outputs(count):
    import torch
    g = torch.full((count,), 7.0, dtype=torch.float32, device="cuda")
    gc = torch.full((count,), 7, dtype=torch.int64, device="cuda")
    return g, g.clone(), gc, gc.clone()


def _np(ts):
    return tuple(t.cpu().numpy() for t in ts)


def _rs(rng, pl, rows):
    n = pl.modulus
    return [int.from_bytes(rng.bytes(pl.n_words * 4), "little") % (n - 1) + 1 for _ in range(rows)]


# ---- 1. the codec kernels ------------------------------------------------------------------------------
@pytest.mark.parametrize("slot_bits", [224, 256])
@pytest.mark.parametrize("name", GOLDEN_KEYS)
def test_codec_kernels_vs_numpy(dev, keys, name, slot_bits):
    import torch
    from fedtree_amd.paillier import gh_slot_count, gh_slot_rows, pack_gh, pack_gh_slots, unpack_gh_slots
    pl = keys[name][0]
    slots = pl.gh_slots(slot_bits)
    assert slots == gh_slot_count(pl.modulus.bit_length(), slot_bits) >= 1
    assert pl.gh_slots(slot_bits, short=True) == gh_slot_count(pl.p.bit_length(), slot_bits)
    sw = slot_bits // 32
    rng = np.random.default_rng(slot_bits)
    for count in sorted({0, 1, slots - 1, slots, slots + 1, 3 * slots + 1, 1000}):
        g, h = padded_float_pairs(1000)
        g, h = g[:count], h[:count]
        rows = gh_slot_rows(count, slots)
        want = pack_gh_slots(pack_gh(g, h), slot_bits, slots)
        m = torch.full((max(rows, 1), slots * sw), -1, dtype=torch.int32, device="cuda")    # stale words everywhere
        pl.pack_gh_slots_dev(_t(g), _t(h), m, slot_bits, slots)
        dev.sync()
        assert _same(m.cpu().numpy().view(np.uint32)[:rows], want), count
        if not count:
            assert (m.cpu().numpy() == -1).all()                    # nothing to write
            continue
        # unpack: the fresh layout, and arbitrary slot contents (sums, residues; pad words not zero), in rows of
        # the layout's width and wider ones whose upper words are not zero either
        anyw = rng.integers(0, 2**32, want.shape, dtype=np.uint64).astype(np.uint32)
        for words in (want, anyw):
            for stride in (slots * sw, pl.n_words + 3):
                wide = rng.integers(0, 2**32, (rows, stride), dtype=np.uint64).astype(np.uint32)
                wide[:, :slots * sw] = words
                outs = _dev_outputs(count)
                pl.unpack_gh_slots_dev(_t(wide.view(np.int32)), count, slot_bits, slots, *outs, stride_words=stride)
                dev.sync()
                wg, wh, wcg, wch = unpack_gh_slots(words, count, slot_bits, slots, codes=True)
                dg, dh, cg, ch = _np(outs)
                assert _same(dg, wg) and _same(dh, wh) and _same(cg, wcg) and _same(ch, wch), (count, stride)
        only_h = torch.zeros(count, dtype=torch.float32, device="cuda")      # nullable outputs
        pl.unpack_gh_slots_dev(_t(want.view(np.int32)), count, slot_bits, slots, h=only_h)
        dev.sync()
        assert _same(only_h.cpu().numpy(), unpack_gh_slots(want, count, slot_bits, slots)[1])


# ---- 2. encrypt against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_KEYS)
def test_encrypt_vs_oracle(dev, keys, name):
    import torch
    from fedtree_amd.paillier import gh_slot_rows, pack_gh, pack_gh_slots
    pl, key = keys[name]
    slot_bits = 224
    slots = pl.gh_slots(slot_bits)
    count = 3 * slots + 1
    g, h = float_pairs()
    g, h = np.concatenate([g[-11:], g])[:count], np.concatenate([h[-11:], h])[:count]   # signs, +-1, next to +-2^63
    rows = gh_slot_rows(count, slots)
    assert rows == 4
    rs = _rs(np.random.default_rng(len(name)), pl, rows)
    ms = [int_of(w) for w in pack_gh_slots(pack_gh(g, h), slot_bits, slots)]
    assert 2**slot_bits <= max(ms) < pl.modulus                     # more than one slot is in use
    want = [pyoracle.encrypt(key, m, r) for m, r in zip(ms, rs)]
    assert pl.lib.fthe_kernel_limbs(2 * pl.keyLength)               # the public form exists at every golden key
    for public in (False, True):
        c = pl.encrypt_gh_slots(g, h, slot_bits, r=rs, public=public)
        assert c.shape == (rows, 2 * pl.n_words)
        assert pyoracle.words_to_ints(c) == want, f"public={public}"
        rw = _t(np.stack([np.frombuffer(r.to_bytes(pl.n_words * 4, "little"), np.uint32) for r in rs]).view(np.int32))
        out = torch.zeros((rows, 2 * pl.n_words), dtype=torch.int32, device="cuda")
        pl.encrypt_gh_slots_dev(_t(g), _t(h), out, slot_bits, r=rw, public=public)
        dev.sync()
        assert _same(out.cpu().numpy().view(np.uint32), c), f"public={public}"
    # a public-only key gives the same rows, and the plaintexts are the layout's integers
    assert pyoracle.words_to_ints(pl.public().encrypt_gh_slots(g, h, slot_bits, r=rs)) == want
    _, full = pl.decrypt_u64(pl.encrypt_gh_slots(g, h, slot_bits, seed=77), full=True)
    assert [int_of(w) for w in full] == ms


# ---- 3. round trip against the pair-packed flow --------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_KEYS)
def test_round_trip_equals_pair_packed_flow(dev, keys, name):
    from fedtree_amd import _lib
    from fedtree_amd.paillier import gh_slot_rows
    pl, _ = keys[name]
    cnt = 273                                           # 256 + 17
    g, h = padded_float_pairs(cnt)
    want = pl.decrypt_gh_packed(pl.encrypt_gh_packed(g, h, seed=5), codes=True)
    for slot_bits in (224, 256):
        for short in (False, True):
            # the layout is built for the decrypt it will meet: the short one holds fewer slots
            slots = pl.gh_slots(slot_bits, short=short)
            assert slots <= pl.gh_slots(slot_bits)
            if not slots:                               # a 256-bit p has no room for a 256-bit slot
                assert name == KEY_512 and short and slot_bits == 256
                with pytest.raises(_lib.FtheError) as e:
                    pl.decrypt_gh_slots(c, cnt, slot_bits, short=True)
                assert e.value.status == _lib.FTHE_ERR_ARG
                continue
            c = pl.encrypt_gh_slots(g, h, slot_bits, seed=6, slots=slots if short else 0)
            assert len(c) == gh_slot_rows(cnt, slots)
            got = pl.decrypt_gh_slots(c, cnt, slot_bits, short=short, codes=True, slots=slots if short else 0)
            assert all(_same(a, b) for a, b in zip(got, want)), (slot_bits, short)
            assert all(_same(a, b) for a, b in zip(pl.decrypt_gh_slots(c, cnt, slot_bits, short=short, slots=slots),
                                                   want[:2])), (slot_bits, short)
            outs = _dev_outputs(cnt)
            pl.decrypt_gh_slots_dev(_t(c.view(np.int32)), cnt, slot_bits, *outs, short=short, slots=slots)
            dev.sync()
            assert all(_same(a, b) for a, b in zip(_np(outs), want)), (slot_bits, short)
    import torch
    th = torch.zeros(cnt, dtype=torch.float32, device="cuda")        # nullable outputs on the device form
    pl.decrypt_gh_slots_dev(_t(pl.encrypt_gh_slots(g, h, 224, seed=7).view(np.int32)), cnt, 224, h=th)
    dev.sync()
    assert _same(th.cpu().numpy(), want[1])


def test_ghpairs_slotted_flow(dev, keys):
    """GHPairs / HEParty on a slot-packed histogram: encrypt, party sums, wire, decrypt."""
    from fedtree_amd.paillier import GHPairs, HEParty, HEServer, gh_slot_rows, wire_decode, wire_encode
    pl, _ = keys[KEY_2048]
    server = HEServer(dev)
    server.paillier = pl
    party = HEParty(pl.public())
    g, h = padded_float_pairs(100)
    enc = [party.encrypt_histogram(GHPairs(g * (k + 1), h, packed=True), seed=k + 1, slot_bits=224) for k in range(2)]
    assert enc[0].slot_bits == 224 and enc[0].slots == 9 and len(enc[0]) == 100 and len(enc[0].g_enc) == 12
    total = enc[0] + enc[1]
    assert (total.pt_bits, total.slot_bits, len(total.g_enc)) == (193, 224, gh_slot_rows(100, 9))
    frame = wire_encode(total.g_enc)
    back, none = wire_decode(frame, 2 * pl.n_words)
    assert none is None and _same(back, total.g_enc)
    ref = [GHPairs(g * (k + 1), h, packed=True).homo_encrypt(pl, seed=k + 1) for k in range(2)]
    want = server.decrypt_gh_pairs(ref[0] + ref[1])
    got = server.decrypt_gh_pairs(total)
    assert not got.encrypted and _same(got.g, want.g) and _same(got.h, want.h)
    with pytest.raises(ValueError, match="not defined on slot-packed"):
        enc[0] - enc[1]
    # compress() of a pair-packed batch is the same batch, slot-packed
    comp = ref[0].compress()
    assert (comp.slot_bits, comp.slots, comp.pt_bits, len(comp), len(comp.g_enc)) == (224, 9, 192, 100, 12)
    one = GHPairs(g, h, packed=True).homo_encrypt(pl, seed=1).homo_decrypt(pl)
    comp.homo_decrypt(pl)
    assert _same(comp.g, one.g) and _same(comp.h, one.h)


# ---- 4. the k-party merge ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [KEY_512, KEY_2048])
def test_merge_of_eight_parties(dev, keys, name):
    pl, _ = keys[name]
    pub = pl.public()
    parties, cnt, slot_bits = 8, 100, 224
    g0, h0 = padded_float_pairs(cnt)
    hists = [(np.roll(g0, k) * np.float32(k + 1), np.roll(h0, 3 * k)) for k in range(parties)]
    packed = np.concatenate([pub.encrypt_gh_packed(g, h, seed=10 + k) for k, (g, h) in enumerate(hists)])
    want = pl.decrypt_gh_packed(pl.reduce_kway(packed.reshape(parties, cnt, -1)), codes=True)
    slotted = np.stack([pub.encrypt_gh_slots(g, h, slot_bits, seed=20 + k) for k, (g, h) in enumerate(hists)])
    assert slotted.shape[1] * pl.gh_slots(slot_bits) >= cnt > (slotted.shape[1] - 1) * pl.gh_slots(slot_bits)
    merged = pub.reduce_kway(slotted)
    assert merged.shape == slotted.shape[1:]
    got = pl.decrypt_gh_slots(merged, cnt, slot_bits, codes=True)
    assert all(_same(a, b) for a, b in zip(got, want))
    assert want[2].any() and want[3].any()


# ---- 5. compress ---------------------------------------------------------------------------------------
def _compress_inputs(pl, count, grown):
    """count pair-packed ciphertexts: fresh ones, or (grown) segment sums minus fresh ones (~385-bit plaintexts)."""
    g, h = padded_float_pairs(3 * count + 140)
    if not grown:
        return pl.encrypt_gh_packed(g[-count:], h[-count:], seed=31)
    c = pl.encrypt_gh_packed(g, h, seed=32)
    seg = np.arange(0, 2 * count + 1, 2, dtype=np.int64)            # sums of two
    seg[-1] += 5                                                    # and one of seven
    sums = pl.reduce_segments(c, seg)
    return pl.sub_bits_batch(sums, c[-count:])


@pytest.mark.parametrize("name,slot_bits", [(KEY_2048, 224), (KEY_2048, 416), (KEY_512, 224), (KEY_512, 416),
                                            (KEY_1023, 224)])
def test_compress_vs_pow(dev, keys, name, slot_bits):
    import torch
    from fedtree_amd.paillier import gh_slot_rows
    pl, _ = keys[name]
    n2 = pl.n2
    slots = pl.gh_slots(slot_bits)
    if name == KEY_512:
        assert slots == (2 if slot_bits == 224 else 1)
    count = 3 * slots + 1
    rows = gh_slot_rows(count, slots)
    x = _compress_inputs(pl, count, grown=slot_bits == 416)
    xi = pyoracle.words_to_ints(x)
    want = []
    for i in range(rows):
        v = 1
        for j in range(slots):
            if j * rows + i < count:
                v = v * pow(xi[j * rows + i], 2**(j * slot_bits), n2) % n2
        want.append(v)
    out = pl.compress_gh_slots(x, slot_bits)
    assert out.shape == (rows, 2 * pl.n_words)
    assert pyoracle.words_to_ints(out) == want
    assert _same(pl.public().compress_gh_slots(x, slot_bits), out)             # a party's job: no private key
    xd = _t(x.view(np.int32))
    od = torch.zeros((rows, 2 * pl.n_words), dtype=torch.int32, device="cuda")
    pl.compress_gh_slots_dev(xd, count, slot_bits, od)
    dev.sync()
    assert _same(od.cpu().numpy().view(np.uint32), out)
    assert _same(xd.cpu().numpy().view(np.uint32), x)                           # the inputs are left alone
    wantd = pl.decrypt_gh_packed(x, codes=True)
    got = pl.decrypt_gh_slots(out, count, slot_bits, codes=True)
    assert all(_same(a, b) for a, b in zip(got, wantd))
    if slots > 2:                                       # fewer slots than the key's maximum, by the trailing argument
        few = pl.compress_gh_slots(x, slot_bits, slots=2)
        assert len(few) == gh_slot_rows(count, 2)
        assert all(_same(a, b) for a, b in zip(pl.decrypt_gh_slots(few, count, slot_bits, codes=True, slots=2), wantd))


# ---- 6. a decrypt of more than one launch chunk --------------------------------------------------------
def test_decrypt_across_a_chunk_boundary(dev, keys):
    """Rows CHUNK .. CHUNK + 4 of the batch are decoded in a second chunk: with the plane order their bins are
    CHUNK .. and rows + CHUNK .., which only the chunk's row offset and the whole call's rows give."""
    from fedtree_amd.paillier import decode_fixed, encode_fixed
    pl, _ = keys[KEY_512]
    slot_bits, slots = 224, 2
    assert pl.gh_slots(slot_bits) == slots
    rows = CHUNK + 5
    count = 2 * rows - 1                                # the last slot of the last row is empty
    rng = np.random.default_rng(6)
    g = rng.normal(0, 1, count).astype(np.float32)
    h = rng.uniform(1e-16, 0.25, count).astype(np.float32)
    c = pl.encrypt_gh_slots(g, h, slot_bits, seed=9)
    assert c.shape == (rows, 2 * pl.n_words)
    outs = _dev_outputs(count)
    pl.decrypt_gh_slots_dev(_t(c.view(np.int32)), count, slot_bits, *outs)
    dev.sync()
    dg, dh, cg, ch = _np(outs)
    wcg, wch = encode_fixed(g), encode_fixed(h)
    wg, wh = decode_fixed(wcg), decode_fixed(wch)
    edge = [0, 1, CHUNK - 1, CHUNK, CHUNK + 4, rows - 1, rows, rows + CHUNK - 1, rows + CHUNK, count - 1]
    for b in edge:                                      # first, last and the bins either side of the boundary
        assert (cg[b], ch[b]) == (wcg.view(np.int64)[b], wch.view(np.int64)[b]), b
        assert (dg[b].tobytes(), dh[b].tobytes()) == (wg[b].tobytes(), wh[b].tobytes()), b
    assert _same(cg, wcg.view(np.int64)) and _same(ch, wch.view(np.int64))
    assert _same(dg, wg) and _same(dh, wh)


# ---- 7. arguments --------------------------------------------------------------------------------------
def test_arguments(dev, keys):
    import torch
    from fedtree_amd import _lib
    from fedtree_amd.paillier import _ptr
    pl, _ = keys[KEY_512]
    lib, ctx, key = pl.lib, dev.ctx, pl._key
    ARG = _lib.FTHE_ERR_ARG
    g = np.array([0.5, -0.25, 1.0], np.float32)
    c = pl.encrypt_gh_slots(g, g, 224, seed=1)
    x = pl.encrypt_gh_packed(g, g, seed=1)
    out = np.zeros_like(x)
    f3, i3 = np.zeros(3, np.float32), np.zeros(3, np.int64)
    m = torch.zeros((2, 32), dtype=torch.int32, device="cuda")
    gd = _t(g)
    p = lambda t: t.data_ptr()

    def codec(sb, slots=2):
        return [lib.fthe_pack_gh_slots_dev(ctx, p(gd), p(gd), 3, sb, slots, p(m)),
                lib.fthe_unpack_gh_slots_dev(ctx, p(m), 32, 3, sb, slots, p(gd), None, None, None)]

    def calls(sb, slots=0, k=key):
        return [lib.fthe_encrypt_gh_slots(k, ctx, _ptr(g), _ptr(g), 3, sb, None, 0, 1, _ptr(out), 0, slots),
                lib.fthe_encrypt_gh_slots_dev(k, ctx, p(gd), p(gd), 3, sb, None, 0, 1, p(m), 0, slots),
                lib.fthe_decrypt_gh_slots(k, ctx, _ptr(c), 3, sb, _ptr(f3), _ptr(f3), _ptr(i3), _ptr(i3), 0, slots),
                lib.fthe_decrypt_gh_slots_dev(k, ctx, p(m), 3, sb, p(gd), None, None, None, 0, slots),
                lib.fthe_compress_gh_slots(k, ctx, _ptr(x), 3, sb, _ptr(out), slots),
                lib.fthe_compress_gh_slots_dev(k, ctx, p(m), 3, sb, p(m), slots)]

    for sb in (192, 200, 230, 0, -224):
        assert codec(sb) + calls(sb) == [ARG] * 8, sb
        assert lib.fthe_gh_slots(key, sb, 0) == 0
    # a slot width that leaves the key no slot (n has 512 bits), and more slots than it has
    assert lib.fthe_gh_slots(key, 512, 0) == 0 and lib.fthe_gh_slots(key, 224, 0) == 2
    assert lib.fthe_gh_slots(key, 224, 1) == 1 and lib.fthe_gh_slots(key, 256, 1) == 0
    assert calls(512) == [ARG] * 6
    assert calls(224, slots=3) == [ARG] * 6
    assert codec(224, slots=-1) + calls(224, slots=-1) == [ARG] * 8
    assert lib.fthe_decrypt_gh_slots(key, ctx, _ptr(c), 3, 224, _ptr(f3), None, None, None, 1, 2) == ARG   # short: one slot
    assert lib.fthe_decrypt_gh_slots(key, ctx, _ptr(c), 3, 256, _ptr(f3), None, None, None, 1, 0) == ARG   # short: none
    assert lib.fthe_unpack_gh_slots_dev(ctx, p(m), 13, 3, 224, 2, p(gd), None, None, None) == ARG          # stride < 14
    assert lib.fthe_pack_gh_slots_dev(ctx, p(gd), p(gd), 3, 224, 0, p(m)) == ARG
    # a public key cannot decrypt (and has no short slot count)
    pub = pl.public()
    assert lib.fthe_gh_slots(pub._key, 224, 0) == 2 and lib.fthe_gh_slots(pub._key, 224, 1) == 0
    for short in (0, 1):
        assert lib.fthe_decrypt_gh_slots(pub._key, ctx, _ptr(c), 3, 224, _ptr(f3), None, None, None, short, 0) \
            == _lib.FTHE_ERR_NOPRIV
        assert lib.fthe_decrypt_gh_slots_dev(pub._key, ctx, p(m), 3, 224, p(gd), None, None, None, short, 0) \
            == _lib.FTHE_ERR_NOPRIV
    with pytest.raises(_lib.FtheError) as e:
        pub.decrypt_gh_slots(c, 3, 224)
    assert e.value.status == _lib.FTHE_ERR_NOPRIV
    # null pointers with a nonzero count; null key / context
    assert lib.fthe_pack_gh_slots_dev(ctx, None, p(gd), 3, 224, 2, p(m)) == ARG
    assert lib.fthe_pack_gh_slots_dev(ctx, p(gd), p(gd), 3, 224, 2, None) == ARG
    assert lib.fthe_pack_gh_slots_dev(None, p(gd), p(gd), 3, 224, 2, p(m)) == ARG
    assert lib.fthe_unpack_gh_slots_dev(ctx, None, 14, 3, 224, 2, p(gd), None, None, None) == ARG
    assert lib.fthe_encrypt_gh_slots(key, ctx, None, _ptr(g), 3, 224, None, 0, 1, _ptr(out), 0, 0) == ARG
    assert lib.fthe_encrypt_gh_slots(key, ctx, _ptr(g), _ptr(g), 3, 224, None, 0, 1, None, 0, 0) == ARG
    assert lib.fthe_encrypt_gh_slots_dev(key, ctx, p(gd), None, 3, 224, None, 0, 1, p(m), 0, 0) == ARG
    assert lib.fthe_decrypt_gh_slots(key, ctx, None, 3, 224, _ptr(f3), None, None, None, 0, 0) == ARG
    assert lib.fthe_decrypt_gh_slots_dev(key, ctx, None, 3, 224, p(gd), None, None, None, 0, 0) == ARG
    assert lib.fthe_compress_gh_slots(key, ctx, None, 3, 224, _ptr(out), 0) == ARG
    assert lib.fthe_compress_gh_slots(key, ctx, _ptr(x), 3, 224, None, 0) == ARG
    assert lib.fthe_compress_gh_slots_dev(key, ctx, None, 3, 224, p(m), 0) == ARG
    assert lib.fthe_compress_gh_slots_dev(None, ctx, p(m), 3, 224, p(m), 0) == ARG
    assert lib.fthe_decrypt_gh_slots(None, ctx, _ptr(c), 3, 224, _ptr(f3), None, None, None, 0, 0) == ARG
    assert lib.fthe_gh_slots(None, 224, 0) == 0
    dev.sync()
    assert not m.cpu().numpy().any() and not out.any()              # the rejected calls wrote nothing
    # count 0 is fine, pointers or not
    assert lib.fthe_pack_gh_slots_dev(ctx, None, None, 0, 224, 2, None) == 0
    assert lib.fthe_encrypt_gh_slots(key, ctx, None, None, 0, 224, None, 0, 1, None, 0, 0) == 0
    assert lib.fthe_decrypt_gh_slots(key, ctx, None, 0, 224, None, None, None, None, 0, 0) == 0
    assert lib.fthe_compress_gh_slots(key, ctx, None, 0, 224, None, 0) == 0
    with pytest.raises(_lib.FtheError) as e:                        # and through the Python methods
        pl.encrypt_gh_slots(g, g, 230, seed=1)
    assert e.value.status == ARG
