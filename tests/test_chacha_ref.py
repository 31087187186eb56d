"""The reference of the device randomness (tests/chacha_ref.py) against published ChaCha20 vectors, an openssl
binary where there is one, and the sampler's contract on tiny moduli.  No GPU."""
import random
import shutil
import subprocess

import numpy as np
import pytest

import chacha_ref as cr


def _block_bytes(key8, counter, nonce):
    return cr.chacha20_block(key8, counter, nonce).astype("<u4").tobytes()


def test_zero_key_block():
    got = _block_bytes([0] * 8, 0, 0)
    assert got[:32].hex() == "76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7"


def test_rfc8439_block():
    """RFC 8439 2.3.2: key 00..1f, state words 12..15 = 1, 0x09000000, 0x4a000000, 0"""
    key = [int.from_bytes(bytes(range(4 * i, 4 * i + 4)), "little") for i in range(8)]
    got = _block_bytes(key, 1 | 0x09000000 << 32, 0x4A000000)
    assert got.hex() == ("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
                         "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")


def test_blocks_vectorise_over_counters():
    key = list(range(1, 9))
    ctrs = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1]
    many = cr.chacha20_block(key, np.array(ctrs, dtype=np.uint64), 77)
    assert many.shape == (len(ctrs), 16) and many.dtype == np.uint32
    for row, c in zip(many, ctrs):
        assert np.array_equal(row, cr.chacha20_block(key, c, 77))
    assert len({bytes(r) for r in many}) == len(ctrs)            # the high counter word is part of the state


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl binary")
def test_blocks_match_openssl():
    rng = random.Random(8439)
    for _ in range(4):
        key = [rng.getrandbits(32) for _ in range(8)]
        ctr, nonce = rng.getrandbits(64), rng.getrandbits(64)
        kb = b"".join(k.to_bytes(4, "little") for k in key)
        iv = ctr.to_bytes(8, "little") + nonce.to_bytes(8, "little")
        res = subprocess.run(["openssl", "enc", "-chacha20", "-K", kb.hex(), "-iv", iv.hex()],
                             input=bytes(64), capture_output=True)
        if res.returncode != 0:
            pytest.skip("this openssl has no chacha20 cipher")
        assert res.stdout == _block_bytes(key, ctr, nonce)       # the keystream of one block


def test_rng_key_expansion():
    """the splitmix64 outputs of seed 1 are the published 0x910a2dec89025cc1, 0xbeeb8da1658eec67, ..."""
    key, nonce = cr.rng_key(1, 0)
    assert key[0] | key[1] << 32 == 0x910A2DEC89025CC1
    assert key[2] | key[3] << 32 == 0xBEEB8DA1658EEC67
    assert len(key) == 8 and all(0 <= k < 1 << 32 for k in key)
    key2, nonce2 = cr.rng_key(1, cr.TWEAK_EXACT)
    assert key2 == key and nonce2 == nonce ^ cr.TWEAK_EXACT
    assert cr.rng_key(2, 0)[0] != key
    # the state advances by the golden-ratio constant: output i of seed s is output 0 of s + i * gamma
    gamma = 0x9E3779B97F4A7C15
    k3, _ = cr.rng_key((1 + gamma) & cr.M64, 0)
    assert k3[:6] == key[2:]


def _candidate(key, nonce, index, attempt, row_words):
    """one candidate, block by block with the scalar block function"""
    nblk = (row_words + 15) // 16
    words = []
    for b in range(nblk):
        words += [int(w) for w in cr.chacha20_block(key, ((index * 64 + attempt) * nblk + b) & cr.M64, nonce)]
    return sum(w << (32 * i) for i, w in enumerate(words[:row_words]))


# (modulus, nbits, row_words): nbits a multiple of 32; rows one word wider than the modulus needs (top word
# must come out zero); 2^k + 1 (acceptance about 1/2); a row that takes two blocks
EDGES = [((1 << 32) - 5, 32, 1), ((1 << 64) - 59, 64, 2), ((1 << 32) - 5, 32, 2), ((1 << 40) - 87, 40, 3),
         ((1 << 20) + 1, 21, 1), ((1 << 63) + 1, 64, 2), ((1 << 63) + 1, 64, 3), ((1 << 520) + 1, 521, 17),
         ((1 << 520) + 1, 521, 18), (3, 2, 1), (2, 2, 1)]


@pytest.mark.parametrize("modulus,nbits,row_words", EDGES,
                         ids=[f"{m.bit_length()}b-in-{nb}b-{w}w-{i}" for i, (m, nb, w) in enumerate(EDGES)])
def test_draw_below_contract(modulus, nbits, row_words):
    key, nonce = cr.rng_key(99, 0)
    idx = list(range(40)) + [(1 << 32) - 1, 1 << 32, (1 << 40) + 3]
    vals, tries = cr.draw_below_many(key, nonce, idx, modulus, nbits, row_words)
    for i, v, t in zip(idx, vals, tries):
        assert (v, t) == cr.draw_below(key, nonce, i, modulus, nbits, row_words)
        assert 0 < v < modulus and 1 <= t <= 64
        # the draw is the first acceptable candidate, masked to nbits whatever the row width
        seen = [_candidate(key, nonce, i, a, row_words) & ((1 << nbits) - 1) for a in range(t)]
        assert all(not 0 < c < modulus for c in seen[:-1])
        assert seen[-1] == v or (t == 64 and v == 1)
    if modulus == (1 << (nbits - 1)) + 1:                        # about half the candidates rejected
        assert max(tries) >= 3 and sum(t > 1 for t in tries) >= len(idx) // 4
    if modulus > 1 << 31:
        assert len(set(vals)) == len(vals)


def test_wider_row_keeps_the_low_words():
    """rows one word wider than the modulus needs draw the same values while the block count is the same: the
    extra word is cleared, not compared"""
    key, nonce = cr.rng_key(5, 0)
    for modulus, nbits, w in (((1 << 64) - 59, 64, 2), ((1 << 63) + 1, 64, 2), ((1 << 40) - 87, 40, 2)):
        a = cr.draw_below_many(key, nonce, range(64), modulus, nbits, w)
        b = cr.draw_below_many(key, nonce, range(64), modulus, nbits, w + 1)
        assert a == b


def test_fallback_after_64_failures():
    """no candidate can be accepted: the value is 1"""
    key, nonce = cr.rng_key(7, 0)
    assert cr.draw_below(key, nonce, 3, 1, 8, 1) == (1, 64)


def test_streams_do_not_share_counters():
    """attempts, indices and the blocks of a row all take different counters"""
    seen = set()
    for row_words in (17, 33):
        nblk = (row_words + 15) // 16
        ctrs = [(i * 64 + a) * nblk + b for i in range(5) for a in range(64) for b in range(nblk)]
        assert len(set(ctrs)) == len(ctrs)
        seen.update(ctrs)
    key, nonce = cr.rng_key(11, 0)
    yp = cr.draw_below_many(key, nonce, range(32), (1 << 127) - 1, 127, 4)[0]
    yq = cr.draw_below_many(key, nonce ^ cr.YQ_XOR, range(32), (1 << 127) - 1, 127, 4)[0]
    assert not set(yp) & set(yq)


def test_digits_layout():
    key, nonce = cr.rng_key(13, cr.TWEAK_FIXED_BASE)
    for nbytes in (1, 64, 65, 136, 264):
        nb = (nbytes + 63) // 64
        for index, side in ((0, 0), (0, 1), (5, 0), ((1 << 33) + 1, 1)):
            want = b"".join(_block_bytes(key, (index * 2 + side) * nb + b, nonce) for b in range(nb))[:nbytes]
            assert cr.digits(key, nonce, index, side, nbytes) == want
            assert cr.digits_many(key, nonce, [index], side, nbytes) == [int.from_bytes(want, "little")]
    assert cr.digits(key, nonce, 0, 1, 64) == cr.digits(key, nonce, 0, 0, 128)[64:]
