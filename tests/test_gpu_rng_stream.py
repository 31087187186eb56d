"""What the device draws, against the reference sampler of tests/chacha_ref.py (the stream contract of
DESIGN.md 1): every seeded encrypt form with device randomness is rebuilt from the reference's draws and Python
integers alone --

  CRT (key holder)   c = CRT((1 + m n) y_p^p mod p^2, (1 + m n) y_q^q mod q^2)
  public key         c = (1 + m n) r^n mod n^2

-- and compared row for row; neither the fthe_debug_direct_y hook nor the C oracle takes part in an expected
value.  A wrong quarter-round, a counter shared between lanes, attempts, chunks or calls, y_p correlated with
y_q, a wrong key expansion or a sampler that leaves its range all change some row.

Keys of the CRT path: (a) keygen(2048): 1024-bit primes, no top mask; (b) 1030/1030 bits: 33-word rows, a 6-bit
mask; (c) 1009/1030, 1030/1009, 1024/1025: the primes' word counts differ, the smaller one is drawn in rows one
word wider than it needs (before k_rng_r cleared the bits above nbits every such draw fell back to y = 1, and one
ciphertext factored n); (d) keygen(1024) and 505/514 (16 and 17 words: uneven like (c)): one block per candidate,
the K = 19 kernel; (e) p just above 2^1023: half the candidates rejected.  Also: index0 (a shard equals the rows of the whole call; block counters past
2^32), the hook, the public-key path at five sizes, the fixed-base modes against their injected-exponent forms, and
unseeded calls (all draws distinct within and between calls, bits fair).  Integer work: exact equality.
"""
import functools
import math
import random

import numpy as np
import pytest

import chacha_ref as cr

pytestmark = pytest.mark.gpu

SEED = 20261019
CHUNK = 393216                  # chunk_lanes() of the engine (fthe.hip)
ENC_CHUNK = 2 * CHUNK           # the large direct-y batches' launches
PUB_CHUNK = CHUNK // 4          # the four-lane public-key kernel's launches


# ---- helpers -----------------------------------------------------------------------------------------------
def _rows(xs, nw):
    return np.stack([np.frombuffer(int(x).to_bytes(4 * nw, "little"), dtype="<u4") for x in xs]).astype(np.uint32)


def _ints(a):
    a = np.ascontiguousarray(a, dtype="<u4")
    return [int.from_bytes(r.tobytes(), "little") for r in a]


def _same_rows(got, want, idx):
    assert got.shape == want.shape
    bad = np.nonzero(~np.all(got == want, axis=1))[0]
    assert bad.size == 0, (f"{bad.size} of {len(idx)} sampled ciphertexts differ from the reference, "
                           f"first at index {int(idx[bad[0]])}")


def _prime(rng, bits):
    from test_gpu_parity import _next_prime
    while True:
        p = _next_prime(rng.getrandbits(bits) | (1 << (bits - 1)))
        if p.bit_length() == bits:
            return p


@functools.lru_cache(maxsize=None)
def _primes(name):
    """test primes by name: "<bits of p>-<bits of q>", or "half" for key (e)"""
    from test_gpu_parity import _next_prime
    rng = random.Random(sum(name.encode()) * 7919 + len(name))
    if name == "half":
        return _next_prime((1 << 1023) + (1 << 500)), _prime(rng, 1024)
    bp, bq = (int(x) for x in name.split("-"))
    while True:
        p, q = _prime(rng, bp), _prime(rng, bq)
        if p != q:
            return p, q


@pytest.fixture(scope="module")
def keys():
    """keys by name, built once: "gen2048" / "gen1024" from the engine's keygen, else _primes(name)"""
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    made = {}

    def get(name):
        if name not in made:
            if name.startswith("gen"):
                made[name] = Paillier(dev).keygen(int(name[3:]), seed=SEED)
            else:
                made[name] = Paillier.from_primes(*_primes(name), dev)
        return made[name]

    get.dev = dev
    return get


def _pq_words(pl):
    return (max(pl.p.bit_length(), pl.q.bit_length()) + 31) // 32


def _draw_y(pl, seed, gidx):
    """the reference's (y_p, y_q, attempts_p, attempts_q) of ciphertext indices gidx"""
    key, nonce = cr.rng_key(seed, 0)
    pw = _pq_words(pl)
    yp, tp = cr.draw_below_many(key, nonce, gidx, pl.p, pl.p.bit_length(), pw)
    yq, tq = cr.draw_below_many(key, nonce ^ cr.YQ_XOR, gidx, pl.q, pl.q.bit_length(), pw)
    return yp, yq, tp, tq


def _crt(p, q, cp, cq):
    p2, q2 = p * p, q * q
    return cq + q2 * ((cp - cq) * pow(q2, -1, p2) % p2)


def _want_crt(pl, m, seed, gidx):
    """rows of c = CRT((1 + m n) y_p^p mod p^2, (1 + m n) y_q^q mod q^2) for plaintexts m at indices gidx"""
    p, q, n = pl.p, pl.q, pl.modulus
    p2, q2 = p * p, q * q
    yp, yq, _, _ = _draw_y(pl, seed, gidx)
    out = []
    for x, a, b in zip(m, yp, yq):
        g = 1 + int(x) * n
        out.append(_crt(p, q, g * pow(a, p, p2) % p2, g * pow(b, q, q2) % q2))
    return _rows(out, 2 * pl.n_words)


def _want_pub(pl, m, seed, gidx):
    """rows of c = (1 + m n) r^n mod n^2"""
    n = pl.modulus
    n2 = n * n
    key, nonce = cr.rng_key(seed, 0)
    rs, _ = cr.draw_below_many(key, nonce, gidx, n, n.bit_length(), pl.n_words)
    return _rows([(1 + int(x) * n) * pow(r, n, n2) % n2 for x, r in zip(m, rs)], 2 * pl.n_words)


def _messages(cnt, salt):
    m = np.random.default_rng(SEED + salt).integers(0, 2**64 - 1, cnt, dtype=np.uint64, endpoint=True)
    m[:3] = [0, 1, 2**64 - 1]
    return m


def _ends(cnt, k):
    return np.concatenate([np.arange(0, k), np.arange(cnt - k, cnt)])


# ---- the key holder's CRT direct-y path --------------------------------------------------------------------
def test_key_a_is_the_even_word_branch(keys):
    pl = keys("gen2048")
    assert pl.p.bit_length() == 1024 and pl.q.bit_length() == 1024


def test_crt_small_batch_four_lane_path(keys):
    pl = keys("gen2048")
    cnt = 1024
    m = _messages(cnt, 1)
    c = pl.encrypt_u64(m, seed=SEED + 1)
    idx = _ends(cnt, 40)
    _same_rows(c[idx], _want_crt(pl, m[idx], SEED + 1, idx), idx)
    assert np.array_equal(pl.decrypt_u64(c), m)


def test_crt_split_path(keys):
    pl = keys("gen2048")
    cnt = 20000
    m = _messages(cnt, 2)
    c = pl.encrypt_u64(m, seed=SEED + 2)
    idx = np.concatenate([_ends(cnt, 24), np.arange(16384 - 8, 16384 + 8)])
    _same_rows(c[idx], _want_crt(pl, m[idx], SEED + 2, idx), idx)


def test_crt_large_device_resident_batch(keys):
    """one full launch plus 4,096 more (the shape of test_large_batch_across_chunk_boundary): rows around the
    engine's chunk, around the launch boundary and at both ends"""
    import torch
    pl = keys("gen2048")
    cnt = ENC_CHUNK + 4096
    m = _messages(cnt, 3)
    md = torch.from_numpy(m.view(np.int64)).to("cuda:0")
    cd = torch.empty((cnt, 2 * pl.n_words), dtype=torch.int32, device="cuda:0")
    pl.encrypt_u64_dev(md, cd, seed=SEED + 3)
    keys.dev.sync()
    idx = np.concatenate([np.arange(0, 16), np.arange(CHUNK - 12, CHUNK + 12),
                          np.arange(ENC_CHUNK - 12, ENC_CHUNK + 12), np.arange(cnt - 16, cnt)])
    c = cd[torch.from_numpy(idx).to("cuda:0")].cpu().numpy().view(np.uint32)
    _same_rows(c, _want_crt(pl, m[idx], SEED + 3, idx), idx)


@pytest.mark.parametrize("cnt", [1024, 16640])
@pytest.mark.parametrize("name", ["1030-1030", "1009-1030", "1030-1009", "1024-1025", "gen1024", "505-514", "half"])
def test_crt_mask_and_row_width_edges(keys, name, cnt):
    """keys (b)-(e); 16,640 ciphertexts reach the matrix-core kernel at K = 37"""
    pl = keys(name)
    if not name.startswith("gen") and name != "half":
        assert [pl.p.bit_length(), pl.q.bit_length()] == [int(x) for x in name.split("-")]
    seed = SEED + 10 + cnt
    m = _messages(cnt, 4)
    idx = np.concatenate([_ends(cnt, 24), np.arange(cnt // 2, cnt // 2 + 16)])
    if name == "half":
        # p = 2^1023 + 2^500 + ...: a 1024-bit candidate is below p half the time.  The sample takes in the indices
        # that reject most often, and -- from the reference alone -- one of them needs 5 or more candidates and
        # none comes near the 64 of the fallback.
        assert pl.p.bit_length() == 1024 and pl.p >> 501 == 1 << 522
        scan = np.arange(1024)
        key, nonce = cr.rng_key(seed, 0)
        _, tries = cr.draw_below_many(key, nonce, scan, pl.p, 1024, _pq_words(pl))
        worst = scan[np.argsort(np.asarray(tries), kind="stable")[-24:]]
        idx = np.unique(np.concatenate([idx, worst]))
        tp = _draw_y(pl, seed, idx)[2]
        assert max(tp) >= 5 and max(tp) < 64, max(tp)
    c = pl.encrypt_u64(m, seed=seed)
    _same_rows(c[idx], _want_crt(pl, m[idx], seed, idx), idx)
    # a lane on the fallback y = 1 has c = 1 + m n (mod P^2): gcd(c - 1, n) = P, one ciphertext factors n
    assert all(math.gcd(x - 1, pl.modulus) == 1 for x in _ints(c[:512]))


# ---- index0: the shard offset ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [{}, {"public": True}, {"fixed_base_exact": True}], ids=["crt", "public", "exact"])
def test_shard_equals_rows_of_the_whole_call(keys, mode):
    pl = keys("gen2048")
    cnt, lo, hi = 2000, 777, 1500
    m = _messages(cnt, 5)
    if mode.get("fixed_base_exact"):
        pl.set_fixed_base_exact(seed=SEED)
    whole = pl.encrypt_u64(m, seed=SEED + 20, **mode)
    part = pl.encrypt_u64(m[lo:hi], seed=SEED + 20, index0=lo, **mode)
    assert np.array_equal(part, whole[lo:hi])
    assert not np.array_equal(pl.encrypt_u64(m[lo:hi], seed=SEED + 20, **mode), whole[lo:hi])   # index0 = 0 differs


def test_counters_cross_2_pow_32(keys):
    """index0 = 2^32 - 8, 16 rows: the ciphertext index, and with it the block counter's high word, carries
    inside the batch"""
    pl = keys("gen2048")
    i0 = 2**32 - 8
    m = _messages(16, 6)
    gidx = [i0 + i for i in range(16)]
    c = pl.encrypt_u64(m, seed=SEED + 21, index0=i0)
    _same_rows(c, _want_crt(pl, m, SEED + 21, gidx), gidx)
    cp = pl.encrypt_u64(m, seed=SEED + 21, index0=i0, public=True)
    _same_rows(cp, _want_pub(pl, m, SEED + 21, gidx), gidx)


# ---- the hook ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gen2048", "1009-1030", "1030-1009", "1024-1025"])
def test_hook_equals_the_reference(keys, name):
    pl = keys(name)
    pw = _pq_words(pl)
    for i0, cnt in ((0, 300), (123457, 300), (2**32 - 5, 10)):
        gidx = [i0 + i for i in range(cnt)]
        yp, yq = pl.direct_y(SEED + 30, i0, cnt)
        wp, wq, _, _ = _draw_y(pl, SEED + 30, gidx)
        _same_rows(yp, _rows(wp, pw), gidx)
        _same_rows(yq, _rows(wq, pw), gidx)


# ---- the public-key path --------------------------------------------------------------------------------------
def test_public_2048_across_a_launch_boundary(keys):
    pl = keys("gen2048")
    cnt = PUB_CHUNK + 512
    m = _messages(cnt, 7)
    c = pl.encrypt_u64(m, seed=SEED + 40, public=True)
    idx = np.concatenate([np.arange(0, 6), np.arange(PUB_CHUNK - 6, PUB_CHUNK + 6), np.arange(cnt - 6, cnt)])
    _same_rows(c[idx], _want_pub(pl, m[idx], SEED + 40, idx), idx)


@pytest.mark.parametrize("nbits", [2045, 2042, 1024, 512])
def test_public_other_sizes(keys, nbits):
    """n of 2045 and 2042 bits with the primes of test_gpu_nadic.py (the Barrett and the Montgomery n-adic
    kernels, a 29- and a 26-bit top mask); Paillier-1024 and Paillier-512"""
    from fedtree_amd.paillier import Paillier
    from test_gpu_nadic import _key_of_bits
    p, q, n = _key_of_bits(np.random.default_rng(nbits), nbits)
    pl = Paillier.from_public(n, keys.dev)
    assert pl.modulus.bit_length() == nbits
    cnt = 2000
    m = _messages(cnt, 8)
    c = pl.encrypt_u64(m, seed=SEED + 41, public=True)
    idx = _ends(cnt, 8 if nbits > 1024 else 32)
    _same_rows(c[idx], _want_pub(pl, m[idx], SEED + 41, idx), idx)
    assert np.array_equal(Paillier.from_primes(p, q, keys.dev).decrypt_u64(c), m)


# ---- fixed-base modes: the seeded call equals the call with the reference's exponents injected ---------------
def _bump(nonce, k):
    return (nonce + (k << 56)) & cr.M64


@pytest.mark.parametrize("name", ["gen2048", "1009-1030", "1024-1025"])
def test_exact_fixed_base_key_holder(keys, name):
    pl = keys(name)
    cnt = 2000
    m = _messages(cnt, 9)
    pl.set_fixed_base_exact(seed=SEED)
    gam, ew = pl.fixed_base_exact_info()
    nb = len(gam[0])
    assert ew == _pq_words(pl)
    key, nonce = cr.rng_key(SEED + 50, cr.TWEAK_EXACT)
    cols = []
    for side, P in enumerate((pl.p, pl.q)):
        for b in range(nb):
            ys, tries = cr.draw_below_many(key, _bump(nonce, 3 * side + b + 1), range(cnt), P, P.bit_length(), ew)
            assert max(tries) < 64
            cols.append(_rows(ys, ew))
    y = np.ascontiguousarray(np.concatenate(cols, axis=1))
    c = pl.encrypt_u64(m, seed=SEED + 50, fixed_base_exact=True)
    want = pl.encrypt_u64(m, r=y, fixed_base_exact=True)
    _same_rows(c, want, np.arange(cnt))
    assert np.array_equal(pl.decrypt_u64(c), m)


def test_exact_fixed_base_published_bases(keys):
    server = keys("gen2048")
    cnt = 2000
    m = _messages(cnt, 10)
    hs = server.public_bases(seed=7)
    party = server.public(bases=hs)
    nb, ew = party.public_bases_info()
    assert nb == len(hs) and ew == [(bits // 16 + 1) // 2 for bits in hs.exp_bits]
    key, nonce = cr.rng_key(SEED + 51, cr.TWEAK_PUBLIC_EXACT)
    ys = [cr.digits_many(key, _bump(nonce, b + 1), range(cnt), 0, hs.exp_bits[b] // 8) for b in range(nb)]
    c = party.encrypt_u64(m, seed=SEED + 51, fixed_base_exact=True)
    want = party.encrypt_u64(m, r=list(zip(*ys)), fixed_base_exact=True)
    _same_rows(c, want, np.arange(cnt))
    assert np.array_equal(server.decrypt_u64(c), m)


def test_fixed_base_public_and_crt(keys):
    pl = keys("gen2048")
    p, q, n = pl.p, pl.q, pl.modulus
    cnt = 2000
    m = _messages(cnt, 11)
    pl.set_fixed_base(int.from_bytes(np.random.default_rng(SEED).bytes(200), "little") % (n - 2) + 2)
    bits_pub, bits_crt, hs = pl.fixed_base_info()
    assert bits_pub and bits_pub % 8 == 0 and bits_crt % 8 == 0
    key, nonce = cr.rng_key(SEED + 52, cr.TWEAK_FIXED_BASE)
    # public form: side 0, the seeded call against the injected alpha
    alpha = cr.digits_many(key, nonce, range(cnt), 0, bits_pub // 8)
    c = pl.encrypt_u64(m, seed=SEED + 52, public=True, fixed_base=True)
    _same_rows(c, pl.encrypt_u64(m, r=alpha, public=True, fixed_base=True), np.arange(cnt))
    # key holder: separate exponents for p (side 0) and q (side 1), which one injected alpha cannot express
    c = pl.encrypt_u64(m, seed=SEED + 52, fixed_base=True)
    idx = _ends(cnt, 24)
    ap = cr.digits_many(key, nonce, idx, 0, bits_crt // 8)
    aq = cr.digits_many(key, nonce, idx, 1, bits_crt // 8)
    assert not set(ap) & set(aq)
    p2, q2 = p * p, q * q
    want = [_crt(p, q, (1 + int(x) * n) * pow(hs, a, p2) % p2, (1 + int(x) * n) * pow(hs, b, q2) % q2)
            for x, a, b in zip(m[idx], ap, aq)]
    _same_rows(c[idx], _rows(want, 2 * pl.n_words), idx)


# ---- unseeded calls (seed 0: the production form) ----------------------------------------------------------------
def test_unseeded_draws_are_fresh_and_fair(keys):
    """c = y_p^p = y_p (mod p): c mod p is the draw itself.  16,640 equal plaintexts, twice: every draw of both
    calls distinct mod p and mod q; the low words of 16,384 draws carry 524,288 bits, of which the ones must be
    within 6 sigma = 2,172 of half (sigma = sqrt(524288) / 2 = 362; a false alarm about once in 10^9 runs)."""
    pl = keys("gen2048")
    cnt = 16640
    m = np.full(cnt, 123456789, dtype=np.uint64)
    ca, cb = pl.encrypt_u64(m), pl.encrypt_u64(m)
    ints = _ints(np.concatenate([ca, cb]))
    modp = [x % pl.p for x in ints]
    assert len(set(modp)) == 2 * cnt
    assert len({x % pl.q for x in ints}) == 2 * cnt
    assert 0 not in modp and 1 not in modp
    ones = sum(bin(x & 0xFFFFFFFF).count("1") for x in modp[:16384])
    assert abs(ones - 262144) <= 2172, ones
    assert np.array_equal(pl.decrypt_u64(cb[:64]), m[:64])


def test_unseeded_public_rows_are_fresh(keys):
    pl = keys("gen2048")
    cnt = 16640
    m = np.full(cnt, 123456789, dtype=np.uint64)
    ca, cb = pl.encrypt_u64(m, public=True), pl.encrypt_u64(m, public=True)
    assert len({r.tobytes() for r in ca} | {r.tobytes() for r in cb}) == 2 * cnt
    assert np.array_equal(pl.decrypt_u64(cb[:64]), m[:64])


def test_unseeded_shared_single_encrypts_differ(keys):
    pl = keys("gen2048")
    one = np.array([42], dtype=np.uint64)
    a, b = pl.encrypt_u64_shared(one), pl.encrypt_u64_shared(one)
    assert not np.array_equal(a, b)
    assert pl.decrypt_u64(np.concatenate([a, b])).tolist() == [42, 42]
