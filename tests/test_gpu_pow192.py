"""Paillier-3072 on fthe_pow192: the public-key encrypt c = (1 + m n) r^n mod n^2 and the uniform scalar mul against
Python's integers, exact equality: at the edges of the modulus range, at every batch shape that takes another way
through the persistent launch, with seeded device randomness against the reference ChaCha20 sampler, through
GHPairs to the key holder's decrypt, in place, and under a memory limit that forces a narrower window."""
import functools
import random

import numpy as np
import pytest

import chacha_ref as cr
import n2_edges as ne
from test_gpu_mul192 import CW, MODULI, _dev, _ints, _key          # shared helpers; _key: Paillier.from_public
from test_pow192_model import mm

pytestmark = pytest.mark.gpu

NW = CW // 2
U64 = (1 << 64) - 1


def _rows(vals, words):
    return np.stack([np.frombuffer(int(v).to_bytes(4 * words, "little"), dtype=np.uint32) for v in vals])


@functools.lru_cache(maxsize=None)
def _rn(r, n):
    return pow(r, n, n * n)


def _enc(n, m, r):
    return [(1 + int(a) * n) * _rn(int(b), n) % (n * n) for a, b in zip(m, r)]


@pytest.mark.parametrize("ni", range(len(MODULI)))
def test_public_encrypt_at_the_modulus_edges(ni):
    pl = _key(ni)
    n, rng = pl.modulus, random.Random(ni)
    rs = [1, 2, n - 1, n - 2, 1 << 3040, rng.randrange(n)]
    m = [a for a in (0, 1, U64) for _ in rs]
    got = pl.encrypt_u64(np.array(m, np.uint64), r=rs * 3)       # without the feature: "not supported" here
    assert _ints(got) == _enc(n, m, rs * 3)
    mw = [n - 1, rng.getrandbits(3000)]
    assert _ints(pl.encrypt_words(mw, r=rs[-2:])) == _enc(n, mw, rs[-2:])
    for words in (1, 3):                                         # a narrow r_words zero-extends
        narrow = [rng.getrandbits(32 * words) | 1 for _ in range(2)]
        got = pl.encrypt_u64(np.array([5, U64], np.uint64), r=_rows(narrow, words))
        assert _ints(got) == _enc(n, [5, U64], narrow)


@pytest.fixture(scope="module")
def batch():
    """(m, r, expected rows by index) for the largest shape: expected values for its first 8 and last 65 rows; the
    rows take 16 values of r in turn (Python's r^n is the slow part) under distinct m"""
    import torch
    cnt = torch.cuda.get_device_properties(0).multi_processor_count * 64 + 3
    n, rng = MODULI[5], np.random.default_rng(50)
    m = rng.integers(0, U64, cnt, dtype=np.uint64, endpoint=True)
    r = rng.integers(0, 1 << 32, (16, NW), dtype=np.uint32)
    r[:, -1] >>= 1                                               # below 2^3071 <= n
    r = np.ascontiguousarray(r[np.arange(cnt) % 16])
    idx = list(range(8)) + list(range(cnt - 65, cnt))
    want = dict(zip(idx, _enc(n, m[idx], _ints(r[idx]))))
    return m, r, want


@pytest.mark.parametrize("count", [1, 7, 9, 65, "n_cu * 64 + 3"])
def test_batch_shapes(batch, count, monkeypatch):
    """the last `count` rows of the set; the largest makes a persistent workgroup take a second batch (its first and
    last 8 rows are checked); device form, and the host form over staging chunks of 4,096 rows"""
    import torch
    monkeypatch.setenv("FTHE_MUL192_CHUNK", "4096")
    pl = _key(5)
    m, r, want = batch
    count = len(m) if isinstance(count, str) else count
    at = list(range(len(m) - count, len(m)))
    at = at if count <= 65 else at[:8] + at[-8:]
    sel = [i - (len(m) - count) for i in at]
    md, rd = (torch.from_numpy(v[-count:].view(np.int32 if v is r else np.int64)).cuda() for v in (m, r))
    out = pl.encrypt_u64_dev(md, torch.empty((count, CW), dtype=torch.int32, device="cuda"), r=rd)
    pl.dev.sync()
    assert [_ints(out[sel])[k] == want[i] for k, i in enumerate(at)] == [True] * len(at)
    host = pl.encrypt_u64(m[-count:], r=r[-count:])
    assert [_ints(host[sel])[k] == want[i] for k, i in enumerate(at)] == [True] * len(at)


def test_seeded_device_randomness():
    """r from the reference sampler, as test_gpu_rng_stream._want_pub forms it; a shard equals the whole call's rows"""
    pl = _key(5)
    n, seed, cnt = pl.modulus, 0x5eed3072, 24
    m = np.random.default_rng(3).integers(0, U64, cnt, dtype=np.uint64, endpoint=True)
    key, nonce = cr.rng_key(seed, 0)
    rs, _ = cr.draw_below_many(key, nonce, range(cnt), n, n.bit_length(), pl.n_words)
    whole = pl.encrypt_u64(m, seed=seed, public=True)
    assert _ints(whole) == _enc(n, m, rs)
    assert np.array_equal(pl.encrypt_u64(m[9:20], seed=seed, public=True, index0=9), whole[9:20])


def test_round_trip_through_gradient_pairs():
    from fedtree_amd.paillier import GHPairs, Paillier
    holder = Paillier(_key(0).dev).keygen(3072, seed=3072)
    party = Paillier.from_public(holder.modulus, holder.dev)
    g = (np.random.default_rng(7).integers(-40, 40, 24) / 8).astype(np.float32)     # exact in the 10^-6 codec
    h = (np.random.default_rng(8).integers(0, 40, 24) / 8).astype(np.float32)
    gh = GHPairs(g.copy(), h.copy()).homo_encrypt(party, seed=11)
    assert gh.encrypted and not gh.g.any()
    gh.homo_decrypt(holder)
    assert np.array_equal(gh.g, g) and np.array_equal(gh.h, h)
    # the key holder's own public path gives what the party's does
    m = np.array([0, 3, U64], np.uint64)
    assert np.array_equal(holder.encrypt_u64(m, seed=5, public=True), party.encrypt_u64(m, seed=5))


@pytest.mark.parametrize("e", [2, 3, U64, random.Random(200).getrandbits(200) | 1 << 199, "n"])
def test_scalar_mul_in_place(e):
    pl = _key(3)
    N = pl.n2
    e = pl.modulus if e == "n" else e
    E = ne.hostile_rows(N, bits=32 * CW, nrand=4, seed=9)        # rows >= N included
    x = _dev(E)
    assert _ints(pl.scalar_mul_dev(x, e, x)) == [pow(v, e, N) for v in E]
    assert pl.dev.last_montmuls() == len(E) * mm.products(mm.plan(e)[1], False)


def test_memory_limit_narrows_the_window():
    """65 rows are two workgroups' tables; a limit between the tables of w = 2 and w = 3 runs w <= 2"""
    pl = _key(5)                                                 # the random n: a dense exponent, w = 5 when free
    N, e = pl.n2, pl.modulus
    E = (ne.hostile_rows(N, bits=32 * CW, nrand=49, seed=12))[:65]
    want, free = [pow(v, e, N) for v in E[:4] + E[-12:]], mm.products(mm.plan(e)[1], False)
    pl.dev.set_mem_limit(2 * 64 * 2 * 1024 + 65536)
    try:
        got = _ints(pl.scalar_mul_dev(_dev(E), e, _dev([0] * 65)))
        narrow = pl.dev.last_montmuls()
    finally:
        pl.dev.set_mem_limit(0)
    assert got[:4] + got[-12:] == want
    assert narrow == 65 * mm.products(mm.plan(e, wmax=2)[1], False) > 65 * free
