"""Paillier-3072 packed and slot-packed pairs: the compress on fthe_horner192 against Horner on Python's integers, exact
equality, at the edges of the modulus range, at every batch shape that takes another way through the persistent
launch and across a launch split; the packed and slot encrypts on the public path against (1 + m n) r^n mod n^2; and
the whole flow from a party's encrypt to the key holder's decrypt against the two-ciphertext flow."""
import functools

import numpy as np
import pytest

import n2_edges as ne
from test_gpu_mul192 import CW, MODULI, _dev, _host, _ints, _key       # shared helpers; _key: Paillier.from_public

pytestmark = pytest.mark.gpu


def _planes(count, rows):
    """planes of output row i when count rows lie in planes of `rows`"""
    return [len(range(i, count, rows)) for i in range(rows)]


def _horner(x, rows, sb, N, only=None):
    """{i: prod_j x[j rows + i]^(2^(j sb)) mod N} from the top plane down; a lone plane is the row itself"""
    out = {}
    for i in range(rows) if only is None else only:
        r, *rest = [x[k] for k in range(i, len(x), rows)][::-1]
        for v in rest:
            r = pow(r, 1 << sb, N) * v % N
        out[i] = r
    return out


def _products(count, rows, sb):
    return sum(1 + (p - 1) * (sb + 1) for p in _planes(count, rows))


@pytest.mark.parametrize("count,slots,sb", [(7, 3, 224), (6, 3, 256), (5, 1, 224), (109, 0, 224)])
@pytest.mark.parametrize("ni", range(len(MODULI)))
def test_compress_at_the_modulus_edges(ni, count, slots, sb):
    """both plane counts in one batch of eight; nA = rows; the copy; the key's 13 slots over two batches"""
    pl = _key(ni)
    N = pl.n2
    x = [N - 1, 0, 1] + [v % N for v in ne.hostile_rows(N, bits=32 * CW, nrand=90, seed=ni)][::-1]
    x = x[:count]
    rows = -(-count // (slots or 13))
    want = list(_horner(x, rows, sb, N).values())
    out = _dev([0] * rows)
    pl.compress_gh_slots_dev(_dev(x), count, sb, out, slots=slots)       # without the feature: "not supported" here
    pl.dev.sync()
    assert _ints(out) == want
    assert pl.dev.last_montmuls() == _products(count, rows, sb)
    assert _ints(pl.compress_gh_slots(_host(x), sb, slots=slots)) == want
    assert pl.dev.last_montmuls() == _products(count, rows, sb)


@pytest.mark.parametrize("rows", [1, 7, 9, 65, "n_cu * 64 + 3"])
def test_batch_shapes(rows, monkeypatch):
    """two slots, the last row with one plane; the largest makes a persistent workgroup take a second batch; device
    form, and the host form over staging chunks of 4,096 output rows"""
    import torch
    monkeypatch.setenv("FTHE_MUL192_CHUNK", "4096")
    pl = _key(5)
    if isinstance(rows, str):
        rows = torch.cuda.get_device_properties(0).multi_processor_count * 64 + 3
    count, pool = 2 * rows - 1, _ints(np.random.default_rng(52).integers(0, 1 << 32, (37, CW), dtype=np.uint32))
    at = np.arange(count) % 37
    sel = sorted(set(range(rows)[:8]) | set(range(rows)[-8:]))
    want = _horner([pool[k] for k in at], rows, 224, pl.n2, only=sel)
    xd = _dev(pool)[torch.from_numpy(at).cuda()]
    out = pl.compress_gh_slots_dev(xd, count, 224, torch.empty((rows, CW), dtype=torch.int32, device="cuda"), slots=2)
    pl.dev.sync()
    assert _ints(out[sel]) == [want[i] for i in sel]
    assert pl.dev.last_montmuls() == _products(count, rows, 224)
    assert _ints(pl.compress_gh_slots(xd.cpu().numpy().view(np.uint32), 224, slots=2)[sel]) == [want[i] for i in sel]


def test_one_launch_split():
    """two slots of 1,504 bits cost 1,506 products a row, so a wave runs 16384 // 1506 = 10 batches in one launch: one
    row more than n_cu * 64 * 10 needs a second launch"""
    import torch
    pl = _key(4)
    rows = torch.cuda.get_device_properties(0).multi_processor_count * 64 * (16384 // 1506) + 1
    pool = ne.hostile_rows(pl.n2, bits=32 * CW, nrand=15, seed=4)
    at = np.arange(2 * rows) % 31
    sel = [0, 1, rows - 2, rows - 1]
    want = [pow(pool[at[rows + i]], 1 << 1504, pl.n2) * pool[at[i]] % pl.n2 for i in sel]
    xd = _dev(pool)[torch.from_numpy(at).cuda()]
    out = pl.compress_gh_slots_dev(xd, 2 * rows, 1504, torch.empty((rows, CW), dtype=torch.int32, device="cuda"), slots=2)
    pl.dev.sync()
    assert _ints(out[sel]) == want
    assert pl.dev.last_montmuls() == rows * 1506


@functools.lru_cache(maxsize=None)
def _rn(r, n):
    return pow(r, n, n * n)


@pytest.mark.parametrize("ni", [1, 3])
def test_packed_and_slot_encrypt_against_the_formula(ni):
    from fedtree_amd import paillier as P
    pl = _key(ni)
    n, rng = pl.modulus, np.random.default_rng(ni)
    g = (rng.integers(-4000, 4000, 15) / 8).astype(np.float32)
    h = (rng.integers(0, 4000, 15) / 8).astype(np.float32)
    rs = [n - 1, 2, int.from_bytes(rng.bytes(380), "little")]
    m = P.pack_gh(g, h)
    for got, ms, r in ((pl.encrypt_gh_packed(g, h, r=(rs * 5)), _ints(m), rs * 5),
                       (pl.encrypt_gh_slots(g, h, 224, r=rs[1:]), _ints(P.pack_gh_slots(m, 224, 13)), rs[1:])):
        assert _ints(got) == [(1 + a * n) * _rn(b, n) % (n * n) for a, b in zip(ms, r)]
    # seeded device randomness: a shard with index0 equals the whole call's rows
    whole = pl.encrypt_gh_packed(g, h, seed=0x5eed)
    assert np.array_equal(pl.encrypt_gh_packed(g[4:9], h[4:9], seed=0x5eed, index0=4), whole[4:9])


def test_party_to_key_holder():
    from fedtree_amd import paillier as P
    holder = P.Paillier(_key(0).dev).keygen(3072, seed=3072)
    party = P.Paillier.from_public(holder.modulus, holder.dev)
    rng = np.random.default_rng(27)
    g, g2 = ((rng.integers(-40, 40, 30) / 8).astype(np.float32) for _ in range(2))
    h, h2 = ((rng.integers(0, 40, 30) / 8).astype(np.float32) for _ in range(2))
    two, two2 = (P.GHPairs(a, b).homo_encrypt(party, seed=s) for a, b, s in ((g, h, 1), (g2, h2, 2)))
    diff = holder.decrypt_u64(party.sub_inv_batch(np.concatenate([two.g_enc, two.h_enc]),
                                                  np.concatenate([two2.g_enc, two2.h_enc]), 1 << 64))
    ref = two.homo_decrypt(holder)
    pk, pk2 = (P.GHPairs(a, b, packed=True).homo_encrypt(party, seed=s) for a, b, s in ((g, h, 3), (g2, h2, 4)))
    flows = [(pk.compress(), False), (pk.compress(slots=6), True),
             (P.GHPairs(g, h, packed=True).homo_encrypt(party, seed=5, slot_bits=224), False)]
    assert [(f.slots, len(f.g_enc)) for f, _ in flows] == [(13, 3), (6, 5), (13, 3)]
    for f, short in flows:
        f.homo_decrypt(holder, short=short)
        assert np.array_equal(f.g, ref.g) and np.array_equal(f.h, ref.h)
    sub = pk.compress().sub_inv(pk2.compress()).homo_decrypt(holder)
    assert np.array_equal(sub.g, P.decode_fixed(diff[:30])) and np.array_equal(sub.h, P.decode_fixed(diff[30:]))
    assert np.array_equal(ref.g, g) and np.array_equal(sub.g, g - g2)
