"""Paillier-3072 keys on the GPU: negate and subtract by the batched inverse on fthe_inv192_up / fthe_inv192_down against
Python's pow(x, -1, N), exact equality: at the edges of the modulus range on hostile unit rows, at every tree shape, in
place, with a non-unit in the batch, under a memory limit, and from a generated key to decrypted differences."""
from math import gcd

import numpy as np
import pytest

import n2_edges as ne
from test_gpu_mul192 import CW, MODULI, _dev, _host, _ints, _key  # shared helpers; MODULI[5]: a random 3072-bit n
from mul192_model import inverse_blocks, inverse_products, inverse_ws_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def radix8(monkeypatch):
    """the radix-8 kernels (read per call); unset, the calls run the binary tree on fthe_mul192"""
    monkeypatch.setenv("FTHE_INV192_TREE", "0")


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _fresh(ni=5):
    from fedtree_amd.paillier import Device, Paillier
    return Paillier.from_public(MODULI[ni], Device(0))


def _units(N, nrand, seed):
    return [v for v in ne.hostile_rows(N, bits=32 * CW, nrand=nrand, seed=seed) if gcd(v, N) == 1]


@pytest.mark.parametrize("ni", range(len(MODULI)))
def test_modulus_edges(ni):
    """1, N - 1 and, where the modulus leaves any, units >= N; every offset width, the widest above the smallest n"""
    pl = _key(ni)
    N, n = pl.n2, MODULI[ni]
    x = _units(N, 24, ni)
    a = x[5:] + x[:5]
    inv = [pow(v % N, -1, N) for v in x]
    assert 1 in x and N - 1 in x and len(x) >= 16 and (ni not in (1, 2, 3) or max(x) >= N)
    assert _ints(pl.invert_batch(_host(x))) == inv   # without the feature: "not supported" here
    for offset in (None, 1, 1 << 128, 1 << 3071):
        want = [s * t * (1 + (offset or 0) * n) % N for s, t in zip(a, inv)]
        assert _ints(pl.sub_inv_batch(_host(a), _host(x), offset)) == want, offset


@pytest.fixture(scope="module")
def pool():
    """1,000 units x and rows a on MODULI[5] as device rows, with x^-1 and a x^-1 (1 + 7 n) as host rows"""
    n = MODULI[5]
    N = n * n
    x = _units(N, 2000, 25)[:1000]
    a = x[1:] + [(1 << (32 * CW)) - 1]
    inv = [pow(v % N, -1, N) for v in x]
    return _dev(x), _dev(a), _host(inv), _host([s * t * (1 + 7 * n) % N for s, t in zip(a, inv)])


def _rows(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("count", [1, 8, 9, 64, 65, 513, "n_cu * 512 + 3"])
def test_tree_shapes(pool, count, monkeypatch):
    """the top alone, a last group of one member, two and three levels, a workgroup's second batch with a part-idle
    last wave; rows drawn with repetition from the pool; at 513 the binary tree on fthe_mul192 agrees byte for byte"""
    import torch
    xp, ap, inv, sub = pool
    pl = _key(5)
    count = _n_cu() * 512 + 3 if isinstance(count, str) else count
    idx = np.random.default_rng(count).integers(0, len(xp), count)
    x, a = xp[torch.from_numpy(idx).cuda()], ap[torch.from_numpy(idx).cuda()]
    got = pl.invert_dev(x, torch.empty_like(x))
    assert pl.dev.last_montmuls() == inverse_products(count, False)
    assert np.array_equal(_rows(got), inv[idx])
    got = pl.sub_inv_dev(a, x, torch.empty_like(x), offset=7)
    assert pl.dev.last_montmuls() == inverse_products(count, True)
    assert np.array_equal(_rows(got), sub[idx])
    if count == 513:
        monkeypatch.delenv("FTHE_INV192_TREE")
        assert torch.equal(pl.sub_inv_dev(a, x, torch.empty_like(x), offset=7), got)


@pytest.mark.parametrize("alias", ["x", "a", "b"])
def test_in_place(pool, alias):
    xp, ap, inv, sub = pool
    pl, x, a = _key(5), xp[100:165].clone(), ap[100:165].clone()
    if alias == "x":
        assert np.array_equal(_rows(pl.invert_dev(x, x)), inv[100:165])
    else:
        assert np.array_equal(_rows(pl.sub_inv_dev(a, x, a if alias == "a" else x, offset=7)), sub[100:165])


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("bad", ["0", "n"])
def test_non_unit_writes_nothing(pool, bad, limited):
    """the bad row last of 65; under half the workspace: chunks of 8, the bad row alone in the ninth"""
    import torch
    from fedtree_amd._lib import FTHE_ERR_ARG, FtheError
    pl = _fresh() if limited else _key(5)
    if limited:
        pl.dev.set_mem_limit(inverse_ws_bytes(65, inverse_blocks(65, _n_cu())) // 2)
    x = pool[0][:65].clone()
    x[64] = _dev([0 if bad == "0" else MODULI[5]])[0]
    out = torch.full_like(x, 0x5A5A5A5A)
    for call in (lambda: pl.invert_dev(x, out), lambda: pl.sub_inv_dev(pool[1][:65], x, out, offset=7)):
        with pytest.raises(FtheError) as e:
            call()
        assert e.value.status == FTHE_ERR_ARG and bool((out == 0x5A5A5A5A).all())


def test_memory_limit(pool):
    """a limit that admits 350 of 1,000 rows: three chunks, exact, every up-sweep run twice; below one row's: NOMEM"""
    import torch
    from fedtree_amd._lib import FTHE_ERR_NOMEM, FtheError
    xp, ap, inv, sub = pool
    pl = _fresh()
    pl.dev.set_mem_limit(inverse_ws_bytes(350, inverse_blocks(350, _n_cu())))
    x, a = xp[:1000], ap[:1000]
    assert np.array_equal(_rows(pl.sub_inv_dev(a, x, torch.empty_like(x), offset=7)), sub[:1000])
    assert pl.dev.last_montmuls() > inverse_products(1000, True)
    small = _fresh()
    small.dev.set_mem_limit(512)
    with pytest.raises(FtheError) as e:
        small.invert_dev(x, torch.empty_like(x))
    assert e.value.status == FTHE_ERR_NOMEM


@pytest.mark.parametrize("arm", ["0", None])
def test_generated_key_end_to_end(monkeypatch, arm):
    from fedtree_amd.paillier import Paillier
    if arm is None:
        monkeypatch.delenv("FTHE_INV192_TREE")      # the default: the binary tree
    pl = Paillier(_key(5).dev).keygen(3072, seed=3072)
    n = pl.modulus
    ma, mb = np.array([5, 1 << 63, 12345, 1], dtype=np.uint64), np.array([9, 3, 1 << 63, 1], dtype=np.uint64)
    ca, cb = pl.encrypt_u64(ma), pl.encrypt_u64(mb)
    diff, neg = pl.sub_inv_batch(ca, cb, 1 << 64), pl.invert_batch(ca)
    assert _ints(pl.decrypt_u64(diff, full=True)[1]) == [int(s) - int(t) + (1 << 64) for s, t in zip(ma, mb)]
    assert _ints(pl.decrypt_u64(neg, full=True)[1]) == [n - int(s) for s in ma]
    pub = Paillier.from_public(n, pl.dev)
    assert np.array_equal(pub.sub_inv_batch(ca, cb, 1 << 64), diff) and np.array_equal(pub.invert_batch(ca), neg)
