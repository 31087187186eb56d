"""Paillier-3072 keys on the GPU: add, k-way product and the uniform scalar mul on fthe_mul192 (rows of 192 words mod
a 6081..6144-bit n^2) against Python's integers -- x y % N and pow(x, e, N), exact equality -- at the edges of the
modulus range, on hostile rows (0, 1, N - 1, all-ones, rows >= N), at every batch shape that takes another way
through the persistent launch, in place, and the calls that stay unsupported at this size."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

import n2_edges as ne

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from mul192_model import edge_moduli  # noqa: E402

pytestmark = pytest.mark.gpu

CW = 192
PER_WAVE, PER_WG = 8, 64                         # rows of a wave's batch and of a workgroup's eight waves
MODULI = edge_moduli()
_PL = {}


def _key(ni):
    from fedtree_amd.paillier import Device, Paillier
    if "dev" not in _PL:
        _PL["dev"] = Device(0)
    if ni not in _PL:
        _PL[ni] = Paillier.from_public(MODULI[ni], _PL["dev"])
    return _PL[ni]


def _host(vals):
    raw = b"".join(int(v).to_bytes(4 * CW, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint32).reshape(len(vals), CW).copy()


def _dev(vals):
    import torch
    return torch.from_numpy(_host(vals).view(np.int32)).cuda()


def _ints(rows):
    a = rows.cpu().numpy() if hasattr(rows, "cpu") else rows
    a = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
    return [int.from_bytes(r.tobytes(), "little") for r in a]


def _same(got, want, label):
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (label, len(bad), bad[:8])


@pytest.mark.parametrize("ni", range(len(MODULI)))
def test_products_at_the_modulus_edges(ni):
    pl = _key(ni)                                # without the feature: FTHE_ERR_UNSUPPORTED here
    N = pl.n2
    E = ne.hostile_rows(N, bits=32 * CW, nrand=24, seed=ni)
    H, R = E[:16], E[16:]
    a = [x for x in H for _ in H] + R + R
    b = [y for _ in H for y in H] + R[1:] + R[:1] + [H[i % 16] for i in range(len(R))]
    _same(_ints(pl.add_batch(_host(a), _host(b))), [x * y % N for x, y in zip(a, b)], "add_batch")
    _same(_ints(pl.add_batch(_host(E), _host(E))), [x * x % N for x in E], "squarings")
    assert pl.dev.last_montmuls() == len(E)


@pytest.fixture(scope="module")
def rows():
    """(a, b, a b mod N) as ints for the largest batch shape: hostile rows at both ends, random rows between"""
    import torch
    n_max = torch.cuda.get_device_properties(0).multi_processor_count * PER_WG + 3
    N = MODULI[5] ** 2
    H = ne.hostile_rows(N, bits=32 * CW)
    w = np.random.default_rng(5).integers(0, 1 << 32, (2, n_max, CW), dtype=np.uint32)
    a, b = _ints(w[0]), _ints(w[1])
    a[:16], b[:16], a[-16:], b[-16:] = H, H[::-1], H[::-1], H[3:] + H[:3]
    return a, b, [x * y % N for x, y in zip(a, b)]


@pytest.mark.parametrize("count", [1, PER_WAVE - 1, PER_WAVE + 1, PER_WG + 1, "n_cu * PER_WG + 3"])
def test_batch_shapes(rows, count):
    """one row, a wave's batch short of a row and one over, a workgroup's rows and one, and three rows more than
    every CU's workgroup holds, so that a persistent workgroup takes a second batch; the last `count` rows of the
    set, device and host form, out apart, out = a, out = b"""
    import torch
    pl = _key(5)
    count = len(rows[0]) if isinstance(count, str) else count
    a, b, want = (v[-count:] for v in rows)
    ah, bh = _host(a), _host(b)
    ad, bd = _dev(a), _dev(b)
    _same(_ints(pl.add_dev(ad, bd, torch.empty_like(ad))), want, "dev")
    x = ad.clone()
    _same(_ints(pl.add_dev(x, bd, x)), want, "dev, out = a")
    y = bd.clone()
    _same(_ints(pl.add_dev(ad, y, y)), want, "dev, out = b")
    pl.dev.sync()
    _same(_ints(pl.add_batch(ah, bh)), want, "host")
    for label, alias in (("host, out = a", 0), ("host, out = b", 1)):
        ops = [ah.copy(), bh.copy()]
        p = [ctypes.c_void_p(v.ctypes.data) for v in ops]
        assert pl.lib.fthe_add(pl._key, pl.dev.ctx, p[0], p[1], count, p[alias]) == 0
        _same(_ints(ops[alias]), want, label)


def test_host_add_in_chunks(rows, monkeypatch):
    """the host form over several staging chunks (4,096 rows each, the last one partial), out apart, = a and = b"""
    monkeypatch.setenv("FTHE_MUL192_CHUNK", "4096")
    pl = _key(5)
    a, b, want = rows
    assert len(a) > 3 * 4096
    for label, alias in (("host", 2), ("host, out = a", 0), ("host, out = b", 1)):
        ops = [_host(a), _host(b), np.zeros((len(a), CW), np.uint32)]
        p = [ctypes.c_void_p(v.ctypes.data) for v in ops]
        assert pl.lib.fthe_add(pl._key, pl.dev.ctx, p[0], p[1], len(a), p[alias]) == 0
        _same(_ints(ops[alias]), want, label)


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_reduce_kway(k):
    import torch
    pl = _key(0)
    N = pl.n2
    E = ne.hostile_rows(N, bits=32 * CW, nrand=4, seed=k)
    planes = [E[j:] + E[:j] for j in range(k)]
    want = [1] * len(E)
    for p in planes:
        want = [w * x % N for w, x in zip(want, p)]
    x = np.stack([_host(p) for p in planes])
    _same(_ints(pl.reduce_kway(x)), want, "host")
    for label, plane in (("out = plane 0", 0), ("out = the last plane", k - 1)):   # the last: through the scratch
        xd = torch.from_numpy(x.view(np.int32)).cuda()
        _same(_ints(pl.reduce_kway_dev(xd, k, xd[plane])), want, label)
    assert pl.dev.last_montmuls() == len(E) * max(k - 1, 1)


@pytest.mark.parametrize("e", [0, 1, 2, (1 << 64) - 1, "n"])
def test_scalar_mul(e):
    pl = _key(3)
    N = pl.n2
    e = pl.modulus if e == "n" else e
    E = ne.hostile_rows(N, bits=32 * CW, nrand=4, seed=7)
    want = [pow(x, e, N) for x in E]
    if e < 1 << 64:
        _same(_ints(pl.scalar_mul(_host(E), e)), want, "host")
    else:
        assert [pl.mul(x, e) for x in E[13:15]] == want[13:15]         # fthe_scalar_mul_words
    x = _dev(E)
    _same(_ints(pl.scalar_mul_dev(x, e, x)), want, "dev, out = x")


def test_untouched_sizes():
    from fedtree_amd.paillier import Paillier
    with pytest.raises(RuntimeError, match="not supported"):
        Paillier.from_public(random.Random(1).getrandbits(2560) | (1 << 2559) | 1, _key(0).dev)
    pl = _key(0)
    one = _host([1, 2])
    with pytest.raises(RuntimeError, match="not supported"):
        pl.sub_batch(one, one)
    assert pl.lib.fthe_kernel_limbs(6144) == 0
