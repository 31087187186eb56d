"""Paillier-3072 keys on the GPU: segmented products, node histogram and scan on fthe_gprod192 against Python's integers,
exact equality, on hostile rows at the lowest and the highest modulus, and from a generated key to decrypted sums."""
from functools import reduce
from math import gcd

import numpy as np
import pytest

import n2_edges as ne
from test_gpu_mul192 import CW, MODULI, _dev, _host, _ints, _key  # shared helpers; MODULI[0]: highest N, [1]: lowest

pytestmark = pytest.mark.gpu


def _i64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _prods(N, x, seg, idx):
    return [reduce(lambda p, t: p * x[t] % N, idx[a:b], 1) for a, b in zip(seg, seg[1:])]


@pytest.mark.parametrize("ni", [1, 0])
def test_segment_lengths(ni):
    """no member (1), one (the all-ones row, >= N, comes out reduced), a full group, a second group of one, two and
    three passes; repeated, permuted members, all units mod N, so that every product is a non-zero integer (the rows
    congruent to 0, which are 0, N and kN, have the last segment to themselves); host CSR, device CSR and the host form"""
    pl = _key(ni)                                # without the feature: FTHE_ERR_UNSUPPORTED here
    x = ne.hostile_rows(pl.n2, bits=32 * CW, nrand=16, seed=ni)
    seg = np.cumsum([0, 0, 1, 2, 7, 8, 9, 64, 65, 3])
    idx = np.random.default_rng(ni).choice([i for i, v in enumerate(x) if gcd(v, pl.n2) == 1], seg[-1])
    idx[0], idx[-3:] = 13, [0, 9, 15]            # hostile_rows' all-ones row; its rows congruent to 0
    want, xd = _prods(pl.n2, x, seg, idx), _dev(x)
    assert want[1] == x[13] % pl.n2 and all(want[:-1]) and want[-1] == 0
    assert _ints(pl.reduce_segments_dev(xd, seg, _dev([0] * 9), idx=idx)) == want
    assert _ints(pl.reduce_segments_csr_dev(xd, _i64(seg), _dev([0] * 9), idx=_i64(idx))) == want
    assert _ints(pl.reduce_segments(_host(x), seg, idx)) == want


@pytest.fixture(scope="module")
def groups():
    import torch
    n_max = torch.cuda.get_device_properties(0).multi_processor_count * 64 + 3
    N = MODULI[5] ** 2
    rng = np.random.default_rng(23)
    x = ne.hostile_rows(N, bits=32 * CW) + _ints(rng.integers(0, 1 << 32, (1008, CW), dtype=np.uint32))
    seg = np.concatenate([[0], np.cumsum(np.arange(n_max) % 8 + 1)])    # 1..8 members in turn: a wave's octets differ
    idx = rng.integers(0, len(x), seg[-1])
    return _dev(x), seg, idx, _prods(N, x, seg, idx)


@pytest.mark.parametrize("count", [1, 7, 9, 65, "n_cu * 64 + 3"])
def test_batch_shapes(groups, count):
    """the last `count` segments; the largest: a persistent workgroup's second batch, a last wave part idle"""
    xd, seg, idx, want = groups
    count = len(want) if isinstance(count, str) else count
    s = seg[-count - 1:]
    got = _key(5).reduce_segments_csr_dev(xd, _i64(s - s[0]), _dev([0] * count), idx=_i64(idx[s[0]:]))
    assert _ints(got) == want[-count:] and _key(5).dev.last_montmuls() == 7 * count


def test_out_over_x():
    """out over the first 16 source rows, all rows units mod N.  Groups 0..7 (one wave's batch) have one member
    each and store after one product; groups 8..15 (another wave's) read rows 0..7 as their eighth member, six
    products later: a pass run in place would read what the first batch stored, the pass in the scratch does not"""
    pl = _key(1)
    x = [v for v in ne.hostile_rows(pl.n2, bits=32 * CW, nrand=24, seed=2) if gcd(v, pl.n2) == 1][:32]
    seg = np.cumsum([0] + [1] * 8 + [8] * 8)
    idx = np.array([16 + g for g in range(8)] + [r for g in range(8) for r in [*range(17 + g, 24 + g), g]])
    want, xd = _prods(pl.n2, x, seg, idx), _dev(x)
    assert len(x) == 32 and all(want) and _ints(pl.reduce_segments_dev(xd, seg, xd[:16], idx=idx)) == want


@pytest.mark.parametrize("zero_first", [False, True])
def test_histogram(zero_first):
    """features of 5, 17 and 40 bins, missing cells, a subset of the instances; an empty bin is 1 either way"""
    import torch
    pl = _key(1)
    N, n, nb, max_bin, rng = pl.n2, 300, 62, 40, np.random.default_rng(40)
    cut = np.array([0, 5, 22, nb], np.int32)
    bins = np.stack([rng.integers(0, w, n) for w in np.diff(cut)], 1).astype(np.uint8)
    bins[rng.random(bins.shape) < 0.1] = max_bin
    inst = np.sort(rng.choice(n, 217, replace=False)).astype(np.int32)
    x = ne.hostile_rows(N, bits=32 * CW, nrand=2 * n - 16, seed=3)
    ez = ne.hostile_rows(N, bits=32 * CW, nrand=2 * nb - 16, seed=4)
    want, populated = [1] * (2 * nb), set()
    for p, f in ((p, f) for p in range(2) for f in range(3)):
        for i in inst[bins[inst, f] != max_bin]:
            b = p * nb + cut[f] + bins[i, f]
            want[b] = want[b] * x[p * n + i] % N
            populated.add(b)
    if zero_first:
        want = [w * ez[b] % N if b in populated else 1 for b, w in enumerate(want)]
    got = pl.histogram_dev(_dev(x), n, 2, torch.from_numpy(bins).cuda(), cut, max_bin, _dev([0] * 2 * nb),
                           inst=torch.from_numpy(inst).cuda(), enc_zero=_dev(ez) if zero_first else None)
    assert _ints(got) == want and len(populated) < len(want)


def test_scan():
    pl = _key(0)
    x = ne.hostile_rows(pl.n2, bits=32 * CW, nrand=72, seed=8)
    seg = np.cumsum([0, 1, 8, 9, 70])
    want = []
    for t, v in enumerate(x):
        want.append(v % pl.n2 if t in seg else want[-1] * v % pl.n2)
    assert _ints(pl.scan_segments(_host(x), seg)) == want
    assert _ints(pl.scan_segments_dev(_dev(x), seg, _dev([0] * len(x)))) == want


def test_gradient_pairs_to_decrypted_sums():
    from fedtree_amd.paillier import GHPairs, HEParty, Paillier
    pl, rng = Paillier(_key(0).dev).keygen(3072, seed=3072), np.random.default_rng(6)
    n, cut, max_bin = 48, np.array([0, 4, 13]), 9
    bins = np.stack([rng.integers(0, 5, n), rng.integers(0, 9, n)], 1).astype(np.uint8)
    bins[bins[:, 0] == 4, 0] = max_bin                   # feature 0 has four bins: missing values
    g, h = (rng.integers(-40, 40, n) / 8).astype(np.float32), (rng.integers(0, 40, n) / 8).astype(np.float32)
    hist = HEParty(pl).compute_histogram(GHPairs(g.copy(), h.copy()).homo_encrypt(pl, seed=1), bins.reshape(-1), cut, 9)
    pre = HEParty(pl).prefix_histogram(hist, cut).homo_decrypt(pl)
    hist.homo_decrypt(pl)
    want = np.zeros((2, 13), np.float32)
    for f in range(2):
        ok = bins[:, f] != max_bin
        np.add.at(want[0], cut[f] + bins[ok, f], g[ok])
        np.add.at(want[1], cut[f] + bins[ok, f], h[ok])
    assert np.array_equal(hist.g, want[0]) and np.array_equal(hist.h, want[1])
    for f in range(2):
        want[:, cut[f]:cut[f + 1]] = np.cumsum(want[:, cut[f]:cut[f + 1]], axis=1)
    assert np.array_equal(pre.g, want[0]) and np.array_equal(pre.h, want[1])


def test_still_unsupported():
    one = _host([1, 2])
    for call in (lambda: _key(0).sub_batch(one, one), lambda: _key(0).dot_segments(one, [3, 4], [0, 2])):
        with pytest.raises(RuntimeError, match="not supported"):
            call()
