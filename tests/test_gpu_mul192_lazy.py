"""The Paillier-3072 kernels of fthe_mul192.hip on the crafted inputs of mul192_cases.py, exact equality
with Python's integers on every row: each class of quotient and of lazy remainder and every borrow pattern of step 4 on
fthe_mul192 and fthe_gprod192, chains that keep bit 6144 in the multiplier column, powers and inverses whose factors
and conversions carry it, and the two loops that split a call into several launches."""
import time

import numpy as np
import pytest

import mul192_cases as mc
import n2_edges as ne
from mul192_cases import mm
from test_gpu_mul192 import CW, MODULI, _dev, _ints
from test_gpu_mul192 import _key as _edge_key

pytestmark = pytest.mark.gpu

MODS = mc.moduli()
ALL = range(len(MODS))
POW_BUDGET = 16384                               # kPowBudget of fedtree_amd/csrc/mul192_image.hpp
_PL = {}


def _key(ni):
    from fedtree_amd.paillier import Paillier
    if ni < len(MODULI):
        return _edge_key(ni)
    if ni not in _PL:
        _PL[ni] = Paillier.from_public(MODS[ni], _edge_key(0).dev)
    return _PL[ni]


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _i64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _same(got, want, label):
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert len(got) == len(want) and not bad, (label, len(bad), bad[:8])


@pytest.mark.parametrize("count", [1, 63, 65, 1100])
@pytest.mark.parametrize("ni", ALL)
def test_mul192_classes_and_borrows(ni, count):
    """all of (a) and (b); at 1,100 rows every case in octet 0 and in octet 7, random rows between; out apart, out = a"""
    import torch
    pl, N = _key(ni), MODS[ni] ** 2
    cases, rng = mc.mul_cases(ni), np.random.default_rng(100 * ni + count)
    fill = _ints(rng.integers(0, 1 << 32, (2 * count, CW), dtype=np.uint32))
    pairs = [(fill[2 * i], fill[2 * i + 1]) if c is None else cases[c] for i, c in enumerate(mc.layout(len(cases), count))]
    a, b = _dev([p[0] for p in pairs]), _dev([p[1] for p in pairs])
    want = [x * y % N for x, y in pairs]
    _same(_ints(pl.add_dev(a, b, torch.empty_like(a))), want, "out apart")
    _same(_ints(pl.add_dev(a, b, a)), want, "out = a")


@pytest.mark.parametrize("ni", ALL)
def test_gprod192_borrows_and_chains(ni):
    """(b) as groups of one and of two members, the chains of (c) between them: a wave's groups differ in length"""
    pl, N = _key(ni), MODS[ni] ** 2
    rows, seg, idx = mc.gprod_input(ni)
    groups = mc.gprod_groups(rows, seg, idx)
    assert any(len({len(g) for g in groups[at:at + 8]}) > 2 for at in range(0, len(groups), 8))
    got = pl.reduce_segments_csr_dev(_dev(rows), _i64(seg), _dev([0] * len(groups)), idx=_i64(idx))
    _same(_ints(got), [mm.reduce_mod(g, N) for g in groups], "groups")
    assert pl.dev.last_montmuls() == 7 * len(groups)


@pytest.mark.parametrize("ni", ALL)
def test_scan_stores_every_prefix_of_a_chain(ni):
    pl, N = _key(ni), MODS[ni] ** 2
    rows, seg = mc.scan_input(ni)
    want = [mm.reduce_mod(g, N) for g in mc.scan_groups(rows, seg)]
    _same(_ints(pl.scan_segments_dev(_dev(rows), seg, _dev([0] * len(rows)))), want, "prefixes")


@pytest.mark.parametrize("e", [2, 3, "n"])
@pytest.mark.parametrize("ni", mc.HIGH)
def test_pow192_factors_with_bit_6144(ni, e):
    """in place; the rows' small powers are lazy remainders N + x0^p at or above 2^6144"""
    pl, N = _key(ni), MODS[ni] ** 2
    e = MODS[ni] if e == "n" else e
    rows = mc.pow_rows(ni, e)
    x = _dev(rows)
    _same(_ints(pl.scalar_mul_dev(x, e, x)), [pow(v, e, N) for v in rows], "out = x")
    assert pl.dev.last_montmuls() == len(rows) * mm.products(mm.plan(e)[1], False)


@pytest.mark.parametrize("count", [9, 64, 65])
@pytest.mark.parametrize("ni", mc.HIGH + (1, 5))
def test_inv192_chains_and_targets(ni, count, monkeypatch):
    """one level, one level of whole groups, two levels with a short last group; out apart and out = x; the binary
    tree on fthe_mul192 agrees byte for byte"""
    import torch
    monkeypatch.setenv("FTHE_INV192_TREE", "0")
    pl, n = _key(ni), MODS[ni]
    N = n * n
    xs, a = mc.inverse_input(ni, count)
    inv = [pow(v, -1, N) for v in xs]
    sub = [s * t * (1 + n) % N for s, t in zip(a, inv)]
    x, ad = _dev(xs), _dev(a)
    got_inv = pl.invert_dev(x, torch.empty_like(x))
    assert pl.dev.last_montmuls() == mm.inverse_products(count, False)
    _same(_ints(got_inv), inv, "invert")
    got_sub = pl.sub_inv_dev(ad, x, torch.empty_like(x), offset=1)
    assert pl.dev.last_montmuls() == mm.inverse_products(count, True)
    _same(_ints(got_sub), sub, "sub_inv")
    y = x.clone()
    assert torch.equal(pl.invert_dev(y, y), got_inv)
    y = x.clone()
    assert torch.equal(pl.sub_inv_dev(ad, y, y, offset=1), got_sub)
    monkeypatch.delenv("FTHE_INV192_TREE")
    assert torch.equal(pl.invert_dev(x, torch.empty_like(x)), got_inv)
    assert torch.equal(pl.sub_inv_dev(ad, x, torch.empty_like(x), offset=1), got_sub)


def _bases(N, seed):
    H = ne.hostile_rows(N, bits=32 * CW, nrand=8, seed=seed)
    return [H[i] for i in (1, 2, 3, 5, 9, 10, 13, 14)] + H[16:]


def _check_period(out, want, first, label):
    """every row against the first period on the device; the period, the rows round `first` and the last 67 by Python"""
    import torch
    count, period = len(out), len(want)
    whole = count // period * period
    assert torch.equal(out[:whole].view(-1, period, CW), out[:period].expand(whole // period, period, CW)), label
    assert torch.equal(out[whole:], out[:count - whole]), label
    at = list(range(period)) + list(range(first - 8, first + 8)) + list(range(count - 67, count))
    got = _ints(out[torch.tensor(at, device=out.device)])
    _same(got, [want[i % period] for i in at], label)


@pytest.fixture(scope="module")
def powers():
    """16 bases (hostile rows among them) and their powers n on the random 3072-bit n"""
    e = MODULI[5]
    rows = _bases(e * e, 31)
    return rows, [pow(v, e, e * e) for v in rows]


@pytest.mark.parametrize("in_place", [False, True])
def test_launch_pow_second_launch(powers, in_place):
    """67 rows more than launch_pow's first launch takes: the second launch's offsets into x and out, with fewer
    workgroups on the same tables.  About 2 s on an MI355X (printed)."""
    import torch
    pl, e = _key(5), MODULI[5]
    products = mm.products(mm.plan(e)[1], False)
    first = 64 * _n_cu() * (POW_BUDGET // products)
    count = first + 67
    assert min(-(-count // 64), _n_cu()) * 64 * max(1, POW_BUDGET // products) == first < count
    rows, want = powers
    x = _dev(rows)[torch.arange(count, device="cuda") % len(rows)].contiguous()
    out = x if in_place else torch.empty_like(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pl.scalar_mul_dev(x, e, out)
    pl.dev.sync()
    torch.cuda.synchronize()
    print(f"launch_pow split: {count} rows, {products} products each, {time.perf_counter() - t0:.2f} s")
    assert pl.dev.last_montmuls() == count * products
    _check_period(out, want, first, "x^n")


def test_launch_pow_second_launch_narrow_rows(monkeypatch):
    """the same split with rows of 3 words: the public encrypt with injected r, one host chunk over the whole call"""
    import torch
    pl, n = _key(5), MODULI[5]
    products = mm.products(mm.plan(n, True)[1], True)
    first = 64 * _n_cu() * (POW_BUDGET // products)
    count = first + 67
    monkeypatch.setenv("FTHE_MUL192_CHUNK", str(-(-count // 256) * 256))
    rng = np.random.default_rng(77)
    r16 = rng.integers(1, 1 << 32, (16, 3), dtype=np.uint32)
    m16 = rng.integers(0, (1 << 64) - 1, 16, dtype=np.uint64, endpoint=True)
    want = [(1 + int(m) * n) * pow(r, n, n * n) % (n * n) for m, r in zip(m16, _ints(r16))]
    sel = torch.arange(count, device="cuda") % 16
    r = torch.from_numpy(r16.view(np.int32)).cuda()[sel].contiguous()
    m = torch.from_numpy(m16.view(np.int64)).cuda()[sel].contiguous()
    out = pl.encrypt_u64_dev(m, torch.empty((count, CW), dtype=torch.int32, device="cuda"), r=r)
    pl.dev.sync()
    assert pl.dev.last_montmuls() == count * products
    _check_period(out, want, first, "(1 + m n) r^n")


def test_launch_mul192_second_launch():
    """2^22 + 67 rows: the second launch's offsets.  Both operands are views of one tiled buffer, half a period apart"""
    import torch
    if torch.cuda.mem_get_info()[0] < 16 << 30:
        pytest.skip("needs 16 GB of free device memory")
    pl, N = _key(5), MODULI[5] ** 2
    period, first = 1024, 1 << 22
    count = first + 67
    H = ne.hostile_rows(N, bits=32 * CW, nrand=period - 16, seed=22)
    rows = H[16:500] + H[:16] + H[500:]
    want = [rows[i] * rows[(i + period // 2) % period] % N for i in range(period)]
    big = _dev(rows).repeat(count // period + 2, 1)
    a, b = big[:count], big[period // 2:period // 2 + count]
    out = torch.empty_like(a)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pl.add_dev(a, b, out)
    pl.dev.sync()
    torch.cuda.synchronize()
    print(f"launch_mul192 split: {count} rows, {time.perf_counter() - t0:.3f} s")
    _check_period(out, want, first, "x y")
