"""Differential matrix of the products mod n^2 over dispatch regimes x operations x hostile operands.

Keys: tests/golden/n2_edge_keys.json (tests/n2_edges.py): N = n^2 at each end of the three ranges that pick the
kernel (matrix-core Barrett add fthe_addb_q152 for N >= 2^4094; the classical MSB-first product MULWC / MULWGC
for 2^4093 <= N < 2^4094; the Montgomery pair below), each on its default path and on the forced alternates
(FTHE_ADD_NO_ADDB=1: classical instead of addb; FTHE_ADD_MONT=1: the Montgomery pair, read at key set-up and
at call time, so it is set around both), plus two Paillier-1024 keys on the one-lane kernels.
Operands: n2_edges.hostile_rows -- 0, 1, N - 1, rows >= N up to the largest multiple of N in a row (7N on
cls_lo; not ciphertexts, but the reference's x y mod n^2, paillier.cpp:103, reduces them all the same), and
random rows.  Every result is compared with Python's integers: exact equality, no tolerance.
The path each call took is asserted from fthe_last_montmuls and the profiled launch count."""
import ctypes

import numpy as np
import pytest

import n2_edges as ne

pytestmark = pytest.mark.gpu

ENV = {"default": (), "noaddb": ("FTHE_ADD_NO_ADDB",), "mont": ("FTHE_ADD_MONT",)}
CASES = [(k, "default") for k in ne.KEYS_2048] + [(k, "noaddb") for k in ne.ADDB_KEYS] + \
        [(k, "mont") for k in ne.KEYS_2048 if ne.REGIME[k] != "mont"] + [(k, "default") for k in ne.KEYS_1024]
IDS = [f"{k}-{p}" for k, p in CASES]
NH = 16                      # hostile rows at the head of E
_PL = {}


def _kind(name, path):
    """the product the pairwise add must run on: 'addb', 'cls', 'mont' (four-lane row I/O) or 'slot'
    (Paillier-1024: one-lane kernels, slot form, Montgomery pair)"""
    if name in ne.KEYS_1024:
        return "slot"
    if path == "mont":
        return "mont"
    reg = ne.REGIME[name]
    return "cls" if (reg == "addb" and path == "noaddb") else reg


@pytest.fixture
def ck(request, monkeypatch):
    """(Paillier, kind, E) of one (key, path) case with the path's switch set for the whole test"""
    from fedtree_amd.paillier import Device, Paillier
    name, path = request.param
    for v in ENV[path]:
        monkeypatch.setenv(v, "1")
    if "dev" not in _PL:
        _PL["dev"] = Device(0)
    if (name, path) not in _PL:
        p, q = ne.load_keys()[name]
        pl = Paillier.from_primes(p, q, _PL["dev"])
        E = ne.hostile_rows(pl.n2, 64 * pl.n_words, nrand=200, seed=len(name))
        _PL[name, path] = (pl, _kind(name, path), E)
    return _PL[name, path]


cases = pytest.mark.parametrize("ck", CASES, ids=IDS, indirect=True)


def _dev(vals, cw):
    import torch
    raw = b"".join(int(v).to_bytes(4 * cw, "little") for v in vals)
    return torch.from_numpy(np.frombuffer(raw, dtype=np.int32).reshape(len(vals), cw).copy()).cuda()


def _host(vals, cw):
    raw = b"".join(int(v).to_bytes(4 * cw, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint32).reshape(len(vals), cw).copy()


def _ints(rows):
    a = rows.cpu().numpy() if hasattr(rows, "cpu") else rows
    a = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
    return [int.from_bytes(r.tobytes(), "little") for r in a]


def _diff(got, want, label):
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (label, len(bad), bad[:8])


def _profiled(pl, fn):
    """run fn with the launch profile on: (montmuls per call from fthe_last_montmuls, profiled program launches)"""
    lib, dev = pl.lib, pl.dev
    lib.fthe_prof_enable(dev.ctx, 1)
    try:
        fn()
        mm = dev.last_montmuls()
        vals = [ctypes.c_double() for _ in range(7)]
        assert lib.fthe_prof_read(dev.ctx, *[ctypes.byref(v) for v in vals]) == 0
    finally:
        lib.fthe_prof_enable(dev.ctx, 0)
    return mm, vals[1].value


def _grid(E):
    """the full hostile x hostile grid, hostile x random, and random pairs"""
    H, R = E[:NH], E[NH:]
    a = [x for x in H for _ in H] + [H[i % NH] for i in range(len(R))] + R + R
    b = [y for _ in H for y in H] + R + [H[(i * 5 + 3) % NH] for i in range(len(R))] + R[1:] + R[:1]
    return a, b


@cases
def test_add(ck):
    import torch
    pl, kind, E = ck
    N, cw = pl.n2, 2 * pl.n_words
    a, b = _grid(E)
    want = [x * y % N for x, y in zip(a, b)]
    ad, bd = _dev(a, cw), _dev(b, cw)
    out = torch.empty_like(ad)
    mm, launches = _profiled(pl, lambda: pl.add_dev(ad, bd, out))
    pl.dev.sync()
    _diff(_ints(out), want, "add_dev")
    # the path taken: one product per row on the matrix-core kernel (its launch bypasses the profiled program
    # launcher) or on the classical product (one program launch); two on the Montgomery pair
    assert mm / len(a) == {"addb": 1, "cls": 1, "mont": 2, "slot": 2}[kind]
    assert (launches == 0) == (kind == "addb"), launches
    x = ad.clone()
    pl.add_dev(x, bd, x)                                     # out = a
    y = bd.clone()
    pl.add_dev(ad, y, y)                                     # out = b
    pl.dev.sync()
    assert torch.equal(x, out) and torch.equal(y, out)
    h = pl.add_batch(_host(a[:300], cw), _host(b[:300], cw))
    _diff(_ints(h), want[:300], "add_batch")


@cases
def test_sub(ck):
    import torch
    pl, kind, E = ck
    N, cw = pl.n2, 2 * pl.n_words
    a, b = _grid(E)
    a, b = a[:NH * NH + 64], b[:NH * NH + 64]
    want = [x * pow(y, 2**64 - 1, N) % N for x, y in zip(a, b)]
    ad, bd = _dev(a, cw), _dev(b, cw)
    out = torch.empty_like(ad)
    pl.sub_dev(ad, bd, out)
    pl.dev.sync()
    _diff(_ints(out), want, "sub_dev")
    h = pl.sub_batch(_host(a[:100], cw), _host(b[:100], cw))
    _diff(_ints(h), want[:100], "sub_batch")


@cases
def test_scalar_mul_and_mul(ck):
    pl, kind, E = ck
    N, cw = pl.n2, 2 * pl.n_words
    rows = E[:NH + 48]
    xw = _host(rows, cw)
    for k in (0, 1, 2, 12345, 2**63, 2**64 - 1):
        _diff(_ints(pl.scalar_mul(xw, k)), [pow(x, k, N) for x in rows], ("scalar_mul", k))
    e = (1 << 100) + 0x1234567890ABCDEF                        # an exponent above 64 bits: fthe_scalar_mul_words
    _diff([pl.mul(x, e) for x in E[:NH]], [pow(x, e, N) for x in E[:NH]], "mul")


@cases
def test_reduce_kway(ck):
    import torch
    pl, kind, E = ck
    N, cw = pl.n2, 2 * pl.n_words
    cnt = len(E)
    for kk in (2, 3, 15, 16):
        # plane j is E rotated and strided, so every output multiplies hostile and random rows
        planes = [[E[(i * (2 * j + 1) + 5 * j) % cnt] for i in range(cnt)] for j in range(kk)]
        want = []
        for i in range(cnt):
            acc = planes[0][i]
            for j in range(1, kk):
                acc = acc * planes[j][i] % N
            want.append(acc % N)
        xd = _dev([v for pj in planes for v in pj], cw)
        out = torch.empty((cnt, cw), dtype=torch.int32, device="cuda")
        mm, launches = _profiled(pl, lambda: pl.reduce_kway_dev(xd, kk, out))
        pl.dev.sync()
        _diff(_ints(out), want, ("reduce_kway", kk))
        # addb: a chain of kk - 1 matrix-core adds; classical: kk - 1 products while the kk + 1 row pointers fit
        # the row-I/O table (16), else the slot form with kk Montgomery products (R^kk correction included)
        rowio = kind != "slot" and kk + 1 <= 16
        assert mm / cnt == {"addb": kk - 1, "cls": kk - 1 if rowio else kk, "mont": kk, "slot": kk}[kind], kk
        assert (launches == 0) == (kind == "addb"), (kk, launches)


SEG_LENS = (0, 1, 7, 8, 9, 64, 65)


@cases
def test_reduce_segments(ck):
    import torch
    pl, kind, E = ck
    N, cw = pl.n2, 2 * pl.n_words
    seg = np.concatenate([[0], np.cumsum(SEG_LENS)]).astype(np.int64)
    total = int(seg[-1])
    # a gather with repeats: two of three members are hostile rows
    idx = np.array([(t * 7) % NH if t % 3 else NH + (t * 11) % (len(E) - NH) for t in range(total)], np.int64)
    xd = _dev(E, cw)

    def ref(members):
        out = []
        for s in range(len(seg) - 1):
            acc = 1
            for t in range(seg[s], seg[s + 1]):
                acc = acc * E[members[t]] % N
            out.append(acc)
        return out
    out = torch.empty((len(seg) - 1, cw), dtype=torch.int32, device="cuda")
    for label, ix in (("gather", idx), ("contiguous", None)):
        want = ref(idx if ix is not None else np.arange(total))
        pl.reduce_segments_dev(xd, seg, out, idx=ix)
        pl.dev.sync()
        _diff(_ints(out), want, ("reduce_segments_dev", label))
        out.zero_()
        pl.reduce_segments_csr_dev(xd, torch.from_numpy(seg).cuda(), out,
                                   idx=None if ix is None else torch.from_numpy(ix).cuda())
        pl.dev.sync()
        _diff(_ints(out), want, ("reduce_segments_csr_dev", label))


@cases
def test_scan_segments(ck):
    import torch
    pl, kind, E = ck
    N, cw = pl.n2, 2 * pl.n_words
    seg = np.concatenate([[0], np.cumsum((0, 1, 8, 9, 65))]).astype(np.int64)
    total = int(seg[-1])
    rows = [E[(t * 5) % 48] for t in range(total)]             # hostile rows at every third position
    want = []
    for s in range(len(seg) - 1):
        acc = 1
        for t in range(seg[s], seg[s + 1]):
            acc = acc * rows[t] % N
            want.append(acc)
    out = torch.empty((total, cw), dtype=torch.int32, device="cuda")
    pl.scan_segments_dev(_dev(rows, cw), seg, out)
    pl.dev.sync()
    _diff(_ints(out), want, "scan_segments_dev")


@cases
def test_mont_resident_rows(ck):
    """to_mont -> add_mont -> from_mont gives the same rows as add (x y mod N) on the hostile grid"""
    import torch
    pl, kind, E = ck
    N, cw = pl.n2, 2 * pl.n_words
    a, b = _grid(E)
    a, b = a[:NH * NH + 64], b[:NH * NH + 64]
    ad, bd = _dev(a, cw), _dev(b, cw)
    am, bm, om, out = (torch.empty_like(ad) for _ in range(4))
    pl.to_mont_dev(ad, am)
    pl.to_mont_dev(bd, bm)
    pl.add_mont_dev(am, bm, om)
    pl.from_mont_dev(om, out)
    pl.dev.sync()
    _diff(_ints(out), [x * y % N for x, y in zip(a, b)], "mont rows")


@pytest.mark.parametrize("ck", [c for c in CASES if c[1] == "default"],
                         ids=[i for i, c in zip(IDS, CASES) if c[1] == "default"], indirect=True)
def test_edge_keys_are_working_keys(ck):
    """encrypt a few u64s and decrypt their add, sub and 3-way merge: keys, not just moduli"""
    pl, kind, E = ck
    m = np.array([[5, 2**40 + 7, 2**62], [3, 11, 2**61 + 1], [1, 2**33, 12345]], dtype=np.uint64)
    c = [pl.encrypt_u64(mi, seed=7 + i) for i, mi in enumerate(m)]
    assert np.array_equal(pl.decrypt_u64(c[0]), m[0])
    assert np.array_equal(pl.decrypt_u64(pl.add_batch(c[0], c[1])), m[0] + m[1])
    assert np.array_equal(pl.decrypt_u64(pl.sub_batch(c[0], c[1])), m[0] - m[1])
    assert np.array_equal(pl.decrypt_u64(pl.reduce_kway(np.stack(c))), m[0] + m[1] + m[2])
