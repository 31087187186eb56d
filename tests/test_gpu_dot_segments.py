"""Weighted segment sums under encryption on the device (include/fthe.h fthe_dot_segments).

Every comparison is exact: the rows of the three forms (composed, 4- and 8-bit buckets) against each other and
against Python's prod pow(x_t, e_t, n^2), at every product path (the keys of tests/test_gpu_sub_inv.py), and the
decrypted plaintexts against sum k_t m_t mod n.

Products of the 300-member segment with 64-bit weights, as tools/dot_model.py counts them and as the engine
accounts for them at the 2,048-bit key: 27,008 composed, 6,334 with 4-bit buckets, 8,446 with 8-bit buckets."""
import math

import numpy as np
import pytest

import pyoracle
from conftest import GOLDEN_KEYS, golden_key, load_golden
from dot_cases import DOT_CASES, dot_case, exp_words, forced_env, rand_rows, want_dot
from n2_edges import load_keys
from sub_inv_cases import key_2041

import dot_model
from fedtree_amd import _lib

pytestmark = pytest.mark.gpu

KEY_512, KEY_1023, KEY_2048 = GOLDEN_KEYS
ALL_KEYS = GOLDEN_KEYS + ["n2041", "cls_hi"]
X_ROWS = 40
FORMS = (0, 4, 8)
# weights of 20, 64 and 96 bits on the call with every segment size; 64 elsewhere
CASE_BITS = {"mixed": (20, 64, 96), "identity": (64,), "zeros": (20,), "digits": (20, 64), "big": (64,)}


@pytest.fixture(scope="module")
def dev():
    from fedtree_amd.paillier import Device
    return Device(0)


@pytest.fixture(scope="module")
def keys(dev):
    """name -> (Paillier, p): made on first use."""
    from fedtree_amd.paillier import Paillier
    made = {}

    def get(name):
        if name not in made:
            if name == "n2041":
                p, q = key_2041()
            elif name in GOLDEN_KEYS:
                p, q = golden_key(load_golden(name))
            else:
                p, q = load_keys()[name]
            made[name] = (Paillier.from_primes(p, q, dev), p)
        return made[name]
    return get


def _t(a, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()


def _np(t):
    return t.cpu().numpy().view(np.uint32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _dev_call(pl, dev, xd, es, seg, idx):
    """The _dev form on device copies of everything: (rows, last_montmuls)."""
    import torch
    ew = max(1, (max(e.bit_length() for e in es) + 31) // 32)
    ed = _t(exp_words(es, ew))
    segd = _t(np.array(seg, dtype=np.int64), np.int64)
    idxd = None if idx is None else _t(np.array(idx, dtype=np.int64), np.int64)
    out = torch.full((len(seg) - 1, xd.shape[1]), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    pl.dot_segments_dev(xd, ed, segd, out, idxd)
    dev.sync()
    return _np(out), dev.last_montmuls()


@pytest.mark.parametrize("name", ALL_KEYS)
@pytest.mark.parametrize("case", DOT_CASES)
def test_forms_equal_python(dev, keys, name, case):
    pl, _ = keys(name)
    n, cw = pl.modulus, 2 * pl.n_words
    xs = rand_rows(n, X_ROWS, 11)
    xw = pyoracle.ints_to_words(xs, cw)
    xd = _t(xw)
    for bits in CASE_BITS[case]:
        seg, idx, es = dot_case(case, bits, X_ROWS, 3)
        want = want_dot(n, xs, es, seg, idx)
        top, nseg = max(e.bit_length() for e in es), len(seg) - 1
        rows, mm = {}, {}
        for w in FORMS:
            with forced_env(FTHE_DOT_WINDOW=w, FTHE_DOT_SEG_CHUNK=None):
                host = pl.dot_segments(xw, es, seg, idx)
                assert pyoracle.words_to_ints(host) == want, (bits, w)
                rows[w], mm[w] = _dev_call(pl, dev, xd, es, seg, idx)
                assert _same(rows[w], host), (bits, w)
        print(name, case, bits, "products by form:", mm)
        assert _same(_np(xd), xw)                            # the rows are read only
        # unforced, the call takes the form the model names
        with forced_env(FTHE_DOT_WINDOW=None, FTHE_DOT_SEG_CHUNK=None):
            plan = pl.dot_plan(top, seg[-1], nseg)
            assert plan == dot_model.dot_plan(top, seg[-1], nseg)
            got, products = _dev_call(pl, dev, xd, es, seg, idx)
            assert _same(got, rows[0]) and products == mm[plan], (bits, plan)
        if name == KEY_2048:
            # where every product is one matrix-core add, the call's count is the model's closed form
            assert mm[0] == dot_model.composed_products(es, seg), bits
            for w in (4, 8):
                assert mm[w] == dot_model.bucket_products(dot_model.bucket_sizes(es, seg, w), nseg, top, w), (bits, w)


@pytest.mark.parametrize("name", [KEY_2048, KEY_512])
def test_the_big_segment_prefers_buckets(dev, keys, name):
    """300 members in one segment, 64-bit weights: fewer products with 8-bit buckets than composed."""
    pl, _ = keys(name)
    n, cw = pl.modulus, 2 * pl.n_words
    xd = _t(pyoracle.ints_to_words(rand_rows(n, X_ROWS, 11), cw))
    seg, idx, es = dot_case("big", 64, X_ROWS, 3)
    mm = {}
    for w in FORMS:
        with forced_env(FTHE_DOT_WINDOW=w, FTHE_DOT_SEG_CHUNK=None):
            mm[w] = _dev_call(pl, dev, xd, es, seg, idx)[1]
    print(name, "big: products by form:", mm)
    assert mm[8] < mm[0], mm


@pytest.mark.parametrize("name", [KEY_2048, KEY_512, "cls_hi"])
def test_segment_chunks(dev, keys, name):
    """FTHE_DOT_SEG_CHUNK=2: the seven segments in four chunks, both bucket widths, the same rows."""
    pl, _ = keys(name)
    n, cw = pl.modulus, 2 * pl.n_words
    xs = rand_rows(n, X_ROWS, 11)
    xd = _t(pyoracle.ints_to_words(xs, cw))
    seg, idx, es = dot_case("mixed", 20, X_ROWS, 3)
    want = want_dot(n, xs, es, seg, idx)
    for w in (4, 8):
        with forced_env(FTHE_DOT_WINDOW=w, FTHE_DOT_SEG_CHUNK=2):
            assert pyoracle.words_to_ints(_dev_call(pl, dev, xd, es, seg, idx)[0]) == want, w


def test_arguments(dev, keys):
    import torch
    pl, _ = keys(KEY_512)
    n, cw = pl.modulus, 2 * pl.n_words
    xs = rand_rows(n, 8, 1)
    xw = pyoracle.ints_to_words(xs, cw)
    # no segment, no term, and weights that are all zero
    assert pl.dot_segments(xw, [], [0]).shape == (0, cw)
    assert pyoracle.words_to_ints(pl.dot_segments(xw, [], [0, 0, 0])) == [1, 1]
    assert pyoracle.words_to_ints(pl.dot_segments(xw, [0] * 8, [0, 3, 8])) == [1, 1]
    assert dev.last_montmuls() == 0
    # an index outside x, more terms than rows without idx, exponent widths outside 1 .. n_words
    with pytest.raises(_lib.FtheError) as err:
        pl.dot_segments(xw, [1, 2], [0, 2], idx=[0, 8])
    assert err.value.status == _lib.FTHE_ERR_ARG
    with pytest.raises(_lib.FtheError):
        pl.dot_segments(xw, [1] * 9, [0, 9])
    seg = np.array([0, 2], dtype=np.int64)
    out = np.zeros((1, cw), np.uint32)
    for words in (0, pl.n_words + 1):
        e = np.ones((2, max(words, 1)), np.uint32)
        assert pl.lib.fthe_dot_segments(pl._key, dev.ctx, xw.ctypes.data, 8, e.ctypes.data, words, seg.ctypes.data,
                                        None, 1, out.ctypes.data) == _lib.FTHE_ERR_ARG
        xd, ed, sd = _t(xw), _t(e), _t(seg, np.int64)
        od = torch.zeros((1, cw), dtype=torch.int32, device="cuda")
        assert pl.lib.fthe_dot_segments_dev(pl._key, dev.ctx, xd.data_ptr(), 8, ed.data_ptr(), words, sd.data_ptr(),
                                            None, 1, od.data_ptr()) == _lib.FTHE_ERR_ARG
    with pytest.raises(ValueError):
        pl.dot_segments(xw, [1, 2, 3], [0, 2])


@pytest.mark.parametrize("name", [KEY_2048, KEY_512])
def test_plaintexts(dev, keys, name):
    """Encrypt 40 u64 plaintexts and take weighted sums: the full decrypt is sum k m mod n; with signed weights
    and offset 2^128 it is sum k m + 2^128; a negative weight on a row that is a multiple of p raises."""
    from fedtree_amd.paillier import Paillier
    pl, p = keys(name)
    n, n2, cw = pl.modulus, pl.n2, 2 * pl.n_words
    rng = np.random.default_rng(6)
    m = rng.integers(0, 2**63, 40, dtype=np.uint64)
    m[:3] = (0, 1, 2**64 - 1)
    c = pl.encrypt_u64(m, seed=9)
    seg, idx = [0, 0, 1, 9, 40], [int(v) for v in rng.permutation(40)]
    ks = [int(v) for v in rng.integers(0, 2**62, 40)]
    ks[5] = 0

    def full(rows):
        return pyoracle.words_to_ints(pl.decrypt_u64(rows, full=True)[1])

    def sums(weights):
        return [sum(weights[t] * int(m[idx[t]]) for t in range(seg[s], seg[s + 1])) for s in range(4)]

    pub = Paillier.from_public(n, dev)                       # no private key is needed
    for form in FORMS:
        with forced_env(FTHE_DOT_WINDOW=form):
            got = pub.dot_segments(c, ks, seg, idx)
            assert full(got) == [v % n for v in sums(ks)], form
    # signed weights: the positive and the negative part, joined by one batched inverse
    signed = [k >> 24 if t % 3 else -(k >> 24) for t, k in enumerate(ks)]      # |sum| < 2^110: the offset covers it
    offset = 1 << 128
    assert all(v + offset >= 0 for v in sums(signed))
    got = pub.dot_segments(c, np.array(signed, dtype=np.int64), seg, idx, offset=offset)
    assert full(got) == [v + offset for v in sums(signed)]
    assert full(pub.dot_segments(c, ks, seg, idx, offset=offset)) == [v + offset for v in sums(ks)]
    # a negative weight on a multiple of p: no unit, the whole call fails
    bad = pyoracle.words_to_ints(c)
    bad[idx[3]] = p * bad[idx[3]] % n2                        # a member of segment 2
    assert math.gcd(bad[idx[3]], n) == p
    bw = pyoracle.ints_to_words(bad, cw)
    weights = list(ks)
    weights[3] = -5
    with pytest.raises(_lib.FtheError) as err:
        pub.dot_segments(bw, weights, seg, idx)
    assert err.value.status == _lib.FTHE_ERR_ARG
    weights[3] = 5                                           # unsigned, the same row goes through
    assert pyoracle.words_to_ints(pub.dot_segments(bw, weights, seg, idx)) == want_dot(n, bad, weights, seg, idx)
