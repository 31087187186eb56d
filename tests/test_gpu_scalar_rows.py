"""One plaintext scalar per ciphertext on the device (include/fthe.h fthe_scalar_mul_rows).

Every comparison is exact, against Python's pow(x, e, n^2), at every product path: the matrix-core add with
gathered operands at the 2,048-bit golden key, the four-lane row-I/O programs in their classical and Montgomery
forms at a 2,047-bit edge key and a 2,041-bit key, the slot programs at the 512- and 1,023-bit keys."""
import math

import numpy as np
import pytest

import pyoracle
from conftest import GOLDEN_KEYS, golden_key, load_golden
from dot_cases import exp_words, forced_env, rand_exponents, rand_rows, want_rows
from n2_edges import load_keys
from sub_inv_cases import key_2041

import dot_model
from fedtree_amd import _lib

pytestmark = pytest.mark.gpu

KEY_512, KEY_1023, KEY_2048 = GOLDEN_KEYS
ALL_KEYS = GOLDEN_KEYS + ["n2041", "cls_hi"]
COUNTS = (1, 2, 17, 257)                             # one row, a pair, a 16-row batch plus one, several workgroups


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


def _t(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()


def _np(t):
    return t.cpu().numpy().view(np.uint32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _host(pl, dev, xw, ew_arr):
    """The host form of the C ABI with the exponent words as given."""
    out = np.zeros_like(xw)
    _lib.check(pl.lib.fthe_scalar_mul_rows(pl._key, dev.ctx, xw.ctypes.data, ew_arr.ctypes.data, ew_arr.shape[1],
                                           len(xw), out.ctypes.data), "scalar_mul_rows")
    return out


def _unit(pl, dev, cw):
    """Products one add of this key accounts for: 1 on the matrix-core and classical paths, 2 where a Montgomery
    product needs its R^2 correction."""
    import torch
    a = torch.ones((4, cw), dtype=torch.int32, device="cuda")
    pl.add_dev(a, a, torch.empty_like(a))
    per = dev.last_montmuls() / 4
    assert per in (1, 2)
    return per


@pytest.mark.parametrize("name", ALL_KEYS)
def test_rows_equal_python(dev, keys, name):
    import torch
    pl, _ = keys(name)
    n, cw = pl.modulus, 2 * pl.n_words
    per = _unit(pl, dev, cw)
    assert per == 1 or name not in (KEY_2048, "cls_hi")
    for count in COUNTS:
        for ew in (1, 2, 3):
            xs = rand_rows(n, count, 10 * count + ew)
            es = rand_exponents(count, 32 * ew, count + ew)      # 0, 1, 2, 15, 16, 2^32 - 1, 2^32, 2^64 - 1 as they fit
            if count > 8:
                es[-1] = (1 << (32 * ew)) - 1                    # the widest exponent of the width
            want = want_rows(n, xs, es)
            xw, ewd = pyoracle.ints_to_words(xs, cw), exp_words(es, ew)
            host = _host(pl, dev, xw, ewd)
            assert pyoracle.words_to_ints(host) == want, (count, ew)
            xd, ed = _t(xw), _t(ewd)
            out = torch.zeros_like(xd)
            pl.scalar_mul_rows_dev(xd, ed, out)
            dev.sync()
            assert _same(_np(out), host), (count, ew)
            bits = max(e.bit_length() for e in es)
            assert dev.last_montmuls() == count * dot_model.rows_products(bits) * per, (count, ew, bits)
            assert _same(_np(xd), xw) and _same(_np(ed), ewd), (count, ew)      # the inputs are read only
            pl.scalar_mul_rows_dev(xd, ed, xd)                  # out = x
            dev.sync()
            assert _same(_np(xd), host), (count, ew)
            assert _same(pl.scalar_mul_rows(xw, es), host), (count, ew)         # the Python form picks its own width


@pytest.mark.parametrize("name", ALL_KEYS)
def test_zero_short_and_uniform_exponents(dev, keys, name):
    import torch
    pl, _ = keys(name)
    n, cw = pl.modulus, 2 * pl.n_words
    per = _unit(pl, dev, cw)
    xs = rand_rows(n, 17, 3)
    xw = pyoracle.ints_to_words(xs, cw)
    xd = _t(xw)
    out = torch.full_like(xd, 0x5A5A5A5A)
    # every exponent 0: ones, 0^0 included, and no product
    pl.scalar_mul_rows_dev(xd, _t(exp_words([0] * 17, 2)), out)
    dev.sync()
    assert pyoracle.words_to_ints(_np(out)) == [1] * 17 and dev.last_montmuls() == 0
    # a largest exponent of 5 bits: two windows of the sixteen a 64-bit exponent has
    es = [int(v) for v in np.random.default_rng(5).integers(0, 32, 17)]
    es[4] = 31
    pl.scalar_mul_rows_dev(xd, _t(exp_words(es, 2)), out)
    dev.sync()
    assert pyoracle.words_to_ints(_np(out)) == want_rows(n, xs, es)
    assert dev.last_montmuls() == 17 * 19 * per
    # one exponent for the batch: fthe_scalar_mul_u64's rows
    for k in (2**64 - 1, 12345, 1):
        ew = exp_words([k] * 17, 2)
        assert _same(_host(pl, dev, xw, ew), pl.scalar_mul(xw, k)), k
    # no row at all, and exponent widths outside 1 .. n_words
    assert pl.scalar_mul_rows(xw[:0], []).shape == (0, cw)
    for words in (0, pl.n_words + 1):
        e = np.ones((17, max(words, 1)), np.uint32)
        got = np.zeros_like(xw)
        for fn, xp, ep, op in ((pl.lib.fthe_scalar_mul_rows, xw.ctypes.data, e.ctypes.data, got.ctypes.data),
                               (pl.lib.fthe_scalar_mul_rows_dev, xd.data_ptr(), _t(e).data_ptr(), out.data_ptr())):
            assert fn(pl._key, dev.ctx, xp, ep, words, 17, op) == _lib.FTHE_ERR_ARG
    with pytest.raises(ValueError):
        pl.scalar_mul_rows(xw, [1 << (32 * pl.n_words)] * 17)


def test_exponents_as_wide_as_the_key(dev, keys):
    pl, _ = keys(KEY_512)
    n, cw = pl.modulus, 2 * pl.n_words
    xs = rand_rows(n, 4, 9)[1:]                          # 1, n^2 - 1 and a random row
    es = [n - 1, (1 << 512) - 1, int.from_bytes(np.random.default_rng(2).bytes(64), "little")]
    got = _host(pl, dev, pyoracle.ints_to_words(xs, cw), exp_words(es, pl.n_words))
    assert pl.n_words == 16 and pyoracle.words_to_ints(got) == want_rows(n, xs, es)


@pytest.mark.parametrize("name", [KEY_2048, KEY_512, "cls_hi"])
def test_chunks(dev, keys, name):
    """FTHE_ROWS_CHUNK=16 and 33 rows: three chunks, the last of one row; in place too."""
    pl, _ = keys(name)
    n, cw = pl.modulus, 2 * pl.n_words
    per = _unit(pl, dev, cw)
    xs, es = rand_rows(n, 33, 5), rand_exponents(33, 64, 6)
    xw, ewd = pyoracle.ints_to_words(xs, cw), exp_words(es, 2)
    whole = _host(pl, dev, xw, ewd)
    assert pyoracle.words_to_ints(whole) == want_rows(n, xs, es)
    with forced_env(FTHE_ROWS_CHUNK=16):
        assert _same(_host(pl, dev, xw, ewd), whole)
        xd = _t(xw)
        pl.scalar_mul_rows_dev(xd, _t(ewd), xd)
        dev.sync()
        assert _same(_np(xd), whole)
        assert dev.last_montmuls() == 33 * dot_model.rows_products(64) * per


@pytest.mark.parametrize("name", [KEY_2048, KEY_512])
def test_signed_weights(dev, keys, name):
    """The Python form: a negative weight is the inverse of the row raised to its magnitude; a row that is no unit
    under a negative weight fails the call."""
    pl, p = keys(name)
    n, n2, cw = pl.modulus, pl.n2, 2 * pl.n_words
    xs = [x for x in rand_rows(n, 24, 8)[1:] if math.gcd(x, n) == 1]
    ks = [int(v) for v in np.random.default_rng(4).integers(-2**40, 2**40, len(xs))]
    ks[0], ks[1], ks[2] = -1, 0, -(2**64 - 1)
    got = pl.scalar_mul_rows(pyoracle.ints_to_words(xs[3:], cw), np.array(ks[3:], dtype=np.int64))
    assert pyoracle.words_to_ints(got) == [pow(x, k, n2) for x, k in zip(xs[3:], ks[3:])]
    got = pl.scalar_mul_rows(pyoracle.ints_to_words(xs, cw), ks)
    assert pyoracle.words_to_ints(got) == [pow(x, k, n2) for x, k in zip(xs, ks)]
    bad = list(xs)
    bad[5] = p * xs[5] % n2
    with pytest.raises(_lib.FtheError) as err:
        pl.scalar_mul_rows(pyoracle.ints_to_words(bad, cw), [-3] * len(bad))
    assert err.value.status == _lib.FTHE_ERR_ARG
    assert pyoracle.words_to_ints(pl.scalar_mul_rows(pyoracle.ints_to_words(bad, cw), [3] * len(bad))) == \
        [pow(x, 3, n2) for x in bad]                    # a positive weight takes any row
