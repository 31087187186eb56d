"""Error behaviour of the C ABI on a live context (the reference aborts through
CHECK / exit(1), common.h:47-52, paillier_gpu.cu:13-16; the engine returns status
codes and leaves the context usable).  Each failing call is followed by a good one."""
import ctypes

import numpy as np
import pytest

from fedtree_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    pl = Paillier(dev).keygen(1024, seed=3)
    pub = Paillier.from_public(pl.modulus, dev)
    return dev, pl, pub


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def test_bad_arguments_return_codes(env):
    dev, pl, pub = env
    lib, ctx, key = dev.lib, dev.ctx, pl._key
    cw = 2 * pl.n_words
    m = np.arange(8, dtype=np.uint64)
    c = np.zeros((8, cw), np.uint32)
    r = np.ones((8, pl.n_words + 1), np.uint32)
    E = _lib
    # r wider than n
    assert lib.fthe_encrypt_u64(key, ctx, _p(m), 8, _p(r), pl.n_words + 1, 0, _p(c), 0) == E.FTHE_ERR_ARG
    # null output with a count
    assert lib.fthe_encrypt_u64(key, ctx, _p(m), 8, None, 0, 0, None, 0) == E.FTHE_ERR_ARG
    # private operations on a public-only key
    low = np.zeros(8, np.uint64)
    assert lib.fthe_decrypt(pub._key, ctx, _p(c), 8, _p(low), None) == E.FTHE_ERR_NOPRIV
    assert lib.fthe_encrypt_u64(pub._key, ctx, _p(m), 8, None, 0, 0, _p(c), E.FTHE_ENC_FIXED_BASE_EXACT) \
        == E.FTHE_ERR_NOPRIV
    assert lib.fthe_key_fixed_base_exact(pub._key, ctx, 1) == E.FTHE_ERR_NOPRIV
    # k-way with k out of range
    x = np.zeros((65, 1, cw), np.uint32)
    assert lib.fthe_reduce_kway(key, ctx, _p(x), 65, 1, _p(c)) == E.FTHE_ERR_ARG
    assert lib.fthe_reduce_kway(key, ctx, _p(x), 0, 1, _p(c)) == E.FTHE_ERR_ARG
    # invalid key material
    out = ctypes.c_void_p()
    w = np.array([7, 0], np.uint32)
    assert lib.fthe_key_from_primes(ctx, _p(w), _p(w), 2, ctypes.byref(out)) == E.FTHE_ERR_KEY      # p == q
    ev = np.array([8, 0], np.uint32)
    assert lib.fthe_key_from_primes(ctx, _p(ev), _p(w), 2, ctypes.byref(out)) == E.FTHE_ERR_KEY     # even p
    assert lib.fthe_key_generate(ctx, 1023, 0, ctypes.byref(out)) == E.FTHE_ERR_ARG                 # odd bits
    assert lib.fthe_strerror(E.FTHE_ERR_NOPRIV)
    # the context still works
    got = pl.encrypt_u64(m, seed=1)
    assert np.array_equal(pl.decrypt_u64(got), m)
    assert np.array_equal(pl.decrypt_u64(pub.encrypt_u64(m, seed=2)), m)


def test_zero_counts_are_no_ops(env):
    dev, pl, pub = env
    cw = 2 * pl.n_words
    e = np.zeros((0, cw), np.uint32)
    assert pl.encrypt_u64(np.zeros(0, np.uint64)).shape == (0, cw)
    assert pl.decrypt_u64(e).shape == (0,)
    assert pl.add_batch(e, e).shape == (0, cw)
    assert pl.encrypt_u64(np.zeros(0, np.uint64), fixed_base_exact=True).shape == (0, cw)
    m = np.arange(3, dtype=np.uint64)
    assert np.array_equal(pl.decrypt_u64(pl.encrypt_u64(m, seed=4)), m)


def _hook_rejections(call, ok_prog, bad_op_list, extra_ops):
    """what both op-program hooks refuse before anything is launched: ops outside their list (the table ops 14-17
    among them, which address memory by lane data), slots at or above nslots, SQR counts outside 1..64, a program
    without an END inside prog_words, null pointers, bad slots and counts"""
    E = _lib.FTHE_ERR_ARG
    assert call(ok_prog) == 0
    for op in bad_op_list:
        assert call([1, 0, op, 0, 2, 1, 0, 0]) == E, op
    assert call([1, 2, 2, 1, 0, 0]) == E and call([1, 0, 2, 2, 0, 0]) == E and call([1, 0, 4, 2, 2, 1, 0, 0]) == E
    assert call([1, 0xFFFFFFFF, 2, 1, 0, 0]) == E
    assert call([1, 0, 3, 0, 2, 1, 0, 0]) == E and call([1, 0, 3, 65, 2, 1, 0, 0]) == E
    assert call([1, 0, 3, 64, 2, 1, 0, 0]) == 0
    assert call([1, 0, 2, 1]) == E and call([1, 0, 2, 1, 0]) == E and call([1, 0, 2, 1, 3]) == E
    assert call([1, 0, 2, 1, 0, 0], out_slot=2) == E and call([1, 0, 2, 1, 0, 0], out_slot=-1) == E
    assert call([1, 0, 2, 1, 0, 0], count=0) == E and call([1, 0, 2, 1, 0, 0], nslots=17) == E
    assert call([1, 0, 2, 1, 0, 0], nslots=0) == E
    assert call(None) == E and call([1, 0, 2, 1, 0, 0], slots=None) == E and call([1, 0, 2, 1, 0, 0], out=None) == E
    for op in extra_ops:
        assert call([1, 0, op, 0, 2, 1, 0, 0]) == 0, op
    assert call(ok_prog) == 0                                    # the context still works


def test_debug_prog_hooks_validate_their_programs(env):
    from fedtree_amd.paillier import Paillier
    dev, pl, pub = env
    lib, ctx = dev.lib, dev.ctx
    big = Paillier(dev).keygen(2048, seed=5)
    E = _lib

    def caller(fn, key, S, *lead):
        def call(words, nslots=2, out_slot=1, count=4, slots=0, out=0):
            w = np.array(words, dtype=np.uint32) if words is not None else None
            sl = np.zeros((max(nslots, 1), 4, S), np.uint32) if slots == 0 else None
            o = np.zeros((4, S), np.uint32) if out == 0 else None
            return fn(key, ctx, *lead, _p(w), len(w) if w is not None else 6, _p(sl), nslots, count, out_slot, _p(o))
        return call
    other = [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 21, 24, 0x80000001]
    for side in (0, 1):
        _hook_rejections(caller(lib.fthe_debug_padic_prog, big._key, 74, side), [22, 0, 23, 1, 0, 0], other + [20], [])
    assert caller(lib.fthe_debug_padic_prog, big._key, 74, 2)([1, 0, 2, 1, 0, 0]) == E.FTHE_ERR_ARG       # side
    assert caller(lib.fthe_debug_padic_prog, big._key, 74, 0)([22, 2, 23, 1, 0, 0]) == E.FTHE_ERR_ARG
    assert caller(lib.fthe_debug_padic_prog, big._key, 74, 0)([22, 0, 23, 2, 0, 0]) == E.FTHE_ERR_ARG
    _hook_rejections(caller(lib.fthe_debug_nadicb_prog, big._key, 152), [1, 0, 20, 0, 2, 1, 0, 0], other + [22, 23], [20])
    ok = [1, 0, 2, 1, 0, 0]
    # a public key has no P-adic contexts; Paillier-1024 runs the K = 19 kernel, and its n is no b76 modulus
    assert caller(lib.fthe_debug_padic_prog, big.public()._key, 74, 0)(ok) == E.FTHE_ERR_NOPRIV
    assert caller(lib.fthe_debug_padic_prog, pub._key, 74, 0)(ok) == E.FTHE_ERR_NOPRIV
    assert caller(lib.fthe_debug_padic_prog, pl._key, 74, 0)(ok) == E.FTHE_ERR_UNSUPPORTED
    assert caller(lib.fthe_debug_nadicb_prog, pl._key, 152)(ok) == E.FTHE_ERR_UNSUPPORTED
    assert caller(lib.fthe_debug_padic_prog, None, 74, 0)(ok) == E.FTHE_ERR_ARG
    assert caller(lib.fthe_debug_nadicb_prog, None, 152)(ok) == E.FTHE_ERR_ARG
    m = np.arange(8, dtype=np.uint64)
    assert np.array_equal(big.decrypt_u64(big.encrypt_u64(m, seed=1)), m)
