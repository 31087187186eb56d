"""The C ABI of the per-row weights (include/fthe.h fthe_scalar_mul_rows / fthe_dot_segments), no device: the
symbols, the form model against tools/dot_model.py, and the argument errors."""
import ctypes

from dot_cases import HERE  # noqa: F401  (puts tools/ on the path)

import dot_model
from fedtree_amd import _lib

NEW_SYMBOLS = ("fthe_scalar_mul_rows_dev", "fthe_scalar_mul_rows", "fthe_dot_segments_dev", "fthe_dot_segments",
               "fthe_debug_dot_plan")


def test_symbols_resolve():
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib._PROTOS and s in _lib.header_symbols(), s


def test_plan_agrees_with_the_model():
    lib = _lib.load()
    w = ctypes.c_int(-1)
    seen = set()
    for bits in (8, 20, 64, 192):
        for terms in (0, 1, 8, 300, 4096, 10**5, 10**6, 10**7):
            for nseg in (1, 7, 28, 1000, 125000, 10**6):
                assert lib.fthe_debug_dot_plan(bits, terms, nseg, ctypes.byref(w)) == _lib.FTHE_OK
                assert w.value == dot_model.dot_plan(bits, terms, nseg), (bits, terms, nseg)
                seen.add(w.value)
    assert seen == {0, 4, 8}                                 # the grid reaches every form
    assert lib.fthe_debug_dot_plan(0, 10**6, 28, ctypes.byref(w)) == _lib.FTHE_OK and w.value == 0
    assert lib.fthe_debug_dot_plan(64, 10**6, 28, None) == _lib.FTHE_ERR_ARG
    assert lib.fthe_debug_dot_plan(-1, 10**6, 28, ctypes.byref(w)) == _lib.FTHE_ERR_ARG


def test_argument_errors_need_no_device():
    lib = _lib.load()
    buf = (ctypes.c_uint32 * 8)()
    seg = (ctypes.c_int64 * 2)(0, 0)
    p, s = ctypes.addressof(buf), ctypes.addressof(seg)
    for e_words in (0, -1, 1, 1 << 20):                      # a null key, whatever the words
        for fn in (lib.fthe_scalar_mul_rows, lib.fthe_scalar_mul_rows_dev):
            assert fn(None, None, p, p, e_words, 1, p) == _lib.FTHE_ERR_ARG
            assert fn(None, None, None, None, e_words, 0, None) == _lib.FTHE_ERR_ARG
        for fn in (lib.fthe_dot_segments, lib.fthe_dot_segments_dev):
            assert fn(None, None, p, 1, p, e_words, s, None, 1, p) == _lib.FTHE_ERR_ARG
            assert fn(None, None, None, 0, None, e_words, None, None, 0, None) == _lib.FTHE_ERR_ARG
