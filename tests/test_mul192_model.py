"""The Paillier-3072 product (fthe_mul192, fedtree_amd/csrc/fthe_mul192.hip) without a GPU: tools/mul192_model.py,
the bit-exact model of its arithmetic (the octet's ring of columns, the Barrett cut points, the quotient error, the
final range), against Python's x y mod N at the edges of the modulus range, and the host builder of the per-key
context (mul192_image.hpp through fthe_debug_mul192_image) byte for byte against the model's."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mul192_model as mm  # noqa: E402
import n2_edges as ne  # noqa: E402

MODULI = mm.edge_moduli()


@pytest.mark.parametrize("ni", range(len(MODULI)))
def test_model_reduces_exactly(ni):
    """every ordered pair of the hostile rows (mul() asserts each bound and the result); the pairs on the diagonal
    and with the all-ones row also lane by lane through the ring of columns"""
    n = MODULI[ni]
    H = ne.hostile_rows(n * n, bits=6144)
    top = (1 << 6144) - 1
    for x in H:
        for y in H:
            mm.mul(x, y, n, lanes=x == y or top in (x, y))


def test_model_refuses_other_sizes():
    for n in ((1 << 3040) - 1, (1 << 3072) + 1, 1 << 3071):
        assert not mm.n_ok(n)


def _image(n):
    lib = ctypes.CDLL(os.path.join(ROOT, "fedtree_amd", "libfthe.so"))
    nw = np.frombuffer(n.to_bytes(4 * 97, "little"), dtype=np.uint32).copy()
    words = (n.bit_length() + 31) // 32
    ln = ctypes.c_size_t()
    rc = lib.fthe_debug_mul192_image(ctypes.c_void_p(nw.ctypes.data), words, None, ctypes.c_size_t(0), ctypes.byref(ln))
    if rc:
        return rc
    buf = np.zeros(ln.value, np.uint8)
    assert lib.fthe_debug_mul192_image(ctypes.c_void_p(nw.ctypes.data), words, ctypes.c_void_p(buf.ctypes.data),
                                       ctypes.c_size_t(buf.size), ctypes.byref(ln)) == 0
    return bytes(buf)


@pytest.mark.parametrize("ni", [1, 5])
def test_host_context_matches_model(ni):
    assert _image(MODULI[ni]) == mm.image(MODULI[ni])


def test_host_context_refuses_other_sizes():
    for n in ((1 << 3040) - 1, (1 << 3072) + 1, (1 << 3071) + 2):
        assert _image(n) == -4                                      # FTHE_ERR_UNSUPPORTED
