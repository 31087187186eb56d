"""Shared cases of the per-row-weight tests (include/fthe.h fthe_scalar_mul_rows / fthe_dot_segments):
rows, exponents, segment layouts and the Python references pow(x, e, n^2) and products of it.  Used by
tests/test_dot_model.py, tests/test_gpu_scalar_rows.py and tests/test_gpu_dot_segments.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

EDGE_EXPONENTS = (0, 1, 2, 15, 16, 2**32 - 1, 2**32, 2**64 - 1)
SEGMENT_SIZES = (0, 1, 2, 7, 8, 9, 300)         # the K = 8 group edges, and more members than a window has buckets


def rand_rows(n, count, seed):
    """count rows mod n^2: 0, 1 and n^2 - 1 first, then random ones."""
    rng = np.random.default_rng(seed)
    n2, nb = n * n, (2 * n.bit_length() + 7) // 8 + 8
    out = [0, 1, n2 - 1][:count]
    while len(out) < count:
        out.append(int.from_bytes(rng.bytes(nb), "little") % n2)
    return out


def rand_exponents(count, bits, seed, edges=True):
    """count exponents below 2^bits: the edge values that fit first (when asked), then random ones of every
    length up to bits."""
    rng = np.random.default_rng(seed)
    out = [e for e in EDGE_EXPONENTS if e.bit_length() <= bits][:count] if edges else []
    while len(out) < count:
        out.append(int.from_bytes(rng.bytes((bits + 7) // 8), "little") >> int(rng.integers(0, 8))
                   & ((1 << bits) - 1))
    return out


def exp_words(es, ew):
    return np.frombuffer(b"".join(e.to_bytes(4 * ew, "little") for e in es), dtype=np.uint32).reshape(len(es), ew).copy()


def want_rows(n, xs, es):
    n2 = n * n
    return [pow(x, e, n2) for x, e in zip(xs, es)]


def want_dot(n, xs, es, seg_ptr, idx):
    n2 = n * n
    out = []
    for s in range(len(seg_ptr) - 1):
        acc = 1
        for t in range(seg_ptr[s], seg_ptr[s + 1]):
            acc = acc * pow(xs[idx[t] if idx is not None else t], es[t], n2) % n2
        out.append(acc)
    return out


def seg_ptr_of(sizes):
    seg = [0]
    for s in sizes:
        seg.append(seg[-1] + s)
    return seg


def dot_case(name, bits, x_rows, seed):
    """(seg_ptr, idx, exponents) of a named case over x_rows rows with weights below 2^bits.
    mixed      segments of SEGMENT_SIZES members, idx with repeats
    identity   the same sizes without the 300, idx = None
    zeros      three segments; the middle one's weights are all 0
    digits     one segment whose weights hit every digit 1 .. 15 of window 0, and the digit 255, beside a
               second random one
    big        one segment of 300 members (more members than an 8-bit window has buckets)"""
    rng = np.random.default_rng(seed)
    if name == "mixed":
        sizes = SEGMENT_SIZES
    elif name == "identity":
        sizes = SEGMENT_SIZES[:-1]
    elif name == "zeros":
        sizes = (3, 5, 2)
    elif name == "digits":
        sizes = (17, 4)
    elif name == "big":
        sizes = (300,)
    else:
        raise KeyError(name)
    seg = seg_ptr_of(sizes)
    terms = seg[-1]
    idx = None if name == "identity" else [int(v) for v in rng.integers(0, x_rows, terms)]
    if idx is not None and terms >= 4:
        idx[1] = idx[0]                                  # a repeated row inside a segment
        idx[-1] = idx[0]                                 # and across segments
    es = rand_exponents(terms, bits, seed + 1, edges=name in ("mixed", "identity"))
    if name == "zeros":
        es[3:8] = [0] * 5
    if name == "digits":
        es[:15] = list(range(1, 16))
        es[15] = 255
        es[16] = 255 << 8 if bits >= 16 else 255
    assert terms <= x_rows or idx is not None
    return seg, idx, es


DOT_CASES = ("mixed", "identity", "zeros", "digits", "big")


class forced_env:
    """Set environment switches the engine reads per call (FTHE_ROWS_CHUNK, FTHE_DOT_WINDOW, FTHE_DOT_SEG_CHUNK) for a
    with-block; None removes one.  os.environ reaches the C library's getenv."""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False
