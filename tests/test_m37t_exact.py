"""Exactness of fthe_padic_m37t's four-tile product 2 on hostile inputs, on the CPU: the model
(tools/padic_mfma_model.py barrett_top: both forms of the reduction against the five-tile product 2, the distance
between r and the estimate within [0, 128] of the 256 units between candidates, r = T - q3 P, r < P + 2^1015) and
one wave of the generated kernel on the emulator (tools/wave_emu.py).

Inputs: T = q P + r for r in {0, 1, 2^1016 - 1, 2^1016, k 2^1016 - 1, k 2^1016 (k up to P >> 1016), P - 1} and q in
{0, 1, P, the largest within the contract}; the largest e (limbs 0..35 all ones, or all 2 (2^28 - 1) as the second
reduction's unnormalised limbs allow, under the largest q1 of the contract); digits 2P - 1 and 3P - 1 (the contract's
bound); the small q1 whose numerators go negative (the clamp), at the largest admitted P.  P of 1009 bits (incl. 2^1008
+ 1, where a digit leaves above 2P), 1024 bits and 1027 bits (incl. the largest, 2^1027 - 1).  A P of 1028 bits trips
the model's assert, and its window bound exceeds the 128 units."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fedtree_amd", "csrc"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import padic_model as pm  # noqa: E402
import padic_mfma_model as mm  # noqa: E402

K, B, MASK = mm.K, mm.B, mm.MASK
BK1 = 1 << (B * (K - 1))
L = mm.TOPEST_MAX_BITS
PS = {
    "1009-min": (1 << 1008) + 1,
    "1009": random.Random(1009).getrandbits(1009) | (1 << 1008) | 1,
    "1024": random.Random(1024).getrandbits(1024) | (1 << 1023) | 1,
    "L": random.Random(L).getrandbits(L) | (1 << (L - 1)) | 1,
    "L-max": (1 << L) - 1,
}


@pytest.fixture(autouse=True)
def top_barrett():
    saved = pm.barrett
    mm.install_top()
    yield
    pm.barrett = saved


@pytest.fixture(scope="module")
def keys():
    out = {}
    for name, P in PS.items():
        out[name] = mm.MfmaKey(P)
        assert mm.topest_check_key(P) <= mm.TOPEST_C // 3            # 42.1 units a priori, a third of the 128
    return out


def _reduce(key, T):
    """one Barrett through barrett_top (which asserts the four-tile forms, the window and r's bound)"""
    if isinstance(T, int):
        T = pm.limbs(T, 2 * K)
    q3, r, cl = mm.barrett_top(key, T)
    assert pm.value(q3) * key.P + pm.value(r) == pm.value(T)
    return pm.value(q3), pm.value(r), cl


@pytest.mark.parametrize("name", list(PS))
def test_remainders_at_the_tile_boundary(keys, name):
    key = keys[name]
    P = key.P
    tmax = mm.topest_t_max(P)
    top = P >> 1016
    ks = sorted({k for k in (1, 2, 3, top // 2, top - 1, top) if k >= 1 and (k << 1016) < P})
    rs = [0, 1, (1 << 1016) - 1, 1 << 1016, P - 1] + [(k << 1016) - 1 for k in ks] + [k << 1016 for k in ks]
    for r in (x for x in rs if 0 <= x < P):
        for q in (0, 1, P, (tmax - r) // P):
            q3, got, _ = _reduce(key, q * P + r)
            assert got % P == r and got - r in (0, P, 2 * P) and q3 + (got - r) // P == q


@pytest.mark.parametrize("name", list(PS))
def test_largest_error_and_contract_digits(keys, name):
    key = keys[name]
    P = key.P
    tmax = mm.topest_t_max(P)
    q1 = (tmax >> (B * (K - 1))) - 2
    mm.SLACK["d_max"] = 0
    _reduce(key, q1 * BK1 + BK1 - 1)                                 # limbs 0..35 all ones under the largest q1
    T = [2 * MASK] * (K - 1) + pm.limbs(q1, K + 1)                   # the second reduction's unnormalised limbs
    assert pm.value(T) <= tmax
    mm.barrett_top(key, T)
    d0 = mm.SLACK["d_max"]
    assert 0 < d0 <= mm.topest_window(P) <= mm.TOPEST_C
    for dv in (2 * P - 1, 3 * P - 1, P - 1):
        x = pm.limbs(dv, K)
        z0, z1 = pm.sqr(key, x, x)
        X = dv + dv * P
        assert (pm.value(z0) + pm.value(z1) * P) % (P * P) == X * X % (P * P)
        assert max(pm.value(z0), pm.value(z1)) < min(P + (1 << 1015), 3 * P)
        y0, y1 = pm.mul(key, z0, z1, x, x)
        assert (pm.value(y0) + pm.value(y1) * P) % (P * P) == X ** 3 % (P * P)
        assert max(pm.value(y0), pm.value(y1)) < min(P + (1 << 1015), 3 * P)


def test_clamp_inputs_at_the_largest_p(keys):
    """the inputs of test_small_q1_goes_negative_at_1030_bits at the largest admitted P: where the numerator goes
    negative the first reduction clamps (r = T < 2^1016, h = 0 under the mask) and the second gives r = T + P"""
    key = keys["L-max"]
    clamped = {}
    for q1 in (0, 1, 2, 15, 16, 17):
        for low in (0, 1, BK1 - 1):
            q3, r, cl = _reduce(key, q1 * BK1 + low)
            clamped[q1, low] = cl
            if cl:
                assert q3 == 0 and r == q1 * BK1 + low < (1 << 1016)
    assert all(clamped[0, low] for low in (0, 1, BK1 - 1)) and clamped[1, 0]    # mu < 2^1046 at 1027 bits
    assert not any(clamped[17, low] for low in (0, 1, BK1 - 1))


def test_wider_p_trips_the_model():
    P = (1 << L) + 1                                                 # the smallest P of L + 1 bits
    key = mm.MfmaKey(P)
    with pytest.raises(AssertionError, match="wider than the admitted size"):
        mm.barrett_top(key, pm.limbs(5 * P + 3, 2 * K))
    assert mm.topest_window((1 << (L + 1)) - 1) > mm.TOPEST_C        # 298 units: the rule itself fails there
    assert 3 * mm.topest_window((1 << L) - 1) <= mm.TOPEST_C


@pytest.mark.parametrize("name", ["1009-min", "L-max"])
def test_wave_emulation(name):
    import wave_emu
    P = PS[name]
    bits = P.bit_length()
    extra = [q * BK1 + j for q in (1, 2, 15, 16, 17) for j in (0, 12345)] + [P * P - P, (P - 1) * P, (1 << 1016) * P]
    assert wave_emu.m37_selftest(seed=bits, bits=bits, extra=extra, variant="m37t", P=P) == 0
    top = P >> 1016
    hostile = [2 * P - 1, 3 * P - 1, (1 << 1016) - 1, 1 << 1016, (top << 1016) - 1, top << 1016, P - 1, P, P + 1]
    hostile = [x for x in hostile if 0 <= x < 3 * P]
    pairs0 = [(a, b) for a in hostile for b in (hostile[0], hostile[1], hostile[-3])][:24]
    assert wave_emu.m37_digits_selftest(seed=bits, bits=bits, variant="m37t", P=P, pairs0=pairs0) == 0
    assert wave_emu.m37_digits_selftest(seed=bits + 1, bits=bits, variant="m37t") == 0
