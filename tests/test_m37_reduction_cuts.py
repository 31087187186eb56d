"""CPU checks of the round-7 cuts in fthe_padic_m37's reduction (gen_padic_mfma.py):

* the instruction counts of a squaring in the default schedule, pinned;
* the model (tools/padic_mfma_model.py) with product 1's window from column 128 and a 2^1046 bias: every bound
  it asserts (int32 column sums, int64 chunk sums, Pi - 2^1064 < N < Pi, N < 0 only where Barrett's estimate is 0,
  the dword fold equal to the packed limb fold) at the inputs that strain them -- digits 5P - 1, a q1 whose bytes
  are all 0xFF (the largest dropped columns), q1 = 1, 2, 15, 16, 17 at a P of 1030 bits (the numerator goes
  negative for a nonzero q1), T = 0 and T = 1 -- and r < 5P;
* one wave of the generated kernel on the CPU emulator (tools/wave_emu.py) with the default schedule and with each
  switch that restores a part of the previous one."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fedtree_amd", "csrc"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import padic_model as pm  # noqa: E402
import padic_mfma_model as mm  # noqa: E402

K, B = mm.K, mm.B
BK1 = 1 << (B * (K - 1))
PARENT_VALU, PARENT_SWAPS = 4076, 230            # the schedule before these cuts (tests/test_m37_codegen.py)


def _counts(ab=""):
    import gen_padic_mfma as g
    from test_m37_codegen import _sections
    s = _sections(g.gen_body("m37", ab))
    body = s[".Lsqr_loop"] + s[".Lreduce"]
    return (sum(1 for i in body if i.startswith("v_") and "mfma" not in i),
            sum(1 for i in body if i.startswith("v_permlane32_swap")),
            sum(1 for i in body if "v_mfma" in i))


def test_squaring_instruction_counts():
    valu, swaps, mfma = _counts()
    assert mfma == 136
    assert valu <= PARENT_VALU - 100
    assert swaps < PARENT_SWAPS
    assert (valu, swaps) == (3947, 220)
    assert _counts("s1lo112,noq3dw")[:2] == (PARENT_VALU, PARENT_SWAPS)


def _key(bits, s1_lo=mm.S1_LO):
    rng = random.Random(bits)
    if bits == 1030:                             # just below 2^1030: mu just above 2^1042, the smallest there is
        P = (1 << 1030) - (1 << 600) + 1
    else:
        P = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
    key = mm.MfmaKey(P, s1_lo=s1_lo)
    key.check_skipped_tiles()
    return key


@pytest.fixture(autouse=True)
def mfma_barrett():
    saved = pm.barrett
    mm.install()
    yield
    pm.barrett = saved


def _reduce(key, Tv):
    """Barrett of T through the model (it asserts its own bounds); returns (q3, clamped)"""
    T = pm.limbs(Tv, 2 * K)
    q3, r, cl = mm.barrett(key, T)
    assert pm.value(q3) * key.P + pm.value(r) == Tv and pm.value(r) < 5 * key.P
    if cl:                                       # where the kernel does not clamp: q3 = -1 mod b^K, r = T + P
        assert pm.value(q3) == 0 and Tv < key.P
        assert pm.value(mm.product2(key, [mm.MASK] * K, T)) == Tv + key.P
    return pm.value(q3), cl


@pytest.mark.parametrize("s1_lo", [128, 112])
@pytest.mark.parametrize("bits", [1009, 1024, 1030])
def test_model_bounds_at_the_straining_inputs(bits, s1_lo):
    key = _key(bits, s1_lo)
    P = key.P
    assert key.bias_bits == 8 * s1_lo + 22 and (s1_lo != 128 or key.bias_bits == 1046)
    top = 5 * P - 1
    z0, z1 = pm.sqr(key, pm.limbs(top, K), pm.limbs(top, K))           # digits 5P - 1 (both reductions)
    assert (pm.value(z0) + pm.value(z1) * P) % (P * P) == (top + top * P) ** 2 % (P * P)
    pm.check_digit(key, z0)
    pm.check_digit(key, z1)
    # q1 of 0xFF bytes: the largest one whose T stays below 50 P^2 through the whole reduction ...
    qtop = (50 * P * P - 1) // BK1
    q1 = (1 << (8 * ((qtop.bit_length() - 1) // 8))) - 1
    assert q1 <= qtop and q1 >> 1000
    _reduce(key, q1 * BK1 + BK1 - 1)
    _reduce(key, q1 * BK1)
    # ... and all 136 bytes (with the bit 28 of the lowest limb) through product 1's bounds alone
    full = pm.limbs((1 << (B * (K + 1))) - 1, K + 1)
    mm.columns1(key, full)
    mm.columns1(key, [full[0] | (1 << B)] + full[1:])
    assert _reduce(key, 0) == (0, True) and _reduce(key, 1) == (0, True)


def test_small_q1_goes_negative_at_1030_bits():
    key = _key(1030)
    clamped = {}
    for q1 in (1, 2, 15, 16, 17):
        for low in (0, 1, BK1 - 1):
            clamped[q1, low] = _reduce(key, q1 * BK1 + low)[1]
    assert all(clamped[q1, low] for q1 in (1, 2, 15) for low in (0, 1, BK1 - 1))     # 15 mu < 2^1046: N < 0
    assert not any(clamped[17, low] for low in (0, 1, BK1 - 1))                     # 17 mu > 2^1046 + 2^1042: N > 0
    old = _key(1030, 112)                        # the previous window: N < 0 only for q1 = 0
    for q1 in (1, 2, 15, 16, 17):
        assert not mm.barrett(old, pm.limbs(q1 * BK1, 2 * K))[2]
    small = _key(1009)                           # mu ~ 2^1063: no nonzero q1 goes negative
    assert not _reduce(small, BK1)[1]


@pytest.mark.parametrize("ab", [None, "s1lo112", "noq3dw"])
@pytest.mark.parametrize("bits", [1009, 1030])
def test_wave_emulation_default_and_each_switch(bits, ab):
    import wave_emu
    extra = [q * BK1 + j for q in (1, 2, 11, 15, 16, 17) for j in (0, 12345)] if bits == 1030 else ()
    assert wave_emu.m37_selftest(seed=bits, bits=bits, ab=ab, extra=extra) == 0
    assert wave_emu.m37_digits_selftest(seed=bits, bits=bits, ab=ab) == 0
