"""CPU checks of the shifted product-1 operand of fthe_padic_m37s (gen_padic_mfma.py q1_shift): with
q1's byte i fed at digit index i + 8 the matrix is A1'[s][i + 8] = A1[s][i], so

* the four sub-diagonal tiles (m - k = 1) hold only mu' digits from index 137 on and are zero for every admitted
  modulus (mu < 2^1064 ends at balanced digit 133), while a shift of 4 leaves digit 133 in them at 1009 bits;
* every column sum over the 15 tiles left equals the one over the 19 tiles of the unshifted layout, whatever the
  operand's pad dwords hold (their A columns are zero);
* both forms of the reduction (limb fold with clamp, dword fold) give the same quotients and remainders;
* the host's image (padic_tiles::build(P, 128, 8)) is the model's, byte for byte."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import padic_model as pm  # noqa: E402
import padic_mfma_model as mm  # noqa: E402
from test_padic_mfma_model import STRUCTURED  # noqa: E402

K, B = mm.K, mm.B
MASK = (1 << B) - 1
BITS = (1009, 1010, 1016, 1024, 1027, 1030)
JUST_ABOVE = (1 << 1008) + 3                     # mu just below 2^1064: its balanced digits reach index 133
P_WIDE = (1 << 1030) - (1 << 600) + 1            # mu ~ 2^1042: small q1 > 0 gives a negative numerator


def _random_p(bits):
    rng = random.Random(bits)
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


KEYS = [(f"{b} bits", _random_p(b)) for b in BITS] + \
       [(f"structured {i}", P) for i, P in enumerate(STRUCTURED)] + [("just above 2^1008", JUST_ABOVE)]


def _top_digit(key):
    return max(i for i, d in enumerate(key.mu_d) if d)


@pytest.mark.parametrize("P", [P for _, P in KEYS], ids=[n for n, _ in KEYS])
def test_tiles_outside_the_15_are_zero(P):
    key = mm.MfmaKey(P, q_shift=mm.Q1_SHIFT)
    assert sum(len(ks) for ks in key.tiles1().values()) == 15
    assert sum(len(ks) for ks in mm.MfmaKey(P).tiles1().values()) == 19
    assert _top_digit(key) <= 133
    key.check_skipped_tiles()                    # zero outside the tile list; shared image slots hold equal tiles
    # the pad columns and the columns above the constant digits are zero in every row
    for s in range(key.s1_lo, key.s1_lo + 160):
        assert all(key.a1(s, i) == 0 for i in list(range(8)) + list(range(146, 160))), s
    assert len(key.tile_image()) == 19 * 1024


def test_a_shift_of_4_is_not_enough_at_1009_bits():
    for P in (_random_p(1009), JUST_ABOVE):
        key = mm.MfmaKey(P, q_shift=4)
        assert _top_digit(key) == 133            # s - i + 4 >= 133 in a sub-diagonal tile: one entry per tile stays
        with pytest.raises(AssertionError):
            key.check_skipped_tiles()
        left = [sum(1 for r in range(32) for i in range(32) if key.a1(128 + 32 * (k + 1) + r, 32 * k + i))
                for k in range(4)]
        assert left == [1, 1, 1, 1], left
        mm.MfmaKey(P, q_shift=8).check_skipped_tiles()


def _extreme_q1(rng):
    zero = [0] * (K + 1)
    ones = [MASK] * (K + 1)                      # every operand byte 0xff
    bit28 = [rng.getrandbits(B) for _ in range(K + 1)]
    bit28[0] |= 1 << B                           # the digit 16 c beside the constant digit
    return [zero, ones, bit28, [1 << B] + [0] * K, [MASK | 1 << B] + [MASK] * K]


def _same_columns(P, q1s, rng):
    k0, k8 = mm.MfmaKey(P), mm.MfmaKey(P, q_shift=mm.Q1_SHIFT)
    for q1 in q1s:
        col0, n0 = mm.columns1(k0, q1)
        col8, n8 = mm.columns1(k8, q1)
        assert col0 == col8 and n0 == n8         # column for column, s = 128..271
        colj, _ = mm.columns1(k8, q1, pad=lambda: rng.getrandbits(32))
        assert colj == col0                      # the pad dwords (0, 1, 37..39) filled at random
        colf, _ = mm.columns1(k8, q1, pad=lambda: 0xFFFFFFFF)
        assert colf == col0
        assert mm.product1(k8, q1) == mm.product1(k0, q1)


@pytest.mark.parametrize("P", [P for _, P in KEYS], ids=[n for n, _ in KEYS])
def test_column_sums_equal_the_unshifted_ones(P):
    rng = random.Random(P & 0xFFFFFFFF)
    q1s = [[rng.getrandbits(B + 1)] + [rng.getrandbits(B) for _ in range(K)] for _ in range(6)] + _extreme_q1(rng)
    _same_columns(P, q1s, rng)


def test_small_quotients_at_a_wide_modulus():
    """q1 = 1, 2, 15, 16, 17 at P = 2^1030 - 2^600 + 1: numerators around zero (the clamp's side of product 1)"""
    rng = random.Random(3)
    _same_columns(P_WIDE, [pm.limbs(v, K + 1) for v in (1, 2, 15, 16, 17)], rng)
    k8 = mm.MfmaKey(P_WIDE, q_shift=mm.Q1_SHIFT)
    assert any(mm.product1(k8, pm.limbs(v, K + 1))[1] for v in (1, 2, 15, 16, 17))      # some of them clamp


@pytest.mark.parametrize("bits", [1009, 1027])
def test_both_reduction_forms_under_the_shifted_layout(bits):
    """squarings and products through fthe_padic_m37t's Barrett (limb fold + clamp and dword fold, each checked
    against the five-tile remainder inside barrett_top) on the shifted key"""
    saved = pm.barrett
    mm.install_top()
    try:
        P = _random_p(bits)
        key = mm.MfmaKey(P, q_shift=mm.Q1_SHIFT)
        rng = random.Random(bits)
        P2 = P * P
        top = mm.TOPEST_DIGIT * P - 1
        for x0v, x1v in ((top, top), (1, 0), (0, 1), (P - 1, P - 1), (rng.randrange(top), rng.randrange(top))):
            z0, z1 = pm.sqr(key, pm.limbs(x0v, K), pm.limbs(x1v, K))
            X = x0v + x1v * P
            assert (pm.value(z0) + pm.value(z1) * P) % P2 == X * X % P2
            y0, y1 = pm.mul(key, z0, z1, pm.limbs(x0v, K), pm.limbs(x1v, K))
            assert (pm.value(y0) + pm.value(y1) * P) % P2 == X ** 3 % P2
            assert max(pm.value(y0), pm.value(y1)) < P + (1 << 1015)
        for X in (0, 1, (1 << 1008) - 1, 1 << 1008, 3 * P2 - 1):                        # LOADP, incl. q1 = 0
            q3, r, _ = mm.barrett(key, pm.limbs(X, 2 * K))
            assert pm.value(q3) * P + pm.value(r) == X
    finally:
        pm.barrett = saved


def test_host_tile_image_matches_model(tmp_path):
    exe = tmp_path / "padic_tiles_dump"
    r = subprocess.run(["g++", "-O1", "-idirafter", "/opt/conda/include", "-o", str(exe),
                        os.path.join(ROOT, "tools", "padic_tiles_dump.cpp"), "-l:libgmp.so.10"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-400:]
    for name, P in KEYS:
        out = tmp_path / "img.bin"
        subprocess.run([str(exe), format(P, "x"), str(out), "8"], check=True)
        key = mm.MfmaKey(P, q_shift=mm.Q1_SHIFT)
        assert out.read_bytes() == key.tile_image() + bytes(1024), name
        subprocess.run([str(exe), format(P, "x"), str(out)], check=True)               # the default image as before
        assert out.read_bytes() == mm.MfmaKey(P).tile_image() + bytes(1024), name
    assert subprocess.run([str(exe), format(KEYS[0][1], "x"), str(out), "4"]).returncode == 1   # 8 or nothing
