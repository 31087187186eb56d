"""CPU checks of the limb-fed product-1 operand of fthe_padic_m37l (gen_padic_mfma.py limb_op): digit
index 4 (t + 1) + j is byte j of q1's radix-2^28 limb t, bytes 0..2 fed as b ^ 0x80 and byte 3 as it is, the constant
digit in byte 3 of limb 37, so A1[s][.] is a balanced digit of mu (even t) or 16 mu (odd t):

* the host's image (padic_tiles::build_limb) is the model's (MfmaKey(P, limb_op=True)), byte for byte, at both ends
  of the admitted range (1009 and 1027 bits), at the bench's 1024 bits and at crafted moduli; 1028 bits are refused;
* every product-1 tile outside the 15 with k >= m is zero there, the pad columns are zero, and without the pad dword
  in front tile (1, 0) is not empty at 1009 bits;
* the column-sum bound (154 terms of at most 2^14), the pairing bound |c_s + 256 c_(s+1)| < 2^31, the window
  Pi - 2^1047 < N < Pi and limb 73's empty byte 3 are asserted by the model on crafted operands: all-ones limbs under
  the digit contract, limb 36 with bit 28, zero, at P = 2^1027 - 1 and P just above 2^1008;
* the quotient is the byte-fed form's or differs from it by one (another truncation), the remainder then by P;
* both forms of the reduction (limb fold with clamp, dword fold) and the four-tile product 2 with its bound on d, on
  squarings and products of the largest digits (barrett_top asserts them)."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import padic_model as pm  # noqa: E402
import padic_mfma_model as mm  # noqa: E402

K, B = mm.K, mm.B
MASK = (1 << B) - 1
JUST_ABOVE = (1 << 1008) + 3                     # the lower end: mu just below 2^1064
P_TOP = (1 << 1027) - 1                          # the upper end
P_WIDE = (1 << 1027) - (1 << 600) + 1


def _random_p(bits):
    rng = random.Random(bits + 15)
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


KEYS = [("1009 bits", _random_p(1009)), ("1024 bits", _random_p(1024)), ("1027 bits", _random_p(1027)),
        ("just above 2^1008", JUST_ABOVE), ("2^1027 - 1", P_TOP), ("2^1027 - 2^600 + 1", P_WIDE)]


@pytest.mark.parametrize("P", [P for _, P in KEYS], ids=[n for n, _ in KEYS])
def test_tiles_outside_the_15_are_zero(P):
    key = mm.MfmaKey(P, limb_op=True)
    tiles = key.tiles1()
    assert sum(len(ks) for ks in tiles.values()) == 15 and all(k >= m for m, ks in tiles.items() for k in ks)
    key.check_skipped_tiles()
    assert sorted(key.tile1_slot(m, k) for m, ks in tiles.items() for k in ks) == list(range(15))
    pads = list(range(4 * mm.LIMB_PAD)) + list(range(4 * (mm.LIMB_PAD + 38), 160))
    assert len(pads) == 8
    for s in range(key.s1_lo, key.s1_lo + 160):
        assert all(key.a1(s, i) == 0 for i in pads), s
    assert len(key.tile_image()) == 24 * 1024


def test_without_the_pad_dword_tile_1_0_is_not_empty_at_1009_bits(monkeypatch):
    monkeypatch.setattr(mm, "LIMB_PAD", 0)
    monkeypatch.setattr(mm, "LIMB_CONST", 4 * 37 + 3)
    for P in (_random_p(1009), JUST_ABOVE):
        key = mm.MfmaKey(P, limb_op=True)
        with pytest.raises(AssertionError):
            key.check_skipped_tiles()
        left = sum(1 for r in range(32) for i in range(32) if key.a1(128 + 32 + r, i))
        assert 0 < left <= 3, left
    mm.MfmaKey(_random_p(1024), limb_op=True).check_skipped_tiles()     # 15 tiles at the bench's size either way


def _crafted_q1(rng):
    top = (1 << (mm.LIMB_T_BITS - B * 73)) - 1                     # limb 73 under T < 2^2068
    ones = [MASK] * K + [top]
    bit28 = [rng.getrandbits(B) | 1 << B] + [rng.getrandbits(B) for _ in range(K - 1)] + [rng.getrandbits(20)]
    return [[0] * (K + 1), ones, [MASK | 1 << B] + ones[1:], bit28, [1 << B] + [0] * K,
            [0x0F7F7F7F] * K + [0x7F7F7F], [0x00808080] * K + [0x808080]]


@pytest.mark.parametrize("P", [P for _, P in KEYS], ids=[n for n, _ in KEYS])
def test_bounds_at_crafted_extremes(P):
    rng = random.Random(P & 0xFFFFFFFF)
    kl, k0 = mm.MfmaKey(P, limb_op=True), mm.MfmaKey(P)
    q1s = _crafted_q1(rng) + [[rng.getrandbits(B + 1)] + [rng.getrandbits(B) for _ in range(K - 1)] +
                              [rng.getrandbits(20)] for _ in range(4)]
    worst = 0
    for q1 in q1s:
        col, N = mm.columns1(kl, q1)               # asserts the column-sum, pairing and window bounds
        worst = max(worst, max(abs(c) for c in col.values()))
        colj, _ = mm.columns1(kl, q1, pad=lambda: rng.getrandbits(32))
        assert colj == col                         # whatever the pad registers hold
        _, N0 = mm.columns1(k0, q1)
        Pi = pm.value(q1) * pm.value(kl.mu)
        assert Pi - (1 << 1047) < N < Pi and Pi - (1 << 1047) < N0 < Pi
        (q3, cl), (q30, cl0) = mm.product1(kl, q1), mm.product1(k0, q1)     # also: dword fold == packed limb fold
        assert abs(pm.value(q3) - pm.value(q30)) <= 1
    assert worst <= mm.LIMB_ENTRIES << 14 < 1 << 22
    with pytest.raises(AssertionError):              # limb 73 with a byte 3: outside the contract
        mm.columns1(kl, [0] * K + [1 << 24])


def test_small_quotients_at_a_wide_modulus():
    """q1 = 0, 1, 2, 15, 16, 17 at P = 2^1027 - 2^600 + 1: numerators around zero, some clamped"""
    kl, k0 = mm.MfmaKey(P_WIDE, limb_op=True), mm.MfmaKey(P_WIDE)
    clamps = []
    for v in (0, 1, 2, 15, 16, 17):
        q3, cl = mm.product1(kl, pm.limbs(v, K + 1))
        assert abs(pm.value(q3) - pm.value(mm.product1(k0, pm.limbs(v, K + 1))[0])) <= 1
        clamps.append(cl)
    assert clamps[0] and not clamps[-1], clamps


@pytest.mark.parametrize("P", [JUST_ABOVE, P_TOP, _random_p(1024)], ids=["just above 2^1008", "2^1027 - 1", "1024 bits"])
def test_both_reduction_forms_and_the_bound_on_d(P):
    saved = pm.barrett
    mm.install_top()
    try:
        key = mm.MfmaKey(P, limb_op=True)
        rng = random.Random(P & 0xFFFF)
        P2 = P * P
        top = mm.TOPEST_DIGIT * P - 1
        allones = (1 << (B * (K - 1))) - 1
        big = allones + (((top - allones) >> (B * (K - 1))) << (B * (K - 1)))
        for x0v, x1v in ((top, top), (big, big), (1, 0), (0, 1), (P - 1, P - 1), (rng.randrange(top), rng.randrange(top))):
            z0, z1 = pm.sqr(key, pm.limbs(x0v, K), pm.limbs(x1v, K))
            X = x0v + x1v * P
            assert (pm.value(z0) + pm.value(z1) * P) % P2 == X * X % P2
            y0, y1 = pm.mul(key, z0, z1, pm.limbs(x0v, K), pm.limbs(x1v, K))
            assert (pm.value(y0) + pm.value(y1) * P) % P2 == X ** 3 % P2
            assert max(pm.value(y0), pm.value(y1)) < P + (1 << 1015)
        for X in (0, 1, (1 << 1008) - 1, 1 << 1008, 3 * P2 - 1):                        # LOADP, incl. q1 = 0
            q3, r, _ = mm.barrett(key, pm.limbs(X, 2 * K))
            assert pm.value(q3) * P + pm.value(r) == X
        assert mm.topest_t_max(P) < 1 << mm.LIMB_T_BITS
    finally:
        pm.barrett = saved


def test_one_size_past_the_range_is_refused():
    P = _random_p(1028)
    with pytest.raises(AssertionError):
        mm.topest_check_key(P)
    assert mm.TOPEST_MAX_BITS == 1027


def test_host_tile_image_matches_model(tmp_path):
    exe = tmp_path / "padic_tiles_dump"
    r = subprocess.run(["g++", "-O1", "-idirafter", "/opt/conda/include", "-o", str(exe),
                        os.path.join(ROOT, "tools", "padic_tiles_dump.cpp"), "-l:libgmp.so.10"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-400:]
    out = tmp_path / "img.bin"
    for name, P in KEYS:
        subprocess.run([str(exe), format(P, "x"), str(out), "l"], check=True)
        assert out.read_bytes() == mm.MfmaKey(P, limb_op=True).tile_image(), name
        subprocess.run([str(exe), format(P, "x"), str(out), "8"], check=True)          # the other images as before
        assert out.read_bytes() == mm.MfmaKey(P, q_shift=mm.Q1_SHIFT).tile_image() + bytes(1024), name
    for P in (_random_p(1028), _random_p(1030), _random_p(1008)):
        assert subprocess.run([str(exe), format(P, "x"), str(out), "l"]).returncode == 1
