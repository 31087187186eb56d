#!/usr/bin/env python3
"""Bit-exact model of the MFMA Barrett reduction of the P-adic kernel (fthe_padic_m37, gen_padic_mfma.py).

The P-adic kernel (tools/padic_model.py) spends ~60% of its multiply-adds in the two Barrett
reductions of every product mod P^2, and both of their products have a CONSTANT operand: the upper
half of q1 * mu and the lower half of q3 * P.  Over the 64 lanes of a wave (64 independent
ciphertext halves) each is a matrix product -- a Toeplitz matrix of the constant's base-256 digits
times the 64 lanes' digit vectors -- which is what the gfx950 matrix core computes:
v_mfma_i32_32x32x32_i8 multiplies a 32x32 i8 tile (the constant, read from LDS) by 32x32 i8 (32 lanes'
digits), accumulating exact int32 column sums.  The variable x variable products (x0^2, 2 x0 x1) stay
on the VALU; the lanes turn column sums back into 28-bit limbs with one v_mad_i64_i32 per column.

Digits.  The matrix core multiplies SIGNED bytes.  The constants are stored in balanced base-256 digits
(each in [-128, 127], same value); a lane's variable bytes b_i are fed as b_i ^ 0x80 = b_i - 128, and the
exact correction 128 * C * sum_i 256^i (a per-key constant) is added back through ONE extra digit
column: the B operand carries a constant digit 1 there and the A tiles that column's balanced digits of
the correction.  So no correction instruction runs on the VALU.

Product 1 (quotient):  q1 = floor(T / b^(K-1)) as bytes i < 136 (its 38 limbs, the lowest one allowed to
be < 2^29), constant digit at i = 136.  Columns s in [128, 272) are formed (the matrix rows reach 287, all
zero from 272 on).  With W = 8 S1_LO = 1024:  the column sums are |c_s| <= 138 * 2^14 < 2^21.2, so the
dropped columns s < 128 hold |L| < 2^21.2 * 256^128 / 255 < 2^(W + 13.3); the constant digit's column
carries floor((c1 - 2^BIAS) / 2^W), which drops 0 <= delta < 2^W more.  So  Pi - N = 2^BIAS + delta + L
for Pi = q1 * mu, and with BIAS = W + 22 = 1046:  Pi - 2^1047 < N < Pi, well inside the  Pi - 2^1064 <
N < Pi  that makes q3 = floor(N / b^(K+1)) Barrett's estimate or one below it.  (Until round 7 the window
began at column 112 with a bias of 2^918: 21 guard columns, folded for an error of 2^-144 of a quotient
unit where 2^-17 serves the same statement; MfmaKey(P, s1_lo=112) still builds that form.)
N < 0 needs Pi < 2^1047, which now also happens for small q1 > 0 when P is near 2^1030 (mu ~ 2^1042);
then floor(Pi / 2^1064) = 0, so the 0 the kernel clamps q3 = -1 to is Barrett's estimate itself (and
q1 < 2^1047 / mu + 1 makes T < (q1 + 1) b^36 < P: the remainder is T).  Where the kernel does not clamp
(the second reduction of a squaring / product), q3 = -1 mod b^K gives r = T + P, the same residue.
The second reduction's q3 only feeds product 2, so the kernel folds it straight into operand dwords
(radix 2^32 from bit QBIT - 8, fold_dwords below) -- equal, dword for dword, to packing the limbs.
Product 2 (remainder):  r = (T - q3 P) mod b^K from columns s < 130 of q3 * P, exact (no truncation):
constant digit at i = 0, q3's bytes at i = 1..132; the matrix columns are s + 1, so that digit i meets
P'[s + 1 - i] (a plain Toeplitz matrix, zero above the diagonal band, as the skipped tiles assume).

This model computes the same column sums (as the tile x digit dot products the lanes feed the matrix
core), the same chunk accumulation (64-bit, arithmetic shifts) and the same clamping, and asserts every
bound (int32 column sums, 64-bit accumulators, digits < 5P).  It also builds the A tiles in the lane
order of the LDS image that the kernel reads (tile_image), which the host code must reproduce.

fthe_padic_m37s feeds product 1's operand 8 digit positions later (MfmaKey(P, q_shift=8)): the same column sums
from 15 tiles instead of 19 (see MfmaKey).

fthe_padic_m37l feeds product 1 the 38 radix-2^28 limbs of q1 as they lie (MfmaKey(P, limb_op=True)): other
column sums, the same Pi = q1 mu and the same window.  Operand digit 4 (t + 1) + j is byte j of limb t, at bit
e = 28 t + 8 j of q1, so its A column holds the balanced digits of mu 2^(e mod 8) from column e div 8 on.  Bytes 0..2
are fed as b ^ 0x80, byte 3 (at most 31) as it is, so the offset's correction is c1 = 128 mu sum_{t<38, j<3} 2^(28 t +
8 j); the constant digit rides in byte 3 of limb 37, which is zero for T < 2^2068.  A column sum has at most 154
terms of at most 2^14: |c_s| < 2^21.3, the dropped columns hold |L| < 2^(1024 + 13.4), and Pi - 2^1047 < N < Pi as
before; the quotient may differ from the byte-fed form's by one (then the remainder by P).

Run:  python tools/padic_mfma_model.py [seed] [trials]
"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import padic_model as pm  # noqa: E402

B = pm.B
MASK = pm.MASK
K = 37
S1_LO = 128                      # product-1 columns S1_LO .. S1_LO + 159 (5 M-tiles of 32)
S1_TOP = 272                     # columns >= 272 are zero: the fold reads S1_LO .. S1_TOP - 1
NQ1 = 136                        # q1 bytes (34 dwords, offset -128)
CONST1 = 136                     # product-1 constant digit position
NQ3 = 132                        # q3 bytes (33 dwords after the constant byte), offset -128
S2_HI = 160                      # product-2 columns 0..159 (only s < 130 are used)
BIAS_BITS = 8 * S1_LO + 22       # 1046
QBIT = B * (K + 1)               # 1064: q3 = floor(N / 2^1064)
DW_BASE = QBIT - 8               # fold_dwords: chunk w holds bits [DW_BASE + 32 w, + 32)
TILE_D1 = (-3, -2, -1, 0, 1)     # product-1 Toeplitz tiles (k <= 3), by d = m - k
TILE_D2 = (0, 1, 2, 3)           # product-2 Toeplitz tiles (k >= 1)


def s32(x):
    assert -(1 << 31) <= x < (1 << 31), "int32 column sum overflow"
    return x


def balanced(x, n):
    """n balanced base-256 digits (each in [-128, 127]) of x >= 0; asserts that they hold x exactly"""
    d = []
    c = 0
    for _ in range(n):
        v = (x & 255) + c
        x >>= 8
        if v >= 128:
            d.append(v - 256)
            c = 1
        else:
            d.append(v)
            c = 0
    assert x == 0 and c == 0, "balanced digits do not hold the value"
    return d


Q1_SHIFT = 8                     # fthe_padic_m37s: q1's byte i is fed at digit index i + 8 (two dwords later)
# fthe_padic_m37l (MfmaKey(P, limb_op=True)): product 1 is fed q1's 38 radix-2^28 limbs as they lie, one
# per operand dword, behind LIMB_PAD pad dwords: digit index 4 (t + LIMB_PAD) + j is byte j of limb t, at bit
# 28 t + 8 j of q1.  Bytes 0..2 are fed as b ^ 0x80, byte 3 (0..15; 0..31 for limb 0, which may hold a bit 28) as it
# is; byte 3 of limb 37 is always zero (T < 2^2068) and carries the constant digit 1.
LIMB_PAD = 1
LIMB_CONST = 4 * (LIMB_PAD + 37) + 3
LIMB_T_BITS = 2068               # the reduced value is below 2^LIMB_T_BITS: limb 73 < 2^24
LIMB_ENTRIES = 154               # a column sum has at most this many non-zero terms, each at most 2^14


class MfmaKey(pm.PadicKey):
    """q_shift (fthe_padic_m37s: Q1_SHIFT): product 1's operand starts q_shift digits later, A1'[s][i + q_shift] =
    A1[s][i] with zero columns below q_shift (the operand's pad), so every column sum is the same and the tiles
    with m - k = 1 hold only mu' digits from index 137 on: zero, since mu < 2^1064 ends at digit 133.  Any shift
    (a multiple of 4 up to 20) is modelled, so that the tests can show that 4 does not empty those tiles."""

    def __init__(self, P, s1_lo=S1_LO, q_shift=0, limb_op=False):
        super().__init__(P, K)
        assert s1_lo in (112, 128)                          # 112: the window and bias of rounds 2-6
        assert q_shift == 0 or (s1_lo == 128 and q_shift % 4 == 0 and 0 < q_shift <= 160 - CONST1 - 2)
        assert not limb_op or (s1_lo == 128 and q_shift == 0)
        self.q_shift = q_shift
        self.limb_op = limb_op
        self.s1_lo, self.bias_bits = s1_lo, 8 * s1_lo + 22
        mu = pm.value(self.mu)
        self.mu_d = balanced(mu, 135)                       # mu < 2^1063: 134 digits + a carry digit
        self.P_d = balanced(P, 130)                         # P < 2^1031
        c1 = 128 * mu * sum(256 ** i for i in range(NQ1))
        g1 = (c1 - (1 << self.bias_bits)) >> (8 * s1_lo)    # columns >= s1_lo (the floor drops < 256^s1_lo)
        self.g1 = balanced(g1, 160)
        c2 = 128 * P * sum(256 ** i for i in range(NQ3))
        self.g2 = balanced(c2 % (1 << 1040), 131)[:130]     # mod 2^1040 (columns < 130; 256^130 = 0 mod b^K)
        if limb_op:
            # the limb-fed operand advances 7 bits per digit index against 8 per column: the A entry of byte j of
            # limb t (bit e = 28 t + 8 j) is a digit of mu 2^(e mod 8), i.e. of mu (even t) or 16 mu (odd t)
            self.mu_dl = (balanced(mu, 136), balanced(16 * mu, 136))
            c1 = 128 * mu * sum(1 << (B * t + 8 * j) for t in range(38) for j in range(3))
            self.g1 = balanced((c1 - (1 << self.bias_bits)) >> (8 * s1_lo), 160)

    def a1_limb(self, s, i):
        u, j = divmod(i, 4)
        t = u - LIMB_PAD
        if not 0 <= t < 38:
            return 0                            # the pad dwords
        if i == LIMB_CONST:
            return self.g1[s - self.s1_lo] if self.s1_lo <= s < self.s1_lo + 160 else 0
        a, b = divmod(B * t + 8 * j, 8)
        d = self.mu_dl[b // 4]
        return d[s - a] if 0 <= s - a < len(d) else 0

    # A[s][i] of the two products (s: output column, i: B digit index)
    def a1(self, s, i):
        if self.limb_op:
            return self.a1_limb(s, i)
        i -= self.q_shift                       # the digit index of the unshifted layout; the pad columns are zero
        if i < 0:
            return 0
        if i == CONST1:
            return self.g1[s - self.s1_lo] if self.s1_lo <= s < self.s1_lo + 160 else 0
        if i == CONST1 + 1:                     # 16 c for the bit 28 of q1's lowest limb (< 2^29)
            j = s - 3
            return self.mu_d[j] if 0 <= j < len(self.mu_d) else 0
        if i > CONST1:
            return 0
        j = s - i
        return self.mu_d[j] if 0 <= j < len(self.mu_d) else 0

    def a2(self, s, i):
        """product 2 in shifted columns: s = 1 + the column of q3 P (weight 256^(s - 1)), so that the
        q3 digit i (byte i - 1) meets P'[s - i]: a plain Toeplitz matrix, zero for i > s"""
        if i == 0:
            return self.g2[s - 1] if 1 <= s <= len(self.g2) else 0
        j = s - i
        return self.P_d[j] if 0 <= j < len(self.P_d) else 0

    def d1_max(self):
        """product 1 forms the tiles with m - k <= d1_max"""
        return 0 if self.q_shift or self.limb_op else 1

    def tiles1(self):
        """product 1's tiles as the kernel forms them: {m: [k ...]}"""
        return {m: [k for k in range(5) if m - k <= self.d1_max()] for m in range(5)}

    def tile1_slot(self, m, k):
        """the image tile that the kernel reads for product 1's tile (m, k) (gen_padic_mfma.tile_index)"""
        if self.limb_op:                        # the band is tilted: every tile has a slot of its own, m-major
            assert k >= m
            return sum(5 - x for x in range(m)) + k - m
        if k == 4:
            return 5 + m
        if self.q_shift and k == 0:
            assert m == 0                       # the pad columns: no instance of the m - k = 0 Toeplitz tile
            return 4
        return TILE_D1.index(m - k)

    def check_skipped_tiles(self):
        """the kernel forms only tiles (m, k) with m - k <= 1 (product 1; m - k <= 0 under q_shift) and m >= k
        (product 2): every other tile of the A matrices must be zero, and the tiles that share an image slot
        equal"""
        for m in range(5):
            for k in range(5):
                for r in range(32):
                    for i in range(32 * k, 32 * k + 32):
                        if m - k > self.d1_max():
                            assert self.a1(self.s1_lo + 32 * m + r, i) == 0, (m, k)
                        if m < k:
                            assert self.a2(32 * m + r, i) == 0, (m, k)
        slots = {}
        for m, ks in self.tiles1().items():
            for k in ks:
                t = [self.a1(self.s1_lo + 32 * m + r, 32 * k + i) for r in range(32) for i in range(32)]
                assert slots.setdefault(self.tile1_slot(m, k), t) == t, (m, k)
        for s in range(S1_TOP, self.s1_lo + 160):           # the rows of M-tile 4 that the fold leaves out
            assert all(self.a1(s, i) == 0 for i in range(160)), s

    def tile_image(self):
        """the 19 A tiles as the kernel's LDS image: tile t is 1 KB, lane l's 16 bytes at l * 16
        (row r = l & 31, digits i = 16 (l >> 5) + j of the tile); order: product 1 Toeplitz d = -3..1
        (k = 0), product 1 k = 4 for m = 0..4, product 2 k = 0 for m = 0..4, product 2 Toeplitz d = 0..3
        (k = 1).  Entries are int8 as unsigned bytes."""
        out = bytearray()

        def tile(fn, s_base, m, k):
            for l in range(64):
                r, h = l & 31, l >> 5
                for j in range(16):
                    out.append(fn(s_base + 32 * m + r, 32 * k + 16 * h + j) & 255)
        if self.limb_op:                        # 15 product-1 tiles in slot order, then product 2's nine: 24 KB
            for m in range(5):
                for k in range(m, 5):
                    assert self.tile1_slot(m, k) * 1024 == len(out)
                    tile(self.a1, self.s1_lo, m, k)
            for m in range(5):
                tile(self.a2, 0, m, 0)
            for d in TILE_D2:
                tile(self.a2, 0, d + 1, 1)
            return bytes(out)
        if self.q_shift:                        # Toeplitz d = -3..0 (k = 3), then tile (0, 0) in the slot of d = 1
            assert self.q_shift == Q1_SHIFT
            for d in TILE_D1[:4]:
                tile(self.a1, self.s1_lo, d + 3, 3)
            tile(self.a1, self.s1_lo, 0, 0)
        else:
            for d in TILE_D1:                   # (m, k) = (d + 3, 3) is one of its instances... any will do
                m, k = (d, 0) if d >= 0 else (0, -d)
                tile(self.a1, self.s1_lo, m, k)
        for m in range(5):
            tile(self.a1, self.s1_lo, m, 4)
        for m in range(5):
            tile(self.a2, 0, m, 0)
        for d in TILE_D2:
            tile(self.a2, 0, d + 1, 1)
        return bytes(out)


def pack(limbs_, shift_bits, ndw):
    """the kernel's radix conversion: limb t (value < 2^30) lands at bit 28 t + shift_bits; dword w is
    acc's low word after the limbs that start in it; acc >>= 32 (acc < 2^64 asserted)"""
    dw = []
    acc = 0
    t = 0
    for w in range(ndw):
        while t < len(limbs_) and (B * t + shift_bits) // 32 == w:
            sh = B * t + shift_bits - 32 * w
            acc += limbs_[t] << sh
            assert acc < (1 << 64)
            t += 1
        dw.append(acc & 0xFFFFFFFF)
        acc >>= 32
    assert acc == 0 and t == len(limbs_), "packed value does not fit"
    return dw


def digits_of(dwords, xor_masks):
    """signed bytes the matrix core sees (dword i XOR xor_masks[i])"""
    out = []
    for w, m in zip(dwords, xor_masks):
        v = w ^ m
        for b in range(4):
            x = (v >> (8 * b)) & 255
            out.append(x - 256 if x >= 128 else x)
    return out


def orpack(limbs_, shift_bits, ndw):
    """the kernel's pack: dword w = (L_lo >> off) | (L_lo+1 << (28 - off)), normalised limbs (< 2^28)"""
    assert all(0 <= v < (1 << B) for v in limbs_)
    val = sum(v << (B * t + shift_bits) for t, v in enumerate(limbs_))
    assert val < (1 << (32 * ndw))
    return [(val >> (32 * w)) & 0xFFFFFFFF for w in range(ndw)]


def columns1(key, q1, pad=None):
    """the int32 column sums s1_lo .. S1_TOP - 1 of product 1 over the tiles the kernel forms (key.tiles1()), and
    Pi = q1 mu.  pad (q_shift): a function giving the dwords the kernel leaves undefined (the operand's pad and
    the dwords above the constant one); default 0"""
    c = q1[0] >> B
    assert c in (0, 1)
    qd = key.q_shift // 4
    fill = pad or (lambda: 0)
    if key.limb_op:
        assert all(0 <= v <= MASK for v in q1[1:]) and q1[37] < (1 << (LIMB_T_BITS - B * 73)), "limb 73's byte 3"
        dw = [fill() for _ in range(LIMB_PAD)] + list(q1) + [fill() for _ in range(2 - LIMB_PAD)]
        dig = digits_of(dw, [0] * LIMB_PAD + [0x00808080] * 37 + [0x01808080] + [0] * (2 - LIMB_PAD))
        assert dig[LIMB_CONST] == 1 and all(0 <= dig[4 * (t + LIMB_PAD) + 3] < (32 if t == 0 else 16) for t in range(37))
    else:
        dw = [fill() for _ in range(qd)] + orpack([q1[0] & MASK] + list(q1[1:]), 0, 34) + [1 | (c << 12)]
        dw += [fill() if qd else 0 for _ in range(40 - len(dw))]
        dig = digits_of(dw, [0] * qd + [0x80808080] * 34 + [0] * (6 - qd))
        assert dig[CONST1 + key.q_shift] == 1 and dig[CONST1 + 1 + key.q_shift] == 16 * c
    col = {}
    tiles = key.tiles1()
    for s in range(key.s1_lo, S1_TOP):
        ks = tiles[(s - key.s1_lo) // 32]
        col[s] = s32(sum(key.a1(s, i) * dig[i] for k in ks for i in range(32 * k, 32 * k + 32) if dig[i]))
    if key.limb_op:
        # 152 operand bytes and the constant digit, |a b| <= 2^14 each: |c_s| < 2^21.3, so the dropped columns hold
        # |L| < 2^21.3 256^128 / 255 < 2^(1024 + 13.4) and the pair sums of the fold stay in 32 bits
        for s in range(key.s1_lo, S1_TOP):
            assert abs(col[s]) <= LIMB_ENTRIES << 14, "column sum bound"
            assert abs(col[s] + 256 * col.get(s + 1, 0)) < (1 << 31), "pairing bound"
    Pi = pm.value(q1) * pm.value(key.mu)
    N = sum(v << (8 * s) for s, v in col.items())
    assert Pi - (1 << (key.bias_bits + 1)) < N < Pi and key.bias_bits + 1 <= QBIT, "Pi - 2^1064 < N < Pi"
    if N < 0:                                   # the clamped 0 is Barrett's estimate floor(Pi / 2^1064)
        assert Pi < (1 << QBIT) and pm.value(q1) * (1 << (B * (K - 1))) + (1 << (B * (K - 1))) <= key.P
    return col, N


def fold_limbs(col, s1_lo):
    """the kernel's limb fold: chunk t holds bits [QBIT + 28 t, + 28) (64-bit sums, arithmetic shifts);
    returns (the K limbs of q3 mod b^K, the final carry: 0, or -1 for N < 0)"""
    acc = 0
    q3 = []
    for t in range((8 * s1_lo - QBIT) // B, 40):
        for s in col:
            if (8 * s - QBIT) // B == t:
                acc = pm.s64(acc + (col[s] << (8 * s - QBIT - B * t)))
        if 0 <= t < K:
            q3.append(acc & MASK)
        acc >>= B
    assert acc in (0, -1)
    return q3, acc


def fold_dwords(col, s1_lo, ndw=33, frac=None):
    """the second reduction's fold: the 33 operand dwords of product 2 (before the XOR with 0x80) straight from
    the column sums -- chunk w holds bits [DW_BASE + 32 w, + 32) (64-bit sums, carry = sum >> 32), dword 0's
    low byte replaced by the constant digit 1, dword 32 cut at q3's bit 28 K.  Columns >= 264 are not read.
    ndw = 32 (fthe_padic_m37t): the fold ends at dword 31, columns >= 260 are not read.  frac: a list that
    receives f32 = bits 1032..1063 of N (chunk -1 and chunk 0's low byte, v_alignbit_b32 by 8)."""
    acc = 0
    dw = []
    lowc = {}
    for w in range((8 * s1_lo - DW_BASE) // 32, ndw):
        for s in col:
            if (8 * s - DW_BASE) // 32 == w:
                acc = pm.s64(acc + (col[s] << (8 * s - DW_BASE - 32 * w)))
        lowc[w] = acc & 0xFFFFFFFF
        if w >= 0:
            dw.append(acc & 0xFFFFFFFF)
        acc >>= 32
    if frac is not None:
        frac.append(((lowc[0] << 32 | lowc[-1]) >> 8) & 0xFFFFFFFF)
    dw[0] = (dw[0] & 0xFFFFFF00) | 1
    if ndw == 33:
        dw[32] &= (1 << (B * K + 8 - 32 * 32)) - 1
    return dw


def frac_limbs(col, s1_lo):
    """f32 of the first reduction's limb fold: chunk -1 (bits 1036..1063 of N) shifted left by 4"""
    acc = 0
    for t in range((8 * s1_lo - QBIT) // B, 0):
        for s in col:
            if (8 * s - QBIT) // B == t:
                acc = pm.s64(acc + (col[s] << (8 * s - QBIT - B * t)))
        lo = acc & 0xFFFFFFFF
        acc >>= B
    return (lo << 4) & 0xFFFFFFFF


# ---- fthe_padic_m37t: four-tile product 2, limb 36 from product 1's fraction -------------------------------
# r = T - q3 P with q3 = floor(N / 2^1064), so r = P (f + e) for f = frac(N / 2^1064) and e = T / P - N / 2^1064:
#   0 <= e <= 2^1009 / P (q1 drops limbs 0..35 of T; the second reduction's carry u1 in unnormalised limbs below
#   2^29, so up to 2 b^36) + T / 2^2072 (mu drops < 1) + 2^-17 (Pi - N < 2^1047).
# So P f <= r < P f + W, W = 2^1009 + T P / 2^2072 + P 2^-17.  The kernel holds f32 = floor(2^32 f) (the dword
# fold) or its top 28 bits (the limb fold) and Pt = floor(P / 2^1000) and forms E = floor(f32 Pt / 2^32):
#   0 <= P f / 2^1000 - E < 1 (Pt) + Pt 2^-28 (f32: <= 1/2 for P < 2^1027) + 1 (floor) < 3.
# Tiles 0..3 give r mod 2^1016 exactly; with b = bits 1008..1015 of r and r = 2^1016 h + 2^1008 b + low, the
# distance d = r / 2^1000 - E (units of 2^1000) lies in [0, W / 2^1000 + 3), and for 0 <= d <= C = 128 * 256
#   E + C - 256 b = 65536 h + (low / 2^1000) + (C - d)  in  [65536 h, 65536 h + 255 + C]:  h = (E + C - 256 b) >> 16.
# (The rule holds for every d in [C - 65535 + 255, C]; the asserted window [0, C] is half of the 256 units.)
# T is at most TOPEST_T(P) = 2 (3P)^2 + 9P + 1, the cross term of digits below 3P plus u1, so W / 2^1008 <
# 2 + 18 P^3 / 2^3080 + P / 2^1025: 42.1 units at P < 2^1027 (a third of C), 298 at P < 2^1028 (too wide).
TOPEST_MAX_BITS = 1027
PT_SHIFT = 1000
TOPEST_C = 128 << 8
TOPEST_DIGIT = 3                 # SQR / MUL digits are below TOPEST_DIGIT * P


def topest_t_max(P):
    return 2 * (TOPEST_DIGIT * P) ** 2 + TOPEST_DIGIT * TOPEST_DIGIT * P + 1


def topest_window(P, Tmax=None, low=2 << (B * (K - 1))):
    """an upper bound of d (units of 2^1000, rounded up) over all T <= Tmax whose limbs 0..35 hold at most low"""
    Tmax = topest_t_max(P) if Tmax is None else Tmax
    W = low + -(-Tmax * P >> 2072) + (P >> 17) + 1
    return -(-W >> PT_SHIFT) + 3


def topest_check_key(P):
    assert P.bit_length() <= TOPEST_MAX_BITS, "fthe_padic_m37t: P wider than the admitted size"
    assert 2 * topest_window(P) <= 2 * TOPEST_C and topest_window(P) <= TOPEST_C, "window wider than half of 256 units"
    return topest_window(P)


SLACK = {"d_max": 0}             # the largest d seen (tests report it against TOPEST_C)


def top_limb(key, r36_low, f32, clamped=False):
    """limb 36 of r from its exact low byte and f32 (the kernel's seven instructions)"""
    Pt = key.P >> PT_SHIFT
    assert Pt < (1 << 32) and 0 <= f32 < (1 << 32)
    E = (f32 * Pt) >> 32
    b = r36_low & 0xFF
    h = ((E + TOPEST_C - (b << 8)) & 0xFFFFFFFF) >> 16
    if clamped:
        h = 0
    return b | (h << 8), E


def product2_top(key, dw, T, f32, clamped=False):
    """the four-tile product 2: operand dwords 0..31 (the constant digit, q3 bytes 0..126), matrix columns
    1..127 folded as in product2, limb 36 by top_limb"""
    assert len(dw) == 32
    dig = digits_of(dw, [0x80808000] + [0x80808080] * 31)
    assert dig[0] == 1
    r = []
    acc = 0
    for t in range(K):
        acc = acc + T[t]
        for s in range(1, 128):
            if (8 * s - 8) // B == t:
                c = s32(sum(key.a2(s, i) * dig[i] for i in range(128) if dig[i]))
                acc = pm.s64(acc - (c << (8 * s - 8 - B * t)))
        r.append(acc & MASK)
        acc >>= B
    r[K - 1], E = top_limb(key, r[K - 1], f32, clamped)
    return r, E


def barrett_top(key, T):
    """one Barrett as fthe_padic_m37t runs it, in both of its forms: the first reduction's (limb fold, clamp) and
    the second's (dword fold to dword 31, no clamp).  Asserts: T within the contract, both forms reproduce the
    five-tile r exactly (the second r + P where the first clamps), d within [0, TOPEST_C] (the candidate is
    unique with a factor of two to spare), r < P + 2^1015.  Returns (q3, r, clamped) like barrett."""
    P = key.P
    topest_check_key(P)
    Tv = pm.value(T)
    assert Tv <= topest_t_max(P), "T beyond the contract (digits below 3P)"
    low = pm.value(T[:K - 1]) + 1
    assert low <= 2 << (B * (K - 1))
    q3, r, clamped = barrett(key, T)
    col, N = columns1(key, T[K - 1:2 * K])
    rv = pm.value(r)
    # first form
    f28 = frac_limbs(col, key.s1_lo)
    assert f28 == ((N >> (QBIT - 28)) & MASK) << 4
    dw = orpack(q3, 8, 33)[:32]
    dw[0] |= 1
    r1, E1 = product2_top(key, dw, T, f28, clamped)
    assert r1 == r, "four-tile product 2 (limb fold) != five-tile"
    # second form
    fr = []
    dw2 = fold_dwords({s: c for s, c in col.items() if s < 260}, key.s1_lo, ndw=32, frac=fr)
    assert fr[0] == (N >> (QBIT - 32)) & 0xFFFFFFFF
    if clamped:                                  # q3 = -1 mod b^K where the kernel does not clamp: r = T + P
        assert dw2 == [0xFFFFFF01] + [0xFFFFFFFF] * 31
        want = pm.limbs(Tv + P, K)
    else:
        assert dw2 == dw
        want = r
    r2, E2 = product2_top(key, dw2, T, fr[0], False)
    assert r2 == want, "four-tile product 2 (dword fold) != five-tile"
    for E, R in ((E1, None if clamped else rv), (E2, pm.value(want))):
        if R is None:
            continue
        d = -(-R >> PT_SHIFT) - E
        wnd = topest_window(P, Tv, low)
        assert 0 <= (R >> PT_SHIFT) - E and d <= wnd <= topest_window(P) <= TOPEST_C, (d, wnd)
        SLACK["d_max"] = max(SLACK["d_max"], d)
        assert R < P + (1 << 1015)
    if clamped:
        assert Tv < (1 << 1016)
    return q3, r, clamped


def product1(key, q1):
    """q1: 38 limbs (q1[0] < 2^29, others < 2^28).  Returns (q3 limbs, clamped).  Bit 28 of q1[0] (c) is
    fed as the digit 16 c at position 137, whose A column is mu' shifted by 3 bytes."""
    col, N = columns1(key, q1)
    q3, acc = fold_limbs(col, key.s1_lo)
    assert (acc == -1) == (N < 0)
    want = orpack(q3, 8, 33)                     # the limb fold, packed as product 2's operand
    want[0] |= 1
    assert fold_dwords(col, key.s1_lo) == want, "dword fold != orpack(limb fold)"
    clamped = acc == -1
    if clamped:
        assert all(v == MASK for v in q3)
        q3 = [0] * K
    return q3, clamped


def product2(key, q3, T):
    """r = (T - q3 P) mod b^K (T: limbs 0..K-1, < 2^29 allowed)"""
    dw = orpack(q3, 8, 33)
    dw[0] |= 1
    dw += [0] * 7
    dig = digits_of(dw, [0x80808000] + [0x80808080] * 32 + [0x00000080] + [0] * 6)
    assert dig[0] == 1
    r = []
    acc = 0
    for t in range(K):
        acc = acc + T[t]
        for s in range(1, 131):
            if (8 * s - 8) // B == t:
                c = s32(sum(key.a2(s, i) * dig[i] for i in range(160) if dig[i]))
                acc = pm.s64(acc - (c << (8 * s - 8 - B * t)))
        r.append(acc & MASK)
        acc >>= B
    return r


def barrett(key, T, clamp=True):
    q1 = T[K - 1:2 * K]
    q3, clamped = product1(key, q1)
    r = product2(key, q3, T)
    assert pm.value(T) - pm.value(q3) * key.P == pm.value(r), "T = q3 P + r"
    return q3, r, clamped


KARA_H = 19                      # kara_cross / kara_cross_mul: a digit's low half is limbs 0..18, its high half 19..36


def kara_cross_mul(x0, x1, y0, y1):
    """MUL's cross term W = x0 y1 + x1 y0 as fthe_padic_m37k forms it (gen_padic_mfma.py kara_cross_mul),
    instruction for instruction on one lane's limbs: P2 and P0 by product scanning, the half sums, the middle columns
    with the biased addend t' and the carry from 3, the ripple through limbs 57..73.  Asserts every bound the kernel
    relies on -- limbs below 2^28 and P2's top limb too (stored by XOR), half sums below 2^29, a middle column within
    38 2^58 + t' + carry < 2^64, t' in [0, 2^30) ([0, 2^31) in column 18), the ripple's 32-bit values non-negative,
    W < 2^LIMB_T_BITS (byte 3 of limb 73 carries the constant digit) -- and that the 74 limbs returned hold
    x0 y1 + x1 y0."""
    H = KARA_H
    for d in (x0, x1, y0, y1):
        assert len(d) == K and all(0 <= v <= MASK for v in d)

    def scan(pairs, n):
        """limbs 0..n-1 of sum a b over (a, b) in pairs by product scanning: 64-bit columns, 28-bit limbs, the last
        limb unmasked"""
        out, carry = [], 0
        for c in range(n):
            col = carry
            for a, b in pairs:
                col += sum(a[i] * b[c - i] for i in range(len(a)) if 0 <= c - i < len(b))
            assert 0 <= col < (1 << 64)
            out.append(col & MASK if c < n - 1 else col)
            carry = col >> B
        return out
    lo, hi = (lambda d: d[:H]), (lambda d: d[H:])
    P2 = scan([(hi(x0), hi(y1)), (hi(x1), hi(y0))], 2 * (K - H))
    assert P2[-1] <= MASK, "P2's top limb is complemented by XOR with the mask"
    P2c = [MASK - v for v in P2]                                 # V[38..73]
    P0 = scan([(lo(x0), lo(y1)), (lo(x1), lo(y0))], 2 * H)
    assert P0[-1] < (1 << 29)
    Vl, C = P0[:H], P0[H:]                                       # V[0..18], C (limb 37 unmasked)
    half = lambda d: [d[i] + d[H + i] for i in range(K - H)] + [d[H - 1]]      # noqa: E731
    A0, A1, B0, B1 = half(x0), half(x1), half(y0), half(y1)
    assert all(v < (1 << 29) for s in (A0, A1, B0, B1) for v in s), "half sum limb"
    mid, carry = [], 3
    for k in range(2 * H):
        if k < H:
            t = C[k] - Vl[k] + P2c[k] + 2 * MASK
        elif k < 2 * (K - H):
            t = P2c[k] - P2c[k - H] - C[k - H] + 3 * MASK
        else:
            t = 4 * MASK - P2c[k - H] - C[k - H]
        # column 18 takes P0's limb 37, which is not masked (below 2^29): t' < 2^29 + 3 mask there, still a dword
        assert 0 <= t < ((1 << 31) if k == H - 1 else (1 << 30)), ("t'", k, t)
        prod = sum(A0[i] * B1[k - i] + A1[i] * B0[k - i] for i in range(H) if 0 <= k - i < H)
        assert prod <= 38 << 58
        col = prod + t + carry
        assert col < (1 << 64)
        mid.append(col & MASK)
        carry = col >> B
    W = Vl + mid + P2c[H:]                                       # limbs 0..18, 19..56, 57..73 (complemented)
    v = (W[57] ^ MASK) + carry - 3                               # 32-bit lane arithmetic
    assert 0 <= carry - 3 and 0 <= v < (1 << 32)
    for j in range(57, 2 * K - 1):
        W[j] = v & MASK
        v = (W[j + 1] ^ MASK) + (v >> B)
        assert 0 <= v < (1 << 32)
    W[2 * K - 1] = v
    assert v < (1 << (LIMB_T_BITS - B * (2 * K - 1))), "W reaches byte 3 of limb 73"
    assert pm.value(W) == pm.value(x0) * pm.value(y1) + pm.value(x1) * pm.value(y0) and max(W) <= MASK
    return W


pm_barrett = pm.barrett


def install():
    """route padic_model's sqr / mul / loadp through this Barrett"""
    pm.barrett = lambda key, T: barrett(key, T)[:2]


def install_top():
    """the same through fthe_padic_m37t's Barrett (loadp too: its inputs below 3 P^2 lie within the contract)"""
    pm.barrett = lambda key, T: barrett_top(key, T)[:2]


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    trials = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    rng = random.Random(seed)
    install()
    nclamp = 0
    for t in range(trials):
        bits = rng.choice([1009, 1010, 1023, 1024, 1024, 1029, 1030])
        P = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        key = MfmaKey(P, q_shift=Q1_SHIFT if t % 2 else 0)      # both layouts give the same column sums
        assert len(key.tile_image()) == 19 * 1024
        key.check_skipped_tiles()
        P2 = P * P
        # random and extreme digits through squaring / product
        for x0v, x1v in ((5 * P - 1, 5 * P - 1), (1, 0), (2, 0), (0, 1), (P - 1, P - 1),
                         (rng.randrange(5 * P), rng.randrange(5 * P))):
            x0, x1 = pm.limbs(x0v, K), pm.limbs(x1v, K)
            z0, z1 = pm.sqr(key, x0, x1)
            X = x0v + x1v * P
            assert (pm.value(z0) + pm.value(z1) * P) % P2 == X * X % P2
            pm.check_digit(key, z0)
            pm.check_digit(key, z1)
        a0, a1 = pm.limbs(rng.randrange(5 * P), K), pm.limbs(rng.randrange(5 * P), K)
        b0, b1 = pm.limbs(rng.randrange(5 * P), K), pm.limbs(rng.randrange(5 * P), K)
        z0, z1 = pm.mul(key, a0, a1, b0, b1)
        A = pm.value(a0) + pm.value(a1) * P
        Bv = pm.value(b0) + pm.value(b1) * P
        assert (pm.value(z0) + pm.value(z1) * P) % P2 == A * Bv % P2
        pm.check_digit(key, z0)
        pm.check_digit(key, z1)
        # LOADP of small and large plain values (clamp path for X < b^36)
        for X in (0, 1, 5, (1 << 1008) - 1, 1 << 1008, 50 * P2 - 1, rng.randrange(P2)):
            T = pm.limbs(X, 2 * K)
            q3, r, cl = barrett(key, T)
            nclamp += cl
            assert pm.value(r) < 5 * P and pm.value(q3) * P + pm.value(r) == X
        if t < 3:
            for X, e in ((rng.randrange(1, P), P), (rng.randrange(P2), P - 1), (1, P), (2, P - 1)):
                got = pm.value(pm.padic_pow(key, X, e))
                assert got % P2 == pow(X, e, P2), t
    print(f"ok: {trials} keys (squaring / product / LOADP through the MFMA Barrett, {nclamp} clamped quotients, "
          f"exponentiations)")
    # fthe_padic_m37t: digits below 3P, P of at most TOPEST_MAX_BITS bits
    install_top()
    for t in range(trials):
        bits = rng.choice([1009, 1010, 1023, 1024, 1024, 1026, TOPEST_MAX_BITS])
        P = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        key = MfmaKey(P, q_shift=Q1_SHIFT if t % 2 else 0)      # fthe_padic_m37s / fthe_padic_m37t
        P2 = P * P
        top = TOPEST_DIGIT * P - 1
        for x0v, x1v in ((top, top), (1, 0), (0, 1), (P - 1, P - 1), (2 * P - 1, 2 * P - 1),
                         (rng.randrange(top), rng.randrange(top))):
            z0, z1 = pm.sqr(key, pm.limbs(x0v, K), pm.limbs(x1v, K))
            X = x0v + x1v * P
            assert (pm.value(z0) + pm.value(z1) * P) % P2 == X * X % P2
            assert max(pm.value(z0), pm.value(z1)) < P + (1 << 1015)
            y0, y1 = pm.mul(key, z0, z1, pm.limbs(x0v, K), pm.limbs(x1v, K))
            assert (pm.value(y0) + pm.value(y1) * P) % P2 == X ** 3 % P2
            assert max(pm.value(y0), pm.value(y1)) < P + (1 << 1015)
        if t < 2:
            X, ex = rng.randrange(P2), rng.getrandbits(48) | 1
            assert pm.value(pm.padic_pow(key, X, ex)) % P2 == pow(X, ex, P2)
    install()
    print(f"ok: {trials} keys through the four-tile product 2 (fthe_padic_m37t): largest distance "
          f"{SLACK['d_max'] / 256:.2f} of the {TOPEST_C // 256} units asserted (256 between candidates)")
    # fthe_padic_m37l: the same reductions with product 1 fed the limbs as they lie
    install_top()
    SLACK["d_max"] = 0
    for t in range(trials):
        bits = rng.choice([1009, 1010, 1023, 1024, 1024, 1026, TOPEST_MAX_BITS])
        P = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        if t == 0:
            P = (1 << TOPEST_MAX_BITS) - 1
        key = MfmaKey(P, limb_op=True)
        assert len(key.tile_image()) == 24 * 1024
        key.check_skipped_tiles()
        P2 = P * P
        top = TOPEST_DIGIT * P - 1
        for x0v, x1v in ((top, top), (1, 0), (0, 1), (P - 1, P - 1), (2 * P - 1, 2 * P - 1),
                         (rng.randrange(top), rng.randrange(top))):
            z0, z1 = pm.sqr(key, pm.limbs(x0v, K), pm.limbs(x1v, K))
            X = x0v + x1v * P
            assert (pm.value(z0) + pm.value(z1) * P) % P2 == X * X % P2
            y0, y1 = pm.mul(key, z0, z1, pm.limbs(x0v, K), pm.limbs(x1v, K))
            assert (pm.value(y0) + pm.value(y1) * P) % P2 == X ** 3 % P2
            assert max(pm.value(y0), pm.value(y1)) < P + (1 << 1015)
        for X in (0, 1, 5, (1 << 1008) - 1, 1 << 1008, 3 * P2 - 1, rng.randrange(P2)):      # LOADP
            q3, r, cl = barrett(key, pm.limbs(X, 2 * K))
            assert pm.value(q3) * P + pm.value(r) == X
        if t < 2:
            X, ex = rng.randrange(P2), rng.getrandbits(48) | 1
            assert pm.value(pm.padic_pow(key, X, ex)) % P2 == pow(X, ex, P2)
    install()
    print(f"ok: {trials} keys through the limb-fed product 1 (fthe_padic_m37l): largest distance "
          f"{SLACK['d_max'] / 256:.2f} of the {TOPEST_C // 256} units asserted")


if __name__ == "__main__":
    main()
