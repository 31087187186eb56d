#!/usr/bin/env python3
"""Generator of the P-adic exponentiation kernel with matrix-core Barrett reductions (gfx950 assembly):
fthe_padic_m37, X^e mod P^2 with X = x0 + x1 P kept as two base-P digits of K = 37 radix-2^28 limbs,
one ciphertext half per lane -- the arithmetic of gen_padic.py (see its docstring), except where the
work goes.

The products of a squaring (2 x0 x1, x0^2) are variable x variable and stay on the VALU (product
scanning, v_mad_u64_u32).  The two Barrett reductions that follow every product are 60% of the
multiply-adds of fthe_padic_k37, and both of their products have a constant operand (mu, P): over the
64 lanes of a wave they are matrix products, so they run on v_mfma_i32_32x32x32_i8:

  * each lane packs its operand (q1 = T >> 28 (K-1), or q3) into base-256 digits fed as b ^ 0x80 = b - 128
    (40 dwords, region XB), and v_permlane32_swap turns them into the B operands of two 32-lane groups
    (lanes 0-31 / 32-63 of the wave);
  * the A operand is a 32 x 32 tile of the constant's Toeplitz matrix in balanced base-256 digits, read
    from LDS (19 tiles, 19 KB, filled once per workgroup from the key's context; the correction for the
    -128 offset and the truncation bias ride in one extra digit column, tools/padic_mfma_model.py);
  * each M-tile (32 output columns) accumulates its K-tiles in int32 (16 VGPRs per group); adjacent rows are
    paired in 32-bit, the two groups' accumulators exchanged with v_permlane32_swap (only the registers the
    fold reads) so that every lane holds its own 32 column sums, and the lane folds them into 28-bit limbs:
    one v_mad_i64_i32 per (paired) column (x 2^sh), one mask and one arithmetic shift per limb, the carry
    entering the next limb's first multiply-add;
  * the limbs that only feed the matrix cores (the upper product halves, q3) are produced with their operand
    bytes already XORed with 0x80 (v_bitop3_b32), so packing them costs no XOR.

Product 1 forms columns 128..271 of q1 mu and yields q3 = Barrett's quotient estimate or one less (q3 = -1,
from a numerator that the truncation bias took below 0, is clamped to 0 where q3 is used as a number; the
second reduction of a squaring / product folds its q3 straight into product 2's operand dwords); product 2 forms columns 0..129 of q3 P (as matrix columns 1..130, the constant
digit leading) and r = (T - q3 P) mod b^K exactly.
The digits stay within [0, 5P) as in fthe_padic_k37 (the bounds are asserted by the model).

Ops: those of gen_padic.py except the fixed-base table ops (LOADXGD / MULGD), which the host keeps on
fthe_padic_k37:  0 END, 1 LOADX, 2 STOREX, 3 SQR, 4 MUL, 22 LOADP, 23 STOREP.
ctx: [-P limbs (K, int32) ...] as for fthe_padic_k37, and the LDS tile image at byte 512 (20 KB).

Three bodies: fthe_padic_m37 (the default output, above); fthe_padic_m37t (top_est=True, for P of at most
TOPEST_MAX_BITS bits), whose product 2 in the reductions of SQR / MUL runs four M-tiles and takes r's bits above
1015 from product 1's fraction (see gen_padic_mfma's docstring), its ctx also holding Pt = P >> 1000 at byte PT_OFF;
and fthe_padic_m37s (top_est=True, q1_shift=8), the same with product 1's operand fed 8 bytes later, which empties
the four tiles with m - k = 1: 15 product-1 tiles, and the image of padic_tiles::build(P, 128, 8).
A fourth, fthe_padic_m37l (top_est=True, limb_op=True), feeds product 1 the radix-2^28 limbs of q1 as they lie -- no
repack into base-256 dwords, the tilted band in 15 tiles of their own: the 24 KB image of padic_tiles::build_limb(P).
A fifth, fthe_padic_m37k (m37l's arguments with mul_kara=True), forms MUL's cross term x0 y1 + x1 y0 by
one level of Karatsuba (kara_cross_mul).  Its second parameter fill0 (off in the table, switch fill0) runs the ripples
of both Karatsuba cross terms and MUL's copy of x0 y0's low half while tile 0 of the first quotient product sits in
the matrix core: each caller of .Lreduce issues that tile itself, its own fillers between the MFMAs, and enters the
shared reduction behind it.
BODIES and K_BODIES hold the five argument sets and gen_body(variant, ab) generates one by name; the A/B switches
(SWITCHES, and m37k's own K_SWITCHES) are the argument ab of either, parsed by parse_ab.
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_montprog import _descriptor  # noqa: E402

TILE_OFF = 512                  # byte offset of the tile image in ctx
TILE_BYTES = 20 * 1024          # 19 tiles of 1 KB, padded to 5 dwordx4 per thread
# product 1's window starts at column 128, not 112: the numerator stays within (Pi - 2^1047, Pi) of Pi = q1 mu
# (tools/padic_mfma_model.py), which is all Barrett asks, and the 16 columns no longer formed are M-tile 4's rows
# 16..31 (columns 272..287: zero), which its fold skips
S1_LO = 128                     # product-1 columns S1_LO .. S1_LO + 159 (the s1lo112 switch: 112, see s1_lo)
S1_TOP = 272                    # q1 mu has no column above 271
QBIT = 28 * 38                  # q3 = floor(N / 2^1064)
TILE_D1 = (-3, -2, -1, 0, 1)    # product-1 Toeplitz tiles (k <= 3) by m - k; then k = 4 for m = 0..4
TILE_D2 = (0, 1, 2, 3)          # product-2: k = 0 for m = 0..4 (tiles 10..14), then Toeplitz (k >= 1) by m - k

# A/B switches (the ab argument of gen_padic_mfma / gen_body: a comma-separated string or a set; tools/build_m37_ab.sh
# and FTHE_BUILD_OUT libraries only, fedtree_amd/build.py passes none to the in-tree library).  Each names what it
# turns off in the default schedule, or restores of an earlier one; the measurements are in DESIGN.md:
#   noswap, nonop, nomfma   timing only (wrong results): no accumulator exchange, no wait for the MFMAs, no MFMAs
#   nodbuf, nointerleave    one accumulator set; the next tile's MFMAs not spread through the fold
#   nopair, noprepair       columns not paired in 32-bit before the fold / before the exchange
#   nodesync                odd workgroups do not start late
#   prioN, noprio           s_setprio N (0..3, default 3) / none over the reduction
#   noprexor                the limbs that only feed the matrix cores are not produced with bit 7 of every operand
#                           byte already flipped (v_bitop3_b32 in place of the mask), so packing them costs a v_xor
#                           per dword: 128 more VALU per squaring (profiles/r03y_m37_prexor_ab.jsonl)
#   nocmerge                a chunk's carry is added in its tail, not in the next chunk's first multiply-add: 162 more
#                           VALU per squaring (profiles/r03za_m37_cmerge_ab.jsonl)
#   nokara                  a squaring's cross term as a plain product, not by Karatsuba (kara_cross below: +0.5%,
#                           profiles/r05i_m37_kara_ab.jsonl)
#   s1lo112                 product 1's window from column 112 (needs the image of padic_tiles::build(P, 112): the
#                           standalone harness and the emulator only)
#   noq3dw                  the second reduction's q3 as 28-bit limbs repacked by orpack, not folded straight into
#                           product 2's operand dwords
#   clampbr, noclampbr      Barrett 1's sign-keyed clamp (37 v_bitop3) behind a wave-uniform branch that skips it
#                           when no lane's numerator went negative (q1 = 0, or a tiny q1 at P near 2^1030), or not;
#                           the mask itself is always formed (the four-tile body's h reads it).  Default: BODIES
#   stamp                   timing build: each wave's start / end realtime and where it ran (tools/m37_stamps.py)
SWITCHES = ("noswap", "nonop", "nomfma", "nodbuf", "nointerleave", "nopair", "noprepair", "nodesync", "noprio",
            "noprexor", "nocmerge", "nokara", "s1lo112", "noq3dw", "clampbr", "noclampbr", "stamp")
PRIOS = tuple(f"prio{n}" for n in range(4))
# fthe_padic_m37k's own switches (K_BODIES below; the other bodies do not know them):
#   nomulkara               MUL's cross term as two plain products (product_cols), not kara_cross_mul
#   fill0, nofill0          tile 0 of every reduction's first quotient product issued by the caller, the ripples of the
#                           Karatsuba cross terms (MUL: and the copy of x0 y0's low half) between its MFMAs and in
#                           place of the three s_nop 7 before its exchange (fill_tile0), or not.  Default: K_BODIES
#                           (off: no clear gain)
K_SWITCHES = ("nomulkara", "fill0", "nofill0")


def parse_ab(ab, more=()):
    """the switch string (exact tokens between commas) or set -> frozenset of known switches (more: a body's own)"""
    toks = frozenset(t.strip() for t in ab.split(',') if t.strip()) if isinstance(ab, str) else frozenset(ab)
    unknown = sorted(toks - set(SWITCHES + PRIOS + tuple(more)))
    if unknown:
        known = SWITCHES + PRIOS + tuple(more)
        raise ValueError(f"unknown m37 switch {', '.join(unknown)}: known are {', '.join(known)}")
    for group in ({"clampbr", "noclampbr"}, {"noprio", *PRIOS}, {"fill0", "nofill0"}):
        if len(toks & group) > 1:
            raise ValueError(f"m37 switches {', '.join(sorted(toks & group))} contradict each other")
    return toks


def s1_lo(ab=""):
    """product 1's first column under the switches ab: the window the tile image must be built for"""
    return 112 if "s1lo112" in parse_ab(ab, K_SWITCHES) else S1_LO


def tile_index(prod, m, k, q1_shift=0, limb_op=False):
    """q1_shift (fthe_padic_m37s): no product-1 tile with m - k = 1; tile (0, 0), whose first q1_shift columns are
    the operand's pad, takes that slot (it is the only one formed with k = 0).
    limb_op (fthe_padic_m37l): the 15 product-1 tiles (k >= m) each have a slot, m-major; product 2's nine follow"""
    if limb_op:
        if prod == 1:
            assert k >= m
            return sum(5 - x for x in range(m)) + k - m
        return 15 + m if k == 0 else 20 + TILE_D2.index(m - k)
    if prod == 1:
        if q1_shift and k == 0:
            assert m == 0
            return 4
        return TILE_D1.index(m - k) if k <= 3 else 5 + m
    return 10 + m if k == 0 else 15 + TILE_D2.index(m - k)


# the four-tile body (gen_padic_mfma(name, top_est=True): fthe_padic_m37t): product 2 of the reductions of SQR / MUL
# forms bits 0..1015 of r only (M-tiles 0..3, K-blocks 0..3) and takes the rest of limb 36 from product 1's fraction
TOPEST_MAX_BITS = 1027          # the widest P the four-tile body admits (tools/padic_mfma_model.py asserts why)
PT_OFF = 400                    # ctx byte offset of Pt = P >> PT_SHIFT (bytes 312..511 are otherwise unused)
PT_SHIFT = 1000
TOPEST_C = 128 << 8             # the window constant c = 128 units of 2^1008, in units of 2^1000


Q1_SHIFT = 8                    # fthe_padic_m37s: q1's byte i is fed at K index i + Q1_SHIFT
LIMB_PAD = 1                    # fthe_padic_m37l: pad dwords in front of the 38 limbs of product 1's operand
TILE_BYTES_L = 24 * 1024        # its image: 15 product-1 tiles and product 2's nine

# the bodies: gen_padic_mfma's arguments, and whether Barrett 1's clamp sits behind a branch (clampbr / noclampbr)
BODIES = {
    "m37": dict(top_est=False, q1_shift=0, limb_op=False, clampbr=False),
    "m37t": dict(top_est=True, q1_shift=0, limb_op=False, clampbr=False),
    "m37s": dict(top_est=True, q1_shift=Q1_SHIFT, limb_op=False, clampbr=False),
    "m37l": dict(top_est=True, q1_shift=0, limb_op=True, clampbr=True),
}
# the fifth body, fthe_padic_m37k: m37l's arguments and two of its own.  It stands beside BODIES and SWITCHES, which
# name the four bodies that share every switch
K_BODIES = {"m37k": dict(BODIES["m37l"], mul_kara=True, fill0=False)}


def gen_body(variant: str, ab="") -> str:
    """the kernel fthe_padic_<variant> (a key of BODIES or K_BODIES) under the switches ab"""
    body = {k: v for k, v in {**BODIES, **K_BODIES}[variant].items() if k != "clampbr"}
    return gen_padic_mfma("fthe_padic_" + variant, ab=ab, **body)


def gen_padic_mfma(name: str, top_est: bool = False, q1_shift: int = 0, limb_op: bool = False,
                   mul_kara: bool = False, fill0: bool = False, ab="") -> str:
    """ab: A/B switches (SWITCHES above), a comma-separated string or a set.
    mul_kara, fill0 (with limb_op: fthe_padic_m37k): MUL's cross term by kara_cross_mul; the first tile of
    every reduction issued by the caller, its MFMAs spaced with the caller's independent VALU work (fill_tile0).
    limb_op (with top_est: fthe_padic_m37l): product 1 reads its B operands straight from the limbs
    T[36..73] (V[36..73] in the second reduction) behind LIMB_PAD pad dwords -- K index 4 (t + LIMB_PAD) + j is byte j
    of q1's limb t, fed as b ^ 0x80 for j < 3 and as it is for j = 3; the constant digit rides in byte 3 of limb 37
    (always zero: T < 2^2068) -- so no orpack and no copy precede product 1; the A image (tools/padic_mfma_model.py
    MfmaKey(P, limb_op=True)) absorbs the layout: 15 product-1 tiles of their own, 24 KB.  The first reduction's q3
    limbs land in XB (D[2..38]) and are packed in place for product 2; the second reduction's dwords in D[0..31].
    q1_shift = 8 (with top_est: fthe_padic_m37s): product 1's operand starts two dwords later -- q1 in D[2..35],
    the constant dword (digits 1 and 16 c, K indices 144 and 145) in D[36] -- so that A1[s][i] = mu'[s - i + 8] and
    the sub-diagonal tiles (m - k = 1: s - i + 8 >= 137, above mu's last digit 133) are zero and are not formed: 15
    tiles instead of 19, every column sum unchanged.  The A columns of K indices 0..7 and 146..159 are
    zero, so D[0], D[1] and D[37..39] are never written: whatever they hold meets zeros.
    top_est: the four-tile body.  In the reductions of SQR and MUL product 2 runs M-tiles 0..3 only (K-blocks
    0..3 of the operand: 20 MFMAs instead of 30), which give r mod 2^1016 exactly, and bits 1016.. of r follow from
    f = frac(N / 2^1064), the guard bits product 1's fold passes through anyway: r = P (f + e) with
    0 <= e P < 2^1015, so with E = floor(f32 Pt / 2^32) (units of 2^1000) and b = bits 1008..1015 of r,
    limb 36 = b | ((E + c - 256 b) >> 16) << 8  (derivation, bounds and slack: tools/padic_mfma_model.py).
    Contract: P of at most TOPEST_MAX_BITS bits; the digits SQR and MUL read (from LOADP, LOADX of a STOREX, or
    the raw digits of a slot) are below 3P -- 2P plus room for P just above 2^1008, where a digit may leave a
    little above 2P -- and the digits they leave are below P + 2^1015 (< 3P, < P + 2^1016).  LOADP's input is a
    plain residue below 3 P^2 (x1 = its quotient); its own reduction keeps the five-tile product 2."""
    K, B = 37, 28
    MASK = (1 << B) - 1
    flags = dict(top_est=top_est, q1_shift=q1_shift, limb_op=limb_op, mul_kara=mul_kara, fill0=fill0)
    body = [b for b in {**BODIES, **K_BODIES}.values() if all(b.get(k, False) == v for k, v in flags.items())]
    assert body, f"{flags}: not one of BODIES (limb_op and q1_shift = {Q1_SHIFT} need top_est and exclude each other)"
    ab = parse_ab(ab, K_SWITCHES if mul_kara or fill0 else ())

    def refuse(sw, why):
        if sw in ab:
            raise ValueError(f"{name}: switch {sw} refused: {why}")
    if q1_shift or limb_op:
        refuse("s1lo112", f"the 15-tile image of the {'limb-fed' if limb_op else 'shifted'} operand exists for the "
               f"window from column {S1_LO} only")
    if limb_op:
        refuse("noprexor", "product 1 reads the limbs as they lie, so they must leave the column tails flipped")
        refuse("noq3dw", "V[36..73] is product 1's operand, so the second q3 has no limbs to land in")
    PREXOR, CMERGE, KARA, Q3DW = (sw not in ab for sw in ("noprexor", "nocmerge", "nokara", "noq3dw"))
    MULKARA = mul_kara and "nomulkara" not in ab
    FILL0 = "fill0" in ab or (fill0 and "nofill0" not in ab)
    assert not (MULKARA and not KARA), "kara_cross_mul keeps its constants where kara_cross does (s76..s78)"
    s1lo = s1_lo(ab)                             # product-1 columns s1lo .. s1lo + 159
    CLAMPBR = "clampbr" in ab or (body[0]["clampbr"] and "noclampbr" not in ab)
    # VALU instructions kept between a tile's last MFMA and the lane exchange that reads its results (>= 24: the
    # 8-pass XDL -> VALU hazard then needs no s_nop; 24..90 within noise, profiles/r03zj_m37_margin_ab.jsonl)
    MARGIN = 30
    tile_bytes = TILE_BYTES_L if limb_op else TILE_BYTES
    QD = q1_shift // 4                           # the operand's first dword
    # ---- VGPR plan ---------------------------------------------------------
    V_TID, V_GOFF = 0, 1
    VA = (2, 6, 10)                              # A-tile buffers v[2:5], v[6:9], v[10:13] (ACC is free)
    # product columns: NCOL adjacent columns side by side (one 64-bit accumulator chain each), two column
    # sets (the tails of one set run inside the next set's multiply-adds)
    NCOL = 2
    ACC0 = 10                                    # v[ACC0 .. ACC0 + 4 NCOL)
    CARRY = ACC0 + 4 * NCOL
    XA = 20                                      # x0 digit (v20..v56); Barrett: accumulators v20..v51
    G0, G1 = XA, XA + 16
    # Barrett scratch in XA above the accumulators: chunk sums v[52:55], clamp mask v56, chunk carry v[58:59]
    XB = 60                                      # x1 digit (v60..v96); Barrett: operand dwords D0..D39
    TT = 100                                     # T limbs v100..v173
    VV = 174                                     # V limbs v174..v247
    V_LDS = 248                                  # (lane & 63) * 16
    PATV = (249, 250)                            # PREXOR: byte-flip patterns of even / odd limbs
    NVGPR = 251 if PREXOR else 249
    if limb_op:
        # T[36..73] and V[36..73] are product 1's operand blocks: each sits between two pad registers (v136 / v175,
        # v212 / v251) that the lane exchange may swap freely, 40 consecutive registers from an even one
        VV = TT + 2 * K + 2
        V_LDS = VV + 2 * K + 2
        PATV = (V_LDS + 1, V_LDS + 2)
        NVGPR = V_LDS + 3 + MULKARA              # kara_cross_mul takes the last register as a temporary
        assert NVGPR <= 256
    L36 = "v14"                                  # limb_op: the unflipped copy of limb 36 (the remainder's init)

    def pat(t):
        """flip pattern of limb t of a packed number (limb t at bit 28 t): bits j with 28 t + j = 7 mod 8"""
        return f"v{PATV[t % 2]}"
    PATVAL = (0x00808080, 0x08080808)
    X0 = [f"v{XA + i}" for i in range(K)]
    X1 = [f"v{XB + i}" for i in range(K)]
    T = [f"v{TT + i}" for i in range(2 * K)]
    V = [f"v{VV + i}" for i in range(2 * K)]
    if limb_op:
        lay = lambda base: [f"v{base + i + (i >= K - 1)}" for i in range(2 * K)]
        blk = lambda base: [f"v{base + K - 1 + i}" for i in range(40)]
        T, V = lay(TT), lay(VV)
        OPB = {id(T): blk(TT), id(V): blk(VV)}   # pad, limbs 36..73, pad
        assert OPB[id(T)][LIMB_PAD:LIMB_PAD + K + 1] == T[K - 1:] and OPB[id(V)][LIMB_PAD:LIMB_PAD + K + 1] == V[K - 1:]

    def pxu(c):
        """flip pattern that limb c >= K of a product leaves its column tail with (PREXOR): as a byte of q1 packed
        from limb K - 1 on, or (limb_op) bytes 0..2 of the limb itself, the top limb also taking the constant digit 1
        into its byte 3 (a literal: its tail is a v_xor_b32_e32)"""
        if limb_op:
            return "0x1808080" if c == 2 * K - 1 else f"v{PATV[0]}"
        return pat(c - (K - 1))
    D = [f"v{XB + i}" for i in range(40)]
    # ---- SGPR plan ---------------------------------------------------------
    # s[0:1] kernarg, s2 wg id, s[2:3] call target, s[4:5] slots, s[6:7] prog, s[8:9] ctx, s10 limb
    # stride, s11 slot stride, s[12:13] return address, s[14:15] op/arg, s[16:17] addr, s19 counter;
    # s20..s27 = 2^0, 2^4, .., 2^28; s28..s34 = -2^0, .., -2^24; -P limbs from s36
    SPOW, SNEG, SNP = 20, 28, 36                   # s35 = 0x0fffffff
    NSGPR = SNP + K
    if KARA:                                     # s76..s78: 2, 3, 4 x mask
        NSGPR = 79
    SPT = NSGPR                                  # top_est: Pt = P >> 1000
    if top_est:
        NSGPR += 1
    POW = lambda sh: f"s{SPOW + sh // 4}"
    NEG = lambda sh: f"s{SNEG + sh // 4}"
    NP = lambda j: f"s{SNP + j}"

    def pair(n):
        return f"v[{n}:{n + 1}]"

    def acc(s, ch):
        n = ACC0 + 2 * (NCOL * s + ch)
        return f"v[{n}:{n + 1}]"

    def acclo(s, ch):
        return f"v{ACC0 + 2 * (NCOL * s + ch)}"

    carry = pair(CARRY)
    o = []
    sink = [o]                                   # capture() redirects the emitter into a side list

    def e(line):
        sink[-1].append(line)

    def capture(fn):
        sink.append([])
        try:
            fn()
        finally:
            out = sink.pop()
        return out

    # ---- column engine (product scanning, two adjacent columns side by side) --------------------
    def columns(cols, signed=False, carry_in=False, bg=()):
        """product scanning over cols (dicts): 'terms' [(a, b)] multiply-adds, 'dbl' (column x 2), 'sq' (one
        more x*x after the doubling), 'out' (the limb register), 'px' (flip pattern of a pre-XORed limb), 'cpl'
        (store mask - limb), 'last' (no mask, no carry), 'addend' (a register pair with a zero high dword: the
        first multiply-add's addend), 'pre' (instructions that must precede the column's first multiply-add:
        emitted during the previous group's multiply-adds).  carry_in: the carry register holds column 0's
        carry.  bg: independent instructions spread over the multiply-adds (one per two while no tail is
        pending), the rest emitted at the end."""
        mad = 'v_mad_i64_i32' if signed else 'v_mad_u64_u32'
        shr = 'v_ashrrev_i64' if signed else 'v_lshrrev_b64'
        pending = []
        bgq = list(bg)

        def flush(n):
            for _ in range(min(n, len(pending))):
                e(pending.pop(0))

        def tick():
            if pending:
                flush(1)
            elif bgq:
                e(bgq.pop(0))

        def tail_of(ci, col, a0, lo0, used):
            t = []
            first = ci == 0 and not carry_in
            if not used:
                if col.get('addend'):
                    t.append(f'  v_lshl_add_u64 {a0}, {col["addend"]}, 0, {"0" if first else carry}')
                else:
                    t.append(f'  v_mov_b64_e32 {a0}, {"0" if first else carry}')
            elif col.get('dbl'):
                t.append(f'  v_lshl_add_u64 {a0}, {a0}, 1, {"0" if first else carry}')
            elif not first:
                t.append(f'  v_lshl_add_u64 {a0}, {a0}, 0, {carry}')
            if col.get('sq'):
                x = col['sq']
                t.append(f'  {mad} {a0}, vcc, {x}, {x}, {a0}')
            if col.get('out') is not None:
                px = col.get('px')
                if col.get('cpl'):                           # mask - limb (the top limb: < 2^28 asserted by
                    assert not px                            # the model, so the XOR is the same)
                    if col.get('last'):
                        t.append(f'  v_xor_b32_e32 {col["out"]}, {SMASK}, {lo0}')
                    else:
                        t.append(f'  v_bitop3_b32 {col["out"]}, {lo0}, {SMASK}, {lo0} bitop3:0xc')
                elif col.get('last'):
                    if px:
                        t.append(f'  v_xor_b32_e32 {col["out"]}, {px}, {lo0}')
                    else:
                        t.append(f'  v_mov_b32_e32 {col["out"]}, {lo0}')
                elif px:                                     # (lo & mask) ^ pattern
                    t.append(f'  v_bitop3_b32 {col["out"]}, {lo0}, {SMASK}, {px} bitop3:0x6a')
                else:
                    t.append(f'  v_and_b32_e32 {col["out"]}, {hex(MASK)}, {lo0}')
            if not col.get('last') and not col.get('nocarry'):
                t.append(f'  {shr} {carry}, {B}, {a0}')
            return t

        for ci in range(min(NCOL, len(cols))):
            for ins in cols[ci].get('pre', ()):
                e(ins)
        for gi in range(0, len(cols), NCOL):
            s = (gi // NCOL) % 2
            members = list(range(gi, min(gi + NCOL, len(cols))))
            seqs = [(acc(s, m), cols[ci]['terms'], cols[ci].get('addend')) for m, ci in enumerate(members)]
            used = [False] * len(seqs)
            for ci in range(gi + NCOL, min(gi + 2 * NCOL, len(cols))):
                pending += list(cols[ci].get('pre', ()))
            n = 0
            for t in range(max(len(q[1]) for q in seqs)):
                for k, (ac, terms, add) in enumerate(seqs):
                    if t < len(terms):
                        a_, b_ = terms[t]
                        e(f'  {mad} {ac}, vcc, {a_}, {b_}, {ac if used[k] else (add or "0")}')
                        used[k] = True
                        n += 1
                        if n % 2 == 0:
                            tick()
            flush(len(pending))
            tail = []
            for m, ci in enumerate(members):
                tail += tail_of(ci, cols[ci], acc(s, m), acclo(s, m), used[m])
            pending = tail
        flush(len(pending))
        for ins in bgq:
            e(ins)

    def product_cols(a, b, n_out, outs, a2=None, b2=None):
        cols = []
        for c in range(n_out):
            terms = []
            for i in range(len(a)):
                j = c - i
                if 0 <= j < len(b):
                    terms.append((a[i], b[j]))
                    if a2 is not None:
                        terms.append((a2[i], b2[j]))
            cols.append({'terms': terms, 'out': outs[c], 'last': c == n_out - 1})
            if PREXOR and c >= K:                      # the upper half only feeds Barrett's q1 bytes
                cols[-1]['px'] = pxu(c)
        return cols

    def move(dst, src):
        n = len(src)
        for i in range(0, n - 1, 2):
            if int(dst[i][1:]) % 2 == 0 and int(src[i][1:]) % 2 == 0:
                e(f'  v_pk_mov_b32 {pair(int(dst[i][1:]))}, {pair(int(src[i][1:]))}, {pair(int(src[i][1:]))} op_sel:[0,1]')
            else:
                e(f'  v_mov_b32_e32 {dst[i]}, {src[i]}')
                e(f'  v_mov_b32_e32 {dst[i + 1]}, {src[i + 1]}')
        if n % 2:
            e(f'  v_mov_b32_e32 {dst[n - 1]}, {src[n - 1]}')

    # ---- matrix-core Barrett -------------------------------------------------
    CACC2 = (pair(XA + 32), pair(XA + 34))      # chunk sums, alternating by chunk parity: v[52:53], v[54:55]
    CCARRY = pair(XA + 38)                      # chunk carry v[58:59]
    SMASK = "s35"                               # 0x0fffffff (v_bfi_b32 operand)
    S2MASK, S3MASK, S4MASK = "s76", "s77", "s78"  # KARA: 2, 3, 4 x 0x0fffffff

    def orpack(limbs, shift_bits, ndw, xor_masks, lead_one=False, norm0=False, pre=(), d0=0):
        """normalised 28-bit limbs (limb t at bit 28 t + shift_bits) -> dwords D[0..ndw-1] XOR xor_masks[w],
        each dword from the (at most two) limbs it overlaps: no carry chain.  lead_one: byte 0 is the
        constant digit 1 (shift_bits = 8).  norm0: limb 0 may hold a bit 28 (masked off here).  pre: the
        limbs already XORed with pat(t) (PREXOR); only the flips they do not carry are applied here.  d0: the
        dwords go to D[d0 ..]."""
        n = len(limbs)
        pre = set(pre)

        def carried(w):
            """bits of dword w already flipped by pre-XORed limbs"""
            m = 0
            for b in range(32):
                q = 32 * w - shift_bits + b                   # bit of the packed number
                if q < 0 or (lead_one and w == 0 and b < 8):
                    continue
                t, j = q // B, q % B
                if t in pre and t < n and (PATVAL[t % 2] >> j) & 1:
                    m |= 1 << b
            return m
        xor_masks = [xor_masks[w] ^ carried(w) for w in range(ndw)]
        for w in range(ndw):
            d = D[w + d0]
            if lead_one and w == 0:
                e(f'  v_lshl_or_b32 {d}, {limbs[0]}, 8, 1')
            else:
                lo = (32 * w - shift_bits) // B
                off = 32 * w - shift_bits - B * lo
                hi_ok = lo + 1 < n
                if norm0 and lo == 0:
                    assert off == 0 and hi_ok
                    e(f'  v_lshlrev_b32_e32 {d}, 28, {limbs[1]}')
                    e(f'  v_bfi_b32 {d}, {SMASK}, {limbs[0]}, {d}')
                elif not hi_ok:
                    e(f'  v_lshrrev_b32_e32 {d}, {off}, {limbs[lo]}')
                elif off == 0:
                    e(f'  v_lshl_or_b32 {d}, {limbs[lo + 1]}, 28, {limbs[lo]}')
                else:
                    e(f'  v_lshrrev_b32_e32 {d}, {off}, {limbs[lo]}')
                    e(f'  v_lshl_or_b32 {d}, {limbs[lo + 1]}, {B - off}, {d}')
            if xor_masks[w]:
                e(f'  v_xor_b32_e32 {d}, {hex(xor_masks[w])}, {d}')

    # the second reduction's product-2 operand block (Q3DW): dwords 0..35 in V[38..73] (its q1 limbs, dead once
    # packed), 36..39 in the product phase's accumulators v16..v19
    D2 = [f"v{VV + 38 + i}" for i in range(36)] + [f"v{16 + i}" for i in range(4)]
    if limb_op:                                 # V[36..73] is product 1's operand: the dwords go to XB
        D2 = D
    OPND = [D]                                  # the block the MFMAs read their B operands from

    def swap_operands(Dl=D, nk=5):
        e('  s_nop 1')
        for k in range(nk):
            for j in range(4):
                e(f'  v_permlane32_swap_b32_e32 {Dl[8 * k + j]}, {Dl[8 * k + 4 + j]}')
        e('  s_nop 4')

    def rd(prod, m, k, n):
        b_ = VA[n % 3]
        e(f'  ds_read_b128 v[{b_}:{b_ + 3}], v{V_LDS} offset:{1024 * tile_index(prod, m, k, q1_shift, limb_op)}')

    def prefetch(prod, m, ks):
        """the first two A-tile reads of M-tile m (issued while the lane still has VALU work)"""
        for n in range(min(2, len(ks))):
            rd(prod, m, ks[n], n)

    GB0, GB1 = TT + 38, TT + 54                  # second accumulator set v[138:153], v[154:169] (T[38..69])

    def issue_tile(prod, m, ks, G0x, G1x, prefetched=True):
        """the MFMAs of M-tile m over K-tiles ks (both lane groups) into accumulators G0x, G1x; with
        prefetched its first two A-tile reads are already in flight, the rest rotate through three
        buffers one step ahead"""
        L = len(ks)
        if not prefetched:
            prefetch(prod, m, ks)
        for n, k in enumerate(ks):
            if n + 2 < L:
                rd(prod, m, ks[n + 2], n + 2)
            e(f'  s_waitcnt lgkmcnt({min(L, n + 3) - n - 1})')
            buf = VA[n % 3]
            for g, G in ((0, G0x), (1, G1x)):
                src_c = "0" if n == 0 else f"v[{G}:{G + 15}]"
                bo = 8 * k + 4 * g
                b0 = int(OPND[0][bo][1:])
                assert b0 % 2 == 0 and [int(r[1:]) for r in OPND[0][bo:bo + 4]] == list(range(b0, b0 + 4))
                if "nomfma" not in ab:
                    e(f'  v_mfma_i32_32x32x32_i8 v[{G}:{G + 15}], v[{buf}:{buf + 3}], v[{b0}:{b0 + 3}], {src_c}')

    P1_TOP = [S1_TOP]                            # product 1: the fold reads the columns below this

    def consumed(prod, m):
        """the rows (output columns rho of M-tile m) the fold reads: product 1 those below P1_TOP (272: the
        product's last column, or what the dword fold needs); product 2 drops matrix column 0 (the constant
        digit's) and the columns above 130"""
        if prod == 1:
            return {rho for rho in range(32) if s1lo + 32 * m + rho < P1_TOP[0]}
        return {rho for rho in range(32) if 1 <= 32 * m + rho <= 130}

    def plan(C):
        """accumulator register rr holds row 8 (rr >> 2) + 4 h + (rr & 3) of the lane half h, i.e. output
        column rho_a = 8 (rr >> 2) + (rr & 3) or rho_a + 4 after the exchange.  Even rr whose two rows are both
        read (or both unread) in both halves are paired before the exchange, c_rho + 256 c_(rho+1) in 32-bit
        arithmetic (|c| < 2^21.2: exact), so the odd register need not move; returns (paired even rr, the rr
        to exchange)"""
        paired, swaps = set(), []
        for rr in range(0, 16, 2):
            ra = 8 * (rr >> 2) + (rr & 3)
            rhos = (ra, ra + 4)
            if "noprepair" not in ab and all((r in C) == (r + 1 in C) for r in rhos) \
                    and any(r in C for r in rhos):
                paired.add(rr)
        for rr in range(16):
            ra = 8 * (rr >> 2) + (rr & 3)
            if (ra in C or ra + 4 in C) and not (rr % 2 and rr - 1 in paired):
                swaps.append(rr)
        return paired, swaps

    def exchange(G0x, G1x, waited=False, tile=None):
        """results -> VALU: wait out the last MFMA writing them (8-pass XDL: 11 wait states on gfx950), pair
        adjacent rows (plan), then exchange the halves of the registers still needed; waited: at least 30
        VALU instructions already separate that MFMA from here"""
        if "nonop" not in ab and not waited:
            e('  s_nop 7')
            e('  s_nop 7')
            e('  s_nop 7')
        paired, swaps = plan(consumed(*tile))
        for rr in sorted(paired):
            for G in (G0x, G1x):
                e(f'  v_lshl_add_u32 v{G + rr}, v{G + rr + 1}, 8, v{G + rr}')
        if paired:
            e('  s_nop 1')
        for rr in (swaps if "noswap" not in ab else []):
            e(f'  v_permlane32_swap_b32_e32 v{G0x + rr}, v{G1x + rr}')
        e('  s_nop 1')

    def tile_cols(prod, m, s_of, creg):
        """(output column, register, pre-paired) of M-tile m in column order, after exchange()"""
        C = consumed(prod, m)
        paired, _ = plan(C)
        out = []
        for rho in sorted(C):
            rr = (rho & 3) + 4 * (rho >> 3)
            if rho % 2 and rr - 1 in paired:
                continue                              # folded into rho - 1 before the exchange
            out.append((s_of(rho), creg(rho), rho % 2 == 0 and rr in paired))
        return out

    def mtile_mfmas(prod, m, ks, nxt=None):
        """one M-tile, issued and then waited for (single accumulator set)"""
        issue_tile(prod, m, ks, G0, G1)
        if nxt is not None:
            prefetch(*nxt)
        exchange(G0, G1, tile=(prod, m))

    def col_reg(rho, G0x=G0, G1x=G1):
        """register of column rho (0..31) of the M-tile after the exchange"""
        rr = (rho & 3) + 4 * (rho >> 3)
        return f"v{(G1x if (rho >> 2) & 1 else G0x) + rr}"

    def fill_tile0(tile, work, nxt):
        """fill0: tile 0 of the first product 1 (one accumulator set: nothing of the reduction can run beside it) with
        the caller's independent instructions (work) between its MFMAs -- the wave would issue nothing while the
        matrix core takes them one after another -- and the last MARGIN of them behind the last MFMA, where three
        s_nop 7 stood (they stand there still if work is shorter).  What follows is the callers' shared text: the
        label .Lreduce ends the part each caller issues itself."""
        issue = capture(lambda: issue_tile(*tile, G0, G1))
        fill = capture(work)
        banned = set(range(G0, G0 + 32)) | {int(r[1:]) for r in OPND[0]} | set(range(VA[0], VA[2] + 4)) | {int(L36[1:])}
        for ins in fill:                         # reordering only: nothing tile 0 or the head before it touches
            regs = {int(r) for r in re.findall(r'\bv(\d+)\b', ins)}
            for lo, hi in re.findall(r'\bv\[(\d+):(\d+)\]', ins):
                regs |= set(range(int(lo), int(hi) + 1))
            assert ins.lstrip().startswith('v_') and not regs & banned, f"fill0: {ins.strip()} meets tile 0's registers"
        n_mf = sum('v_mfma' in ins for ins in issue)
        tail = len(fill) if n_mf == 0 else MARGIN if len(fill) >= MARGIN else 0
        head = fill[:len(fill) - tail]
        gaps = max(1, n_mf - 1)
        seen = 0
        for ins in issue:
            e(ins)
            if 'v_mfma' in ins and seen < gaps:
                for x in head[seen * len(head) // gaps:(seen + 1) * len(head) // gaps]:
                    e(x)
                seen += 1
        prefetch(*nxt)
        for x in fill[len(fill) - tail:]:
            e(x)
        if tail < MARGIN and "nonop" not in ab:
            for _ in range(3):
                e('  s_nop 7')
        e('.Lreduce:')

    def run_tiles(tiles, consume, nxt, dbuf, after_issue0=None):
        """all M-tiles of a product: consume(m, col_reg_of_the_tile) after each; dbuf: two accumulator sets,
        tile m+1's MFMAs issued before tile m's results are folded, so the matrix core works while the
        lane does (needs T[38..69] free); tile 0's first A tiles are prefetched by the caller"""
        nt = len(tiles)
        if not dbuf:
            for m in range(nt):
                if m == 0 and after_issue0 is not None:
                    fill_tile0(tiles[0], after_issue0, tiles[1])
                    exchange(G0, G1, waited=True, tile=tuple(tiles[0][:2]))
                else:
                    mtile_mfmas(*tiles[m], nxt=tiles[m + 1] if m < nt - 1 else nxt)
                consume(m, col_reg)
            return
        sets = ((G0, G1), (GB0, GB1))
        issue_tile(*tiles[0], *sets[0])
        separated = False                        # >= 30 VALU instructions after this tile's last MFMA
        if after_issue0 is not None:             # independent VALU work while tile 0 runs
            work = capture(after_issue0)
            for ins in work:
                e(ins)
            separated = len(work) >= MARGIN
        for m in range(nt):
            if m < nt - 1:
                nxt_issue = capture(lambda: issue_tile(*tiles[m + 1], *sets[(m + 1) % 2], prefetched=False))
            else:
                nxt_issue = capture(lambda: prefetch(*nxt)) if nxt is not None else []
            ga, gb = sets[m % 2]
            # tiles after the first were issued inside the previous fold, whose last 40% has no MFMA
            exchange(ga, gb, waited=separated, tile=tuple(tiles[m][:2]))
            fold = capture(lambda: consume(m, lambda rho, ga=ga, gb=gb: col_reg(rho, ga, gb)))
            if "nointerleave" in ab:
                for ins in nxt_issue + fold:
                    e(ins)
                separated = False
                continue
            # the next tile's reads and MFMAs spread through this tile's fold: an in-order wave waiting to
            # issue its next MFMA issues nothing else, so the MFMAs go out between VALU instructions
            items, grp = [], []
            for ins in nxt_issue:
                grp.append(ins)
                if "v_mfma" in ins or "ds_read" in ins:
                    items.append(grp)
                    grp = []
            if grp:
                items.append(grp)
            room = len(fold) - MARGIN              # the MFMAs go before the last MARGIN instructions of the fold
            gap = max(1, room // (len(items) + 1)) if items else 0
            separated = items != [] and len(fold) - gap * len(items) >= MARGIN
            k = 0
            for i, ins in enumerate(fold):
                if items and k < len(items) and i % gap == 0:
                    for x in items[k]:
                        e(x)
                    k += 1
                e(ins)
            for grp in items[k:]:
                for x in grp:
                    e(x)

    class Chunks:
        """column sums -> 28-bit limbs.  Chunk t (bits [base + 28 t, +28)) sums its columns (x 2^sh) into its
        own accumulator (two, alternating), independent of the carry; its tail (+ carry, mask, carry out)
        is deferred into the next chunk's multiply-adds, so the carry chain never stalls the wave.
        radix / out: chunks of radix bits whose low dword leaves through out(t, register) -> instructions
        (the dword fold) instead of a masked limb in outs[t].  tap: {t: register -> instructions} run on chunk
        t's low dword beside its limb (top_est: the fraction below QBIT)."""

        def __init__(self, base_bits, t0, t_last, outs, neg, inits=None, nocarry_last=False, px=False,
                     radix=B, out=None, tap=None):
            self.tap = tap or {}
            self.base, self.t, self.t0, self.t_last, self.outs, self.neg = base_bits, t0, t0, t_last, outs, neg
            self.inits, self.nocarry_last, self.px = inits, nocarry_last, px
            self.radix, self.out = radix, out
            self.pending = []
            self.fresh = True
            self.begun = False

        def acc(self):
            return CACC2[(self.t - self.t0) & 1]

        def emit(self, ins):
            e(ins)
            if self.pending:
                e(self.pending.pop(0))

        def addend0(self):
            """addend of a chunk's first multiply-add: the previous chunk's carry under CMERGE"""
            return CCARRY if CMERGE and self.t != self.t0 else "0"

        def start(self):
            if self.inits is not None and 0 <= self.t < len(self.inits):
                self.emit(f'  v_mad_u64_u32 {self.acc()}, vcc, {self.inits[self.t]}, 1, {self.addend0()}')
                self.fresh = False

        def close(self):
            for ins in self.pending:
                e(ins)
            a = self.acc()
            tail = []
            if self.t != self.t0 and not CMERGE:
                tail.append(f'  v_lshl_add_u64 {a}, {a}, 0, {CCARRY}')
            if self.t in self.tap:
                tail += self.tap[self.t](f'v{a[2:a.index(":")]}')
            if self.out is not None:
                tail += self.out(self.t, f'v{a[2:a.index(":")]}')
            elif 0 <= self.t < len(self.outs):
                if self.px:                              # q3 limbs leave pre-flipped (PREXOR)
                    tail.append(f'  v_bitop3_b32 {self.outs[self.t]}, v{a[2:a.index(":")]}, {SMASK}, '
                                f'{pat(self.t)} bitop3:0x6a')
                else:
                    tail.append(f'  v_and_b32_e32 {self.outs[self.t]}, {hex(MASK)}, v{a[2:a.index(":")]}')
            if not (self.nocarry_last and self.t == self.t_last):
                if CMERGE:                               # the next chunk's first multiply-add reads it
                    e(f'  v_ashrrev_i64 {CCARRY}, {self.radix}, {a}')
                else:
                    tail.append(f'  v_ashrrev_i64 {CCARRY}, {self.radix}, {a}')
            self.pending = tail
            self.t += 1
            self.fresh = True
            if self.t <= self.t_last:
                self.start()

        def column(self, s, reg):
            t = (8 * s - self.base) // self.radix
            while t > self.t:
                self.close()
            if not self.begun:
                self.begun = True
                self.start()
            sh = 8 * s - self.base - self.radix * t
            mul = NEG(sh) if self.neg else POW(sh)
            a = self.acc()
            self.emit(f'  v_mad_i64_i32 {a}, vcc, {reg}, {mul}, {self.addend0() if self.fresh else a}')
            self.fresh = False

        def finish(self):
            while self.t <= self.t_last:
                self.close()
            for ins in self.pending:
                e(ins)
            self.pending = []

    def fold_columns(ch, cols):
        """cols: [(s, reg, paired)] of one tile in column order (paired: reg already holds c_s + 256 c_(s+1),
        formed before the exchange).  Two adjacent unpaired columns of the same chunk whose shifts are sh
        and sh + 8 <= 24 are combined first, c_s + 256 c_(s+1) in 32-bit arithmetic (|c| < 2^21.2, so |sum| <
        2^29.3: exact), and enter the chunk as one v_mad_i64_i32: ~2 instead of 3.5 64-bit multiply-adds per
        28-bit chunk.  A pair whose second column lies in the next chunk enters this chunk at shift sh <= 24:
        its bits above 28 leave through the chunk's carry, exactly."""
        i = 0
        while i < len(cols):
            s_, r_, pr_ = cols[i]
            if not pr_ and i + 1 < len(cols) and "nopair" not in ab:
                s2_, r2_, pr2_ = cols[i + 1]
                t1, t2 = (8 * s_ - ch.base) // ch.radix, (8 * s2_ - ch.base) // ch.radix
                if not pr2_ and s2_ == s_ + 1 and t1 == t2 and 8 * s_ - ch.base - ch.radix * t1 <= 16:
                    e(f'  v_lshl_add_u32 {r_}, {r2_}, 8, {r_}')
                    ch.column(s_, r_)
                    i += 2
                    continue
            ch.column(s_, r_)
            i += 1

    P1_TILES = [(1, m, [k for k in range(5) if m - k <= (0 if q1_shift or limb_op else 1)]) for m in range(5)]
    P2_TILES = [(2, m, [k for k in range(5) if m >= k]) for m in range(5)]

    V_FRAC = XA + 37                            # top_est: f32, the 32 bits of N below QBIT (v57)
    assert V_FRAC not in range(G0, G0 + 32) and V_FRAC not in range(XA + 32, XA + 37) and \
        V_FRAC not in (XA + 38, XA + 39) and V_FRAC < XB and V_FRAC >= CARRY + 2 and V_FRAC not in VA

    nclamp = [0]

    def mfma_barrett(Tl, q3out, clamp, prefetched=False, dbuf=False, pre_in=None, dw=None, t4=False, fill=None):
        """product 1: q3 = Barrett's quotient of T (Tl: 2K limbs, Tl[K-1] < 2^29 allowed) -> q3out (K regs,
        may be Tl[K:]); clamp: q3 = -1 (numerator < 0: q1 = 0, or a small q1 at P near 2^1030) -> 0; prefetched: its first A-tile reads are in flight;
        dbuf: double-buffered accumulators (T[38..69] free); pre_in: Tl[K..2K-1] arrive pre-flipped
        (PREXOR, default); q3out leaves pre-flipped under PREXOR.
        dw (no clamp): q3 mod b^K leaves as product 2's operand dwords dw[0..32] instead (byte 0 the constant
        digit 1, the others b ^ 0x80; tools/padic_mfma_model.py fold_dwords); may overlap Tl[K..]
        t4 (top_est): f32 -> V_FRAC for the four-tile product 2, which reads operand dwords 0..31 only: the dword
        fold ends at dword 31
        fill (fill0, no dbuf): the caller's independent work for tile 0 (fill_tile0)"""
        if pre_in is None:
            pre_in = PREXOR
        if not prefetched:
            prefetch(*P1_TILES[0])
        if limb_op:
            # the limbs are the operand: limb 36 (not pre-flipped: the remainder's init, copied) is flipped in
            # place; its byte 3 (bit 28 included) and the others' are valid i8 as they are
            e(f'  v_mov_b32_e32 {L36}, {Tl[K - 1]}')
            e(f'  v_xor_b32_e32 {Tl[K - 1]}, v{PATV[0]}, {Tl[K - 1]}')
            if not pre_in:                                          # LOADP: plain limbs
                for t in range(K, 2 * K):
                    e(f'  v_xor_b32_e32 {Tl[t]}, {pxu(t)}, {Tl[t]}')
            swap_operands(OPB[id(Tl)])
            OPND[0] = OPB[id(Tl)]
        else:
            orpack(Tl[K - 1:2 * K], 0, 34, [0x80808080] * 34, norm0=True, pre=range(1, K + 1) if pre_in else (), d0=QD)
            DC = D[34 + QD]
            e(f'  v_bfe_u32 {DC}, {Tl[K - 1]}, 28, 1')                  # c = bit 28 of q1[0] -> digit 16 c at byte 137
            e(f'  v_lshl_or_b32 {DC}, {DC}, 12, 1')                     # and the constant digit 1 at byte 136
            if not q1_shift:                                            # q1_shift: the pads meet zero A columns
                for w in range(35, 40):
                    e(f'  v_mov_b32_e32 {D[w]}, 0')
            swap_operands()
        if dw is None:
            # chunk -1 is bits 1036..1063 of N: f32 = its 28 bits over four zeros
            tap = {-1: lambda lo: [f'  v_lshlrev_b32_e32 v{V_FRAC}, 4, {lo}']} if t4 else None
            ch = Chunks(QBIT, (8 * s1lo - QBIT) // B, 39, q3out, neg=False, px=PREXOR, tap=tap)
        else:
            assert not clamp
            base = QBIT - 8                                          # dw[0]'s byte 0 is the constant digit

            ndw = 32 if t4 else 33
            # chunk -1 is bits 1024..1055 of N, chunk 0's low byte bits 1056..1063: f32 = bits 1032..1063
            tap = {-1: lambda lo: [f'  v_mov_b32_e32 v{V_FRAC}, {lo}'],
                   0: lambda lo: [f'  v_alignbit_b32 v{V_FRAC}, {lo}, v{V_FRAC}, 8']} if t4 else None

            def out(w, lo):
                if w < 0:
                    return []
                if w == 0:
                    return [f'  v_and_b32_e32 {dw[0]}, 0xffffff00, {lo}', f'  v_xor_b32_e32 {dw[0]}, 0x80808001, {dw[0]}']
                if w == 32:                                          # q3 mod b^K ends at bit 20 of dword 32
                    return [f'  v_and_b32_e32 {dw[32]}, {hex((1 << (B * K + 8 - 1024)) - 1)}, {lo}',
                            f'  v_xor_b32_e32 {dw[32]}, 0x80808080, {dw[32]}']
                return [f'  v_xor_b32_e32 {dw[w]}, 0x80808080, {lo}']
            ch = Chunks(base, (8 * s1lo - base) // 32, ndw - 1, None, neg=False, nocarry_last=True, radix=32,
                        out=out, tap=tap)
            P1_TOP[0] = (base + ndw * 32) // 8                       # columns from 264 (260) on lie above the last dword

        def consume(m, creg):
            fold_columns(ch, tile_cols(1, m, lambda rho: s1lo + 32 * m + rho, creg))
        run_tiles(P1_TILES, consume, P2_TILES[0], dbuf, after_issue0=fill)
        ch.finish()
        OPND[0] = D
        P1_TOP[0] = S1_TOP
        if clamp:                                  # final carry = 0, or -1 when the numerator < 0 (q3 = -1 -> 0)
            e(f'  v_not_b32_e32 v{XA + 36}, v{XA + 38}')
            if CLAMPBR:                            # no lane of the wave went negative (the usual case): mask all ones
                nclamp[0] += 1
                e(f'  v_cmp_ne_u32_e32 vcc, 0, v{XA + 38}')
                e('  s_nop 4')                     # VALU vcc -> vccz read
                e(f'  s_cbranch_vccz .Lnoclamp{nclamp[0]}')
            for t, r in enumerate(q3out):
                if PREXOR:                         # ((r ^ pat) & m) ^ pat
                    e(f'  v_bitop3_b32 {r}, {r}, v{XA + 36}, {pat(t)} bitop3:0xe2')
                else:
                    e(f'  v_and_b32_e32 {r}, {r}, v{XA + 36}')
            if CLAMPBR:
                e(f'.Lnoclamp{nclamp[0]}:')
        return q3out

    def mfma_remainder(Tl, q3, rout, nxt_p1, dbuf=False, after_pack=None, dw=None, t4=False, clamped=False,
                       inits=None):
        """product 2: r = (T - q3 P) mod b^K -> rout (may be Tl[:K]); the product-2 tile-0 reads are already
        in flight; nxt_p1: prefetch product 1's first tiles at the end (the next Barrett); after_pack: the
        caller's last use of the q3 limbs (dbuf may then take their registers); dw: the operand block whose
        dwords 0..32 mfma_barrett has written (q3 is None)
        t4 (top_est): M-tiles 0..3 over operand dwords 0..31 (the constant digit and q3 bytes 0..126) give bits
        0..1015 of r; limb 36 = b | h << 8 with b = bits 1008..1015 and h from V_FRAC (see gen_padic_mfma's
        docstring); clamped: mfma_barrett forced a negative quotient to 0 (r = T < 2^1016): h = 0 under its mask"""
        Dl = D if dw is None else dw
        nk = 4 if t4 else 5
        if limb_op and dw is None:
            # q3's limbs lie in D[2..38] and are packed in place: dword w reads limbs (32 w - 8) div 28 >= w - 1 and
            # the next, so D[w] holds a limb no later dword reads; the caller's use of the limbs comes first
            if after_pack:
                after_pack()
                after_pack = None
            for w in range(33):
                assert D[w] not in q3[max(0, (32 * w - 8) // B):]
        if dw is None:
            orpack(q3, 8, 32 if t4 else 33, [0x80808000] + [0x80808080] * 32, lead_one=True,
                   pre=range(K) if PREXOR else ())
        if after_pack and not dbuf:
            after_pack()
        if not t4:
            e(f'  v_mov_b32_e32 {Dl[33]}, 0x80')         # q3 byte 131 (zero, offset) at byte 132; pads 0
            for w in range(34, 40):
                e(f'  v_mov_b32_e32 {Dl[w]}, 0')
        swap_operands(Dl, nk)
        OPND[0] = Dl
        # matrix column s holds column s - 1 of q3 P (bits 8 s - 8): P'[s - i] is a plain Toeplitz band
        ch = Chunks(8, 0, K - 1, rout, neg=True, inits=inits or Tl[:K], nocarry_last=True)

        def consume(m, creg):
            fold_columns(ch, tile_cols(2, m, lambda rho: 32 * m + rho, creg))
        # dbuf: the caller's last use of q3 runs while tile 0 (first accumulator set) is in the matrix core;
        # the second set (q3's registers) is first written by tile 1
        run_tiles(P2_TILES[:nk], consume, P1_TILES[0] if nxt_p1 else None, dbuf,
                  after_issue0=after_pack if dbuf else None)
        ch.finish()
        OPND[0] = D
        if t4:
            # tiles 0..3 leave chunk 36 = (T[36] + carry - column 127) mod 2^28: its low byte is exact
            lo, hi = XA + 32, XA + 33                                # the chunk sums are free again
            vb, vh = f'v{XA + 34}', f'v{XA + 35}'
            e(f'  v_mad_u64_u32 {pair(lo)}, vcc, v{V_FRAC}, s{SPT}, 0')   # hi = E = floor(f32 Pt / 2^32)
            e(f'  v_and_b32_e32 {vb}, 0xff, {rout[K - 1]}')
            e(f'  v_lshlrev_b32_e32 {vh}, 8, {vb}')
            e(f'  v_sub_u32_e32 {vh}, v{hi}, {vh}')
            e(f'  v_add_u32_e32 {vh}, {hex(TOPEST_C)}, {vh}')
            e(f'  v_lshrrev_b32_e32 {vh}, 16, {vh}')
            if clamped:
                e(f'  v_and_b32_e32 {vh}, {vh}, v{XA + 36}')
            e(f'  v_lshl_or_b32 {rout[K - 1]}, {vh}, 8, {vb}')

    # ---- prologue ------------------------------------------------------------
    e('.amdgcn_target "amdgcn-amd-amdhsa--gfx950"')
    e('.amdhsa_code_object_version 5')
    e('.text')
    e(f'.globl {name}')
    e('.p2align 8')
    e(f'.type {name},@function')
    e(f'{name}:')
    STAMP = "stamp" in ab                        # timing build: each wave's start / end realtime (100 MHz) and
    if STAMP:                                    # where it ran, 16 B at kernarg rows[15] + 16 (4 wg + wave)
        e('  s_memrealtime s[80:81]')
        e('  s_mov_b32 s85, s2')
    e('  s_load_dwordx2 s[4:5], s[0:1], 0x0')
    e('  s_load_dwordx2 s[6:7], s[0:1], 0x8')
    e('  s_load_dwordx2 s[8:9], s[0:1], 0x10')
    e('  s_load_dwordx2 s[10:11], s[0:1], 0x18')
    e('  s_waitcnt lgkmcnt(0)')
    off, sreg, rem = 0, SNP, K
    for width in (16, 8, 4, 2, 1):
        while rem >= width:
            suffix = f"x{width}" if width > 1 else ""
            dst = f"s[{sreg}:{sreg + width - 1}]" if width > 1 else f"s{sreg}"
            e(f'  s_load_dword{suffix} {dst}, s[8:9], {hex(off)}')
            off += 4 * width
            sreg += width
            rem -= width
    if top_est:
        e(f'  s_load_dword s{SPT}, s[8:9], {hex(PT_OFF)}')
    for i in range(8):
        e(f'  s_mov_b32 s{SPOW + i}, {hex(1 << (4 * i))}')
    for i in range(7):
        e(f'  s_mov_b32 s{SNEG + i}, {hex((-(1 << (4 * i))) & 0xFFFFFFFF)}')
    e(f'  s_mov_b32 s35, {hex(MASK)}')
    if KARA:
        for r_, m_ in ((S2MASK, 2), (S3MASK, 3), (S4MASK, 4)):
            e(f'  s_mov_b32 {r_}, {hex(m_ * MASK)}')
    if PREXOR:
        for v_, val in zip(PATV, PATVAL):
            e(f'  v_mov_b32_e32 v{v_}, {hex(val)}')
    e('  s_lshl_b32 s14, s2, 10')
    e(f'  v_lshlrev_b32_e32 v{V_GOFF}, 2, v{V_TID}')
    e(f'  v_add_u32_e32 v{V_GOFF}, s14, v{V_GOFF}')
    # LDS tile image: 5 x 4 KB, each thread one dwordx4 per 4 KB
    e(f'  v_lshlrev_b32_e32 v10, 4, v{V_TID}')
    for it in range(tile_bytes // 4096):
        e(f'  global_load_dwordx4 v[2:5], v10, s[8:9] offset:{TILE_OFF}')
        e('  s_waitcnt vmcnt(0)')
        e('  ds_write_b128 v10, v[2:5]')
        if it != tile_bytes // 4096 - 1:
            e('  v_add_u32_e32 v10, 0x1000, v10')
    e(f'  v_and_b32_e32 v{V_LDS}, 63, v{V_TID}')
    e(f'  v_lshlrev_b32_e32 v{V_LDS}, 4, v{V_LDS}')
    e('  s_waitcnt lgkmcnt(0)')
    e('  s_barrier')
    if "nodesync" not in ab:
        # odd workgroups start ~8K cycles late: the two waves of a SIMD then reach their matrix-core
        # phases at different times (s_sleep spends no issue slots); 1.5% (profiles/r02zt_desync_ab.jsonl)
        e('  s_bitcmp1_b32 s2, 0')
        e('  s_cbranch_scc0 .Ldesync_done')
        e('  s_sleep 127')
        e('.Ldesync_done:')

    e('.Lprog:')
    e('  s_load_dwordx2 s[14:15], s[6:7], 0x0')
    e('  s_add_u32 s6, s6, 8')
    e('  s_addc_u32 s7, s7, 0')
    e('  s_waitcnt lgkmcnt(0)')
    for code, lab in ((1, '.Lloadx'), (2, '.Lstorex'), (3, '.Lsqr'), (4, '.Lmul'), (22, '.Lloadp'), (23, '.Lstorep')):
        e(f'  s_cmp_eq_u32 s14, {code}')
        e(f'  s_cbranch_scc1 {lab}')
    e('  s_branch .Lend')

    def slot_addr():
        e('  s_mul_i32 s16, s15, s11')
        e('  s_mul_hi_u32 s17, s15, s11')
        e('  s_add_u32 s16, s4, s16')
        e('  s_addc_u32 s17, s5, s17')

    def load_limbs(regs):
        slot_addr()
        for k, r in enumerate(regs):
            e(f'  global_load_dword {r}, v{V_GOFF}, s[16:17]')
            if k != len(regs) - 1:
                e('  s_add_u32 s16, s16, s10')
                e('  s_addc_u32 s17, s17, 0')
        e('  s_waitcnt vmcnt(0)')

    def store_limbs(regs):
        slot_addr()
        for k, r in enumerate(regs):
            e(f'  global_store_dword v{V_GOFF}, {r}, s[16:17]')
            if k != len(regs) - 1:
                e('  s_add_u32 s16, s16, s10')
                e('  s_addc_u32 s17, s17, 0')
        e('  s_waitcnt vmcnt(0)')

    ncall = [0]

    def call(label):
        n = ncall[0]
        ncall[0] += 1
        e('  s_getpc_b64 s[2:3]')
        e(f'.Lpc{n}:')
        e(f'  s_add_u32 s2, s2, {label}-.Lpc{n}')
        e('  s_addc_u32 s3, s3, 0')
        e('  s_swappc_b64 s[12:13], s[2:3]')

    e('.Lloadx:')
    load_limbs(X0 + X1)
    e('  s_branch .Lprog')
    e('.Lstorex:')
    store_limbs(X0 + X1)
    e('  s_branch .Lprog')

    def kara_cross():
        """V = 2 x0 x1 (74 limbs, the upper 37 pre-XORed) by one level of Karatsuba; returns the ripple of the
        final carry through V[57..73] as independent instructions for x0^2's column pass.  Halves: x = xL + xH
        b^19, xL = limbs 0..18, xH = limbs 19..36.  Temporaries in T (free until x0^2): S0 = x0L + x0H (T[0..17],
        S0_18 = x0_18), S1 = 2 (x1L + x1H) (T[18..36]), C = limbs 19..37 of 2 P0 (T[37..55]); the middle
        columns' addends in v2 / v4 over permanently zero v3 / v5.
          1. 2 P0 = 2 x0L x1L: limbs 0..18 -> V[0..18], 19..37 -> C (limb 37 < 2^29, unmasked);
          2. 2 P2 = 2 x0H x1H: limbs 0..35 -> V[38..73] as mask - limb (complemented);
          3. column k = 0..37 of S0 S1 (at most 2^63.1: unsigned) plus t'_k = L_k - P0_k - P2_k + 3 mask, where
             L_k is the limb of 2 P0 + 2 P2 b^38 at position k + 19 and P0_k, P2_k the limbs subtracted (t'_k in
             [0, 2^30): the first multiply-add's addend), plus the carry, which starts at 3: with t' biased by
             3 mask = 3 (2^28 - 1) every column value is the true one plus 3 2^28 >= 0 (the true one >= -2^29 - 2),
             so its limb is exact and its carry the true one plus 3; limb -> V[k + 19];
          4. V[57..73] += the final carry (>= 0, minus the bias 3), complemented limbs restored."""
        S0 = T[:18] + [X0[18]]
        S1 = T[18:37]
        C = T[37:56]
        TPL, TPH = ("v2", "v4"), ("v3", "v5")
        bg = []
        for i in range(18):
            bg.append(f'  v_add_u32_e32 {S0[i]}, {X0[i]}, {X0[19 + i]}')
            bg.append(f'  v_add_lshl_u32 {S1[i]}, {X1[i]}, {X1[19 + i]}, 1')
        bg.append(f'  v_lshlrev_b32_e32 {S1[18]}, 1, {X1[18]}')
        bg += [f'  v_mov_b32_e32 {h}, 0' for h in TPH]
        cols = []
        for c in range(38):                                     # 2 P0
            terms = [(X0[i], X1[c - i]) for i in range(19) if 0 <= c - i < 19]
            cols.append({'terms': terms, 'dbl': True, 'out': V[c] if c < 19 else C[c - 19], 'last': c == 37})
        columns(cols, bg=bg)
        cols = []
        for c in range(36):                                     # 2 P2, complemented
            terms = [(X0[19 + i], X1[19 + c - i]) for i in range(18) if 0 <= c - i < 18]
            cols.append({'terms': terms, 'dbl': True, 'out': V[38 + c], 'cpl': True, 'last': c == 35})
        columns(cols)
        return kara_middle(lambda k: [(S0[i], S1[k - i]) for i in range(19) if 0 <= k - i < 19], C)

    RIP = ("v58", "v59") if FILL0 else ("v2", "v3")     # the ripple's value and carry: clear of the A-tile buffers

    def kara_middle(terms_of, C):
        """steps 3 and 4 of kara_cross / kara_cross_mul: the middle columns (terms_of(k): their multiply-adds) over
        V[0..18] = P0's low limbs, C = its limbs 19..37 and V[38..73] = P2 complemented; returns the ripple"""
        TPL = ("v2", "v4")
        RV, RC = RIP
        e(f'  v_mov_b64_e32 {carry}, 3')
        cols = []
        for k in range(38):                                     # middle columns at b^19
            tl = TPL[k % 2]
            if k <= 18:                                         # C_k - P0_k + (mask - P2_k) + 2 mask
                pre = [f'  v_sub_u32_e32 {tl}, {C[k]}, {V[k]}',
                       f'  v_add3_u32 {tl}, {tl}, {V[38 + k]}, {S2MASK}']
            elif k <= 35:                                       # P2c_k - P2c_(k-19) - C_(k-19) + 3 mask
                pre = [f'  v_sub_u32_e32 {tl}, {V[38 + k]}, {V[k + 19]}',
                       f'  v_sub_u32_e32 {tl}, {tl}, {C[k - 19]}',
                       f'  v_add_u32_e32 {tl}, {S3MASK}, {tl}']
            else:                                               # P2_36 = P2_37 = 0: 4 mask - P2c - C
                pre = [f'  v_sub_u32_e32 {tl}, {S4MASK}, {V[k + 19]}',
                       f'  v_sub_u32_e32 {tl}, {tl}, {C[k - 19]}']
            col = {'terms': terms_of(k), 'out': V[k + 19], 'addend': f'v[{tl[1:]}:{int(tl[1:]) + 1}]', 'pre': pre}
            if PREXOR and k + 19 >= K:
                col['px'] = pxu(k + 19)
            cols.append(col)
        columns(cols, carry_in=True)
        # 4. ripple: v = (mask ^ P2c_19) + carry - 3, then limb / carry through V[73] (v2 value, v3 carry)
        e(f'  v_xad_u32 {RV}, {V[57]}, {SMASK}, v{CARRY}')
        rip = [f'  v_add_u32_e32 {RV}, -3, {RV}']
        for j in range(57, 2 * K):
            px = pxu(j) if PREXOR else None
            if j == 2 * K - 1:
                rip.append(f'  v_xor_b32_e32 {V[j]}, {px}, {RV}' if px else f'  v_mov_b32_e32 {V[j]}, {RV}')
                break
            rip.append(f'  v_bitop3_b32 {V[j]}, {RV}, {SMASK}, {px} bitop3:0x6a' if px
                       else f'  v_and_b32_e32 {V[j]}, {hex(MASK)}, {RV}')
            rip.append(f'  v_lshrrev_b32_e32 {RC}, 28, {RV}')
            rip.append(f'  v_xad_u32 {RV}, {V[j + 1]}, {SMASK}, {RC}')
        return rip

    def kara_cross_mul():
        """V = W = x0 y1 + x1 y0 (74 limbs, the upper 37 pre-XORed, the constant digit in byte 3 of limb 73) by one
        level of Karatsuba applied to both products at once -- kara_cross's scheme with P0 = x0L y1L + x1L y0L,
        P2 = x0H y1H + x1H y0H and the middle (x0L + x0H)(y1L + y1H) + (x1L + x1H)(y0L + y0H), whose sizes are those
        of 2 x0L x1L, 2 x0H x1H and S0 S1 there, so the addends t', the bias 3 and the ripple are kara_middle's as
        they stand (bounds: tools/padic_mfma_model.py kara_cross_mul).  Returns (the ripple, the instructions that
        must follow the middle columns before x0 y0 is formed).
        Registers.  x0 and y0 outlive W (x0 y0 follows), x1 and y1 die in it, and 15 registers lie idle in a product
        phase (IDLE below).  P2 comes first, on the raw high halves; then x1H += x1L and y1H += y1L in place
        (A1, B1; limb 18 of a half sum is the low half's own) while P0 is formed, whose limbs 19..37 (C) go to IDLE
        and, the last four, to x1's limbs 0..3 (last read 13 columns earlier).  x1L, y1L are then free: they take
        limbs 2..17 of A0 = x0L + x0H and B0 = y0L + y0H and the addends' zero high dwords stay v3 / v5; limbs 0
        and 1 of A0 and B0 find no register and are formed in x0H's and y0H's limbs 19, 20, which are restored
        (minus the low limb) after the middle columns: four more instructions."""
        assert limb_op and NVGPR == 256
        IDLE = ["v6", "v7", "v8", "v9", f"v{XA + 37}", f"v{XA + 38}", f"v{XA + 39}", D[37], D[38], D[39],
                OPB[id(T)][0], OPB[id(T)][39], OPB[id(V)][0], OPB[id(V)][39], "v255"]
        assert len(set(IDLE)) == 15 and not set(IDLE) & set(X0 + X1 + T + V + [f"v{V_LDS}", *map(pat, (0, 1))])
        C = IDLE + X1[:4]
        A1, B1 = X1[19:] + [X1[18]], Y1[19:] + [Y1[18]]
        pool = X1[4:18] + Y1[:18]
        A0 = X0[19:21] + pool[:16] + [X0[18]]
        B0 = Y0[19:21] + pool[16:] + [Y0[18]]
        assert all(len(x) == 19 for x in (C, A0, A1, B0, B1))
        cols = []
        for c in range(36):                                     # P2, complemented
            terms = []
            for i in range(18):
                if 0 <= c - i < 18:
                    terms += [(X0[19 + i], Y1[19 + c - i]), (X1[19 + i], Y0[19 + c - i])]
            cols.append({'terms': terms, 'out': V[38 + c], 'cpl': True, 'last': c == 35})
        columns(cols)
        bg = []
        for i in range(18):                                     # the high halves of x1, y1 are spent
            bg.append(f'  v_add_u32_e32 {A1[i]}, {X1[i]}, {X1[19 + i]}')
            bg.append(f'  v_add_u32_e32 {B1[i]}, {Y1[i]}, {Y1[19 + i]}')
        for i in range(2):
            bg.append(f'  v_add_u32_e32 {A0[i]}, {X0[i]}, {X0[19 + i]}')
            bg.append(f'  v_add_u32_e32 {B0[i]}, {Y0[i]}, {Y0[19 + i]}')
        bg += ['  v_mov_b32_e32 v3, 0', '  v_mov_b32_e32 v5, 0']
        cols = []
        for c in range(38):                                     # P0
            terms = []
            for i in range(19):
                if 0 <= c - i < 19:
                    terms += [(X0[i], Y1[c - i]), (X1[i], Y0[c - i])]
            cols.append({'terms': terms, 'out': V[c] if c < 19 else C[c - 19], 'last': c == 37})
        columns(cols, bg=bg)
        for i in range(2, 18):                                  # the low halves of x1, y1 are spent
            e(f'  v_add_u32_e32 {A0[i]}, {X0[i]}, {X0[19 + i]}')
            e(f'  v_add_u32_e32 {B0[i]}, {Y0[i]}, {Y0[19 + i]}')

        def mid(k):
            terms = []
            for i in range(19):
                if 0 <= k - i < 19:
                    terms += [(A0[i], B1[k - i]), (A1[i], B0[k - i])]
            return terms
        rip = kara_middle(mid, C)
        restore = []
        for i in range(2):
            restore.append(f'  v_sub_u32_e32 {X0[19 + i]}, {X0[19 + i]}, {X0[i]}')
            restore.append(f'  v_sub_u32_e32 {Y0[19 + i]}, {Y0[19 + i]}, {Y0[i]}')
        return rip, restore

    Q = D[2:2 + K]                               # limb_op: the first reduction's q3 limbs
    RINIT = (lambda Tl: Tl[:K - 1] + [L36]) if limb_op else (lambda Tl: None)

    def reduce_body(fill=None):
        """the reduction of SQR and MUL, from the label .Lreduce; fill (fill0): the caller's instructions for tile 0
        of the first product 1 -- the text then starts in the caller and .Lreduce stands behind that tile's issue"""
        if fill is None:
            e('.Lreduce:')
        # default s_setprio 3 over the reduction (noprio: none): -0.5..1% (profiles/r03s_m37_prio_ab.jsonl)
        PRIO = next((int(t[4:]) for t in ab & set(PRIOS)), 0 if "noprio" in ab else 3)
        if PRIO:
            e(f'  s_setprio {PRIO}')                # the latency-bound matrix phases win the SIMD's VALU issue
        dbuf = "nodbuf" not in ab
        # the first product 1 has one accumulator set: T[38..69] is its operand (limb_op) or takes its q3, and V is live
        q3 = mfma_barrett(T, Q if limb_op else T[K:], clamp=True, t4=top_est, fill=fill)    # u1 -> T[K..2K-1]

        def add_u1():
            for i in range(K):
                if PREXOR:                                      # V += u1 ^ pat (u1 arrives pre-flipped)
                    e(f'  v_xad_u32 {V[i]}, {q3[i]}, {pat(i)}, {V[i]}')
                else:
                    e(f'  v_add_u32_e32 {V[i]}, {V[i]}, {q3[i]}')  # V += u1 (limbs < 2^29); u1 dies here
        mfma_remainder(T, q3, T[:K], nxt_p1=True, dbuf=dbuf, after_pack=add_u1, t4=top_est, clamped=True,
                       inits=RINIT(T))               # u0 -> T[0..K-1]
        if Q3DW:
            mfma_barrett(V, None, clamp=False, prefetched=True, dbuf=dbuf, dw=D2, t4=top_est)    # T[K..] is free
            mfma_remainder(V, None, V[:K], nxt_p1=False, dbuf=dbuf, dw=D2, t4=top_est, inits=RINIT(V))
        else:
            q3b = mfma_barrett(V, V[K:], clamp=False, prefetched=True, dbuf=dbuf, t4=top_est)
            mfma_remainder(V, q3b, V[:K], nxt_p1=False, dbuf=dbuf, t4=top_est)
        move(X0, T[:K])
        move(X1, V[:K])
        if PRIO:
            e('  s_setprio 0')
        e('  s_setpc_b64 s[12:13]')

    REDUCE = []                                  # fill0: the callers' shared text, from .Lreduce on

    def call_reduce(fill):
        """fill0: the caller issues the reduction up to tile 0 of the first product 1 itself, fill between that tile's
        MFMAs, and enters the shared text behind it"""
        if FILL0:
            nclamp[0] = 1                        # the reduction's clamp label follows LOADP's, as in the other bodies
            text = capture(lambda: reduce_body(lambda: [e(ins) for ins in fill]))
            nclamp[0] = 0
            cut = text.index('.Lreduce:')
            assert not REDUCE or REDUCE[0] == text[cut:], "the callers of .Lreduce disagree on its text"
            REDUCE[:] = [text[cut:]]
            for ins in text[:cut]:
                e(ins)
        call('.Lreduce')

    # SQR: V = 2 x0 x1, T = x0^2, reduce
    e('.Lsqr:')
    e('  s_mov_b32 s19, s15')
    e('.Lsqr_loop:')
    e('  s_cmp_eq_u32 s19, 0')
    e('  s_cbranch_scc1 .Lprog')
    rip = []
    if KARA:
        rip = kara_cross()
    else:
        cols = []
        for c in range(2 * K):
            terms = [(X0[i], X1[c - i]) for i in range(K) if 0 <= c - i < K]
            cols.append({'terms': terms, 'dbl': True, 'out': V[c], 'last': c == 2 * K - 1})
            if PREXOR and c >= K:
                cols[-1]['px'] = pxu(c)
        columns(cols)
    cols = []
    for c in range(2 * K):
        terms = [(X0[i], X0[c - i]) for i in range(K) if i < c - i < K]
        sq = X0[c // 2] if c % 2 == 0 and c // 2 < K else None
        col = {'terms': terms, 'out': T[c], 'last': c == 2 * K - 1}
        if PREXOR and c >= K:
            col['px'] = pxu(c)
        if terms:
            col['dbl'] = True
            if sq:
                col['sq'] = sq
        elif sq:
            col['terms'] = [(sq, sq)]
        cols.append(col)
    columns(cols, bg=() if FILL0 else rip)
    call_reduce(rip)
    e('  s_sub_u32 s19, s19, 1')
    e('  s_branch .Lsqr_loop')

    # MUL slot: y0 -> T[0..K-1], y1 -> T[K..]; W = x0 y1 + x1 y0 -> V; T = x0 y0 -> (XB, T[K..]); move
    e('.Lmul:')
    Y0, Y1 = T[:K], T[K:]
    load_limbs(Y0 + Y1)
    rip = []
    if MULKARA:
        rip, restore = kara_cross_mul()
        for ins in restore:
            e(ins)
    else:
        columns(product_cols(X0, Y1, 2 * K, V, a2=X1, b2=Y0))
    TM = X1 + T[K:]                              # x1, y1 dead
    columns(product_cols(X0, Y0, 2 * K, TM), bg=() if FILL0 else rip)
    if FILL0:                                    # limb 36 is read before tile 0 is issued; the rest fills it
        move(T[K - 1:K], X1[K - 1:])
        call_reduce(rip + capture(lambda: move(T[:K - 1], X1[:K - 1])))
    else:
        move(T[:K], X1)
        call_reduce(())
    e('  s_branch .Lprog')

    # LOADP slot: plain X -> T -> (q3 = x1, r = x0)
    e('.Lloadp:')
    load_limbs(T)
    if limb_op:
        q3 = mfma_barrett(T, Q, clamp=True, pre_in=False)
        for i in range(K):                       # x1 waits, unflipped, where product 1's operand has died
            e(f'  v_xor_b32_e32 {T[K + i]}, {pat(i)}, {Q[i]}')
        mfma_remainder(T, q3, T[:K], nxt_p1=False, inits=RINIT(T))
    else:
        q3 = mfma_barrett(T, T[K:], clamp=True, pre_in=False)
        mfma_remainder(T, q3, T[:K], nxt_p1=False)
    move(X0, T[:K])
    if limb_op:
        move(X1, T[K:2 * K])
    elif PREXOR:
        for i in range(K):
            e(f'  v_xor_b32_e32 {X1[i]}, {pat(i)}, {T[K + i]}')
    else:
        move(X1, T[K:2 * K])
    e('  s_branch .Lprog')

    # STOREP slot: x0 + x1 P with -P in SGPRs (scratch -x1 in T[0..K-1]; out V)
    e('.Lstorep:')
    NX1 = T[:K]
    for i in range(K):
        e(f'  v_sub_u32_e32 {NX1[i]}, 0, {X1[i]}')
    cols = []
    for c in range(2 * K):
        terms = [(X0[c], '1')] if c < K else []
        terms += [(NX1[i], NP(c - i)) for i in range(K) if 0 <= c - i < K]
        cols.append({'terms': terms, 'out': V[c], 'last': c == 2 * K - 1})
    columns(cols, signed=True)
    store_limbs(V)
    e('  s_branch .Lprog')

    e('.Lend:')
    if STAMP:
        e('  s_waitcnt vmcnt(0)')
        e('  s_memrealtime s[82:83]')
        e('  s_getreg_b32 s84, hwreg(HW_REG_HW_ID)')
        e('  s_getreg_b32 s86, hwreg(HW_REG_XCC_ID)')
        e('  s_load_dwordx2 s[88:89], s[0:1], 0xa0')
        e('  s_waitcnt lgkmcnt(0)')
        e('  s_cmp_eq_u64 s[88:89], 0')
        e('  s_cbranch_scc1 .Lstamp_done')
        e('  s_mov_b64 exec, 1')
        e(f'  v_lshrrev_b32_e32 v2, 6, v{V_TID}')
        e('  v_lshl_add_u32 v2, s85, 2, v2')                           # wave index in the launch
        e('  v_lshlrev_b32_e32 v7, 4, v2')
        e('  v_mov_b32_e32 v2, s80')
        e('  v_mov_b32_e32 v3, s82')
        e('  v_mov_b32_e32 v4, s84')
        e('  v_mov_b32_e32 v5, s86')
        e('  global_store_dwordx4 v7, v[2:5], s[88:89]')
        e('  s_waitcnt vmcnt(0)')
        e('.Lstamp_done:')
    e('  s_endpgm')

    # reduce (SQR, MUL): T (x0^2 or x0 y0), V (cross terms) -> x0 = T mod P, x1 = (V + T div P) mod P
    if FILL0:
        for ins in REDUCE[0]:
            e(ins)
    else:
        reduce_body()

    e(f'.Lfunc_end_{name}:')
    e(f'  .size {name}, .Lfunc_end_{name}-{name}')
    e('')
    o.extend(_descriptor(name, tile_bytes, NVGPR, 90 if STAMP else NSGPR).splitlines())
    return "\n".join(o) + "\n"


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--body', default='m37', choices=sorted({**BODIES, **K_BODIES}), help='the kernel fthe_padic_<body>')
    ap.add_argument('--ab', default='', help='A/B switches, comma-separated: ' + ', '.join(SWITCHES + K_SWITCHES) + ', prioN')
    ap.add_argument('-o', '--out', required=True)
    a = ap.parse_args()
    with open(a.out, 'w') as f:
        f.write(gen_body(a.body, a.ab))
