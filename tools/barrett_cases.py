"""Crafted digits for the two matrix-core Barrett kernel families, one list for every level that tests them, and the
checker of what a kernel returns.

The key holder's P-adic kernels (fthe_padic_m37 / m37t / m37s / m37l / m37k and the VALU fthe_padic_k37: X mod P^2 as two
base-P digits of 37 limbs of 28 bits) and the parties' fthe_nadic_b76 (X mod n^2 as two base-n digits of 76 limbs of
27 bits) reduce every product with Barrett's quotient estimate and never correct the remainder: a digit may stay as
large as `top` = 5P - 1 (m37, k37), 3P - 1 (the four-tile bodies), 3n - 1 (b76), and the next product must take it.
The cases below sit where that arithmetic is tight: the largest digit, digits next to a multiple of the modulus,
all-ones limbs (the largest column sums), zero halves, one-limb digits, and products so small that the estimate is
clamped to 0.  The wave emulator's self-tests (tools/wave_emu.py), the bring-up probe
(tools/nadicb_probe.py) and, through tests/digit_cases.py, which adds the test keys, the CPU test that runs every case
through the bit-exact models (tests/test_digit_checker.py) and the GPU tests that run them on the real matrix cores
(tests/test_gpu_padic_digits.py, tests/test_gpu_nadicb_digits.py, through fthe_debug_padic_prog /
fthe_debug_nadicb_prog) all draw from here.  The module lies beside the models and the emulator, which it needs and
which need it, so that the tools stand without the test directory.  Every admitted range is the models' own (their assertions fire on a
case outside a kernel's contract).

Programs are flat lists of (op, argument) pairs as the kernels read them: 0 END, 1 LOADX slot, 2 STOREX slot,
3 SQR count, 4 MUL slot, 20 CANON (b76), 22 LOADP slot, 23 STOREP slot (P-adic).  A slot holds a digit pair (x0, x1)
or, for LOADP / STOREP, a plain integer.
"""
import contextlib
import os
import random
import sys

_TOOLS = os.path.dirname(os.path.abspath(__file__))
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)

END, LOADX, STOREX, SQR, MUL, CANON, LOADP, STOREP = 0, 1, 2, 3, 4, 20, 22, 23

# the programs every level runs (the output slot is the last one stored); slots 0 and 1 are inputs
PADIC_PROGS = {
    "io": [LOADX, 0, STOREX, 1, 0, 0],
    "loadp": [LOADP, 0, STOREP, 1, 0, 0],
    "sqr_storep": [LOADX, 0, SQR, 1, STOREP, 1, 0, 0],
    "sqr2": [LOADX, 0, SQR, 2, STOREX, 1, 0, 0],
    "mul": [LOADX, 0, MUL, 1, STOREP, 2, 0, 0],
    "sqr3_mul": [LOADX, 0, SQR, 3, MUL, 1, STOREP, 2, 0, 0],
}
# 64 squarings: the profiling counters take a launch of at least 64 products per lane for an exponentiation and count
# it under the variant id of the body that ran (BODY_ID)
PADIC_WITNESS = [LOADX, 0, SQR, 64, STOREP, 1, 0, 0]
NADICB_PROGS = {
    "io": [LOADX, 0, STOREX, 1, 0, 0],
    "canon": [LOADX, 0, CANON, 0, STOREX, 1, 0, 0],
    "sqr": [LOADX, 0, SQR, 1, STOREX, 2, 0, 0],
    "mul": [LOADX, 0, MUL, 1, STOREX, 2, 0, 0],
    "sqr3_mul": [LOADX, 0, SQR, 3, MUL, 1, STOREX, 2, 0, 0],
}

# ---- the P-adic kernels ----------------------------------------------------------------------------------------
PK, PB = 37, 28
PMASK = (1 << PB) - 1
BODIES = ("m37l", "m37s", "m37t", "m37", "k37")
# fthe_padic_m37k (m37l with MUL's cross term by Karatsuba) stands beside BODIES: the same contract, model and image
# as m37l, its own product cases (padic_kara_mul_pairs)
LIMB_FED = ("m37k", "m37l")
FOUR_TILE = LIMB_FED + ("m37s", "m37t")
# the environment that makes key set-up choose a body, and the profiling variant id that then counts its launches
BODY_ENV = {"m37k": {}, "m37l": {"FTHE_NO_M37K": "1"}, "m37s": {"FTHE_NO_M37L": "1"}, "m37t": {"FTHE_NO_M37S": "1"},
            "m37": {"FTHE_NO_M37T": "1"},
            "k37": {"FTHE_NO_PADIC_MFMA": "1"}}
BODY_ID = {"k37": 1037, "m37": 1137, "m37t": 1237, "m37s": 1337, "m37l": 1437, "m37k": 1537}


def padic_body_for(P, variant):
    """the body that runs for P when the key is set up for `variant`: a P wider than the four-tile bodies admit
    (padic_mfma_model.TOPEST_MAX_BITS) falls to m37"""
    import padic_mfma_model as mm
    assert 1009 <= P.bit_length() <= 1030, "the K = 37 kernels take P of 1009..1030 bits"
    if variant in FOUR_TILE and P.bit_length() > mm.TOPEST_MAX_BITS:
        return "m37"
    return variant


def padic_nd(variant):
    """SQR / MUL take digits below padic_nd * P"""
    import padic_mfma_model as mm
    return mm.TOPEST_DIGIT if variant in FOUR_TILE else 5


def padic_plain_limit(P, variant):
    """LOADP takes a plain X below this: 50 P^2 (gen_padic.py; the quotient, below 50 P, fits 37 limbs), 3 P^2 on the
    four-tile bodies (gen_padic_mfma.py: the quotient becomes the digit x1 < 3P)"""
    return (padic_nd(variant) if variant in FOUR_TILE else 50) * P * P


def padic_special_digits(P, variant):
    """the digits of wave_emu.m37_digits_selftest: the squaring's cross term at the extremes the kernel admits --
    low 36 limbs all 2^28 - 1 under the largest top limb (the largest Karatsuba half sums and column sums), zero
    halves, one-limb digits, the top digit"""
    top = padic_nd(variant) * P - 1
    allones = (1 << (PB * (PK - 1))) - 1                         # limbs 0..35 = 2^28 - 1
    big = allones + (((top - allones) >> (PB * (PK - 1))) << (PB * (PK - 1)))
    assert big <= top
    low19 = (1 << (PB * 19)) - 1                                 # xL all ones, xH 0
    high18 = big - (big & low19)                                 # xL 0, xH max
    return [big, 0, 1, low19, high18, top, P - 1, (1 << (PB * 19)), PMASK, big ^ (PMASK << (PB * 18))]


def padic_edge_digits(P, variant):
    """digits next to the multiples of P below the bound, and the top digit"""
    return [P - 1, P, P + 1, 2 * P - 1, 2 * P, padic_nd(variant) * P - 1]


def padic_emu_pairs(P, variant, pairs0=()):
    """the crafted pairs of wave_emu.m37_digits_selftest: pairs0, then special x special, cut at 40"""
    special = padic_special_digits(P, variant)
    return (list(pairs0) + [(a, b) for a in special for b in special])[:max(40, len(pairs0))]


def padic_edge_pairs(P, variant):
    """pairs of the edge digits, and pairs whose x0^2 is below P: the first reduction's quotient is 0 (clamped where
    q1 mu is below the bias) while x1 stays at the bound"""
    edge = padic_edge_digits(P, variant)
    top = edge[-1]
    out = []
    for a in edge:
        for b in (a, 0, top):
            if (a, b) not in out:
                out.append((a, b))
    out += [(0, top), (1, top), (2, 0), (PMASK, top), (1 << 500, P + 1), (1 << 300, 2 * P - 1)]
    return out


def padic_sqr_pairs(P, variant):
    """every crafted pair a squaring program is run on (at most 64: one wave of the emulator)"""
    pairs = padic_emu_pairs(P, variant)
    pairs += [p for p in padic_edge_pairs(P, variant) if p not in pairs]
    assert len(pairs) <= 64
    return pairs


def padic_mul_pairs(P, variant):
    """crafted x crafted operands ((a0, a1), (b0, b1)) of a product, and operands with a0 b0 < P (a clamped or zero
    first quotient) that land beside them in a wave"""
    sp = padic_special_digits(P, variant)
    D = [0, 1] + padic_edge_digits(P, variant) + [sp[0], sp[3], sp[4], sp[9]]
    top = padic_nd(variant) * P - 1
    m = len(D)
    out = []
    for i, a in enumerate(D):
        for b in (a, D[(i + 3) % m], top):
            out.append(((a, D[(i + 1) % m]), (b, D[(i + 5) % m])))
    out += [((1, top), (1, top)), ((3, top), (5, P)), ((1 << 400, 2 * P), (1 << 500, top)), ((0, top), (top, top)),
            ((PMASK, 1), (PMASK, top)), ((1 << 504, P - 1), ((P - 1) >> 504, top)), ((2, top), ((P - 1) // 2, top))]
    for (a0, _), (b0, _) in out[-7:]:
        assert a0 * b0 < P
    return out


def padic_kara_mul_pairs(P, variant):
    """operands ((a0, a1), (b0, b1)) at the extremes of the Karatsuba cross term a0 b1 + a1 b0 of fthe_padic_m37k:
    every low half all ones under zero high halves and the reverse (the largest P0 / P2 against the smallest middle
    term and the other way round: the two ends of the middle columns' addend), every limb 2^28 - 1 up to the digit
    bound (the largest middle column), zero digits and zero cross terms (the carry's bias must ripple out through
    limbs 57..73), a0 b0 < P (a zero first quotient); then padic_mul_pairs"""
    sp = padic_special_digits(P, variant)
    big, low19, high18 = sp[0], sp[3], sp[4]
    top = padic_nd(variant) * P - 1
    out = [((low19, low19), (low19, low19)), ((high18, high18), (high18, high18)),
           ((low19, high18), (low19, high18)), ((low19, high18), (high18, low19)), ((high18, low19), (low19, high18)),
           ((big, big), (big, big)), ((top, top), (top, top)), ((big, top), (top, big)),
           ((0, 0), (0, 0)), ((big, 0), (big, 0)), ((top, 0), (top, 0)), ((0, 0), (top, top)), ((top, top), (0, 0)),
           ((1, big), (1, big)), ((1 << 504, low19), ((P - 1) >> 504, high18))]
    for (a0, _), (b0, _) in out[-2:]:
        assert a0 * b0 < P
    return out + padic_mul_pairs(P, variant)


def padic_plain_values(P, variant):
    """LOADP inputs: the values of wave_emu.m37_selftest (0, 1, P - 1, P, P^2 - 1), the neighbours of P^2, values around
    b^36 (below it the quotient is clamped) and the largest admitted X"""
    P2 = P * P
    return [0, 1, P - 1, P, P2 - 1, P2, P2 + 1, (1 << 1008) - 1, 1 << 1008, padic_plain_limit(P, variant) - 1]


def padic_emu_values(P):
    """the plain values that take the first lanes of wave_emu.m37_selftest"""
    return padic_plain_values(P, "m37")[:5]


def plimbs(x, n=PK):
    assert 0 <= x < (1 << (PB * n))
    return [(x >> (PB * i)) & PMASK for i in range(n)]


def padic_row(v):
    """the 74 limbs of a slot: a digit pair (x0 in limbs 0..36, x1 in 37..73) or a plain integer"""
    return plimbs(v[0]) + plimbs(v[1]) if isinstance(v, tuple) else plimbs(v, 2 * PK)


@contextlib.contextmanager
def _padic_barrett(P, variant):
    """the model's key for a body, with padic_model.sqr / mul routed through that body's Barrett"""
    import padic_mfma_model as mm
    import padic_model as pm
    old = pm.barrett
    if variant == "k37":
        key, red = pm.PadicKey(P, PK), mm.pm_barrett
    else:
        key = mm.MfmaKey(P, q_shift=mm.Q1_SHIFT if variant == "m37s" else 0, limb_op=variant in LIMB_FED)
        if variant in FOUR_TILE:
            red = lambda k, T: mm.barrett_top(k, T)[:2]            # noqa: E731
        else:
            red = lambda k, T: mm.barrett(k, T)[:2]                # noqa: E731
    pm.barrett = red
    try:
        yield key
    finally:
        pm.barrett = old


def padic_model_run(P, variant, prog, slots):
    """one lane of a program through the bit-exact model of a body (tools/padic_model.py with the Barrett of
    tools/padic_mfma_model.py): the 74 limbs of the last slot stored.  The model's assertions fire on an input
    outside the body's contract."""
    import padic_mfma_model as mm
    import padic_model as pm
    slots = {s: padic_row(v) for s, v in slots.items()}
    last = None
    with _padic_barrett(P, variant) as key:
        x0 = x1 = None
        for op, a in zip(prog[::2], prog[1::2]):
            if op == END:
                break
            if op == LOADX:
                x0, x1 = slots[a][:PK], slots[a][PK:]
            elif op == STOREX:
                slots[a] = list(x0) + list(x1)
                last = a
            elif op == SQR:
                for _ in range(a):
                    x0, x1 = pm.sqr(key, x0, x1)
            elif op == MUL:
                x0, x1 = pm.mul(key, x0, x1, slots[a][:PK], slots[a][PK:])
            elif op == LOADP:
                X = pm.value(slots[a])
                assert X < padic_plain_limit(P, variant), "LOADP input beyond the contract"
                if variant in FOUR_TILE:                          # LOADP keeps the five-tile product 2
                    x1, x0 = mm.barrett(key, slots[a])[:2]
                else:
                    x0, x1 = pm.loadp(key, X)
            elif op == STOREP:
                slots[a] = pm.storep(key, x0, x1)
                last = a
            else:
                raise ValueError(op)
    return slots[last]


# ---- fthe_nadic_b76 ----------------------------------------------------------------------------------------------
NS, NB = 76, 27
NMASK = (1 << NB) - 1


def nadicb_emu_values(n):
    """the r of wave_emu.nadicb_selftest's first ciphertexts"""
    return [0, 1, n - 1]


def nadicb_pairs(n):
    """crafted digit pairs in [0, 3n): the probe's and the model's extremes, digits whose low 75 limbs are all
    2^27 - 1 under the largest top limb, one-limb digits, and pairs whose x0^2 is below n (Barrett 1's quotient 0,
    clamped where q1 mu is below the bias)"""
    top = 3 * n - 1
    allones = (1 << (NB * (NS - 1))) - 1
    big = allones + (((top - allones) >> (NB * (NS - 1))) << (NB * (NS - 1)))
    assert allones < big <= top
    return [(0, 0), (1, 0), (0, 1), (n, n - 1), (top, top), (top, 0), (0, top),             # the issue's list
            (1, 1), (n, n), (n - 1, 2 * n + 5), (n - 1, n - 1), (2 * n - 1, 2 * n), (n + 1, 2 * n - 1),
            (big, big), (big, 0), (allones, big), (top, big), (NMASK, top), (1 << (NB * 38), top),
            (1, top), (2, top), (1 << 1000, top), (1 << 1019, n + 1)]


def nadicb_mul_pairs(n):
    """crafted x crafted operands of a product, and operands with x0 y0 < n"""
    ps = nadicb_pairs(n)
    top = 3 * n - 1
    m = len(ps)
    out = [(ps[i], ps[(i + 4) % m]) for i in range(m)] + [(ps[i], (top, top)) for i in range(0, m, 3)]
    small = [((1, top), (1, top)), ((1 << 1000, top), (1 << 1020, top)), ((3, n), (n // 4, top)), ((0, top), (top, top))]
    for (a0, _), (b0, _) in small:
        assert a0 * b0 < n
    return out + small


def nlimbs(x):
    assert 0 <= x < (1 << (NB * NS))
    return [(x >> (NB * i)) & NMASK for i in range(NS)]


def nadicb_row(v):
    return nlimbs(v[0]) + nlimbs(v[1])


def nadicb_model_run(key, prog, slots, fast=True):
    """one ciphertext of a program through tools/nadicb_model.py: the digit pair of the last slot stored, exactly as
    the kernel leaves it.  fast: the products as integers and only the two reductions through the model (Key.reduce
    on convolved column sums) -- what Digits.mul computes once its VALU pass has asserted z = x y; else Digits."""
    import nadicb_model as nm
    old = nm.FAST[0]
    nm.FAST[0] = fast
    try:
        slots = dict(slots)
        D = last = None
        for op, a in zip(prog[::2], prog[1::2]):
            if op == END:
                break
            if op == LOADX:
                D = nm.Digits(key, *slots[a])
            elif op == STOREX:
                slots[a] = (D.x0, D.x1)
                last = a
            elif op in (SQR, MUL):
                for _ in range(a if op == SQR else 1):
                    y0, y1 = (D.x0, D.x1) if op == SQR else slots[a]
                    if fast:
                        r1, q3 = key.reduce(D.x0 * y0)
                        r2, _ = key.reduce(D.x0 * y1 + D.x1 * y0 + q3)
                        D.x0, D.x1 = r1, r2
                        D.check()
                    else:
                        D.mul(y0, y1, sq=op == SQR)
            elif op == CANON:
                D.canon()
            else:
                raise ValueError(op)
        return slots[last]
    finally:
        nm.FAST[0] = old


# ---- layout ------------------------------------------------------------------------------------------------------
def rotated_layout(ncases, count, wave, wg):
    """which case each of `count` consecutive elements holds (None: a random one).  wave / wg: elements per wave and
    per workgroup (64 / 256 lanes of the P-adic kernels, 16 / 192 ciphertexts of b76, four lanes each).  Where the
    launch is large enough every case lands once in the lower half of a wave of workgroup 0 and once in the upper
    half of a wave other than the first of workgroup 1, and the first cases again at the very end (the partial
    wave); a smaller launch takes the cases in turn from an offset that differs from count to count."""
    half = wave // 2
    out = [None] * count
    need = wg + wave * (2 + (ncases - 1) // half)
    if count >= need and wave * (1 + (ncases - 1) // half) <= wg:
        for i in range(ncases):
            out[wave * (i // half) + i % half] = i
            out[wg + wave * (1 + i // half) + half + i % half] = i
        for i in range(min(ncases, count - need)):
            out[count - 1 - i] = i
    else:
        for j in range(min(count, 2 * ncases)):
            out[j] = (j + count) % ncases
    return out


# ---- the checker -------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def _value(v, M):
    return v[0] + v[1] * M if isinstance(v, tuple) else v


def expected(M, prog, slots):
    """a program on Python integers: (op that stored the result, its value mod M^2, the stored object itself when
    nothing was computed on the way -- LOADX; STOREX returns the digit pair limb for limb, LOADP; STOREP the plain
    value ("plain", X) --, else None)"""
    M2 = M * M
    slots = dict(slots)
    X = same = kind = last = None
    for op, a in zip(prog[::2], prog[1::2]):
        if op == END:
            break
        if op in (LOADX, LOADP):
            assert isinstance(slots[a], tuple) == (op == LOADX), "LOADX reads a digit pair, LOADP a plain value"
            X, same = _value(slots[a], M) % M2, slots[a] if op == LOADX else ("plain", slots[a])
        elif op == STOREX:
            slots[a], kind, last = (same if same is not None and same[0] != "plain" else ("residue", X)), op, a
        elif op == STOREP:                                       # LOADP; STOREP: x0 + x1 P is the input itself
            slots[a], kind, last = (same if same is not None and same[0] == "plain" else ("residue", X)), op, a
        elif op == SQR:
            assert 1 <= a <= 64
            X, same = pow(X, 1 << a, M2), None
        elif op == MUL:
            v = slots[a]
            assert isinstance(v, tuple) and v[0] != "residue", "MUL by an input slot"
            X, same = X * _value(v, M) % M2, None
        elif op == CANON:
            same = None
        else:
            raise ValueError(op)
    v = slots[last]
    if v[0] == "residue":
        return kind, X, None
    return kind, (v[1] if v[0] == "plain" else _value(v, M)) % M2, v


def check_padic(P, variant, prog, slots, out):
    """one lane of a P-adic program: out, the 74 limbs the kernel returned for the slot the program stored last, must
    hold limbs below 2^28 and, after STOREX, digits below the bound the next product relies on (5P, 3P on the
    four-tile bodies) with (x0 + x1 P) mod P^2 the integer result, after STOREP a plain value below 6 P^2 congruent
    to it.  LOADX; STOREX and LOADP; STOREP alone return their input.  Raises Mismatch."""
    out = [int(v) for v in out]
    if len(out) != 2 * PK or not all(0 <= v <= PMASK for v in out):
        raise Mismatch("a limb at or above 2^28")
    kind, want, same = expected(P, prog, slots)
    if same is not None:
        if out != padic_row(same[1] if same[0] == "plain" else same):
            raise Mismatch("LOADP; STOREP changed the value" if same[0] == "plain" else "LOADX; STOREX changed the digits")
        return
    P2 = P * P
    val = lambda ls: sum(v << (PB * i) for i, v in enumerate(ls))      # noqa: E731
    if kind == STOREP:
        got = val(out)
        if got >= 6 * P2:
            raise Mismatch("STOREP value at or above 6 P^2")
        if got % P2 != want:
            raise Mismatch("STOREP value is not the residue")
        return
    x0, x1 = val(out[:PK]), val(out[PK:])
    bound = padic_nd(variant) * P
    if x0 >= bound or x1 >= bound:
        raise Mismatch(f"digit at or above {padic_nd(variant)} P")
    if (x0 + x1 * P) % P2 != want:
        raise Mismatch("digits do not hold the residue")


def nadicb_digits(out):
    out = [int(v) for v in out]
    return (sum(v << (NB * i) for i, v in enumerate(out[:NS])), sum(v << (NB * i) for i, v in enumerate(out[NS:])))


def check_nadicb(n, prog, slots, out, model=None):
    """one ciphertext of a b76 program: limbs below 2^27, digits below 3n (below n after a final CANON), (x0 + x1 n)
    mod n^2 the integer result, and with model (the digit pair of nadicb_model_run) the digits themselves.  Returns
    (x0 // n, x1 // n): after a product, how far each Barrett quotient fell below the true one.  Raises Mismatch."""
    out = [int(v) for v in out]
    if len(out) != 2 * NS or not all(0 <= v <= NMASK for v in out):
        raise Mismatch("a limb at or above 2^27")
    kind, want, same = expected(n, prog, slots)
    x0, x1 = nadicb_digits(out)
    if same is not None:
        if (x0, x1) != same:
            raise Mismatch("LOADX; STOREX changed the digits")
        return 0, 0
    ops = [op for op in prog[::2]]
    canon = CANON in ops and not any(op in (SQR, MUL) for op in ops[len(ops) - ops[::-1].index(CANON):])
    bound = n if canon else 3 * n
    if x0 >= bound or x1 >= bound:
        raise Mismatch("digit at or above " + ("n after CANON" if canon else "3n"))
    if (x0 + x1 * n) % (n * n) != want:
        raise Mismatch("digits do not hold the residue")
    if model is not None and (x0, x1) != tuple(model):
        raise Mismatch("digits differ from the model's")
    return x0 // n, x1 // n


def filler(rng, bound, pair=True):
    return (rng.randrange(bound), rng.randrange(bound)) if pair else rng.randrange(bound)


def make_rng(*seed):
    return random.Random(":".join(str(s) for s in seed))
