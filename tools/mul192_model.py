#!/usr/bin/env python3
"""Bit-exact model of the Paillier-3072 ciphertext product (fthe_mul192, fedtree_amd/csrc/fthe_mul192.hip).

out = x y mod N for N = n^2, n odd with 96 words (3041..3072 bits, so 2^6080 <= N < 2^6144), x and y any rows
of 192 dwords (below 2^6144, rows >= N included).  Limbs have B = 27 bits; an operand has 232 of them (8 lanes
x 29), a product 464 columns.

Product (ring()).  Lane l of the octet owns limbs [29 l, 29 l + 29).  Step s adds x_limb * m[s] into the lane's
ring of 29 columns (lane l: columns 29 l + s .. 29 l + s + 28); the lowest column then moves one lane down, lane
7 takes 0, lane 0's retires through a carry chain as limb s.  A column receives at most 232 products below
2^54, so every 64-bit accumulator stays below 2^62 (asserted), carry included.

Barrett.  With a = 27 * 225 = 6075 and b = 27 * 231 = 6237:
    z1 = floor(z / 2^a) < 2^(12288 - 6075) = 2^6213             231 limbs
    mu = floor(2^(a + b) / N) <= 2^(12312 - 6080) = 2^6232       231 limbs
    q  = floor(z1 mu / 2^b) < 2^6208                             230 limbs
z1 mu / 2^b <= z / N, and z1 > z / 2^a - 1, mu > 2^(a+b) / N - 1 give
    z1 mu / 2^b > z / N - z / 2^(a+b) - 2^a / N > z / N - 2^-24 - 2^-5,
so q is floor(z / N) or one below it and r = z - q N lies in [0, 2N): one conditional subtraction.  The
kernel forms r modulo 2^(27 * 228) (2N < 2^6145), limb by limb in the borrow chain of z - q N.  r may reach
2^6144, one bit more than a row: the subtraction runs on the row's 192 dwords, and is taken when it leaves no
borrow or when that bit (limb 227, bit 15) is set.

chain() is the gathered product of fthe_gprod192 (one lazy factor per product), power() the sliding-window walk of
fthe_pow192 (both factors lazy) with its schedule builder: schedule(), products(), plan().  inverse() is the radix-8
tree of fthe_inv192_up / fthe_inv192_down with its count and workspace formulas: inverse_levels(),
inverse_products(), inverse_blocks(), inverse_ws_bytes().  horner() is the walk over planes of fthe_horner192
(DESIGN.md 27), horner_products() its count.

Run:  python tools/mul192_model.py [seed] [trials]
"""
import random
import sys

import numpy as np

B = 27
MASK = (1 << B) - 1
LANES, PER = 8, 29
LIMBS = LANES * PER                 # 232
WORDS = 192
SHIFT_A, SHIFT_B = 225, 231         # limbs
R_LIMBS = 228


def edge_moduli(seed=3072):
    """odd n at the edges of the range: the largest and the smallest N, a 3071-bit n, N just below and just above
    2^6143, and a seeded random 3072-bit n (none needs to be a semiprime)"""
    from math import isqrt
    s = isqrt(1 << 6143)
    lo = s - (1 - s % 2)
    assert lo * lo < 1 << 6143 < (lo + 2) ** 2
    return [(1 << 3072) - 1, (1 << 3040) + 1, (1 << 3071) - 1, lo, lo + 2,
            random.Random(seed).getrandbits(3072) | (1 << 3071) | 1]


def n_ok(n):
    return n % 2 == 1 and 3041 <= n.bit_length() <= 3072


def limbs(v, count=LIMBS):
    assert 0 <= v < 1 << (B * count)
    return [(v >> (B * j)) & MASK for j in range(count)]


def value(ls):
    return sum(int(x) << (B * j) for j, x in enumerate(ls))


def mu_of(N):
    return (1 << (B * (SHIFT_A + SHIFT_B))) // N


def image(n):
    """the kernel's per-key context bytes (mul192_image.hpp): mu limbs, N limbs, N dwords"""
    assert n_ok(n)
    N = n * n
    mu = mu_of(N)
    assert mu < 1 << (B * SHIFT_B)
    words = limbs(mu) + limbs(N) + [(N >> (32 * j)) & 0xFFFFFFFF for j in range(WORDS)]
    return np.array(words, dtype="<u4").tobytes()


def ring(xl, ml, drain=True):
    """the limbs of value(xl) * value(ml) as the octet forms them: 232 (drain: 464) of them"""
    x = np.array(xl, dtype=np.uint64).reshape(LANES, PER)
    acc = np.zeros((LANES, PER), dtype=np.uint64)
    out, carry, peak = [], 0, 0
    for s in range(2 * LIMBS if drain else LIMBS):
        t = s % PER
        if s < LIMBS:
            acc[:, (t + np.arange(PER)) % PER] += x * np.uint64(ml[s])
            peak = max(peak, int(acc.max()))
        carry += int(acc[0, t])
        peak = max(peak, carry)
        out.append(carry & MASK)
        carry >>= B
        acc[:-1, t] = acc[1:, t]
        acc[-1, t] = 0
    assert peak < 1 << 62, "64-bit column overflow"
    assert not drain or (carry == 0 and not acc.any())
    return out


def mul(x, y, n, lanes=False):
    """x y mod n^2 step by step; lanes: the three products through ring() (slow), else by Python integers"""
    assert n_ok(n) and 0 <= x < 1 << (32 * WORDS) and 0 <= y < 1 << (32 * WORDS)
    N = n * n
    mu = mu_of(N)
    assert 1 << 6080 <= N < 1 << 6144 and mu < 1 << (B * SHIFT_B)
    prod = (lambda a, b: value(ring(limbs(a), limbs(b)))) if lanes else (lambda a, b: a * b)
    z = prod(x, y)
    assert z == x * y and z < 1 << (B * (SHIFT_A + SHIFT_B))
    z1 = z >> (B * SHIFT_A)
    assert z1 < 1 << (B * SHIFT_B)                       # fits the operand registers (232 limbs)
    q = prod(z1, mu) >> (B * SHIFT_B)
    assert q < 1 << (B * 230) and z // N - 1 <= q <= z // N
    if lanes:
        t = ring(limbs(q), limbs(N), drain=False)        # the low 232 limbs of q N
        zl, rl, borrow = limbs(z, 2 * LIMBS), [], 0
        for s in range(LIMBS):
            d = (zl[s] - t[s] - borrow) & 0xFFFFFFFF
            borrow = d >> 31
            rl.append(d & MASK if s < R_LIMBS else 0)
        r = value(rl)
    else:
        r = (z - q * N) % (1 << (B * R_LIMBS))
    assert r == z - q * N and 0 <= r < 2 * N
    # the row holds r mod 2^6144; r >= N when the subtraction leaves no borrow or r has a bit above the row
    row, high = r % (1 << (32 * WORDS)), r >> (32 * WORDS)
    assert high == limbs(r)[R_LIMBS - 1] >> (32 * WORDS % B)
    if high or row >= N:
        row = (row - N) % (1 << (32 * WORDS))
    r = row
    assert r == x * y % N
    return r


def chain(rows, n, lanes=False, observer=None):
    """prod(rows) mod n^2 as fthe_gprod192 forms it: the first row is the multiplier column, every
    further row x gives z = x r and the lazy remainder r = z - q N in [0, 2N), which stays in limbs as the next
    multiplier; only the last r is made canonical.  Fewer than two rows are filled up with the integer 1, so there is
    always one product.  The multiplier is now below 2N <= 2^6145, not below 2^6144:
        z  = x r              < 2^(6144 + 6145) = 2^12289
        z1 = floor(z / 2^a)   < 2^6214                     231 limbs (below 2^6237)
        q  = floor(z1 mu/2^b) <= z / N < 2^6209            230 limbs (below 2^6210)
        z1 mu / 2^b > z / N - z / 2^(a+b) - 2^a / N > z / N - 2^-23 - 2^-5
    so q is still floor(z / N) or one below it, and r < 2N < 2^(27 * 228) with limbs 228..231 zero.  Every bound is
    asserted.  lanes: the three products of every step through ring() (slow).  observer: as lazy_product()'s and
    canonical()'s."""
    assert n_ok(n) and all(0 <= x < 1 << (32 * WORDS) for x in rows)
    N = n * n
    mu = mu_of(N)
    prod = (lambda a, b: value(ring(limbs(a), limbs(b)))) if lanes else (lambda a, b: a * b)
    rows = list(rows) + [1] * (2 - len(rows))
    r = rows[0]
    for x in rows[1:]:
        assert r < 1 << 6145 and limbs(r)[R_LIMBS:] == [0] * (LIMBS - R_LIMBS)
        col = r
        z = prod(x, r)
        assert z == x * r and z < 1 << 12289
        z1 = z >> (B * SHIFT_A)
        assert z1 < 1 << 6214 < 1 << (B * SHIFT_B)
        t = prod(z1, mu)
        assert t < 1 << (B * 2 * LIMBS)                      # the 464 limbs the drain retires
        q = t >> (B * SHIFT_B)
        assert q < 1 << 6209 < 1 << (B * 230) and z // N - 1 <= q <= z // N
        if lanes:
            low = ring(limbs(q), limbs(N), drain=False)
            zl, rl, borrow = limbs(z, 2 * LIMBS), [], 0
            for s in range(LIMBS):
                d = (zl[s] - low[s] - borrow) & 0xFFFFFFFF
                borrow = d >> 31
                rl.append(d & MASK if s < R_LIMBS else 0)
            r = value(rl)
        else:
            r = (z - q * N) % (1 << (B * R_LIMBS))
        assert r == z - q * N and 0 <= r < 2 * N
        if observer is not None:
            observer("product", x, col, r, q == z // N)
    if observer is not None:
        observer("canonical", r)
    row, high = r % (1 << (32 * WORDS)), r >> (32 * WORDS)
    assert high == limbs(r)[R_LIMBS - 1] >> (32 * WORDS % B)
    if high or row >= N:
        row = (row - N) % (1 << (32 * WORDS))
    want = 1
    for x in rows:
        want = want * x % N
    assert row == want
    return row


MAX_WINDOW = 5


def schedule(e, w):
    """the walk of fthe_pow192 for e >= 1 as one byte string (mul192_image.hpp pow_schedule restates it): sliding
    windows of at most w bits over a table of odd powers, entry j = x^(2 j - 1).  Byte 0 is the entry that seeds the
    running value; every further byte is 0 for a square or j for a product by entry j."""
    assert e >= 1 and 1 <= w <= MAX_WINDOW
    s, i = [], e.bit_length() - 1
    while i >= 0:
        if not (e >> i) & 1:
            s.append(0)
            i -= 1
            continue
        lo = max(i - w + 1, 0)
        while not (e >> lo) & 1:
            lo += 1
        v = (e >> lo) & ((1 << (i - lo + 1)) - 1)
        if s:
            s += [0] * (i - lo + 1)
        s.append((v + 1) // 2)
        i = lo - 1
    return bytes(s)


def products(sched, tail):
    """products per row: the base by 1, the table (x^2, then one per entry after the first; only the entries the
    walk uses are built), the walk, and the tail's product by t"""
    entries = max(sched)
    return 1 + (entries if entries > 1 else 0) + len(sched) - 1 + (1 if tail else 0)


def plan(e, tail=False, wmax=MAX_WINDOW):
    """(w, schedule) with the fewest products among w = 1 .. wmax, the smaller w on a tie"""
    return min(((w, schedule(e, w)) for w in range(1, wmax + 1)), key=lambda p: (products(p[1], tail), p[0]))


def lazy_product(xl, r, N, lanes=False, ran=None, observer=None):
    """registers xl times the multiplier column r, both below 2^6145 -> the lazy remainder in [0, 2N): one product of
    fthe_pow192 and of the inverse kernels, every bound of power()'s docstring asserted.  ran[0] counts the calls.
    observer: called as observer("product", xl, r, out, exact) after every product, exact telling whether the
    quotient was floor(z / N) (out < N) or one below it; canonical() calls it as observer("canonical", r) and
    inverse() as observer("phase", name) where a sweep begins.  It changes no result."""
    prod = (lambda a, b: value(ring(limbs(a), limbs(b)))) if lanes else (lambda a, b: a * b)
    mu = mu_of(N)
    assert xl < 1 << 6145 and r < 1 << 6145 and limbs(r)[R_LIMBS:] == [0] * (LIMBS - R_LIMBS)
    z = prod(xl, r)
    assert z == xl * r and z < 1 << 12290
    z1 = z >> (B * SHIFT_A)
    assert z1 < 1 << (B * SHIFT_B)
    zm = prod(z1, mu)
    assert zm < 1 << (B * 2 * LIMBS)
    q = zm >> (B * SHIFT_B)
    assert q < 1 << (B * 230) and z // N - 1 <= q <= z // N
    if lanes:
        low = ring(limbs(q), limbs(N), drain=False)
        zl, rl, borrow = limbs(z, 2 * LIMBS), [], 0
        for s in range(LIMBS):
            d = (zl[s] - low[s] - borrow) & 0xFFFFFFFF
            borrow = d >> 31
            rl.append(d & MASK if s < R_LIMBS else 0)
        out = value(rl)
    else:
        out = (z - q * N) % (1 << (B * R_LIMBS))
    assert out == z - q * N and 0 <= out < 2 * N
    if ran is not None:
        ran[0] += 1
    if observer is not None:
        observer("product", xl, r, out, q == z // N)
    return out


def canonical(r, N, observer=None):
    """step 4: a lazy remainder in [0, 2N) -> the row in [0, N)"""
    if observer is not None:
        observer("canonical", r)
    row, high = r % (1 << (32 * WORDS)), r >> (32 * WORDS)
    assert high == limbs(r)[R_LIMBS - 1] >> (32 * WORDS % B)
    if high or row >= N:
        row = (row - N) % (1 << (32 * WORDS))
    assert row == r % N
    return row


RADIX = 8
ENTRY_BYTES = 32 * LANES * 4        # a lazy limb row: each lane's 29 limbs padded to 32 words
PER_WG = 64                         # rows (here: groups) of a workgroup's eight waves


def inverse_levels(count):
    """rows of level 0 .. t of the radix-8 tree: a row per group of 8 of the level below, down to at most 8 rows"""
    ms = [count]
    while ms[-1] > RADIX:
        ms.append(-(-ms[-1] // RADIX))
    return ms


def inverse_products(count, with_a):
    """products as the kernels run them (fthe_last_montmuls): per level below the top 7 per group up and 14 down, 8
    more per group of level 0 for a; a tree that is the top alone multiplies its rows by a on fthe_mul192"""
    ms = inverse_levels(count)
    if len(ms) == 1:
        return count if with_a else 0
    return 21 * sum(ms[1:]) + (8 * ms[1] if with_a else 0)


def inverse_blocks(count, n_cu):
    """workgroups of the level-0 launches, one per CU at most; none when the tree is the top alone"""
    return 0 if count <= RADIX else min(-(-(-(-count // RADIX)) // PER_WG), max(n_cu, 1))


def inverse_ws_bytes(count, blocks):
    """workspace of one tree: the rows of the levels above level 0 (the top's own rows when it stands alone), 7 prefix
    entries per group of every level below the top, a parking entry per slot (workgroup, wave, octet)"""
    ms = inverse_levels(count)
    rows = count if len(ms) == 1 else sum(ms[1:])
    return rows * WORDS * 4 + sum(ms[1:]) * (RADIX - 1) * ENTRY_BYTES + blocks * PER_WG * ENTRY_BYTES


def inverse(N, xs, a=None, offset=0, n=None, lanes=False, count=None, observer=None):
    """[a_i x_i^-1 (1 + offset n) mod N] (a None: 1) as fthe_inv192_up / fthe_inv192_down form it, N =
    n^2 (n None: its root), xs any rows of 192 words that are units mod N.  Groups of eight consecutive rows of a level,
    a short last group filled up with 1; the level above holds the groups' products as canonical rows; the first level
    of at most 8 rows is inverted on Python's integers as the host does it; going down, group g turns R_7 = row g of
    the level above into I_j = R_j p_(j-1) (times a_j at level 0) and R_(j-1) = R_j x_j for j = 7 .. 1, I_0 = R_0.
    Every product goes through lazy_product(), which asserts power()'s bounds.  count: a list that receives the
    number of products run.  observer: lazy_product()'s, told "up", "top" (a tree that is the top alone: its products by a
    on fthe_mul192) and "down" as phases.  Returns the canonical rows."""
    from math import isqrt
    n = isqrt(N) if n is None else n
    assert n_ok(n) and n * n == N and all(0 <= v < 1 << (32 * WORDS) for v in list(xs) + list(a or []))
    ran = [0]

    def step(xl, r):
        return lazy_product(xl, r, N, lanes, ran, observer)

    def canon(r):
        return canonical(r, N, observer)

    def phase(name):
        if observer is not None:
            observer("phase", name)

    ms = inverse_levels(len(xs))
    phase("up")
    levels, prefixes = [list(xs)], []
    for m in ms[1:]:                                      # up
        src, pre, tot = levels[-1], [], []
        for g in range(m):
            x = (src[RADIX * g:RADIX * g + RADIX] + [1] * RADIX)[:RADIX]
            p = [x[0]]
            for j in range(1, RADIX):
                p.append(step(x[j], p[-1]))
            pre.append(p[:RADIX - 1])
            tot.append(canon(p[-1]))
        prefixes.append(pre)
        levels.append(tot)
    top = [v % N for v in levels[-1]]                     # the host: prefix products, one inversion, walk back
    inv = pow(reduce_mod(top, N), -1, N) * (1 + offset * n) % N
    invs = [0] * len(top)
    for j in reversed(range(len(top))):
        invs[j] = inv * reduce_mod(top[:j], N) % N
        inv = inv * top[j] % N
    if len(ms) == 1 and a is not None:
        phase("top")
        invs = [canon(step(a[i], invs[i])) for i in range(len(xs))]
    phase("down")
    for l in reversed(range(len(ms) - 1)):                # down
        src, out = levels[l], [None] * ms[l]
        for g in range(ms[l + 1]):
            x = (src[RADIX * g:RADIX * g + RADIX] + [1] * RADIX)[:RADIX]
            r = invs[g]
            for j in reversed(range(RADIX)):
                i = step(prefixes[l][g][j - 1], r) if j else r
                if l == 0 and a is not None:
                    i = step(a[RADIX * g + j] if RADIX * g + j < ms[l] else 1, i)
                if RADIX * g + j < ms[l]:
                    out[RADIX * g + j] = canon(i)
                if j:
                    r = step(x[j], r)
        invs = out
    assert ran[0] == inverse_products(len(xs), a is not None)
    if count is not None:
        count.append(ran[0])
    for i, v in enumerate(invs):
        assert v == (1 if a is None else a[i]) * pow(xs[i], -1, N) * (1 + offset * n) % N
    return invs


def reduce_mod(vs, N):
    r = 1
    for v in vs:
        r = r * v % N
    return r


def power(x, e, n, t=None, w=None, lanes=False, count=None, observer=None):
    """x^e t mod n^2 as fthe_pow192 forms it, e >= 2, x any row of at most 192 words, t any row or None
    (the integer 1); w: the window width, None for plan()'s.  Every product multiplies registers xl by the multiplier
    column r, and from the second product on both are lazy remainders below 2N <= 2^6145:
        z  = xl r             < 2^12290 < 2^(a + b) = 2^12312
        z1 = floor(z / 2^a)   < 2^6215 < 2^(27 * 231)
        q  = floor(z1 mu/2^b) <= z / N < 2^6210 = 2^(27 * 230)
        z1 mu                 < 2^(6215 + 6232) < 2^(27 * 464)
        z1 mu / 2^b > z / N - z / 2^(a+b) - 2^a / N > z / N - 2^-22 - 2^-5
    so q is floor(z / N) or one below it and r = z - q N stays in [0, 2N) with limbs 228..231 zero.  Each bound, and
    ring()'s column sum below 2^62 where lanes is set, is asserted at every product.  count: a list that receives the
    number of products run.  observer: lazy_product()'s.  Returns the canonical result."""
    assert n_ok(n) and e >= 2 and 0 <= x < 1 << (32 * WORDS) and (t is None or 0 <= t < 1 << (32 * WORDS))
    N = n * n
    ran = [0]

    def step(xl, r):
        return lazy_product(xl, r, N, lanes, ran, observer)

    sched = schedule(e, w) if w else plan(e, t is not None)[1]
    entries = max(sched)
    table = [step(x, 1)]                                  # the base by 1: entry 1
    if entries > 1:
        r = step(table[0], table[0])                      # x^2, parked in the last entry's place
        x2 = r
        for k in range(1, entries):
            r = step(table[0] if k == 1 else x2, r)       # x^2 times the entry before (k = 1: x times x^2)
            table.append(r)
    r = table[sched[0] - 1]
    for j in sched[1:]:
        r = step(table[j - 1] if j else r, r)
    if t is not None:
        r = step(t, r)
    assert ran[0] == products(sched, t is not None)
    if count is not None:
        count.append(ran[0])
    row = canonical(r, N, observer)
    assert row == pow(x, e, N) * (1 if t is None else t) % N
    return row


def horner_products(planes, sq):
    """products of one row of fthe_horner192: the seed by 1, then sq squarings and a product per plane below the top"""
    return 1 + (planes - 1) * (sq + 1)


def horner(xs, sq, n, lanes=False, count=None, observer=None):
    """prod_j xs[j]^(2^(j sq)) mod n^2 as fthe_horner192 forms one output row: xs the row's planes from
    plane 0 up, any rows of 192 words, sq >= 1.  A lone plane is the device copy of its row: no product, the row as it
    is (a row >= N stays so).  Else Horner from the top plane: the seed xs[-1] times the column 1, then per plane below
    it sq squarings of the multiplier column and one product by that plane's row.  The seed and the rows are below
    2^6144, the column after the seed a lazy remainder below 2N <= 2^6145: every product is power()'s case, whose
    bounds lazy_product() asserts.  count: a list that receives the number of products run.  observer:
    lazy_product()'s.  Returns the canonical result."""
    assert n_ok(n) and sq >= 1 and xs and all(0 <= v < 1 << (32 * WORDS) for v in xs)
    N = n * n
    ran = [0]
    if len(xs) == 1:
        if count is not None:
            count.append(0)
        return xs[0]

    def step(xl, r):
        return lazy_product(xl, r, N, lanes, ran, observer)

    r = step(xs[-1], 1)
    for x in reversed(xs[:-1]):
        for _ in range(sq):
            r = step(r, r)
        r = step(x, r)
    assert ran[0] == horner_products(len(xs), sq)
    if count is not None:
        count.append(ran[0])
    row = canonical(r, N, observer)
    assert row == reduce_mod([pow(x, 1 << (j * sq), N) for j, x in enumerate(xs)], N)
    return row


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    trials = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rng = random.Random(seed)
    top = (1 << (32 * WORDS)) - 1
    for n in edge_moduli(seed):
        assert mul(top, top, n, lanes=True) == top * top % (n * n)
        for _ in range(trials):
            x, y = rng.getrandbits(32 * WORDS), rng.getrandbits(32 * WORDS)
            mul(x, y, n, lanes=trials <= 4)
        chain([top] * 3 + [rng.getrandbits(32 * WORDS) for _ in range(5)], n, lanes=trials <= 4)
        power(top, n, n, t=top)
        power(rng.getrandbits(32 * WORDS), rng.getrandbits(12) | 2, n, w=3, lanes=trials <= 4)
        N = n * n
        inverse(N, [top // N * N - 1, N - 1, 2, 1] * 3, a=[top] * 12, offset=1, n=n)
        horner([top, rng.getrandbits(32 * WORDS), top], 3, n, lanes=trials <= 4)
    print("mul192 model: ok")


if __name__ == "__main__":
    main()
