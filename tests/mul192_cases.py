"""Crafted inputs for the Paillier-3072 kernels of fthe_mul192.hip, and a census of the states they reach: host only,
built on tools/mul192_model.py.  One list for the CPU tests (test_mul192_cases.py) and the GPU (test_gpu_mul192_lazy.py).

A product multiplies registers x by the multiplier column y; its lazy remainder r = z - q N lies in [0, 2N).  Three
classes: "exact" (q = floor(z / N), r < N), "low" (q one below it, N <= r < 2^6144) and "high" (q one low and
r >= 2^6144: bit 6144, limb 227 bit 15, is set).  q comes out low only when z mod N < loss N with
    loss < z / 2^12312 + 2^6075 / N  (z1 and mu are both rounded down),
and "high" needs z mod N >= 2^6144 - N on top of it.  With N > 2^6143 (else 2N <= 2^6144) the second term is below
2^-68, and z < 2^12290 bounds the first by 2^-22: the state exists only where 2^6144 - N < 2^-22 N, that is for n
within 2^-23 of 2^3072 (2^-25 for fthe_mul192, whose z is below 2^12288).  Of edge_moduli() only n = 2^3072 - 1 is
that close, and its Barrett fraction frac(2^12312 / N) is 2^-2903, so HIGH_N adds two n with fractions 0.66 and
0.999.  On every other modulus of moduli() "high" is unreachable, and says so: reachable_high().

Crafting is a seeded search: for a wanted z mod N = s take a unit column y, x = s / y mod N (plus a multiple of N
where the row has room, so that z is large), and keep the pair only when the model puts it in the wanted class.
"""
import os
import random
import sys
from collections import namedtuple
from math import gcd, isqrt

_TOOLS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)
import mul192_model as mm  # noqa: E402

ROW = 1 << (32 * mm.WORDS)          # 2^6144: a row holds values below it
TOP = ROW - 1                       # the all-ones row
LANE = 768                          # bits of the 24 dwords a lane converts in step 4
HIGH_N = ((1 << 3072) - (1 << 3044) + 1, (1 << 3072) - (1 << 3046) + 1)
HIGH = (0, 6, 7)                    # the moduli() on which r >= 2^6144 is reachable

_CACHE = {}


def moduli():
    return mm.edge_moduli() + list(HIGH_N)


def reachable_high(N):
    """whether a lazy remainder mod N can reach 2^6144 (the bound of the module's docstring, for z < 2^12290)"""
    return N > 1 << 6143 and (ROW - N) << 22 < N + (N >> 40)


# ---- one product ---------------------------------------------------------------------------------------------------
Class = namedtuple("Class", "low ge_n high out")


def classify(x, r, N):
    """the model's view of registers x times column r: quotient one low, lazy result >= N, its bit 6144, the result"""
    seen = []
    out = mm.lazy_product(x, r, N, observer=lambda *e: seen.append(e))
    exact = seen[0][4]
    assert (out >= N) == (not exact)
    return Class(not exact, out >= N, out >= ROW, out)


def klass(x, r, N):
    c = classify(x, r, N)
    return "high" if c.high else "low" if c.low else "exact"


def unit_near_top(N, rng):
    """an odd unit mod N in the top 2^-40 of the rows"""
    while True:
        y = (TOP - (rng.getrandbits(6100) << 1)) | 1
        if gcd(y, N) == 1:
            return y


def ones_row(N):
    """the all-ones row, or where it is no unit mod N (n = 2^3072 - 1 divides it) the row below it"""
    return TOP if gcd(TOP, N) == 1 else TOP - 1


def residue_for(N, want, rng):
    """a random z mod N from which the class `want` can come out"""
    if want == "exact":
        return rng.randrange(N >> 3, N)
    if want == "low":
        return rng.getrandbits(min(3000, (ROW - N).bit_length() - 2)) | 1 if N > 1 << 6143 else rng.getrandbits(3000) | 1
    gap = ROW - N
    return gap + rng.getrandbits(gap.bit_length() - 3 if gap.bit_length() > 6000 else 6000)


def craft(N, want, rng, s=None, col=None, tries=60):
    """(x, y) with x a row, y the column (col, else a fresh unit near 2^6144), x y = s mod N (s None: a fresh residue
    per try) and the product in class `want`; None when `tries` candidates all miss"""
    for _ in range(tries):
        y = unit_near_top(N, rng) if col is None else col
        t = residue_for(N, want, rng) if s is None else s
        if s is None and gcd(t, N) != 1:                  # a crafted row is a unit wherever its residue is free
            continue
        x0 =t * pow(y, -1, N) % N
        for k in range((TOP - x0) // N, -1, -1):
            x = x0 + k * N
            if klass(x, y, N) == want:
                assert classify(x, y, N).out % N == t % N
                return x, y
        if col is not None and s is not None:
            return None
    return None


# ---- (a) the three classes ------------------------------------------------------------------------------------------
def class_cases(ni, per=3):
    """[(name, x, y, class)]: `per` pairs of each class that the modulus admits"""
    if ("a", ni) not in _CACHE:
        N, rng, out = moduli()[ni] ** 2, random.Random(1000 + ni), []
        for want in ("exact", "low") + (("high",) if reachable_high(N) else ()):
            for i in range(per):
                x, y = craft(N, want, rng)
                out.append((f"{want} {i}", x, y, want))
        _CACHE["a", ni] = out
    return _CACHE["a", ni]


# ---- (b) what step 4 converts ---------------------------------------------------------------------------------------
def borrow_targets(N, rng):
    """[(name, v)]: lazy remainders v in [0, 2N) whose subtraction of N walks the lanes' borrow scan in every way"""
    lane = lambda v, k: (v >> (LANE * k)) & ((1 << LANE) - 1)      # noqa: E731
    out = []
    for k in range(8):
        L = 1 << (LANE * k)
        out += [(f"born {k}", N - L), (f"taken {k} - 1", N + L - 1), (f"taken {k}", N + L)]
        if k:
            out.append((f"kept {k}", (N >> (LANE * k) << (LANE * k)) - 1))
        if lane(N, k) + 1 < 1 << LANE:                             # lanes above k equal N's, lane k greater
            v = (N >> (LANE * k + LANE) << (LANE * k + LANE)) | (lane(N, k) + 1) << (LANE * k) | rng.getrandbits(LANE * k)
            assert N < v < ROW and all(lane(v, j) == lane(N, j) for j in range(k + 1, 8)) and lane(v, k) > lane(N, k)
            out.append((f"armed {k}", v))
    out += [("N - 1", N - 1), ("N", N), ("N + 1", N + 1), ("2N - 1", 2 * N - 1)]
    if ROW < 2 * N:                                                    # round bit 6144; the row part is tiny
        out += [("2^6144 - 1", ROW - 1), ("2^6144", ROW)]
        out += [(f"over {k}", ROW + (1 << (LANE * k)) - j) for k in range(1, 8) for j in (1, 0) if ROW + (1 << (LANE * k)) < 2 * N]
    assert all(0 <= v < 2 * N for _, v in out)
    return out


def borrow_cases(ni):
    """[(name, x, y, v)]: products whose conversion input is exactly v (asserted), for the targets above.  v < 2^6144
    comes as v * 1, unless the model's quotient for it is 1 (then the kernel converts v - N, and the case is left
    out); v >= N also as a pair with the quotient one low and z = v - N mod N.  That pair exists only for v - N below
    loss N < N / 16; the targets next to 2N have none, and a target t < N cannot be seen as t + N either."""
    if ("b", ni) not in _CACHE:
        N, rng, out = moduli()[ni] ** 2, random.Random(2000 + ni), []
        for name, v in borrow_targets(N, rng):
            if v < ROW and classify(v, 1, N).out == v:
                out.append((name + " * 1", v, 1, v))
            if v >= N and (v - N) << 4 < N:
                pair = craft(N, "high" if v >= ROW else "low", rng, s=v - N, tries=12)
                if pair:
                    assert classify(*pair, N).out == v
                    out.append((name + " low", pair[0], pair[1], v))
        _CACHE["b", ni] = out
    return _CACHE["b", ni]


def mul_cases(ni):
    """[(x, y)] for fthe_mul192: all of (a) and (b)"""
    return [(c[1], c[2]) for c in class_cases(ni) + borrow_cases(ni)]


def layout(ncases, count):
    """which case each of `count` consecutive rows holds (None: a random row).  A wave's batch is 8 rows, one per
    octet, and workgroup b mod nwg takes batch b.  With room for a batch per case, batch i has case i in octet 0 and
    case i + ncases // 2 + 1 in octet 7: every case sits once in either octet, in two batches that differ.  A smaller
    launch takes the cases in turn from an offset that differs from count to count."""
    out = [None] * count
    if count >= 8 * ncases:
        for i in range(ncases):
            out[8 * i] = i
            out[8 * i + 7] = (i + ncases // 2 + 1) % ncases
    else:
        for j in range(count):
            out[j] = (j + count) % ncases
    return out


# ---- (c) chains -----------------------------------------------------------------------------------------------------
def lazy_columns(rows, N):
    """the columns of chain(rows): rows[0], then every lazy remainder"""
    cols = [rows[0]]
    for x in rows[1:]:
        cols.append(classify(x, cols[-1], N).out)
    return cols


def make_chain(N, length, rng, tail_top=True):
    """`length` >= 2 unit rows: the first product lands in the top class the modulus admits ("high", else "low"), the
    third member is the all-ones row (z next to 2^12289), every later member keeps the column >= N, in the top class
    where the search finds it; tail_top: the last remainder is in the top class too"""
    top = "high" if reachable_high(N) else "low"
    while True:
        x, y = craft(N, top, rng)
        rows, col = [y, x], classify(x, y, N).out
        while len(rows) < length:
            if len(rows) == 2 and length > 3:
                nxt = (ones_row(N), None)
            else:
                last = len(rows) == length - 1
                nxt = craft(N, top, rng, col=col, tries=8) or (None if last and tail_top else craft(N, "low", rng, col=col, tries=8))
            if not nxt:
                break
            rows.append(nxt[0])
            col = classify(nxt[0], col, N).out
        if len(rows) == length and all(gcd(v, N) == 1 for v in rows):
            return rows


def run_above(rows, N):
    """the longest run of consecutive products of chain(rows) whose multiplier column is >= N"""
    best = run = 0
    for c in lazy_columns(rows, N)[1:-1]:
        run = run + 1 if c >= N else 0
        best = max(best, run)
    return best


def chains(ni):
    """chains of 2..8 members whose last remainder is in the top class, and of 5..8 whose last is not forced"""
    if ("c", ni) not in _CACHE:
        N, rng = moduli()[ni] ** 2, random.Random(3000 + ni)
        _CACHE["c", ni] = [make_chain(N, k, rng) for k in range(2, 9)] + [make_chain(N, k, rng, False) for k in (5, 6, 7, 8)]
    return _CACHE["c", ni]


def gprod_input(ni):
    """(rows, seg, idx) for reduce_segments_csr_dev: the (b) cases as groups of one member (v) and of two (y, x), then
    the chains, in an order that mixes the lengths within a wave's eight groups"""
    N = moduli()[ni] ** 2
    groups = []
    for name, x, y, v in borrow_cases(ni):
        groups.append([v] if y == 1 else [y, x])
    cs = chains(ni)
    for i, c in enumerate(cs):
        groups.insert((5 * i + 3) % (len(groups) + 1), c)
    rows, idx, seg = [], [], [0]
    for g in groups:
        for v in g:
            idx.append(len(rows))
            rows.append(v)
        seg.append(len(idx))
    assert all(v < ROW for v in rows) and N
    return rows, seg, idx


def gprod_groups(rows, seg, idx):
    """the member rows of each group of one pass (segments of at most 8 members), in launch order"""
    assert all(b - a <= 8 for a, b in zip(seg, seg[1:]))
    return [[rows[i] for i in idx[a:b]] for a, b in zip(seg, seg[1:])]


def scan_groups(rows, seg):
    """the groups of fthe_scan_segments_dev over segments of at most 8 rows: element t multiplies x[t], x[t - 1], ...
    down to its segment's start"""
    out = []
    for a, b in zip(seg, seg[1:]):
        assert b - a <= 8
        out += [[rows[u] for u in range(t, a - 1, -1)] for t in range(a, b)]
    return out


def scan_input(ni):
    """(rows, seg): an 8-member chain stored last member first, so that the last prefix walks it in order, between
    two short segments"""
    c = chains(ni)[6]
    assert len(c) == 8
    rows = [ones_row(moduli()[ni] ** 2), 3] + c[::-1] + [5]
    return rows, [0, 2, 10, 11]


# ---- fthe_pow192 ----------------------------------------------------------------------------------------------------
def _root(v, p):
    lo, hi = 0, 1 << (v.bit_length() // p + 1)
    while lo < hi:                                                     # the largest lo with lo^p <= v
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if mid ** p <= v else (lo, mid - 1)
    return lo


def pow_rows(ni, e):
    """rows for x^e on a high modulus.  x = N + x0 with x0 small is a legal row whose powers stay small integers:
    where x0^p lies in [2^6144 - N, loss N) the walk's value x^p is the lazy remainder N + x0^p, with bit 6144.  p = 2
    and p = 3 put that into the conversions of e = 2 and e = 3 (and into the column of e = 3's last product); p = the
    power that seeds the walk of e puts it into a square, whose two factors both have the bit.  e = 2, 3 get the rows
    for p = 2, 3, a larger e those for its seed; with them, for every e, the high rows of (a)."""
    N = moduli()[ni] ** 2
    assert reachable_high(N)
    gap = ROW - N
    rows = []
    seed = 2 * mm.plan(e)[1][0] - 1
    for p in (2, 3) if e < 4 else (seed,):
        for num in (5, 6, 9):
            x0 = _root(gap * num // 4, p) + 1
            if gap <= x0 ** p and x0 < gap:
                rows.append(N + x0)
    high = [v for c in class_cases(ni) if c[3] == "high" for v in c[1:3]]
    return rows + high


# ---- (d) the inverse -------------------------------------------------------------------------------------------------
def targets(ni):
    """{name: v} of borrow_targets() as borrow_cases() draws them"""
    if ("t", ni) not in _CACHE:
        _CACHE["t", ni] = dict(borrow_targets(moduli()[ni] ** 2, random.Random(2000 + ni)))
    return _CACHE["t", ni]


def _residue(v, N):
    return v if v < N else v - N


def target_groups(ni, rng):
    """groups of eight for the targets of (b) whose residue is a unit: seven rows t^-1, which the down-sweep of
    invert turns into the lazy remainder t (t >= N: where its quotient comes out one low), and an eighth row that
    steers the group's product, the up-sweep's conversion input, to a further target (a borrow born in a lane above
    0, an armed pass, a kept lane) where the search finds such a row"""
    N = moduli()[ni] ** 2
    t = targets(ni)
    down = [k for k in t if k.split()[0] in ("born", "kept", "armed") or k.endswith("- 1")]
    down = [k for k in down if _residue(t[k], N) and gcd(_residue(t[k], N), N) == 1]
    up = [k for k in ("born 1", "armed 1", "born 4", "kept 2", "born 6", "armed 3", "born 2", "kept 5", "born 7") if k in t]
    groups = []
    for at in range(0, len(down), 7):
        rows = [pow(_residue(t[k], N), -1, N) for k in down[at:at + 7]]
        while len(rows) < 7:
            rows.append(unit_near_top(N, rng))
        v = t[up[len(groups) % len(up)]]
        last = craft(N, "exact" if v < N else "high" if v >= ROW else "low", rng, s=_residue(v, N), col=lazy_columns(rows, N)[-1])
        groups.append(rows + [last[0] if last and gcd(last[0], N) == 1 else unit_near_top(N, rng)])
    return groups


def inverse_input(ni, count):
    """(x, a) for invert_dev and sub_inv_dev(offset=1) over `count` rows, all x units, a all-ones.  Groups of eight,
    taken in turn from a start that differs from count to count: chains of (c), whose prefixes the up-sweep forms and
    the down-sweep reads back as register factors; rows t^-1 for small residues t, which the down-sweep converts and
    stores as lazy N + t (the offset-1 call sees them through rows (1 + n) t^-1, and multiplies them by a as
    columns); target_groups(), which put the borrow patterns of (b) into both sweeps' conversions."""
    key = ("d", ni)
    if key not in _CACHE:
        n = moduli()[ni]
        N, rng = n * n, random.Random(4000 + ni)
        top = "high" if reachable_high(N) else "low"
        small = []
        while len(small) < 24:
            t = residue_for(N, top, rng)
            small += [t] if gcd(t, N) == 1 else []
        small += [1 << (LANE * k) for k in range(1, 8)]
        inv0 = [pow(t, -1, N) for t in small[:8]]
        inv1 = [(1 + n) * pow(t, -1, N) % N for t in small[8:16]]
        inv2 = [pow(t, -1, N) * (1 + (i % 2) * n) % N for i, t in enumerate(small[16:24])]
        lanes = [pow(t, -1, N) for t in small[-7:]] + [N - 1]
        fixed = [make_chain(N, 8, rng), inv0, inv1, make_chain(N, 8, rng, False), lanes, inv2, make_chain(N, 8, rng)]
        tg = target_groups(ni, rng)
        groups = []
        while fixed or tg:                                # the two kinds in turn
            groups += [fixed.pop(0)] if fixed else []
            groups += [tg.pop(0)] if tg else []
        assert all(len(g) == 8 and all(0 < v < ROW and gcd(v, N) == 1 for v in g) for g in groups)
        _CACHE[key] = groups, [unit_near_top(N, rng) for _ in range(8)]
    groups, extra = _CACHE[key]
    turn = {9: 3, 64: 0, 65: 8}.get(count, count) % len(groups)
    x = [v for g in groups[turn:] + groups[:turn] for v in g][:count // 8 * 8] + extra
    assert count <= len(x) and count // 8 <= len(groups)
    return x[:count], [TOP] * count


def conversion_inputs(kernel, inputs, N):
    """the lazy remainders that the conversions of "inv_up" / "inv_down" on `inputs` (as census() takes them) start from"""
    seen, on = [], [False]

    def watch(kind, *e):
        if kind == "phase":
            on[0] = e[0] == kernel[4:]
        elif kind == "canonical" and on[0]:
            seen.append(e[0])
    x, a, offset = inputs
    mm.inverse(N, list(x), a=None if a is None else list(a), offset=offset, n=isqrt(N), observer=watch)
    return seen


# ---- step 4 as the lanes run it ----------------------------------------------------------------------------------------
def lane_canonical(v, N, ignore_bit=False, no_pass=False):
    """canonical_dwords on Python integers, lane for lane: each lane's own borrow g of r - N over its 768 bits, `pass`
    where its difference is 0, the borrow handed up lane by lane, `keep` from the last borrow and bit 6144.  The two
    switches are the mistakes the crafted cases exist to catch: the bit left out of keep, and a lane that never passes
    a borrow on."""
    mask = (1 << LANE) - 1
    row, high = v % ROW, v >> (32 * mm.WORDS)
    r = [(row >> (LANE * k)) & mask for k in range(8)]
    nd = [(N >> (LANE * k)) & mask for k in range(8)]
    bins, bout = [], 0
    for k in range(8):
        bins.append(bout)
        bout = int(r[k] < nd[k] or (r[k] == nd[k] and bout and not no_pass))
    if bout and (ignore_bit or not high):
        return row
    return sum(((r[k] - nd[k] - bins[k]) & mask) << (LANE * k) for k in range(8))


# ---- the census ------------------------------------------------------------------------------------------------------
CELLS = ("products", "col_bit", "reg_bit", "both_bit", "out_ge_n", "conversions", "conv_ge_n", "conv_bit")


class Census:
    """an observer of the model that counts, over the phases it is told to watch"""

    def __init__(self, N, phases=None):
        self.N, self.phases, self.on = N, phases, phases is None
        self.n = dict.fromkeys(CELLS, 0)

    def __call__(self, kind, *e):
        if kind == "phase":
            self.on = self.phases is None or e[0] in self.phases
        elif self.on and kind == "product":
            xl, col, out, _ = e
            self.n["products"] += 1
            self.n["col_bit"] += col >= ROW
            self.n["reg_bit"] += xl >= ROW
            self.n["both_bit"] += col >= ROW and xl >= ROW
            self.n["out_ge_n"] += out >= self.N
        elif self.on and kind == "canonical":
            self.n["conversions"] += 1
            self.n["conv_ge_n"] += e[0] >= self.N
            self.n["conv_bit"] += e[0] >= ROW


def census(kernel, inputs, N):
    """the counts of CELLS over exactly the products and conversions that `kernel` runs on `inputs`:
    "mul"       [(x, y)]: one product and one conversion each;
    "gprod"     the groups of a launch in order: a wave's eight groups all run max(2, its longest group) - 1 products, a
                shorter group multiplying by 1;
    "pow"       (rows, e, t rows or None);
    "inv_up", "inv_down"   (x, a or None, offset): the sweep's share of inverse()."""
    n = isqrt(N)
    assert n * n == N
    if kernel in ("inv_up", "inv_down"):
        c = Census(N, ("up",) if kernel == "inv_up" else ("down",))
        x, a, offset = inputs
        mm.inverse(N, list(x), a=None if a is None else list(a), offset=offset, n=n, observer=c)
        return c.n
    c = Census(N)
    if kernel == "mul":
        for x, y in inputs:
            mm.canonical(mm.lazy_product(x, y, N, observer=c), N, observer=c)
    elif kernel == "gprod":
        for at in range(0, len(inputs), 8):
            wave = inputs[at:at + 8]
            steps = max(2, max(len(g) for g in wave)) - 1
            for g in wave:
                mm.chain((list(g) or [1]) + [1] * (steps + 1 - max(len(g), 1)), n, observer=c)
    elif kernel == "pow":
        rows, e, t = inputs
        for i, x in enumerate(rows):
            mm.power(x, e, n, t=None if t is None else t[i], observer=c)
    else:
        raise ValueError(kernel)
    return c.n
