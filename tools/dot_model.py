"""Per-row plaintext weights on Python integers (include/fthe.h fthe_scalar_mul_rows / fthe_dot_segments;
DESIGN.md 21): the windowed per-row power and the bucket (Pippenger) dot product exactly as the engine orders
them, each counting the products mod n^2 it makes, the closed forms of those counts, and the product-count model
that picks the dot product's form (mirrored in fthe.hip dot_plan and exposed by fthe_debug_dot_plan).

A product is counted whenever two rows are multiplied, a factor 1 included: the engine launches whole row ranges
and does not look at their values.  Taking a table row, the integer 1 or a copy costs nothing."""

ROW_WINDOW = 4                  # the per-row power's window width
TABLE_PRODUCTS = 14             # x^2 .. x^15 from x
GROUP = 8                       # members of one group of the segmented product (GatherProd::K)
LAUNCH = 32768                  # dot_plan: what one launch of the digit-weight loop costs, in products, however few its rows


class Counter:
    """Multiplies mod n2 and counts."""

    def __init__(self, n2):
        self.n2, self.products = n2, 0

    def mul(self, a, b):
        self.products += 1
        return a * b % self.n2


def windows(bits, w):
    return (bits + w - 1) // w


def digit(e, j, w):
    return (e >> (j * w)) & ((1 << w) - 1)


# ---- the per-row power -----------------------------------------------------------------------------------------
def rows_products(bits):
    """Products per row of fthe_scalar_mul_rows when the call's largest exponent has `bits` bits."""
    return TABLE_PRODUCTS + 5 * (windows(bits, ROW_WINDOW) - 1) if bits > 0 else 0


def scalar_mul_rows(xs, es, n2):
    """([x^e mod n2], products): the table x^1 .. x^15, acc = T[top digit], then per lower window four squarings
    and a product by T[digit] (by 1 for a zero digit).  Windows above the largest exponent's are not run."""
    c = Counter(n2)
    bits = max((e.bit_length() for e in es), default=0)
    if bits == 0:
        return [1 % n2 for _ in xs], 0
    nwin = windows(bits, ROW_WINDOW)
    out = []
    for x, e in zip(xs, es):
        tab = [1, x % n2]
        for _ in range(TABLE_PRODUCTS):
            tab.append(c.mul(tab[-1], tab[1]))
        acc = tab[digit(e, nwin - 1, ROW_WINDOW)]
        for j in range(nwin - 2, -1, -1):
            for _ in range(4):
                acc = c.mul(acc, acc)
            acc = c.mul(acc, tab[digit(e, j, ROW_WINDOW)])
        out.append(acc % n2)
    return out, c.products


# ---- the segmented product and the bucket products ---------------------------------------------------------------
def segmented_products(sizes):
    """Products the engine's segmented K-way product spends on segments of these sizes: passes of groups of up to
    GROUP members (an empty segment still one group), GROUP - 1 products a group, until one group per segment."""
    total, sizes = 0, list(sizes)
    while True:
        groups = [max(1, (s + GROUP - 1) // GROUP) for s in sizes]
        total += (GROUP - 1) * sum(groups)
        if all(g == 1 for g in groups):
            return total
        sizes = groups


def bucket_pass_products(sizes):
    """Products of the bucket products (fthe.hip dot_bucket_rows): the same passes, but only a group of two
    members or more is multiplied out (GROUP - 1 products, factors 1 for the members it lacks); a group of one
    member or none is copied."""
    total, sizes = 0, list(sizes)
    while True:
        total += (GROUP - 1) * sum(s // GROUP + (s % GROUP >= 2) for s in sizes)
        groups = [max(1, (s + GROUP - 1) // GROUP) for s in sizes]
        if all(g == 1 for g in groups):
            return total
        sizes = groups


def _bucket_rows(c, buckets):
    """Product of every bucket's members, pass by pass over all buckets as dot_bucket_rows runs them."""
    rows = [list(m) for m in buckets]
    while True:
        nxt = []
        for seg in rows:
            groups = []
            for q in range(max(1, (len(seg) + GROUP - 1) // GROUP)):
                grp = seg[q * GROUP:(q + 1) * GROUP]
                if len(grp) < 2:
                    groups.append(grp[0] if grp else 1)
                    continue
                grp += [1] * (GROUP - len(grp))
                acc = grp[0]
                for r in grp[1:]:
                    acc = c.mul(acc, r)
                groups.append(acc)
            nxt.append(groups)
        if all(len(g) == 1 for g in nxt):
            return [g[0] for g in nxt]
        rows = nxt


# ---- the bucket dot product -------------------------------------------------------------------------------------
def horner_products(nwin, w):
    """Per segment: each window below the top costs w squarings, one product into Montgomery form, one by the
    window's row."""
    return (nwin - 1) * (w + 2)


def digit_weight_products(w):
    """Per (segment, window): S <- S R_d and W <- W S for the D - 1 digits below the top one."""
    return 2 * ((1 << w) - 2)


def dot_buckets(xs, es, seg_ptr, idx, n2, w):
    """(out, parts) of the bucket form with window width w: out[s] = prod_t x[idx[t]]^e[t] mod n2.  parts counts the
    products: buckets (the bucket products over the bucket CSR), weights, horner, total; sizes lists the
    bucket sizes."""
    c = Counter(n2)
    nseg = len(seg_ptr) - 1
    terms = seg_ptr[nseg]
    bits = max((es[t].bit_length() for t in range(terms)), default=0)
    if bits == 0:
        return [1 % n2] * nseg, {"buckets": 0, "weights": 0, "horner": 0, "total": 0, "sizes": []}
    nwin, D = windows(bits, w), (1 << w) - 1
    # bucket (s, j, d) at (s nwin + j) D + (D - d): digits descending inside a (segment, window)
    members = [[] for _ in range(nseg * nwin * D)]
    for s in range(nseg):
        for t in range(seg_ptr[s], seg_ptr[s + 1]):
            for j in range(nwin):
                d = digit(es[t], j, w)
                if d:
                    members[(s * nwin + j) * D + (D - d)].append(xs[idx[t] if idx is not None else t] % n2)
    parts = {"sizes": [len(m) for m in members]}
    R = _bucket_rows(c, members)
    parts["buckets"] = c.products
    W = []
    for q in range(nseg * nwin):
        S = acc = R[q * D]
        for i in range(1, D):
            S = c.mul(S, R[q * D + i])
            acc = c.mul(acc, S)
        W.append(acc)
    parts["weights"] = c.products - parts["buckets"]
    out = []
    for s in range(nseg):
        X = W[s * nwin + nwin - 1]
        for j in range(nwin - 2, -1, -1):
            X = c.mul(X, 1)                              # the step into Montgomery form
            for _ in range(w):
                X = c.mul(X, X)
            X = c.mul(X, W[s * nwin + j])
        out.append(X % n2)
    parts["horner"] = c.products - parts["buckets"] - parts["weights"]
    parts["total"] = c.products
    return out, parts


def bucket_sizes(es, seg_ptr, w):
    """Members of every bucket, in bucket order, without multiplying anything."""
    nseg = len(seg_ptr) - 1
    bits = max((es[t].bit_length() for t in range(seg_ptr[nseg])), default=0)
    nwin, D = windows(bits, w), (1 << w) - 1
    sizes = [0] * (nseg * nwin * D)
    for s in range(nseg):
        for t in range(seg_ptr[s], seg_ptr[s + 1]):
            for j in range(nwin):
                d = digit(es[t], j, w)
                if d:
                    sizes[(s * nwin + j) * D + (D - d)] += 1
    return sizes


def composed_products(es, seg_ptr):
    """Products of the composed form: the per-row powers of every term, then the segmented product."""
    nseg = len(seg_ptr) - 1
    bits = max((es[t].bit_length() for t in range(seg_ptr[nseg])), default=0)
    if bits == 0:
        return 0
    return seg_ptr[nseg] * rows_products(bits) + segmented_products([b - a for a, b in zip(seg_ptr, seg_ptr[1:])])


def bucket_products(sizes, nseg, bits, w):
    """Closed form of dot_buckets' count from the bucket sizes, the segments and the largest exponent's bit
    length (one chunk of segments: the engine's passes run over all of a chunk's buckets together)."""
    nwin = windows(bits, w)
    return bucket_pass_products(sizes) + nseg * (nwin * digit_weight_products(w) + horner_products(nwin, w))


def dot_direct(xs, es, seg_ptr, idx, n2):
    """The reference: prod pow(x, e, n2) per segment."""
    out = []
    for s in range(len(seg_ptr) - 1):
        acc = 1 % n2
        for t in range(seg_ptr[s], seg_ptr[s + 1]):
            acc = acc * pow(xs[idx[t] if idx is not None else t], es[t], n2) % n2
        out.append(acc)
    return out


# ---- the choice of form ------------------------------------------------------------------------------------------
def dot_cost(bits, terms, nseg, w):
    """Estimated cost of one form (w = 0: composed) in half products, in integers only so that the C++ mirror agrees
    exactly.  Every term is taken to have a nonzero digit in every window and the grouped products to cost about
    8/7 per member.  Two measured constants: a product of the bucket forms costs 3/2 of one of the
    composed form (gathered operands, Horner on the program kernel), and each of the 2 (D - 1) launches of the
    digit-weight loop costs LAUNCH products however few rows it covers."""
    if w == 0:
        return 2 * (terms * rows_products(bits) + terms + terms // 7 + nseg)
    nwin, D = windows(bits, w), (1 << w) - 1
    entries = terms * nwin
    return 3 * (entries + entries // 7 + nseg * (nwin * 2 * (D - 1) + (nwin - 1) * (w + 2))) + 2 * 2 * (D - 1) * LAUNCH


def dot_plan(bits, terms, nseg):
    """0 (composed), 4 or 8: the cheapest form by dot_cost; ties go to the earlier of 0, 4, 8."""
    if bits <= 0 or terms == 0:
        return 0
    best, best_cost = 0, dot_cost(bits, terms, nseg, 0)
    for w in (4, 8):
        cost = dot_cost(bits, terms, nseg, w)
        if cost < best_cost:
            best, best_cost = w, cost
    return best
