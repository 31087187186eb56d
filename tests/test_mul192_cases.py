"""The crafted inputs of mul192_cases.py against the model (tools/mul192_model.py), host only: every case is in the class
it claims, every chain, power and inverse input passes the model's bounds, the inputs that test_gpu_mul192_lazy.py
sends reach every state that the kernel they go to can reach, and a model of step 4 with the bit or the
lane pass left out is caught by them."""
from math import gcd

import pytest

import mul192_cases as mc
from mul192_cases import mm

MODS = mc.moduli()
ALL = range(len(MODS))


def test_moduli():
    """HIGH are the moduli on which r >= 2^6144 is reachable, by the bound alone; the two added n are legal keys with
    the Barrett fractions the census wants (n = 2^3072 - 1 has none)"""
    assert [ni for ni in ALL if mc.reachable_high(MODS[ni] ** 2)] == list(mc.HIGH)
    frac = lambda N: ((1 << 12312) % N) / N                           # noqa: E731
    assert all(mm.n_ok(n) and n.bit_length() == 3072 for n in mc.HIGH_N)
    assert 0.6 < frac(mc.HIGH_N[0] ** 2) < 0.7 and frac(mc.HIGH_N[1] ** 2) > 0.99 and frac(MODS[0] ** 2) < 2 ** -64
    assert (mc.ROW - mc.HIGH_N[0] ** 2).bit_length() == 6117
    for ni in ALL:                                                    # unreachable: the window is empty
        N = MODS[ni] ** 2
        assert ni in mc.HIGH or mc.ROW - N > N >> 21 or 2 * N <= mc.ROW


@pytest.mark.parametrize("ni", ALL)
def test_cases_are_in_their_class(ni):
    N = MODS[ni] ** 2
    a, b = mc.class_cases(ni), mc.borrow_cases(ni)
    assert {c[3] for c in a} == ({"exact", "low", "high"} if ni in mc.HIGH else {"exact", "low"})
    for name, x, y, want in a:
        c = mc.classify(x, y, N)
        assert mc.klass(x, y, N) == want and c.low == c.ge_n and (not c.high or c.low), name
        assert mm.mul(x, y, MODS[ni]) == x * y % N
    kinds = {name.split()[0] for name, *_ in b}
    assert {"born", "taken", "kept", "armed", "N"} <= kinds            # 2N - 1 needs z mod N = N - 1 with q low: never
    for name, x, y, v in b:
        assert mc.classify(x, y, N).out == v and x < mc.ROW and y < mc.ROW, name
        assert mc.lane_canonical(v, N) == mm.canonical(v, N) == x * y % N, name
    for k in range(8):                                                # a borrow born in every lane, taken in every lane
        assert any(name == f"born {k} * 1" for name, *_ in b) and any(name.startswith(f"taken {k} ") for name, *_ in b)
    if ni in mc.HIGH:
        assert sum(v >= mc.ROW for *_, v in b) >= 2
    assert 8 * len(mc.mul_cases(ni)) <= 1100                          # the layout's large form fits the GPU test's launch


@pytest.mark.parametrize("ni", ALL)
def test_chains(ni):
    n = MODS[ni]
    N, cs = n * n, mc.chains(ni)
    assert sorted(len(c) for c in cs) == [2, 3, 4, 5, 5, 6, 6, 7, 7, 8, 8]
    for c in cs:
        cols = mc.lazy_columns(c, N)
        assert all(gcd(v, N) == 1 and v < mc.ROW for v in c) and mm.chain(c, n) == mc.mm.reduce_mod(c, N)
        assert cols[1] >= (mc.ROW if ni in mc.HIGH else N)             # the first product: the top class
        assert len(c) < 4 or c[2] == mc.ones_row(N)
        # Two consecutive products on a column >= N need six members.  The column after the all-ones row is
        # ones * r1 mod N with r1's residue already fixed by the first product's class, so it cannot be steered too,
        # and is >= N only by chance: the run starts at the member after it (columns r3, r4 under members 5 and 6).
        # A chain of 4 or 5 has r1 and r3 >= N with that free column between them.
        assert len(c) < 6 or mc.run_above(c, N) >= 2
        assert len(c) < 5 or (cols[1] >= N and cols[3] >= N)
    assert all(mc.lazy_columns(c, N)[-1] >= (mc.ROW if ni in mc.HIGH else N) for c in cs[:7])
    assert max(mc.run_above(c, N) for c in cs) >= 4


def test_lanes_walk_one_case_of_each_class():
    """the ring of columns (lanes=True) on one product of each class, a chain, a power and an inverse"""
    ni = 6
    n = MODS[ni]
    N = n * n
    for want in ("exact", "low", "high"):
        x, y = next(c[1:3] for c in mc.class_cases(ni) if c[3] == want)
        assert mm.mul(x, y, n, lanes=True) == x * y % N
        assert mm.canonical(mm.lazy_product(x, y, N, lanes=True), N) == x * y % N
    x, y, v = next(c[1:] for c in mc.borrow_cases(ni) if c[0] == "2^6144 low")
    assert mm.mul(x, y, n, lanes=True) == (v - N) % N
    mm.chain(mc.chains(ni)[2], n, lanes=True)
    mm.power(mc.pow_rows(ni, 3)[-4], 3, n, lanes=True)
    xs, a = mc.inverse_input(ni, 9)
    mm.inverse(N, xs[1:], a=a[1:], offset=1, n=n, lanes=True)


@pytest.mark.parametrize("count", [1, 63, 65, 1100])
def test_layout(count):
    for ncases in (59, 77, 88):
        lay = mc.layout(ncases, count)
        assert len(lay) == count
        if count < 8 * ncases:
            assert None not in lay and len(set(lay)) == min(count, ncases)
            continue
        nwg = -(-count // 64)                                         # fewer than any GPU's CUs
        for i in range(ncases):
            at = [p for p, c in enumerate(lay) if c == i]
            assert sorted(p % 8 for p in at) == [0, 7]                # octet 0 and octet 7
            assert any((p // 8) % nwg for p in at)                    # a workgroup other than the first
            assert any((p // 8) // nwg for p in at)                   # a batch that is not its workgroup's first
    assert len({mc.layout(70, c)[0] for c in (1, 63, 65)}) == 3


def _total(parts):
    return {k: sum(p[k] for p in parts) for k in mc.CELLS}


def gpu_census(ni):
    """the census, kernel by kernel, of what test_gpu_mul192_lazy.py sends on modulus ni"""
    n = MODS[ni]
    N = n * n
    out = {"mul": mc.census("mul", mc.mul_cases(ni), N)}
    rows, seg, idx = mc.gprod_input(ni)
    srows, sseg = mc.scan_input(ni)
    out["gprod"] = _total([mc.census("gprod", mc.gprod_groups(rows, seg, idx), N),
                           mc.census("gprod", mc.scan_groups(srows, sseg), N)])
    if ni in mc.HIGH:
        out["pow"] = _total([mc.census("pow", (mc.pow_rows(ni, e), e, None), N) for e in (2, 3, n)])
    for kernel in ("inv_up", "inv_down"):
        parts = []
        for count in (9, 64, 65):
            x, a = mc.inverse_input(ni, count)
            parts += [mc.census(kernel, (x, None, 0), N), mc.census(kernel, (x, a, 1), N)]
        out[kernel] = _total(parts)
    return out


# the cells a kernel can reach on a modulus of HIGH.  fthe_mul192 and fthe_gprod192 and the up-sweep take their register
# factor from a row, which is below 2^6144; fthe_mul192's column is a row too.
REACH = {"mul": ("out_ge_n", "conv_ge_n", "conv_bit"),
         "gprod": ("col_bit", "out_ge_n", "conv_ge_n", "conv_bit"),
         "pow": ("col_bit", "reg_bit", "both_bit", "out_ge_n", "conv_ge_n", "conv_bit"),
         "inv_up": ("col_bit", "out_ge_n", "conv_ge_n", "conv_bit"),
         "inv_down": ("col_bit", "reg_bit", "out_ge_n", "conv_ge_n", "conv_bit")}


@pytest.mark.parametrize("ni", mc.HIGH)
def test_census_reaches_every_cell(ni):
    got = gpu_census(ni)
    print(ni, got)
    for kernel, cells in REACH.items():
        for cell in mc.CELLS:
            if cell in cells:
                assert got[kernel][cell] > 0, (kernel, cell)
            elif cell.endswith("_bit") and kernel != "inv_down":      # unreachable by construction: stays 0
                assert got[kernel][cell] == 0, (kernel, cell)


def test_census_off_the_high_moduli():
    """the random 3072-bit n: no bit anywhere, every other state still reached"""
    got = gpu_census(5)
    for kernel, c in got.items():
        assert not (c["col_bit"] or c["reg_bit"] or c["conv_bit"]) and c["out_ge_n"] and c["conv_ge_n"], kernel


@pytest.mark.parametrize("ni", mc.HIGH + (1, 5))
def test_inverse_conversions_see_the_borrow_targets(ni):
    """each kernel has its own compiled copy of step 4: the conversions of both sweeps, over the counts and calls that
    the GPU test runs, start from a borrow born in a lane above 0 and from an armed pass that no borrow reaches, and
    step 4 with lanes that never pass a borrow on differs from Python on conversion inputs of either sweep other than
    N - 1 (lane 0's chain, which the hostile rows had)"""
    N = MODS[ni] ** 2
    name = {v: k for k, v in mc.targets(ni).items()}
    for kernel in ("inv_up", "inv_down"):
        conv = []
        for count in (9, 64, 65):
            x, a = mc.inverse_input(ni, count)
            conv += mc.conversion_inputs(kernel, (x, None, 0), N) + mc.conversion_inputs(kernel, (x, a, 1), N)
        seen = {name[v] for v in conv if v in name}
        caught = {name.get(v, "other") for v in conv if mc.lane_canonical(v, N, no_pass=True) != v % N}
        print(ni, kernel, sorted(seen), "caught:", sorted(caught))
        assert all(mc.lane_canonical(v, N) == v % N for v in conv)
        assert any(k.startswith("born") and k != "born 0" for k in seen), kernel
        assert any(k.startswith("armed") and k != "armed 0" for k in seen), kernel
        assert any(k.startswith("born") and k != "born 0" for k in caught), kernel
        if kernel == "inv_down":
            assert {"born", "kept", "armed", "taken"} <= {k.split()[0] for k in seen}
            # the smallest N has three lanes that are not 0: a borrow born below one of them needs no pass above it
            assert len({k for k in seen if k.startswith("born")}) >= 5 and len(caught - {"N - 1", "born 0"}) >= 3


@pytest.mark.parametrize("ni", ALL)
def test_wrong_step_4_is_caught(ni):
    """step 4 with bit 6144 left out of `keep`, or with lanes that never pass a borrow on, differs from Python on a
    crafted case of (a) or (b); the hostile rows and random pairs of the older tests catch neither on HIGH_N"""
    N = MODS[ni] ** 2
    cases = [(c[0], mc.classify(c[1], c[2], N).out) for c in mc.class_cases(ni) + mc.borrow_cases(ni)]
    assert all(mc.lane_canonical(v, N) == v % N for _, v in cases)
    no_pass = [name for name, v in cases if mc.lane_canonical(v, N, no_pass=True) != v % N]
    no_bit = [name for name, v in cases if mc.lane_canonical(v, N, ignore_bit=True) != v % N]
    print(ni, "no pass:", no_pass, "no bit:", no_bit)
    assert sum(name.startswith("born") for name in no_pass) >= 4 and "N - 1 * 1" in no_pass
    assert (len(no_bit) >= 4 and any(name.startswith("high") for name in no_bit)) if ni in mc.HIGH else not no_bit
