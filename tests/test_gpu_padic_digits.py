"""Single products of the key holder's P-adic kernels on crafted digits, on the real matrix cores.

Every other GPU test of fthe_padic_m37 / m37t / m37s / m37l / k37 is a whole exponentiation, whose digits are as good
as uniform after the first squaring.  Here fthe_debug_padic_prog runs one-op programs on the crafted digits of
tests/digit_cases.py -- the largest admitted digit, digits next to multiples of P, all-ones limbs, products small
enough to clamp Barrett's quotient beside ordinary ones in the same wave, LOADP up to its largest input -- under every
body and prime pair, on both sides of the key, at launches of 1, 63, 64, 65 and 1,100 lanes (more than four
workgroups and a partial wave), each case once in either half of a wave, in a wave other than the first and in a
workgroup other than the first, random digits in the remaining lanes.  Every lane of every launch is checked by
digit_cases.check_padic against Python integers: limbs below 2^28, digits below the bound the next product relies
on, the residue (the plain value after STOREP, below 6 P^2) exact.  The profiling variant ids tell that the intended
body ran: they count launches of at least 64 products per lane, so each test adds one launch of 64 squarings on the
crafted pairs (checked like the rest) and reads which id it went to.  Integer work: no tolerance.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import digit_cases as dc

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 1100)
NPOOL = max(COUNTS)
WAVE, WG = 64, 256
IDS = (1037, 1137, 1237, 1337, 1437)
ANCESTORS = {"k37": (1037,), "m37": (1137,), "m37t": (1137, 1237), "m37s": (1137, 1237, 1337),
             "m37l": (1137, 1237, 1337, 1437)}          # a later body's launches also count under its ancestors'


def _key_with(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", params=[(k, b) for k in dc.PADIC_KEYS for b in dc.BODIES], ids=lambda kb: "-".join(kb))
def keyed(request):
    from fedtree_amd.paillier import Device, Paillier
    name, body = request.param
    dev = Device(0)
    p, q = dc.padic_prime_pairs()[name]
    pl = _key_with(dc.BODY_ENV[body], lambda: Paillier.from_primes(p, q, dev))
    return dev, pl, body, (p, q)


@functools.lru_cache(maxsize=None)
def _pool(P, body):
    """the rows of one (prime, body): every crafted case and NPOOL random fillers per kind, converted to limbs once"""
    rng = dc.make_rng("padic", P, body)
    nd, lim = dc.padic_nd(body), dc.padic_plain_limit(P, body)
    rows = lambda vs: np.array([dc.padic_row(v) for v in vs], dtype=np.uint32)      # noqa: E731
    sq = dc.padic_sqr_pairs(P, body)
    mu = dc.padic_mul_pairs(P, body)
    pv = dc.padic_plain_values(P, body)
    rx = [dc.filler(rng, nd * P) for _ in range(NPOOL)]
    ry = [dc.filler(rng, nd * P) for _ in range(NPOOL)]
    rp = [dc.filler(rng, lim, pair=False) for _ in range(NPOOL)]
    return {"sqr": (sq, rows(sq), rx, rows(rx)), "mula": ([a for a, _ in mu], rows([a for a, _ in mu]), rx, rows(rx)),
            "mulb": ([b for _, b in mu], rows([b for _, b in mu]), ry, rows(ry)), "plain": (pv, rows(pv), rp, rows(rp))}


def _fill(kind, lay):
    cases, crows, rnd, rrows = kind
    vals = [cases[c] if c is not None else rnd[j] for j, c in enumerate(lay)]
    arr = np.stack([crows[c] if c is not None else rrows[j] for j, c in enumerate(lay)])
    return vals, arr


def _launches(dev, fn):
    lib = dev.lib
    lib.fthe_prof_enable(dev.ctx, 1)
    try:
        fn()
        vals = [ctypes.c_double() for _ in range(7)]
        assert lib.fthe_prof_read(dev.ctx, *[ctypes.byref(v) for v in vals]) == 0
        got = {}
        for S in IDS:
            ms, nl = ctypes.c_double(), ctypes.c_double()
            assert lib.fthe_prof_variant(dev.ctx, S, ctypes.byref(ms), ctypes.byref(nl)) == 0
            got[S] = nl.value
    finally:
        lib.fthe_prof_enable(dev.ctx, 0)
    return got


@pytest.mark.parametrize("pn", list(dc.PADIC_PROGS))
def test_program_on_crafted_digits(keyed, pn):
    dev, pl, body, primes = keyed
    prog = dc.PADIC_PROGS[pn]
    out_slot = 2 if dc.MUL in prog[::2] else 1
    for side, P in enumerate(primes):
        ran = dc.padic_body_for(P, body)                     # a P past the four-tile bodies' range falls to m37
        pool = _pool(P, ran)
        kinds = {"io": ("sqr",), "loadp": ("plain",), "sqr_storep": ("sqr",), "sqr2": ("sqr",)}.get(pn, ("mula", "mulb"))
        outs = []

        def run():
            for count in COUNTS:
                lay = dc.rotated_layout(len(pool[kinds[0]][0]), count, WAVE, WG)
                slots = np.zeros((3, count, 2 * dc.PK), dtype=np.uint32)
                vals = []
                for s, k in enumerate(kinds):
                    v, slots[s] = _fill(pool[k], lay)
                    vals.append(v)
                outs.append((prog, count, vals, pl.debug_padic_prog(side, prog, slots, out_slot)))
            # which body the hook's launches run: one more of them with 64 squarings, which the counters see
            cases, crows, _, _ = pool["sqr"]
            outs.append((dc.PADIC_WITNESS, len(cases), [cases],
                         pl.debug_padic_prog(side, dc.PADIC_WITNESS, np.stack([crows, crows]), 1)))
        got = _launches(dev, run)
        assert got == {S: 1.0 if S in ANCESTORS[ran] else 0.0 for S in IDS}, (pn, side, ran, got)
        lanes = 0
        for pr, count, vals, out in outs:
            assert out.shape == (count, 2 * dc.PK)
            for g in range(count):                           # every lane
                try:
                    dc.check_padic(P, ran, pr, {s: v[g] for s, v in enumerate(vals)}, out[g])
                except dc.Mismatch as e:
                    raise AssertionError(f"{pn} side {side} ({ran}) count {count} lane {g}: {e}; inputs "
                                         f"{[hex(x) for v in vals for x in (v[g] if isinstance(v[g], tuple) else (v[g],))]}")
                lanes += 1
        assert lanes == sum(COUNTS) + len(pool["sqr"][0])

