"""tools/msb_model.py, the bit-exact model of the classical MSB-first product MULWC / MULWGC
(gen_montprog.py), against Python's a x mod N at both ends of the range MontMod::classical_ok
(bn_host.hpp) admits, N >= 2^(27 * 152 - 11) = 2^4093: the synthetic ends 2^4093 + 1 and 2^4096 - 1, the
addb threshold 2^4094 -+ 1, and the prime-product edge keys of tests/golden/n2_edge_keys.json.  check=True
asserts the model's invariant after every step (0 <= value < 2N, |column| < 2^63, q < 2^29).  X is canonical (the
kernel's CANON guarantees it); the A row is never canonicalised, so A also takes rows >= N.  CPU only."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import msb_model  # noqa: E402
import n2_edges as ne  # noqa: E402

S = 152
MODULI = {
    "2^4093+1": (1 << 4093) + 1,
    "2^4094-1": (1 << 4094) - 1,
    "2^4094+1": (1 << 4094) + 1,
    "2^4096-1": (1 << 4096) - 1,
    "cls_lo": None, "cls_hi": None, "addb_lo": None, "addb_hi": None,
}


def _N(name):
    return MODULI[name] or ne.modulus(name)


@pytest.mark.parametrize("name", list(MODULI))
def test_model_is_exact_with_invariant(name):
    N = _N(name)
    assert N.bit_length() >= 27 * S - 10                      # classical_ok
    xs = [0, 1, 2, N - 1, N - 2, N // 2, N - (1 << 64)]
    As = xs + [N, N + 12345, (1 << 4096) - 1]
    rng = random.Random(len(name))
    pairs = [(a, x) for a in As for x in xs]
    pairs += [(rng.randrange(N), rng.randrange(N)) for _ in range(4)]
    pairs += [(rng.getrandbits(4096), rng.randrange(N)) for _ in range(2)]
    for a, x in pairs:
        got, qmax = msb_model.msb_mulmod(a, x, N, S, check=True)
        assert got == a * x % N
        assert qmax < 1 << 29


def test_noncanonical_x_breaks_the_invariant():
    """The precondition X < N is real: X = 2^4096 - 1 on the smallest admitted N = 2^4093 + 1 (X ~ 8N) leaves
    the model's invariant.  This is why CANON has to reduce every 4096-bit row completely before MULWC.
    The part that goes is the bound q < 2^29 (q reaches 31 bits); see test_noncanonical_x_margin."""
    N = (1 << 4093) + 1
    with pytest.raises(AssertionError):
        msb_model.msb_mulmod((1 << 4096) - 1, (1 << 4096) - 1, N, S, check=True)


def test_noncanonical_x_margin():
    """How far outside: for any 4096-bit X the estimate still follows the value and the product is exact, with
    q < 2^31 (the kernel multiplies by -q as a signed 32-bit factor, so 8N is the end of that margin, not its
    middle); with a large multiplier already X = 4N + 1 breaks q < 2^29; an all-ones S-limb X (2^4104 - 1, ~2048 N) clamps q and
    loses the value itself."""
    N = (1 << 4093) + 1
    top = (1 << 4096) - 1
    for a, x in ((top, top), (N - 1, top // N * N - 1), (top, 4 * N + 1)):
        got, qmax = msb_model.msb_mulmod(a, x, N, S, check=False)
        assert got == a * x % N and qmax < 1 << 31
        assert qmax >= 1 << 29 or a != top                       # a large multiplier limb is what shows it
    big = (1 << 27 * S) - 1
    got, qmax = msb_model.msb_mulmod(big, big, N, S, check=False)
    assert qmax == (1 << 32) - 1 and got != big * big % N


def test_main_samples_every_admitted_length():
    assert set(msb_model.N_BITS) == {4094, 4095, 4096}
