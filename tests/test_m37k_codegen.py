"""CPU checks of the generated fthe_padic_m37k (gen_padic_mfma.py K_BODIES: fthe_padic_m37l with MUL's cross term
x0 y1 + x1 y0 by one level of Karatsuba, kara_cross_mul, and -- generator parameter fill0, off in the body's table
because it measured no clear gain, on under the switch fill0 -- tile 0 of every reduction's first quotient product
issued by the caller with its own independent work between the MFMAs):

* the four older bodies are byte for byte what they were before the fifth was added (digests of their texts, the
  committed gen/padic_m37.s among them), and m37k with both of its cuts switched off is m37l's text under its own name;
* counts, taken from m37l's text in the same run: MUL issues 646 fewer v_mad_u64_u32 and at least 250 fewer VALU
  instructions, a squaring or product still runs 100 MFMAs and 208 lane swaps, 256 VGPRs;
* with fill0 no s_nop 7 stands between tile 0's last MFMA and its lane exchange but at least MARGIN VALU instructions,
  none of which touches tile 0's accumulators, operand block or A-tile buffers, and at most about five sit between two
  MFMAs; both callers enter one shared text at .Lreduce;
* the bounds of the Karatsuba cross term (tools/padic_mfma_model.py kara_cross_mul) on every crafted case;
* one wave on the CPU emulator (tools/wave_emu.py) against Python integers for P of 1009 and 1027 bits and the wide
  P = 2^1027 - 2^600 + 1: LOADP, SQR and MUL on random values, runs of squarings on crafted digits, and single products
  on the crafted operands of tools/barrett_cases.py padic_kara_mul_pairs beside ordinary lanes in the same wave."""
import hashlib
import os
import random
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fedtree_amd", "csrc"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_padic_mfma as g  # noqa: E402
from test_m37_codegen import _sections as _sections_by_label  # noqa: E402

GEN = os.path.join(ROOT, "fedtree_amd", "csrc", "gen")
P_WIDE = (1 << 1027) - (1 << 600) + 1
P_NARROW = (1 << 1008) + (1 << 500) + 1          # 1009 bits, just above 2^1008: the largest mu
MARGIN = 30                                      # gen_padic_mfma.py: VALU instructions between an MFMA and its exchange
# sha256 of the four bodies' texts before fthe_padic_m37k existed
PARENT = {"m37": "628e1c7f09bb9d10143063ccc2ae2bd5358d1cb050ad57ea556b888b5912b3a4",
          "m37t": "347aa2d93607dae2f123831c41f5e8b4006e1658dc8e5e8a7a396d8283a0a025",
          "m37s": "0f6541003e4d61e88ef50fd457ef3afc245f6d9f1bf8f38599e9b2cd9873a28b",
          "m37l": "3ef69e797ad30bb11e28ca8e0cc4b95a81cedd80ab864e31e1a1e013bcdec78b"}


def _sections(asm):
    return _sections_by_label(re.sub(r"(?m)^\.Lnoclamp\d+:\n", "", asm))


def _valu(ins):
    return sum(1 for i in ins if i.startswith("v_") and "mfma" not in i)


def _mads(ins):
    return sum(1 for i in ins if i.startswith("v_mad_u64_u32"))


def test_older_bodies_are_untouched_and_the_cuts_switch_off():
    for variant, digest in PARENT.items():
        assert hashlib.sha256(g.gen_body(variant).encode()).hexdigest() == digest, variant
    assert hashlib.sha256(open(os.path.join(GEN, "padic_m37.s"), "rb").read()).hexdigest() == PARENT["m37"]
    plain = g.gen_body("m37k", "nomulkara,nofill0")
    assert plain.replace("fthe_padic_m37k", "fthe_padic_m37l") == g.gen_body("m37l")
    k = g.gen_body("m37k")
    assert k == g.gen_padic_mfma("fthe_padic_m37k", **{a: v for a, v in g.K_BODIES["m37k"].items() if a != "clampbr"})
    built = os.path.join(GEN, "padic_m37k.s")
    if os.path.exists(built):                                # a copy the build left behind
        assert k == open(built).read()
    assert k == g.gen_body("m37k", "nofill0") != g.gen_body("m37k", "fill0")     # the table's default, spelt out
    for sw in g.K_SWITCHES:                                  # the other bodies do not know m37k's switches
        with pytest.raises(ValueError, match="unknown"):
            g.gen_body("m37l", sw)
    with pytest.raises(ValueError, match="contradict"):
        g.gen_body("m37k", "fill0,nofill0")
    with pytest.raises(AssertionError):
        g.gen_padic_mfma("x", top_est=True, q1_shift=8, mul_kara=True)


def test_mul_counts_against_m37l():
    l, k = _sections(g.gen_body("m37l")), _sections(g.gen_body("m37k"))
    assert _mads(l[".Lmul"]) - _mads(k[".Lmul"]) == 646
    assert _valu(l[".Lmul"]) - _valu(k[".Lmul"]) >= 250
    assert l[".Lsqr_loop"] == k[".Lsqr_loop"] and l[".Lreduce"] == k[".Lreduce"]
    # with tile 0 in the callers: per op, the caller's section and the shared text together
    f, both = _sections(g.gen_body("m37k", "nomulkara,fill0")), _sections(g.gen_body("m37k", "fill0"))
    for op in (".Lsqr_loop", ".Lmul"):
        for text in (l, k, f, both):
            ins = text[op] + text[".Lreduce"]
            assert sum(1 for i in ins if "v_mfma" in i) == 100, op
            assert sum(1 for i in ins if i.startswith("v_permlane32_swap")) == 208, op
    valu = lambda s, op: _valu(s[op] + s[".Lreduce"])        # noqa: E731
    assert valu(l, ".Lmul") - valu(both, ".Lmul") >= 250
    assert valu(both, ".Lsqr_loop") == valu(l, ".Lsqr_loop")  # fill0 moves instructions, it removes none


def test_registers():
    for ab in ("", "fill0", "nomulkara", "nomulkara,fill0"):
        asm = g.gen_body("m37k", ab)
        nv = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", asm).group(1))
        assert nv == (255 if "nomulkara" in ab else 256) and nv <= 256
        body = asm.split(".rodata")[0]
        top = max(int(b or a) for a, b in re.findall(r"v(?:\[\d+:(\d+)\]|(\d+))", body) if (a or b))
        assert top < nv
        assert "scratch" not in body and int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", asm).group(1)) == \
            g.TILE_BYTES_L                                   # nothing moved to LDS or scratch


def _regs(ins):
    out = set()
    for a, b, c in re.findall(r"\bv(?:\[(\d+):(\d+)\]|(\d+))", ins):
        out |= set(range(int(a), int(b) + 1)) if a else {int(c)}
    return out


def test_tile_0_is_filled_by_its_caller():
    asm = g.gen_body("m37k", "fill0")
    s = _sections(asm)
    assert asm.count(".Lreduce:") == 1
    red = s[".Lreduce"]
    first = next(i for i, x in enumerate(red) if "v_mfma" in x)
    assert not any(x == "s_nop 7" for x in red[:first])      # the shared text opens with the exchange, no wait
    assert red[0].startswith("v_lshl_add_u32 v20") and sum(1 for x in red if "v_mfma" in x) == 90
    banned = set(range(2, 15)) | set(range(20, 52)) | set(range(136, 176))     # A tiles, limb 36's copy, G0 / G1, T's block
    for op, nfill in ((".Lsqr_loop", 50), (".Lmul", 50 + 18)):       # the ripple behind its first instruction; the copy
        sec = s[op]
        mf = [i for i, x in enumerate(sec) if "v_mfma" in x]
        assert len(mf) == 10 and all("v[20:35]" in sec[i] or "v[36:51]" in sec[i] for i in mf)
        tail = sec[mf[-1] + 1:]
        assert "s_nop 7" not in tail
        assert _valu(tail) >= MARGIN
        fill = [x for x in sec[mf[0] + 1:] if x.startswith("v_") and "mfma" not in x]
        assert len(fill) == nfill
        for x in fill:
            assert not _regs(x) & banned, (op, x)
        for a, b in zip(mf, mf[1:]):
            assert _valu(sec[a + 1:b]) <= 5, (op, a)
        # before the first MFMA: the head alone (limb 36's copy and flip), then the operand's lane swaps
        head = sec[:mf[0]]
        sw = next(i for i, x in enumerate(head) if x.startswith("v_permlane32_swap"))
        assert [x for x in head[sw - 4:sw] if x.startswith("v_")] == ["v_mov_b32_e32 v14, v137",
                                                                       "v_xor_b32_e32 v137, v253, v137"]
    # switched off: the callers call a reduction that issues tile 0 itself and waits
    off = _sections(g.gen_body("m37k"))
    assert not any("v_mfma" in x for x in off[".Lsqr_loop"] + off[".Lmul"])
    r = off[".Lreduce"]
    m10 = [i for i, x in enumerate(r) if "v_mfma" in x][9]
    assert r[m10 + 1:m10 + 6].count("s_nop 7") == 3


def _kara_cases(P):
    import barrett_cases as bc
    return bc.padic_kara_mul_pairs(P, "m37k")


@pytest.mark.parametrize("P", [P_WIDE, (1 << 1008) + (1 << 500) + 1, (1 << 1027) - 1], ids=["wide", "1009", "2^1027-1"])
def test_model_bounds_on_every_crafted_product(P):
    import barrett_cases as bc
    import padic_mfma_model as mm
    rng = random.Random(P % 1000003)
    ops = list(_kara_cases(P)) + [(bc.filler(rng, 3 * P), bc.filler(rng, 3 * P)) for _ in range(20)]
    assert len(_kara_cases(P)) == 15 + 43
    for a, b in ops:
        W = mm.kara_cross_mul(*(bc.plimbs(d) for d in (a[0], a[1], b[0], b[1])))
        assert sum(v << (28 * i) for i, v in enumerate(W)) == a[0] * b[1] + a[1] * b[0] < 1 << mm.LIMB_T_BITS
    with pytest.raises(AssertionError):                      # a digit far beyond the contract trips a bound
        mm.kara_cross_mul(*([bc.PMASK] * 37 for _ in range(4)))


@pytest.mark.parametrize("bits", [1009, 1027])
def test_wave_emulation_of_the_kernel(bits):
    """LOADP, STOREX, SQR, MUL, STOREP = x^3 mod P^2 on 64 lanes, the pad registers holding random words"""
    import wave_emu
    assert wave_emu.m37_selftest(seed=bits, bits=bits, variant="m37k", junk_pads=True) == 0
    assert wave_emu.m37_selftest(seed=bits, bits=bits, variant="m37k", ab="fill0", junk_pads=True) == 0


def test_wave_emulation_of_the_kernel_wide_prime():
    import wave_emu
    assert wave_emu.m37_selftest(seed=7, variant="m37k", P=P_WIDE, junk_pads=True) == 0


@pytest.mark.parametrize("P", [P_WIDE, None], ids=["wide", "1009"])
def test_wave_emulation_runs_of_squarings_on_crafted_digits(P):
    """the existing squaring pairs, also with tile 0 filled (it then carries the ripple of kara_cross)"""
    import barrett_cases as bc
    import wave_emu
    if P is None:
        P = random.Random(9).getrandbits(1009) | (1 << 1008) | 1
    assert wave_emu.m37_digits_selftest(seed=3, variant="m37k", P=P) == 0
    assert wave_emu.m37_digits_selftest(seed=4, variant="m37k", ab="fill0", P=P,
                                        pairs0=bc.padic_edge_pairs(P, "m37k")) == 0


@pytest.mark.parametrize("bits", [1009, 1027, 0], ids=["1009", "1027", "wide"])
@pytest.mark.parametrize("ab", ["", "fill0"])
def test_wave_emulation_products_on_crafted_operands(bits, ab):
    """LOADX a; MUL b; STOREX on the 58 crafted operand pairs and six random ones in one wave: digits within the
    four-tile bodies' promise (limbs below 2^28, digits below P + 2^1015) and the residue exact, the model's bounds on
    each cross term"""
    import wave_emu
    P = P_WIDE if not bits else P_NARROW if bits == 1009 else random.Random(bits).getrandbits(bits) | (1 << (bits - 1)) | 1
    assert wave_emu.m37_mul_selftest(seed=bits, variant="m37k", P=P, ab=ab) == 0
