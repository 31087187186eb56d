"""CPU checks of the generated fthe_padic_m37s (gen_padic_mfma.py top_est=True, q1_shift=8: the four-tile body with
product 1's operand fed two dwords later, so that its four sub-diagonal tiles are zero and are not formed;
DESIGN.md 14):

* with the parameter at its default the generator still gives the committed gen/padic_m37.s and the same
  fthe_padic_m37t, byte for byte; the new body is a build product (gen/padic_m37s.s, not committed);
* the instruction counts of a squaring (.Lsqr_loop + .Lreduce): 100 MFMAs (116 - 2 x 8), the same 208 lane swaps, no
  more VALU instructions than fthe_padic_m37t's 3,924 (3,914: the five zeroed pad dwords of each product 1 go, none
  is written in their place); LOADP 60 MFMAs (68 - 8); 251 VGPRs, 80 SGPRs;
* product 1 reads 15 A tiles per Barrett, tile slot 4 (the tile with the pad columns) once, within M-tile 0;
* the packing the generator emits for Barrett 1, run on one lane: q1's dwords land at XB + 2 .., the constant dword
  at XB + 36, and XB + 0, 1, 37, 38, 39 keep whatever they held;
* one wave of the kernel on the CPU emulator (tools/wave_emu.py) with those five registers holding random words,
  against Python integers."""
import os
import random
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fedtree_amd", "csrc"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_padic_mfma as g  # noqa: E402
from test_m37_codegen import PAT, M32, _run, _sections  # noqa: E402
from test_m37t_codegen import _counts  # noqa: E402

GEN = os.path.join(ROOT, "fedtree_amd", "csrc", "gen")
M37T_VALU = 3924


def _asm():
    return g.gen_body("m37s")


def test_defaults_reproduce_the_two_bodies():
    assert g.Q1_SHIFT == 8
    assert g.gen_padic_mfma("fthe_padic_m37", q1_shift=0) == open(os.path.join(GEN, "padic_m37.s")).read()
    assert g.gen_padic_mfma("fthe_padic_m37") == open(os.path.join(GEN, "padic_m37.s")).read()
    t = g.gen_body("m37t")
    assert t == g.gen_padic_mfma("fthe_padic_m37t", top_est=True, q1_shift=0)
    s = _asm()
    assert s == _asm() and s != t.replace("fthe_padic_m37t", "fthe_padic_m37s")
    for stem, text in (("padic_m37t", t), ("padic_m37s", s)):
        built = os.path.join(GEN, stem + ".s")
        if os.path.exists(built):                            # a copy the build left behind
            assert text == open(built).read(), stem
    # outside LOADP and the reduction's subroutine the new body is fthe_padic_m37t's text
    cut = lambda a: (a.split(".Lloadp:")[0] + a.split(".Lstorep:")[1].split(".Lreduce:")[0])
    assert cut(s) == cut(t).replace("fthe_padic_m37t", "fthe_padic_m37s")


def test_squaring_instruction_counts():
    assert _counts(g.gen_body("m37t")) == (M37T_VALU, 208, 116, 68)
    valu, swaps, mfma, loadp = _counts(_asm())
    assert mfma == 100
    assert swaps == 208
    assert valu <= M37T_VALU and valu == 3914
    assert loadp == 60


def test_registers():
    asm = _asm()
    nv = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", asm).group(1))
    ns = int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", asm).group(1))
    assert nv <= 256 and nv == 251
    assert ns == 80                                          # as fthe_padic_m37t (Pt in s79)
    body = asm.split(".rodata")[0]
    top = max(int(b or a) for a, b in re.findall(r"v(?:\[\d+:(\d+)\]|(\d+))", body) if (a or b))
    assert top < nv
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", asm).group(1)) == 20 * 1024


def test_product_1_reads_15_tiles():
    s = _sections(_asm())
    for sec, barretts in ((".Lreduce", 2), (".Lloadp", 1)):
        offs = [int(i.rsplit("offset:", 1)[1]) // 1024 for i in s[sec] if i.startswith("ds_read_b128")]
        p1 = [o for o in offs if o < 10]
        assert len(p1) == 15 * barretts, (sec, len(p1))
        assert all(o < 19 for o in offs)
        assert p1.count(4) == barretts                       # tile (0, 0): the pad columns, in the slot of m - k = 1
        # M-tile 0 = K-tiles 0..4: slot 4, Toeplitz -1, -2, -3 (slots 2, 1, 0), then the edge tile 5; M-tile m
        # then reads Toeplitz 0, -1, .. and its edge tile 5 + m (the first Barrett's first two reads may have been
        # issued by the caller, so only the multiset is pinned)
        assert sorted(p1[:5]) == [0, 1, 2, 4, 5], p1[:5]
        assert sorted(p1[:15]) == sorted([4, 2, 1, 0, 5, 3, 2, 1, 6, 3, 2, 7, 3, 8, 9])
    # fthe_padic_m37t reads 19
    t = _sections(g.gen_body("m37t"))[".Lloadp"]
    assert len([i for i in t if i.startswith("ds_read_b128") and int(i.rsplit("offset:", 1)[1]) < 10 * 1024]) == 19


def test_packing_puts_q1_two_dwords_later():
    s = _sections(_asm())[".Lreduce"]
    pack = []
    for ins in s:
        if ins.startswith("v_permlane32_swap") or ins.startswith("s_nop"):
            break
        if ins.startswith("v_"):
            pack.append(ins)
    assert pack and not any("bitop3" in x for x in pack)
    K, TT, XB = 37, 100, 60
    written = set()
    for ins in pack:
        written.add(int(ins.split(None, 1)[1].split(",")[0].strip()[1:]))
    assert written == set(range(XB + 2, XB + 37)), sorted(written)    # never XB + 0, 1, 37, 38, 39
    rng = random.Random(8)
    for trial in range(200):
        limbs = [rng.getrandbits(28) for _ in range(2 * K)]
        limbs[K - 1] = rng.getrandbits(29)                 # T[36] may carry a bit 28 (u1 added)
        limbs[2 * K - 1] = rng.getrandbits(22)
        if trial == 0:
            limbs = [(1 << 28) - 1] * (2 * K)
            limbs[2 * K - 1] = (1 << 22) - 1
        regs = [0] * 256
        junk = {XB + w: rng.getrandbits(32) for w in (0, 1, 37, 38, 39)}
        for r, v in junk.items():
            regs[r] = v
        for i, x in enumerate(limbs):                      # T[37..73] as the product tails leave them
            regs[TT + i] = x ^ PAT[(i - (K - 1)) % 2] if i >= K else x
        _run(pack, regs, {35: (1 << 28) - 1})
        q1 = sum((limbs[K - 1 + t] & ((1 << 28) - 1 if t == 0 else M32)) << (28 * t) for t in range(K + 1))
        for w in range(34):
            want = ((q1 >> (32 * w)) & M32) ^ 0x80808080
            assert regs[XB + 2 + w] == want, (trial, w, hex(regs[XB + 2 + w]), hex(want))
        assert regs[XB + 36] == (((limbs[K - 1] >> 28) & 1) << 12 | 1)   # digit 1 at K index 144, 16 c at 145
        assert all(regs[r] == v for r, v in junk.items())


@pytest.mark.parametrize("bits", [1009, 1027])
def test_wave_emulation_of_the_kernel(bits):
    """one wave of the generated fthe_padic_m37s on the CPU: LOADP, STOREX, SQR, MUL, STOREP = x^3 mod P^2 on 64
    lanes, P at the ends of the body's range, the operand's pad registers holding random words from the start"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import wave_emu
    assert wave_emu.m37_selftest(seed=bits, bits=bits, variant="m37s", junk_pads=True) == 0
