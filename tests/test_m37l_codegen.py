"""CPU checks of the generated fthe_padic_m37l (gen_padic_mfma.py top_est=True, limb_op=True: the four-tile body whose
product 1 reads its B operands straight from the limbs T[36..73] / V[36..73], no repack and no copy):

* with the parameter at its default the generator still gives the committed gen/padic_m37.s and the same
  fthe_padic_m37t and fthe_padic_m37s, byte for byte; the new body is a build product (gen/padic_m37l.s);
* the instruction counts of a squaring (.Lsqr_loop + .Lreduce): 100 MFMAs as fthe_padic_m37s, the same 208 lane swaps
  (the pads ride in swaps product 1 already had), 3,785 VALU instructions in the text (3,914 - 130 + the clamp
  branch's compare), of which the 37 of the clamp are skipped unless a lane's numerator went negative: 3,748 run;
  LOADP 60 MFMAs; 255 VGPRs, 80 SGPRs, 24 KB of LDS;
* the clamp of Barrett 1 sits behind a wave-uniform branch on the chunk carry, the mask is formed before it, and the
  noclampbr switch gives the straight-line text back;
* product 1 reads 15 tiles of its own per Barrett (slots 0..14) from operand blocks of 40 consecutive registers that
  start even (v136.., v212..), whose first and last registers nothing else reads or writes;
* nothing between the reduction's entry and product 1's first lane swap packs anything: a copy and a flip of limb 36;
* one wave of the kernel on the CPU emulator (tools/wave_emu.py) -- LOADP, SQR, MUL on random and extreme digits, the
  pad registers holding random words, and lanes whose q1 is 0, 1, 2, 15, 16, 17 at P = 2^1027 - 2^600 + 1 (numerators
  around zero: the clamp's two sides) beside ordinary lanes in one wave -- against Python integers."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fedtree_amd", "csrc"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_padic_mfma as g  # noqa: E402
from test_m37_codegen import _sections as _sections_by_label  # noqa: E402
from test_m37t_codegen import _counts as _counts_by_label  # noqa: E402

GEN = os.path.join(ROOT, "fedtree_amd", "csrc", "gen")
M37S_VALU = 3914
P_WIDE = (1 << 1027) - (1 << 600) + 1


def _asm():
    return g.gen_body("m37l")


def _flat(asm):
    """the text without the clamp branch's landing labels, so that an op's section holds all of its instructions"""
    return re.sub(r"(?m)^\.Lnoclamp\d+:\n", "", asm)


def _sections(asm):
    return _sections_by_label(_flat(asm))


def _counts(asm):
    return _counts_by_label(_flat(asm))


def test_defaults_reproduce_the_three_bodies():
    assert g.gen_padic_mfma("fthe_padic_m37", limb_op=False) == open(os.path.join(GEN, "padic_m37.s")).read()
    t = g.gen_body("m37t")
    s = g.gen_body("m37s")
    assert t == g.gen_padic_mfma("fthe_padic_m37t", top_est=True, limb_op=False)
    assert s == g.gen_padic_mfma("fthe_padic_m37s", top_est=True, q1_shift=8, limb_op=False)
    a = _asm()
    assert a == _asm() and a != s.replace("fthe_padic_m37s", "fthe_padic_m37l")
    for stem, text in (("padic_m37t", t), ("padic_m37s", s), ("padic_m37l", a)):
        built = os.path.join(GEN, stem + ".s")
        if os.path.exists(built):                            # a copy the build left behind
            assert text == open(built).read(), stem
    with pytest.raises(AssertionError):
        g.gen_padic_mfma("x", limb_op=True)                  # only on the four-tile body
    with pytest.raises(AssertionError):
        g.gen_padic_mfma("x", top_est=True, q1_shift=8, limb_op=True)


def test_squaring_instruction_counts():
    assert _counts(g.gen_body("m37s")) == (M37S_VALU, 208, 100, 60)
    valu, swaps, mfma, loadp = _counts(_asm())
    assert mfma == 100
    assert swaps == 208                                      # the pads need no swap of their own
    assert valu <= M37S_VALU - 120 and valu == 3785          # 3,914 - 130 + v_cmp; 37 of them behind the branch
    assert loadp == 60
    red = lambda a: sum(1 for i in _sections(a)[".Lreduce"] if i.startswith("v_"))
    assert red(g.gen_body("m37s")) - red(_asm()) == 129


def test_the_clamp_sits_behind_a_wave_uniform_branch():
    asm = _asm()
    assert asm.count("s_cbranch_vccz .Lnoclamp") == 2 and ".Lnoclamp1:" in asm and ".Lnoclamp2:" in asm   # LOADP, reduce
    red = _sections_by_label(asm)[".Lreduce"]                # up to the landing label
    i = red.index("s_cbranch_vccz .Lnoclamp2")
    assert red[i - 3:i] == ["v_not_b32_e32 v56, v58", "v_cmp_ne_u32_e32 vcc, 0, v58", "s_nop 4"]
    skipped = red[i + 1:]
    assert len(skipped) == 37 and all(x.startswith("v_bitop3_b32") and x.endswith("v56, v253 bitop3:0xe2") or
                                      x.endswith("v56, v254 bitop3:0xe2") for x in skipped)
    assert [int(x.split()[1].strip(",")[1:]) for x in skipped] == list(range(62, 99))      # q3's limbs in D[2..38]
    after = _sections_by_label(asm)[".Lnoclamp2"]
    assert after[0].startswith("v_xad_u32")                  # V += u1 follows on both paths
    assert any("v_and_b32_e32" in x and "v56" in x for x in after)     # the four-tile body's h reads the mask
    plain = g.gen_body("m37l", "noclampbr")
    assert "Lnoclamp" not in plain and _counts_by_label(plain)[0] == 3784
    assert [x for x in _flat(asm).splitlines() if x not in set(plain.splitlines())] == \
        ["  v_cmp_ne_u32_e32 vcc, 0, v58", "  s_cbranch_vccz .Lnoclamp1",
         "  v_cmp_ne_u32_e32 vcc, 0, v58", "  s_cbranch_vccz .Lnoclamp2"]


def test_registers():
    asm = _asm()
    nv = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", asm).group(1))
    ns = int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", asm).group(1))
    assert nv <= 256 and nv == 255
    assert ns == 80
    body = asm.split(".rodata")[0]
    top = max(int(b or a) for a, b in re.findall(r"v(?:\[\d+:(\d+)\]|(\d+))", body) if (a or b))
    assert top < nv
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", asm).group(1))
    assert lds == g.TILE_BYTES_L == 24 * 1024 and 2 * lds <= 160 * 1024        # two workgroups per CU
    assert body.count("ds_write_b128") == lds // 4096                         # the image fill


def _regs(ins):
    out = set()
    for a, b, c in re.findall(r"\bv(?:\[(\d+):(\d+)\]|(\d+))", ins):
        out |= set(range(int(a), int(b) + 1)) if a else {int(c)}
    return out


def test_product_1_reads_15_tiles_from_the_limbs():
    s = _sections(_asm())
    PADS = {136, 175, 212, 251}
    for sec, barretts in ((".Lreduce", 2), (".Lloadp", 1)):
        offs = [int(i.rsplit("offset:", 1)[1]) // 1024 for i in s[sec] if i.startswith("ds_read_b128")]
        p1 = [o for o in offs if o < 15]
        assert len(p1) == 15 * barretts and sorted(p1) == sorted(list(range(15)) * barretts), (sec, p1)
        assert all(o < 24 for o in offs)
        # an MFMA's B operand: four registers from an even one, inside T's block, V's block or XB
        blocks = {136: 0, 212: 0, 60: 0}
        for ins in (i for i in s[sec] if "v_mfma" in i):
            b = re.findall(r"v\[(\d+):(\d+)\]", ins)[2]
            lo, hi = int(b[0]), int(b[1])
            assert hi == lo + 3 and lo % 2 == 0
            base = next(x for x in blocks if x <= lo < x + 40)
            assert (lo - base) % 4 == 0
            blocks[base] += 1
        assert blocks == ({136: 30, 212: 30, 60: 40} if sec == ".Lreduce" else {136: 30, 212: 0, 60: 30}), blocks
    # the pad registers: touched by lane swaps alone (and read, against zero A columns, by the MFMAs of their blocks)
    for sec in s:
        for ins in s[sec]:
            if _regs(ins) & PADS and not ins.startswith(("v_permlane32_swap", "v_mfma")):
                assert False, (sec, ins)


def test_nothing_is_packed_before_product_1():
    s = _sections(_asm())[".Lreduce"]
    head = []
    for ins in s:
        if ins.startswith("v_permlane32_swap"):
            break
        if ins.startswith("v_"):
            head.append(ins)
    assert head == ["v_mov_b32_e32 v14, v137", "v_xor_b32_e32 v137, v253, v137"], head
    # the top limb's tail carries the constant digit 1 in its byte 3; the others use the one pattern register
    sq = _sections(_asm())[".Lsqr_loop"]
    assert sum(1 for i in sq if "0x1808080" in i) == 2                          # T[73] and V[73]
    assert not any(re.search(r"\bv254\b", i) for i in sq)                       # no pat(odd) in the product phase
    m37s = g.gen_body("m37s")
    assert any(re.search(r"\bv250\b", i) for i in _sections(m37s)[".Lsqr_loop"])


@pytest.mark.parametrize("bits", [1009, 1027])
def test_wave_emulation_of_the_kernel(bits):
    """LOADP, STOREX, SQR, MUL, STOREP = x^3 mod P^2 on 64 lanes, P at the ends of the body's range, the four pad
    registers holding random words from the start"""
    import wave_emu
    assert wave_emu.m37_selftest(seed=bits, bits=bits, variant="m37l", junk_pads=True) == 0


def test_wave_emulation_extreme_digits():
    """two squarings of crafted digit pairs (all-ones low limbs, zero halves, the largest digit 3P - 1) at the widest
    modulus, against Python integers"""
    import wave_emu
    assert wave_emu.m37_digits_selftest(seed=3, variant="m37l", P=(1 << 1027) - 1) == 0


def test_wave_emulation_small_quotients_beside_ordinary_lanes():
    """q1 = 0, 1, 2, 15, 16, 17 at P = 2^1027 - 2^600 + 1, in LOADP (x = q1 2^1008 + low) and in the first reduction
    of a squaring (x0^2 >> 1008 = q1), beside random lanes of the same wave: the clamp taken and not taken"""
    import math
    import wave_emu
    qs = (0, 1, 2, 15, 16, 17)
    xs = [(v << 1008) + 12345 + v for v in qs]
    assert wave_emu.m37_selftest(seed=11, variant="m37l", P=P_WIDE, extra=xs, junk_pads=True) == 0
    pairs = []
    for v in qs:
        x0 = math.isqrt(v << 1008) + (1 if v else 0)
        assert (x0 * x0) >> 1008 == v
        pairs += [(x0, 0), (x0, P_WIDE - 1)]
    assert wave_emu.m37_digits_selftest(seed=12, variant="m37l", P=P_WIDE, pairs0=pairs) == 0


def test_wave_emulation_no_clamped_lane_skips_the_clamp(capsys):
    """64 ordinary lanes: the branch is taken in both squarings (74 instructions fewer than a wave with a clamped
    lane), same results"""
    import wave_emu
    rng = __import__("random").Random(5)
    P = rng.getrandbits(1024) | (1 << 1023) | 1
    ordinary = [(rng.randrange(P >> 1, P), rng.randrange(P)) for _ in range(64)]
    steps = []
    for pairs in (ordinary, [(1, 0)] + ordinary[1:]):
        assert wave_emu.m37_digits_selftest(seed=5, variant="m37l", P=P, pairs0=pairs) == 0
        steps.append(int(re.search(r"(\d+) wave-instructions", capsys.readouterr().out).group(1)))
    assert steps[1] - steps[0] == 2 * 37, steps
