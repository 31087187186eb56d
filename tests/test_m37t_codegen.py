"""CPU checks of the generated fthe_padic_m37t (gen_padic_mfma.py top_est=True: product 2 of the reductions of SQR /
MUL without its fifth M-tile, limb 36 from product 1's fraction):

* the default generator output is still byte-identical to the committed gen/padic_m37.s; the four-tile body is a
  build product (gen/padic_m37t.s, not committed): generated twice it is the same text, it differs from the default
  only where it should, and a copy the build left behind equals it;
* the instruction counts of a squaring (.Lsqr_loop + .Lreduce), pinned: 116 MFMAs (136 - 2 x 10), 208 lane swaps
  (220 - 2 x 4 operand swaps of K-block 4 - 2 x 2 accumulator swaps of the fifth tile's exchange, which goes with
  the tile), 3,924 VALU instructions (3,947 before); LOADP keeps its 68 MFMAs;
* the register budget, the fraction register (written by the three capture instructions only, never part of an
  accumulator or operand range) and the operand dwords product 2 reads (0..31)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fedtree_amd", "csrc"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_padic_mfma as g  # noqa: E402
from test_m37_codegen import _sections  # noqa: E402

GEN = os.path.join(ROOT, "fedtree_amd", "csrc", "gen")
M37_VALU, M37_SWAPS, M37_MFMA = 3947, 220, 136


def _counts(asm):
    s = _sections(asm)
    body = s[".Lsqr_loop"] + s[".Lreduce"]
    return (sum(1 for i in body if i.startswith("v_") and "mfma" not in i),
            sum(1 for i in body if i.startswith("v_permlane32_swap")),
            sum(1 for i in body if "v_mfma" in i),
            sum(1 for i in s[".Lloadp"] if "v_mfma" in i))


def test_committed_kernels_are_the_generator_output():
    assert g.gen_padic_mfma("fthe_padic_m37") == open(os.path.join(GEN, "padic_m37.s")).read()
    assert g.gen_padic_mfma("fthe_padic_m37", top_est=False) == open(os.path.join(GEN, "padic_m37.s")).read()
    t = g.gen_body("m37t")
    assert t == g.gen_padic_mfma("fthe_padic_m37t", top_est=True)
    built = os.path.join(GEN, "padic_m37t.s")
    if os.path.exists(built):
        assert t == open(built).read()
    # outside the reduction's subroutine and the names, the two bodies are the same text but for the load of Pt
    base = g.gen_body("m37")
    head = lambda a: a.split(".Lreduce:")[0].replace("fthe_padic_m37t", "fthe_padic_m37").splitlines()
    extra = [x for x in head(t) if x not in set(head(base))]
    assert extra == [f"  s_load_dword s79, s[8:9], {hex(g.PT_OFF)}"], extra


def test_squaring_instruction_counts():
    base = _counts(g.gen_body("m37"))
    assert base == (M37_VALU, M37_SWAPS, M37_MFMA, 68)
    valu, swaps, mfma, loadp = _counts(g.gen_body("m37t"))
    assert mfma == 116
    assert swaps <= 212 and swaps == 208
    assert valu <= M37_VALU and valu == 3924
    assert loadp == 68                                       # LOADP keeps the five-tile product 2


def test_registers_and_the_fraction_register():
    asm = g.gen_body("m37t")
    nv = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", asm).group(1))
    ns = int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", asm).group(1))
    assert nv <= 256 and ns == 80
    body = asm.split(".rodata")[0]
    assert f"s_load_dword s79, s[8:9], {hex(g.PT_OFF)}" in body and g.PT_OFF == 400
    red = _sections(asm)[".Lreduce"]
    frac = 57
    writes = []
    for ins in red:
        if not ins.startswith(("v_", "ds_read")):
            continue
        dst = ins.split(None, 1)[1].split(",")[0].strip()
        m = re.match(r"v\[(\d+):(\d+)\]", dst)
        lo, hi = (int(m.group(1)), int(m.group(2))) if m else (int(dst[1:]), int(dst[1:]))
        if lo <= frac <= hi:
            writes.append(ins)
        if ins.startswith("v_permlane32_swap"):              # the swap writes both of its operands
            assert f"v{frac}" not in [x.strip() for x in ins.split(None, 1)[1].split(",")]
    assert [w.split()[0] for w in writes] == ["v_lshlrev_b32_e32", "v_mov_b32_e32", "v_alignbit_b32"], writes
    reads = [i for i in red if i.startswith("v_") and "alignbit" not in i
             and re.search(rf"\bv{frac}\b", i.split(None, 1)[1].split(",", 1)[1])]
    assert len(reads) == 2 and all(r.startswith("v_mad_u64_u32") and "s79" in r for r in reads), reads
    # every MFMA of the reductions reads its B operand from dwords 0..31 of an operand block in product 2: count the
    # product-2 tiles by their LDS offsets (tiles 10..18 of the image)
    p2_reads = [i for i in red if i.startswith("ds_read_b128") and int(i.rsplit("offset:", 1)[1]) >= 10 * 1024]
    assert len(p2_reads) == 2 * (1 + 2 + 3 + 4)
    assert not any(int(i.rsplit("offset:", 1)[1]) == 14 * 1024 for i in p2_reads)     # tile (m = 4, k = 0)
