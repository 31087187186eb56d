"""CPU checks of gen_addb.py and gen_nadicb.py on the shared Barrett emission (barrett_mfma.py), and of their
switches as an argument:

* the default text is the committed gen/addb_q152.s and gen/nadic_b76.s, byte for byte;
* an unknown token -- a misspelling, a substring of a known one, a switch of a removed experiment -- raises and the
  message names the known tokens; the string and set forms agree and token order does not matter;
* every switch generates, changes the text (but for the two that only act under mfz) and assembles (the assembler
  line of fedtree_amd/build.py); calls do not affect each other;
* FTHE_GEN_ADDB_DBG, FTHE_GEN_NADICB_DBG and FTHE_GEN_NADICB_WAVES in the environment reach neither generator, at
  import or in a call: only fedtree_amd/build.py reads them; the wave count is an argument down to the layout header;
* gen_montprog._descriptor's default kernarg table is the op-program kernels' 168 bytes, gen_addb's its 56."""
import importlib.util
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fedtree_amd", "csrc")
sys.path.insert(0, ROOT)
sys.path.insert(0, CSRC)
import barrett_mfma as bm  # noqa: E402
import gen_addb as ga  # noqa: E402
import gen_nadicb as gb  # noqa: E402
from fedtree_amd import build  # noqa: E402
from gen_montprog import _descriptor  # noqa: E402

GENS = {"addb": (ga, lambda dbg="": ga.gen_addb("fthe_addb_q152", dbg), "addb_q152.s"),
        "nadicb": (gb, lambda dbg="": gb.gen_nadicb("fthe_nadic_b76", dbg=dbg), "nadic_b76.s")}
REMOVED = {"addb": ["acc2", "norm1", "pf0", "pf8", "prio", "prioinv"],
           "nadicb": ["acc2", "chunkloop", "desync1", "desync2", "prio", "prioinv"]}
SAME = {"addb": {"mznorm", "mzmfma"}, "nadicb": set()}          # no-ops without mfz


@pytest.fixture(scope="module")
def default():
    return {k: gen() for k, (_, gen, _) in GENS.items()}


@pytest.mark.parametrize("which", list(GENS))
def test_default_is_the_committed_kernel(which, default):
    assert default[which] == open(os.path.join(CSRC, "gen", GENS[which][2])).read()


@pytest.mark.parametrize("which", list(GENS))
def test_unknown_token_raises_and_names_the_known_ones(which):
    mod, gen, _ = GENS[which]
    for dbg in REMOVED[which] + ["nokarra", "kara", "mf", "noq", "nomfma,stam", "Stamp", {"nonorm", "x"}]:
        with pytest.raises(ValueError) as ei:
            gen(dbg)
        last = dbg.split(",")[-1] if isinstance(dbg, str) else "x"
        assert all(t in str(ei.value) for t in mod.SWITCHES) and last in str(ei.value), dbg


@pytest.mark.parametrize("which", list(GENS))
def test_tokens_are_exact_string_and_set_agree(which, default):
    mod, gen, _ = GENS[which]
    assert mod.parse_dbg("") == mod.parse_dbg(",") == mod.parse_dbg(()) == frozenset()
    assert mod.parse_dbg("nomfma, stamp") == mod.parse_dbg({"stamp", "nomfma"}) == {"nomfma", "stamp"}
    a = gen("nomfma,stamp")
    assert a == gen("stamp,nomfma") == gen({"stamp", "nomfma"}) == gen(frozenset(("nomfma", "stamp")))
    assert a != gen("nomfma") != gen("stamp") != a
    assert gen("") == gen(set()) == default[which]           # and calls do not affect each other


def test_noq3_is_an_ordinary_token(default):
    a = GENS["nadicb"][1]("noq3,nonorm")
    assert ".Ldbg_skip_q3:" in a and ".Ldbg_skip_q3:" in GENS["nadicb"][1]("noq3") and \
        ".Ldbg_skip_q3" not in default["nadicb"] and a != GENS["nadicb"][1]("nonorm")


@pytest.mark.parametrize("which", list(GENS))
def test_every_switch_generates_and_assembles(which, default, tmp_path):
    mod, gen, _ = GENS[which]
    for sw in mod.SWITCHES + (("mfz,mznorm", "mfz,mzmfma", "nokara,stamp") if which == "addb" else ()):
        asm = gen(sw)
        assert (asm == default[which]) == (sw in SAME[which]), sw
        src = tmp_path / f"{which}_{sw}.s"
        src.write_text(asm)
        r = subprocess.run([f"{build.LLVM}/clang", "-x", "assembler", "-target", "amdgcn-amd-amdhsa",
                            f"-mcpu={build.ARCH}", "-c", str(src), "-o", str(tmp_path / "out.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, (sw, r.stderr[-2000:])


def test_wave_count_is_an_argument(default):
    assert gb.WAVES == 12 and gb.gen_nadicb("fthe_nadic_b76", 12) == default["nadicb"]
    for waves in (1, 4):
        asm = gb.gen_nadicb("fthe_nadic_b76", waves)
        assert f".amdhsa_group_segment_fixed_size {gb.lds_bytes(waves)}\n" in asm
        assert f".max_flat_workgroup_size: {64 * waves}\n" in asm
        hdr = gb.layout_header(waves)
        assert f"kNbWaves = {waves};" in hdr and f"kNbPerWg = {16 * waves};" in hdr and \
            f"kNbLdsBytes = {gb.lds_bytes(waves)};" in hdr
    assert gb.layout_header() == gb.layout_header(12) and gb.lds_bytes() == gb.lds_bytes(12)


def test_the_environment_does_not_reach_the_generators(default, monkeypatch):
    monkeypatch.setenv("FTHE_GEN_ADDB_DBG", "nokara,stamp")
    monkeypatch.setenv("FTHE_GEN_NADICB_DBG", "noq3")
    monkeypatch.setenv("FTHE_GEN_NADICB_WAVES", "4")
    fresh = {}
    for name in ("barrett_mfma", "gen_addb", "gen_nadicb"):
        spec = importlib.util.spec_from_file_location(name + "_fresh", os.path.join(CSRC, name + ".py"))
        fresh[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(fresh[name])
        src = open(os.path.join(CSRC, name + ".py")).read()
        assert "environ" not in src and "getenv" not in src, name
    assert fresh["gen_addb"].gen_addb("fthe_addb_q152") == default["addb"] == GENS["addb"][1]()
    assert fresh["gen_nadicb"].gen_nadicb("fthe_nadic_b76") == default["nadicb"] == GENS["nadicb"][1]()
    assert fresh["gen_nadicb"].WAVES == 12 and fresh["gen_nadicb"].layout_header() == gb.layout_header(12)


def test_descriptor_kernarg_tables(default):
    d = _descriptor("k", 0, 8, 8)
    assert ".amdhsa_kernarg_size 168\n" in d and ".kernarg_segment_size: 168\n" in d and d.count(".offset:") == 23
    assert ".amdhsa_kernarg_size 56\n" in default["addb"] and ".kernarg_segment_size: 56\n" in default["addb"]
    assert default["addb"].count(".offset:") == len(ga.KARGS) == 8
    assert ".amdhsa_kernarg_size 168\n" in default["nadicb"]


def test_tile_geometry_is_shared():
    assert ga.copy_slot is gb.copy_slot is bm.copy_slot and sorted(map(bm.copy_slot, range(16))) == list(range(16))
    assert ga.ACT1 == bm.active(ga.ND1, ga.S1_BASE, ga.TILES1, ga.KB1) and sum(map(len, ga.ACT1 + ga.ACT2)) == 185 + 153
    assert sum(map(len, gb.ACT1)) == 61 and sum(map(len, gb.ACT2)) == 45
