"""CPU checks of the A/B switches of gen_padic_mfma.py as an argument (ab) and of its table of bodies:

* an unknown token -- a misspelling, a substring of a known one, a switch of a removed experiment -- raises and the
  message names the known tokens; two tokens that contradict each other raise;
* each combination of a switch and a body that the generator cannot honour raises with its reason;
* every switch generates and assembles (the assembler line of fedtree_amd/build.py) for every body that accepts it;
* calls do not affect each other: the default text after a call under s1lo112 is the default text before it;
* gen_body(variant) is the kernel fedtree_amd/build.py writes to gen/padic_<variant>.s, and the module reads no
  environment variable."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fedtree_amd", "csrc"))
import gen_padic_mfma as g  # noqa: E402
from fedtree_amd import build  # noqa: E402

GEN = os.path.join(ROOT, "fedtree_amd", "csrc", "gen")
# switch -> the bodies that refuse it, with a word of the reason
REFUSED = {"s1lo112": {"m37s": "shifted", "m37l": "limb-fed"},
           "noprexor": {"m37l": "as they lie"},
           "noq3dw": {"m37l": "V[36..73]"}}
ALL = g.SWITCHES + g.PRIOS


@pytest.fixture(scope="module")
def default():
    return {v: g.gen_body(v) for v in g.BODIES}


@pytest.mark.parametrize("ab", ["nokarra", "kara", "clamp", "nokara,spil", "prio", "prio4", "prio11", "noprio3",
                                "spill", "pingpong", "ppodd", "ldsx", "ldsxa", "col3", "col4", "margin40", "dyn"])
def test_unknown_token_raises_and_names_the_known_ones(ab):
    with pytest.raises(ValueError) as ei:
        g.gen_body("m37", ab)
    assert all(t in str(ei.value) for t in ALL) and ab.split(",")[-1] in str(ei.value)
    with pytest.raises(ValueError):
        g.s1_lo(ab)


@pytest.mark.parametrize("ab", ["clampbr,noclampbr", "noprio,prio2", "prio1,prio2"])
def test_contradicting_tokens_raise(ab):
    with pytest.raises(ValueError, match="contradict"):
        g.gen_body("m37l", ab)


def test_tokens_are_exact_and_a_set_is_taken_as_it_is():
    assert g.parse_ab("") == g.parse_ab(",") == frozenset()
    assert g.parse_ab("nokara, noprio") == g.parse_ab({"noprio", "nokara"}) == {"nokara", "noprio"}
    assert g.gen_body("m37", {"noprio", "nokara"}) == g.gen_body("m37", "nokara,noprio")
    assert g.s1_lo() == g.s1_lo("noq3dw") == g.S1_LO == 128 and g.s1_lo("noq3dw,s1lo112") == 112


@pytest.mark.parametrize("sw,variant", [(sw, v) for sw, bodies in REFUSED.items() for v in bodies])
def test_refused_combination_raises_with_its_reason(sw, variant):
    with pytest.raises(ValueError) as ei:
        g.gen_body(variant, "nokara," + sw)
    msg = str(ei.value)
    assert sw in msg and "fthe_padic_" + variant in msg and REFUSED[sw][variant] in msg
    with pytest.raises(ValueError):
        g.gen_padic_mfma("x", ab=sw, **{k: v for k, v in g.BODIES[variant].items() if k != "clampbr"})


def test_bodies_table():
    assert list(g.BODIES) == ["m37", "m37t", "m37s", "m37l"]
    assert [b["clampbr"] for b in g.BODIES.values()] == [False, False, False, True]
    assert g.BODIES["m37s"]["q1_shift"] == g.Q1_SHIFT and g.BODIES["m37l"]["limb_op"] and \
        not any(b["top_est"] for v, b in g.BODIES.items() if v == "m37")
    with pytest.raises(KeyError):
        g.gen_body("m37x")


@pytest.mark.parametrize("variant", list(g.BODIES))
def test_every_switch_generates_and_assembles(variant, default, tmp_path):
    same = {"noclampbr"} if not g.BODIES[variant]["clampbr"] else {"clampbr"}      # the body's default, spelt out
    same |= {"nopair", "prio3"}           # nopair: every pair the fold could form is formed before the exchange
    for sw in ALL:
        if variant in REFUSED.get(sw, ()):
            continue
        asm = g.gen_body(variant, sw)
        assert f".globl fthe_padic_{variant}\n" in asm
        assert (asm == default[variant]) == (sw in same), sw
        src = tmp_path / f"{variant}_{sw}.s"
        src.write_text(asm)
        r = subprocess.run([f"{build.LLVM}/clang", "-x", "assembler", "-target", "amdgcn-amd-amdhsa",
                            f"-mcpu={build.ARCH}", "-c", str(src), "-o", str(tmp_path / "out.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, (sw, r.stderr[-2000:])


def test_calls_do_not_affect_each_other(default):
    for variant, sw in (("m37", "s1lo112"), ("m37t", "s1lo112"), ("m37s", "noq3dw"), ("m37l", "noclampbr")):
        assert g.gen_body(variant, sw) != default[variant]
        assert g.gen_body(variant, "") == default[variant]
    a = g.gen_body("m37", "s1lo112,noq3dw")
    assert a != g.gen_body("m37", "s1lo112") != g.gen_body("m37", "noq3dw") != a
    assert a == g.gen_body("m37", "noq3dw,s1lo112")
    assert g.s1_lo() == 128


def test_gen_body_gives_the_kernels_the_build_writes(default, monkeypatch):
    spelt = {"m37": g.gen_padic_mfma("fthe_padic_m37"),
             "m37t": g.gen_padic_mfma("fthe_padic_m37t", top_est=True),
             "m37s": g.gen_padic_mfma("fthe_padic_m37s", top_est=True, q1_shift=8),
             "m37l": g.gen_padic_mfma("fthe_padic_m37l", top_est=True, limb_op=True)}
    assert spelt == default
    assert default["m37"] == open(os.path.join(GEN, "padic_m37.s")).read()          # the committed one
    for variant in g.BODIES:
        built = os.path.join(GEN, f"padic_{variant}.s")
        if os.path.exists(built):                            # a copy the build left behind
            assert default[variant] == open(built).read(), variant
    # the environment no longer reaches the generator, at import or in a call
    monkeypatch.setenv("FTHE_GEN_M37_AB", "s1lo112,nokara")
    monkeypatch.setenv("FTHE_GEN_M37_SLEEPS", "3")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_padic_mfma_fresh", g.__file__)
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    assert fresh.gen_body("m37") == default["m37"] and g.gen_body("m37l") == default["m37l"]
    src = open(g.__file__).read()
    assert "environ" not in src and "getenv" not in src
