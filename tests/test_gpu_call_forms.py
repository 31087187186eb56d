"""Which form a CRT encrypt / decrypt takes (fthe.hip plan_call): both halves on the four-lane s80 kernel
(quad), the q half on the side stream in a second slot region (the small split, and large calls while
FTHE_SPLIT_ALL is on), or the halves in turn in one region -- pinned at the smallest shapes that reach
every form.

The thresholds are read once per process, so a child process per setting runs the calls with the thresholds
pulled down to a few hundred rows, on the golden keys with n of 2048, 1024 and 512 bits (the key_length_arg of
the golden files counts the bits of n^2):
  200 rows   quad on the Paillier-2048 key; the smaller keys have no s80 shape and take the small split
  400 rows   the small split
  2500 rows  two chunks of 1024 and one of 452: halves side by side, or in turn under FTHE_SPLIT_ALL=0
Every encrypt's bits equal those of the same seeded call at the default thresholds (made in this process),
every decrypt returns its plaintexts, and every call's fingerprint -- fthe_last_montmuls, the profiled launches
and the exponentiation launches per kernel variant -- equals a literal below.  The s80 count tells quad from
the rest, the launch count one chunk from three and the split forms (p program + CRT tail) from the in-turn one.

The literals were measured, not predicted: this probe's report against the library as it was before
plan_call gathered the form and region decisions of encrypt_impl and decrypt_impl in one place.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden_key, load_golden

pytestmark = pytest.mark.gpu

KNOBS = dict(FTHE_CHUNK="1024", FTHE_ENC_CHUNK="1024", FTHE_DEC_QUAD="256", FTHE_DEC_SPLIT="512")
SETTINGS = {"side_by_side": {}, "in_turn": {"FTHE_SPLIT_ALL": "0"}}
KEYS = {2048: "ref_gmp_L4096.json", 1024: "ref_gmp_L2048.json", 512: "ref_gmp_L1024.json"}    # by the bits of n
COUNTS = (200, 400, 2500)
OPS = ("enc", "dec", "short", "enc_r")
VARIANTS = (37, 74, 80, 1019, 1037, 1137)
SEED = 1234

# (key bits, rows, call) -> (fthe_last_montmuls, profiled launches, exponentiation launches per VARIANTS)
FORMS = {
    (2048, 200, 'enc'): (481200, 3, (0, 0, 2, 0, 0, 0)),
    (2048, 200, 'dec'): (481400, 5, (0, 0, 2, 0, 0, 0)),
    (2048, 200, 'short'): (240200, 2, (0, 0, 1, 0, 0, 0)),
    (2048, 200, 'enc_r'): (961800, 6, (2, 0, 0, 0, 0, 2)),
    (2048, 400, 'enc'): (962400, 5, (0, 0, 0, 0, 0, 2)),
    (2048, 400, 'dec'): (964400, 9, (0, 0, 0, 0, 0, 2)),
    (2048, 400, 'short'): (481200, 4, (0, 0, 0, 0, 0, 1)),
    (2048, 400, 'enc_r'): (1923600, 6, (2, 0, 0, 0, 0, 2)),
    (2048, 2500, 'enc'): (6015000, 15, (0, 0, 0, 0, 0, 6)),
    (2048, 2500, 'dec'): (6027500, 27, (0, 0, 0, 0, 0, 6)),
    (2048, 2500, 'short'): (3007500, 12, (0, 0, 0, 0, 0, 3)),
    (2048, 2500, 'enc_r'): (12022500, 18, (6, 0, 0, 0, 0, 6)),
    (1024, 200, 'enc'): (245200, 5, (0, 0, 0, 2, 0, 0)),
    (1024, 200, 'dec'): (246400, 9, (0, 0, 0, 2, 0, 0)),
    (1024, 200, 'short'): (123200, 4, (0, 0, 0, 1, 0, 0)),
    (1024, 200, 'enc_r'): (489200, 6, (2, 0, 0, 2, 0, 0)),
    (1024, 400, 'enc'): (490400, 5, (0, 0, 0, 2, 0, 0)),
    (1024, 400, 'dec'): (492800, 9, (0, 0, 0, 2, 0, 0)),
    (1024, 400, 'short'): (246400, 4, (0, 0, 0, 1, 0, 0)),
    (1024, 400, 'enc_r'): (978400, 6, (2, 0, 0, 2, 0, 0)),
    (1024, 2500, 'enc'): (3065000, 15, (0, 0, 0, 6, 0, 0)),
    (1024, 2500, 'dec'): (3080000, 27, (0, 0, 0, 6, 0, 0)),
    (1024, 2500, 'short'): (1540000, 12, (0, 0, 0, 3, 0, 0)),
    (1024, 2500, 'enc_r'): (6115000, 18, (6, 0, 0, 6, 0, 0)),
    (512, 200, 'enc'): (125400, 3, (2, 0, 0, 0, 0, 0)),
    (512, 200, 'dec'): (125600, 5, (2, 0, 0, 0, 0, 0)),
    (512, 200, 'short'): (62600, 2, (1, 0, 0, 0, 0, 0)),
    (512, 200, 'enc_r'): (250000, 4, (4, 0, 0, 0, 0, 0)),
    (512, 400, 'enc'): (250800, 3, (2, 0, 0, 0, 0, 0)),
    (512, 400, 'dec'): (251200, 5, (2, 0, 0, 0, 0, 0)),
    (512, 400, 'short'): (125200, 2, (1, 0, 0, 0, 0, 0)),
    (512, 400, 'enc_r'): (500000, 4, (4, 0, 0, 0, 0, 0)),
    (512, 2500, 'enc'): (1567500, 9, (6, 0, 0, 0, 0, 0)),
    (512, 2500, 'dec'): (1570000, 15, (6, 0, 0, 0, 0, 0)),
    (512, 2500, 'short'): (782500, 6, (3, 0, 0, 0, 0, 0)),
    (512, 2500, 'enc_r'): (3125000, 12, (12, 0, 0, 0, 0, 0)),
}
# the 2,500-row calls that differ with the halves in turn (FTHE_SPLIT_ALL=0): the encrypts, whose split form runs
# the CRT tail as a launch of its own; a decrypt makes the same launches either way, on one stream or two
FORMS_IN_TURN = {
    (2048, 2500, 'enc'): (6015000, 12, (0, 0, 0, 0, 0, 6)),
    (1024, 2500, 'enc'): (3065000, 12, (0, 0, 0, 6, 0, 0)),
    (512, 2500, 'enc'): (1567500, 6, (6, 0, 0, 0, 0, 0)),
}

def inputs(bits):
    """(p, q, plaintexts, injected r words) of a key: 2,500 rows, the smaller counts take the first rows."""
    g = load_golden(KEYS[bits])
    p, q = golden_key(g)
    rng = np.random.default_rng(bits)
    m = rng.integers(0, 2**64, max(COUNTS), dtype=np.uint64)
    m[:4] = [0, 1, 2**64 - 1, 2**63]
    r = rng.integers(1, 2**32, (max(COUNTS), g["n_words"] - 1), dtype=np.uint32)    # r < 2^(32 (n_words - 1)) < n
    return p, q, m, r


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


_PROBE = r'''
import ctypes, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_call_forms as T
from fedtree_amd import _lib
from fedtree_amd.paillier import Device, Paillier

dev = Device(0)
lib = dev.lib


def profiled(fn):
    """fn's result and its fingerprint: products, launches, exponentiation launches per kernel variant."""
    lib.fthe_prof_enable(dev.ctx, 1)
    try:
        out = fn()
        mm = dev.last_montmuls()
        vals = [ctypes.c_double() for _ in range(7)]
        _lib.check(lib.fthe_prof_read(dev.ctx, *[ctypes.byref(v) for v in vals]), "prof_read")
        per = []
        for S in T.VARIANTS:
            ms, n = ctypes.c_double(), ctypes.c_double()
            lib.fthe_prof_variant(dev.ctx, S, ctypes.byref(ms), ctypes.byref(n))
            per.append(int(n.value))
    finally:
        lib.fthe_prof_enable(dev.ctx, 0)
    return out, [mm, int(vals[1].value), per]


report = {"calls": []}
for bits in T.KEYS:
    p, q, m, r = T.inputs(bits)
    pl = Paillier.from_primes(p, q, dev)
    for n in T.COUNTS:
        c, f_enc = profiled(lambda: pl.encrypt_u64(m[:n], seed=T.SEED))
        lo, f_dec = profiled(lambda: pl.decrypt_u64(c))
        sh, f_short = profiled(lambda: pl.decrypt_u64(c, short=True))
        cr, f_r = profiled(lambda: pl.encrypt_u64(m[:n], r=r[:n]))
        back = pl.decrypt_u64(cr)
        for op, f, dg, ok in (("enc", f_enc, T.digest(c), None), ("dec", f_dec, None, np.array_equal(lo, m[:n])),
                              ("short", f_short, None, np.array_equal(sh, m[:n])),
                              ("enc_r", f_r, T.digest(cr), np.array_equal(back, m[:n]))):
            report["calls"].append({"bits": bits, "n": n, "op": op, "form": f, "digest": dg,
                                    "ok": None if ok is None else bool(ok)})
if sys.argv[2] == "cap":
    # the context's cap falling by 0.8x from one that holds the two regions of a 1,024-row chunk several times
    # over, down to the first that cannot hold one (tests/test_gpu_split_streams.py
    # test_mem_limit_one_region_fallback, at this size); the Paillier-1024 key is that test's
    report["cap"] = {}
    for bits in (2048, 1024):
        p, q, m, _ = T.inputs(bits)
        want = Paillier.from_primes(p, q, dev).encrypt_u64(m, seed=404)
        cap, ok_caps, failed, status, same = 128 << 20, [], None, None, True
        while cap > (1 << 20):
            d = Device(0)
            d.set_mem_limit(cap)
            pc = Paillier.from_primes(p, q, d)
            try:
                c = pc.encrypt_u64(m, seed=404)
            except _lib.FtheError as ex:
                failed, status = cap, ex.status
                break
            same = same and bool(np.array_equal(c, want)) and bool(np.array_equal(pc.decrypt_u64(c), m))
            ok_caps.append(cap)
            cap = int(cap * 0.8)
        report["cap"][str(bits)] = {"ok_caps": ok_caps, "failed": failed, "status": status, "same": same}
print(json.dumps(report))
'''


def run_child(tmp, setting, lib=None):
    """The probe's report under KNOBS and a setting (lib: another library, for measuring the literals)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    probe = tmp / "probe.py"
    probe.write_text(_PROBE)
    env = dict(os.environ, **KNOBS, **SETTINGS[setting])
    if lib:
        env["FTHE_LIB"] = lib
    r = subprocess.run([sys.executable, str(probe), root, "cap" if setting == "side_by_side" else "-"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    rep = json.loads(r.stdout.splitlines()[-1])
    rep["calls"] = {(c["bits"], c["n"], c["op"]): c for c in rep["calls"]}
    return rep


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("call_forms")
    return {s: run_child(tmp, s) for s in SETTINGS}


@pytest.fixture(scope="module")
def default_digests():
    """The encrypts' ciphertext digests at the default thresholds (this process)."""
    from fedtree_amd.paillier import Device, Paillier
    dev, out = Device(0), {}
    for bits in KEYS:
        p, q, m, r = inputs(bits)
        pl = Paillier.from_primes(p, q, dev)
        for n in COUNTS:
            out[bits, n, "enc"] = digest(pl.encrypt_u64(m[:n], seed=SEED))
            out[bits, n, "enc_r"] = digest(pl.encrypt_u64(m[:n], r=r[:n]))
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_same_bits_in_every_form(children, default_digests, setting):
    calls = children[setting]["calls"]
    assert len(calls) == len(KEYS) * len(COUNTS) * len(OPS)
    for key, want in default_digests.items():
        assert calls[key]["digest"] == want, key


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_round_trip_in_every_form(children, setting):
    for key, c in children[setting]["calls"].items():
        if key[2] != "enc":
            assert c["ok"] is True, key


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_form_of_every_call(children, setting):
    want = {**FORMS, **(FORMS_IN_TURN if setting == "in_turn" else {})}
    got = {key: (c["form"][0], c["form"][1], tuple(c["form"][2])) for key, c in children[setting]["calls"].items()}
    for key in got:
        print(key, got[key])
    assert got == want


@pytest.mark.parametrize("bits", [2048, 1024])
def test_mem_cap_one_region_fallback_small(children, bits):
    """test_mem_limit_one_region_fallback at 2,500 rows in chunks of 1,024: identical ciphertexts (and plaintexts
    back) at every cap above the failing one, NOMEM there, and the last good cap below twice the failing one --
    so that call ran in one region."""
    from fedtree_amd import _lib
    cap = children["side_by_side"]["cap"][str(bits)]
    print(cap)
    assert cap["same"] is True
    assert cap["failed"] is not None and cap["status"] == _lib.FTHE_ERR_NOMEM, cap
    assert cap["ok_caps"] and cap["ok_caps"][-1] < 2 * cap["failed"], cap
