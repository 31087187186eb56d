"""Paillier-3072 on fthe_pow192: r^n mod n^2 (the uniform scalar mul) and public-key encrypts per second, device-resident.

  python tools/pubenc3072_rate.py [--rows 16384,65536] [--rounds 3] [--reps 2] [--other-lib FILE] [--out FILE]

Arm "this": this tree's library, scalar_mul_dev(r, n) over `rows` random rows for each size, then encrypt_u64_dev of as
many u64 plaintexts with device-drawn r.  Arm "other" (--other-lib: a libfthe.so built from another commit, loaded
through FTHE_LIB): the same scalar_mul_dev call, and no encrypt, which the parent of this kernel does not have at this
size.  The arms run interleaved: each reading is a fresh child process (this one never opens the GPU) that makes one
untimed pass at full size and then times `reps` calls queued back to back under a host clock ending in a device
synchronise; seconds are per call.  Medians, every reading for the spread, products per row from the engine's own
count, and a verdict per size: "this" is called faster only if every one of its readings lies below every reading of
"other".  The first rows of the child's results are checked against Python's pow.  Prints (and with --out writes)
one JSON line."""
import argparse
import json
import os
import random
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CW = 192


def child(sizes, reps, encrypt):
    import torch
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    n = random.Random(3072).getrandbits(3072) | (1 << 3071) | 1
    pl = Paillier.from_public(n, dev)
    g = torch.Generator(device="cuda").manual_seed(1)

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        dev.sync()
        return (time.perf_counter() - t0) / k

    def ints(t):
        a = np.ascontiguousarray(t.cpu().numpy()).view(np.uint8).reshape(len(t), -1)
        return [int.from_bytes(r.tobytes(), "little") for r in a]

    res = {"pow_s": {}, "enc_s": {}, "products_per_row": {}, "equal_python": True}
    for rows in sizes:
        x = torch.randint(-2**31, 2**31, (rows, CW), dtype=torch.int32, device="cuda", generator=g)
        x[:, CW // 2:] = 0                                  # r below 2^3072, as an encrypt's
        out = torch.empty_like(x)
        fn = lambda: pl.scalar_mul_dev(x, n, out)
        timed(fn, 1)
        res["products_per_row"][rows] = dev.last_montmuls() / rows
        res["pow_s"][rows] = timed(fn, reps)
        res["equal_python"] &= ints(out[:2]) == [pow(v, n, pl.n2) for v in ints(x[:2])]
        if encrypt:
            m = torch.randint(0, 2**62, (rows,), dtype=torch.int64, device="cuda", generator=g)
            fe = lambda: pl.encrypt_u64_dev(m, out, seed=7)
            timed(fe, 1)
            res["enc_s"][rows] = timed(fe, reps)
    print(json.dumps(res), flush=True)


def run(sizes, rounds, reps, other):
    arms = {"this": None, **({"other": other} if other else {})}
    seen = {a: [] for a in arms}
    for _ in range(rounds):
        for a, lib in arms.items():
            env = dict(os.environ, **({"FTHE_LIB": os.path.abspath(lib)} if lib else {}))
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rows", ",".join(map(str, sizes)),
                   "--reps", str(reps)] + ([] if lib is None else ["--no-encrypt"])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode:
                raise SystemExit(f"{a}: exit {r.returncode}\n{r.stderr[-2000:]}")
            seen[a].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"tool": "pubenc3072_rate", "key_bits": 3072, "kernel": "fthe_pow192", "rows": sizes, "rounds": rounds,
           "calls_per_reading": reps, "other_lib": other,
           "results_equal_python": all(c["equal_python"] for v in seen.values() for c in v), "sizes": {}}
    for rows in sizes:
        k = str(rows)
        s = {"products_per_row": {a: seen[a][0]["products_per_row"][k] for a in arms}}
        for a in arms:
            t = [c["pow_s"][k] for c in seen[a]]
            s[f"pow_s_{a}"] = [round(v, 4) for v in t]
            s[f"pow_rows_per_s_{a}"] = round(rows / float(np.median(t)))
        enc = [c["enc_s"][k] for c in seen["this"]]
        s["encrypt_s"] = [round(v, 4) for v in enc]
        s["encrypts_per_s"] = round(rows / float(np.median(enc)))
        if other:
            s["this_faster_beyond_both_spreads"] = bool(max(s["pow_s_this"]) < min(s["pow_s_other"]))
            s["other_over_this"] = round(float(np.median(s["pow_s_other"]) / np.median(s["pow_s_this"])), 3)
        out["sizes"][k] = s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="16384,65536")
    ap.add_argument("--rounds", type=int, default=3, help="readings of each arm, in turn, one child process each")
    ap.add_argument("--reps", type=int, default=2, help="calls per reading")
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-encrypt", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    sizes = [int(v) for v in a.rows.split(",")]
    if a.child:
        return child(sizes, a.reps, not a.no_encrypt)
    line = json.dumps(run(sizes, a.rounds, a.reps, a.other_lib))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
