"""Paillier-3072 negate and subtract: invert_dev and sub_inv_dev per second on the radix-8 kernels (fthe_inv192_up /
fthe_inv192_down, FTHE_INV192_TREE=0) against the binary tree on fthe_mul192 of the same library (the default),
device-resident.

  python tools/sub_inv3072_rate.py [--rows 16384,65536,1048576] [--rounds 3] [--reps 2] [--out FILE]

A seeded 3072-bit key (keygen, seed 3072; its public copy runs the calls), random rows of 192 words, which are units mod
n^2 but for a negligible chance.  The arms "fused" and "tree" run interleaved: each reading is a fresh child process
(this one never opens the GPU) that makes one untimed pass at full size and then times `reps` calls queued back to back
under a host clock ending in a device synchronise; seconds are per call.  Each child also times four add_dev calls on
the same rows, the yardstick of DESIGN.md 20.  Medians, every reading for the spread, products per row from the engine's
own count, and a verdict per size and call: "fused" is called faster (or slower) only if every one of its readings lies
below (above) every reading of "tree".  The two arms' results are compared byte for byte through a digest, and the
first rows against Python's pow.  Prints (and with --out writes) one JSON line."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CW = 192
CALLS = ("invert", "sub_inv", "four_adds")


def child(sizes, reps):
    import torch
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    pl = Paillier.from_public(Paillier(dev).keygen(3072, seed=3072).modulus, dev)
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

    res = {c: {} for c in CALLS}
    res.update(products_per_row={}, digest={}, equal_python=True)
    for rows in sizes:
        x = torch.randint(-2**31, 2**31, (rows, CW), dtype=torch.int32, device="cuda", generator=g)
        a = torch.randint(-2**31, 2**31, (rows, CW), dtype=torch.int32, device="cuda", generator=g)
        out = torch.empty_like(x)

        def adds():
            for _ in range(4):
                pl.add_dev(a, x, out)
        fns = {"four_adds": adds, "invert": lambda: pl.invert_dev(x, out),
               "sub_inv": lambda: pl.sub_inv_dev(a, x, out, offset=1 << 64)}
        per = {}
        for c in CALLS:
            timed(fns[c], 1)
            per[c] = dev.last_montmuls() / rows
            res[c][rows] = timed(fns[c], reps)
            if c == "sub_inv":
                N = pl.n2
                want = [s * pow(t % N, -1, N) * (1 + (pl.modulus << 64)) % N
                        for s, t in zip(ints(a[-2:]), ints(x[-2:]))]
                res["equal_python"] &= ints(out[-2:]) == want
                res["digest"][rows] = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()
        res["products_per_row"][rows] = {"invert": per["invert"], "sub_inv": per["sub_inv"]}
    print(json.dumps(res), flush=True)


def run(sizes, rounds, reps):
    arms = {"fused": {"FTHE_INV192_TREE": "0"}, "tree": {"FTHE_INV192_TREE": "1"}}
    seen = {a: [] for a in arms}
    for _ in range(rounds):
        for a, extra in arms.items():
            env = {k: v for k, v in os.environ.items() if k != "FTHE_INV192_TREE"}
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rows", ",".join(map(str, sizes)),
                   "--reps", str(reps)]
            r = subprocess.run(cmd, env=dict(env, **extra), capture_output=True, text=True, timeout=900)
            if r.returncode:
                raise SystemExit(f"{a}: exit {r.returncode}\n{r.stderr[-2000:]}")
            seen[a].append(json.loads(r.stdout.strip().splitlines()[-1]))
    every = [c for v in seen.values() for c in v]
    out = {"tool": "sub_inv3072_rate", "key_bits": 3072, "kernels": "fthe_inv192_up / fthe_inv192_down", "rows": sizes,
           "rounds": rounds, "calls_per_reading": reps, "results_equal_python": all(c["equal_python"] for c in every),
           "arms_equal_bytes": all(c["digest"] == every[0]["digest"] for c in every), "sizes": {}}
    for rows in sizes:
        k = str(rows)
        s = {"products_per_row": {a: seen[a][0]["products_per_row"][k] for a in arms}}
        for c in CALLS:
            for a in arms:
                t = [r[c][k] for r in seen[a]]
                s[f"{c}_s_{a}"] = [round(v, 5) for v in t]
                s[f"{c}_rows_per_s_{a}"] = round(rows / float(np.median(t)))
            f, t = s[f"{c}_s_fused"], s[f"{c}_s_tree"]
            s[f"{c}_tree_over_fused"] = round(float(np.median(t) / np.median(f)), 3)
            s[f"{c}_verdict"] = "fused faster" if max(f) < min(t) else "fused slower" if min(f) > max(t) else "within spread"
        out["sizes"][k] = s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="16384,65536,1048576")
    ap.add_argument("--rounds", type=int, default=3, help="readings of each arm, in turn, one child process each")
    ap.add_argument("--reps", type=int, default=2, help="calls per reading")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    sizes = [int(v) for v in a.rows.split(",")]
    if a.child:
        return child(sizes, a.reps)
    line = json.dumps(run(sizes, a.rounds, a.reps))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
