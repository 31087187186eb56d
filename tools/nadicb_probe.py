#!/usr/bin/env python3
"""GPU bring-up probe of fthe_nadic_b76 through fthe_debug_nadicb_prog: the five single-op programs of
tools/barrett_cases.py (LOADX/STOREX, CANON, one SQR, one MUL, SQR x3 + MUL) on its crafted pairs, then random digits in
[0, 3n), every ciphertext's output digits against tools/nadicb_model.py's (the exact digits, not only the residue) by
barrett_cases.check_nadicb -- the cases and the checker of tests/test_gpu_nadicb_digits.py, here on one seeded key and
with a report of where the mismatches lie.  Prints one JSON line per program.
    python tools/nadicb_probe.py [count]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import barrett_cases as dc  # noqa: E402
import nadicb_model as nm  # noqa: E402
from fedtree_amd.paillier import Device, Paillier  # noqa: E402


def main():
    cnt = int(sys.argv[1]) if len(sys.argv) > 1 else 1536
    dev = Device(0)
    pl = Paillier(dev).keygen(2048, seed=7)
    n = pl.modulus
    key = nm.Key(n)
    rng = dc.make_rng("probe", n)
    total = 0
    for name, prog in dc.NADICB_PROGS.items():
        two = dc.MUL in prog[::2]
        crafted = dc.nadicb_mul_pairs(n) if two else [(x, (0, 0)) for x in dc.nadicb_pairs(n)]
        ops = (crafted + [(dc.filler(rng, 3 * n), dc.filler(rng, 3 * n)) for _ in range(cnt)])[:cnt]
        slots = np.zeros((4, cnt, 2 * dc.NS), dtype=np.uint32)
        for s in range(2):
            slots[s] = np.array([dc.nadicb_row(op[s]) for op in ops], dtype=np.uint32)
        out = pl.debug_nadicb_prog(prog, slots, 1 if name in ("io", "canon") else 2)
        bad, why = [], None
        for g, (x, y) in enumerate(ops):
            try:
                dc.check_nadicb(n, prog, {0: x, 1: y}, out[g], model=dc.nadicb_model_run(key, prog, {0: x, 1: y}))
            except dc.Mismatch as e:
                bad.append(g)
                why = why or str(e)
        info = {"test": name, "count": cnt, "bad": len(bad)}
        if bad:
            info.update(first=bad[0], why_first=why, bad_ct_in_wave=sorted({b % 16 for b in bad}),
                        bad_waves=sorted({(b // 16) % 12 for b in bad}))
        print(json.dumps(info), flush=True)
        total += len(bad)
    sys.exit(1 if total else 0)


if __name__ == "__main__":
    main()
