"""Paillier-3072 adds on fthe_mul192: rows / s, device-resident.

  python tools/add3072_rate.py [--rows 1048576] [--merge-rows 262144] [--rounds 5] [--reps 100] [--out FILE]

Two arms in one process on a seeded 3072-bit odd n (a public key; the product needs no factorisation): fthe_add_dev
over `rows` random rows, and the 8-way fthe_reduce_kway_dev of `merge-rows` rows (seven products per row).  One
untimed pass of each at full size, then `rounds` readings of each in turn, a reading being `reps` calls queued back
to back under a host clock that ends in a device synchronise (seconds are per call); medians, every reading for the
spread, and the kernel time of the last call from the engine's own events.  Bytes per second against HBM count what
an add must move: 3 x 768 B per product.  The yardstick is a * b % N on Python integers on one host thread, labelled as such
(not a multi-threaded GMP figure).  The first 64 rows of each result are checked against Python's integers.  Prints (and with --out writes) one JSON line."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CW = 192
HBM_BYTES_PER_S = 8.0e12          # MI355X peak, for the share only


def _timed(dev, fn, reps=1):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dev.sync()
    return (time.perf_counter() - t0) / reps


def _ints(t):
    a = np.ascontiguousarray(t.cpu().numpy()).view(np.uint8).reshape(len(t), -1)
    return [int.from_bytes(r.tobytes(), "little") for r in a]


def run(rows, merge_rows, rounds, reps):
    import torch
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    n = random.Random(3072).getrandbits(3072) | (1 << 3071) | 1
    pl = Paillier.from_public(n, dev)
    N = pl.n2
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda *shape: torch.randint(-2**31, 2**31, shape, dtype=torch.int32, device="cuda", generator=g)
    a, b = rand(rows, CW), rand(rows, CW)
    out = torch.empty_like(a)
    x8 = rand(8, merge_rows, CW)
    out8 = torch.empty((merge_rows, CW), dtype=torch.int32, device="cuda")
    arms = {"add": (lambda: pl.add_dev(a, b, out), rows, 1),
            "merge8": (lambda: pl.reduce_kway_dev(x8, 8, out8), merge_rows, 7)}
    times = {k: [] for k in arms}
    kernel_ms, products = {}, {}
    for k, (fn, cnt, _) in arms.items():                # one untimed pass at full size
        _timed(dev, fn)
        products[k] = dev.last_montmuls() / cnt
    for _ in range(rounds):
        for k, (fn, _, _) in arms.items():
            times[k].append(_timed(dev, fn, reps))
            kernel_ms[k] = round(dev.last_kernel_ms(), 3)
    w = 64
    xa, xb = _ints(a[:w]), _ints(b[:w])
    ok_add = _ints(out[:w]) == [p * q % N for p, q in zip(xa, xb)]
    planes = [_ints(x8[j, :w]) for j in range(8)]
    want = [1] * w
    for p in planes:
        want = [u * v % N for u, v in zip(want, p)]
    ok_merge = _ints(out8[:w]) == want
    # the host yardstick: one thread, Python integers
    t0 = time.perf_counter()
    host_reps = 200
    for _ in range(host_reps):
        for p, q in zip(xa, xb):
            p * q % N
    host_rate = host_reps * w / (time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in times.items()}
    rate = {k: arms[k][1] * arms[k][2] / med[k] for k in arms}        # products / s
    return {"tool": "add3072_rate",
            "command": f"python tools/add3072_rate.py --rows {rows} --merge-rows {merge_rows} --rounds {rounds} --reps {reps}",
            "key_bits": 3072, "kernel": "fthe_mul192 (VALU product, VALU Barrett)",
            "rows": rows, "merge_rows": merge_rows, "rounds": rounds, "calls_per_reading": reps,
            "seconds": {k: [round(t, 5) for t in v] for k, v in times.items()},
            "spread": {k: round(max(v) / min(v), 4) for k, v in times.items()},
            "last_kernel_ms": kernel_ms, "products_per_row": products,
            "adds_per_s": round(rate["add"]), "merge8_rows_per_s": round(merge_rows / med["merge8"]),
            "merge8_products_per_s": round(rate["merge8"]),
            "add_bytes_per_s": round(rate["add"] * 3 * 4 * CW),
            "add_share_of_hbm_peak": round(rate["add"] * 3 * 4 * CW / HBM_BYTES_PER_S, 4),
            "host_python_int_one_thread_products_per_s": round(host_rate),
            "adds_over_host_one_thread": round(rate["add"] / host_rate, 1),
            "beats_16x_host_one_thread": bool(rate["add"] > 16 * host_rate),
            "paillier2048_adds_per_s_for_orientation": 863e6,
            "results_equal_python": bool(ok_add and ok_merge)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--merge-rows", type=int, default=1 << 18)
    ap.add_argument("--rounds", type=int, default=5, help="timed readings of each arm, in turn")
    ap.add_argument("--reps", type=int, default=100, help="calls per reading (0.8 s and 1.4 s windows at the default sizes)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = json.dumps(run(a.rows, a.merge_rows, a.rounds, a.reps))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
