"""Per-row plaintext weights beside what the engine had before them: rows / s and terms / s, device-resident,
Paillier-2048.

  python tools/dot_rate.py [--n 1000000] [--rounds 3] [--out FILE]

(a) fthe_scalar_mul_rows_dev over n rows, every exponent 2^64 - 1 and random 20-bit exponents, against
    fthe_scalar_mul_u64_dev (one exponent for the batch) on the same rows.
(b) fthe_dot_segments_dev over n terms with random 64-bit weights, forced to each of its three forms
    (FTHE_DOT_WINDOW = 0, 4, 8), in 28 segments and in n / 8 segments of 8, against the composition the engine
    allowed before: a host loop of fthe_scalar_mul_u64_dev calls, one per distinct weight (16 of them, each over
    its sixteenth of the terms), then fthe_reduce_segments_csr_dev.
One process; one untimed pass of every arm at full size, then `rounds` readings of each in turn; medians, and every
reading for the spread.  The form dot_plan names at each shape is recorded beside the fastest.  Prints (and with
--out writes) one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(dev, fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    dev.sync()
    return time.perf_counter() - t0


def _u64(pl, dev, x, k, out):
    """fthe_scalar_mul_u64_dev: one exponent for the rows of x."""
    from fedtree_amd import _lib
    _lib.check(pl.lib.fthe_scalar_mul_u64_dev(pl._key, dev.ctx, ctypes.c_void_p(x.data_ptr()), int(k), x.shape[0],
                                              ctypes.c_void_p(out.data_ptr())), "scalar_mul_u64_dev")


def _forced(window, fn):
    def run():
        os.environ["FTHE_DOT_WINDOW"] = str(window)
        try:
            fn()
        finally:
            del os.environ["FTHE_DOT_WINDOW"]
    return run


def _measure(dev, arms, rounds, n):
    times, products = {k: [] for k in arms}, {}
    for k, fn in arms.items():                          # one untimed pass at full size: buffers, programs
        _timed(dev, fn)
        products[k] = round(dev.last_montmuls() / n, 3)
    for _ in range(rounds):
        for k, fn in arms.items():
            times[k].append(_timed(dev, fn))
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"seconds": {k: [round(t, 5) for t in v] for k, v in times.items()},
            "per_s": {k: round(n / med[k]) for k in arms},
            "spread": {k: round(max(v) / min(v), 4) for k, v in times.items()},
            "products_per_item": products}, med


def run(n, rounds):
    import torch
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    pl = Paillier(dev).keygen(2048, seed=20261021)
    cw = 2 * pl.n_words
    rng = np.random.default_rng(1)
    m = torch.from_numpy(rng.integers(0, 2**62, n, dtype=np.int64)).cuda()
    x = torch.empty((n, cw), dtype=torch.int32, device="cuda")
    pl.encrypt_u64_dev(m, x, seed=2)
    dev.sync()
    out = torch.empty_like(x)
    res = {"tool": "dot_rate", "key_bits": 2048, "n": n, "rounds": rounds}

    # (a) one exponent per row
    def words(vals):
        return torch.from_numpy(np.ascontiguousarray(vals.astype(np.uint64)).view(np.int32).reshape(n, 2)).cuda()

    e_ones = words(np.full(n, 2**64 - 1, dtype=np.uint64))
    e_20 = words(rng.integers(0, 2**20, n, dtype=np.uint64))
    arms = {"rows_all_ones_64": lambda: pl.scalar_mul_rows_dev(x, e_ones, out),
            "rows_random_20": lambda: pl.scalar_mul_rows_dev(x, e_20, out),
            "u64_all_ones_64": lambda: _u64(pl, dev, x, 2**64 - 1, out),
            "u64_20_bits": lambda: _u64(pl, dev, x, 2**20 - 1, out)}
    res["rows"], med = _measure(dev, arms, rounds, n)
    res["rows"]["rows_over_u64_time"] = {"all_ones_64": round(med["rows_all_ones_64"] / med["u64_all_ones_64"], 3),
                                         "20_bits": round(med["rows_random_20"] / med["u64_20_bits"], 3)}
    # of the launches of a 64-bit call's main loop and table, the share that are squarings (a later entry point
    # that keeps the limbs in registers between squarings works on these)
    res["rows"]["squaring_share_of_products_64"] = round(60 / 89, 3)

    # (b) weighted segment sums
    e_64 = words(rng.integers(0, 2**64, n, dtype=np.uint64))
    distinct = [int(v) for v in rng.integers(1, 2**64, 16, dtype=np.uint64)]
    block = (n + 15) // 16
    res["dot"] = {}
    for label, nseg in (("28_segments", 28), ("segments_of_8", n // 8)):
        bounds = np.linspace(0, n, nseg + 1).astype(np.int64)
        seg = torch.from_numpy(bounds).cuda()
        o = torch.empty((nseg, cw), dtype=torch.int32, device="cuda")

        def parent_composition():
            for j, k in enumerate(distinct):
                lo, hi = j * block, min(n, (j + 1) * block)
                if lo < hi:
                    _u64(pl, dev, x[lo:hi], k, out[lo:hi])
            pl.reduce_segments_csr_dev(out, seg, o)

        arms = {f"dot_w{w}": _forced(w, lambda: pl.dot_segments_dev(x, e_64, seg, o)) for w in (0, 4, 8)}
        arms["u64_loop_16_weights"] = parent_composition
        r, med = _measure(dev, arms, rounds, n)
        forms = {w: med[f"dot_w{w}"] for w in (0, 4, 8)}
        fastest = min(forms, key=forms.get)
        plan = pl.dot_plan(64, n, nseg)
        r.update({"nseg": nseg, "plan": plan, "fastest": fastest,
                  "plan_over_fastest_time": round(forms[plan] / forms[fastest], 4),
                  "fastest_over_u64_loop_time": round(forms[fastest] / med["u64_loop_16_weights"], 4)})
        res["dot"][label] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3, help="timed readings of each arm, in turn")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = json.dumps(run(a.n, a.rounds))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
