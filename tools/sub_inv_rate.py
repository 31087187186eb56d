"""The packed sibling subtraction by b's inverse beside the all-ones exponent: rows / s, device-resident,
Paillier-2048.

  python tools/sub_inv_rate.py [--n 1000000] [--rounds 3] [--out FILE]

a - b over n pair-packed ciphertexts, four ways in one process: fthe_sub_bits_dev(..., 192) (201 products mod
n^2 per row), fthe_sub_inv_dev with offset 2^192 (about 4: include/fthe.h) with the paired down step
and, FTHE_INV_NO_PAIR=1, composed of plain adds, and four fthe_add_dev
calls over the same rows -- the floor: the same product count with no tree, no host inversion and no stream
synchronisation.  One untimed pass of each at full size, then `rounds` readings of each in turn; medians, and every
reading for the spread.  Then GHPairs.compress of both differences at the slot widths their plaintext bounds
allow, and the bins a ciphertext holds after one and after two subtractions on either route.  Prints (and with
--out writes) one JSON line."""
import argparse
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


def _slot_width(pt_bits):
    from fedtree_amd.paillier import GH_SLOT_BITS_MIN
    return (max(pt_bits, GH_SLOT_BITS_MIN) + 31) // 32 * 32      # GHPairs.compress's default


def run(n, rounds):
    import torch
    from fedtree_amd.paillier import GH_PACKED_BITS, Device, Paillier, gh_slot_count, gh_slot_rows, packed_bits_after
    dev = Device(0)
    pl = Paillier(dev).keygen(2048, seed=20261021)
    cw = 2 * pl.n_words
    rng = np.random.default_rng(1)
    g = torch.from_numpy(rng.normal(0, 0.5, n).astype(np.float32)).cuda()
    h = torch.from_numpy(rng.uniform(1e-16, 0.25, n).astype(np.float32)).cuda()
    a = torch.empty((n, cw), dtype=torch.int32, device="cuda")
    pl.encrypt_gh_packed_dev(g, h, a, seed=2)
    dev.sync()
    b = a.roll(1, 0)                                    # father - computed: b is the a rows in another order
    d_bits, d_inv, d_add = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    offset = 1 << GH_PACKED_BITS

    def four_adds():
        pl.add_dev(a, b, d_add)
        for _ in range(3):
            pl.add_dev(d_add, b, d_add)

    def composed():                                     # the down-sweep's pairs as two adds each (read per call)
        os.environ["FTHE_INV_NO_PAIR"] = "1"
        try:
            pl.sub_inv_dev(a, b, d_inv, offset)
        finally:
            del os.environ["FTHE_INV_NO_PAIR"]

    os.environ.pop("FTHE_INV_NO_PAIR", None)
    arms = {"sub_bits": lambda: pl.sub_bits_dev(a, b, d_bits, GH_PACKED_BITS),
            "sub_inv": lambda: pl.sub_inv_dev(a, b, d_inv, offset),
            "sub_inv_composed": composed,
            "four_adds": four_adds}
    times = {k: [] for k in arms}
    products = {}
    for k, fn in arms.items():                          # one untimed pass at full size: buffers, programs
        _timed(dev, fn)
        products[k] = round(dev.last_montmuls() / n * (4 if k == "four_adds" else 1), 3)
    for _ in range(rounds):
        for k, fn in arms.items():
            times[k].append(_timed(dev, fn))
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"tool": "sub_inv_rate", "key_bits": 2048, "rows": n, "rounds": rounds,
           "seconds": {k: [round(t, 5) for t in v] for k, v in times.items()},
           "rows_per_s": {k: round(n / med[k]) for k in arms},
           "products_per_row": products,
           "sub_bits_spread": round(max(times["sub_bits"]) / min(times["sub_bits"]), 4),
           "sub_inv_over_sub_bits": round(med["sub_bits"] / med["sub_inv"], 2),
           "sub_inv_time_over_four_adds": round(med["sub_inv"] / med["four_adds"], 3),
           # the paired down step (fthe_addb_pair) against the two adds it replaces, same process, in turn
           "paired_over_composed_time": round(med["sub_inv"] / med["sub_inv_composed"], 4),
           "composed_spread": round(max(times["sub_inv_composed"]) / min(times["sub_inv_composed"]), 4)}
    # both differences decode to the same floats and codes (the first rows of the batch)
    w = min(n, 4096)
    dec = [pl.decrypt_gh_packed(x[:w].cpu().numpy().view(np.uint32), codes=True) for x in (d_bits, d_inv)]
    res["decoded_equal"] = all(np.array_equal(x, y) for x, y in zip(*dec))
    # compress each difference at the slot width its bound allows
    one = {"sub_bits": packed_bits_after("sub", GH_PACKED_BITS, GH_PACKED_BITS),
           "sub_inv": packed_bits_after("sub_inv", GH_PACKED_BITS, GH_PACKED_BITS)}
    two = {"sub_bits": packed_bits_after("sub", one["sub_bits"], one["sub_bits"]),
           "sub_inv": packed_bits_after("sub_inv", one["sub_inv"], one["sub_inv"])}
    res["bins_per_ciphertext"] = {
        k: {"after_one": gh_slot_count(pl.keyLength, _slot_width(one[k])), "slot_bits_after_one": _slot_width(one[k]),
            "after_two": gh_slot_count(pl.keyLength, _slot_width(two[k])), "slot_bits_after_two": _slot_width(two[k])}
        for k in one}
    res["compress"] = {}
    for k, x in (("sub_bits", d_bits), ("sub_inv", d_inv)):
        sb = _slot_width(one[k])
        slots = gh_slot_count(pl.keyLength, sb)
        out = torch.empty((gh_slot_rows(n, slots), cw), dtype=torch.int32, device="cuda")
        fn = lambda: pl.compress_gh_slots_dev(x, n, sb, out, slots)
        _timed(dev, fn)
        ts = [_timed(dev, fn) for _ in range(rounds)]
        res["compress"][k] = {"slot_bits": sb, "slots": slots, "seconds": [round(t, 5) for t in ts],
                              "bins_per_s": round(n / float(np.median(ts)))}
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
