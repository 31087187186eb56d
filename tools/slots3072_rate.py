"""Paillier-3072 packed and slot-packed pairs: the compress on fthe_horner192 against the same result composed from
scalar mul and add, and bins per second of the packed forms beside the two-ciphertext flow, device-resident.

  python tools/slots3072_rate.py [--rows 16384,65536] [--bins 212992] [--rounds 3] [--reps 2] [--out FILE]

Compress.  Arm "fused": compress_gh_slots_dev of 13 rows x `rows` random ciphertext rows into `rows` outputs of 13
slots of 224 bits, one call.  Arm "composed": the same Horner walk from calls that do not touch fthe_horner192, per
plane below the top scalar_mul_dev(acc, 2^224, acc) then add_dev(acc, x_j, acc).  The arms run interleaved, each
reading a fresh child process (this one never opens the GPU) that makes one untimed pass at full size and then times
`reps` calls queued back to back under a host clock ending in a device synchronise; seconds are per call.  A child
reports the SHA-256 of its result: the two arms must agree byte for byte.  "fused" is called faster only if every
one of its readings lies below every reading of "composed".

Rates.  One more child: a key holder's 3072-bit key, `bins` (g, h) pairs; the public-key encrypt, the 8-way merge and
the full and short decrypt in the two-ciphertext, pair-packed and slot-packed forms (13 slots below n, 6 below p),
the forms timed in turn `rounds` times after one untimed pass; bins per second from the medians, every reading for
the spread.  Prints (and with --out writes) one JSON line."""
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

CW, SLOTS, SLOT_BITS, PARTIES = 192, 13, 224, 8


def _timed(dev, fn, k=1):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    dev.sync()
    return (time.perf_counter() - t0) / k


def compress_child(arm, sizes, reps):
    import random
    import torch
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    pl = Paillier.from_public(random.Random(3072).getrandbits(3072) | (1 << 3071) | 1, dev)
    g = torch.Generator(device="cuda").manual_seed(1)
    res = {"s": {}, "sha256": {}, "products_per_row": {}}
    for rows in sizes:
        x = torch.randint(-2**31, 2**31, (SLOTS * rows, CW), dtype=torch.int32, device="cuda", generator=g)
        out = torch.empty((rows, CW), dtype=torch.int32, device="cuda")

        def composed():
            out.copy_(x[(SLOTS - 1) * rows:])
            for j in reversed(range(SLOTS - 1)):
                pl.scalar_mul_dev(out, 1 << SLOT_BITS, out)
                pl.add_dev(out, x[j * rows:(j + 1) * rows], out)

        fn = composed if arm == "composed" else lambda: pl.compress_gh_slots_dev(x, SLOTS * rows, SLOT_BITS, out)
        _timed(dev, fn)
        if arm == "fused":
            res["products_per_row"][rows] = dev.last_montmuls() / rows
        res["s"][rows] = _timed(dev, fn, reps)
        res["sha256"][rows] = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()
    print(json.dumps(res), flush=True)


def rates_child(n, rounds):
    import torch
    from fedtree_amd.paillier import Device, Paillier, decode_fixed, encode_fixed, gh_slot_rows
    dev = Device(0)
    pl = Paillier(dev).keygen(3072, seed=3072)
    short_slots = pl.gh_slots(SLOT_BITS, short=True)
    rng = np.random.default_rng(1)
    g = rng.normal(0, 0.5, n).astype(np.float32)
    h = rng.uniform(1e-16, 0.25, n).astype(np.float32)
    gd, hd = torch.from_numpy(g).cuda(), torch.from_numpy(h).cuda()
    md = torch.from_numpy(np.concatenate([encode_fixed(g), encode_fixed(h)]).view(np.int64)).cuda()
    rows = lambda k: torch.empty((k, CW), dtype=torch.int32, device="cuda")
    x2, xp, xs, xss = rows(2 * n), rows(n), rows(gh_slot_rows(n, SLOTS)), rows(gh_slot_rows(n, short_slots))
    res = {"slots": pl.gh_slots(SLOT_BITS), "slots_short": short_slots}

    def rate(key, forms):
        for fn in forms.values():
            _timed(dev, fn)
        ts = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                ts[k].append(_timed(dev, fn))
        res[key] = {**{f"{k}_bins_per_s": round(n / float(np.median(v))) for k, v in ts.items()},
                    **{f"{k}_s": [round(t, 4) for t in v] for k, v in ts.items()}}

    rate("encrypt_public", {"two_ct": lambda: pl.encrypt_u64_dev(md, x2, seed=2, public=True),
                            "pair_packed": lambda: pl.encrypt_gh_packed_dev(gd, hd, xp, seed=2, public=True),
                            "slotted": lambda: pl.encrypt_gh_slots_dev(gd, hd, xs, SLOT_BITS, seed=2, public=True)})
    pl.encrypt_gh_slots_dev(gd, hd, xss, SLOT_BITS, seed=2, public=True, slots=short_slots)
    k2, kp, ks = (torch.cat([x.roll(k, 0) for k in range(PARTIES)]) for x in (x2, xp, xs))
    o2, op, os_ = torch.empty_like(x2), torch.empty_like(xp), torch.empty_like(xs)
    rate("merge", {"two_ct": lambda: pl.reduce_kway_dev(k2, PARTIES, o2),
                   "pair_packed": lambda: pl.reduce_kway_dev(kp, PARTIES, op),
                   "slotted": lambda: pl.reduce_kway_dev(ks, PARTIES, os_)})
    del k2, kp, ks, o2, op, os_
    low = torch.empty(2 * n, dtype=torch.int64, device="cuda")
    dg, dh, sg, sh = (torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(4))
    for short in (False, True):
        src, s = (xss, short_slots) if short else (xs, SLOTS)
        rate("decrypt_short" if short else "decrypt_full", {
            "two_ct": lambda: pl.decrypt_u64_dev(x2, low, short=short),
            "pair_packed": lambda: pl.decrypt_gh_packed_dev(xp, dg, dh, short=short),
            "slotted": lambda: pl.decrypt_gh_slots_dev(src, n, SLOT_BITS, sg, sh, short=short, slots=s)})
    lo = low.cpu().numpy().view(np.uint64)
    res["decoded_equal"] = bool(np.array_equal(decode_fixed(lo[:n]), sg.cpu().numpy())
                                and np.array_equal(decode_fixed(lo[n:]), sh.cpu().numpy())
                                and np.array_equal(dg.cpu().numpy(), sg.cpu().numpy())
                                and np.array_equal(dh.cpu().numpy(), sh.cpu().numpy()))
    print(json.dumps(res), flush=True)


def _child(args, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode:                                     # nothing more runs on the GPU after a failed child
        raise SystemExit(f"{args}: exit {r.returncode}\n{(r.stdout + r.stderr)[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def run(sizes, bins, rounds, reps, timeout):
    arms = ("fused", "composed")
    seen = {a: [] for a in arms}
    for _ in range(rounds):
        for a in arms:
            seen[a].append(_child(["--child", a, "--rows", ",".join(map(str, sizes)), "--reps", str(reps)], timeout))
    out = {"tool": "slots3072_rate", "key_bits": 3072, "kernel": "fthe_horner192", "slots": SLOTS, "slot_bits": SLOT_BITS,
           "rounds": rounds, "calls_per_reading": reps, "compress": {}}
    for rows in sizes:
        k = str(rows)
        t = {a: [c["s"][k] for c in seen[a]] for a in arms}
        out["compress"][k] = {
            "products_per_row": seen["fused"][0]["products_per_row"][k],
            **{f"{a}_s": [round(v, 4) for v in t[a]] for a in arms},
            **{f"{a}_bins_per_s": round(SLOTS * rows / float(np.median(t[a]))) for a in arms},
            "composed_over_fused": round(float(np.median(t["composed"]) / np.median(t["fused"])), 4),
            "fused_faster_beyond_both_spreads": bool(max(t["fused"]) < min(t["composed"])),
            "results_equal_bytes": len({c["sha256"][k] for a in arms for c in seen[a]}) == 1}
    out["rates"] = {"bins": bins, **_child(["--child", "rates", "--bins", str(bins), "--rounds", str(rounds)], timeout)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="16384,65536", help="output rows of the compress, 13 slots each")
    ap.add_argument("--bins", type=int, default=212992, help="(g, h) pairs of the per-bin rates")
    ap.add_argument("--rounds", type=int, default=3, help="readings of each arm or form, in turn")
    ap.add_argument("--reps", type=int, default=2, help="compress calls per reading")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=("fused", "composed", "rates"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sizes = [int(v) for v in a.rows.split(",")]
    if a.child == "rates":
        return rates_child(a.bins, a.rounds)
    if a.child:
        return compress_child(a.child, sizes, a.reps)
    line = json.dumps(run(sizes, a.bins, a.rounds, a.reps, a.timeout))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
