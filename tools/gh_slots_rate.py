"""Slot-packed histograms beside the two-ciphertext and pair-packed forms: bins / s, device-resident, Paillier-2048.

  python tools/gh_slots_rate.py [--n 500000] [--parties 8] [--slot-bits 224] [--timeout 300] [--out FILE]

One 8-party horizontal round, per histogram bin: a party's public-key encrypt, the server's 8-way merge, and
the full and short decrypt.  A bin is two ciphertexts in the reference flow, one in the pair-packed mode and
1 / slots of one in the slot-packed mode (include/fthe.h FTHE_GH_SLOT_*; 9 slots of 224 bits below a 2048-bit
n, 4 below p for the short decrypt), so every rate is in bins / s.  Then the compress (pair-packed ->
slot-packed on the ciphertext side) at slot_bits 224, 416 and 608.  Each step runs in a child process of its
own, under its own time limit, with the three forms measured in turn in that one process (medians of
alternating readings); the chain stops at the first step that fails.  Prints (and with --out writes) one
JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("encrypt_public", "merge", "decrypt", "compress")
COMPRESS_BITS = (224, 416, 608)


def _timed(dev, fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    dev.sync()
    return time.perf_counter() - t0


def step(name, n, parties, slot_bits, rounds, n_compress):
    import torch
    from fedtree_amd.paillier import Device, Paillier, decode_fixed, encode_fixed, gh_slot_rows
    dev = Device(0)
    pl = Paillier(dev).keygen(2048, seed=20261020)
    cw = 2 * pl.n_words
    slots, slots_short = pl.gh_slots(slot_bits), pl.gh_slots(slot_bits, short=True)
    rows, rows_short = gh_slot_rows(n, slots), gh_slot_rows(n, slots_short)
    rng = np.random.default_rng(1)
    g = rng.normal(0, 0.5, n).astype(np.float32)
    h = rng.uniform(1e-16, 0.25, n).astype(np.float32)
    gd, hd = torch.from_numpy(g).cuda(), torch.from_numpy(h).cuda()
    md = torch.from_numpy(np.concatenate([encode_fixed(g), encode_fixed(h)]).view(np.int64)).cuda()
    x2 = torch.empty((2 * n, cw), dtype=torch.int32, device="cuda")     # g plane, h plane
    xp = torch.empty((n, cw), dtype=torch.int32, device="cuda")         # pair-packed
    xs = torch.empty((rows, cw), dtype=torch.int32, device="cuda")      # slot-packed
    res = {"slots": slots, "slots_short": slots_short}

    def rate(key, forms, count=n):
        """forms: name -> callable; one untimed pass of each at full size, then the forms in turn, `rounds`
        times: the medians, and every reading for the spread."""
        for fn in forms.values():
            _timed(dev, fn)
        ts = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                ts[k].append(_timed(dev, fn))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        out = {f"{k}_bins_per_s": round(count / med[k]) for k in forms}
        out.update({f"{k}_s": [round(t, 4) for t in v] for k, v in ts.items()})
        first = next(iter(forms))
        out.update({f"{k}_over_{first}": round(med[first] / med[k], 3) for k in forms if k != first})
        res[key] = out

    if name == "encrypt_public":
        rate("encrypt_public", {
            "two_ct": lambda: pl.encrypt_u64_dev(md, x2, seed=2, public=True),
            "pair_packed": lambda: pl.encrypt_gh_packed_dev(gd, hd, xp, seed=2, public=True),
            "slotted": lambda: pl.encrypt_gh_slots_dev(gd, hd, xs, slot_bits, seed=2, public=True)})
        return res
    if name == "compress":
        m = min(n, n_compress)
        pl.encrypt_gh_packed_dev(gd[:m], hd[:m], xp[:m], seed=2)
        dev.sync()
        for sb in COMPRESS_BITS:
            s = pl.gh_slots(sb)
            out = torch.empty((gh_slot_rows(m, s), cw), dtype=torch.int32, device="cuda")
            rate(f"compress_{sb}", {"compress": lambda: pl.compress_gh_slots_dev(xp[:m], m, sb, out)}, count=m)
            res[f"compress_{sb}"].update(slots=s, inputs=m, montmuls_per_bin=round(dev.last_montmuls() / m, 1))
        return res
    # the inputs of the merge and of the decrypt: the key holder's CRT encrypt (the rows do not depend on the form)
    pl.encrypt_u64_dev(md, x2, seed=2)
    pl.encrypt_gh_packed_dev(gd, hd, xp, seed=2)
    pl.encrypt_gh_slots_dev(gd, hd, xs, slot_bits, seed=2)
    dev.sync()
    if name == "merge":
        # eight parties' histograms: the same rows in another order per party (a product does not care)
        k2 = torch.cat([x2.roll(k, 0) for k in range(parties)])
        kp = torch.cat([xp.roll(k, 0) for k in range(parties)])
        ks = torch.cat([xs.roll(k, 0) for k in range(parties)])
        o2, op, os_ = torch.empty_like(x2), torch.empty_like(xp), torch.empty_like(xs)
        rate("merge", {"two_ct": lambda: pl.reduce_kway_dev(k2, parties, o2),
                       "pair_packed": lambda: pl.reduce_kway_dev(kp, parties, op),
                       "slotted": lambda: pl.reduce_kway_dev(ks, parties, os_)})
        res["merge"].update(parties=parties)
        return res
    low = torch.empty(2 * n, dtype=torch.int64, device="cuda")
    dg = torch.empty(n, dtype=torch.float32, device="cuda")
    dh, sg, sh = torch.empty_like(dg), torch.empty_like(dg), torch.empty_like(dg)
    xss = torch.empty((rows_short, cw), dtype=torch.int32, device="cuda")      # built for the short decrypt
    pl.encrypt_gh_slots_dev(gd, hd, xss, slot_bits, seed=2, slots=slots_short)
    dev.sync()
    for short in (False, True):
        src, s = (xss, slots_short) if short else (xs, slots)
        rate("decrypt_short" if short else "decrypt_full", {
            "two_ct": lambda: pl.decrypt_u64_dev(x2, low, short=short),
            "pair_packed": lambda: pl.decrypt_gh_packed_dev(xp, dg, dh, short=short),
            "slotted": lambda: pl.decrypt_gh_slots_dev(src, n, slot_bits, sg, sh, short=short, slots=s)})
    lo = low.cpu().numpy().view(np.uint64)
    res["decoded_equal"] = bool(np.array_equal(decode_fixed(lo[:n]), sg.cpu().numpy())
                                and np.array_equal(decode_fixed(lo[n:]), sh.cpu().numpy())
                                and np.array_equal(dg.cpu().numpy(), sg.cpu().numpy())
                                and np.array_equal(dh.cpu().numpy(), sh.cpu().numpy()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000, help="histogram bins")
    ap.add_argument("--parties", type=int, default=8)
    ap.add_argument("--slot-bits", type=int, default=224)
    ap.add_argument("--n-compress", type=int, default=90_000, help="pair-packed ciphertexts per compress")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    ap.add_argument("--rounds", type=int, default=3, help="timed readings of each form, in turn")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.step:
        print("GH_SLOTS_STEP " + json.dumps(step(a.step, a.n, a.parties, a.slot_bits, a.rounds, a.n_compress)),
              flush=True)
        return 0
    res = {"tool": "gh_slots_rate", "key_bits": 2048, "bins": a.n, "slot_bits": a.slot_bits, "rounds": a.rounds,
           "status": "ok"}
    for s in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--n", str(a.n), "--parties", str(a.parties),
               "--slot-bits", str(a.slot_bits), "--rounds", str(a.rounds), "--n-compress", str(a.n_compress)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            rc, tail = r.returncode, (r.stdout + r.stderr)[-2000:]
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("GH_SLOTS_STEP ")]
        except subprocess.TimeoutExpired:
            rc, tail, lines = 124, f"{s}: no result within {a.timeout} s", []
        if rc != 0 or not lines:                        # nothing more runs on the GPU after a failed step
            res.update(status="failed", failed_step=s, rc=rc, tail=tail)
            break
        res.update(json.loads(lines[-1][len("GH_SLOTS_STEP "):]))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["status"] == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
