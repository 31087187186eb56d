"""Packed gradient pairs beside the two-ciphertext flow: pairs / s, device-resident, Paillier-2048.

  python tools/gh_packed_rate.py [--n 1000000] [--cols 28] [--timeout 240] [--out FILE]

One (g, h) pair is two ciphertexts in the reference flow and one in the packed mode (include/fthe.h
FTHE_GH_*), so every rate is in pairs / s: CRT encrypt, histogram_dev of one node (cols features x 255
bins), the sibling subtraction (exponent 2^64 - 1 on 2n rows, 2^192 - 1 on n rows) and the full and short
decrypt.  Each operation runs in a child process of its own, under its own time limit, with both flows
measured in that one process; the chain stops at the first step that fails.  Prints (and with --out
writes) one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("encrypt", "histogram", "sibling_sub", "decrypt")


def _timed(dev, fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    dev.sync()
    return time.perf_counter() - t0


def step(name, n, cols, rounds):
    import torch
    from fedtree_amd.paillier import Device, Paillier, encode_fixed
    dev = Device(0)
    pl = Paillier(dev).keygen(2048, seed=20261015)
    cw = 2 * pl.n_words
    rng = np.random.default_rng(1)
    g = rng.normal(0, 0.5, n).astype(np.float32)
    h = rng.uniform(1e-16, 0.25, n).astype(np.float32)
    gd, hd = torch.from_numpy(g).cuda(), torch.from_numpy(h).cuda()
    md = torch.from_numpy(np.concatenate([encode_fixed(g), encode_fixed(h)]).view(np.int64)).cuda()
    x = torch.empty((2 * n, cw), dtype=torch.int32, device="cuda")      # g plane, h plane
    xp = torch.empty((n, cw), dtype=torch.int32, device="cuda")         # packed
    w = min(n, 4096)                                                    # warm-up size: buffers, programs
    res = {}

    def rate(key, unpacked, packed):
        # one untimed pass of each at full size (the slot regions and chunk buffers grow with the batch), then
        # the two flows in turn, `rounds` times: the medians, and every reading for the spread
        _timed(dev, unpacked), _timed(dev, packed)
        tus, tps = [], []
        for _ in range(rounds):
            tus.append(_timed(dev, unpacked))
            tps.append(_timed(dev, packed))
        tu, tp = float(np.median(tus)), float(np.median(tps))
        res[key] = {"unpacked_pairs_per_s": round(n / tu), "packed_pairs_per_s": round(n / tp),
                    "unpacked_s": [round(t, 4) for t in tus], "packed_s": [round(t, 4) for t in tps],
                    "packed_over_unpacked": round(tu / tp, 3)}

    pl.encrypt_u64_dev(md[:w], x[:w], seed=2)
    pl.encrypt_gh_packed_dev(gd[:w], hd[:w], xp[:w], seed=2)
    dev.sync()
    rate("encrypt_crt", lambda: pl.encrypt_u64_dev(md, x, seed=2),
         lambda: pl.encrypt_gh_packed_dev(gd, hd, xp, seed=2))
    if name == "encrypt":
        # the six-word 1 + m n beside the 64-bit one, on the same number of ciphertexts
        rate("encrypt_crt_same_count", lambda: pl.encrypt_u64_dev(md[:n], x[:n], seed=2),
             lambda: pl.encrypt_gh_packed_dev(gd, hd, xp, seed=2))
        e = res.pop("encrypt_crt_same_count")
        res["encrypt_crt"].update(u64_ciphertexts_per_s=e["unpacked_pairs_per_s"],
                                  packed_ciphertexts_per_s=e["packed_pairs_per_s"],
                                  packed_over_u64_per_ciphertext=e["packed_over_unpacked"])
        return res
    del res["encrypt_crt"]                                              # here the encrypt only made the inputs
    if name == "histogram":
        gen = torch.Generator(device="cuda").manual_seed(1)
        bins = torch.randint(0, 256, (n, cols), dtype=torch.uint8, device="cuda", generator=gen)
        cut = (np.arange(cols + 1) * 255).astype(np.int32)
        nb = int(cut[-1])
        out = torch.empty((2 * nb, cw), dtype=torch.int32, device="cuda")
        pl.histogram_dev(x[:2 * w], w, 2, bins[:w], cut, 255, out)
        pl.histogram_dev(xp[:w], w, 1, bins[:w], cut, 255, out)
        dev.sync()
        rate("histogram_dev", lambda: pl.histogram_dev(x, n, 2, bins, cut, 255, out),
             lambda: pl.histogram_dev(xp, n, 1, bins, cut, 255, out))
        res["histogram_dev"].update(features=cols, bins=nb)
    elif name == "sibling_sub":
        out = torch.empty_like(x)
        pl.sub_dev(x[:w], x[w:2 * w], out[:w])
        pl.sub_bits_dev(xp[:w], xp[w:2 * w], out[:w])
        dev.sync()
        # father - computed over as many bins as pairs: b is the a rows in another order
        xb, xpb = x.roll(1, 0), xp.roll(1, 0)
        rate("sibling_sub", lambda: pl.sub_dev(x, xb, out), lambda: pl.sub_bits_dev(xp, xpb, out[:n]))
    elif name == "decrypt":
        low = torch.empty(2 * n, dtype=torch.int64, device="cuda")
        dg = torch.empty(n, dtype=torch.float32, device="cuda")
        dh = torch.empty_like(dg)
        for short in (False, True):
            pl.decrypt_u64_dev(x[:w], low[:w], short=short)
            pl.decrypt_gh_packed_dev(xp[:w], dg[:w], dh[:w], short=short)
            dev.sync()
            rate("decrypt_short" if short else "decrypt_full",
                 lambda: pl.decrypt_u64_dev(x, low, short=short),
                 lambda: pl.decrypt_gh_packed_dev(xp, dg, dh, short=short))
        # the packed decode agrees with the two-ciphertext one on this batch
        from fedtree_amd.paillier import decode_fixed
        lo = low.cpu().numpy().view(np.uint64)
        res["decoded_equal"] = bool(np.array_equal(decode_fixed(lo[:n]), dg.cpu().numpy())
                                    and np.array_equal(decode_fixed(lo[n:]), dh.cpu().numpy()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=28)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--rounds", type=int, default=3, help="timed readings of each flow, in turn")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.step:
        print("GH_PACKED_STEP " + json.dumps(step(a.step, a.n, a.cols, a.rounds)), flush=True)
        return 0
    res = {"tool": "gh_packed_rate", "key_bits": 2048, "pairs": a.n, "rounds": a.rounds, "status": "ok"}
    for s in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--n", str(a.n), "--cols", str(a.cols),
               "--rounds", str(a.rounds)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            rc, tail = r.returncode, (r.stdout + r.stderr)[-2000:]
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("GH_PACKED_STEP ")]
        except subprocess.TimeoutExpired:
            rc, tail, lines = 124, f"{s}: no result within {a.timeout} s", []
        if rc != 0 or not lines:                        # nothing more runs on the GPU after a failed step
            res.update(status="failed", failed_step=s, rc=rc, tail=tail)
            break
        res.update(json.loads(lines[-1][len("GH_PACKED_STEP "):]))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["status"] == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
