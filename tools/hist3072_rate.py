"""Paillier-3072 segmented products on fthe_gprod192: segments / s, device-resident.

  python tools/hist3072_rate.py [--segments 262144] [--instances 65536] [--features 28] [--rounds 5] [--reps 100] [--out FILE]

Two arms in one process on a seeded 3072-bit odd n (a public key; the product needs no factorisation), both over the
same `segments` x 8 gathered members of 8 x `segments` random rows:
  fused     fthe_reduce_segments_csr_dev: the planner's kernels and one launch of fthe_gprod192;
  composed  the yardstick from the public interface alone: eight index_select gathers into planes, then
            fthe_reduce_kway_dev, seven launches of fthe_mul192.
One untimed pass of each, then `rounds` readings of each in turn, a reading being `reps` calls queued back to back
under a host clock that ends in a device synchronise (seconds are per call); medians, and every reading for the spread.
The first 64 segments of each arm are checked against Python's integers.  Then one node histogram, fthe_histogram_dev
over 2 planes of `instances` rows and `features` features of 32 bins (every cell populated), timed the same way (half
the calls per reading) and checked in its first bins.  The record also holds what the compiler reports for both kernels
of fthe_mul192.hip (registers, LDS, scratch, spills, occupancy), from a compile of that file by this tool.  Prints (and
with --out writes) one JSON line."""
import argparse
import json
import os
import random
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CW, K, BINS = 192, 8, 32


def _compiled():
    """kernel name -> the resource report of hipcc -O3 for gfx950 (the flags of fedtree_amd/build.py)"""
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-idirafter",
                            "/opt/conda/include", "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(ROOT, "fedtree_amd", "csrc", "fthe_mul192.hip"), "-o", os.path.join(tmp, "k.o")],
                           capture_output=True, text=True, check=True)
    out, name = {}, None
    for key, val in re.findall(r"remark:\s+([A-Za-z /\[\]]+): (\S+)", r.stderr):
        if key == "Function Name":
            name = re.search(r"fthe_\w+?_kernel", val).group(0)
            out[name] = {}
        elif key.split(" [")[0] in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "Occupancy",
                                     "LDS Size"):
            out[name][key] = int(val)
    return out


def _timed(dev, fn, reps=1):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dev.sync()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def _ints(t):
    a = np.ascontiguousarray(t.cpu().numpy()).view(np.uint8).reshape(len(t), -1)
    return [int.from_bytes(r.tobytes(), "little") for r in a]


def _prod(N, vals):
    p = 1
    for v in vals:
        p = p * v % N
    return p


def run(segments, instances, features, rounds, reps):
    import torch
    from fedtree_amd.paillier import Device, Paillier
    dev = Device(0)
    pl = Paillier.from_public(random.Random(3072).getrandbits(3072) | (1 << 3071) | 1, dev)
    N = pl.n2
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda *shape: torch.randint(-2**31, 2**31, shape, dtype=torch.int32, device="cuda", generator=g)
    x = rand(K * segments, CW)
    idx = torch.randperm(K * segments, device="cuda", generator=g)
    seg = torch.arange(segments + 1, device="cuda", dtype=torch.int64) * K
    members = idx.view(segments, K).t().contiguous()                 # members[j]: member j of every segment
    planes = torch.empty((K, segments, CW), dtype=torch.int32, device="cuda")
    out = {a: torch.empty((segments, CW), dtype=torch.int32, device="cuda") for a in ("fused", "composed")}

    def composed():
        for j in range(K):
            torch.index_select(x, 0, members[j], out=planes[j])
        pl.reduce_kway_dev(planes, K, out["composed"])

    # the node histogram: plane p, feature f, bin b <- the instances with bins[i, f] == b
    hx = x[:2 * instances]
    bins = torch.randint(0, BINS, (instances, features), dtype=torch.uint8, device="cuda", generator=g)
    cut = np.arange(features + 1, dtype=np.int32) * BINS
    hout = torch.empty((2 * features * BINS, CW), dtype=torch.int32, device="cuda")
    arms = {"fused": lambda: pl.reduce_segments_csr_dev(x, seg, out["fused"], idx=idx),
            "composed": composed,
            "histogram": lambda: pl.histogram_dev(hx, instances, 2, bins, cut, BINS, hout)}
    times = {a: [] for a in arms}
    products = {}
    for a, fn in arms.items():                           # one untimed pass at full size
        _timed(dev, fn)
        products[a] = dev.last_montmuls()
    for _ in range(rounds):
        for a, fn in arms.items():
            times[a].append(_timed(dev, fn, reps if a != "histogram" else max(1, reps // 2)))
    w = 64
    rows = _ints(x[idx[:K * w]])
    want = [_prod(N, rows[K * s:K * s + K]) for s in range(w)]
    b0 = bins[:, 0].cpu().numpy()
    hrows = _ints(hx[:instances])
    hwant = [_prod(N, [hrows[i] for i in np.nonzero(b0 == b)[0]]) for b in range(2)]
    med = {a: float(np.median(v)) for a, v in times.items()}
    spread = {a: round(max(v) / min(v), 4) for a, v in times.items()}
    return {"tool": "hist3072_rate",
            "command": f"python tools/hist3072_rate.py --segments {segments} --instances {instances} "
                       f"--features {features} --rounds {rounds} --reps {reps}",
            "key_bits": 3072, "kernel": "fthe_gprod192 (gathered 8-way product, running product resident in LDS)",
            "compiled": _compiled(),
            "segments": segments, "members_per_segment": K, "rounds": rounds, "calls_per_reading": reps,
            "seconds": {a: [round(t, 5) for t in v] for a, v in times.items()},
            "spread": spread, "products_per_call": products,
            "fused_segments_per_s": round(segments / med["fused"]),
            "composed_segments_per_s": round(segments / med["composed"]),
            "fused_products_per_s": round(segments * (K - 1) / med["fused"]),
            "fused_over_composed": round(med["composed"] / med["fused"], 4),
            "fused_not_slower_than_composed_beyond_its_spread": bool(med["fused"] <= med["composed"] * spread["composed"]),
            "histogram": {"planes": 2, "instances": instances, "features": features, "bins_per_feature": BINS,
                          "members": 2 * instances * features, "seconds_per_node": round(med["histogram"], 5),
                          "members_per_s": round(2 * instances * features / med["histogram"])},
            "results_equal_python": bool(_ints(out["fused"][:w]) == want and _ints(out["composed"][:w]) == want
                                         and _ints(hout[:2]) == hwant)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=1 << 18)
    ap.add_argument("--instances", type=int, default=1 << 16)
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--rounds", type=int, default=5, help="timed readings of each arm, in turn")
    ap.add_argument("--reps", type=int, default=100, help="calls per reading (the histogram: half of it); windows above a second")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = json.dumps(run(a.segments, a.instances, a.features, a.rounds, a.reps))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
