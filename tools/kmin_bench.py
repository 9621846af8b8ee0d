#!/usr/bin/env python3
"""km_linear_kmin (`km linear_kmin` for a catalog) on four catalog shapes; prints one JSON line.

Per shape: the wall time of the ABI call (host staging, copies, kernel, result copy, device buffers
allocated and freed inside the call), targets/s, and byte-pair comparisons/s, n(n-1)/2 per target.
Kernel time comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool.

usage: kmin_bench.py [--reps 5] [--device 0] [--shapes 500nt,5kb,100kb,mixed]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from km_amd import lib as kmlib  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)


def shape(name, rng):
    """(lengths, blob): random ACGT targets; 'mixed' is the size mix of tests/test_linear_kmin.py."""
    if name == "500nt":
        lens = [500] * 10_000
    elif name == "5kb":
        lens = [5_000] * 1_000
    elif name == "100kb":
        lens = [100_000] * 20
    elif name == "mixed":
        lens = [0, 1, 2, 3, 64, 65, 66, 127, 128, 129] + rng.choice([500, 1000, 5000, 20_000, 50_000], 40).tolist()
    else:
        raise ValueError(name)
    blob = ACGT[rng.integers(0, 4, sum(lens))]
    return np.array(lens, np.uint64), blob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--shapes", default="500nt,5kb,100kb,mixed")
    args = ap.parse_args()
    lib = kmlib.load()
    rng = np.random.default_rng(2026)
    out = {"tool": "kmin_bench", "reps": args.reps, "shapes": {}}
    for name in args.shapes.split(","):
        lens, blob = shape(name, rng)
        offs = np.zeros(lens.size + 1, np.uint64)
        np.cumsum(lens, out=offs[1:])
        kmin = np.zeros(lens.size, np.int32)
        rep = np.zeros(lens.size, np.int32)
        P = kmlib.ptr

        def call():
            kmlib.check(lib.km_linear_kmin(args.device, P(blob), P(offs), lens.size, 10, P(kmin), P(rep), None, None))

        call()                                   # warm-up: code object load, first allocations
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        pairs = float((lens.astype(np.float64) * (lens.astype(np.float64) - 1) / 2).sum())
        best, med = min(times), float(np.median(times))
        out["shapes"][name] = {
            "targets": int(lens.size), "bases": int(lens.sum()), "byte_pairs": pairs,
            "call_ms_median": med * 1e3, "call_ms_min": best * 1e3,
            "targets_per_s": lens.size / med, "byte_pairs_per_s": pairs / med,
            "R_median": float(np.median(rep)), "kmin_median": float(np.median(kmin)),
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
