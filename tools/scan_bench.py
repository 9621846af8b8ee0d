#!/usr/bin/env python3
"""The scan (Database.cov_seqs / scan_text: k-mers of sequences cut and looked up on the GPU) against the route it
replaces, where the k-mers are cut on the host; prints one JSON line.

Input: seeded random bases, no N, in three shapes: `1m` (one sequence of 1 M bases), `64m` (one of 64 M) and `100k`
(100 000 sequences of 200 bases), each against a canonical table built from a tenth of the shape's distinct k-mers
(seeded counts 1..1000).  Per shape, wall time around the whole call (packing the sequences included), best and all of
--reps runs:
  cov_seqs    Database.cov_seqs of the sequences: seconds, windows/s, and the time of the scan kernels by HIP events
              (km_scan_kernel_ms)
  scan_text   Database.scan_text of the sequences to /dev/null: seconds, windows/s, bytes_out, pieces, the time of the
              scan kernels and of the text kernels (km_dump_kernel_ms)
  host_cov    the route of the commit before the scan: count._windows per sequence (k numpy passes over 8-byte
              windows) + canonical minimum, Database.query of all keys, then total / min / max / zeros per sequence
              with numpy (reduceat)
  host_text   the same keys through Database.query_text to /dev/null
and the ratios host / device of the best times.  The two routes must agree: the sums of the statistics are compared,
and bytes_out of both texts.  --host-max-bases skips the host route of shapes above that many bases (it needs about
40 bytes of host memory per base).

usage: scan_bench.py [--device 0] [--shapes 1m,64m,100k] [-k 31] [--reps 3] [--host-max-bases N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from km_amd import count as kc  # noqa: E402
from km_amd import kmer as km  # noqa: E402
from km_amd import lib as kmlib  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
SHAPES = {"1m": (1, 1_000_000), "64m": (1, 64_000_000), "100k": (100_000, 200)}      # sequences, bases each


def host_keys(seqs, k):
    """What query_keys does for the records of its files: the canonical key of every window, sequence after sequence."""
    keys = np.concatenate([kc._windows(s, k) for s in seqs])
    return np.minimum(keys, km.revcomp(keys, k))


def host_cov(db, seqs, k):
    keys = host_keys(seqs, k)
    counts = db.query(keys).astype(np.uint64)
    sizes = np.array([max(0, s.size - k + 1) for s in seqs])
    at = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    return {"total": np.add.reduceat(counts, at), "min": np.minimum.reduceat(counts, at),
            "max": np.maximum.reduceat(counts, at), "n_zero": np.add.reduceat((counts == 0).astype(np.uint64), at),
            "n_kmers": sizes}


def best_all(prefix, values):
    return {prefix: min(values), prefix + "_all": values}


def run_shape(name, k, device, rng, reps, host_max):
    n_seqs, length = SHAPES[name]
    flat = ACGT[rng.integers(0, 4, n_seqs * length)]
    seqs = [flat[i * length:(i + 1) * length] for i in range(n_seqs)]
    windows = n_seqs * (length - k + 1)
    with_host = n_seqs * length <= host_max
    # the table: a tenth of the distinct k-mers (from the device's own text when the host route is skipped)
    null = open(os.devnull, "wb")
    distinct = np.unique(host_keys(seqs, k)) if with_host else np.unique(host_keys(seqs[:1], k)[: 8_000_000])
    keys = distinct[::10]
    db = kmlib.Database.from_records(keys, rng.integers(1, 1001, keys.size).astype(np.uint32), k, True).upload(device)
    out = {"sequences": n_seqs, "bases": n_seqs * length, "windows": windows, "table_records": int(keys.size)}
    try:
        db.cov_seqs(seqs[:1])                                 # code object load, first allocations
        cov_s, cov_ms, text_s, text_scan_ms, text_dump_ms = [], [], [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            cov = db.cov_seqs(seqs)
            cov_s.append(time.perf_counter() - t0)
            cov_ms.append(kmlib.scan_kernel_ms())
            t0 = time.perf_counter()
            st = db.scan_text(seqs, null)
            text_s.append(time.perf_counter() - t0)
            text_scan_ms.append(kmlib.scan_kernel_ms())
            text_dump_ms.append(kmlib.dump_kernel_ms())
        assert int(cov["n_kmers"].sum()) == windows == st["records_in"] == st["records_out"]
        out.update({**best_all("cov_seqs_s", cov_s), **best_all("cov_seqs_kernel_ms", cov_ms),
                    "cov_seqs_windows_per_s": windows / min(cov_s),
                    **best_all("scan_text_s", text_s), **best_all("scan_text_scan_kernel_ms", text_scan_ms),
                    **best_all("scan_text_dump_kernel_ms", text_dump_ms), "scan_text_windows_per_s": windows / min(text_s),
                    "scan_text_bytes_out": st["bytes_out"], "scan_text_pieces": st["pieces"],
                    "total": int(cov["total"].sum()), "n_zero": int(cov["n_zero"].sum())})
        if with_host:
            host_cov_s, host_text_s = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                ref = host_cov(db, seqs, k)
                host_cov_s.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                st_host = db.query_text(host_keys(seqs, k), null)
                host_text_s.append(time.perf_counter() - t0)
            for field in ("total", "min", "max", "n_zero", "n_kmers"):
                assert np.array_equal(ref[field].astype(np.uint64), cov[field].astype(np.uint64)), field
            assert st_host["bytes_out"] == st["bytes_out"]
            out.update({**best_all("host_cov_s", host_cov_s), **best_all("host_text_s", host_text_s),
                        "host_cov_windows_per_s": windows / min(host_cov_s),
                        "cov_host_over_device": min(host_cov_s) / min(cov_s),
                        "text_host_over_device": min(host_text_s) / min(text_s)})
    finally:
        db.close()
        null.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--shapes", default="1m,64m,100k")
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-max-bases", type=int, default=1 << 40)
    args = ap.parse_args()
    kmlib.load()
    rng = np.random.default_rng(2026)
    out = {"tool": "scan_bench", "k": args.k, "reps": args.reps, "shapes": {}}
    for name in args.shapes.split(","):
        out["shapes"][name] = run_shape(name, args.k, args.device, rng, args.reps, args.host_max_bases)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
