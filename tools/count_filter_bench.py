#!/usr/bin/env python3
"""Filtered counting (Counter.set_filter, `count --if`) against full counting over the same text; prints one JSON line.

Input: 64 MB of seeded synthetic FASTQ: reads of 100 nt from both strands of a seeded random genome of 10 Mb, 1 %
substitutions, 0.1 % N, qualities all 'I'.  The text goes through Counter.add_fastq in 8 MB blocks (lines and mask on the
device), so the counting kernel streams every byte of it.  Timed is the counting kernel alone, by HIP events on the
counter's stream around every launch of it (KM_COUNT_TIME_FILTER=1, Counter.filter_stats()["kernel_ms"]); GB/s is the
text's bytes over that time.  Four configurations, one warm-up pass of each and then --reps passes, taken in turn
within a pass so that none has the device to itself for long:
  unfiltered   - k_count_insert into a table sized in advance (no growth), the kernel of the plain km_counter
  lds          - the filter holds lds_keys (4096) k-mers of the genome: the LDS tier
  hbm_same     - the same set with KM_COUNT_FILTER_LDS=0: the HBM tier
  hbm_1m       - the k-mers of 1 M windows of the genome: the HBM tier at a table of 32 MB
Per configuration: kernel_ms (best), kernel_ms_median, kernel_ms_all, GBs (from the best), kmers_hit, table_slots.
lds and hbm_same must count the same (asserted).  `lds_faster_beyond_spread` is true when every lds pass is faster than
every hbm_same pass.

usage: count_filter_bench.py [--device 0] [-k 31] [--reps 7] [--mb 64]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["KM_COUNT_TIME_FILTER"] = "1"
from km_amd import kmer as km  # noqa: E402
from km_amd import lib as kmlib  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")
BLOCK = 8 << 20


def make_text(rng, genome, n_reads, read_len=100):
    """4-line FASTQ of n_reads reads as one uint8 array."""
    starts = rng.integers(0, genome.size - read_len + 1, n_reads)
    reads = genome[starts[:, None] + np.arange(read_len)[None, :]]
    rev = rng.integers(0, 2, n_reads).astype(bool)
    reads[rev] = COMP[reads[rev]][:, ::-1]
    sub = rng.random(reads.shape) < 0.01
    reads[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
    reads[rng.random(reads.shape) < 0.001] = ord("N")
    rows = np.empty((n_reads, 3 + read_len + 3 + read_len + 1), np.uint8)
    rows[:, :3] = np.frombuffer(b"@r\n", np.uint8)
    rows[:, 3:3 + read_len] = reads
    rows[:, 3 + read_len:6 + read_len] = np.frombuffer(b"\n+\n", np.uint8)
    rows[:, 6 + read_len:6 + 2 * read_len] = ord("I")
    rows[:, -1] = ord("\n")
    return rows.reshape(-1)


def genome_keys(genome, k, n):
    """The canonical k-mers of the first windows of the genome, n distinct ones."""
    codes = km.encode(genome[:n + n // 8 + k].tobytes())
    keys = np.unique(km.canonical(km.sliding_kmers(codes, k), k))
    assert keys.size >= n
    return np.ascontiguousarray(keys[:n])


def one_pass(k, device, text, keys, force_hbm, expected_distinct):
    if force_hbm:
        os.environ["KM_COUNT_FILTER_LDS"] = "0"
    else:
        os.environ.pop("KM_COUNT_FILTER_LDS", None)
    c = kmlib.Counter(k=k, device=device, expected_distinct=expected_distinct)
    try:
        if keys is not None:
            c.set_filter(keys)
        pos, tail = 0, None
        while pos < text.size:
            buf = text[pos:pos + BLOCK]
            pos += BLOCK
            if tail is not None and tail.size:
                buf = np.concatenate([tail, buf])
            used = c.add_fastq(buf, final=False)
            tail = buf[used:]
        c.add_fastq(tail, final=True)
        fs, st = c.filter_stats(), c.stats()
    finally:
        c.close()
        os.environ.pop("KM_COUNT_FILTER_LDS", None)
    return fs, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mb", type=int, default=64)
    args = ap.parse_args()
    kmlib.load()
    rng = np.random.default_rng(2027)
    genome = ACGT[rng.integers(0, 4, 10_000_000)]
    text = make_text(rng, genome, (args.mb << 20) // 207)
    probe = kmlib.Counter(k=args.k, device=args.device, expected_distinct=1)
    lds_keys = probe.filter_stats()["lds_keys"]
    probe.close()
    small, large = genome_keys(genome, args.k, lds_keys), genome_keys(genome, args.k, 1_000_000)
    configs = {                                          # name: (filter keys, force the HBM tier, expected_distinct)
        "unfiltered": (None, False, int(text.size)),          # (every byte a new key: counter_reserve never grows it)
        "lds": (small, False, 1),
        "hbm_same": (small, True, 1),
        "hbm_1m": (large, True, 1),
    }
    ms = {name: [] for name in configs}
    last = {}
    for rep in range(args.reps + 1):
        for name, (keys, force_hbm, expected) in configs.items():
            fs, st = one_pass(args.k, args.device, text, keys, force_hbm, expected)
            if rep:                                      # (pass 0 warms: code object, allocations, clocks)
                ms[name].append(fs["kernel_ms"])
            last[name] = (fs, st)
    assert last["lds"][0]["tier"] == "lds" and last["hbm_same"][0]["tier"] == last["hbm_1m"][0]["tier"] == "hbm"
    assert last["lds"][0]["kmers_hit"] == last["hbm_same"][0]["kmers_hit"]
    assert len({st["kmers"] for _, st in last.values()}) == 1 and last["unfiltered"][1]["n_grow"] == 0
    out = {"tool": "count_filter_bench", "k": args.k, "text_bytes": int(text.size), "reps": args.reps,
           "lds_keys": lds_keys, "kmers": last["lds"][1]["kmers"], "configs": {}}
    for name in configs:
        fs, st = last[name]
        best = min(ms[name])
        out["configs"][name] = {
            "kernel_ms": best, "kernel_ms_median": float(np.median(ms[name])), "kernel_ms_all": ms[name],
            "GBs": text.size / (best * 1e-3) / 1e9, "kmers_hit": fs["kmers_hit"], "filter_kmers": fs["n_keys"],
            "tier": fs["tier"], "table_slots": st["slots"]}
    out["lds_faster_beyond_spread"] = max(ms["lds"]) < min(ms["hbm_same"])
    out["km_device_copy_GBs"] = kmlib.device_copy_GBs(args.device, 1 << 30, 10)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
