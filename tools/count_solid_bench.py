#!/usr/bin/env python3
"""Two-pass solid counting (Counter.set_sketch, `count --solid`) against plain counting over the same reads; prints one
JSON line.

Input: 64 MB of seeded synthetic FASTQ: reads of 100 nt from both strands of a seeded random genome of 1 Mb (about 30-fold
coverage), 1 % substitutions, 0.1 % N, qualities all 'I'.  Most distinct k-mers of such reads are errors seen once.  The
text goes through Counter.add_fastq in 8 MB blocks (lines and mask on the device).  Both counters start at the smallest
table and grow as they need to (expected_distinct = 1), so `slots` is what the input made of the table.  Timed are the
counting kernels alone, by HIP events on the counter's stream around every launch (KM_COUNT_TIME_FILTER=1): k_count_insert
of the plain counter, k_sketch_note (pass 1) and k_count_solid (pass 2) of the other; rehashing a grown table is in none
of them, `wall_ms` has everything from the first byte fed to the last statistic read.  One warm-up pass of each and then
--reps passes, taken in turn.  The sketch is sized for the number of distinct k-mers the plain counter found.

A table has room for every window of the piece that comes next (counter_reserve), so with the default staging buffers
of 16 MiB no table that has taken such a piece is smaller than 2^25 slots, whatever it holds; --stage-mb 1 makes the
pieces small enough for the keys to set the size.

Fields: plain / solid: kernel_ms (best; solid: pass 1 + pass 2), kernel_ms_median, kernel_ms_all, wall_ms (best), slots,
n_grow, distinct (keys in the table); solid also note_ms, count_ms (of the best pass), note_ms_all, count_ms_all (of
every pass), sketch_words, sketch_bits_1, sketch_bits_2; kmers_solid (records after the cut at 2: equal for both, asserted, as are the records themselves),
kmers_singleton (distinct k-mers seen once), kmers_admitted (keys the solid counter's table held), false_positives
(admitted - solid).

usage: count_solid_bench.py [--device 0] [-k 31] [--reps 5] [--mb 64] [--stage-mb 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["KM_COUNT_TIME_FILTER"] = "1"
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


def feed(c, text):
    pos, tail = 0, None
    while pos < text.size:
        buf = text[pos:pos + BLOCK]
        pos += BLOCK
        if tail is not None and tail.size:
            buf = np.concatenate([tail, buf])
        used = c.add_fastq(buf, final=False)
        tail = buf[used:]
    c.add_fastq(tail, final=True)


def one_pass(k, device, text, sketch_words, want_records):
    """-> dict of one counter's figures; sketch_words None: the plain counter."""
    c = kmlib.Counter(k=k, device=device, expected_distinct=1)
    try:
        t0 = time.perf_counter()
        if sketch_words is not None:
            c.set_sketch(sketch_words)
            feed(c, text)
            c.sketch_done()
        feed(c, text)
        st = c.stats()
        if sketch_words is None:
            out = {"kernel_ms": c.filter_stats()["kernel_ms"]}
        else:
            ss = c.sketch_stats()
            out = {"kernel_ms": ss["note_ms"] + ss["count_ms"], "note_ms": ss["note_ms"], "count_ms": ss["count_ms"],
                   "sketch_words": ss["words"], "sketch_bits_1": ss["bits_1"], "sketch_bits_2": ss["bits_2"]}
        out["wall_ms"] = (time.perf_counter() - t0) * 1e3
        out.update(slots=st["slots"], n_grow=st["n_grow"], distinct=st["distinct"], kmers=st["kmers"])
        c.finish(2).close()
        out["kmers_solid"] = c.n_records()
        if want_records:
            keys, counts = c.records()
            order = np.argsort(keys, kind="stable")
            out["records"] = (keys[order], counts[order])
    finally:
        c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mb", type=int, default=64)
    ap.add_argument("--stage-mb", type=float, default=16.0)
    args = ap.parse_args()
    os.environ["KM_COUNT_STAGE_BYTES"] = str(int(args.stage_mb * (1 << 20)))
    kmlib.load()
    rng = np.random.default_rng(2028)
    genome = ACGT[rng.integers(0, 4, 1_000_000)]
    text = make_text(rng, genome, (args.mb << 20) // 207)
    runs = {"plain": [], "solid": []}
    words = None
    for rep in range(args.reps + 1):
        last = rep == args.reps
        plain = one_pass(args.k, args.device, text, None, last)
        words = kmlib.sketch_words(plain["distinct"])
        solid = one_pass(args.k, args.device, text, words, last)
        if rep:                                          # (pass 0 warms: code object, allocations, clocks)
            runs["plain"].append(plain)
            runs["solid"].append(solid)
    a, b = plain.pop("records"), solid.pop("records")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "the records after the cut at 2 differ"
    assert plain["kmers_solid"] == solid["kmers_solid"] and plain["kmers"] == solid["kmers"]
    out = {"tool": "count_solid_bench", "k": args.k, "text_bytes": int(text.size), "reps": args.reps,
           "stage_bytes": int(os.environ["KM_COUNT_STAGE_BYTES"]), "kmers": plain["kmers"],
           "kmers_solid": plain["kmers_solid"], "kmers_singleton": plain["distinct"] - plain["kmers_solid"],
           "kmers_admitted": solid["distinct"], "false_positives": solid["distinct"] - solid["kmers_solid"]}
    for name, rows in runs.items():
        best = min(rows, key=lambda r: r["kernel_ms"])
        ms = [r["kernel_ms"] for r in rows]
        out[name] = {"kernel_ms": best["kernel_ms"], "kernel_ms_median": float(np.median(ms)), "kernel_ms_all": ms,
                     "wall_ms": min(r["wall_ms"] for r in rows), "slots": best["slots"], "n_grow": best["n_grow"],
                     "distinct": best["distinct"]}
        if name == "solid":
            out[name].update({key: best[key] for key in ("note_ms", "count_ms", "sketch_words", "sketch_bits_1",
                                                         "sketch_bits_2")})
            out[name].update(note_ms_all=[r["note_ms"] for r in rows], count_ms_all=[r["count_ms"] for r in rows])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
