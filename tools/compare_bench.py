#!/usr/bin/env python3
"""`compare` (Counter.mark_jf, Counter.cooccurrence) against the kernels it is built beside; prints one JSON line.

Input: --inputs (32) synthetic files of --keys (2^20) records each, k = 31, twelve-byte records, drawn without
replacement from one seeded pool of --pool (2^21) random keys, so every pair of inputs overlaps heavily (about half of
either) and the union is the pool.  The files are written once to a temporary directory (--dir, default /dev/shm when it
exists).  Everything runs in one process; all times are kernel times by HIP events on the counter's stream
(KM_COUNT_TIME_MERGE=1), a warm-up pass and then --reps passes, best / median / all reported:
  mark        - k_mark_records over the 32 files (Counter.mark_jf), table sized in advance: ns per record
  sum         - k_count_add_records (sum) over the same files into a table of the same size (Counter.add_jf)
  cooc        - k_cooc_table over the table the 32 inputs left; cooc_by_n: the same pass after 1, 2, 8, 16 inputs
                (the same table size, fewer ballots and pairs)
  histo       - k_histo_table over the sum counter's table: the same slots, the same bytes streamed
With --loop also the wall time of the loop `compare` replaces, over the five fixture tables of tests/data/jf, every
command a process of its own: one `compare` against ten `merge --min` each followed by `stats`.

usage: compare_bench.py [--device 0] [--inputs 32] [--keys 1048576] [--pool 2097152] [--reps 5] [--dir DIR] [--loop]
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["KM_COUNT_TIME_MERGE"] = "1"
from km_amd import count as kc  # noqa: E402
from km_amd import lib as kmlib  # noqa: E402

STEPS = (1, 2, 8, 16)


def summary(values):
    return {"best": min(values), "median": statistics.median(values), "all": [round(v, 4) for v in values]}


def mark_pass(paths, size, device):
    c = kmlib.Counter(k=31, device=device, expected_distinct=size)
    try:
        by_n, seen = {}, 0.0
        for i, p in enumerate(paths):
            c.mark_jf(p)
            if i + 1 in STEPS and i + 1 < len(paths):
                ms = c.cooccurrence()["kernel_ms"]
                by_n[i + 1], seen = ms - seen, ms
        result = c.cooccurrence()
        merged, stats = c.merge_stats(), c.stats()
        return {"mark_ms": merged["kernel_ms"], "records_in": merged["records_in"], "cooc_ms": result["kernel_ms"] - seen,
                "by_n": by_n, "slots": stats["slots"], "n_grow": stats["n_grow"], "union": result["union"],
                "core": int(result["in_exactly"][-1]), "shared_0_1": int(result["shared"][1][0]) if len(paths) > 1 else 0}
    finally:
        c.close()


def sum_pass(paths, size, device):
    c = kmlib.Counter(k=31, device=device, expected_distinct=size)
    try:
        for p in paths:
            c.add_jf(p)
        merged, stats = c.merge_stats(), c.stats()
        _, _, hs = c.histo()
        return {"sum_ms": merged["kernel_ms"], "histo_ms": kmlib.histo_kernel_ms(), "slots": stats["slots"],
                "distinct": hs["distinct"]}
    finally:
        c.close()


def loop_wall(device):
    """One `compare` over the five fixture tables against ten `merge --min` + `stats`, every command a fresh process."""
    jf_dir = os.path.join(ROOT, "tests", "data", "jf")
    names = sorted(f for f in os.listdir(jf_dir) if f.endswith(".jf"))
    paths = [os.path.join(jf_dir, f) for f in names]
    env = dict(os.environ, PYTHONPATH=ROOT, KM_DEVICE=str(device))
    env.pop("KM_COUNT_TIME_MERGE", None)
    work = tempfile.mkdtemp(prefix="compare_loop_")

    def run(*args):
        subprocess.run([sys.executable, "-m", "km_amd"] + list(args), check=True, env=env, cwd=work, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
    try:
        t0 = time.perf_counter()
        run("compare", "-o", "pairs.tsv", *paths)
        t1 = time.perf_counter()
        for i in range(len(paths)):
            for j in range(i + 1, len(paths)):
                run("merge", "--min", "-o", "m.jf", paths[i], paths[j])
                run("stats", "-o", "s.txt", "m.jf")
        t2 = time.perf_counter()
        t3 = time.perf_counter()
        kc.compare_files(paths, device=device)
        t4 = time.perf_counter()
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return {"files": len(paths), "compare_process_s": t1 - t0, "merge_min_stats_20_processes_s": t2 - t1,
            "compare_files_in_process_s": t4 - t3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--inputs", type=int, default=32)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--pool", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--loop", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    pool = np.unique(rng.integers(0, 1 << 62, args.pool + args.pool // 64, dtype=np.uint64))[:args.pool]
    assert pool.size == args.pool >= args.keys
    work = tempfile.mkdtemp(prefix="compare_bench_", dir=args.dir)
    try:
        paths = []
        for i in range(args.inputs):
            keys = rng.choice(pool, args.keys, replace=False)
            paths.append(os.path.join(work, "in%02d.jf" % i))
            kc.write_records(paths[-1], keys, rng.integers(1, 200, keys.size).astype(np.uint32), 31, True)
        marks, sums = [], []
        for rep in range(args.reps + 1):                                # (pass 0 warms up)
            # (sized for the pool plus one more file of new keys, the worst case counter_reserve reckons with: no growth)
            size = args.pool + args.keys
            m, s = mark_pass(paths, size, args.device), sum_pass(paths, size, args.device)
            if rep:
                marks.append(m)
                sums.append(s)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    first = marks[0]
    assert first["slots"] == sums[0]["slots"] and first["union"] == sums[0]["distinct"], (first, sums[0])
    records = first["records_in"]
    out = {"tool": "compare_bench", "library": kmlib.LIB_PATH, "inputs": args.inputs, "keys_per_input": args.keys,
           "pool": args.pool, "records": records, "slots": first["slots"], "table_MiB": first["slots"] * 16 / 2 ** 20,
           "n_grow": first["n_grow"], "union": first["union"], "core": first["core"], "shared_0_1": first["shared_0_1"], "reps": args.reps,
           "mark_ms": summary([m["mark_ms"] for m in marks]), "sum_ms": summary([s["sum_ms"] for s in sums]),
           "cooc_ms": summary([m["cooc_ms"] for m in marks]), "histo_ms": summary([s["histo_ms"] for s in sums]),
           "cooc_ms_by_n": {str(n): min(m["by_n"][n] for m in marks) for n in STEPS if n in first["by_n"]}}
    out["mark_ns_per_record"] = out["mark_ms"]["best"] * 1e6 / records
    out["sum_ns_per_record"] = out["sum_ms"]["best"] * 1e6 / records
    out["cooc_GBs"] = first["slots"] * 16 / out["cooc_ms"]["best"] / 1e6
    out["histo_GBs"] = first["slots"] * 16 / out["histo_ms"]["best"] / 1e6
    if args.loop:
        out["loop"] = loop_wall(args.device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
