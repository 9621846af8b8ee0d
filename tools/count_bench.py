#!/usr/bin/env python3
"""km_counter (counting k-mers from reads on the GPU) at two table sizes; prints one JSON line.

Input: seeded synthetic reads, 100 nt, drawn from both strands of a seeded random genome, 1 % substitutions and
0.1 % N.  Two sizes: `cache` (a 100 kb genome at 200x through 1 MiB staging buffers: the counting table stays at
134 MB, inside the 256 MB last-level cache) and `hbm` (a 100 Mb genome at 2x: a table of some GB).  Per size,
timed as wall time around calls that end in km_counter_stats (which waits for the device):
  add_bases  - pre-stripped bytes, table sized in advance (expected_distinct): k-mers/s, and the table traffic
               that stands for (8-byte key read + 4-byte add per k-mer, 8-byte compare-and-swap per new key)
  add_text   - the same reads as FASTQ text in 8 MB blocks, table grown from the default: bytes/s, n_grow
  add_fastq  - the same FASTQ text in the same blocks through Counter.add_fastq (lines, qualities and the mask on
               the device), with Q = 0 and with Q = '+': wall time, text bytes/s, k-mers/s, and the time of the
               line-table and mask kernels by HIP events on the counter's stream (KM_COUNT_TIME_FASTQ).  The
               qualities are seeded bytes in '!'..'I', 2 % of them below '+'.  add_text and the two add_fastq runs
               alternate --text-reps times within the run; best and all times are reported, the base of any
               comparison is add_text of the same run
  finish     - compaction + lookup-table build, seconds
  write_jf   - the kept records as a file in Jellyfish's own record order (Counter.write_jf: sorted on the device,
               drained through pinned staging), wall seconds, best and all of --write-reps runs; the time of its
               kernels alone (position, scan, scatter, sort; HIP events inside the call) and the bucket figures;
               and beside them the path it replaces for a key-sorted file: Counter.records() + write_records,
               which sorts with np.argsort (host_sorted_*).  Files go to /dev/shm if there is one, else to the temp directory.
  merge      - the two halves of the reads counted separately and written as two files (Counter.write_jf), then
               Counter.add_jf of both into a counter sized as merge_files sizes it: wall time to km_counter_stats,
               input records/s, the time of the record kernel by HIP events (KM_COUNT_TIME_MERGE), best and all of
               --write-reps runs; and beside it the host path a user has today: Database.open(..).records() of both
               files combined with np.unique + np.add.at (host_merge_*); and set_ops: sum, intersect and subtract
               over the same two files, the record kernels of each input on their own (Counter.set_jf; --only merge
               runs this group alone, without the host path)
  histo      - the count histogram and the four statistics (Counter.histo, default layout): wall time and the time of
               its kernel by HIP events (km_histo_kernel_ms), best and all of --write-reps runs, on the full counting
               table before finish (table_*: a stream read of 16 * slots bytes, also given as GB/s and as a fraction
               of the same run's km_device_copy_GBs) and on the kept counts after finish(2) (kept_*); histo_file of
               the file write_jf wrote (file_*); the kernel time of each of the three also with 0..4 wave aggregation
               rounds (*_kernel_ms_by_rounds, KM_HISTO_ROUNDS); and beside them the paths a user has today:
               Counter.records() + np.bincount (host_records_*) and Database.open(path).records() + np.bincount
               (host_open_*)
  dump       - dump_file of the file write_jf wrote, column format, to /dev/null and to a file beside it: wall time,
               best and all of --write-reps runs; the time of the text kernels by HIP events (km_dump_kernel_ms),
               bytes_out, bytes/s, pieces; and beside it the path a user has today: Database.open(path).records() and
               a vectorised numpy formatter that writes the same bytes to a file (host_dump_*; compared byte for byte
               at the `cache` size only).  --only dump runs this group alone, after the counting it needs
and km_device_copy_GBs of the same run for scale.

usage: count_bench.py [--device 0] [--sizes cache,hbm] [-k 31] [--write-reps 3] [--text-reps 3] [--only dump|merge]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from km_amd import count as kc  # noqa: E402
from km_amd import lib as kmlib  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")
SIZES = {"cache": (100_000, 200_000, 1 << 20), "hbm": (100_000_000, 2_000_000, None)}   # genome, reads, staging


def make_reads(rng, genome_len, n_reads, read_len=100):
    """(n_reads, read_len) uint8."""
    genome = ACGT[rng.integers(0, 4, genome_len)]
    out = np.empty((n_reads, read_len), np.uint8)
    for lo in range(0, n_reads, 200_000):
        hi = min(n_reads, lo + 200_000)
        starts = rng.integers(0, genome_len - read_len + 1, hi - lo)
        part = genome[starts[:, None] + np.arange(read_len)[None, :]]
        rev = rng.integers(0, 2, hi - lo).astype(bool)
        part[rev] = COMP[part[rev]][:, ::-1]
        sub = rng.random(part.shape) < 0.01
        part[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
        part[rng.random(part.shape) < 0.001] = ord("N")
        out[lo:hi] = part
    return out


def as_stream(reads):
    rows = np.full((reads.shape[0], reads.shape[1] + 1), ord("\n"), np.uint8)
    rows[:, :-1] = reads
    return rows.reshape(-1)


def as_fastq(reads, rng):
    n, ln = reads.shape
    rows = np.empty((n, 3 + ln + 3 + ln + 1), np.uint8)
    rows[:, :3] = np.frombuffer(b"@r\n", np.uint8)
    rows[:, 3:3 + ln] = reads
    rows[:, 3 + ln:6 + ln] = np.frombuffer(b"\n+\n", np.uint8)
    qual = rows[:, 6 + ln:6 + 2 * ln]
    qual[:] = ord("I")
    for lo in range(0, n, 200_000):
        part = qual[lo:lo + 200_000]
        low = rng.random(part.shape) < 0.02
        part[low] = rng.integers(ord("!"), ord("+"), int(low.sum()))
    rows[:, -1] = ord("\n")
    return rows.reshape(-1)


def feed_blocks(add, text, block=8 << 20):
    pos, tail = 0, b""
    while pos < text.size:
        buf = text[pos:pos + block]
        pos += block
        if len(tail):
            buf = np.concatenate([tail, buf])
        used = add(buf, False)
        tail = buf[used:]
    add(tail, True)


def time_text_paths(k, device, text, reps):
    """add_text and add_fastq (Q = 0, Q = '+') on the same text, alternating, each on a counter of its own grown
    from the default; wall time around calls that end in stats()."""
    os.environ["KM_COUNT_TIME_FASTQ"] = "1"
    paths = {"add_text": None, "add_fastq_q0": 0, "add_fastq_qplus": ord("+")}
    wall = {name: [] for name in paths}
    kernel_ms = {name: [] for name in paths if paths[name] is not None}
    stats = {}
    for _ in range(reps):
        for name, q in paths.items():
            c = kmlib.Counter(k=k, device=device)
            if q is None:
                add = lambda buf, final: c.add_text(buf, final=final)                         # noqa: E731
            else:
                add = lambda buf, final: c.add_fastq(buf, final=final, min_qual_char=q)       # noqa: E731
            t0 = time.perf_counter()
            feed_blocks(add, text)
            stats[name] = c.stats()
            wall[name].append(time.perf_counter() - t0)
            if q is not None:
                kernel_ms[name].append(c.fastq_kernel_ms())
            c.finish(2).close()
            c.close()
    assert (stats["add_fastq_q0"]["kmers"], stats["add_fastq_q0"]["distinct"]) == (
        stats["add_text"]["kmers"], stats["add_text"]["distinct"])
    out = {"text_reps": reps, "text_bytes": int(text.size)}
    for name in paths:
        best = min(wall[name])
        out.update({name + "_s": best, name + "_s_all": wall[name], name + "_bytes_per_s": text.size / best,
                    name + "_kmers": stats[name]["kmers"], name + "_kmers_per_s": stats[name]["kmers"] / best,
                    name + "_n_grow": stats[name]["n_grow"], name + "_table_slots": stats[name]["slots"]})
        if name in kernel_ms:
            out.update({name + "_kernel_ms": min(kernel_ms[name]), name + "_kernel_ms_all": kernel_ms[name]})
    return out, stats["add_text"]


def best_all(prefix, values):
    return {prefix: min(values), prefix + "_all": values}


def time_histo(call, reps):
    """call() -> (base, bins, stats); wall seconds and kernel ms of every repeat, and the last result."""
    wall, kernel, res = [], [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = call()
        wall.append(time.perf_counter() - t0)
        kernel.append(kmlib.histo_kernel_ms())
    return wall, kernel, res


def host_bincount(counts):
    """What a user does today with the counts on the host: the default layout's bins and the four numbers."""
    bins = np.bincount(np.minimum(counts, 10001).astype(np.int64), minlength=10002)[1:]
    return bins, {"unique": int((counts == 1).sum()), "distinct": int(counts.size),
                  "total": int(counts.sum(dtype=np.uint64)), "max_count": int(counts.max()) if counts.size else 0}


def time_histo_table(counter, reps):
    """Counter.histo() on the full counting table (before finish), and the same pass at 0..4 aggregation rounds."""
    wall, kernel, res = time_histo(counter.histo, reps)
    slots = counter.stats()["slots"]
    sweep = {}
    for rounds in range(5):
        os.environ["KM_HISTO_ROUNDS"] = str(rounds)
        sweep[str(rounds)] = time_histo(counter.histo, reps)[1]
    os.environ.pop("KM_HISTO_ROUNDS", None)
    return {**best_all("table_s", wall), **best_all("table_kernel_ms", kernel), "table_slots": slots,
            "table_bytes": 16 * slots, "table_GBs": 16 * slots / (min(kernel) * 1e-3) / 1e9,
            "table_kernel_ms_by_rounds": sweep, "table_stats": res[2]}


def time_histo_kept(counter, reps):
    """Counter.histo() after finish, against Counter.records() + np.bincount."""
    wall, kernel, res = time_histo(counter.histo, reps)
    sweep = {}
    for rounds in range(5):
        os.environ["KM_HISTO_ROUNDS"] = str(rounds)
        sweep[str(rounds)] = time_histo(counter.histo, reps)[1]
    os.environ.pop("KM_HISTO_ROUNDS", None)
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        _, counts = counter.records()
        bins, stats = host_bincount(counts)
        host.append(time.perf_counter() - t0)
    assert np.array_equal(bins, res[1].astype(bins.dtype)) and stats == res[2]
    return {**best_all("kept_s", wall), **best_all("kept_kernel_ms", kernel), "kept_stats": res[2],
            "kept_kernel_ms_by_rounds": sweep,
            **best_all("host_records_s", host)}


def time_histo_file(path, device, reps):
    """histo_file of a written file, against Database.open(path).records() + np.bincount."""
    wall, kernel, res = time_histo(lambda: kc.histo_file(path, device=device), reps)
    sweep = {}
    for rounds in range(5):
        os.environ["KM_HISTO_ROUNDS"] = str(rounds)
        sweep[str(rounds)] = time_histo(lambda: kc.histo_file(path, device=device), reps)[1]
    os.environ.pop("KM_HISTO_ROUNDS", None)
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        db = kmlib.Database.open(path)
        _, counts = db.records()
        bins, stats = host_bincount(counts)
        db.close()
        host.append(time.perf_counter() - t0)
    assert np.array_equal(bins, res[1].astype(bins.dtype)) and all(stats[key] == res[2][key] for key in stats)
    return {**best_all("file_s", wall), **best_all("file_kernel_ms", kernel), "file_bytes": os.path.getsize(path),
            "file_kernel_ms_by_rounds": sweep,
            **best_all("host_open_s", host)}


POW10 = 10 ** np.arange(1, 10, dtype=np.uint64)


def host_dump_column(keys, counts, k, fh, chunk=1 << 20):
    """`dump -c` on the host with numpy: "MER COUNT\n" per record into fh, a chunk of records at a time."""
    shifts = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    for lo in range(0, keys.size, chunk):
        key, cnt = keys[lo:lo + chunk], counts[lo:lo + chunk].astype(np.uint64)
        nd = np.searchsorted(POW10, cnt, side="right").astype(np.int64) + 1
        end = np.cumsum(k + 2 + nd)
        at = end - (k + 2 + nd)
        out = np.empty(int(end[-1]), np.uint8)
        out[at[:, None] + np.arange(k)[None, :]] = ACGT[((key[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)]
        out[at + k] = 32
        for d in range(10):
            has = nd > d
            out[(end - 2 - d)[has]] = (48 + (cnt[has] // np.uint64(10 ** d)) % np.uint64(10)).astype(np.uint8)
        out[end - 1] = 10
        fh.write(out.tobytes())


def time_dump_file(counter, k, reps, compare):
    """The field group `dump`: the finished counter's file (Counter.write_jf), then dump_file of it in column format to
    /dev/null and to a file beside it, against Database.open(path).records() + host_dump_column (the same bytes:
    compared when `compare`)."""
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
    path = os.path.join(tmp, "count_bench_%d_dump.jf" % os.getpid())
    device = counter.device
    out_path, host_path = path + ".dump.txt", path + ".host_dump.txt"
    null, to_file, kernel, host, parts, st = [], [], [], [], None, None
    try:
        counter.write_jf(path)
        for _ in range(reps):
            with open(os.devnull, "wb") as fh:
                t0 = time.perf_counter()
                st = kc.dump_file(path, out=fh, fmt="column", device=device)
                null.append(time.perf_counter() - t0)
            kernel.append(kmlib.dump_kernel_ms())
        for _ in range(reps):
            t0 = time.perf_counter()
            kc.dump_file(path, out=out_path, fmt="column", device=device)
            to_file.append(time.perf_counter() - t0)
        for _ in range(reps):
            t0 = time.perf_counter()
            db = kmlib.Database.open(path)
            keys, counts = db.records()
            db.close()
            t1 = time.perf_counter()
            with open(host_path, "wb") as fh:
                host_dump_column(keys, counts, k, fh)
            t2 = time.perf_counter()
            host.append(t2 - t0)
            if parts is None or host[-1] <= min(host):
                parts = {"open_records_s": t1 - t0, "format_write_s": t2 - t1}
        assert os.path.getsize(out_path) == os.path.getsize(host_path) == st["bytes_out"]
        if compare:
            with open(out_path, "rb") as a, open(host_path, "rb") as b:
                assert a.read() == b.read()
    finally:
        for p in (path, out_path, host_path):
            if os.path.exists(p):
                os.unlink(p)
    return {"dump": {
        "reps": reps, "dir": tmp, "records": st["records_out"], "bytes_out": st["bytes_out"], "pieces": st["pieces"],
        **best_all("null_s", null), **best_all("file_s", to_file), **best_all("kernel_ms", kernel),
        "null_bytes_per_s": st["bytes_out"] / min(null), "file_bytes_per_s": st["bytes_out"] / min(to_file),
        "kernel_bytes_per_s": st["bytes_out"] / (min(kernel) * 1e-3), "compared": bool(compare),
        **best_all("host_dump_s", host), "host_dump_parts": parts,
    }}


def time_writers(counter, k, reps):
    """The field group of the two file writers on a finished counter (and, on the file they leave, histo_file)."""
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
    path = os.path.join(tmp, "count_bench_%d.jf" % os.getpid())
    native, kernels, host, parts = [], [], [], None
    try:
        for _ in range(reps):
            t0 = time.perf_counter()
            counter.write_jf(path)
            native.append(time.perf_counter() - t0)
            stats = kmlib.jf_sort_stats()
            kernels.append(stats["kernel_ms"])
            size = os.path.getsize(path)
        for _ in range(reps):
            t0 = time.perf_counter()
            keys, counts = counter.records()
            t1 = time.perf_counter()
            kc.write_records(path, keys, counts, k, counter.canonical)      # (its np.argsort included)
            t2 = time.perf_counter()
            host.append(t2 - t0)
            if parts is None or host[-1] <= min(host):
                parts = {"records_s": t1 - t0, "write_records_s": t2 - t1}
        histo_file = time_histo_file(path, counter.device, reps)
    finally:
        if os.path.exists(path):
            os.unlink(path)
    return {
        "write_reps": reps, "write_dir": tmp, "write_jf_file_bytes": size,
        "write_jf_s": min(native), "write_jf_s_all": native,
        "write_jf_kernel_ms": min(kernels), "write_jf_kernel_ms_all": kernels,
        "write_jf_buckets": stats["buckets"], "write_jf_largest_bucket": stats["largest"],
        "write_jf_oversized_buckets": stats["oversized"],
        "host_sorted_s": min(host), "host_sorted_s_all": host, "host_sorted_parts": parts,
    }, histo_file


def time_set_ops(paths, n_in, k, device, reps):
    """sum, intersect and subtract over the same two files, each input's kernels timed on their own (merge_stats waits
    for the device between the inputs, so the wall time of these runs is not that of add_jf_s)."""
    out = {}
    for mode in ("sum", "intersect", "subtract"):
        per_input, kept = [], None
        for _ in range(reps):
            c = kmlib.Counter(k=k, device=device, expected_distinct=max(n_in) if mode == "sum" else n_in[0])
            ms = [0.0]
            for p in paths:
                if mode == "sum":
                    c.add_jf(p)
                else:
                    c.set_jf(p, op=mode)
                ms.append(c.merge_stats()["kernel_ms"])
            per_input.append([b - a for a, b in zip(ms, ms[1:])])
            st = c.stats()
            c.finish(1).close()
            kept = c.n_records()
            c.close()
        out[mode] = {"kernel_ms_per_input_all": per_input, "kernel_ms_per_input": [min(r[i] for r in per_input) for i in (0, 1)],
                     "records_out": kept, "table_slots": st["slots"], "n_grow": st["n_grow"]}
    return out


def time_merge(stream, k, device, reps, host_path=True):
    """The field group of merging: two files from the halves of the reads, add_jf of both against the host path; then
    the set operations over the same two files (time_set_ops)."""
    os.environ["KM_COUNT_TIME_MERGE"] = "1"
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
    paths = [os.path.join(tmp, "count_bench_%d_half%d.jf" % (os.getpid(), i)) for i in range(2)]
    half = stream.size // 2
    half -= half % 101                                   # (a read and its newline: the cut falls between reads)
    try:
        for path, part in zip(paths, (stream[:half], stream[half:])):
            c = kmlib.Counter(k=k, device=device)
            c.add_bases(part)
            c.finish(1).close()
            c.write_jf(path)
            c.close()
        n_in = [kmlib.jf_file_info(p)["n_records"] for p in paths]
        wall, kernel, host, parts = [], [], [], None
        for _ in range(reps):
            c = kmlib.Counter(k=k, device=device, expected_distinct=max(n_in))
            t0 = time.perf_counter()
            for p in paths:
                c.add_jf(p)
            st = c.stats()
            wall.append(time.perf_counter() - t0)
            kernel.append(c.merge_stats()["kernel_ms"])
            c.close()
        set_ops = time_set_ops(paths, n_in, k, device, reps)
        for _ in range(reps if host_path else 0):
            t0 = time.perf_counter()
            recs = []
            for p in paths:
                db = kmlib.Database.open(p)
                recs.append(db.records())
                db.close()
            t1 = time.perf_counter()
            keys, inverse = np.unique(np.concatenate([r[0] for r in recs]), return_inverse=True)
            total = np.zeros(keys.size, np.uint64)
            np.add.at(total, inverse, np.concatenate([r[1] for r in recs]))
            t2 = time.perf_counter()
            host.append(t2 - t0)
            if parts is None or host[-1] <= min(host):
                parts = {"open_records_s": t1 - t0, "unique_add_s": t2 - t1}
        assert not host_path or keys.size == st["distinct"]
    finally:
        for p in paths:
            if os.path.exists(p):
                os.unlink(p)
    return {"merge": {
        "reps": reps, "dir": tmp, "records_in": n_in, "distinct": st["distinct"], "n_grow": st["n_grow"],
        "table_slots": st["slots"], "add_jf_s": min(wall), "add_jf_s_all": wall,
        "add_jf_records_per_s": sum(n_in) / min(wall), "add_jf_kernel_ms": min(kernel), "add_jf_kernel_ms_all": kernel,
        "host_merge_s": min(host) if host else None, "host_merge_s_all": host, "host_merge_parts": parts,
        "set_ops": set_ops,
    }}


def run_size(name, k, device, rng, write_reps=3, text_reps=3, only=None):
    genome_len, n_reads, stage = SIZES[name]
    if stage:
        os.environ["KM_COUNT_STAGE_BYTES"] = str(stage)
    else:
        os.environ.pop("KM_COUNT_STAGE_BYTES", None)
    reads = make_reads(rng, genome_len, n_reads)
    stream, text = as_stream(reads), as_fastq(reads, rng)
    warm = kmlib.Counter(k=k, device=device)              # code object load, first allocations
    warm.add_bases(stream[:1_000_000])
    warm.finish().close()
    warm.close()
    if only == "merge":
        return {"reads": n_reads, "staging_bytes": stage or 16 << 20, **time_merge(stream, k, device, write_reps, host_path=False)}

    sized = kmlib.Counter(k=k, device=device, expected_distinct=0 if stage else 2 * genome_len + stream.size // 20)
    t0 = time.perf_counter()
    sized.add_bases(stream)
    st = sized.stats()
    t_bases = time.perf_counter() - t0
    histo = time_histo_table(sized, write_reps) if not only else {}
    t0 = time.perf_counter()
    db = sized.finish(2)
    t_finish = time.perf_counter() - t0
    n_kept = int(db.info.n_records)
    db.close()
    dump = time_dump_file(sized, k, write_reps, compare=name == "cache")
    if only == "dump":
        sized.close()
        return {"reads": n_reads, "kmers": st["kmers"], "distinct": st["distinct"], "kept_at_L2": n_kept,
                "staging_bytes": stage or 16 << 20, **dump}
    histo.update(time_histo_kept(sized, write_reps))
    writers, histo_file = time_writers(sized, k, write_reps)
    histo.update(histo_file)
    sized.close()

    merged = time_merge(stream, k, device, write_reps)
    text_paths, st_text = time_text_paths(k, device, text, text_reps)
    assert (st_text["kmers"], st_text["distinct"]) == (st["kmers"], st["distinct"])
    traffic = 12 * st["kmers"] + 8 * st["distinct"]
    return {
        "reads": n_reads, "bases": st["bases"], "kmers": st["kmers"], "distinct": st["distinct"],
        "kept_at_L2": n_kept, "table_slots": st["slots"], "table_MB": st["slots"] * 16 / 1e6,
        "staging_bytes": stage or 16 << 20,
        "add_bases_s": t_bases, "add_bases_kmers_per_s": st["kmers"] / t_bases, "add_bases_n_grow": st["n_grow"],
        "add_bases_table_GBs": traffic / t_bases / 1e9,
        **text_paths,
        "finish_s": t_finish,
        **writers,
        **merged,
        "histo": histo,
        **dump,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sizes", default="cache,hbm")
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--write-reps", type=int, default=3)
    ap.add_argument("--text-reps", type=int, default=3)
    ap.add_argument("--only", choices=["dump", "merge"], default=None,
                    help="this field group alone, after the counting it needs (merge: without the host path)")
    args = ap.parse_args()
    kmlib.load()
    rng = np.random.default_rng(2026)
    out = {"tool": "count_bench", "k": args.k, "sizes": {}}
    for name in args.sizes.split(","):
        out["sizes"][name] = run_size(name, args.k, args.device, rng, args.write_reps, args.text_reps, args.only)
    out["km_device_copy_GBs"] = kmlib.device_copy_GBs(args.device, 1 << 30, 10)
    for size in out["sizes"].values() if not args.only else ():
        size["histo"]["table_fraction_of_copy"] = size["histo"]["table_GBs"] / out["km_device_copy_GBs"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
