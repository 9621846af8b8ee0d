"""Microbenchmark of the read selection (``bait``): 64 MB of seeded 100-nt FASTQ reads against the canonical 31-mers of
the nine catalog targets; prints ONE JSON line.

The reads are random bases; about one in a thousand is a stretch of a catalog target instead (either strand), so
``bait`` keeps about 0.1 % of them and ``bait -v`` all the others: the two ends of the gather, which copies next to
nothing in the first shape and nearly the whole input in the second.  Per shape:
  wall_s         - count.select_files of the text (one plain file) to /dev/null, best of --reps, all listed
  kernel_ms      - lib.select_kernel_ms() of that run (KM_SELECT_TIME=1): front (line table, mask), hits, sizes (sizes
                   and scan), gather (k_sel_gather alone), summed over the pieces
  gather_GBs     - (bytes_out read + bytes_out written) / k_sel_gather's time: beside km_device_copy_GBs, which is
                   read + write of a large device-to-device copy in the same run; group_GBs: the same over sizes +
                   scan + gather
  bytes_in / bytes_out / reads_in / reads_out / pieces
`paired` holds `bait` and `bait -v` over the same reads as two mate files of half of them each
(count.select_pair_files, rule any, names checked): wall_s, kernel_ms (both mates summed; "sizes" holds the pair's
sizes, the name check and both scans, "gather" the one launch for both mates), pairs_in / pairs_out, bytes per mate,
pieces, resent_bytes and resent_share = resent bytes / bytes_in.
`bait_v_one_piece` is `bait -v` again with staging buffers (KM_COUNT_STAGE_BYTES) and blocks that hold the whole text,
so that every kernel runs once over 64 MB;
and once: the same text in the same blocks through Counter.add_fastq (counting its k-mers: the other consumer of the
front half), and km_device_copy_GBs.

usage: select_bench.py [--device 0] [--mb 64] [--reps 3]
"""
import argparse
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from km_amd import count as kc  # noqa: E402
from km_amd import lib as kmlib  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")
READ = 100


def make_text(rng, n_bytes, targets, fraction=0.001):
    """4-line FASTQ, "@r\\n" headers, qualities 'I': n_bytes / 207 reads, `fraction` of them cut from a target."""
    n = n_bytes // (2 * READ + 7)
    reads = ACGT[rng.integers(0, 4, (n, READ))]
    long_enough = [t for t in targets if t.size >= READ]
    for i in np.flatnonzero(rng.random(n) < fraction):
        t = long_enough[int(rng.integers(len(long_enough)))]
        a = int(rng.integers(0, t.size - READ + 1))
        r = t[a:a + READ]
        reads[i] = COMP[r][::-1] if rng.integers(2) else r
    rows = np.empty((n, 2 * READ + 7), np.uint8)
    rows[:, :3] = np.frombuffer(b"@r\n", np.uint8)
    rows[:, 3:3 + READ] = reads
    rows[:, 3 + READ:6 + READ] = np.frombuffer(b"\n+\n", np.uint8)
    rows[:, 6 + READ:6 + 2 * READ] = ord("I")
    rows[:, -1] = ord("\n")
    return rows.reshape(-1), n


def time_shape(db, path, invert, reps, block=kc.BLOCK):
    wall, kernel, stats = [], [], None
    with open(os.devnull, "wb") as null:
        for _ in range(reps):
            t0 = time.perf_counter()
            stats = kc.select_files(db, [path], out=null, invert=invert, block=block)
            wall.append(time.perf_counter() - t0)
            kernel.append(kmlib.select_kernel_ms())
    best = min(range(reps), key=lambda i: wall[i])
    ms = kernel[best]
    out = {"wall_s": wall[best], "wall_s_all": wall, "kernel_ms": ms, "kernel_ms_all": kernel,
           "bytes_per_s": stats["bytes_in"] / wall[best],
           "reads_in": stats["records_in"], "reads_out": stats["records_out"], "bytes_in": stats["bytes_in"],
           "bytes_out": stats["bytes_out"], "pieces": stats["pieces"]}
    gather_ms = min(k["gather"] for k in kernel)
    group_ms = min(k["sizes"] + k["gather"] for k in kernel)
    out["gather_ms_best"], out["group_ms_best"] = gather_ms, group_ms
    out["gather_GBs"] = 2 * stats["bytes_out"] / (gather_ms * 1e-3) / 1e9 if gather_ms > 0 else None
    out["group_GBs"] = 2 * stats["bytes_out"] / (group_ms * 1e-3) / 1e9 if group_ms > 0 else None
    return out


def time_paired(db, path1, path2, invert, reps, block=kc.BLOCK):
    wall, kernel, stats = [], [], None
    with open(os.devnull, "wb") as null1, open(os.devnull, "wb") as null2:
        for _ in range(reps):
            t0 = time.perf_counter()
            stats = kc.select_pair_files(db, [path1], [path2], null1, null2, invert=invert, block=block)
            wall.append(time.perf_counter() - t0)
            kernel.append(kmlib.select_kernel_ms())
    best = min(range(reps), key=lambda i: wall[i])
    bytes_in = sum(stats["bytes_in"])
    return {"wall_s": wall[best], "wall_s_all": wall, "kernel_ms": kernel[best], "kernel_ms_all": kernel,
            "bytes_per_s": bytes_in / wall[best], "pairs_in": stats["pairs_in"], "pairs_out": stats["pairs_out"],
            "bytes_in": stats["bytes_in"], "bytes_out": stats["bytes_out"], "pieces": stats["pieces"],
            "resent_bytes": stats["resent_bytes"], "resent_share": sum(stats["resent_bytes"]) / bytes_in}


def time_counter(text, device, reps, block=kc.BLOCK):
    wall = []
    for _ in range(reps):
        c = kmlib.Counter(k=31, device=device)
        t0 = time.perf_counter()
        pos, tail = 0, b""
        while pos < text.size:
            buf = text[pos:pos + block]
            pos += block
            if len(tail):
                buf = np.concatenate([tail, buf])
            used = c.add_fastq(buf, final=False)
            tail = buf[used:]
        c.add_fastq(tail, final=True)
        c.stats()
        wall.append(time.perf_counter() - t0)
        c.close()
    return {"add_fastq_s": min(wall), "add_fastq_s_all": wall, "add_fastq_bytes_per_s": text.size / min(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--mb", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    kmlib.load()
    os.environ["KM_SELECT_TIME"] = "1"
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "data", "catalog", "GRCh38", "*.fa")))
    targets = [seq for f in files for seq in kc._fasta_records(f)]
    db, _ = kc.count_files(files, k=31, canonical=True, device=args.device)
    rng = np.random.default_rng(2027)
    text, n_reads = make_text(rng, args.mb << 20, targets)
    out = {"tool": "select_bench", "k": 31, "targets": len(files), "bait_kmers": int(db.info.n_records),
           "text_bytes": int(text.size), "reads": n_reads, "reps": args.reps}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "reads.fq")
        text.tofile(path)
        time_shape(db, path, False, 1)                    # code object load, first allocations
        out["bait"] = time_shape(db, path, False, args.reps)
        out["bait_v"] = time_shape(db, path, True, args.reps)
        half = (n_reads // 2) * (2 * READ + 7)            # the same text as two mate files of half the reads each
        path1, path2 = os.path.join(tmp, "reads_1.fq"), os.path.join(tmp, "reads_2.fq")
        text[:half].tofile(path1)
        text[half:2 * half].tofile(path2)
        time_paired(db, path1, path2, False, 1)
        out["paired"] = {"bait": time_paired(db, path1, path2, False, args.reps),
                         "bait_v": time_paired(db, path1, path2, True, args.reps)}
        out.update(time_counter(text, args.device, args.reps))      # (before the large buffers of the last shape)
        os.environ["KM_COUNT_STAGE_BYTES"] = str(text.size + 4096)
        time_shape(db, path, True, 1, block=text.size + 4096)
        out["bait_v_one_piece"] = time_shape(db, path, True, args.reps, block=text.size + 4096)
        del os.environ["KM_COUNT_STAGE_BYTES"]
    db.close()
    out["km_device_copy_GBs"] = kmlib.device_copy_GBs(args.device, 1 << 30, 10)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
