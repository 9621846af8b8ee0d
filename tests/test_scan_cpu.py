"""The scan (kmjf_cov_seqs, kmjf_scan_text, `cov`, `query -s`) where no GPU is needed: the model every scan test
compares with, that model pinned to the reference's answers, the window rule of csrc/scan_rule.h driven on the CPU
under AddressSanitizer + UBSan, and the `cov` command's arguments and rows.

``model_cov`` and ``model_text`` are written from the rule of include/kmgpu.h alone, as a loop over windows with a dict
as the table; they share nothing with csrc/scan_rule.h, km_amd.count._windows or km_amd.kmer.sliding_kmers."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from km_amd import cli
from oracle import jf_reader as jr
from oracle import km_oracle as ko

HERE = os.path.dirname(os.path.abspath(__file__))
JF_DIR = os.path.join(HERE, "data", "jf")
CATALOG = os.path.join(HERE, "data", "catalog", "GRCh38")
NONE = 0xFFFFFFFF

# ------------------------------------------------------------------ the model
_BASES = b"ACGTacgt"
_DIGITS = bytes.maketrans(b"ACGTacgt", b"01230123")
_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")


def as_bytes(seq):
    if isinstance(seq, str):
        return seq.encode("latin-1")
    return bytes(seq) if not isinstance(seq, np.ndarray) else seq.tobytes()


def pack(window):
    """k bases -> the packed k-mer: A 0, C 1, G 2, T 3, the first base most significant."""
    return int(window.translate(_DIGITS), 4)


def windows(seq, k, canonical):
    """Per window of one sequence, in order: None for a window with a non-base, else (looked-up key, printed key).
    A sequence shorter than k has none."""
    seq = as_bytes(seq)
    for i in range(len(seq) - k + 1):
        w = seq[i:i + k]
        if w.translate(None, _BASES):
            yield None
            continue
        key = pack(w)
        if canonical:
            key = min(key, pack(w.translate(_COMPLEMENT)[::-1]))
        yield key, key


def model_cov(seqs, table, k, canonical):
    """[(total, n_kmers, n_zero, n_skipped, n_nonbase, min, max)] per sequence, as km_cov_t."""
    out = []
    for seq in seqs:
        seq = as_bytes(seq)
        counts, skipped = [], 0
        for w in windows(seq, k, canonical):
            if w is None:
                skipped += 1
            else:
                counts.append(table.get(w[0], 0))
        out.append((sum(counts), len(counts), sum(1 for c in counts if c == 0), skipped, len(seq.translate(None, _BASES)),
                    min(counts) if counts else NONE, max(counts) if counts else 0))
    return out


def model_text(seqs, table, k, canonical):
    """The bytes `query -s` prints: "MER COUNT" per valid window, sequence after sequence."""
    lines = []
    for seq in seqs:
        for w in windows(seq, k, canonical):
            if w is not None:
                mer = "".join("ACGT"[(w[1] >> (2 * (k - 1 - j))) & 3] for j in range(k))
                lines.append("%s %d\n" % (mer, table.get(w[0], 0)))
    return "".join(lines).encode("ascii")


def n_windows(seqs, k):
    return sum(max(0, len(as_bytes(s)) - k + 1) for s in seqs)


def file_table(path):
    rec = jr.read_jf(path)
    return dict(zip(rec["keys"].tolist(), rec["counts"].tolist())), int(rec["k"]), bool(rec["canonical"])


def fasta_records(path):
    """The records of a FASTA file, lines joined, as this test reads them (plain text files only)."""
    records = []
    with open(path, "rb") as fh:
        for line in fh:
            if line.startswith(b">"):
                records.append([])
            elif records:
                records[-1].append(line.strip())
    return [b"".join(r) for r in records]


def cov_tuple(seq, c):
    """A model cell as the tuple of common.get_cov."""
    return (c[0], len(seq), c[5], c[6], float(c[0]) / c[1], c[1], c[2])


def cov_rows(dbs, files, tables=None):
    """What `cov` prints for these databases and FASTA files, from the model."""
    text = "DB\ttarget\trecord\tcount\tlength\tmin\tmax\tmean\tkmer_nb\tkmer_nb_0\tkmer_nb_skipped\n"
    for db in dbs:
        table, k, canonical = file_table(db)
        for path in files:
            stem = os.path.splitext(os.path.basename(path))[0]
            records = fasta_records(path)
            for i, (seq, c) in enumerate(zip(records, model_cov(records, table, k, canonical)), 1):
                mid = "%d\t%d\t%.2f" % (c[5], c[6], float(c[0]) / c[1]) if c[1] else "NA\tNA\tNA"
                text += "%s\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d\n" % (db, stem, i, c[0], len(seq), mid, c[1], c[2], c[3])
    return text


# ------------------------------------------------------------------ the model against the reference
def test_the_model_equals_the_reference_on_the_bundled_fixtures(monkeypatch):
    monkeypatch.chdir(HERE)
    with open(os.path.join(HERE, "golden", "fixtures_children.json")) as fh:
        cases = json.load(fh)["min_cov"]
    assert len(cases) >= 5
    for g in cases:
        seq = ko.read_fasta_concat(g["target"])
        table, k, canonical = file_table(g["db"])
        (c,) = model_cov([seq], table, k, canonical)
        assert c[3] == c[4] == 0
        assert list(cov_tuple(seq, c)) == g["cov"] == list(ko.coverage(g["db"], seq))
    seq = ko.read_fasta_concat("./data/catalog/GRCh38/FLT3-ITD_exons_13-15.fa")
    table, k, canonical = file_table("./data/jf/03H112_IandI.jf")
    total, length, lo, hi, mean, n, n0 = cov_tuple(seq, model_cov([seq], table, k, canonical)[0])
    assert (total, length, lo, hi, "%.2f" % mean, n, n0) == (275596, 345, 618, 1368, "874.91", 315, 0)
    text = model_text([seq], table, k, canonical).split(b"\n")
    assert len(text) == 316 and sum(int(ln.split()[1]) for ln in text[:-1]) == 275596


def test_the_model_on_cases_read_off_the_rule():
    table = {pack(b"ACG"): 7, pack(b"AAA"): 2}
    assert model_cov([b"ACGT", b"", b"AC", b"ACNGT", b"acgt"], table, 3, True) == [
        (14, 2, 0, 0, 0, 7, 7),              # ACG, and CGT whose reverse complement is ACG
        (0, 0, 0, 0, 0, NONE, 0), (0, 0, 0, 0, 0, NONE, 0),
        (0, 0, 0, 3, 1, NONE, 0),            # every window holds the N
        (14, 2, 0, 0, 0, 7, 7)]
    assert model_cov([b"ACGT"], table, 3, False) == [(7, 2, 1, 0, 0, 0, 7)]
    assert model_text([b"ACGT", b"TTTN"], table, 3, True) == b"ACG 7\nACG 7\nAAA 2\n"
    assert model_text([b"ACGT", b"TTTN"], table, 3, False) == b"ACG 7\nCGT 0\nTTT 0\n"


# ------------------------------------------------------------------ csrc/scan_rule.h on the CPU
def random_bases(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def rule_batches():
    """(name, k, canonical, sequences): the shapes of tests/test_scan.py, small enough for a sanitizer build."""
    rng = np.random.default_rng(7)
    out = []
    for k in (5, 31):
        lengths = [0, 1, k - 1, k, k + 1, 32, 33, 32 + k - 1, 2047, 2048, 2049, 2048 + k - 1, 8191, 8192, 8193, 3 * 8192 + 5]
        out.append(("lengths", k, True, [random_bases(rng, n) for n in lengths]))
        tiny = [random_bases(rng, int(n)) for n in rng.integers(0, k + 3, 600)]
        tiny[100] = random_bases(rng, 3000)
        out.append(("tiny", k, k == 5, tiny))
        edges = []
        for at in (31, 32, 33, 2047, 2048, 2049):
            edges += [random_bases(rng, at), random_bases(rng, k + 3), random_bases(rng, (-at - k - 3) % 64)]
        out.append(("edges", k, False, edges))
        long_n = bytearray(random_bases(rng, 300))
        long_n[::k] = b"N" * len(long_n[::k])
        out.append(("non-bases", k, True, [b"N" + random_bases(rng, 70) + b"N", bytes(long_n), b"AN"[: k - 1], b"acgtacgtacgtnacgtacgtacgtacgtacgtacgtacgt",
                                           random_bases(rng, 40) + b"N", b"N" + random_bases(rng, 40), b"", b"N", b""]))
    # the structured corpus of tests/test_text_kernels_every_k.py, a few KB of it: k = 32 (no mask, keys above 2^63), even
    # k (palindromes), k = 2 .. 4, 2k across 32 bits, homopolymers, microsatellites, both strands, non-bases at the ends
    # of a lane's range
    import test_text_kernels_every_k as every_k
    for k in every_k.RULE_KS:
        for canonical in (True, False):
            out.append(("structured", k, canonical, every_k.structured_reads(k, small=True)))
    return out


def rule_input(path, k, canonical, seqs, table, stages):
    off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.uint64)
    text = b"".join(seqs)
    with open(path, "wb") as fh:
        fh.write(b"%d %d %d %d %d %d\n" % (k, canonical, len(seqs), len(table), len(stages), len(text)))
        fh.write(b" ".join(b"%d" % v for v in off.tolist()) + b"\n")
        fh.write(b" ".join(b"%d" % v for v in stages) + b"\n")
        fh.write(b"".join(b"%d %d\n" % kv for kv in table.items()))
        fh.write(b"TEXT\n" + text)


def a_tenth_of_the_kmers(seqs, k, canonical, rng):
    """A table of about a tenth of the batch's k-mers, counts over the whole 32-bit range."""
    keys = sorted({w[0] for s in seqs for w in windows(s, k, canonical) if w is not None})
    picked = [key for key in keys if rng.random() < 0.1] or keys[:1]
    special = [1, 9, 65534, 65535, 65536, NONE]
    return {key: special[i % len(special)] if i % 3 == 0 else int(rng.integers(1, 1 << 20)) for i, key in enumerate(picked)}


def test_rule_program_under_sanitizers(tmp_path):
    """csrc/scan_rule.h built for the CPU with AddressSanitizer + UBSan (tests/host/scan_rule.cpp): window validity,
    the sequence a window belongs to, the pieces and their overlap, and the walk of every lane of every piece at four
    staging sizes, against the model: statistics per sequence and the text, byte for byte."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "scan_rule")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "host", "scan_rule.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    rng = np.random.default_rng(8)
    for name, k, canonical, seqs in rule_batches():
        table = a_tenth_of_the_kmers(seqs, k, canonical, rng)
        stages = [k, 256, 4096, 1 << 24]
        if name != "tiny":
            stages = stages[1:]
        path = str(tmp_path / "in.bin")
        rule_input(path, k, int(canonical), seqs, table, stages)
        proc = subprocess.run([exe, path], capture_output=True, env=env, timeout=600)
        assert proc.returncode == 0 and proc.stdout.endswith(b"SCAN RULE OK\n"), (name, k, proc.stdout[-2000:], proc.stderr[-3000:])
        assert b"ERROR: AddressSanitizer" not in proc.stderr and b"runtime error" not in proc.stderr, proc.stderr[-3000:]
        cells = "".join("%d %d %d %d %d %d %d\n" % c for c in model_cov(seqs, table, k, canonical)).encode()
        text = model_text(seqs, table, k, canonical)
        total = sum(len(s) for s in seqs)
        want = b"WINDOWS %d\n" % n_windows(seqs, k)
        for stage in stages:
            pieces = -(-total // (stage - (k - 1)))
            want += b"STAGE %d PIECES %d\n" % (stage, pieces) + cells + b"TEXT %d\n" % len(text) + text
        assert proc.stdout == want + b"SCAN RULE OK\n", (name, k)


# ------------------------------------------------------------------ the cov command without a GPU
def test_cov_arguments(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">r\nACGT\n")
    gz = tmp_path / "b.fa.gz"
    gz.write_bytes(b"\x1f\x8b\x08\x00")
    p = cli.parse_args(["cov", "-o", "out.tsv", "-t", str(fa), str(gz), "x.jf", "y.jf"])
    assert (p.targets, p.jellyfish_fn, p.output) == ([str(fa), str(gz)], ["x.jf", "y.jf"], "out.tsv")
    p = cli.parse_args(["cov", "-t", str(tmp_path), "x.jf"])
    assert (p.targets, p.jellyfish_fn, p.output) == ([str(tmp_path)], ["x.jf"], None)
    p = cli.parse_args(["cov", "-t", str(fa), "-o", "o", "x.jf"])           # an option in between: argparse's own split
    assert (p.targets, p.jellyfish_fn) == ([str(fa)], ["x.jf"])
    for bad in (["cov", "x.jf"], ["cov", "-t", str(fa)], ["cov", "-t", "x.jf"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(bad)
        assert e.value.code == 2


def test_cov_rows():
    cell = np.zeros(1, [("total", "<u8"), ("n_kmers", "<u8"), ("n_zero", "<u8"), ("n_skipped", "<u8"), ("n_nonbase", "<u8"),
                        ("min", "<u4"), ("max", "<u4")])[0]
    cell["min"] = NONE
    assert cli.cov_row("s.jf", "NPM1", 1, 27, cell) == "s.jf\tNPM1\t1\t0\t27\tNA\tNA\tNA\t0\t0\t0\n"
    cell["n_skipped"] = 4
    assert cli.cov_row("s.jf", "NPM1", 1, 27, cell) == "s.jf\tNPM1\t1\t0\t27\tNA\tNA\tNA\t0\t0\t4\n"
    cell["total"], cell["n_kmers"], cell["n_zero"], cell["min"], cell["max"] = 275596, 315, 0, 618, 1368
    assert cli.cov_row("d", "FLT3", 2, 345, cell) == "d\tFLT3\t2\t275596\t345\t618\t1368\t874.91\t315\t0\t4\n"
    cell["total"] = 3 * NONE + 5
    cell["n_kmers"], cell["max"] = 4, NONE
    assert cli.cov_row("d", "t", 1, 40, cell).split("\t")[3:8] == ["12884901890", "40", "618", "4294967295", "3221225472.50"]
    assert cli.COV_HEADER == "DB\ttarget\trecord\tcount\tlength\tmin\tmax\tmean\tkmer_nb\tkmer_nb_0\tkmer_nb_skipped\n"
    assert cov_rows([], []) == cli.COV_HEADER
