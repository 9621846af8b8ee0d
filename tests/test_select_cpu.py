"""The selection of FASTQ reads by a k-mer table (km_select_*, kmjf_fastq_hits, `bait`) where no GPU is needed: the
model every select test compares with, that model pinned to the reference's answers, csrc/select_rule.h driven on the
CPU under AddressSanitizer + UBSan, and the `bait` command's argument rules.

``model_hits`` and ``model_select`` are written from the rule of include/kmgpu.h alone, record by record and window by
window with a dict as the table; they share nothing with csrc/select_rule.h, csrc/scan_rule.h or km_amd.count._windows."""
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

# ------------------------------------------------------------------ the model
_BASES = b"ACGTacgt"
_DIGITS = bytes.maketrans(b"ACGTacgt", b"01230123")
_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")
NO_AT, NO_PLUS, QUAL_LEN, TRUNCATED = 1, 2, 3, 4
KIND_TEXT = {NO_AT: "does not start with '@'", NO_PLUS: "lacks its '+' line",
             QUAL_LEN: "quality line is not as long as its sequence", TRUNCATED: "is incomplete"}


class Malformed(Exception):
    def __init__(self, kind, offset):
        Exception.__init__(self, "kind %d at %d" % (kind, offset))
        self.kind, self.offset = kind, offset


def _pack(window):
    return int(window.translate(_DIGITS), 4)


def _content(line):
    """A line without its newline and without one '\\r' in front of that."""
    line = line[:-1] if line.endswith(b"\n") else line
    return line[:-1] if line.endswith(b"\r") else line


def fastq_records(text):
    """[(header, sequence, plus, quality)], every line raw with its newline (the last may lack it).  Malformed text
    raises Malformed with the smallest (offset, kind) of what the validation of include/kmgpu.h finds."""
    text = bytes(text)
    lines = [ln + b"\n" for ln in text.split(b"\n")]                   # (splitlines would break at a lone '\r')
    lines[-1] = lines[-1][:-1]
    if not lines[-1]:
        lines.pop()
    starts = np.concatenate(([0], np.cumsum([len(ln) for ln in lines]))).tolist()
    found = []
    if len(lines) % 4:
        found.append((starts[len(lines) & ~3], TRUNCATED))
    for i, ln in enumerate(lines):
        if i % 4 == 0 and ln[:1] != b"@":
            found.append((starts[i], NO_AT))
        if i % 4 == 2 and ln[:1] != b"+":
            found.append((starts[i], NO_PLUS))
        if i % 4 == 3 and len(_content(ln)) != len(_content(lines[i - 2])):
            found.append((starts[i], QUAL_LEN))
    if found:
        offset, kind = min(found)
        raise Malformed(kind, offset)
    return [tuple(lines[i:i + 4]) for i in range(0, len(lines), 4)]


def read_hits(seq, qual, table, k, canonical, min_qual=0):
    """hits of one read: the windows of k bases (a base whose quality byte is below min_qual is none) whose k-mer the
    table holds with a count > 0."""
    if min_qual:
        seq = bytes(b if q >= min_qual else 0x4E for b, q in zip(seq, qual))
    hits = 0
    for i in range(len(seq) - k + 1):
        w = seq[i:i + k]
        if w.translate(None, _BASES):
            continue
        key = _pack(w)
        if canonical:
            key = min(key, _pack(w.translate(_COMPLEMENT)[::-1]))
        hits += table.get(key, 0) > 0
    return hits


def model_hits(text, table, k, canonical, min_qual=0):
    return [read_hits(_content(s), _content(q), table, k, canonical, min_qual) for _, s, _, q in fastq_records(text)]


def model_select(text, table, k, canonical, min_hits=1, invert=False, min_qual=0):
    """The bytes a final stream `text` leaves on the descriptor."""
    records = fastq_records(text)
    hits = [read_hits(_content(s), _content(q), table, k, canonical, min_qual) for _, s, _, q in records]
    out = b"".join(b"".join(rec) for rec, h in zip(records, hits) if (h >= min_hits) != bool(invert))
    return out + b"\n" if out and not out.endswith(b"\n") else out


def file_table(path):
    rec = jr.read_jf(path)
    return dict(zip(rec["keys"].tolist(), rec["counts"].tolist())), int(rec["k"]), bool(rec["canonical"])


def kmers_of(seqs, k, canonical):
    """{key: 1} of every valid window of the sequences: the table `bait -t` builds."""
    table = {}
    for seq in seqs:
        for i in range(len(seq) - k + 1):
            w = seq[i:i + k]
            if not w.translate(None, _BASES):
                key = _pack(w)
                table[min(key, _pack(w.translate(_COMPLEMENT)[::-1])) if canonical else key] = 1
    return table


def random_bases(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def fastq(reads, names=None, quals=None, eol=b"\n", last_newline=True, plus=None):
    """4-line FASTQ text of the reads; names[i] is the header without '@', quals[i] the quality line."""
    out = []
    for i, seq in enumerate(reads):
        name = names[i] if names else b"r%d" % i
        qual = quals[i] if quals else b"I" * len(seq)
        out.append(b"@" + name + eol + seq + eol + (plus[i] if plus else b"+") + eol + qual + eol)
    text = b"".join(out)
    return text if last_newline or not text else text[:-len(eol)]


# ------------------------------------------------------------------ the model against the reference and the rule
def test_the_model_equals_the_reference_on_the_bundled_fixtures(monkeypatch):
    monkeypatch.chdir(HERE)
    with open(os.path.join(HERE, "golden", "fixtures_children.json")) as fh:
        cases = json.load(fh)["min_cov"]
    assert len(cases) >= 5
    for g in cases:
        seq = ko.read_fasta_concat(g["target"]).encode("ascii")
        table, k, canonical = file_table(g["db"])
        kmer_nb, kmer_nb_0 = g["cov"][5], g["cov"][6]
        assert model_hits(fastq([seq]), table, k, canonical) == [kmer_nb - kmer_nb_0]
    seq = ko.read_fasta_concat("./data/catalog/GRCh38/FLT3-ITD_exons_13-15.fa").encode("ascii")
    table, k, canonical = file_table("./data/jf/03H112_IandI.jf")
    assert model_hits(fastq([seq]), table, k, canonical) == [315 - 0]


def test_the_model_on_cases_read_off_the_rule():
    table = {_pack(b"ACG"): 7, _pack(b"AAA"): 2, _pack(b"GGG"): 0}
    text = fastq([b"ACGT", b"", b"AC", b"ACNGT", b"acgt", b"TTTGGG"])
    assert model_hits(text, table, 3, True) == [2, 0, 0, 0, 2, 1]          # CGT's reverse complement is ACG; GGG counts 0
    assert model_hits(text, table, 3, False) == [1, 0, 0, 0, 1, 0]
    recs = [b"".join(r) for r in fastq_records(text)]
    assert recs[1] == b"@r1\n\n+\n\n"
    assert model_select(text, table, 3, True) == recs[0] + recs[4] + recs[5]
    assert model_select(text, table, 3, True, min_hits=2) == recs[0] + recs[4]
    assert model_select(text, table, 3, True, invert=True) == recs[1] + recs[2] + recs[3]
    assert model_select(text, table, 3, True, min_hits=3) == b""
    # quality masking: the G below '5' is no base any more
    assert model_hits(fastq([b"ACGT"], quals=[b"II4I"]), table, 3, True, min_qual=ord("5")) == [0]
    assert model_hits(fastq([b"ACGT"], quals=[b"II5I"]), table, 3, True, min_qual=ord("5")) == [2]
    # a last record without newline gets one; '\r' stays and is no base
    assert model_select(text[:-1], table, 3, True) == model_select(text, table, 3, True)
    crlf = fastq([b"ACGT", b"TT"], eol=b"\r\n")
    assert model_hits(crlf, table, 3, True) == [2, 0] and model_select(crlf, table, 3, True) == crlf[:len(crlf) // 2 + 2]
    for bad, kind, offset in ((b"r0\nAC\n+\nII\n", NO_AT, 0), (b"@r0\nAC\n-\nII\n", NO_PLUS, 7), (b"@r0\nAC\n+\nI\n", QUAL_LEN, 9),
                              (b"@r0\nAC\n+\nII\n@r1\nAC\n", TRUNCATED, 12)):
        with pytest.raises(Malformed) as e:
            model_hits(bad, table, 3, True)
        assert (e.value.kind, e.value.offset) == (kind, offset)


# ------------------------------------------------------------------ csrc/select_rule.h on the CPU
def rule_cases():
    """(name, k, canonical, min_hits, invert, min_qual, text, bait sequences): the shapes of tests/test_select.py,
    small enough for a sanitizer build."""
    rng = np.random.default_rng(17)
    out = []
    for k in (5, 31):
        lengths = [0, 1, k - 1, k, k + 1, 32, 33, 2047, 2048, 2049, 8191, 8192, 8193]
        reads = [random_bases(rng, n) for n in lengths]
        out.append(("lengths", k, True, 1, 0, 0, fastq(reads), reads[3::2]))
        out.append(("lengths -v", k, True, 1, 1, 0, fastq(reads, last_newline=False), reads[3::2]))
        # every pair of residues mod 16 of source and output offset: header lengths 0..15 twice over, every other kept
        reads = [random_bases(rng, 40) for _ in range(600)]
        names = [b"x" * int(n) for n in rng.integers(0, 16, 600)]
        out.append(("residues", k, False, 1, 0, 0, fastq(reads, names=names), reads[::2]))
        out.append(("residues, runs", k, True, 2, 0, 0, fastq(reads, names=names),
                    [r for i, r in enumerate(reads) if (i % 41) < (i // 41) + 1]))
        # records of 6 and 8 bytes: three or more per output word
        tiny = [b"", b"A"] * 200
        out.append(("tiny", k, True, 1, 1, 0, fastq(tiny, names=[b""] * 400), []))
        quals = [bytearray(b"I" * 60) for _ in range(300)]
        for q in quals:                                      # two bases of every read fall below the threshold
            for at in rng.integers(0, 60, 2):
                q[at] = 33 + int(rng.integers(0, 20))
        quals = [bytes(q) for q in quals]
        reads = [random_bases(rng, 60) for _ in range(300)]
        out.append(("quality", k, True, 1, 0, 53, fastq(reads, quals=quals, eol=b"\r\n", last_newline=False), reads[::3]))
    # the structured corpus of tests/test_text_kernels_every_k.py, a few KB of it, baited with every third of its reads
    import test_text_kernels_every_k as every_k
    for k in every_k.RULE_KS:
        reads = every_k.structured_reads(k, small=True)
        quals = every_k.structured_quals(k, reads)
        for canonical in (True, False):
            out.append(("structured", k, canonical, 1, 0, 0, fastq(reads), reads[::3]))
            out.append(("structured -v, quality", k, canonical, 2, 1, 43, fastq(reads, quals=quals, last_newline=False), reads[1::3]))
    return out


def rule_input(path, k, canonical, min_hits, invert, min_qual, table, stages, text):
    with open(path, "wb") as fh:
        fh.write(b"%d %d %d %d %d %d %d %d\n" % (k, canonical, min_hits, invert, min_qual, len(table), len(stages), len(text)))
        fh.write(b" ".join(b"%d" % v for v in stages) + b"\n")
        fh.write(b"".join(b"%d %d\n" % kv for kv in table.items()))
        fh.write(b"TEXT\n" + text)


def test_rule_program_under_sanitizers(tmp_path):
    """csrc/select_rule.h built for the CPU with AddressSanitizer + UBSan (tests/host/select_rule.cpp): record bounds
    from a line table, the hit walk of every lane, the sizes, offsets and gather arithmetic of every output word, into
    buffers of exactly the device buffers' sizes, at staging sizes 256, 4 096 and 16 MiB, against the model: the hits
    per record and the output, byte for byte."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "select_rule")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "host", "select_rule.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name, k, canonical, min_hits, invert, min_qual, text, baits in rule_cases():
        table = kmers_of(baits, k, canonical)
        longest = max(len(b"".join(r)) for r in fastq_records(text))
        stages = [s for s in (256, 4096, 1 << 24) if s >= longest]
        path = str(tmp_path / "in.bin")
        rule_input(path, k, int(canonical), min_hits, invert, min_qual, table, stages, text)
        proc = subprocess.run([exe, path], capture_output=True, env=env, timeout=600)
        assert proc.returncode == 0 and proc.stdout.endswith(b"SELECT RULE OK\n"), (name, k, proc.stdout[-500:], proc.stderr[-3000:])
        assert b"ERROR: AddressSanitizer" not in proc.stderr and b"runtime error" not in proc.stderr, proc.stderr[-3000:]
        hits = model_hits(text, table, k, canonical, min_qual)
        kept = model_select(text, table, k, canonical, min_hits, invert, min_qual)
        if k == 31 and name != "tiny" and "-v" not in name:
            assert 0 < len(kept) < len(text), name              # the case selects: some records, not all
        body = b"".join(b"%d\n" % h for h in hits) + b"OUT %d\n" % len(kept) + kept
        got = proc.stdout
        for stage in stages:
            head, _, got = got.partition(b"\n")
            words = head.split()
            assert words[:2] == [b"STAGE", b"%d" % stage] and words[4:] == [b"RECORDS", b"%d" % len(hits)], (name, k, head)
            assert int(words[3]) >= -(-len(text) // stage)
            if stage == 1 << 24:
                assert int(words[3]) == 1
            assert got.startswith(body), (name, k, stage)
            got = got[len(body):]
        assert got == b"SELECT RULE OK\n", (name, k)


# ------------------------------------------------------------------ the bait command without a GPU
def test_bait_arguments(tmp_path):
    fa = tmp_path / "t.fa"
    fa.write_text(">r\nACGT\n")
    p = cli.parse_args(["bait", "-t", str(fa), "-t", str(tmp_path), "-m", "21", "-n", "3", "-v", "-Q", "5", "-o", "o.fq", "a.fq", "b.fq.gz"])
    assert (p.targets, p.db, p.mer_len, p.min_hits, p.invert, p.min_qual_char, p.output, p.reads) == (
        [str(fa), str(tmp_path)], None, 21, 3, True, "5", "o.fq", ["a.fq", "b.fq.gz"])
    p = cli.parse_args(["bait", "-d", "db.jf", "-"])
    assert (p.targets, p.db, p.mer_len, p.min_hits, p.invert, p.min_qual_char, p.output, p.reads) == (
        [], "db.jf", None, 1, False, None, None, ["-"])
    assert cli.parse_args(["bait", "-t", str(fa), "a.fq"]).mer_len is None          # (31 where the table is built)
    for bad in (["bait", "-t", str(fa), "-d", "db.jf", "a.fq"], ["bait", "a.fq"], ["bait", "-d", "db.jf", "-m", "31", "a.fq"],
                ["bait", "-d", "db.jf"], ["bait", "-d", "db.jf", "-n", "0", "a.fq"], ["bait", "-d", "db.jf", "-Q", "ab", "a.fq"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(bad)
        assert e.value.code == 2, bad
