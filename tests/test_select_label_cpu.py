"""The labelled selection of FASTQ reads (km_select_labels_*, kmjf_fastq_label_hits, `bait --split-dir`) where no GPU is
needed: the model every labelled test compares with, csrc/select_label_rule.h driven on the CPU under AddressSanitizer +
UBSan, count.label_table and count.rows_labels, and the command's argument rules.

``model_label_hits`` and ``model_label_select`` are written from the rule of include/kmgpu.h alone, record by record and
window by window with a dict {key: mask} as the table; they share nothing with csrc/select_label_rule.h,
csrc/select_rule.h, csrc/scan_rule.h or km_amd.count._windows.  The records come from test_select_cpu.fastq_records."""
import io
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from km_amd import cli
from km_amd import count as kc
import test_select_cpu as sm

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_PAD, WORD = 16, 16                     # csrc/select_rule.h

fastq, random_bases, fastq_records = sm.fastq, sm.random_bases, sm.fastq_records


# ------------------------------------------------------------------ the model
def read_label_hits(seq, qual, table, k, canonical, n_labels, min_qual=0):
    """hits_l of one read for every l < n_labels: the windows of k bases (a base whose quality byte is below min_qual is
    none) whose k-mer's mask in `table` has bit l."""
    if min_qual:
        seq = bytes(b if q >= min_qual else 0x4E for b, q in zip(seq, qual))
    hits = [0] * n_labels
    for i in range(len(seq) - k + 1):
        w = seq[i:i + k]
        if w.translate(None, sm._BASES):
            continue
        key = sm._pack(w)
        if canonical:
            key = min(key, sm._pack(w.translate(sm._COMPLEMENT)[::-1]))
        mask = table.get(key, 0)
        for l in range(n_labels):
            hits[l] += (mask >> l) & 1
    return hits


def model_label_hits(text, table, k, canonical, n_labels, min_qual=0):
    """[n_labels][n_records]"""
    per_record = [read_label_hits(sm._content(s), sm._content(q), table, k, canonical, n_labels, min_qual)
                  for _, s, _, q in fastq_records(text)]
    return [[h[l] for h in per_record] for l in range(n_labels)]


def model_label_select(text, table, k, canonical, n_labels, min_hits=1, min_qual=0):
    """The bytes a final stream `text` leaves on each of the n_labels descriptors."""
    records = fastq_records(text)
    hits = model_label_hits(text, table, k, canonical, n_labels, min_qual)
    outs = []
    for l in range(n_labels):
        out = b"".join(b"".join(rec) for rec, h in zip(records, hits[l]) if h >= min_hits)
        outs.append(out + b"\n" if out and not out.endswith(b"\n") else out)
    return outs


def model_pieces(text, stage):
    """The pieces a final stream is cut into: all that is left if it fits a staging buffer, else the whole records
    within the next `stage` bytes."""
    records = [b"".join(r) for r in fastq_records(text)]
    pieces, i = [], 0
    while i < len(records):
        if sum(len(r) for r in records[i:]) <= stage:
            pieces.append(b"".join(records[i:]))
            break
        j, size = i, 0
        while size + len(records[j]) <= stage:
            size += len(records[j])
            j += 1
        assert j > i, "a record longer than a staging buffer"
        pieces.append(b"".join(records[i:j]))
        i = j
    return pieces


def model_streams(text, table, k, canonical, n_labels, stage, min_hits=1, min_qual=0):
    """Per piece of a final stream (label_off[0 .. n_labels], the records' (label, end offset) in the virtual stream)."""
    out = []
    for piece in model_pieces(text, stage):
        records = fastq_records(piece)
        hits = model_label_hits(piece, table, k, canonical, n_labels, min_qual)
        off, ends, at = [0], [], 0
        for l in range(n_labels):
            for rec, h in zip(records, hits[l]):
                if h >= min_hits:
                    at += len(b"".join(rec))
                    ends.append(at)
            off.append(at)
        out.append((off, ends))
    return out


def pass_cap(stage):
    return (stage + OUT_PAD) // WORD * WORD


def model_passes(text, table, k, canonical, n_labels, stage, min_hits=1, min_qual=0):
    """(gather_passes, the kinds of the pass boundaries met: "label" on a label boundary, "record" at another record's
    end, "inside" within a record)."""
    cap, passes, kinds = pass_cap(stage), 0, set()
    for off, ends in model_streams(text, table, k, canonical, n_labels, stage, min_hits, min_qual):
        total = off[-1]
        passes += max(1, -(-total // cap))
        for b in range(cap, total, cap):
            kinds.add("label" if b in off else "record" if b in ends else "inside")
    return passes, kinds


def model_any_multi(text, table, k, canonical, n_labels, min_hits=1, min_qual=0):
    hits = model_label_hits(text, table, k, canonical, n_labels, min_qual)
    kept = [sum(h[r] >= min_hits for h in hits) for r in range(len(hits[0]))] if hits and hits[0] else []
    return sum(c >= 1 for c in kept), sum(c >= 2 for c in kept)


def label_kmers(label_seqs, k, canonical):
    """{key: mask} of the valid windows of label l's sequences, for every l."""
    table = {}
    for l, seqs in enumerate(label_seqs):
        for key in sm.kmers_of(seqs, k, canonical):
            table[key] = table.get(key, 0) | (1 << l)
    return table


def test_the_model_on_cases_read_off_the_rule():
    pack = sm._pack
    table = {pack(b"ACG"): 0b01, pack(b"AAA"): 0b10, pack(b"CCC"): 0b11, pack(b"TTA"): 0b100}
    text = fastq([b"ACGT", b"AAAA", b"CCCAAA", b"", b"TTAC", b"acgt"])
    recs = [b"".join(r) for r in fastq_records(text)]
    # canonical: CGT's reverse complement is ACG; TTT's is AAA; GGG's is CCC; TTA/TAA: TAA is the smaller, so no hit
    assert model_label_hits(text, table, 3, True, 2) == [[2, 0, 1, 0, 0, 2], [0, 2, 2, 0, 0, 0]]
    assert model_label_hits(text, table, 3, False, 3) == [[1, 0, 1, 0, 0, 1], [0, 2, 2, 0, 0, 0], [0, 0, 0, 0, 1, 0]]
    # bit 2 is ignored in a 2-label run
    assert model_label_select(text, table, 3, False, 2) == [recs[0] + recs[2] + recs[5], recs[1] + recs[2]]
    assert model_label_select(text, table, 3, True, 2, min_hits=2) == [recs[0] + recs[5], recs[1] + recs[2]]
    assert model_any_multi(text, table, 3, False, 3) == (5, 1)
    # the last record without newline: only the output that holds it gains a byte
    outs = model_label_select(text[:-1], table, 3, False, 2)
    assert outs == [recs[0] + recs[2] + recs[5], recs[1] + recs[2]]
    # quality masking
    assert model_label_hits(fastq([b"ACGT"], quals=[b"II4I"]), table, 3, True, 1, min_qual=ord("5")) == [[0]]
    # pieces and passes: 4 records of 16 bytes, stage 32 -> 2 pieces; both labels keep everything -> 64 bytes a piece
    t4 = fastq([b"CCCA"] * 4, names=[b"nn"] * 4)
    assert [len(p) for p in model_pieces(t4, 32)] == [32, 32] and [len(p) for p in model_pieces(t4, 1 << 20)] == [64]
    assert model_passes(t4, table, 3, False, 2, 32) == (4, {"record"})         # cap 48: [0, 48) and [48, 64) of either piece
    assert model_passes(t4, table, 3, False, 2, 1 << 20) == (1, set())
    assert model_streams(t4, table, 3, False, 2, 32)[0] == ([0, 32, 64], [16, 32, 48, 64])


# ------------------------------------------------------------------ csrc/select_label_rule.h on the CPU
def seam_reads(rng, k=5):
    """Reads for the mask runs: a base read of distinct k-mers whose consecutive windows carry the masks A, A, B, AB, A,
    none, B, ... (A = bit 0, B = bit 1), copies of it behind headers of every length 0..63 so that every lane seam
    (window start = 31 / 0 mod 32 of the piece) falls at every position of the pattern, and short pieces of it whose
    hits_A and hits_B are small and differ -> (reads, names, table)."""
    pattern = (1, 1, 2, 3, 1, 0, 2)
    while True:
        base = random_bases(rng, 80)
        kmers = [sm._pack(base[i:i + k]) for i in range(len(base) - k + 1)]
        if len(set(kmers)) == len(kmers):
            break
    table = {key: pattern[i % len(pattern)] for i, key in enumerate(kmers) if pattern[i % len(pattern)]}
    reads, names = [], []
    for n in range(64):
        reads.append(base)
        names.append(b"h" * n)
    for start in range(0, 14):
        for length in (k, k + 1, k + 2, k + 3, k + 6):
            reads.append(base[start:start + length])
            names.append(b"s%d" % start)
    return reads, names, table, pattern


def label_rule_cases():
    """(name, k, canonical, n_labels, min_hits, min_qual, text, table, stages)"""
    rng = np.random.default_rng(23)
    out = []
    # 32 labels over reads of mixed lengths: every (source residue, output residue) at a label boundary
    reads = [random_bases(rng, int(n)) for n in rng.integers(20, 90, 2600)]
    names = [b"x" * int(n) for n in rng.integers(0, 16, 2600)]
    groups = [[r for i, r in enumerate(reads) if i % 37 in (l, (l * 5 + 3) % 37)] for l in range(32)]
    out.append(("32 labels, residues", 11, True, 32, 1, 0, fastq(reads, names=names), label_kmers(groups, 11, True), (4096,)))
    # three labels of a table that has bits above them, a last record without newline, quality masking
    quals = [bytes(33 + int(v) for v in rng.integers(5, 40, len(r))) for r in reads[:300]]
    table = label_kmers(groups[:5], 11, True)
    out.append(("3 of 5 labels, quality", 11, True, 3, 2, 43, fastq(reads[:300], names=names[:300], quals=quals, eol=b"\r\n",
                                                                     last_newline=False), table, (256, 4096, 1 << 20)))
    # the mask runs at every lane seam
    sreads, snames, stable, _ = seam_reads(rng)
    for min_hits in (1, 2, 3):
        out.append(("mask runs", 5, False, 2, min_hits, 0, fastq(sreads, names=snames), stable, (256, 4096, 1 << 20)))
    # passes: every read in all labels; a pass boundary inside a record, at a record's end and on a label boundary
    same = [random_bases(rng, 60) for _ in range(40)]
    everything = label_kmers([same] * 8, 31, True)
    out.append(("8 x everything", 31, True, 8, 1, 0, fastq(same), everything, (256, 4096)))
    # one record of 136 bytes in three labels at stage 256 (cap 272): label_off = 0, 136, 272, 408
    one = [random_bases(rng, 60)]
    out.append(("label boundary on a pass boundary", 31, True, 3, 1, 0, fastq(one, names=[b"n" * 10]),
                label_kmers([one] * 3, 31, True), (256,)))
    # a label without bytes between two that have some, two labels of equal content
    a, b = [random_bases(rng, 50) for _ in range(30)], [random_bases(rng, 50) for _ in range(30)]
    mixed = [r for pair in zip(a, b) for r in pair]
    out.append(("empty label, equal labels", 31, True, 4, 1, 0, fastq(mixed, last_newline=False),
                label_kmers([a, [], b, a], 31, True), (256, 4096)))
    return out


def label_rule_input(path, k, canonical, min_hits, min_qual, n_labels, table, stages, text):
    with open(path, "wb") as fh:
        fh.write(b"%d %d %d %d %d %d %d %d\n" % (k, canonical, min_hits, min_qual, n_labels, len(table), len(stages), len(text)))
        fh.write(b" ".join(b"%d" % v for v in stages) + b"\n")
        fh.write(b"".join(b"%d %d\n" % kv for kv in table.items()))
        fh.write(b"TEXT\n" + text)


def boundary_residues(text, table, k, canonical, n_labels, stage, min_hits):
    """{(source offset mod 16, output offset mod 16)} of the first kept record of a label, over the pieces."""
    seen = set()
    for piece in model_pieces(text, stage):
        records = fastq_records(piece)
        starts = np.concatenate(([0], np.cumsum([len(b"".join(r)) for r in records]))).tolist()
        hits = model_label_hits(piece, table, k, canonical, n_labels)
        at = 0
        for l in range(n_labels):
            kept = [r for r, h in enumerate(hits[l]) if h >= min_hits]
            if kept and l:
                seen.add((starts[kept[0]] % 16, at % 16))
            at += sum(starts[r + 1] - starts[r] for r in kept)
    return seen


def test_label_rule_program_under_sanitizers(tmp_path):
    """csrc/select_label_rule.h built for the CPU with AddressSanitizer + UBSan (tests/host/select_label_rule.cpp): the
    lane sink, the sizes, the one scan, the label offsets and every word of every gather pass with its w0, into buffers
    of exactly the device buffers' sizes, against the model: hits per label and record, the outputs byte for byte, the
    number of passes, and the records kept by any and by several labels."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "select_label_rule")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "host", "select_label_rule.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    kinds, residues, seams = set(), set(), set()
    for name, k, canonical, n_labels, min_hits, min_qual, text, table, stages in label_rule_cases():
        path = str(tmp_path / "in.bin")
        label_rule_input(path, k, int(canonical), min_hits, min_qual, n_labels, table, stages, text)
        proc = subprocess.run([exe, path], capture_output=True, env=env, timeout=600)
        assert proc.returncode == 0 and proc.stdout.endswith(b"SELECT LABEL RULE OK\n"), (name, proc.stdout[-300:], proc.stderr[-3000:])
        assert b"ERROR: AddressSanitizer" not in proc.stderr and b"runtime error" not in proc.stderr, proc.stderr[-3000:]
        hits = model_label_hits(text, table, k, canonical, n_labels, min_qual)
        outs = model_label_select(text, table, k, canonical, n_labels, min_hits, min_qual)
        any_, multi = model_any_multi(text, table, k, canonical, n_labels, min_hits, min_qual)
        got = proc.stdout
        for stage in stages:
            passes, met = model_passes(text, table, k, canonical, n_labels, stage, min_hits, min_qual)
            kinds |= met
            head, _, got = got.partition(b"\n")
            assert head == b"STAGE %d PIECES %d RECORDS %d PASSES %d ANY %d MULTI %d" % (
                stage, len(model_pieces(text, stage)), len(hits[0]), passes, any_, multi), (name, stage, head)
            for l in range(n_labels):
                head, _, got = got.partition(b"\n")
                kept = sum(h >= min_hits for h in hits[l])
                want = b"LABEL %d KEPT %d OUT %d HITS" % (l, kept, len(outs[l])) + b"".join(b" %d" % h for h in hits[l])
                assert head == want, (name, stage, l, head[:200], want[:200])
                assert got.startswith(outs[l]), (name, stage, l)
                got = got[len(outs[l]):]
        assert got == b"SELECT LABEL RULE OK\n", name
        if name == "32 labels, residues":
            residues = boundary_residues(text, table, k, canonical, n_labels, stages[0], min_hits)
            assert sum(len(o) > 0 for o in outs) == 32
        if name == "mask runs" and min_hits == 1:
            _, _, _, pattern = seam_reads(np.random.default_rng(0))
            for rec_start, (h, s, _, _) in zip(np.cumsum([0] + [len(b"".join(r)) for r in fastq_records(text)]), fastq_records(text)):
                for j in range(len(s) - 1 - k + 1):
                    if (rec_start + len(h) + j) % 32 in (0, 31):
                        seams.add(((rec_start + len(h) + j) % 32, j % len(pattern)))
            assert hits[0] != hits[1] and any(0 < a < 3 and 0 < b < 3 and a != b for a, b in zip(*hits))
    assert kinds == {"label", "record", "inside"}
    assert len(residues) == 256                                  # every source residue x every output residue
    assert len(seams) == 2 * 7                                   # either side of a lane seam at every pattern position


# ------------------------------------------------------------------ count.label_table and count.rows_labels
class _Db:
    """What label_table hands to Database.from_records, kept."""
    def __init__(self, keys, masks, k, canonical):
        self.keys, self.masks, self.k, self.canonical, self.device = keys, masks, k, canonical, None

    def upload(self, device):
        self.device = device
        return self

    def close(self):
        pass


def test_label_table_against_a_dict(monkeypatch):
    monkeypatch.setattr(kc._lib.Database, "from_records", classmethod(lambda cls, keys, masks, k, canonical: _Db(keys, masks, k, canonical)))
    rng = np.random.default_rng(5)
    label_keys = [np.concatenate(([999], rng.integers(0, 400, int(n)))).astype(np.uint64) for n in rng.integers(0, 120, 32)]
    label_keys[7] = np.array([999], np.uint64)                   # 999 is held by all 32 labels
    label_keys[9] = np.array([999, 3, 3], np.uint64)             # (a key twice in one label)
    want = {}
    for l, keys in enumerate(label_keys):
        for key in keys.tolist():
            want[key] = want.get(key, 0) | (1 << l)
    db = kc.label_table(label_keys, 21, True, device=0)
    assert (db.k, db.canonical, db.device) == (21, True, 0)
    assert db.keys.dtype == np.uint64 and db.masks.dtype == np.uint32
    assert dict(zip(db.keys.tolist(), db.masks.tolist())) == want and len(db.keys) == len(want)
    assert want[999] == 0xFFFFFFFF
    with pytest.raises(ValueError):
        kc.label_table([np.zeros(0, np.uint64)] * 33, 21, True)
    with pytest.raises(ValueError):
        kc.label_table([], 21, True)


def golden_cases():
    with open(os.path.join(HERE, "golden", "fixtures_tsv.json")) as fh:
        return json.load(fh)["cases"]


def canonical_kmers(seq, k):
    seq = seq.upper().encode("ascii")
    return set(sm.kmers_of([seq], k, True))


def test_rows_labels_on_the_golden_rows(tmp_path):
    cases = golden_cases()[:5]
    want = [("NPM1_4ins_exons_10-11utr", "Insertion", 30, 26), ("FLT3-ITD_exons_13-15", "ITD", 30, 0),
            ("FLT3-ITD_exons_13-15", "ITD", 32, 0), ("FLT3-TKD_exon_20", "Deletion", 28, 31),
            ("DNMT3A_R882_exon_23", "Substitution", 31, 31)]
    for case, (query, kind, n_alt, n_ref) in zip(cases, want):
        text = "\n".join(case["lines"]) + "\n"
        labels = kc.rows_labels(io.StringIO(text), 31, with_ref=True)
        assert [(lab["name"], lab["allele"], lab["keys"].size) for lab in labels] == [
            ("01_%s_%s.alt" % (query, kind), "alt", n_alt), ("01_%s_%s.ref" % (query, kind), "ref", n_ref)]
        row = [ln.split("\t") for ln in case["lines"] if not ln.startswith("#") and ln.split("\t")[2] == kind and ln.endswith("vs_ref")][0]
        assert (labels[0]["query"], labels[0]["type"], labels[0]["variant_name"]) == (row[1], row[2], row[3])
        alt, ref = canonical_kmers(row[8], 31), canonical_kmers(row[10], 31)
        assert set(labels[0]["keys"].tolist()) == alt - ref and set(labels[1]["keys"].tolist()) == ref - alt
        assert labels[0]["keys"].dtype == np.uint64 and labels[0]["keys"].tolist() == sorted(alt - ref)
        # from a path, without the .ref labels, and the cluster rows through -i
        path = tmp_path / "rows.tsv"
        path.write_text(text)
        assert [lab["name"] for lab in kc.rows_labels(str(path), 31)] == ["01_%s_%s.alt" % (query, kind)]
        cluster = kc.rows_labels(str(path), 31, info="cluster")
        assert len(cluster) == 1 and cluster[0]["keys"].size > 0
        assert len(kc.rows_labels(str(path), 31, info="cluster|vs_ref")) == 2
        assert kc.rows_labels(str(path), 31, info="no such info") == []
    # several rows: numbered from 1 among the taken rows, names made safe
    lines = [ln for case in cases for ln in case["lines"]]
    names = [lab["name"] for lab in kc.rows_labels(io.StringIO("\n".join(lines)), 31)]
    assert names == ["%02d_%s_%s.alt" % (i + 1, q, t) for i, (q, t, _, _) in enumerate(want)]
    odd = "\n".join(cases[0]["lines"]).replace("NPM1_4ins_exons_10-11utr", "a b/c:d")
    assert kc.rows_labels(io.StringIO(odd), 31)[0]["name"] == "01_a_b_c_d_Insertion.alt"
    # k = 21 differs from k = 31: the TSV does not record its k
    assert kc.rows_labels(io.StringIO("\n".join(cases[0]["lines"])), 21)[0]["keys"].size != 30


def test_more_than_32_labels_is_refused():
    cases = golden_cases()[:5]
    head = [ln for ln in cases[0]["lines"] if ln.startswith("#") or ln.startswith("Database")]
    rows = [ln for case in cases for ln in case["lines"] if ln.endswith("vs_ref") and "\tReference\t" not in ln]
    assert len(rows) == 5
    text = "\n".join(head + rows * 7)                            # 35 rows
    with pytest.raises(ValueError) as e:
        kc.rows_labels(io.StringIO(text), 31)
    assert "35" in str(e.value) and "split" in str(e.value)
    text = "\n".join(head + rows * 4)                            # 20 rows: fine alone, 40 labels with the references
    assert len(kc.rows_labels(io.StringIO(text), 31)) == 20
    with pytest.raises(ValueError) as e:
        kc.rows_labels(io.StringIO(text), 31, with_ref=True)
    assert "20" in str(e.value) and "40" in str(e.value) and "split" in str(e.value)
    assert len(kc.rows_labels(io.StringIO("\n".join(head + rows * 3 + rows[:1])), 31, with_ref=True)) == 32


# ------------------------------------------------------------------ bait --split-dir without a GPU
def test_bait_split_arguments(tmp_path):
    fa = tmp_path / "t.fa"
    fa.write_text(">r\nACGT\n")
    p = cli.parse_args(["bait", "--split-dir", "d", "-t", str(fa), "-t", str(tmp_path), "-m", "21", "-n", "3", "-Q", "5", "a.fq", "b.fq.gz"])
    assert (p.split_dir, p.targets, p.rows, p.with_ref, p.info, p.mer_len, p.min_hits, p.min_qual_char, p.reads) == (
        "d", [str(fa), str(tmp_path)], None, False, None, 21, 3, "5", ["a.fq", "b.fq.gz"])
    p = cli.parse_args(["bait", "--split-dir", "d", "--rows", "r.tsv", "--with-ref", "-i", "cluster", "-"])
    assert (p.split_dir, p.targets, p.rows, p.with_ref, p.info, p.mer_len, p.reads) == ("d", [], "r.tsv", True, "cluster", None, ["-"])
    assert cli.parse_args(["bait", "--split-dir", "d", "--rows", "-", "-m", "25", "a.fq"]).mer_len == 25
    split = ["bait", "--split-dir", "d", "-t", str(fa)]
    for bad in (split + ["-v", "a.fq"], split + ["-o", "o.fq", "a.fq"], split + ["-O", "o2.fq", "a.fq"],
                ["bait", "--split-dir", "d", "-d", "db.jf", "a.fq"], split + ["-d", "db.jf", "a.fq"],
                split + ["-1", "a.fq", "-2", "b.fq"], split + ["-1", "a.fq", "r.fq"], split + ["-2", "b.fq", "r.fq"],
                ["bait", "--rows", "r.tsv", "a.fq"], ["bait", "--rows", "r.tsv", "-t", str(fa), "a.fq"],
                split + ["--rows", "r.tsv", "a.fq"], ["bait", "--split-dir", "d", "a.fq"], split,
                ["bait", "--split-dir", "d", "--rows", "-", "-"], ["bait", "--split-dir", "d", "--rows", "-", "a.fq", "-"],
                split + ["--with-ref", "a.fq"], split + ["-i", "vs_ref", "a.fq"], ["bait", "-t", str(fa), "--with-ref", "a.fq"],
                split + ["-n", "0", "a.fq"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(bad)
        assert e.value.code == 2, bad
    assert "does not record" in cli.build_parser()._subparsers._group_actions[0].choices["bait"].format_help()


def test_split_labels_of_targets(tmp_path):
    catalog = os.path.join(HERE, "data", "catalog", "GRCh38")
    args = cli.parse_args(["bait", "--split-dir", "d", "-t", catalog, "a.fq"])
    k, labels = cli.split_labels(args)
    files = cli.list_target_files([catalog])
    assert k == 31 and [lab["name"] for lab in labels] == [os.path.splitext(os.path.basename(f))[0] for f in files]
    assert len(labels) == 9 and all(lab["allele"] == "target" and lab["query"] == lab["type"] == lab["variant_name"] == "" for lab in labels)
    for lab, f in zip(labels, files):                           # record by record, as `bait -t` counts them
        with open(f, "rb") as fh:
            records = [b"".join(part.split(b"\n")[1:]) for part in fh.read().split(b">")[1:]]
        assert lab["keys"].tolist() == sorted(sm.kmers_of(records, 31, True))
    other = tmp_path / "sub"
    other.mkdir()
    shutil.copy(files[0], other / os.path.basename(files[0]))
    args = cli.parse_args(["bait", "--split-dir", "d", "-t", files[0], "-t", str(other), "a.fq"])
    with pytest.raises(ValueError) as e:
        cli.split_labels(args)
    assert "one stem" in str(e.value)
    # a usage error of the command: exit status through main_bait's own way out
    with pytest.raises(SystemExit) as e:
        cli.main_bait(args, err=io.StringIO())
    assert "one stem" in str(e.value)
