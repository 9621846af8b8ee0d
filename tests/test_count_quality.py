"""Quality masking with FASTQ parsed on the GPU (km_counter_add_fastq, Counter.add_fastq, `count -Q CHAR`).

Every comparison is exact and covers the full record set.  The model is written from the definition (DESIGN.md
§10 "Quality masking, FASTQ on the device"): the text is split into lines in Python, a '\\r' at a line's end is
dropped, a base whose quality byte is below Q becomes N, and the reads go through sliding windows over bytes, a
break at every byte outside ACGTacgt, 2-bit keys, oracle.jf_reader.canonical_np and np.unique.  It shares no
code with the kernels or with km_fastq_cut."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from km_amd import lib as kmlib
from oracle import jf_reader as jr
from oracle import km_oracle as ko

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLT3 = os.path.join(HERE, "data", "catalog", "GRCh38", "FLT3-ITD_exons_13-15.fa")
E_FORMAT, E_STATE, E_CAPACITY = 2, 7, 8

_CODE = np.full(256, 4, np.uint8)
for _ch, _c in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
    _CODE[_ch] = _c
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
ACGT = np.frombuffer(b"ACGT", np.uint8)


# ------------------------------------------------------------------ the model
def model(data, k, canonical):
    """(keys sorted, counts) of every window of k bases in `data` (bytes); any other byte is a break."""
    codes = _CODE[np.frombuffer(bytes(data), np.uint8)]
    n = codes.size - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    keys = np.zeros(n, np.uint64)
    bad = np.zeros(n, bool)
    for j in range(k):
        c = codes[j:j + n]
        bad |= c > 3
        keys = (keys << np.uint64(2)) | (c & 3).astype(np.uint64)
    keys = keys[~bad]
    if canonical:
        keys = jr.canonical_np(keys, k)
    u, c = np.unique(keys, return_counts=True)
    return u, c.astype(np.uint32)


def fastq_lines(text):
    """[(offset, line without newline and without a '\\r' before it)]; the last line needs no newline."""
    out, pos = [], 0
    for raw in text.split(b"\n"):
        out.append((pos, raw[:-1] if raw.endswith(b"\r") else raw))
        pos += len(raw) + 1
    if not text or text.endswith(b"\n"):                    # what split leaves behind the last newline is no line
        out.pop()
    return out


def masked_reads(text, q):
    """The sequence lines of well-formed 4-line FASTQ, a base with quality byte < q turned into N."""
    lines = fastq_lines(text)
    assert len(lines) % 4 == 0
    reads = []
    for r in range(0, len(lines), 4):
        head, seq, plus, qual = (ln for _, ln in lines[r:r + 4])
        assert head[:1] == b"@" and plus[:1] == b"+" and len(seq) == len(qual)
        s = np.frombuffer(seq, np.uint8).copy()
        s[np.frombuffer(qual, np.uint8) < q] = ord("N")
        reads.append(s.tobytes())
    return reads


def model_fastq(text, q, k, canonical):
    return model(b"\n".join(masked_reads(text, q)), k, canonical)


def model_first_fault(text):
    """Byte offset of the first line that breaks the 4-line structure, or None."""
    lines = fastq_lines(text)
    for i, (off, ln) in enumerate(lines):
        if i % 4 == 0 and ln[:1] != b"@":
            return off
        if i % 4 == 2 and ln[:1] != b"+":
            return off
        if i % 4 == 3 and len(ln) != len(lines[i - 2][1]):
            return off
    return lines[len(lines) // 4 * 4][0] if len(lines) % 4 else None


def sorted_records(counter):
    keys, counts = counter.records()
    order = np.argsort(keys, kind="stable")
    return keys[order], counts[order]


def same(a, b):
    return a[0].dtype == b[0].dtype and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def feed(counter, text, q, step=None):
    """The text through add_fastq: in one final call, or in calls of `step` new bytes with the tail carried."""
    if step is None:
        assert counter.add_fastq(text, final=True, min_qual_char=q) == len(text)
        return
    pos, tail = 0, b""
    while pos < len(text):
        buf = tail + text[pos:pos + step]
        pos += step
        used = counter.add_fastq(buf, final=False, min_qual_char=q)
        assert used <= len(buf)
        tail = buf[used:]
    assert counter.add_fastq(tail, final=True, min_qual_char=q) == len(tail)


def count_fastq(text, q, k=31, canonical=True, step=None):
    c = kmlib.Counter(k=k, canonical=canonical)
    try:
        feed(c, text, q, step)
        stats = c.stats()
        c.finish().close()
        return sorted_records(c), stats
    finally:
        c.close()


# ------------------------------------------------------------------ the text
def qualities(rng, n):
    """Bytes in '!'..'I' with runs of low values."""
    q = rng.integers(ord("5"), ord("I") + 1, n).astype(np.uint8)
    at = 0
    while at < n:
        at += int(rng.integers(5, 60))
        run = int(rng.integers(1, 12))
        q[at:at + run] = rng.integers(ord("!"), ord("5"), max(0, min(n, at + run) - min(n, at)))
        at += run
    return q


def record(name, seq, qual, nl=b"\n", plus=b"+"):
    return b"@" + name + nl + seq + nl + plus + nl + qual + nl


@functools.lru_cache(maxsize=None)
def small_text():
    """300 reads of 20-120 nt from a 2 kb genome, and the special records; the last one has no newline."""
    rng = np.random.default_rng(61)
    genome = ACGT[rng.integers(0, 4, 2000)]
    recs = []
    for i in range(300):
        ln = int(rng.integers(20, 121))
        a = int(rng.integers(0, 2000 - ln + 1))
        seq = genome[a:a + ln].tobytes()
        if rng.integers(2):
            seq = seq.translate(_COMP)[::-1]
        recs.append(record(b"read%d len=%d" % (i, ln), seq, qualities(rng, ln).tobytes(),
                           plus=b"+read%d" % i if i % 7 == 0 else b"+"))
    g = genome.tobytes()
    special = [
        record(b"short", g[5:15], b"IIIIIIIIII"),                                    # shorter than k = 31
        record(b"empty", b"", b""),
        record(b"at", g[100:160], b"@" + b"I" * 59),                                 # quality starts with '@'
        record(b"at_plus", g[300:350], b"@+" + b"5" * 48),
        record(b"plus", g[350:400], b"+" + b"I" * 49),
        record(b"n_lower", g[500:540] + b"N" + g[541:580].lower() + b"n" + g[581:640], b"I" * 140),
        record(b"low_n", g[700:800], b"I" * 40 + b"*" + b"I" * 59),                  # one base below '+'
    ]
    for j, s in enumerate(special):
        recs.insert(40 * (j + 1), s)
    last = record(b"last", g[900:1000], b"I" * 50 + b"!" + b"I" * 49)
    text = b"".join(recs) + last[:-1]
    assert not text.endswith(b"\n")
    return text, max(len(r) for r in recs + [last])


QS = [0, ord("+"), ord("5"), ord("J")]


@functools.lru_cache(maxsize=None)
def small_want(q, k, canonical):
    return model_fastq(small_text()[0], q, k, canonical)


# ------------------------------------------------------------------ masking against the model
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [31, 5])
@pytest.mark.parametrize("q", QS)
def test_masking_equals_the_model(q, k, canonical):
    text, _ = small_text()
    want = small_want(q, k, canonical)
    got, stats = count_fastq(text, q, k, canonical)
    assert same(got, want)
    assert stats["kmers"] == int(want[1].sum(dtype=np.uint64)) and stats["distinct"] == want[0].size
    if q == ord("J"):
        assert want[0].size == 0 and stats["bases"] == 0
    if q == ord("+") and k == 31:
        assert not same(want, small_want(0, k, canonical))          # the masked bases do change the records


def test_q0_equals_the_host_path():
    text, _ = small_text()
    host = kmlib.Counter(k=31)
    assert host.add_text(text, final=True) == len(text)
    host.finish().close()
    got, _ = count_fastq(text, 0)
    assert same(got, sorted_records(host))
    host.close()


# ------------------------------------------------------------------ piece and tile boundaries
@pytest.mark.parametrize("stage", ["4096", "longest record"])
def test_small_staging_buffers_and_small_calls(monkeypatch, stage):
    text, longest = small_text()
    assert longest >= 256
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(longest) if stage == "longest record" else stage)
    for q in (0, ord("+")):
        want = small_want(q, 31, True)
        for step in (None, 1000, longest + 1):
            got, stats = count_fastq(text, q, step=step)
            assert same(got, want), (q, step)
            assert stats["kmers"] == int(want[1].sum(dtype=np.uint64))


def test_default_staging_small_calls():
    text, longest = small_text()
    want = small_want(ord("5"), 31, True)
    for step in (1000, longest + 1):
        assert same(count_fastq(text, ord("5"), step=step)[0], want), step


def test_three_megabytes_many_tiles_per_piece():
    """30 000 records in one piece of the default staging: 700 tiles, the quality line of a record in a later
    tile than its sequence for most tiles' last records."""
    rng = np.random.default_rng(62)
    genome = ACGT[rng.integers(0, 4, 50_000)]
    n, ln = 30_000, 44
    starts = rng.integers(0, genome.size - ln + 1, n)
    reads = genome[starts[:, None] + np.arange(ln)[None, :]]
    qual = rng.integers(ord("!"), ord("J"), (n, ln)).astype(np.uint8)
    qual[rng.random((n, ln)) < 0.9] = ord("I")
    recs = [record(b"r%d" % i, reads[i].tobytes(), qual[i].tobytes()) for i in range(n)]
    text = b"".join(recs)
    assert 2_900_000 < len(text) < 3_200_000
    want = model_fastq(text, ord("+"), 31, True)
    got, stats = count_fastq(text, ord("+"))
    assert same(got, want)
    assert stats["kmers"] == int(want[1].sum(dtype=np.uint64)) and stats["distinct"] == want[0].size


def test_crlf_gives_the_same_records(monkeypatch):
    text, _ = small_text()
    crlf = text.replace(b"\n", b"\r\n")
    for q in (0, ord("+")):
        assert same(count_fastq(crlf, q)[0], small_want(q, 31, True))
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")
    assert same(count_fastq(crlf, ord("+"), step=1000)[0], small_want(ord("+"), 31, True))


# ------------------------------------------------------------------ errors
def plain_records(n=40, ln=100):
    rng = np.random.default_rng(63)
    return [(b"rec%d" % i, ACGT[rng.integers(0, 4, ln)].tobytes(), qualities(rng, ln).tobytes()) for i in range(n)]


def faulty_text(kind, at=25):
    parts = []
    for i, (name, seq, qual) in enumerate(plain_records()):
        rec = record(name, seq, qual)
        if i == at:
            if kind == "no plus":
                rec = b"@" + name + b"\n" + seq + b"\n" + qual + b"\n"
            elif kind == "no at":
                rec = b"X" + rec[1:]
            elif kind == "short quality":
                rec = record(name, seq, qual[:-1])
            elif kind == "blank line":
                rec = b"\n" + rec
        parts.append(rec)
    return b"".join(parts)


@pytest.mark.parametrize("kind", ["no plus", "no at", "short quality", "blank line"])
def test_format_errors_surface_at_stats_with_the_stream_offset(monkeypatch, kind):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")
    text = faulty_text(kind)
    where = model_first_fault(text)
    assert 4096 + 500 < where < 2 * 4096 - 1200                      # inside the second piece, away from its ends
    for step in (None, 3000):
        c = kmlib.Counter(k=31)
        try:
            if step is None:
                c.add_fastq(text, final=True, min_qual_char="+")
            else:                                                    # the offset counts over the calls of a stream
                used = c.add_fastq(text[:step], final=False, min_qual_char="+")
                assert 0 < used <= step
                c.add_fastq(text[used:], final=True, min_qual_char="+")
            with pytest.raises(kmlib.KmError) as e:
                c.stats()
            assert e.value.code == E_FORMAT
            if kind != "blank line":
                assert ("offset %d" % where) in str(e.value), (str(e.value), where)
            for call in (lambda: c.finish(), lambda: c.stats(), lambda: c.add_bases(b"ACGT"),
                         lambda: c.add_fastq(b"", final=True)):
                with pytest.raises(kmlib.KmError) as e:
                    call()
                assert e.value.code == E_FORMAT
        finally:
            c.close()


def test_well_formed_text_reports_nothing():
    assert model_first_fault(faulty_text("none")) is None
    got, _ = count_fastq(faulty_text("none"), ord("+"))
    assert same(got, model_fastq(faulty_text("none"), ord("+"), 31, True))


def test_capacity_state_and_argument_errors(monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "256")
    c = kmlib.Counter(k=31)
    ok = record(b"a", b"ACGT" * 10, b"I" * 40)
    long = record(b"long", b"ACGT" * 75, b"I" * 300)
    with pytest.raises(kmlib.KmError) as e:
        c.add_fastq(ok + long + ok, final=True)
    assert e.value.code == E_CAPACITY and ("offset %d" % len(ok)) in str(e.value)
    c.close()
    monkeypatch.delenv("KM_COUNT_STAGE_BYTES")
    c = kmlib.Counter(k=31)
    for bad in (-1, 256):
        with pytest.raises(kmlib.KmError) as e:
            c.add_fastq(ok, final=True, min_qual_char=bad)
        assert e.value.code == 4
    assert c.add_fastq(b"", final=False) == 0
    assert c.add_fastq(ok + ok[:7], final=False) == len(ok)
    c.finish().close()
    with pytest.raises(kmlib.KmError) as e:
        c.add_fastq(ok, final=True)
    assert e.value.code == E_STATE
    c.close()


# ------------------------------------------------------------------ mixed calls
def test_add_bases_add_fastq_add_text_on_one_counter():
    rng = np.random.default_rng(64)
    text, _ = small_text()
    bases = ACGT[rng.integers(0, 4, 5000)].tobytes()
    fasta = b">x\n" + bases[100:900] + b"\n" + bases[2000:2400] + b"\n>y\n" + bases[3000:3100] + b"\n"
    stream = b"\n".join([bases] + masked_reads(text, ord("+")) + [bases[100:900] + bases[2000:2400], bases[3000:3100]])
    want = model(stream, 31, True)
    c = kmlib.Counter(k=31)
    c.add_bases(bases)
    feed(c, text, ord("+"), step=5000)
    assert c.add_text(fasta, final=True) == len(fasta)
    stats = c.stats()
    c.finish().close()
    assert same(sorted_records(c), want) and stats["kmers"] == int(want[1].sum(dtype=np.uint64))
    c.close()


# ------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def itd_fastq(seed=65, depth=120, read_len=100, fraction=0.3):
    """FASTQ of reads tiling the FLT3 target; a fraction carries a 30-nt tandem duplication, and in half of the
    reads that cover its junction the four bases around the junction have quality '!'."""
    rng = np.random.default_rng(seed)
    ref = ko.read_fasta_concat(FLT3)
    p = 150
    itd = ref[:p + 30] + ref[p:p + 30] + ref[p + 30:]
    junction = 100 + p + 30                                 # in the padded source: first base of the second copy
    pad = "".join("ACGT"[i] for i in rng.integers(0, 4, 200))
    recs = []
    for i in range(depth * (len(ref) + 2 * read_len) // read_len):
        dup = rng.random() < fraction
        src = pad[:100] + (itd if dup else ref) + pad[100:]
        a = int(rng.integers(0, len(src) - read_len + 1))
        seq = src[a:a + read_len].encode()
        qual = np.full(read_len, ord("I"), np.uint8)
        if dup and a <= junction - 2 and junction + 2 <= a + read_len and rng.integers(2):
            qual[junction - 2 - a:junction + 2 - a] = ord("!")
        if rng.integers(2):
            seq, qual = seq.translate(_COMP)[::-1], qual[::-1]
        recs.append(record(b"read%d" % i, seq, qual.tobytes()))
    return ref, b"".join(recs)


def oracle_rows(ref, text, q, db_name):
    keys, counts = model_fastq(text, q, 31, True)
    keep = counts >= 2
    keys, counts = keys[keep], counts[keep]
    cpu = ko.KmerDB(records={"k": 31, "canonical": True, "keys": keys, "counts": counts}, cutoff=0.05, n_cutoff=5)
    rows = ko.target_rows(ko.analyse_target(ref, "FLT3-ITD_exons_13-15", cpu), db_name)
    assert any(r.split("\t")[2] == "ITD" for r in rows), rows
    return rows, keys, counts


def run_cli(tmp_path, *args):
    env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, "-m", "km_amd"] + list(args), cwd=tmp_path, capture_output=True, text=True,
                         timeout=300, env=env)
    assert res.returncode == 0, res.stderr
    return res


def find_mutation_rows(tmp_path, jf):
    res = run_cli(tmp_path, "find_mutation", FLT3, jf)
    body = [ln for ln in res.stdout.splitlines() if not ln.startswith("#")]
    assert body[0].startswith("Database\t")
    return body[1:]


def test_cli_count_with_q_then_find_mutation(tmp_path):
    ref, text = itd_fastq()
    (tmp_path / "reads.fq").write_bytes(text)
    res = run_cli(tmp_path, "count", "-m", "31", "-C", "-Q", "+", "-L", "2", "-o", "x.jf", "reads.fq")
    stats = dict(line[1:].split(":", 1) for line in res.stderr.splitlines() if line.startswith("#"))
    full = model_fastq(text, ord("+"), 31, True)
    assert stats["min_qual_char"] == "+"
    assert int(stats["kmers"]) == int(full[1].sum(dtype=np.uint64)) and int(stats["distinct"]) == full[0].size
    want, keys, counts = oracle_rows(ref, text, ord("+"), "x.jf")
    rec = jr.read_jf(str(tmp_path / "x.jf"))
    assert np.array_equal(rec["keys"], keys) and np.array_equal(rec["counts"], counts)
    cmdline = rec["header"]["cmdline"]
    assert cmdline[cmdline.index("-Q") + 1] == "+"
    assert find_mutation_rows(tmp_path, "x.jf") == want
    assert want != oracle_rows(ref, text, 0, "x.jf")[0]              # the masked junction bases change the rows


def test_cli_count_with_q_in_jellyfish_order(tmp_path):
    ref, text = itd_fastq()
    (tmp_path / "reads.fq").write_bytes(text)
    run_cli(tmp_path, "count", "-m", "31", "-C", "-Q", "+", "-L", "2", "--jellyfish-order", "-o", "y.jf", "reads.fq")
    _, keys, counts = oracle_rows(ref, text, ord("+"), "y.jf")
    rec = jr.read_jf(str(tmp_path / "y.jf"))
    order = np.argsort(rec["keys"], kind="stable")
    assert np.array_equal(rec["keys"][order], keys) and np.array_equal(rec["counts"][order], counts)
    cmdline = rec["header"]["cmdline"]
    assert cmdline[cmdline.index("-Q") + 1] == "+" and "--jellyfish-order" in cmdline


def test_cli_count_without_q_gives_the_unmasked_rows(tmp_path):
    ref, text = itd_fastq()
    (tmp_path / "reads.fq").write_bytes(text)
    res = run_cli(tmp_path, "count", "-m", "31", "-C", "-L", "2", "-o", "plain.jf", "reads.fq")
    assert "min_qual_char" not in res.stderr
    want, keys, counts = oracle_rows(ref, text, 0, "plain.jf")
    rec = jr.read_jf(str(tmp_path / "plain.jf"))
    assert np.array_equal(rec["keys"], keys) and np.array_equal(rec["counts"], counts)
    assert find_mutation_rows(tmp_path, "plain.jf") == want
