"""The selection of FASTQ reads on the GPU: lib.Selector (km_select_*), Database.fastq_hits (kmjf_fastq_hits),
count.select_files and `python -m km_amd bait`.

Every comparison is exact, integers equal and output byte-identical, against model_hits / model_select of
tests/test_select_cpu.py, which are written from the rule of include/kmgpu.h and pinned there to the reference's answers.
The sizes are the ends of what a lane of the hit walk (32 window starts), a wave (2 048) and a block (8 192) own, a lane
(16 bytes) and a tile (4 096) of the line table, and the 16-byte words of the gather."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from km_amd import lib as kmlib
from oracle import km_oracle as ko
import test_select_cpu as sm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CATALOG = os.path.join(HERE, "data", "catalog", "GRCh38")
FLT3 = os.path.join(CATALOG, "FLT3-ITD_exons_13-15.fa")
IANDI = os.path.join(HERE, "data", "jf", "03H112_IandI.jf")
KM_E_IO, KM_E_FORMAT, KM_E_ARG, KM_E_STATE, KM_E_CAPACITY = 1, 2, 4, 7, 8
EDGES = (15, 16, 17, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)
COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")

pytestmark = pytest.mark.gpu

fastq, random_bases, model_hits, model_select, kmers_of = sm.fastq, sm.random_bases, sm.model_hits, sm.model_select, sm.kmers_of


# ------------------------------------------------------------------ helpers
def make_db(table, k, canonical):
    keys = np.fromiter(table.keys(), np.uint64, len(table))
    counts = np.fromiter(table.values(), np.uint32, len(table))
    return kmlib.Database.from_records(keys, counts, k, canonical).upload(0)


def select(db, streams, min_hits=1, invert=False, min_qual=None, cuts=None):
    """The streams (bytes each) through one Selector into one descriptor, a stream in one final call or, with `cuts`
    (ascending offsets into the one stream), block by block with the unconsumed tail carried forward
    -> (the descriptor's bytes, stats, the sum of what the calls consumed)."""
    if isinstance(streams, bytes):
        streams = [streams]
    consumed = 0
    with tempfile.TemporaryFile() as fh:
        with kmlib.Selector(db, fh, min_hits=min_hits, invert=invert, min_qual_char=min_qual) as sel:
            for text in streams:
                if cuts is None:
                    consumed += sel.add_fastq(text, final=True)
                    continue
                tail = b""
                for a, b in zip([0] + list(cuts), list(cuts) + [len(text)]):
                    buf = tail + text[a:b]
                    used = sel.add_fastq(buf, final=False)
                    assert used <= len(buf)
                    consumed += used
                    tail = buf[used:]
                consumed += sel.add_fastq(tail, final=True)
            stats = sel.stats()
        fh.seek(0)
        return fh.read(), stats, consumed


def check(db, text, table, k, canonical, min_hits=1, invert=False, min_qual=None, ctx=None):
    """Selector and fastq_hits of one final stream against the model -> the output."""
    q = sm_qual(min_qual)
    want_hits = model_hits(text, table, k, canonical, q)
    got_hits = db.fastq_hits(text, min_qual_char=min_qual)
    assert got_hits.dtype == np.uint32 and got_hits.tolist() == want_hits, (ctx, [(i, g, w) for i, (g, w) in enumerate(zip(got_hits.tolist(), want_hits)) if g != w][:5])
    want = model_select(text, table, k, canonical, min_hits, invert, q)
    got, stats, consumed = select(db, text, min_hits, invert, min_qual)
    assert got == want, (ctx, len(got), len(want))
    assert consumed == len(text)
    kept = sum(1 for h in want_hits if (h >= min_hits) != bool(invert))
    assert stats == {"records_in": len(want_hits), "records_out": kept, "bytes_in": len(text), "bytes_out": len(want),
                     "pieces": stats["pieces"]}, ctx
    return got


def sm_qual(min_qual):
    return 0 if min_qual is None else kmlib._qual_byte(min_qual)


def greedy_pieces(text, stage):
    """The pieces a final stream is cut into: what is left if it fits `stage` bytes, else as many whole records as do
    -> their texts."""
    recs = [b"".join(r) for r in sm.fastq_records(text)]
    left = len(text)
    pieces, i = [], 0
    while i < len(recs):
        if left <= stage:
            pieces.append(b"".join(recs[i:]))
            break
        cur = b""
        while len(cur) + len(recs[i]) <= stage:
            cur += recs[i]
            i += 1
        assert cur, "a record longer than a buffer"
        pieces.append(cur)
        left -= len(cur)
    assert b"".join(pieces) == text
    return pieces


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("k", [31, 5])
def test_read_lengths(monkeypatch, k):
    monkeypatch.setenv("KM_SELECT_TIME", "1")
    rng = np.random.default_rng(k)
    lengths = [0, 1, k - 1, k, k + 1, 32, 33, 2047, 2048, 2049, 8191, 8192, 8193]
    reads = [random_bases(rng, n) for n in lengths]
    table = kmers_of([r[:n // 2 + k] for r, n in zip(reads, lengths)][3::2], k, True)
    db = make_db(table, k, True)
    try:
        out = check(db, fastq(reads), table, k, True, ctx="all")
        assert 0 < len(out)
        alone = [check(db, fastq([r], names=[b"r%d" % i]), table, k, True, ctx=n) for i, (r, n) in enumerate(zip(reads, lengths))]
        assert b"".join(alone) == out
        ms = kmlib.select_kernel_ms()
        assert ms["front"] > 0 and ms["hits"] > 0 and ms["sizes"] > 0 and ms["gather"] > 0
        monkeypatch.delenv("KM_SELECT_TIME")                # not asked for: no events, no figures
        check(db, fastq(reads), table, k, True, ctx="untimed")
        assert kmlib.select_kernel_ms() == {"front": 0.0, "hits": 0.0, "sizes": 0.0, "gather": 0.0}
    finally:
        db.close()


@pytest.mark.parametrize("k", [31, 5])
def test_record_and_line_boundaries_at_every_edge(monkeypatch, k):
    """A sequence line that starts, and a record that ends, at each end of a lane's and a tile's range of the line table,
    of a lane's, a wave's and a block's range of the hit walk.  (Buffers of 64 KiB, still one piece per call: the many
    small calls here spend their time allocating the default 16 MiB ones.)"""
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(1 << 16))
    rng = np.random.default_rng(200 + k)
    hit, miss = random_bases(rng, 60), random_bases(rng, 60)
    table = kmers_of([hit], k, False)
    db = make_db(table, k, False)
    try:
        for at in EDGES:
            for first in (hit, miss):
                # the sequence line of the first record starts at `at`
                text = fastq([first, miss, hit, miss], names=[b"n" * (at - 2), b"a", b"b", b"c"])
                assert text.index(b"\n") + 1 == at
                check(db, text, table, k, False, ctx=("line", at))
                # the first record ends at `at`
                s = min(40, (at - 6) // 2)
                text = fastq([first[:s], hit, miss, hit], names=[b"n" * (at - 6 - 2 * s), b"", b"b", b""])
                assert len(b"".join(sm.fastq_records(text)[0])) == at
                check(db, text, table, k, False, ctx=("record", at))
                check(db, text, table, k, False, invert=True, ctx=("record -v", at))
    finally:
        db.close()


# ------------------------------------------------------------------ gather
def test_every_pair_of_source_and_output_residues():
    k = 31
    rng = np.random.default_rng(3)
    reads = [random_bases(rng, 40) for _ in range(6000)]
    names = [b"x" * int(n) for n in rng.integers(0, 16, 6000)]
    keep = rng.random(6000) < 0.5
    table = kmers_of([r for r, kp in zip(reads, keep) if kp], k, True)
    text = fastq(reads, names=names)
    # on the CPU: the kept records' source and output offsets take every pair of residues mod 16
    src = out = 0
    pairs = set()
    for rec, h in zip(sm.fastq_records(text), model_hits(text, table, k, True)):
        n = len(b"".join(rec))
        if h:
            pairs.add((src % 16, out % 16))
            out += n
        src += n
    assert len(pairs) == 256
    db = make_db(table, k, True)
    try:
        check(db, text, table, k, True)
        check(db, text, table, k, True, invert=True)
    finally:
        db.close()


def test_records_of_six_eight_and_ten_bytes():
    """Three or more records per output word: "@\\n\\n+\\n\\n", one base, two bases (k = 2, where two bases can hit)."""
    rng = np.random.default_rng(4)
    pool = [b"", b"A", b"AC", b"GT", b"TT", b"C"]
    reads = [pool[i] for i in rng.integers(0, len(pool), 5000)]
    text = fastq(reads, names=[b""] * len(reads))
    assert len(text) == sum(6 + 2 * len(r) for r in reads)
    for canonical in (True, False):
        table = kmers_of([b"AC"], 2, canonical)
        db = make_db(table, 2, canonical)
        try:
            out = check(db, text, table, 2, canonical)
            assert len(out) == 10 * sum(r == b"AC" or (canonical and r == b"GT") for r in reads)
            assert len(check(db, text, table, 2, canonical, invert=True)) == len(text) - len(out)
            check(db, fastq([b"", b"A"] * 300, names=[b""] * 600), table, 2, canonical, invert=True)
        finally:
            db.close()


def test_keep_patterns():
    k = 31
    rng = np.random.default_rng(5)
    n = 2 * sum(range(1, 41))
    reads = [random_bases(rng, 50) for _ in range(n)]
    text = fastq(reads)
    runs = []
    for ln in range(1, 41):                                 # runs of 1 .. 40 kept, each followed by as many dropped
        runs += [True] * ln + [False] * ln
    patterns = {"all": [True] * n, "none": [False] * n, "first only": [True] + [False] * (n - 1),
                "last only": [False] * (n - 1) + [True], "every other": [i % 2 == 0 for i in range(n)], "runs": runs}
    for name, pattern in patterns.items():
        table = kmers_of([r for r, kp in zip(reads, pattern) if kp], k, True) or {0: 1}
        db = make_db(table, k, True)
        try:
            out = check(db, text, table, k, True, ctx=name)
            assert out == b"".join(b"".join(rec) for rec, kp in zip(sm.fastq_records(text), pattern) if kp), name
            if name == "none":                              # nothing kept: no write() at all, so a reader that is
                r, w = os.pipe()                            # gone is never noticed
                os.close(r)
                try:
                    with kmlib.Selector(db, w) as sel:
                        assert sel.add_fastq(text, final=True) == len(text)
                        assert sel.stats()["records_out"] == 0 and sel.stats()["bytes_out"] == 0
                finally:
                    os.close(w)
        finally:
            db.close()


# ------------------------------------------------------------------ the rule
def test_min_hits_and_invert():
    k = 31
    rng = np.random.default_rng(6)
    bait = random_bases(rng, 120)
    reads = [bait[:k], bait[:k + 1], bait[10:80], random_bases(rng, 70), bait[:k - 1], bait]
    text = fastq(reads)
    table = kmers_of([bait], k, True)
    db = make_db(table, k, True)
    try:
        assert model_hits(text, table, k, True) == [1, 2, 40, 0, 0, 90]
        for min_hits in (1, 2, 40, 41, 90, 91):             # exactly a read's window count, and one more
            for invert in (False, True):
                check(db, text, table, k, True, min_hits=min_hits, invert=invert, ctx=(min_hits, invert))
    finally:
        db.close()


def test_non_bases_strands_case_and_quality():
    k = 31
    rng = np.random.default_rng(7)
    bait = random_bases(rng, 200)
    every_kth = bytearray(bait)
    every_kth[k - 1::k] = b"N" * len(every_kth[k - 1::k])   # N at every k-th base: no window is left
    almost = bytearray(bait)
    almost[k::k + 1] = b"N" * len(almost[k::k + 1])         # ... at every (k + 1)-th: one window between two of them
    rc = bait.translate(COMPLEMENT)[::-1]
    reads = [bait, bytes(every_kth), bytes(almost), rc, bait.lower(), rc.lower(), random_bases(rng, 200)]
    quals = [b"I" * 200 for _ in reads]
    text = fastq(reads, quals=quals)
    for canonical, want in ((True, [170, 0, 6, 170, 170, 170, 0]), (False, [170, 0, 6, 0, 170, 0, 0])):
        table = kmers_of([bait], k, canonical)
        db = make_db(table, k, canonical)
        try:
            assert model_hits(text, table, k, canonical) == want
            check(db, text, table, k, canonical, ctx=canonical)
            check(db, text, table, k, canonical, min_hits=7, invert=True, ctx=canonical)
        finally:
            db.close()
    # -Q turns a hit read into a miss: one low quality in the middle of the only stretch that hits
    table = kmers_of([bait[:40]], k, True)
    db = make_db(table, k, True)
    try:
        low = bytearray(b"I" * 200)
        low[20] = ord("4")
        text = fastq([bait, bait, bait], quals=[b"I" * 200, bytes(low), b"5" * 200])
        assert model_hits(text, table, k, True, ord("5")) == [10, 0, 10] and model_hits(text, table, k, True) == [10, 10, 10]
        check(db, text, table, k, True, min_qual="5")
        check(db, text, table, k, True, min_qual=ord("5"), invert=True)
        check(db, text, table, k, True)
        # a quality line that starts with '@', a '+' line that repeats the header, "\r\n" line ends
        text = fastq([bait, random_bases(rng, 50), bait[:35]], names=[b"a 1", b"b 2", b"c 3"],
                     quals=[b"@" + b"I" * 199, b"@" * 50, b"@+" + b"I" * 33], plus=[b"+a 1", b"+", b"+c 3"])
        check(db, text, table, k, True)
        check(db, text, table, k, True, min_qual="A")        # '@' is below 'A': the first base of each read is masked
        crlf = text.replace(b"\n", b"\r\n")
        out = check(db, crlf, table, k, True)
        assert out.count(b"\r\n") == 8 and out == model_select(text, table, k, True).replace(b"\n", b"\r\n")
    finally:
        db.close()


def test_last_record_without_newline():
    k = 31
    rng = np.random.default_rng(8)
    hit, miss = random_bases(rng, 50), random_bases(rng, 50)
    table = kmers_of([hit], k, True)
    db = make_db(table, k, True)
    try:
        kept_last, dropped_last = fastq([miss, hit], last_newline=False), fastq([hit, miss], last_newline=False)
        assert check(db, kept_last, table, k, True) == fastq([hit], names=[b"r1"])            # the host's newline
        assert check(db, dropped_last, table, k, True) == fastq([hit], names=[b"r0"])
        assert check(db, dropped_last, table, k, True, invert=True) == fastq([miss], names=[b"r1"])
        for a, b in ((kept_last, kept_last), (kept_last, dropped_last), (dropped_last, kept_last)):
            got, stats, consumed = select(db, [a, b])
            assert got == model_select(a, table, k, True) + model_select(b, table, k, True)
            assert consumed == len(a) + len(b) and stats["bytes_out"] == len(got) and stats["bytes_in"] == consumed
    finally:
        db.close()


# ------------------------------------------------------------------ pieces
def piece_text(seed=9, n=1500):
    rng = np.random.default_rng(seed)
    genome = random_bases(rng, 3000)
    reads, names = [], []
    for i in range(n):
        ln = int(rng.integers(20, 90))
        if rng.random() < 0.4:
            a = int(rng.integers(0, len(genome) - ln))
            reads.append(genome[a:a + ln])
        else:
            reads.append(random_bases(rng, ln))
        names.append(b"read%d/%d" % (i, ln))
    return fastq(reads, names=names), kmers_of([genome], 31, True)


CHILD = """
import json, sys
from km_amd import lib
import numpy as np
table = np.load(sys.argv[1])
db = lib.Database.from_records(table["keys"], table["counts"], 31, True).upload(0)
text = open(sys.argv[2], "rb").read()
with open(sys.argv[3], "wb") as out:
    with lib.Selector(db, out, min_hits=2) as sel:
        used = sel.add_fastq(text, final=True)
        stats = sel.stats()
hits = db.fastq_hits(text)
db.close()
print(json.dumps({"used": used, "stats": stats, "hits": hits.tolist()}))
"""


def test_staging_sizes_in_child_processes(tmp_path):
    text, table = piece_text()
    assert max(len(b"".join(r)) for r in sm.fastq_records(text)) <= 256
    np.savez(tmp_path / "table.npz", keys=np.fromiter(table.keys(), np.uint64, len(table)),
             counts=np.ones(len(table), np.uint32))
    (tmp_path / "reads.fq").write_bytes(text)
    (tmp_path / "child.py").write_text(CHILD)
    want = model_select(text, table, 31, True, min_hits=2)
    want_hits = model_hits(text, table, 31, True)
    assert 0 < len(want) < len(text)
    for stage in (256, 4096, None):
        env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system")
        env.pop("KM_COUNT_STAGE_BYTES", None)
        if stage is not None:
            env["KM_COUNT_STAGE_BYTES"] = str(stage)
        res = subprocess.run([sys.executable, "child.py", "table.npz", "reads.fq", "out.fq"], cwd=tmp_path,
                             capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == 0, res.stderr
        got = json.loads(res.stdout.splitlines()[-1])
        assert (tmp_path / "out.fq").read_bytes() == want, stage
        assert got["used"] == len(text) and got["hits"] == want_hits
        pieces = 1 if stage is None else len(greedy_pieces(text, stage))
        assert got["stats"]["pieces"] == pieces and got["stats"]["bytes_out"] == len(want), stage
        if stage is not None:
            assert pieces >= len(text) // stage and pieces > 20


def test_one_call_and_a_thousand_random_cuts(monkeypatch):
    text, table = piece_text(seed=10)
    db = make_db(table, 31, True)
    try:
        whole, stats, consumed = select(db, text, min_hits=2)
        assert whole == model_select(text, table, 31, True, min_hits=2) and consumed == len(text)
        cuts = sorted(np.random.default_rng(11).integers(1, len(text), 1000).tolist())
        for stage in (None, 4096):
            if stage is not None:
                monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))
            got, cut_stats, cut_consumed = select(db, text, min_hits=2, cuts=cuts)
            assert got == whole and cut_consumed == consumed == len(text), stage
            assert {f: cut_stats[f] for f in ("records_in", "records_out", "bytes_in", "bytes_out")} == {
                f: stats[f] for f in ("records_in", "records_out", "bytes_in", "bytes_out")}
    finally:
        db.close()


def test_a_record_longer_than_a_buffer(monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "256")
    rng = np.random.default_rng(12)
    short, long_one = random_bases(rng, 40), random_bases(rng, 200)
    table = kmers_of([short], 31, True)
    db = make_db(table, 31, True)
    try:
        text = fastq([short, short, long_one, short])
        first_two = len(fastq([short, short]))
        with tempfile.TemporaryFile() as fh:
            with kmlib.Selector(db, fh) as sel:
                with pytest.raises(kmlib.KmError) as e:
                    sel.add_fastq(text, final=True)
                assert e.value.code == KM_E_CAPACITY and "byte offset %d" % first_two in str(e.value)
                with pytest.raises(kmlib.KmError) as e:
                    sel.add_fastq(text[:first_two], final=True)
                assert e.value.code == KM_E_CAPACITY and "byte offset %d" % first_two in str(e.value)
            fh.seek(0)
            assert fh.read() == text[:first_two]              # the pieces before it are written
        with pytest.raises(kmlib.KmError) as e:
            db.fastq_hits(text)
        assert e.value.code == KM_E_CAPACITY and "byte offset %d" % first_two in str(e.value)
    finally:
        db.close()


# ------------------------------------------------------------------ fastq_hits: two device paths, one answer
def test_fastq_hits_equals_the_model_and_cov_seqs():
    text, table = piece_text(seed=13, n=800)
    db = make_db(table, 31, True)
    try:
        hits = db.fastq_hits(text)
        assert hits.tolist() == model_hits(text, table, 31, True)
        seqs = [sm._content(s) for _, s, _, _ in sm.fastq_records(text)]
        cov = db.cov_seqs(seqs)
        assert np.array_equal(hits, (cov["n_kmers"] - cov["n_zero"]).astype(np.uint32))
        assert hits.max() > 30 and (hits == 0).sum() > 100
        assert db.fastq_hits(b"").size == 0
    finally:
        db.close()
    # the reference's own figure through the device: the FLT3-ITD target as one read against its sample
    seq = ko.read_fasta_concat(FLT3).encode("ascii")
    db = kmlib.Database.load(IANDI)
    try:
        assert db.fastq_hits(fastq([seq])).tolist() == [315]
    finally:
        db.close()


# ------------------------------------------------------------------ errors
@pytest.mark.parametrize("kind", [sm.NO_AT, sm.NO_PLUS, sm.QUAL_LEN, sm.TRUNCATED])
def test_malformed_record_in_a_later_piece(monkeypatch, kind):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")
    text, table = piece_text(seed=14, n=300)
    pieces = greedy_pieces(text, 4096)
    assert len(pieces) >= 4
    before = sum(len(p) for p in pieces[:2])
    recs = [b"".join(r) for r in sm.fastq_records(pieces[2])]
    at = before + sum(len(r) for r in recs[:5])                # the sixth record of the third piece
    lines = recs[5].split(b"\n")
    if kind == sm.NO_AT:
        bad, offset = text[:at] + b"#" + text[at + 1:], at
    elif kind == sm.NO_PLUS:
        offset = at + len(lines[0]) + len(lines[1]) + 2
        bad = text[:offset] + b"-" + text[offset + 1:]
    elif kind == sm.QUAL_LEN:
        offset = at + len(lines[0]) + len(lines[1]) + len(lines[2]) + 3
        bad = text[:offset] + text[offset + 1:]                # a quality byte less
    else:
        offset = at
        bad = text[:at + len(lines[0]) + len(lines[1]) + 2]    # the stream ends behind the record's sequence line
    with pytest.raises(sm.Malformed) as m:
        model_hits(bad, table, 31, True)
    assert (m.value.kind, m.value.offset) == (kind, offset)
    db = make_db(table, 31, True)
    try:
        with tempfile.TemporaryFile() as fh:
            with kmlib.Selector(db, fh) as sel:
                with pytest.raises(kmlib.KmError) as e:
                    sel.add_fastq(bad, final=True)
                assert e.value.code == KM_E_FORMAT
                assert sm.KIND_TEXT[kind] in str(e.value) and str(e.value).endswith("at byte offset %d" % offset), str(e.value)
                with pytest.raises(kmlib.KmError) as e:         # and it stays
                    sel.add_fastq(text, final=True)
                assert e.value.code == KM_E_FORMAT
            fh.seek(0)
            assert fh.read() == model_select(text[:before], table, 31, True)      # exactly the earlier pieces
        with pytest.raises(kmlib.KmError) as e:
            db.fastq_hits(bad)
        assert e.value.code == KM_E_FORMAT and str(e.value).endswith("at byte offset %d" % offset)
        # a second stream's offsets start again at 0
        with tempfile.TemporaryFile() as fh:
            with kmlib.Selector(db, fh) as sel:
                assert sel.add_fastq(text, final=True) == len(text)
                with pytest.raises(kmlib.KmError) as e:
                    sel.add_fastq(bad, final=True)
                assert str(e.value).endswith("at byte offset %d" % offset)
    finally:
        db.close()


def test_argument_state_and_descriptor_errors():
    rng = np.random.default_rng(15)
    hit = random_bases(rng, 60)
    table = kmers_of([hit], 31, True)
    text = fastq([hit] * 50)
    db = make_db(table, 31, True)
    try:
        with tempfile.TemporaryFile() as fh:
            for kwargs, code in (({"min_hits": 0}, KM_E_ARG), ({"min_qual_char": 256}, KM_E_ARG), ({"min_qual_char": -1}, KM_E_ARG)):
                with pytest.raises(kmlib.KmError) as e:
                    kmlib.Selector(db, fh, **kwargs)
                assert e.value.code == code, kwargs
            with kmlib.Selector(db, fh) as sel:
                assert sel.add_fastq(b"", final=True) == 0 and sel.add_fastq(b"", final=False) == 0
                assert sel.stats() == {"records_in": 0, "records_out": 0, "bytes_in": 0, "bytes_out": 0, "pieces": 0}
                consumed = C.c_uint64()
                lib = kmlib.load()
                assert lib.km_select_add_fastq(sel._s, None, 5, 1, C.byref(consumed)) == KM_E_ARG
                assert lib.km_select_add_fastq(sel._s, text, len(text), 1, None) == KM_E_ARG
                assert lib.km_select_stats(sel._s, None) == KM_E_ARG
            assert kmlib.load().km_select_create(db._h, 1, 0, 0, fh.fileno(), None, None) == KM_E_ARG
            assert kmlib.load().km_select_kernel_ms(None) == KM_E_ARG
            fh.seek(0)
            assert fh.read() == b""
        # a descriptor that is not open
        r, w = os.pipe()
        os.close(r)
        os.close(w)
        with pytest.raises(kmlib.KmError) as e:
            kmlib.Selector(db, w)
        assert e.value.code == KM_E_IO
        # a reader that went away (Python ignores SIGPIPE): the code, and the library goes on
        r, w = os.pipe()
        os.close(r)
        try:
            with kmlib.Selector(db, w) as sel:
                with pytest.raises(kmlib.KmError) as e:
                    sel.add_fastq(text, final=True)
                assert e.value.code == KM_E_IO and "writing the text failed" in str(e.value)
                with pytest.raises(kmlib.KmError) as e:         # and it stays, whatever the failure was
                    sel.add_fastq(text, final=True)
                assert e.value.code == KM_E_IO and "writing the text failed" in str(e.value)
        finally:
            os.close(w)
        assert select(db, text)[0] == text
    finally:
        db.close()
    # no uploaded table
    host_only = kmlib.Database.from_records(np.array([1], np.uint64), np.array([1], np.uint32), 31, True)
    try:
        with tempfile.TemporaryFile() as fh:
            with pytest.raises(kmlib.KmError) as e:
                kmlib.Selector(host_only, fh)
            assert e.value.code == KM_E_STATE
        with pytest.raises(kmlib.KmError) as e:
            host_only.fastq_hits(text)
        assert e.value.code == KM_E_STATE
    finally:
        host_only.close()


# ------------------------------------------------------------------ the command
def run_cli(tmp_path, *args, stdin=None, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system")
    env.pop("KM_COUNT_STAGE_BYTES", None)
    res = subprocess.run([sys.executable, "-m", "km_amd"] + list(args), cwd=tmp_path, capture_output=True, timeout=300,
                         env=env, input=stdin)
    if ok:
        assert res.returncode == 0, res.stderr
    return res


def figures(stderr):
    return dict(line[1:].split(":") for line in stderr.decode().splitlines() if line.startswith("#"))


def fasta_records(path):
    """The records of a FASTA file, lines joined: what `bait -t` takes its k-mers from, record by record."""
    records = []
    with open(path, "rb") as fh:
        for line in fh:
            if line.startswith(b">"):
                records.append([])
            elif records:
                records[-1].append(line.strip())
    return [b"".join(r) for r in records]


def target_reads(seed, n_random=300):
    """Reads cut from the FLT3-ITD target, both strands, and random ones, shuffled."""
    rng = np.random.default_rng(seed)
    ref = ko.read_fasta_concat(FLT3).encode("ascii")
    reads = []
    for _ in range(300):
        a = int(rng.integers(0, len(ref) - 100))
        r = ref[a:a + 100]
        reads.append(r.translate(COMPLEMENT)[::-1] if rng.integers(2) else r)
    reads += [random_bases(rng, 100) for _ in range(n_random)]
    order = rng.permutation(len(reads))
    return ref, [reads[i] for i in order]


def test_cli_bait(tmp_path):
    ref, reads = target_reads(16)
    text = fastq(reads)
    (tmp_path / "reads.fq").write_bytes(text)
    with gzip.open(tmp_path / "reads.fq.gz", "wb") as fh:
        fh.write(text)
    # -t, gzip input, -o, two files: two streams
    table = kmers_of(fasta_records(FLT3), 31, True)
    want = model_select(text, table, 31, True)
    assert want.count(b"\n") == 4 * 300 and len(fasta_records(FLT3)) > 1
    res = run_cli(tmp_path, "bait", "-t", FLT3, "-o", "out.fq", "reads.fq.gz", "reads.fq")
    assert res.stdout == b"" and (tmp_path / "out.fq").read_bytes() == want + want
    assert figures(res.stderr) == {"bait_kmers": str(len(table)), "reads_in": "1200", "reads_out": "600",
                                   "bytes_in": str(2 * len(text)), "bytes_out": str(2 * len(want)), "pieces": "2"}
    # -d with the sample's own table, -v, -n, stdin, standard output
    sample, k, canonical = sm.file_table(IANDI)
    assert (k, canonical) == (31, True)
    want = model_select(text, sample, 31, True, min_hits=5, invert=True)
    res = run_cli(tmp_path, "bait", "-d", IANDI, "-v", "-n", "5", "-", stdin=text)
    assert res.stdout == want and 0 < len(want) < len(text)
    fig = figures(res.stderr)
    assert fig["bait_kmers"] == str(len(sample)) and fig["reads_in"] == "600" and fig["bytes_out"] == str(len(want))
    assert set(fig) == {"bait_kmers", "reads_in", "reads_out", "bytes_in", "bytes_out", "pieces"}
    # a FASTA file is refused, a malformed one named
    (tmp_path / "reads.fa").write_bytes(b">r\nACGT\n")
    res = run_cli(tmp_path, "bait", "-t", FLT3, "reads.fa", ok=False)
    assert res.returncode == 1 and res.stderr.startswith(b"ERROR: bait: ") and b"4-line FASTQ" in res.stderr and res.stdout == b""
    res = run_cli(tmp_path, "bait", "-t", FLT3, "-", stdin=text[:-30], ok=False)
    assert res.returncode == 1 and res.stderr.startswith(b"ERROR: bait: ") and b"quality line" in res.stderr


def test_files_are_streams_of_their_own(tmp_path):
    """select_files over files that end in a newline (so the last block leaves no tail): a malformed record in the
    second file is reported with that file's name and the offset within it; the inputs are looked at before the output
    is opened."""
    from km_amd import count as kc
    rng = np.random.default_rng(18)
    hit, miss = random_bases(rng, 60), random_bases(rng, 60)
    table = kmers_of([hit], 31, True)
    good = fastq([hit, miss, hit])
    bad = fastq([miss, hit, hit, miss])
    offset = len(fastq([miss, hit])) + len(b"@r2\n") + 61        # the '+' of the third record
    assert bad[offset:offset + 1] == b"+" and good.endswith(b"\n")
    bad = bad[:offset] + b"-" + bad[offset + 1:]
    with pytest.raises(sm.Malformed) as m:
        model_hits(bad, table, 31, True)
    assert (m.value.kind, m.value.offset) == (sm.NO_PLUS, offset)
    (tmp_path / "a.fq").write_bytes(good)
    (tmp_path / "b.fq").write_bytes(bad)
    (tmp_path / "c.fq").write_bytes(good)
    a, b, c = (str(tmp_path / n) for n in ("a.fq", "b.fq", "c.fq"))
    db = make_db(table, 31, True)
    try:
        with open(tmp_path / "out.fq", "wb") as out:
            with pytest.raises(kmlib.KmError) as e:
                kc.select_files(db, [a, a, b, c], out=out)
        assert e.value.code == KM_E_FORMAT
        assert str(e.value) == "libkmgpu: %s: FASTQ record lacks its '+' line at byte offset %d" % (b, offset)
        assert (tmp_path / "out.fq").read_bytes() == 2 * model_select(good, table, 31, True)     # the files before it
        # three good files: three streams, every one from offset 0 (their stats add up)
        stats = kc.select_files(db, [a, c, a], out=str(tmp_path / "three.fq"))
        assert (tmp_path / "three.fq").read_bytes() == 3 * model_select(good, table, 31, True)
        assert stats["records_in"] == 9 and stats["records_out"] == 6 and stats["pieces"] == 3
        # a missing file, or FASTA, is found before the output is opened: an existing one keeps its bytes
        (tmp_path / "fa.fa").write_bytes(b">r\nACGT\n")
        for wrong, error in ((str(tmp_path / "none.fq"), OSError), (str(tmp_path / "fa.fa"), ValueError)):
            with pytest.raises(error):
                kc.select_files(db, [a, wrong], out=str(tmp_path / "three.fq"))
            with pytest.raises(error):
                kc.select_files(db, [a, wrong], out=str(tmp_path / "new.fq"))
            assert not (tmp_path / "new.fq").exists()
        assert (tmp_path / "three.fq").read_bytes() == 3 * model_select(good, table, 31, True)
        # the C call itself: an empty final call ends a stream
        with tempfile.TemporaryFile() as fh:
            with kmlib.Selector(db, fh) as sel:
                assert sel.add_fastq(good, final=False) == len(good) and sel.add_fastq(b"", final=True) == 0
                with pytest.raises(kmlib.KmError) as e:
                    sel.add_fastq(bad, final=False)
                assert str(e.value).endswith("at byte offset %d" % offset)
    finally:
        db.close()


# ------------------------------------------------------------------ closing the loop
def test_bait_then_count_then_find_mutation(tmp_path):
    """The whole FLT3 sample of tests/test_count.py (30 % of its reads carry the 30-nt tandem duplication) among as
    many random reads: `bait -t FLT3-ITD`, then `count`, then `find_mutation` give the rows that `count` and
    `find_mutation` give on the whole sample.

    That sample tiles the target with 100 random bases on either side, so about one read in seven lies (almost) wholly
    in that padding, shares no 31 bases with an exon and is dropped by `bait` like a random read.  Nothing
    `find_mutation` needs goes with them, and the test checks the reason on the CPU first: every read of the sample
    that holds a 31-mer of the joined target or of the duplicated allele, on either strand, also holds 31 bases of one
    exon, so the model keeps it, and every k-mer of the target and of the ITD keeps its count.  What the dropped reads
    would have added is k-mers with padding bases in them, which lie outside the walk between the target's first and
    last k-mer."""
    import test_count as tc
    ref, sample = tc.itd_reads()
    exons = fasta_records(FLT3)                             # (`bait -t` takes the k-mers of each record, not of their join)
    assert b"".join(exons).decode() == ref
    rng = np.random.default_rng(17)
    noise = [random_bases(rng, 100) for _ in sample]
    text = fastq([r for pair in zip(sample, noise) for r in pair])
    table = kmers_of(exons, 31, True)
    hits = model_hits(text, table, 31, True)
    assert not any(hits[1::2])                              # no random read is kept
    itd = ref[:180] + ref[150:180] + ref[180:]
    needed = kmers_of([ref.encode(), itd.encode()], 31, True)
    n_needed = 0
    for r, h in zip(sample, hits[0::2]):
        if model_hits(fastq([r]), needed, 31, True)[0]:
            n_needed += 1
            assert h > 0                                    # every read find_mutation's k-mers come from is kept
    kept = [r for r, h in zip(sample, hits[0::2]) if h]
    assert 500 < n_needed <= len(kept) < len(sample)        # ... and some reads of the sample are not
    (tmp_path / "mixed.fq").write_bytes(text)
    (tmp_path / "sample.fq").write_bytes(fastq(sample))
    res = run_cli(tmp_path, "bait", "-t", FLT3, "-o", "baited.fq", "mixed.fq")
    names = [b"r%d" % (2 * i) for i, h in enumerate(hits[0::2]) if h]
    assert (tmp_path / "baited.fq").read_bytes() == fastq(kept, names=names)
    assert figures(res.stderr)["reads_out"] == str(len(kept)) and figures(res.stderr)["reads_in"] == str(2 * len(sample))
    rows = {}
    for name in ("baited", "sample"):
        run_cli(tmp_path, "count", "-m", "31", "-C", "-L", "2", "-o", name + ".jf", name + ".fq")
        res = run_cli(tmp_path, "find_mutation", FLT3, name + ".jf")
        body = [ln for ln in res.stdout.decode().splitlines() if not ln.startswith("#")]
        rows[name] = [ln.split("\t", 1)[1] for ln in body[1:]]                   # (without the database's name)
    assert rows["baited"] == rows["sample"] and any(r.split("\t")[1] == "ITD" for r in rows["sample"]), (rows["baited"], rows["sample"])
