"""The labelled selection of FASTQ reads on the GPU: lib.LabelSelector (km_select_labels_*), Database.fastq_label_hits
(kmjf_fastq_label_hits), count.label_table / select_label_files and `python -m km_amd bait --split-dir`.

Every comparison is exact, integers equal and outputs byte-identical, against model_label_hits / model_label_select of
tests/test_select_label_cpu.py, which are written from the rule of include/kmgpu.h; with one label of mask 1 the new path
must equal lib.Selector / Database.fastq_hits byte for byte.  The shapes are the smallest at which the kernels can go
wrong: the seams of a lane of the hit walk (32 window starts), masks that alternate window by window, a virtual stream
longer than an output buffer (staging buffers of 256 and 4 096 bytes), a pass boundary inside a record, at a record's
end and on a label boundary, a label without bytes between two that have some."""
import ctypes as C
import io
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from km_amd import cli
from km_amd import count as kc
from km_amd import lib as kmlib
import test_select as ts
import test_select_cpu as sm
import test_select_label_cpu as lm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CATALOG = os.path.join(HERE, "data", "catalog", "GRCh38")
KM_E_IO, KM_E_FORMAT, KM_E_ARG, KM_E_STATE, KM_E_CAPACITY = 1, 2, 4, 7, 8
STAT_KEYS = {"records_in", "records_any", "records_multi", "bytes_in", "pieces", "gather_passes", "records_out", "bytes_out"}

pytestmark = pytest.mark.gpu

fastq, random_bases, kmers_of = sm.fastq, sm.random_bases, sm.kmers_of


# ------------------------------------------------------------------ helpers
def select_labels(db, n_labels, streams, min_hits=1, min_qual=None, cuts=None):
    """The streams (bytes each) through one LabelSelector into n_labels descriptors, as test_select.select feeds one
    -> ([the descriptors' bytes], stats, the sum of what the calls consumed)."""
    if isinstance(streams, bytes):
        streams = [streams]
    consumed = 0
    files = [tempfile.TemporaryFile() for _ in range(n_labels)]
    try:
        with kmlib.LabelSelector(db, files, min_hits=min_hits, min_qual_char=min_qual) as sel:
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
        outs = []
        for fh in files:
            fh.seek(0)
            outs.append(fh.read())
        return outs, stats, consumed
    finally:
        for fh in files:
            fh.close()


def check_labels(db, text, table, k, canonical, n_labels, min_hits=1, min_qual=None, stage=None, ctx=None):
    """LabelSelector and fastq_label_hits of one final stream against the model -> (outputs, stats).  stage: the
    KM_COUNT_STAGE_BYTES in force, for the pieces and passes."""
    q = ts.sm_qual(min_qual)
    want_hits = lm.model_label_hits(text, table, k, canonical, n_labels, q)
    got_hits = db.fastq_label_hits(n_labels, text, min_qual_char=min_qual)
    assert got_hits.dtype == np.uint32 and got_hits.shape == (n_labels, len(want_hits[0]))
    assert got_hits.tolist() == want_hits, (ctx, [(l, r) for l in range(n_labels) for r in range(len(want_hits[0]))
                                                  if got_hits[l, r] != want_hits[l][r]][:5])
    want = lm.model_label_select(text, table, k, canonical, n_labels, min_hits, q)
    got, stats, consumed = select_labels(db, n_labels, text, min_hits, min_qual)
    for l in range(n_labels):
        assert got[l] == want[l], (ctx, l, len(got[l]), len(want[l]))
    assert consumed == len(text) and set(stats) == STAT_KEYS
    any_, multi = lm.model_any_multi(text, table, k, canonical, n_labels, min_hits, q)
    assert (stats["records_in"], stats["records_any"], stats["records_multi"], stats["bytes_in"]) == (
        len(want_hits[0]), any_, multi, len(text)), (ctx, stats)
    assert stats["records_out"] == [sum(h >= min_hits for h in want_hits[l]) for l in range(n_labels)], ctx
    assert stats["bytes_out"] == [len(w) for w in want], ctx
    if stage is not None:
        assert stats["pieces"] == len(lm.model_pieces(text, stage)), ctx
        assert stats["gather_passes"] == lm.model_passes(text, table, k, canonical, n_labels, stage, min_hits, q)[0], ctx
    return got, stats


# ------------------------------------------------------------------ one label of mask 1 is the single selector
@pytest.mark.parametrize("k", [31, 5])
def test_one_label_equals_the_single_selector(monkeypatch, k):
    monkeypatch.setenv("KM_SELECT_TIME", "1")
    rng = np.random.default_rng(100 + k)
    lengths = list(range(0, 201))
    reads = [random_bases(rng, n) for n in lengths]
    table = {key: 1 for key in kmers_of([r[:len(r) // 2 + k] for r in reads[k::3]], k, True)}
    db = ts.make_db(table, k, True)
    try:
        for text, min_hits, min_qual in ((fastq(reads), 1, None), (fastq(reads, last_newline=False), 3, None),
                                         # (a quality below '5' at every 37th base: windows of 31 bases are left between two of them)
                                         (fastq(reads, quals=[bytes(40 if (i * 7 + j) % 37 == 0 else 70 for j in range(n)) for i, n in enumerate(lengths)]), 1, "5")):
            old_out, old_stats, _ = ts.select(db, text, min_hits, False, min_qual)
            old_hits = db.fastq_hits(text, min_qual_char=min_qual)
            (new_out,), stats, consumed = select_labels(db, 1, text, min_hits, min_qual)
            new_hits = db.fastq_label_hits(1, text, min_qual_char=min_qual)
            assert new_out == old_out and 0 < len(old_out) < len(text) + 1
            assert new_hits.shape == (1, len(old_hits)) and np.array_equal(new_hits[0], old_hits)
            assert consumed == len(text)
            assert (stats["records_in"], stats["records_out"], stats["bytes_in"], stats["bytes_out"], stats["pieces"]) == (
                old_stats["records_in"], [old_stats["records_out"]], old_stats["bytes_in"], [old_stats["bytes_out"]], old_stats["pieces"])
            assert (stats["records_any"], stats["records_multi"], stats["gather_passes"]) == (old_stats["records_out"], 0, old_stats["pieces"])
            check_labels(db, text, table, k, True, 1, min_hits, min_qual, ctx=(k, min_hits))
        ms = kmlib.select_kernel_ms()
        assert ms["front"] > 0 and ms["hits"] > 0 and ms["sizes"] > 0 and ms["gather"] > 0
        monkeypatch.delenv("KM_SELECT_TIME")
        select_labels(db, 1, fastq(reads))
        assert kmlib.select_kernel_ms() == {"front": 0.0, "hits": 0.0, "sizes": 0.0, "gather": 0.0}
    finally:
        db.close()


# ------------------------------------------------------------------ 32 labels, the overflow side table, ignored bits
def test_32_labels_single_bits_all_bits_and_ignored_bits(monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")
    rng = np.random.default_rng(31)
    k = 21
    reads = [random_bases(rng, 60) for _ in range(120)]
    table = {}
    for i, r in enumerate(reads[:100]):                         # one mask per read: every window of the read carries it
        mask = (1 << 0, 1 << 15, 1 << 16, 1 << 31, 0xFFFFFFFF, 0xFFFF, 0x10000, 0x80000001, 0xFFFFFFF8, 0xFFFE)[i % 10]
        for key in kmers_of([r], k, True):
            table[key] = mask
    assert sum(m >= 0xFFFF for m in table.values()) > 1000       # the overflow side table holds most keys
    order = rng.permutation(len(reads))
    text = fastq([reads[i] for i in order], names=[b"r%d" % i for i in order])
    db = ts.make_db(table, k, True)
    try:
        outs, stats = check_labels(db, text, table, k, True, 32, stage=4096, ctx="32")
        assert all(len(o) > 0 for o in outs) and stats["records_multi"] > 0 and stats["gather_passes"] > stats["pieces"] > 1
        # three labels of the same table: bits 3 and above are ignored, a key with only such bits hits nothing
        outs3, stats3 = check_labels(db, text, table, k, True, 3, stage=4096, ctx="3 of 32")
        assert outs3 == outs[:3] and stats3["records_any"] < stats["records_any"]
        outs17, _ = check_labels(db, text, table, k, True, 17, min_hits=40, stage=4096, ctx="17, min_hits")
        assert any(outs17)
    finally:
        db.close()


# ------------------------------------------------------------------ masks that change from window to window, lane seams
@pytest.mark.parametrize("min_hits", [1, 2, 3])
def test_mask_runs_at_every_lane_seam(min_hits):
    reads, names, table, pattern = lm.seam_reads(np.random.default_rng(23))
    text = fastq(reads, names=names)
    seams, at = set(), 0
    for h, s, p, q in sm.fastq_records(text):
        for j in range(len(s) - 1 - 5 + 1):
            if (at + len(h) + j) % 32 in (0, 31):
                seams.add(((at + len(h) + j) % 32, j % len(pattern)))
        at += len(h) + len(s) + len(p) + len(q)
    assert len(seams) == 2 * len(pattern)
    db = ts.make_db(table, 5, False)
    try:
        outs, stats = check_labels(db, text, table, 5, False, 2, min_hits=min_hits, ctx=min_hits)
        hits = lm.model_label_hits(text, table, 5, False, 2)
        assert any(a != b and (a >= min_hits) != (b >= min_hits) for a, b in zip(*hits))
        assert outs[0] != outs[1]
    finally:
        db.close()


# ------------------------------------------------------------------ more bytes than an output buffer: gather passes
def pass_cases():
    rng = np.random.default_rng(41)
    same = [random_bases(rng, 60) for _ in range(150)]
    one = [random_bases(rng, 60)]
    a, b = [random_bases(rng, 50) for _ in range(60)], [random_bases(rng, 50) for _ in range(60)]
    mixed = [r for pair in zip(a, b) for r in pair]
    eight = [random_bases(rng, 120) for _ in range(8)]
    fifteen = [random_bases(rng, 120) for _ in range(15)]
    return [
        # every read in all 32 labels: the virtual stream is 32 times the piece
        ("32 x everything", 32, fastq(same), lm.label_kmers([same] * 32, 31, True), (4096, 256)),
        # one record of 136 bytes in three labels at stage 256 (cap 272): label_off = 0, 136, 272, 408
        ("136 x 3", 3, fastq(one, names=[b"n" * 10]), lm.label_kmers([one] * 3, 31, True), (256,)),
        # eight records of 257 bytes in three labels at stage 4096 (cap 4112): label_off = 0, 2056, 4112, 6168
        ("2056 x 3", 3, fastq(eight, names=[b"n" * 11] * 8), lm.label_kmers([eight] * 3, 31, True), (4096,)),
        # fifteen records of 257 bytes in two labels at stage 4096: 4112 is the end of label 1's first record
        ("3855 x 2", 2, fastq(fifteen, names=[b"n" * 10 + b"%d" % (i % 10) for i in range(15)]), lm.label_kmers([fifteen] * 2, 31, True), (4096,)),
        # a label without bytes between two that have some; two labels of equal content; the last record open
        ("empty, equal", 4, fastq(mixed, last_newline=False), lm.label_kmers([a, [], b, a], 31, True), (256, 4096)),
    ]


def test_gather_passes(monkeypatch):
    kinds = set()
    for name, n_labels, text, table, stages in pass_cases():
        db = ts.make_db(table, 31, True)
        try:
            for stage in stages:
                monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))
                passes, met = lm.model_passes(text, table, 31, True, n_labels, stage)
                kinds |= met
                outs, stats = check_labels(db, text, table, 31, True, n_labels, stage=stage, ctx=(name, stage))
                assert stats["gather_passes"] == passes
                if name == "32 x everything":
                    assert all(o == text for o in outs) and passes >= 15 * stats["pieces"]
                if name in ("136 x 3", "2056 x 3"):
                    assert "label" in met and passes == 2 and stats["pieces"] == 1
                if name == "3855 x 2":
                    assert met == {"record"} and passes == 2 and stats["pieces"] == 1
                if name == "empty, equal":
                    assert outs[1] == b"" and outs[0] == outs[3] and outs[0] != outs[2] and len(outs[0]) and len(outs[2])
                    assert outs[2].endswith(b"\n") and not text.endswith(b"\n")
        finally:
            db.close()
    assert kinds == {"label", "record", "inside"}


# ------------------------------------------------------------------ streams
def stream_text(seed, n=400):
    """Reads of mixed lengths over five labels that overlap -> (text, table)."""
    rng = np.random.default_rng(seed)
    reads = [random_bases(rng, int(v)) for v in rng.integers(0, 150, n)]
    names = [b"q" * int(v) for v in rng.integers(0, 20, n)]
    groups = [[r for i, r in enumerate(reads) if i % 11 in (l, l + 1)] for l in range(5)]
    return fastq(reads, names=names), lm.label_kmers(groups, 31, True)


def test_one_call_and_a_few_hundred_random_cuts(monkeypatch):
    text, table = stream_text(51)
    rng = np.random.default_rng(52)
    db = ts.make_db(table, 31, True)
    try:
        want = lm.model_label_select(text, table, 31, True, 5)
        assert all(0 < len(w) < len(text) for w in want)
        for stage in (4096, 1 << 24):
            monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))
            outs, stats, consumed = select_labels(db, 5, text)
            assert outs == want and consumed == len(text)
            cuts = sorted(set(rng.integers(1, len(text), 300).tolist()))
            outs, cut_stats, consumed = select_labels(db, 5, text, cuts=cuts)
            assert outs == want and consumed == len(text)
            for key in ("records_in", "records_any", "records_multi", "bytes_in", "records_out", "bytes_out"):
                assert cut_stats[key] == stats[key], key
            assert cut_stats["pieces"] >= stats["pieces"]
    finally:
        db.close()


def test_two_streams_and_a_last_record_without_newline(monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")
    rng = np.random.default_rng(53)
    a, b, c = (random_bases(rng, 70) for _ in range(3))
    table = lm.label_kmers([[a], [b], [a, c], [random_bases(rng, 70)]], 31, True)
    filler = [random_bases(rng, 70) for _ in range(80)]
    # the open last record is `a`: labels 0 and 2 hold it, label 1 ends in an earlier record, label 3 holds nothing
    first = fastq(filler[:40] + [b, c] + filler[40:] + [a], last_newline=False)
    second = fastq([c, b] + filler[:10])
    db = ts.make_db(table, 31, True)
    try:
        want1, want2 = (lm.model_label_select(t, table, 31, True, 4) for t in (first, second))
        assert not first.endswith(b"\n") and want1[0].endswith(a + b"\n+\n" + b"I" * 70 + b"\n") and want1[2].endswith(b"I\n")
        assert want1[1].endswith(b"\n") and want1[3] == b"" and want2[0] == b""
        outs, stats, consumed = select_labels(db, 4, [first, second])
        assert outs == [w1 + w2 for w1, w2 in zip(want1, want2)] and consumed == len(first) + len(second)
        closed = fastq(filler[:40] + [b, c] + filler[40:] + [a])
        outs_closed, stats_closed, _ = select_labels(db, 4, [closed, second])
        assert outs_closed == outs
        assert [x - y for x, y in zip(stats["bytes_out"], stats_closed["bytes_out"])] == [0, 0, 0, 0]
        assert stats["bytes_in"] == stats_closed["bytes_in"] - 1
        # what the device gathered is a byte less in the outputs that hold the record, and the host's newline is counted
        assert stats["bytes_out"] == [len(o) for o in outs]
        alone, stats_alone, _ = select_labels(db, 4, first)
        assert alone == want1 and stats_alone["bytes_out"] == [len(w) for w in want1]
    finally:
        db.close()


# ------------------------------------------------------------------ errors
@pytest.mark.parametrize("kind", [sm.NO_AT, sm.NO_PLUS, sm.QUAL_LEN, sm.TRUNCATED])
def test_malformed_record_in_a_later_piece(monkeypatch, kind):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")
    text, table = stream_text(61, n=300)
    pieces = ts.greedy_pieces(text, 4096)
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
        assert len(lines[1]) > 0
        offset = at + len(lines[0]) + len(lines[1]) + len(lines[2]) + 3
        bad = text[:offset] + text[offset + 1:]                # a quality byte less
    else:
        offset = at
        bad = text[:at + len(lines[0]) + len(lines[1]) + 2]    # the stream ends behind the record's sequence line
    with pytest.raises(sm.Malformed) as m:
        lm.model_label_hits(bad, table, 31, True, 5)
    assert (m.value.kind, m.value.offset) == (kind, offset)
    db = ts.make_db(table, 31, True)
    try:
        files = [tempfile.TemporaryFile() for _ in range(5)]
        with kmlib.LabelSelector(db, files) as sel:
            with pytest.raises(kmlib.KmError) as e:
                sel.add_fastq(bad, final=True)
            assert e.value.code == KM_E_FORMAT
            assert sm.KIND_TEXT[kind] in str(e.value) and str(e.value).endswith("at byte offset %d" % offset), str(e.value)
            with pytest.raises(kmlib.KmError) as e:             # and it stays
                sel.add_fastq(text, final=True)
            assert e.value.code == KM_E_FORMAT
        want = lm.model_label_select(text[:before], table, 31, True, 5)
        for fh, w in zip(files, want):                          # exactly the earlier pieces
            fh.seek(0)
            assert fh.read() == w
            fh.close()
        assert sum(len(w) for w in want) > 0
        with pytest.raises(kmlib.KmError) as e:
            db.fastq_label_hits(5, bad)
        assert e.value.code == KM_E_FORMAT and str(e.value).endswith("at byte offset %d" % offset)
    finally:
        db.close()


def test_a_record_longer_than_a_buffer(monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "256")
    rng = np.random.default_rng(62)
    short, long_one = random_bases(rng, 40), random_bases(rng, 200)
    table = lm.label_kmers([[short], [short, long_one]], 31, True)
    db = ts.make_db(table, 31, True)
    try:
        text = fastq([short, short, long_one, short])
        first_two = len(fastq([short, short]))
        files = [tempfile.TemporaryFile() for _ in range(2)]
        with kmlib.LabelSelector(db, files) as sel:
            with pytest.raises(kmlib.KmError) as e:
                sel.add_fastq(text, final=True)
            assert e.value.code == KM_E_CAPACITY and "byte offset %d" % first_two in str(e.value)
            with pytest.raises(kmlib.KmError) as e:
                sel.add_fastq(text[:first_two], final=True)
            assert e.value.code == KM_E_CAPACITY
        for fh in files:
            fh.seek(0)
            assert fh.read() == text[:first_two]                # the pieces before it are written
            fh.close()
        with pytest.raises(kmlib.KmError) as e:
            db.fastq_label_hits(2, text)
        assert e.value.code == KM_E_CAPACITY and "byte offset %d" % first_two in str(e.value)
    finally:
        db.close()


def test_argument_state_and_descriptor_errors():
    rng = np.random.default_rng(63)
    hit = random_bases(rng, 60)
    table = {key: 3 for key in kmers_of([hit], 31, True)}
    text = fastq([hit] * 50)
    lib = kmlib.load()
    db = ts.make_db(table, 31, True)
    try:
        with tempfile.TemporaryFile() as f0, tempfile.TemporaryFile() as f1:
            for kwargs in ({"min_hits": 0}, {"min_qual_char": 256}, {"min_qual_char": -1}):
                with pytest.raises(kmlib.KmError) as e:
                    kmlib.LabelSelector(db, [f0, f1], **kwargs)
                assert e.value.code == KM_E_ARG, kwargs
            with pytest.raises(kmlib.KmError) as e:
                kmlib.LabelSelector(db, [])
            assert e.value.code == KM_E_ARG and "n_labels 0" in str(e.value)
            with pytest.raises(kmlib.KmError) as e:
                kmlib.LabelSelector(db, [f0, f1, f0])
            assert e.value.code == KM_E_ARG and "descriptor of its own" in str(e.value)
            many = [tempfile.TemporaryFile() for _ in range(33)]
            try:
                with pytest.raises(kmlib.KmError) as e:
                    kmlib.LabelSelector(db, many)
                assert e.value.code == KM_E_ARG and "n_labels 33" in str(e.value)
                with kmlib.LabelSelector(db, many[:32]) as sel:
                    assert sel.add_fastq(text, final=True) == len(text)
                    assert sel.stats()["records_out"] == [50, 50] + [0] * 30
            finally:
                for fh in many:
                    fh.close()
            for n in (0, 33):
                with pytest.raises(kmlib.KmError) as e:
                    db.fastq_label_hits(n, text)
                assert e.value.code == KM_E_ARG
            fds = (C.c_int32 * 2)(f0.fileno(), f1.fileno())
            handle, consumed, n_rec = C.c_void_p(), C.c_uint64(), C.c_uint64()
            assert lib.km_select_labels_create(None, 2, fds, 1, 0, None, C.byref(handle)) == KM_E_ARG
            assert lib.km_select_labels_create(db._h, 2, None, 1, 0, None, C.byref(handle)) == KM_E_ARG
            assert lib.km_select_labels_create(db._h, 2, fds, 1, 0, None, None) == KM_E_ARG
            with kmlib.LabelSelector(db, [f0, f1]) as sel:
                assert sel.add_fastq(b"", final=True) == 0 and sel.add_fastq(b"", final=False) == 0
                assert sel.stats() == {"records_in": 0, "records_any": 0, "records_multi": 0, "bytes_in": 0, "pieces": 0,
                                       "gather_passes": 0, "records_out": [0, 0], "bytes_out": [0, 0]}
                assert lib.km_select_labels_add_fastq(None, text, len(text), 1, C.byref(consumed)) == KM_E_ARG
                assert lib.km_select_labels_add_fastq(sel._s, None, 5, 1, C.byref(consumed)) == KM_E_ARG
                assert lib.km_select_labels_add_fastq(sel._s, text, len(text), 1, None) == KM_E_ARG
                st, two = kmlib.SelectLabelsStats(), (C.c_uint64 * 2)()
                assert lib.km_select_labels_stats(None, C.byref(st), two, two) == KM_E_ARG
                assert lib.km_select_labels_stats(sel._s, None, two, two) == KM_E_ARG
                assert lib.km_select_labels_stats(sel._s, C.byref(st), None, two) == KM_E_ARG
                assert lib.km_select_labels_stats(sel._s, C.byref(st), two, None) == KM_E_ARG
            hits = np.zeros(200, np.uint32)
            assert lib.kmjf_fastq_label_hits(None, 2, text, len(text), 0, kmlib.ptr(hits), 100, C.byref(n_rec), None) == KM_E_ARG
            assert lib.kmjf_fastq_label_hits(db._h, 2, None, len(text), 0, kmlib.ptr(hits), 100, C.byref(n_rec), None) == KM_E_ARG
            assert lib.kmjf_fastq_label_hits(db._h, 2, text, len(text), 0, None, 100, C.byref(n_rec), None) == KM_E_ARG
            assert lib.kmjf_fastq_label_hits(db._h, 2, text, len(text), 0, kmlib.ptr(hits), 100, None, None) == KM_E_ARG
            assert lib.kmjf_fastq_label_hits(db._h, 2, text, len(text), 0, kmlib.ptr(hits), 49, C.byref(n_rec), None) == KM_E_CAPACITY
            f0.seek(0)
            assert f0.read() == b""
        # a descriptor that is not open
        r, w = os.pipe()
        os.close(r)
        os.close(w)
        with tempfile.TemporaryFile() as f0:
            with pytest.raises(kmlib.KmError) as e:
                kmlib.LabelSelector(db, [f0, w])
            assert e.value.code == KM_E_IO
            # a descriptor that cannot be written: the reader went away (Python ignores SIGPIPE)
            r, w = os.pipe()
            os.close(r)
            try:
                with kmlib.LabelSelector(db, [f0, w]) as sel:
                    with pytest.raises(kmlib.KmError) as e:
                        sel.add_fastq(text, final=True)
                    assert e.value.code == KM_E_IO and "writing the text of label 1 failed" in str(e.value)
                    with pytest.raises(kmlib.KmError) as e:     # and it stays
                        sel.add_fastq(text, final=True)
                    assert e.value.code == KM_E_IO
            finally:
                os.close(w)
        assert select_labels(db, 2, text)[0] == [text, text]
    finally:
        db.close()
    host_only = kmlib.Database.from_records(np.array([1], np.uint64), np.array([1], np.uint32), 31, True)
    try:
        with tempfile.TemporaryFile() as fh:
            with pytest.raises(kmlib.KmError) as e:
                kmlib.LabelSelector(host_only, [fh])
            assert e.value.code == KM_E_STATE
        with pytest.raises(kmlib.KmError) as e:
            host_only.fastq_label_hits(1, text)
        assert e.value.code == KM_E_STATE
    finally:
        host_only.close()


CHILD = """
import sys, tempfile
import numpy as np
from km_amd import lib as kmlib
db = kmlib.Database.from_records(np.array([1], np.uint64), np.array([1], np.uint32), 31, True).upload(0)
files = [tempfile.TemporaryFile() for _ in range(int(sys.argv[1]))]
try:
    kmlib.LabelSelector(db, files)
    print("made")
except kmlib.KmError as e:
    print("code %d: %s" % (e.code, e))
"""


def test_labels_times_stage_must_fit_32_bits(tmp_path):
    (tmp_path / "child.py").write_text(CHILD)
    stage = 1 << 27
    env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system", KM_COUNT_STAGE_BYTES=str(stage))
    res = subprocess.run([sys.executable, "child.py", "32"], cwd=tmp_path, capture_output=True, timeout=300, env=env)
    assert res.returncode == 0, res.stderr
    out = res.stdout.decode()
    assert out.startswith("code %d:" % KM_E_CAPACITY) and "32 labels" in out and str(stage) in out, out


# ------------------------------------------------------------------ the command
def catalog_reads(seed, n_random=150):
    """Reads cut from every record of the nine targets, both strands, and random ones, shuffled."""
    rng = np.random.default_rng(seed)
    reads = []
    for f in sorted(os.listdir(CATALOG)):
        for rec in ts.fasta_records(os.path.join(CATALOG, f)):
            for _ in range(12):
                a = int(rng.integers(0, max(1, len(rec) - 60)))
                r = rec[a:a + 60]
                reads.append(r.translate(ts.COMPLEMENT)[::-1] if rng.integers(2) else r)
    reads += [random_bases(rng, 60) for _ in range(n_random)]
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def test_cli_split_by_target(tmp_path):
    reads = catalog_reads(71)
    text = fastq(reads)
    (tmp_path / "reads.fq").write_bytes(text)
    files = [os.path.join(CATALOG, f) for f in os.listdir(CATALOG)]
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    table = lm.label_kmers([ts.fasta_records(f) for f in files], 31, True)
    res = ts.run_cli(tmp_path, "bait", "--split-dir", "split", "-t", CATALOG, "reads.fq")
    assert res.stdout == b""
    want = lm.model_label_select(text, table, 31, True, 9)
    any_, multi = lm.model_any_multi(text, table, 31, True, 9)
    rows = (tmp_path / "split" / "labels.tsv").read_text().splitlines()
    assert rows[0].split("\t") == ["label", "query", "type", "variant_name", "allele", "kmers", "reads", "bytes"]
    assert sorted(os.listdir(tmp_path / "split")) == sorted([s + ".fq" for s in stems] + ["labels.tsv"])
    for l, (f, stem) in enumerate(zip(files, stems)):
        got = (tmp_path / "split" / (stem + ".fq")).read_bytes()
        assert got == want[l] and len(got) > 0, stem
        # ... and equals what `bait -t <that file>` alone writes
        err = io.StringIO()                                     # (the command in this process: no interpreter start per target)
        cli.main_bait(cli.parse_args(["bait", "-t", f, "-o", str(tmp_path / "alone.fq"), str(tmp_path / "reads.fq")]), err=err)
        assert (tmp_path / "alone.fq").read_bytes() == got, stem
        n_keys = len(kmers_of(ts.fasta_records(f), 31, True))
        assert ts.figures(err.getvalue().encode())["bait_kmers"] == str(n_keys)
        assert rows[1 + l].split("\t") == [stem, "", "", "", "target", str(n_keys), str(want[l].count(b"\n") // 4), str(len(want[l]))]
    assert ts.figures(res.stderr) == {"labels": "9", "bait_kmers": str(len(table)), "reads_in": str(len(reads)),
                                      "reads_any": str(any_), "reads_multi": str(multi), "bytes_in": str(len(text)),
                                      "pieces": "1", "gather_passes": "1"}
    assert any_ > 0 and len(rows) == 10


def test_cli_split_by_rows(tmp_path):
    case = lm.golden_cases()[0]
    (tmp_path / "npm1.tsv").write_text("\n".join(case["lines"]) + "\n")
    row = [ln.split("\t") for ln in case["lines"] if ln.endswith("vs_ref") and "\tInsertion\t" in ln][0]
    alt, ref = row[8].encode(), row[10].encode()
    site = alt.index(b"TCTGTCTG") + 4                           # the insertion: alt[site - 4 : site] is the inserted TCTG
    assert alt[:site - 4] + alt[site:] == ref
    across_alt = [alt[a:a + 50] for a in range(site - 40, site - 12, 3)]            # hold the whole insertion
    across_ref = [ref[a:a + 50] for a in range(site - 4 - 40, site - 4 - 12, 3)]    # span the unbroken site
    flank = [ref[:31], ref[-31:], alt[:33]]                     # k-mers both alleles have
    rng = np.random.default_rng(72)
    reads = across_alt + across_ref + flank + [random_bases(rng, 50) for _ in range(20)]
    names = [b"alt%d" % i for i in range(len(across_alt))] + [b"ref%d" % i for i in range(len(across_ref))] + \
            [b"flank%d" % i for i in range(len(flank))] + [b"rnd%d" % i for i in range(20)]
    text = fastq(reads, names=names, last_newline=False)
    (tmp_path / "reads.fq").write_bytes(text)
    res = ts.run_cli(tmp_path, "bait", "--split-dir", "rows", "--rows", "npm1.tsv", "--with-ref", "reads.fq")
    stem = "01_NPM1_4ins_exons_10-11utr_Insertion"
    alt_out, ref_out = ((tmp_path / "rows" / (stem + end)).read_bytes() for end in (".alt.fq", ".ref.fq"))
    assert alt_out == fastq(across_alt, names=names[:len(across_alt)])
    assert ref_out == fastq(across_ref, names=names[len(across_alt):len(across_alt) + len(across_ref)])
    rows = [ln.split("\t") for ln in (tmp_path / "rows" / "labels.tsv").read_text().splitlines()]
    assert rows[1] == [stem + ".alt", row[1], "Insertion", "45:/TCTG:45", "alt", "30", str(len(across_alt)), str(len(alt_out))]
    assert rows[2] == [stem + ".ref", row[1], "Insertion", "45:/TCTG:45", "ref", "26", str(len(across_ref)), str(len(ref_out))]
    assert ts.figures(res.stderr) == {"labels": "2", "bait_kmers": "56", "reads_in": str(len(reads)),
                                      "reads_any": str(len(across_alt) + len(across_ref)), "reads_multi": "0",
                                      "bytes_in": str(len(text)), "pieces": "2", "gather_passes": "2"}
    # (two pieces: the file's last record is open, so it waits for the final call)
    # the TSV on standard input, the cluster rows, no reference labels
    res = ts.run_cli(tmp_path, "bait", "--split-dir", "rows2", "--rows", "-", "-i", "cluster", "reads.fq",
                     stdin=(tmp_path / "npm1.tsv").read_bytes())
    assert sorted(os.listdir(tmp_path / "rows2")) == [stem + ".alt.fq", "labels.tsv"]
    assert (tmp_path / "rows2" / (stem + ".alt.fq")).read_bytes() == alt_out


def test_cli_failed_run_leaves_no_label_files(tmp_path):
    reads = catalog_reads(73, n_random=10)
    text = fastq(reads)
    (tmp_path / "bad.fq").write_bytes(text[:-30])
    res = ts.run_cli(tmp_path, "bait", "--split-dir", "new", "-t", CATALOG, "bad.fq", ok=False)
    assert res.returncode == 1 and res.stderr.startswith(b"ERROR: bait: ") and b"bad.fq" in res.stderr and b"quality line" in res.stderr
    assert os.listdir(tmp_path / "new") == []                   # the directory it made holds no label file
    # a label file that was there before the run stays; a FASTA input is refused before anything is made
    (tmp_path / "reads.fa").write_bytes(b">r\nACGT\n")
    res = ts.run_cli(tmp_path, "bait", "--split-dir", "never", "-t", CATALOG, "reads.fa", ok=False)
    assert res.returncode == 1 and b"4-line FASTQ" in res.stderr and not os.path.exists(tmp_path / "never")
    # more than 32 labels: refused before anything touches the GPU or the directory
    case = lm.golden_cases()[0]
    head = [ln for ln in case["lines"] if ln.startswith("#") or ln.startswith("Database")]
    rows = [ln for ln in case["lines"] if ln.endswith("vs_ref") and "\tInsertion\t" in ln]
    (tmp_path / "many.tsv").write_text("\n".join(head + rows * 17) + "\n")
    res = ts.run_cli(tmp_path, "bait", "--split-dir", "many", "--rows", "many.tsv", "--with-ref", "bad.fq", ok=False)
    assert res.returncode == 1 and b"17 variant rows give 34 labels" in res.stderr and not os.path.exists(tmp_path / "many")


def test_select_label_files(tmp_path):
    text, table = stream_text(74, n=200)
    (tmp_path / "a.fq").write_bytes(text)
    (tmp_path / "b.fq").write_bytes(text[:-1])
    label_keys = [np.array([key for key, m in table.items() if m >> l & 1], np.uint64) for l in range(5)]
    db = kc.label_table(label_keys, 31, True)
    try:
        keys, masks = db.records()
        assert dict(zip(keys.tolist(), masks.tolist())) == table
        names = ["l%d" % l for l in range(5)]
        stats = kc.select_label_files(db, names, [str(tmp_path / "a.fq"), str(tmp_path / "b.fq")], str(tmp_path / "out" / "deep"))
        want = lm.model_label_select(text, table, 31, True, 5)
        assert stats["files"] == [str(tmp_path / "out" / "deep" / (n + ".fq")) for n in names]
        for path, w in zip(stats["files"], want):
            with open(path, "rb") as fh:
                assert fh.read() == w + w
        assert stats["bytes_out"] == [2 * len(w) for w in want] and stats["records_in"] == 400 and stats["pieces"] == 3   # (b.fq's open last record is a piece of its own)
        with pytest.raises(ValueError):
            kc.select_label_files(db, ["x", "x"], [str(tmp_path / "a.fq")], str(tmp_path / "dup"))
        assert not os.path.exists(tmp_path / "dup")
    finally:
        db.close()
