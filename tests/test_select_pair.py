"""The paired selection of FASTQ reads on the GPU: lib.PairSelector (km_select_pair_*), count.select_pair_files and
`python -m km_amd bait -1 .. -2 ..`.

Every comparison is exact, integers equal and outputs byte-identical, against model_pair_select of
tests/test_select_pair_cpu.py, which is written from the rule of include/kmgpu.h.  The sizes are the ends of what a wave
(64 pairs) and a block (256) of k_pair_sizes and a scan chunk (4 096) own, staging buffers of 256 and 4 096 bytes where
the two mates' pieces hold different numbers of records, and names that cross 16-byte boundaries at every residue."""
import ctypes as C
import gzip
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from km_amd import lib as kmlib
from oracle import km_oracle as ko
import test_select_cpu as sm
import test_select_pair_cpu as pm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLT3 = os.path.join(HERE, "data", "catalog", "GRCh38", "FLT3-ITD_exons_13-15.fa")
KM_E_IO, KM_E_FORMAT, KM_E_ARG, KM_E_STATE = 1, 2, 4, 7
COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")
RULES = pm.RULES

pytestmark = pytest.mark.gpu

fastq, random_bases, kmers_of, model = sm.fastq, sm.random_bases, sm.kmers_of, pm.model_pair_select


# ------------------------------------------------------------------ helpers
def make_db(table):
    keys = np.fromiter(table.keys(), np.uint64, len(table))
    counts = np.fromiter(table.values(), np.uint32, len(table))
    return kmlib.Database.from_records(keys, counts, 31, True).upload(0)


def feed(sel, text1, text2, cuts=None):
    """Two streams through a PairSelector: one final call, or with cuts = (offsets into stream 1, offsets into stream 2,
    equally many) block by block with either unconsumed tail carried forward -> the bytes consumed of either."""
    if cuts is None:
        return sel.add_fastq(text1, text2, final=True)
    assert len(cuts[0]) == len(cuts[1])
    blocks = [[text[a:b] for a, b in zip([0] + list(c), list(c) + [len(text)])] for text, c in zip((text1, text2), cuts)]
    tails, consumed = [b"", b""], [0, 0]
    for blk1, blk2 in zip(*blocks):
        bufs = [tails[0] + blk1, tails[1] + blk2]
        used = sel.add_fastq(bufs[0], bufs[1], final=False)
        for m in (0, 1):
            assert used[m] <= len(bufs[m])
            consumed[m] += used[m]
            tails[m] = bufs[m][used[m]:]
    used = sel.add_fastq(tails[0], tails[1], final=True)
    return consumed[0] + used[0], consumed[1] + used[1]


def pair_select(db, text1, text2, cuts=None, **kwargs):
    """-> (out1, out2, stats, (consumed1, consumed2))"""
    with tempfile.TemporaryFile() as f1, tempfile.TemporaryFile() as f2:
        with kmlib.PairSelector(db, f1, f2, **kwargs) as sel:
            consumed = feed(sel, text1, text2, cuts)
            stats = sel.stats()
        f1.seek(0)
        f2.seek(0)
        return f1.read(), f2.read(), stats, consumed


def model_kwargs(kwargs):
    out = {"min_hits": kwargs.get("min_hits", 1), "invert": kwargs.get("invert", False), "rule": kwargs.get("rule", "any"),
           "check_names": kwargs.get("check_names", True)}
    q = kwargs.get("min_qual_char")
    out["min_qual"] = 0 if q is None else kmlib._qual_byte(q)
    return out


def check(db, text1, text2, table, ctx=None, cuts=None, **kwargs):
    """One pair of final streams against the model, outputs and stats -> (out1, out2, stats)."""
    mk = model_kwargs(kwargs)
    want = model(text1, text2, table, 31, True, **mk)
    out1, out2, stats, consumed = pair_select(db, text1, text2, cuts=cuts, **kwargs)
    assert (out1, out2) == want, (ctx, len(out1), len(want[0]), len(out2), len(want[1]))
    assert consumed == (len(text1), len(text2)), ctx
    n_pairs = len(sm.fastq_records(text1)) if text1 else 0
    kept = len(pm.kept_pairs(text1, text2, table, 31, True, mk["min_hits"], mk["invert"], mk["min_qual"], mk["rule"])) if text1 else 0
    assert stats == {"pairs_in": n_pairs, "pairs_out": kept, "bytes_in": [len(text1), len(text2)],
                     "bytes_out": [len(want[0]), len(want[1])], "pieces": stats["pieces"], "resent_bytes": stats["resent_bytes"]}, ctx
    return out1, out2, stats


@pytest.fixture
def small_buffers(monkeypatch):
    """Buffers of 1 MiB: one piece per call for everything here that does not ask for more, without the time the default
    16 MiB ones take to allocate."""
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(1 << 20))


# ------------------------------------------------------------------ shapes
_EDGE = {}


def edge_texts():
    """4 097 pairs of 40-nt reads, made once: every prefix of whole pairs is a case."""
    if not _EDGE:
        t1, t2, table = pm.pair_texts(50, 4097)
        _EDGE["recs"] = ([b"".join(r) for r in sm.fastq_records(t1)], [b"".join(r) for r in sm.fastq_records(t2)])
        _EDGE["table"] = table
    return _EDGE["recs"], _EDGE["table"]


@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_pair_counts_at_the_edges(small_buffers, n_pairs):
    (recs1, recs2), table = edge_texts()
    text1, text2 = b"".join(recs1[:n_pairs]), b"".join(recs2[:n_pairs])
    db = make_db(table)
    try:
        outs = {}
        for rule in RULES:
            out1, out2, stats = check(db, text1, text2, table, ctx=(n_pairs, rule), rule=rule, min_hits=10)
            assert stats["pieces"] == 1 and stats["resent_bytes"] == [0, 0]
            outs[rule] = (out1, out2)
            if n_pairs >= 63:
                assert 0 < stats["pairs_out"] < n_pairs, rule
        if n_pairs >= 63:
            assert len({outs[r] for r in RULES}) == 3
            assert len(outs["both"][0]) < len(outs["any"][0]) < len(outs["sum"][0])
        check(db, text1, text2, table, ctx=(n_pairs, "-v"), rule="both", min_hits=10, invert=True, check_names=False)
    finally:
        db.close()


def unequal_texts(seed=60, n=1500):
    return pm.pair_texts(seed, n, lengths=((20, 90), (20, 90)))


@pytest.mark.parametrize("stage", [256, 4096, None])
def test_unequal_pieces(monkeypatch, stage):
    if stage is None:
        monkeypatch.delenv("KM_COUNT_STAGE_BYTES", raising=False)
    else:
        monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))
    monkeypatch.setenv("KM_SELECT_TIME", "1")
    text1, text2, table = unequal_texts()
    assert len(text1) != len(text2) and max(len(b"".join(r)) for t in (text1, text2) for r in sm.fastq_records(t)) <= 256
    db = make_db(table)
    try:
        for rule, min_hits in (("any", 1), ("both", 2), ("sum", 40)):
            out1, out2, stats = check(db, text1, text2, table, ctx=(stage, rule), rule=rule, min_hits=min_hits)
            assert 0 < stats["pairs_out"] < stats["pairs_in"] == 1500
            if stage is None:
                assert stats["pieces"] == 1 and stats["resent_bytes"] == [0, 0]
            else:
                assert stats["resent_bytes"][0] > 0 and stats["resent_bytes"][1] > 0
                assert stats["pieces"] >= max(len(text1), len(text2)) // stage
                if stage == 256:
                    assert stats["pieces"] > 20
        ms = kmlib.select_kernel_ms()
        assert ms["front"] > 0 and ms["hits"] > 0 and ms["sizes"] > 0 and ms["gather"] > 0
    finally:
        db.close()


def test_two_hundred_random_cuts_per_stream(monkeypatch):
    text1, text2, table = unequal_texts(seed=61)
    rng = np.random.default_rng(62)
    cuts = (sorted(rng.integers(1, len(text1), 200).tolist()), sorted(rng.integers(1, len(text2), 200).tolist()))
    db = make_db(table)
    try:
        for stage in (1 << 20, 4096):
            monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))
            whole = check(db, text1, text2, table, rule="sum", min_hits=3)
            got = check(db, text1, text2, table, cuts=cuts, rule="sum", min_hits=3)
            assert got[:2] == whole[:2]
            same = ("pairs_in", "pairs_out", "bytes_in", "bytes_out")
            assert {f: got[2][f] for f in same} == {f: whole[2][f] for f in same}
    finally:
        db.close()


def test_one_stream_far_ahead(small_buffers):
    text1, text2, table = unequal_texts(seed=63, n=600)
    db = make_db(table)
    try:
        want = model(text1, text2, table, 31, True)
        for ahead in (0, 1):
            texts = (text1, text2)
            with tempfile.TemporaryFile() as f1, tempfile.TemporaryFile() as f2:
                with kmlib.PairSelector(db, f1, f2) as sel:
                    far, near, done = texts[ahead], b"", 0
                    blocks = [texts[1 - ahead][a:a + 700] for a in range(0, len(texts[1 - ahead]), 700)]
                    for i, blk in enumerate(blocks):
                        near += blk
                        used = sel.add_fastq(*((far, near) if ahead == 0 else (near, far)), final=False)
                        far, near = far[used[ahead]:], near[used[1 - ahead]:]
                        done += used[1 - ahead]
                        assert len(near) < 256                       # whole records of the slow side are all taken
                        assert len(far) > 0 or i == len(blocks) - 1
                    assert done > 0 and len(blocks) > 50
                    used = sel.add_fastq(*((far, near) if ahead == 0 else (near, far)), final=True)
                    assert used[ahead] == len(far) and used[1 - ahead] == len(near)
                    stats = sel.stats()
                f1.seek(0)
                f2.seek(0)
                assert (f1.read(), f2.read()) == want
            assert stats["pairs_in"] == 600 and stats["bytes_in"] == [len(text1), len(text2)]
            assert stats["resent_bytes"][ahead] > 0
    finally:
        db.close()


def test_agreement_with_fastq_hits(small_buffers):
    text1, text2, table = unequal_texts(seed=64, n=800)
    db = make_db(table)
    try:
        h1, h2 = db.fastq_hits(text1), db.fastq_hits(text2)
        keep = (h1 > 0) | (h2 > 0)
        assert 0 < keep.sum() < keep.size == 800
        out1, out2, stats, _ = pair_select(db, text1, text2)
        recs1 = [b"".join(r) for r in sm.fastq_records(text1)]
        recs2 = [b"".join(r) for r in sm.fastq_records(text2)]
        assert out1 == b"".join(r for r, kp in zip(recs1, keep) if kp) and out2 == b"".join(r for r, kp in zip(recs2, keep) if kp)
        assert stats["pairs_out"] == int(keep.sum())
    finally:
        db.close()


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("last_newline", [(False, True), (True, False), (False, False)])
def test_invert_min_hits_quality_and_line_ends(small_buffers, last_newline):
    t1, t2, table = pm.pair_texts(65, 150, lengths=(60, (35, 70)), eol=b"\r\n", quals=True, last_newline=last_newline)
    assert t1.endswith(b"\n") == last_newline[0] and t2.endswith(b"\n") == last_newline[1] and b"\r\n" in t1
    db = make_db(table)
    try:
        seen = set()
        for rule in RULES:
            for min_hits in (1, 2, 3):
                for invert in (False, True):
                    for q in (None, "5"):
                        out = check(db, t1, t2, table, ctx=(rule, min_hits, invert, q), rule=rule, min_hits=min_hits,
                                    invert=invert, min_qual_char=q)
                        seen.add(out[:2])
        assert len(seen) >= 12
        # the last pair kept: both outputs end in a newline of the host's where the input had none
        keep_last = table.copy()
        keep_last.update(kmers_of([sm._content(sm.fastq_records(t1)[-1][1])], 31, True))
        db2 = make_db(keep_last)
        try:
            out1, out2, stats = check(db2, t1, t2, keep_last)
            last1, last2 = b"".join(sm.fastq_records(t1)[-1]), b"".join(sm.fastq_records(t2)[-1])
            assert out1.endswith(last1 + (b"" if last_newline[0] else b"\n")) and out2.endswith(last2 + (b"" if last_newline[1] else b"\n"))
            # two pairs of streams through one selector do not run together
            with tempfile.TemporaryFile() as f1, tempfile.TemporaryFile() as f2:
                with kmlib.PairSelector(db2, f1, f2) as sel:
                    assert sel.add_fastq(t1, t2, final=True) == (len(t1), len(t2))
                    assert sel.add_fastq(t1, t2, final=True) == (len(t1), len(t2))
                    assert sel.stats()["bytes_out"] == [2 * len(out1), 2 * len(out2)]
                f1.seek(0)
                f2.seek(0)
                assert (f1.read(), f2.read()) == (out1 + out1, out2 + out2)
        finally:
            db2.close()
    finally:
        db.close()


def test_all_dropped_all_kept_and_empty_calls(small_buffers):
    t1, t2, table = pm.pair_texts(66, 500)
    db = make_db(table)
    try:
        out1, out2, stats = check(db, t1, t2, table, min_hits=1000)
        assert (out1, out2) == (b"", b"") and stats["pairs_out"] == 0
        out1, out2, stats = check(db, t1, t2, table, min_hits=1000, invert=True)
        assert (out1, out2) == (t1, t2) and stats["pairs_out"] == 500
        with tempfile.TemporaryFile() as f1, tempfile.TemporaryFile() as f2:
            with kmlib.PairSelector(db, f1, f2) as sel:
                assert sel.add_fastq(b"", b"", final=True) == (0, 0) and sel.add_fastq(b"", b"", final=False) == (0, 0)
                assert sel.add_fastq(t1, b"", final=False) == (0, 0) and sel.add_fastq(b"", t2, final=False) == (0, 0)
                assert sel.add_fastq(t1[:50], t2, final=False) == (0, 0)          # no whole record on one side
                assert sel.stats() == {"pairs_in": 0, "pairs_out": 0, "bytes_in": [0, 0], "bytes_out": [0, 0], "pieces": 0,
                                       "resent_bytes": [0, 0]}
                assert sel.add_fastq(t1, t2, final=False) == (len(t1), len(t2))
                assert sel.add_fastq(b"", b"", final=True) == (0, 0)              # ends the streams: indices start again
                bad = t2.replace(b"@read4/2\n", b"@other\n", 1)
                assert bad != t2
                with pytest.raises(kmlib.KmError) as e:
                    sel.add_fastq(t1, bad, final=True)
                assert "pair 4:" in str(e.value)
    finally:
        db.close()


# ------------------------------------------------------------------ names
def test_names_at_every_residue(small_buffers):
    """Names of 0 .. 40 bytes behind headers at every offset mod 16, with and without /1, /2 and comments."""
    t1, t2, table = pm.pair_texts(67, 41 * 16, lengths=((33, 48), (33, 48)), name_lengths=list(range(41)))
    for t in (t1, t2):
        at, starts, lengths = 0, set(), set()
        for rec in sm.fastq_records(t):
            starts.add((at % 16, len(pm.pair_name(rec[0])) % 16))
            lengths.add(len(pm.pair_name(rec[0])))
            at += len(b"".join(rec))
        assert {s for s, _ in starts} == set(range(16)) and len(starts) > 100 and lengths >= set(range(39))
    db = make_db(table)
    try:
        check(db, t1, t2, table, rule="any")
        check(db, t1.replace(b"\n", b"\r\n"), t2, table, rule="both")
        # each single difference is found, at its pair: a byte changed, a byte more, another suffix
        recs2 = sm.fastq_records(t2)
        for r, change in ((0, lambda h: b"@x" + h[2:] if len(pm.pair_name(h)) else b"@x" + h[1:]),
                          (17, lambda h: b"@" + pm.pair_name(h) + b"y\n"),
                          (200, lambda h: b"@" + pm.pair_name(h) + b"/3\n"),
                          (655, lambda h: b"@" + pm.pair_name(h)[:-1] + b"#" + b" c\n")):
            lines = list(recs2[r])
            lines[0] = change(lines[0])
            bad = b"".join(b"".join(x) for x in recs2[:r]) + b"".join(lines) + b"".join(b"".join(x) for x in recs2[r + 1:])
            with pytest.raises(pm.PairError) as m:
                model(t1, bad, table, 31, True)
            assert (m.value.kind, m.value.index) == ("names", r)
            with tempfile.TemporaryFile() as f1, tempfile.TemporaryFile() as f2:
                with kmlib.PairSelector(db, f1, f2) as sel:
                    with pytest.raises(kmlib.KmError) as e:
                        sel.add_fastq(t1, bad, final=True)
                    assert e.value.code == KM_E_FORMAT and "mate names differ at pair %d:" % r in str(e.value), str(e.value)
    finally:
        db.close()


def test_name_mismatch_in_a_later_piece(monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")
    t1, t2, table = pm.pair_texts(68, 400, lengths=(40, 75))
    recs1, recs2 = sm.fastq_records(t1), sm.fastq_records(t2)
    at = 250
    off1 = sum(len(b"".join(r)) for r in recs1[:at])
    off2 = sum(len(b"".join(r)) for r in recs2[:at])
    assert off2 > 3 * 4096
    bad = t2[:off2] + b"@other" + t2[off2 + t2[off2:].index(b"\n"):]
    with pytest.raises(pm.PairError) as m:
        model(t1, bad, table, 31, True)
    assert (m.value.kind, m.value.index) == ("names", at)
    full = model(t1, bad, table, 31, True, check_names=False)
    kept = pm.kept_pairs(t1, bad, table, 31, True)
    db = make_db(table)
    try:
        with tempfile.TemporaryFile() as f1, tempfile.TemporaryFile() as f2:
            with kmlib.PairSelector(db, f1, f2) as sel:
                with pytest.raises(kmlib.KmError) as e:
                    sel.add_fastq(t1, bad, final=True)
                assert e.value.code == KM_E_FORMAT
                assert "mate names differ at pair %d: the header of mate 1 at byte offset %d, of mate 2 at byte offset %d" % (
                    at, off1, off2) in str(e.value), str(e.value)
                with pytest.raises(kmlib.KmError) as e2:     # and it stays
                    sel.add_fastq(t1, t2, final=True)
                assert e2.value.code == KM_E_FORMAT and str(e2.value) == str(e.value)
                stats = sel.stats()
            f1.seek(0)
            f2.seek(0)
            out1, out2 = f1.read(), f2.read()
        # both outputs are prefixes of the fault-free run's and end at the same pair, which lies before the faulty one
        done = stats["pairs_in"]
        assert 0 < done <= at and stats["pieces"] >= 3
        want1 = b"".join(b"".join(recs1[r]) for r in kept if r < done)
        want2 = b"".join(b"".join(sm.fastq_records(bad)[r]) for r in kept if r < done)
        assert (out1, out2) == (want1, want2) and full[0].startswith(out1) and full[1].startswith(out2) and len(out1) > 0
        assert stats["pairs_out"] == sum(1 for r in kept if r < done)
        # the same input without the check
        check(db, t1, bad, table, check_names=False)
    finally:
        db.close()


# ------------------------------------------------------------------ errors
@pytest.mark.parametrize("short", [1, 2])
def test_count_mismatch(monkeypatch, short):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")
    t1, t2, table = pm.pair_texts(69, 300, lengths=(40, 75))
    texts = [t1, t2]
    recs = sm.fastq_records(texts[short - 1])
    texts[short - 1] = b"".join(b"".join(r) for r in recs[:-1])
    with pytest.raises(pm.PairError) as m:
        model(texts[0], texts[1], table, 31, True)
    assert (m.value.kind, m.value.mate, m.value.index) == ("count", 3 - short, 299)
    cut = [t1, t2]
    cut[2 - short] = b"".join(b"".join(r) for r in sm.fastq_records(cut[2 - short])[:-1])
    cut[short - 1] = texts[short - 1]
    want = model(cut[0], cut[1], table, 31, True)
    db = make_db(table)
    try:
        with tempfile.TemporaryFile() as f1, tempfile.TemporaryFile() as f2:
            with kmlib.PairSelector(db, f1, f2) as sel:
                # not final: the shorter mate may still come
                used = sel.add_fastq(texts[0], texts[1], final=False)
                assert used[short - 1] == len(texts[short - 1]) and used[2 - short] < len(texts[2 - short])
                assert sel.stats()["pairs_in"] == 299
                rest = [texts[0][used[0]:], texts[1][used[1]:]]
                with pytest.raises(kmlib.KmError) as e:
                    sel.add_fastq(rest[0], rest[1], final=True)
                assert e.value.code == KM_E_FORMAT and "mate files differ in their number of records" in str(e.value)
                assert "mate %d has more" % (3 - short) in str(e.value) and "pair 299" in str(e.value), str(e.value)
                with pytest.raises(kmlib.KmError) as e:
                    sel.add_fastq(b"", b"", final=True)
                assert e.value.code == KM_E_FORMAT
            f1.seek(0)
            f2.seek(0)
            assert (f1.read(), f2.read()) == want              # the earlier pieces are written
        # in one final call as well
        with tempfile.TemporaryFile() as f1, tempfile.TemporaryFile() as f2:
            with kmlib.PairSelector(db, f1, f2) as sel:
                with pytest.raises(kmlib.KmError) as e:
                    sel.add_fastq(texts[0], texts[1], final=True)
                assert "mate %d has more" % (3 - short) in str(e.value) and "pair 299" in str(e.value)
            f1.seek(0)
            f2.seek(0)
            assert (f1.read(), f2.read()) == want
    finally:
        db.close()


def test_malformed_record_in_mate_2_in_a_later_piece(monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")
    t1, t2, table = pm.pair_texts(70, 300, lengths=(40, 75))
    recs2 = sm.fastq_records(t2)
    at = 200
    off = sum(len(b"".join(r)) for r in recs2[:at]) + len(recs2[at][0]) + len(recs2[at][1])
    assert t2[off:off + 1] == b"+" and off > 3 * 4096
    bad = t2[:off] + b"-" + t2[off + 1:]
    with pytest.raises(pm.PairError) as m:
        model(t1, bad, table, 31, True)
    assert (m.value.kind, m.value.mate, m.value.cause.kind, m.value.cause.offset) == ("malformed", 2, sm.NO_PLUS, off)
    full = model(t1, t2, table, 31, True)
    db = make_db(table)
    try:
        with tempfile.TemporaryFile() as f1, tempfile.TemporaryFile() as f2:
            with kmlib.PairSelector(db, f1, f2) as sel:
                with pytest.raises(kmlib.KmError) as e:
                    sel.add_fastq(t1, bad, final=True)
                assert e.value.code == KM_E_FORMAT and "mate 2" in str(e.value) and sm.KIND_TEXT[sm.NO_PLUS] in str(e.value)
                assert str(e.value).endswith("at byte offset %d" % off), str(e.value)
                stats = sel.stats()
            f1.seek(0)
            f2.seek(0)
            out1, out2 = f1.read(), f2.read()
        done = stats["pairs_in"]
        kept = pm.kept_pairs(t1, t2, table, 31, True)
        assert 0 < done <= at and len(out1) > 0
        assert out1 == b"".join(b"".join(sm.fastq_records(t1)[r]) for r in kept if r < done)
        assert out2 == b"".join(b"".join(recs2[r]) for r in kept if r < done)
        assert full[0].startswith(out1) and full[1].startswith(out2)
        # mate 1, in the first piece: nothing is written
        with tempfile.TemporaryFile() as f1, tempfile.TemporaryFile() as f2:
            with kmlib.PairSelector(db, f1, f2) as sel:
                with pytest.raises(kmlib.KmError) as e:
                    sel.add_fastq(b"#" + t1[1:], t2, final=True)
                assert "mate 1" in str(e.value) and str(e.value).endswith("at byte offset 0")
            f1.seek(0)
            f2.seek(0)
            assert (f1.read(), f2.read()) == (b"", b"")
    finally:
        db.close()


def test_argument_state_and_descriptor_errors(small_buffers):
    t1, t2, table = pm.pair_texts(71, 50)
    db = make_db(table)
    lib = kmlib.load()
    try:
        with tempfile.TemporaryFile() as f1, tempfile.TemporaryFile() as f2:
            for kwargs in ({"min_hits": 0}, {"min_qual_char": 256}, {"min_qual_char": -1}, {"rule": "either"}, {"rule": 3}, {"rule": -1}):
                with pytest.raises(kmlib.KmError) as e:
                    kmlib.PairSelector(db, f1, f2, **kwargs)
                assert e.value.code == KM_E_ARG, kwargs
            with pytest.raises(kmlib.KmError) as e:
                kmlib.PairSelector(db, f1, f1)
            assert e.value.code == KM_E_ARG
            with pytest.raises(kmlib.KmError) as e:
                kmlib.PairSelector(db, f1.fileno(), f1.fileno())
            assert e.value.code == KM_E_ARG
            s = C.c_void_p()
            assert lib.km_select_pair_create(db._h, 1, 0, 0, 0, 1, f1.fileno(), f2.fileno(), None, None) == KM_E_ARG
            assert lib.km_select_pair_create(None, 1, 0, 0, 0, 1, f1.fileno(), f2.fileno(), None, C.byref(s)) == KM_E_ARG
            with kmlib.PairSelector(db, f1, f2, rule=2) as sel:
                used = (C.c_uint64(), C.c_uint64())
                assert lib.km_select_pair_add_fastq(sel._s, None, 5, t2, len(t2), 1, C.byref(used[0]), C.byref(used[1])) == KM_E_ARG
                assert lib.km_select_pair_add_fastq(sel._s, t1, len(t1), None, 5, 1, C.byref(used[0]), C.byref(used[1])) == KM_E_ARG
                assert lib.km_select_pair_add_fastq(sel._s, t1, len(t1), t2, len(t2), 1, None, C.byref(used[1])) == KM_E_ARG
                assert lib.km_select_pair_add_fastq(sel._s, t1, len(t1), t2, len(t2), 1, C.byref(used[0]), None) == KM_E_ARG
                assert lib.km_select_pair_stats(sel._s, None) == KM_E_ARG
                assert sel.stats()["pieces"] == 0
            f1.seek(0)
            assert f1.read() == b""
            # a descriptor that is not open, on either side
            r, w = os.pipe()
            os.close(r)
            os.close(w)
            for outs in ((w, f2), (f1, w)):
                with pytest.raises(kmlib.KmError) as e:
                    kmlib.PairSelector(db, *outs)
                assert e.value.code == KM_E_IO
            # a reader of mate 2 that went away: the code, and the selector is dead
            r, w = os.pipe()
            os.close(r)
            try:
                with kmlib.PairSelector(db, f1, w, min_hits=1000, invert=True) as sel:
                    for _ in range(2):
                        with pytest.raises(kmlib.KmError) as e:
                            sel.add_fastq(t1, t2, final=True)
                        assert e.value.code == KM_E_IO and "writing the text failed" in str(e.value)
            finally:
                os.close(w)
        assert pair_select(db, t1, t2, min_hits=1000, invert=True)[:2] == (t1, t2)
    finally:
        db.close()
    host_only = kmlib.Database.from_records(np.array([1], np.uint64), np.array([1], np.uint32), 31, True)
    try:
        with tempfile.TemporaryFile() as f1, tempfile.TemporaryFile() as f2:
            with pytest.raises(kmlib.KmError) as e:
                kmlib.PairSelector(host_only, f1, f2)
            assert e.value.code == KM_E_STATE
    finally:
        host_only.close()


# ------------------------------------------------------------------ the command
def run_cli(tmp_path, *args, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system")
    env.pop("KM_COUNT_STAGE_BYTES", None)
    res = subprocess.run([sys.executable, "-m", "km_amd"] + list(args), cwd=tmp_path, capture_output=True, timeout=300, env=env)
    if ok:
        assert res.returncode == 0, res.stderr
    return res


def figures(stderr):
    return dict(line[1:].split(":") for line in stderr.decode().splitlines() if line.startswith("#"))


def flt3_pairs(seed, n_target=300, n_random=300):
    """Mates cut from the two ends of fragments of the FLT3-ITD target (mate 2 from the other strand), and random pairs,
    shuffled -> (text1, text2)."""
    rng = np.random.default_rng(seed)
    ref = ko.read_fasta_concat(FLT3).encode("ascii")
    pairs = []
    for _ in range(n_target):
        a = int(rng.integers(0, len(ref) - 260))
        frag = ref[a:a + int(rng.integers(180, 260))]
        pairs.append((frag[:100], frag[-100:].translate(COMPLEMENT)[::-1]))
    pairs += [(random_bases(rng, 100), random_bases(rng, 100)) for _ in range(n_random)]
    order = rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    names = [b"frag%d" % i for i in range(len(pairs))]
    return (fastq([p[0] for p in pairs], names=[n + b"/1" for n in names]),
            fastq([p[1] for p in pairs], names=[n + b"/2" for n in names]))


def fasta_records(path):
    records = []
    with open(path, "rb") as fh:
        for line in fh:
            if line.startswith(b">"):
                records.append([])
            elif records:
                records[-1].append(line.strip())
    return [b"".join(r) for r in records]


def test_cli_paired_bait(tmp_path):
    a1, a2 = flt3_pairs(72)
    b1, b2 = flt3_pairs(73, n_target=100, n_random=200)
    for name, text in (("a_1.fq.gz", a1), ("a_2.fq.gz", a2)):
        with gzip.open(tmp_path / name, "wb") as fh:
            fh.write(text)
    (tmp_path / "b_1.fq").write_bytes(b1)
    (tmp_path / "b_2.fq").write_bytes(b2)
    table = kmers_of(fasta_records(FLT3), 31, True)
    # -t, a gzip pair and a plain pair: two pairs of streams
    want_a, want_b = model(a1, a2, table, 31, True), model(b1, b2, table, 31, True)
    res = run_cli(tmp_path, "bait", "-t", FLT3, "-1", "a_1.fq.gz", "-1", "b_1.fq", "-2", "a_2.fq.gz", "-2", "b_2.fq",
                  "-o", "out_1.fq", "-O", "out_2.fq")
    out1, out2 = (tmp_path / "out_1.fq").read_bytes(), (tmp_path / "out_2.fq").read_bytes()
    assert res.stdout == b"" and (out1, out2) == (want_a[0] + want_b[0], want_a[1] + want_b[1])
    n_out = out1.count(b"\n") // 4
    assert 300 < n_out < 900 and out2.count(b"\n") // 4 == n_out
    assert figures(res.stderr) == {"bait_kmers": str(len(table)), "pairs_in": "900", "pairs_out": str(n_out),
                                   "bytes_in_1": str(len(a1) + len(b1)), "bytes_in_2": str(len(a2) + len(b2)),
                                   "bytes_out_1": str(len(out1)), "bytes_out_2": str(len(out2)), "pieces": "2", "pair_rule": "any"}
    # -d with a table written by count, --pair-rule both, -n, -v, --no-name-check
    run_cli(tmp_path, "count", "-m", "31", "-C", "-o", "bait.jf", FLT3)
    want = model(b1, b2.replace(b"/2\n", b"x\n"), table, 31, True, min_hits=5, invert=True, rule="both", check_names=False)
    (tmp_path / "c_2.fq").write_bytes(b2.replace(b"/2\n", b"x\n"))
    res = run_cli(tmp_path, "bait", "-d", "bait.jf", "-n", "5", "-v", "--pair-rule", "both", "--no-name-check", "-1", "b_1.fq",
                  "-2", "c_2.fq", "-o", "inv_1.fq", "-O", "inv_2.fq")
    assert ((tmp_path / "inv_1.fq").read_bytes(), (tmp_path / "inv_2.fq").read_bytes()) == want and 0 < len(want[0]) < len(b1)
    fig = figures(res.stderr)
    assert fig["pair_rule"] == "both" and fig["pairs_in"] == "300" and fig["bytes_out_2"] == str(len(want[1]))
    # a failing run removes the outputs it created and leaves one that was there
    (tmp_path / "old_2.fq").write_bytes(b"before\n")
    res = run_cli(tmp_path, "bait", "-d", "bait.jf", "-1", "b_1.fq", "-2", "c_2.fq", "-o", "new_1.fq", "-O", "old_2.fq", ok=False)
    assert res.returncode == 1 and res.stderr.startswith(b"ERROR: bait: ") and b"mate names differ at pair 0" in res.stderr
    assert b"b_1.fq, c_2.fq" in res.stderr
    assert not (tmp_path / "new_1.fq").exists() and (tmp_path / "old_2.fq").exists()
    (tmp_path / "old_2.fq").write_bytes(b"before\n")
    for wrong in ("none.fq", "bait.jf"):                         # found before either output is opened
        res = run_cli(tmp_path, "bait", "-d", "bait.jf", "-1", "b_1.fq", "-2", wrong, "-o", "new_1.fq", "-O", "old_2.fq", ok=False)
        assert res.returncode == 1 and res.stderr.startswith(b"ERROR: bait: ")
        assert not (tmp_path / "new_1.fq").exists() and (tmp_path / "old_2.fq").read_bytes() == b"before\n"
    # the argument rules through the command itself
    res = run_cli(tmp_path, "bait", "-d", "bait.jf", "-1", "b_1.fq", "-2", "b_2.fq", "-o", "x.fq", ok=False)
    assert res.returncode == 2


def test_paired_bait_then_count_then_find_mutation(tmp_path):
    """Mates of the FLT3 sample of tests/test_count.py among random pairs: the kept mate-1 and mate-2 files, counted into
    one table, give find_mutation the rows of the whole sample."""
    import test_count as tc
    ref, sample = tc.itd_reads()
    rng = np.random.default_rng(74)
    half = len(sample) // 2
    mates1, mates2 = list(sample[:half]), [r.translate(COMPLEMENT)[::-1] for r in sample[half:2 * half]]
    noise = [(random_bases(rng, 100), random_bases(rng, 100)) for _ in range(half)]
    reads1 = [r for pair in zip(mates1, (n[0] for n in noise)) for r in pair]
    reads2 = [r for pair in zip(mates2, (n[1] for n in noise)) for r in pair]
    (tmp_path / "mixed_1.fq").write_bytes(fastq(reads1))
    (tmp_path / "mixed_2.fq").write_bytes(fastq(reads2))
    (tmp_path / "sample.fq").write_bytes(fastq(mates1 + mates2))
    res = run_cli(tmp_path, "bait", "-t", FLT3, "-1", "mixed_1.fq", "-2", "mixed_2.fq", "-o", "baited_1.fq", "-O", "baited_2.fq")
    fig = figures(res.stderr)
    assert fig["pairs_in"] == str(2 * half) and 0 < int(fig["pairs_out"]) <= half
    table = kmers_of(fasta_records(FLT3), 31, True)
    assert ((tmp_path / "baited_1.fq").read_bytes(), (tmp_path / "baited_2.fq").read_bytes()) == model(
        fastq(reads1), fastq(reads2), table, 31, True)
    rows = {}
    for name, files in (("baited", ["baited_1.fq", "baited_2.fq"]), ("sample", ["sample.fq"])):
        run_cli(tmp_path, "count", "-m", "31", "-C", "-L", "2", "-o", name + ".jf", *files)
        res = run_cli(tmp_path, "find_mutation", FLT3, name + ".jf")
        body = [ln for ln in res.stdout.decode().splitlines() if not ln.startswith("#")]
        rows[name] = [ln.split("\t", 1)[1] for ln in body[1:]]
    assert rows["baited"] == rows["sample"] and any(r.split("\t")[1] == "ITD" for r in rows["sample"]), (rows["baited"], rows["sample"])
