"""The four consumers of raw FASTQ text cut it alike: Counter.add_fastq (km_counter_add_fastq), Selector
(km_select_add_fastq), Database.fastq_hits (kmjf_fastq_hits) and PairSelector (km_select_pair_add_fastq) send one text
to the device in the same pieces of whole records (csrc/fastq_cut.h), give what a single piece gives, and refuse a
record longer than a staging buffer with one message.  About 2 KB of text through 256-byte staging buffers."""
import tempfile

import numpy as np
import pytest

from km_amd import lib as kmlib
import test_select_cpu as sm

KM_E_CAPACITY = 8
STAGE = 256
K = 5

pytestmark = pytest.mark.gpu


def small_text(seed=21, n=40):
    """n records of 20 to 60 bytes and a dozen of the text's k-mers as the table."""
    rng = np.random.default_rng(seed)
    reads = [sm.random_bases(rng, int(rng.integers(6, 26))) for _ in range(n)]
    text = sm.fastq(reads)
    assert all(20 <= len(b"".join(r)) <= 60 for r in sm.fastq_records(text)) and 1500 < len(text) < 2500
    keys = sorted(sm.kmers_of(reads, K, True))
    table = {key: 1 for key in keys[::len(keys) // 12][:12]}
    assert len(table) == 12
    return text, table


def host_pieces(text, stage):
    """The number of pieces of a final stream, by lib.fastq_cut over windows of `stage` bytes."""
    pos = pieces = 0
    while pos < len(text):
        take = len(text) - pos if len(text) - pos <= stage else kmlib.fastq_cut(text[pos:pos + stage])
        assert 0 < take <= stage
        pos += take
        pieces += 1
    return pieces


def make_db(table):
    keys = np.fromiter(table.keys(), np.uint64, len(table))
    counts = np.fromiter(table.values(), np.uint32, len(table))
    return kmlib.Database.from_records(keys, counts, K, True).upload(0)


def run_all(db, text):
    """One final stream through the four consumers -> what each made of it."""
    out = {"hits": db.fastq_hits(text).tolist()}
    with tempfile.TemporaryFile() as fh:
        with kmlib.Selector(db, fh, min_hits=1) as sel:
            assert sel.add_fastq(text, final=True) == len(text)
            out["select_stats"] = sel.stats()
        fh.seek(0)
        out["select"] = fh.read()
    with tempfile.TemporaryFile() as fh1, tempfile.TemporaryFile() as fh2:
        with kmlib.PairSelector(db, fh1, fh2, min_hits=1) as sel:
            assert sel.add_fastq(text, text, final=True) == (len(text), len(text))
            out["pair_stats"] = sel.stats()
        fh1.seek(0)
        fh2.seek(0)
        out["pair"] = (fh1.read(), fh2.read())
    with kmlib.Counter(k=K, canonical=True) as counter:
        assert counter.add_fastq(text, final=True) == len(text)
        out["kmers"] = counter.stats()["kmers"]
    return out


def test_the_four_consumers_cut_alike(monkeypatch):
    text, table = small_text()
    pieces = host_pieces(text, STAGE)
    assert pieces > len(text) // STAGE                     # (no piece is longer than a buffer)
    db = make_db(table)
    try:
        monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(STAGE))
        cut = run_all(db, text)
        monkeypatch.delenv("KM_COUNT_STAGE_BYTES")            # (read per object: the next ones have the default size)
        whole = run_all(db, text)
        print("pieces: host %d, selector %d / %d, pair %d / %d" % (pieces, cut["select_stats"]["pieces"],
              whole["select_stats"]["pieces"], cut["pair_stats"]["pieces"], whole["pair_stats"]["pieces"]))
        assert cut["select_stats"]["pieces"] == pieces and cut["pair_stats"]["pieces"] == pieces
        assert whole["select_stats"]["pieces"] == 1 and whole["pair_stats"]["pieces"] == 1
        # the single-piece run against the model, then the cut run against the single-piece run
        assert whole["hits"] == sm.model_hits(text, table, K, True) and any(whole["hits"]) and not all(whole["hits"])
        assert whole["select"] == sm.model_select(text, table, K, True, 1)
        assert cut["hits"] == whole["hits"]
        assert cut["select"] == whole["select"]
        assert cut["pair"] == whole["pair"] == (whole["select"], whole["select"])
        for name in ("records_in", "records_out", "bytes_in", "bytes_out"):
            assert cut["select_stats"][name] == whole["select_stats"][name], name
        for name in ("pairs_in", "pairs_out", "bytes_in", "bytes_out", "resent_bytes"):
            assert cut["pair_stats"][name] == whole["pair_stats"][name], name
        assert cut["kmers"] == whole["kmers"] > 0
    finally:
        db.close()


def test_a_record_longer_than_a_buffer_fails_alike(monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(STAGE))
    rng = np.random.default_rng(22)
    short = [sm.random_bases(rng, 20), sm.random_bases(rng, 11)]
    long_one = sm.fastq([sm.random_bases(rng, 145)], names=[b"bigg"])
    assert len(long_one) == 300
    first_two = len(sm.fastq(short))
    text = sm.fastq(short) + long_one + sm.fastq(short)
    db = make_db(sm.kmers_of(short, K, True))
    details = {}

    def refused(name, call):
        with pytest.raises(kmlib.KmError) as e:
            call()
        assert e.value.code == KM_E_CAPACITY, name
        detail = e.value.detail
        assert "the %d bytes" % STAGE in detail and detail.endswith("byte offset %d" % first_two), (name, detail)
        details[name] = detail

    try:
        refused("fastq_hits", lambda: db.fastq_hits(text))
        with kmlib.Counter(k=K, canonical=True) as counter:
            refused("counter", lambda: counter.add_fastq(text, final=True))
        with tempfile.TemporaryFile() as fh:
            with kmlib.Selector(db, fh) as sel:
                refused("selector", lambda: sel.add_fastq(text, final=True))
                refused("selector, next call", lambda: sel.add_fastq(text[:first_two], final=True))
            fh.seek(0)
            assert fh.read() == text[:first_two]               # the piece before it is written
        with tempfile.TemporaryFile() as fh1, tempfile.TemporaryFile() as fh2:
            with kmlib.PairSelector(db, fh1, fh2) as sel:
                refused("pair", lambda: sel.add_fastq(text, text, final=True))
                refused("pair, next call", lambda: sel.add_fastq(text[:first_two], text[:first_two], final=True))
            fh1.seek(0)
            fh2.seek(0)
            assert fh1.read() == fh2.read() == text[:first_two]
        assert len(details) == 6 and len(set(details.values())) == 1, details
    finally:
        db.close()
