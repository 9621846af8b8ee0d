"""The kernels that cut k-mers out of text at every k from 2 to 32 and on structured text: k_count_insert
(Counter.add_bases / add_text), k_fq_mask + insert (Counter.add_fastq), k_scan_stats / k_scan_text (Database.cov_seqs /
scan_text), k_sel_hits .. k_sel_gather (Database.fastq_hits, Selector) and the pair kernels (PairSelector).

Every lane of these kernels rolls a forward and a reverse-complement key over its 64 bytes; the places where that goes
wrong are k = 32 (no mask, a shift by 62, keys at and above 2^63, T^32 = the counter's empty mark), even k (palindromes:
fwd == rev), k = 2 .. 4 (more windows than bytes in a word, the whole key space in the table), k = 16 / 17 (2k crosses
32 bits) and low-complexity text (one key under every lane of a wave).  One structured corpus per k goes through all of
them.  Every comparison is exact, integers equal and bytes identical, against the plain-Python models of
tests/test_count.py, test_count_quality.py, test_scan_cpu.py, test_select_cpu.py and test_select_pair_cpu.py; what a
corpus is meant to show is asserted from the models' side first (corpus_case), before anything touches the GPU."""
import functools

import numpy as np
import pytest

from km_amd import lib as kmlib
import test_count as tc
from test_count_filter_cpu import canonical_key
import test_count_quality as tq
import test_scan as ts
import test_scan_cpu as sc
import test_select as tsel
import test_select_cpu as sm
import test_select_pair as tpair
import test_select_pair_cpu as pm
from test_structured_kmers import EDGE_COUNTS

gpu = pytest.mark.gpu
U32 = 0xFFFFFFFF
ALL_T = 0xFFFFFFFFFFFFFFFF
TOP_BIT = 1 << 63
COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
BASES = b"ACGTacgt"
EVERY_K = list(range(2, 33))
RULE_KS = (2, 3, 4, 16, 17, 30, 32)          # the k of the CPU rule programs' structured cases
LOW_QUAL = ord("#")                          # below '+', not below '!'


def revcomp(seq):
    return seq.translate(COMPLEMENT)[::-1]


# ------------------------------------------------------------------ the corpus
def n_positions(k, length):
    """Where a read of `length` bases gets its non-base, one list per read: the first byte, the last byte of the first
    window, the first byte behind it, the last byte a lane owns and the first of its neighbour's, the read's last byte,
    and every k-th byte."""
    return [[0], [k - 1], [k], [31], [32], [length - 1], list(range(0, length, k))]


def structured_reads(k, small=False):
    """The structured corpus of one k: a few hundred reads, under about 20 KB of bases (small: a few KB and no read
    above 110 bases, for the sanitizer builds of the CPU rule programs)."""
    rng = np.random.default_rng(7100 + k)

    def rb(n):
        return sc.random_bases(rng, n)

    # a lane's 32 starts, its 64 loaded bytes, a wave's 2 048 starts
    lengths = [k - 1, k, k + 1, 31, 32, 33, 32 + k - 1, 63, 64, 65] + ([] if small else [2047, 2048, 2049])
    reads = [rb(n) for n in lengths]
    homo, sat = (100, 96) if small else (200, 150)
    for base in (b"A", b"C", b"G", b"T"):                    # one key under every lane
        reads += [base * n for n in (k, k + 1, homo)]
    for period in range(2, 7):                               # microsatellites, upper and lower case
        unit = rb(period)
        while len(set(unit)) < 2:
            unit = rb(period)
        s = (unit * (sat // period + 1))[:sat]
        reads += [s, s.lower()]
    if k % 2 == 0:                                           # palindromes: fwd == rev
        for _ in range(3):
            w = rb(k // 2)
            reads += [w + revcomp(w), rb(20) + w + revcomp(w) + rb(20)]
        reads += [b"AT" * (k // 2), b"CG" * (k // 2 + 3)]
    r = rb(40 if small else 100)                             # both strands of every window
    reads += [r, revcomp(r), r + revcomp(r)]
    for ends in (b"TA", b"GC", b"AT", b"CG", b"TT", b"GG", b"AA", b"CC"):
        # first base T / G: the top bits of fwd are set; last base A / C: those of rev are
        reads += [ends[:1] + rb(k - 2) + ends[1:], ends[:1] + rb(k + 5) + ends[1:]]
    length = 64 + k
    for positions in n_positions(k, length):
        s = bytearray(rb(length))
        for p in positions:
            s[p] = ord("N")
        reads.append(bytes(s))
    s = bytearray(rb((3 if small else 6) * k + 3))
    s[k - 1::k] = b"n" * len(s[k - 1::k])                    # no window is left
    reads.append(bytes(s))
    reads.append(rb(k + 2) + b"-" + rb(k) + b"\x00\xff" + rb(k + 1) + b"*")
    for n in rng.integers(k - 1, k + 31, 40 if small else 150).tolist():
        reads.append(rb(int(n)))
    return reads


def structured_quals(k, reads):
    """Quality lines that put a base below '+' at each of n_positions, read after read."""
    out = []
    for i, r in enumerate(reads):
        q = bytearray(b"I" * len(r))
        for p in n_positions(k, len(r))[i % 7]:
            if 0 <= p < len(r):
                q[p] = LOW_QUAL
        out.append(bytes(q))
    return out


def key_space_table(k, canonical, rng):
    """Every (canonical) key of a small k, a third of them left out, counts from EDGE_COUNTS (0 among them)."""
    table = {}
    for x in range(4 ** k):
        mer = bytes(b"ACGT"[(x >> (2 * (k - 1 - j))) & 3] for j in range(k))
        if canonical and sc.pack(revcomp(mer)) < x:
            continue
        if rng.random() >= 1 / 3:
            table[x] = int(EDGE_COUNTS[int(rng.integers(0, EDGE_COUNTS.size))])
    return table


@functools.lru_cache(maxsize=None)
def corpus_case(k, canonical):
    """reads, the table of the scan and select tests, and what the corpus shows -- asserted here, from the models alone."""
    reads = structured_reads(k)
    assert 200 <= len(reads) and sum(len(r) for r in reads) <= 21000
    pairs, skipped = [], 0
    for s in reads:
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if w.translate(None, BASES):
                skipped += 1
            else:
                pairs.append((sc.pack(w), sc.pack(revcomp(w))))
    looked = {min(f, r) if canonical else f for f, r in pairs}
    assert looked == {w[0] for s in reads for w in sc.windows(s, k, canonical) if w is not None}
    assert any(r < f for f, r in pairs) and any(f < r for f, r in pairs)
    assert k % 2 or any(f == r for f, r in pairs)
    if k == 32:                                              # where a signed compare picks the other strand
        assert any(f >= TOP_BIT > r for f, r in pairs) and any(r >= TOP_BIT > f for f, r in pairs)
    top = 4 ** k - 1
    assert 0 in looked and (canonical or top in looked)
    assert skipped >= 1
    rng = np.random.default_rng(7200 + 2 * k + canonical)
    if k <= 6:
        table = key_space_table(k, canonical, rng)
    else:
        table = sc.a_tenth_of_the_kmers(reads, k, canonical, rng)
        table[0] = 65536
        if top in looked:
            table[top] = U32
    assert any(table.get(key, 0) > 0 for key in looked) and any(key not in table for key in looked)
    return {"reads": reads, "table": table, "looked": looked, "n_windows": len(pairs), "n_skipped": skipped}


@functools.lru_cache(maxsize=None)
def scan_model(k, canonical):
    case = corpus_case(k, canonical)
    return (sc.model_cov(case["reads"], case["table"], k, canonical), sc.model_text(case["reads"], case["table"], k, canonical))


@functools.lru_cache(maxsize=None)
def count_model(k, canonical):
    return tc.model(b"\n".join(corpus_case(k, canonical)["reads"]), k, canonical)


@pytest.fixture(autouse=True)
def small_buffers(monkeypatch):
    """Staging buffers of 128 KiB: still one piece per call for the corpus, without the time the default 16 MiB ones
    take to allocate in every one of the many small calls here."""
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(1 << 17))


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", EVERY_K)
def test_the_corpus_shows_its_cases(k, canonical):
    """CPU: what every test below rests on, from the models alone (corpus_case asserts it)."""
    case = corpus_case(k, canonical)
    cov, text = scan_model(k, canonical)
    assert sum(c[1] for c in cov) == case["n_windows"] == text.count(b"\n") and sum(c[3] for c in cov) == case["n_skipped"]
    assert any(c[2] for c in cov) and any(c[1] > c[2] for c in cov)          # lines with count 0, and with more
    keys, counts = count_model(k, canonical)
    assert set(keys.tolist()) == case["looked"] and int(counts.sum()) == case["n_windows"]


# ------------------------------------------------------------------ (a) the counter
def fasta_text(reads, width=61):
    return b"".join(b">read %d\n" % i + b"".join(r[j:j + width] + b"\n" for j in range(0, len(r), width)) for i, r in enumerate(reads))


@gpu
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", EVERY_K)
def test_count_every_k(monkeypatch, k, canonical):
    reads = corpus_case(k, canonical)["reads"]
    want = count_model(k, canonical)
    data = b"\n".join(reads)
    n_bases = len(data.translate(None, bytes(set(range(256)) - set(BASES))))
    text = fasta_text(reads)
    cut = text.index(reads[12][122:183]) + 30                # inside the third line of the 2 049-base read
    assert len(reads[12]) == 2049 and text[cut - 30:cut + 30].count(b"\n") == 0
    n_all_t = sum(r[i:i + 32].upper() == b"T" * 32 for r in reads for i in range(len(r) - 31))
    for stage in (None, 4096):                               # one piece; pieces that overlap by k - 1 bytes
        if stage:
            monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))
        for how in ("bases", "text"):
            c = kmlib.Counter(k=k, canonical=canonical)
            try:
                if how == "bases":
                    c.add_bases(data)
                else:
                    used = c.add_text(text[:cut], final=False)
                    assert 0 < used <= cut
                    assert c.add_text(text[used:], final=True) == len(text) - used
                stats = c.stats()
                c.finish().close()
                got = tc.sorted_records(c)
            finally:
                c.close()
            ctx = (k, canonical, stage, how)
            assert tc.same(got, want), ctx
            assert stats["bases"] == n_bases and stats["kmers"] == int(want[1].sum(dtype=np.uint64)), ctx
            assert stats["distinct"] == want[0].size, ctx
            if k == 32 and not canonical:                    # T^32, counted beside the table
                assert n_all_t > 100 and int(got[0][-1]) == ALL_T and int(got[1][-1]) == n_all_t, ctx


def corpus_stream(k, canonical):
    """data, n_bases, n_all_t and the (text, cut) of the two add_text calls, as test_count_every_k feeds them."""
    reads = corpus_case(k, canonical)["reads"]
    data = b"\n".join(reads)
    n_bases = len(data.translate(None, bytes(set(range(256)) - set(BASES))))
    text = fasta_text(reads)
    cut = text.index(reads[12][122:183]) + 30
    assert len(reads[12]) == 2049 and text[cut - 30:cut + 30].count(b"\n") == 0
    n_all_t = sum(r[i:i + 32].upper() == b"T" * 32 for r in reads for i in range(len(r) - 31))
    return data, n_bases, text, cut, n_all_t


@gpu
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", EVERY_K)
def test_count_filtered_every_k(monkeypatch, k, canonical):
    """k_count_filtered, both tiers: the filter is the table's keys and one key the corpus does not hold."""
    case = corpus_case(k, canonical)
    data, n_bases, _, _, n_all_t = corpus_stream(k, canonical)
    model = dict(zip(*(a.tolist() for a in count_model(k, canonical))))
    keys = sorted(case["table"])
    assert all(canonical_key(key, k, canonical) == key for key in keys)
    stranger = next((x for x in range(min(4 ** k, 1 << 20)) if canonical_key(x, k, canonical) == x and x not in model), None)
    assert stranger is not None or k <= 5                    # (only a tiny key space is all in the corpus)
    if stranger is not None:
        keys.append(stranger)
    want = {key: model.get(key, 0) for key in keys}
    assert sum(want.values()) > 0 and (0 in want.values() or stranger is None) and set(want) != set(model)
    order = np.array(sorted(want), np.uint64)
    want_rec = (order, np.array([want[key] for key in order.tolist()], np.uint32))
    slots = 64
    while slots < 2 * len(want):
        slots <<= 1
    monkeypatch.setenv("KM_COUNT_FILTER_BLOCKS", "1")
    # pieces that overlap by k - 1 bytes, then one block that makes several trips over one piece; either in both tiers
    for stage, force_hbm in ((4096, False), (4096, True), (None, False), (None, True)):
        if stage:
            monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))
        else:
            monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(1 << 17))
            assert len(data) > 256 * 32                      # (a block of 256 lanes of 32 starts: two trips or three)
        if force_hbm:
            monkeypatch.setenv("KM_COUNT_FILTER_LDS", "0")
        else:
            monkeypatch.delenv("KM_COUNT_FILTER_LDS", raising=False)
        c = kmlib.Counter(k=k, canonical=canonical)
        try:
            c.set_filter(np.array(keys, np.uint64))
            c.add_bases(data)
            stats, fs = c.stats(), c.filter_stats()
            c.finish(0).close()
            got = tc.sorted_records(c)
        finally:
            c.close()
        ctx = (k, canonical, stage, force_hbm)
        assert tc.same(got, want_rec), ctx
        assert fs["tier"] == ("hbm" if force_hbm or slots > 2 * fs["lds_keys"] else "lds"), ctx
        assert fs["kmers_hit"] == sum(want.values()) and fs["n_keys"] == len(want) == stats["distinct"], ctx
        assert stats["bases"] == n_bases and stats["kmers"] == case["n_windows"], ctx
        if k == 32 and not canonical:                        # T^32: in the filter, counted beside the table
            assert n_all_t > 100 and want[ALL_T] == n_all_t and int(got[0][-1]) == ALL_T and int(got[1][-1]) == n_all_t, ctx


@gpu
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", EVERY_K)
def test_count_solid_every_k(monkeypatch, k, canonical):
    """k_sketch_note through add_bases, k_count_solid through two add_text calls cut mid-line."""
    case = corpus_case(k, canonical)
    data, n_bases, text, cut, n_all_t = corpus_stream(k, canonical)
    keys, counts = count_model(k, canonical)
    want = (keys[counts >= 2], counts[counts >= 2])
    assert 0 < want[0].size and (want[0].size < keys.size or k <= 5)
    noted = case["n_windows"] - (n_all_t if k == 32 and not canonical else 0)
    for stage in (None, 4096):                               # one piece; pieces that overlap by k - 1 bytes
        if stage:
            monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))
        c = kmlib.Counter(k=k, canonical=canonical)
        try:
            c.set_sketch(kmlib.sketch_words(int(keys.size)))
            c.add_bases(data)
            c.sketch_done()
            used = c.add_text(text[:cut], final=False)
            assert 0 < used <= cut
            assert c.add_text(text[used:], final=True) == len(text) - used
            stats, ss = c.stats(), c.sketch_stats()
            c.finish(2).close()
            got = tc.sorted_records(c)
        finally:
            c.close()
        ctx = (k, canonical, stage)
        assert tc.same(got, want), ctx
        assert ss["kmers_noted"] == noted and stats["kmers"] == case["n_windows"] and stats["bases"] == n_bases, ctx
        if k == 32 and not canonical:
            assert n_all_t > 100 and int(got[0][-1]) == ALL_T and int(got[1][-1]) == n_all_t, ctx


# ------------------------------------------------------------------ (b) the scan
@gpu
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", EVERY_K)
def test_scan_every_k(monkeypatch, k, canonical):
    case = corpus_case(k, canonical)
    reads, table = case["reads"], case["table"]
    model = scan_model(k, canonical)
    total = sum(len(r) for r in reads)
    db = ts.make_db(table, k, canonical)
    try:
        for stage in (1 << 17, 4096):                        # a piece or two; pieces that overlap by k - 1 bytes
            monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))
            _, _, st = ts.check(db, reads, table, k, canonical, (k, canonical, stage), model)
            assert st["pieces"] == -(-total // min(stage - (k - 1), stage // (k + 13))), stage     # (as tests/test_scan.py)
        assert st["pieces"] > 4
    finally:
        db.close()


# ------------------------------------------------------------------ (c) the selection
@gpu
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", EVERY_K)
def test_select_every_k(k, canonical):
    case = corpus_case(k, canonical)
    reads, table = case["reads"], case["table"]
    text = sm.fastq(reads)
    masked = sm.fastq(reads, quals=structured_quals(k, reads), last_newline=False)
    hits = sm.model_hits(text, table, k, canonical)
    assert hits != sm.model_hits(masked, table, k, canonical, LOW_QUAL + 1)  # the masked bases do change the hits
    assert min(hits) == 0 and max(hits) >= 2 and 1 in hits
    db = ts.make_db(table, k, canonical)
    try:
        tsel.check(db, text, table, k, canonical, min_hits=1, ctx=(k, canonical, 1))
        tsel.check(db, text, table, k, canonical, min_hits=2, ctx=(k, canonical, 2))
        tsel.check(db, text, table, k, canonical, min_hits=2, invert=True, ctx=(k, canonical, "-v"))
        tsel.check(db, masked, table, k, canonical, min_qual="+", ctx=(k, canonical, "-Q"))
    finally:
        db.close()


# ------------------------------------------------------------------ (d) the counter's quality mask
@gpu
@pytest.mark.parametrize("q", ["!", "+"])
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [2, 3, 4, 8, 16, 17, 30, 32])
def test_count_fastq_mask_every_k(k, canonical, q):
    reads = corpus_case(k, canonical)["reads"]
    text = sm.fastq(reads, quals=structured_quals(k, reads))
    want = tq.model_fastq(text, ord(q), k, canonical)
    if q == "!":
        assert tc.same(want, count_model(k, canonical))      # nothing is below '!'
    else:
        assert int(want[1].sum()) < int(count_model(k, canonical)[1].sum())
    c = kmlib.Counter(k=k, canonical=canonical)
    try:
        assert c.add_fastq(text, final=True, min_qual_char=q) == len(text)
        stats = c.stats()
        c.finish().close()
        got = tq.sorted_records(c)
    finally:
        c.close()
    assert tq.same(got, want)
    assert stats["kmers"] == int(want[1].sum(dtype=np.uint64)) and stats["distinct"] == want[0].size


# ------------------------------------------------------------------ (e) the pairs
@functools.lru_cache(maxsize=None)
def pair_case(k, small=False):
    """Mate 1: the corpus; mate 2: the reverse complement of mate 1 for every other pair, random bases for the rest."""
    rng = np.random.default_rng(7300 + k)
    mate1 = structured_reads(k, small)
    mate2 = [revcomp(r) if i % 2 == 0 else sc.random_bases(rng, len(r)) for i, r in enumerate(mate1)]
    names = [b"pair%d" % i for i in range(len(mate1))]
    return (sm.fastq(mate1, names=[n + b"/1" for n in names]), sm.fastq(mate2, names=[n + b"/2" for n in names], last_newline=False))


@gpu
@pytest.mark.parametrize("rule", ["sum", "both"])
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [2, 4, 16, 17, 30, 32])
def test_pair_select_every_k(k, canonical, rule):
    table = corpus_case(k, canonical)["table"]
    text1, text2 = pair_case(k)
    h1, h2 = sm.model_hits(text1, table, k, canonical), sm.model_hits(text2, table, k, canonical)
    if canonical:                                            # a read and its reverse complement hold the same k-mers
        assert h1[0::2] == h2[0::2] and max(h1[0::2]) > 2
    else:
        assert h1[0::2] != h2[0::2]
    min_hits = 3 if rule == "sum" else 2
    want = pm.model_pair_select(text1, text2, table, k, canonical, min_hits=min_hits, rule=rule)
    kept = pm.kept_pairs(text1, text2, table, k, canonical, min_hits=min_hits, rule=rule)
    assert 0 < len(kept) < len(h1)
    db = ts.make_db(table, k, canonical)
    try:
        out1, out2, stats, consumed = tpair.pair_select(db, text1, text2, rule=rule, min_hits=min_hits)
    finally:
        db.close()
    assert (out1, out2) == want
    assert consumed == (len(text1), len(text2))
    assert (stats["pairs_in"], stats["pairs_out"]) == (len(h1), len(kept))
    assert stats["bytes_out"] == [len(want[0]), len(want[1])]


# ------------------------------------------------------------------ (f) counted, then scanned
@gpu
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [2, 16, 17, 32])
def test_count_then_scan_round_trip(k, canonical):
    reads = corpus_case(k, canonical)["reads"]
    keys, counts = count_model(k, canonical)
    table = dict(zip(keys.tolist(), counts.tolist()))
    want = (sc.model_cov(reads, table, k, canonical), sc.model_text(reads, table, k, canonical))
    assert all(c[2] == 0 for c in want[0])                   # every valid window is found
    assert sum(c[0] for c in want[0]) == sum(c * c for c in counts.tolist())
    c = kmlib.Counter(k=k, canonical=canonical)
    db = None
    try:
        c.add_bases(b"\n".join(reads))
        db = c.finish()
        _, text, _ = ts.check(db, reads, table, k, canonical, (k, canonical), want)
        if k == 32 and not canonical:                        # T^32: from the counter's own cell into the table and out
            assert b"T" * 32 + b" %d\n" % table[ALL_T] in text
    finally:
        if db is not None:
            db.close()
        c.close()


# ------------------------------------------------------------------ (g) one key, many waves
@gpu
@pytest.mark.parametrize("base", [b"A", b"T"])
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [2, 32])
def test_one_key_under_contention(monkeypatch, k, canonical, base):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(1 << 20))
    read = base * 200_000
    n = len(read) - k + 1
    key = 0 if base == b"A" or canonical else 4 ** k - 1     # (at k = 32 the second is T^32, the counter's empty mark)
    c = kmlib.Counter(k=k, canonical=canonical)
    db = None
    try:
        c.add_bases(read)
        stats = c.stats()
        db = c.finish()
        got = c.records()
        assert (got[0].tolist(), got[1].tolist()) == ([key], [n])
        assert (stats["bases"], stats["kmers"], stats["distinct"]) == (len(read), n, 1)
        assert ts.cells(db.cov_seqs([read])) == [(n * n, n, 0, 0, 0, n, n)]
        assert db.fastq_hits(sm.fastq([read])).tolist() == [n]
        assert db.fastq_hits(sm.fastq([revcomp(read)])).tolist() == [n if canonical else 0]
    finally:
        if db is not None:
            db.close()
        c.close()
