"""Solid k-mers in two passes on the GPU (km_counter_set_sketch, Counter.set_sketch, count_files(solid=),
`count --solid`).

Every comparison is exact.  The counts come from test_count.model (numpy, from the definition); what the sketch may and
must admit from test_count_solid_cpu.solid_model (plain Python, written from the rule, checked there against the rule
played sequentially); the plain counter on the same GPU is a second reference."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import test_count as tc
import test_count_quality as tq
from km_amd import cli
from km_amd import count as kc
from km_amd import lib as kmlib
from test_count_solid_cpu import (ALLT, CASES, TABLE_EXPECTED, as_fasta, as_stream, distinct_canonical_mers, mers_of,
                                  solid_model, solid_reads, table_text)

pytestmark = pytest.mark.gpu

E_FORMAT, E_ARG, E_STATE = 2, 4, 7
ACGT = np.frombuffer(b"ACGT", np.uint8)


def records_dict(counter):
    keys, counts = counter.records()
    out = dict(zip(keys.tolist(), counts.tolist()))
    assert len(out) == keys.size                            # (no key twice)
    return out


def as_dict(model):
    return dict(zip(model[0].tolist(), model[1].tolist()))


def solid(words, first, second, lower, k=31, canonical=True, **kw):
    """One counter with a sketch: first(counter), sketch_done, second(counter), finish(lower)
    -> (records dict, stats, sketch_stats)."""
    c = kmlib.Counter(k=k, canonical=canonical, **kw)
    try:
        c.set_sketch(words)
        first(c)
        c.sketch_done()
        second(c)
        stats, ss = c.stats(), c.sketch_stats()
        c.finish(lower).close()
        return records_dict(c), stats, ss
    finally:
        c.close()


def plain(data, lower, k=31, canonical=True, **kw):
    got, stats, db = tc.count_bases(data, k, canonical, lower=lower, **kw)
    db.close()
    return as_dict(got), stats


def bases(data):
    return lambda c: c.add_bases(data)


def in_three_add_text_calls(text):
    """The FASTA text in three calls cut in the middle of a sequence line, the unconsumed tail carried along."""
    def mid_line(at):                                       # 20 bases either side (a header line is shorter than that)
        while b"\n" in text[at - 20:at + 20]:
            at += 1
        return at
    cuts = [mid_line(len(text) // 3), mid_line(2 * len(text) // 3), len(text)]
    assert 40 < cuts[0] < cuts[1] - 40 < len(text) - 80

    def feed(c):
        pos, tail = 0, b""
        for cut in cuts:
            buf = tail + text[pos:cut]
            pos = cut
            used = c.add_text(buf, final=False)
            assert used < len(buf) or cut == len(text)
            tail = buf[used:]
        c.add_text(tail, final=True)
    return feed


# ------------------------------------------------------------------ 1: exactness
@pytest.mark.parametrize("k,canonical", CASES)
def test_records_after_the_cut_equal_the_plain_count(monkeypatch, k, canonical):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "2048")      # several pieces per pass, windows across every cut
    reads = solid_reads(100 + 2 * k + canonical)
    data, fasta = as_stream(reads), as_fasta(reads)
    words = kmlib.sketch_words(2000)
    brute, S, upper, bounds = solid_model(data, k, canonical, words)
    assert S and S <= upper and (k < 31 or len(S) < len(brute))
    plain_stats = plain(data, 1, k, canonical)[1]
    for lower in (2, 3):
        want = {key: n for key, n in brute.items() if n >= lower}
        assert want
        rec, stats, ss = solid(words, bases(data), in_three_add_text_calls(fasta), lower, k, canonical)
        assert rec == want
        assert (stats["bases"], stats["kmers"]) == (plain_stats["bases"], plain_stats["kmers"])
        assert len(S) <= stats["distinct"] <= len(upper)
        assert ss["words"] == words and ss["bits_1"] == bounds["bits_1"]
        assert ss["kmers_noted"] == sum(n for key, n in brute.items() if key != ALLT)
        assert bounds["kmers_admitted"][0] <= ss["kmers_admitted"] <= bounds["kmers_admitted"][1]
        assert bounds["bits_2"][0] <= ss["bits_2"] <= bounds["bits_2"][1]
    assert plain(data, 2, k, canonical)[0] == {key: n for key, n in brute.items() if n >= 2}


# ------------------------------------------------------------------ 2: no false negatives under contention
def _primitive_units(rng, n):
    """n 8-mers such that no window of one's periodic text is a window of another's, on either strand, and none is
    periodic with a shorter period."""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seen, units = set(), []
    while len(units) < n:
        u = ACGT[rng.integers(0, 4, 8)].tobytes()
        rc = u.translate(comp)[::-1]
        rotations = {(u + u)[i:i + 8] for i in range(8)}
        if len(rotations) < 8 or rc in rotations:
            continue
        cls = min(rotations | {(rc + rc)[i:i + 8] for i in range(8)})
        if cls not in seen:
            seen.add(cls)
            units.append(u)
    return units


def contention_text():
    """10 000 distinct 31-mers, each exactly twice, 2 500 at each of four distances -> (text, planted keys, stage).
    A  both copies start in one lane's 32 starts: 39 bases of period 8 at the head of a 64-byte row (starts 0 and 8; the
       seven windows between them occur once)
    B  in neighbouring lanes: starts 0 and 32 of a 64-byte row
    C  in different blocks: 80 000 bytes apart
    D  in different staging pieces: 80 000 bytes apart with a piece's first own byte, 560 000, between them."""
    rng = np.random.default_rng(31)
    n = 2500
    rows_a = np.full((n, 64), ord("N"), np.uint8)
    for i, u in enumerate(_primitive_units(rng, n)):
        rows_a[i, :39] = np.frombuffer((u * 5)[:39], np.uint8)
    keys = distinct_canonical_mers(rng, 3 * n)
    keys = keys[rng.permutation(keys.size)]
    mers = mers_of(keys)
    rows_b = np.full((n, 64), ord("N"), np.uint8)
    rows_b[:, :31] = rows_b[:, 32:63] = mers[:n]
    once = np.full((2 * n, 32), ord("N"), np.uint8)
    once[:, :31] = mers[n:]
    text = b"".join([rows_a.tobytes(), rows_b.tobytes(), once[:n].tobytes(), once[:n].tobytes(), once[n:].tobytes(),
                     once[n:].tobytes()])
    assert len(text) == 640_000
    planted_a = [int(tc.model(rows_a[i, :31].tobytes(), 31, True)[0][0]) for i in range(n)]
    return text, planted_a + keys.tolist(), 280_000 + 30


def test_every_key_seen_twice_survives_a_saturated_sketch(monkeypatch):
    text, planted, stage = contention_text()
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))  # piece i owns the bytes from 280 000 i
    brute, S, upper, bounds = solid_model(text, 31, True, 64)
    assert len(set(planted)) == 10_000 and all(brute[key] == 2 for key in planted) and S == set(planted)
    assert len(brute) == 10_000 + 7 * 2500                  # (the singletons between the two starts of an A row)
    assert bounds["bits_2"][0] == 64 * 32                   # plane 2 is full whatever the order: every key is admitted
    assert upper == set(brute)
    want = {key: 2 for key in planted}
    assert plain(text, 2)[0] == want
    rec, stats, ss = solid(64, bases(text), bases(text), 2)
    assert rec == want
    assert stats["distinct"] == len(brute)
    assert ss["bits_1"] == ss["bits_2"] == 64 * 32 and ss["kmers_noted"] == ss["kmers_admitted"] == stats["kmers"]


# ------------------------------------------------------------------ 3: the table really is smaller
def test_the_table_holds_the_solid_keys_and_few_others(monkeypatch):
    # (a table has room for every window of the piece to come: small pieces, so that the keys set its size)
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "1024")
    data = table_text()
    words = kmlib.sketch_words(TABLE_EXPECTED)
    brute, S, upper, bounds = solid_model(data, 31, True, words)
    singletons = [key for key, n in brute.items() if n == 1]
    assert len(upper) - len(S) <= len(singletons) / 4       # (the precondition; test_count_solid_cpu checks it too)
    rec, stats, ss = solid(words, bases(data), bases(data), 0, expected_distinct=1)
    A = set(rec)
    assert S <= A <= upper
    assert all(rec[key] == brute[key] for key in A)
    assert stats["distinct"] == len(A) and len(A) - len(S) <= len(singletons) / 4
    assert ss["bits_1"] == bounds["bits_1"]
    assert bounds["bits_2"][0] <= ss["bits_2"] <= bounds["bits_2"][1]
    assert bounds["kmers_admitted"][0] <= ss["kmers_admitted"] <= bounds["kmers_admitted"][1]
    assert ss["kmers_admitted"] == sum(rec.values()) and ss["kmers_noted"] == stats["kmers"] == sum(brute.values())
    everything, plain_stats = plain(data, 0, expected_distinct=1)
    assert everything == brute and plain_stats["distinct"] == len(brute)
    assert stats["slots"] * 4 <= plain_stats["slots"] and stats["n_grow"] < plain_stats["n_grow"]


# ------------------------------------------------------------------ 4: the all-T k-mer of a non-canonical k = 32 counter
@pytest.mark.parametrize("times", [1, 2])
def test_all_t_kmer_is_cut_as_for_a_plain_counter(times):
    data = b"ACG" + b"T" * (31 + times) + b"\n" + b"A" * 34 + b"\nGATTACA" * 3
    brute = as_dict(tc.model(data, 32, False))
    assert brute[ALLT] == times and brute[0] == 3
    want = {key: n for key, n in brute.items() if n >= 2}
    assert (ALLT in want) == (times == 2)
    assert plain(data, 2, 32, False)[0] == want
    rec, stats, ss = solid(64, bases(data), bases(data), 2, 32, False)
    assert rec == want
    assert stats["kmers"] == sum(brute.values()) and ss["kmers_noted"] == stats["kmers"] - times
    # a canonical counter stores T^32 as A^32, which has a slot and a sketch entry like any key
    rec, _, _ = solid(64, bases(data), bases(data), 2, 32, True)
    assert rec == {key: n for key, n in as_dict(tc.model(data, 32, True)).items() if n >= 2} and rec[0] == 3 + times


# ------------------------------------------------------------------ 5: growth in pass 2
def test_the_table_grows_in_the_second_pass(monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")      # (room is made piece by piece: the table grows on the way)
    rng = np.random.default_rng(51)
    seq = tc.random_bases(rng, 40_030).tobytes()
    data = seq + b"\n" + seq
    want = as_dict(tc.model(data, 31, True))
    assert len(want) > 39_000 and set(want.values()) == {2}
    rec, stats, ss = solid(kmlib.sketch_words(40_000), bases(data), bases(data), 2)
    assert stats["n_grow"] >= 1 and stats["slots"] == 1 << 17 and stats["distinct"] == len(want)
    assert rec == want


# ------------------------------------------------------------------ 6: add_fastq with -Q
def test_fastq_with_quality_masking(monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "65536")     # several pieces per pass
    reads = tc.make_reads(61, 1500)
    text = tc.as_fastq(reads, np.random.default_rng(62))
    half = kmlib.fastq_cut(text[:len(text) // 2])

    def whole(q):
        return lambda c: c.add_fastq(text, final=True, min_qual_char=q)

    def halves(q):
        def feed(c):
            assert c.add_fastq(text[:half], final=False, min_qual_char=q) == half
            c.add_fastq(text[half:], final=True, min_qual_char=q)
        return feed

    want = {}
    for q in (">", 0):
        ref = kmlib.Counter(k=31)
        ref.add_fastq(text, final=True, min_qual_char=q)
        ref.finish(2).close()
        want[q] = records_dict(ref)
        ref.close()
        rec, stats, ss = solid(kmlib.sketch_words(100_000), whole(q), halves(q), 2)
        assert rec == want[q] and want[q]
    assert want[">"] != want[0]


def test_a_malformed_record_fails_in_the_first_pass(monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")
    text = tq.faulty_text("short quality")
    where = tq.model_first_fault(text)
    c = kmlib.Counter(k=31)
    try:
        c.set_sketch(1024)
        c.add_fastq(text, final=True, min_qual_char="+")
        with pytest.raises(kmlib.KmError) as e:
            c.sketch_done()
        assert e.value.code == E_FORMAT and ("offset %d" % where) in str(e.value), str(e.value)
        for call in (c.sketch_done, c.stats, c.sketch_stats, lambda: c.add_bases(b"ACGT")):
            with pytest.raises(kmlib.KmError) as e:
                call()
            assert e.value.code == E_FORMAT
    finally:
        c.close()


# ------------------------------------------------------------------ 7: state
def _refused(code, call):
    with pytest.raises(kmlib.KmError) as e:
        call()
    assert e.value.code == code, e.value


def test_state_and_argument_errors_leave_the_counter_usable(tmp_path):
    data = b"ACGTACGTTGCATGCAACGT"
    keys = tc.model(data, 5, False)[0]
    ones = np.ones(3, np.uint32)
    jf = str(tmp_path / "k5.jf")
    kc.write_records(jf, keys, np.ones(keys.size, np.uint32), 5, False)
    # a counter that has been fed, or has a filter, refuses a sketch and goes on as it was
    c = kmlib.Counter(k=5, canonical=False)
    _refused(E_STATE, c.sketch_done)
    c.add_bases(data)
    _refused(E_STATE, lambda: c.set_sketch(64))
    _refused(E_STATE, c.sketch_done)
    assert c.sketch_stats()["words"] == 0
    c.finish().close()
    assert tc.same(tc.sorted_records(c), tc.model(data, 5, False))
    c.close()
    c = kmlib.Counter(k=5, canonical=False)
    c.set_filter(keys[:3])
    _refused(E_STATE, lambda: c.set_sketch(64))
    c.close()
    # sizes that are no power of two from 64 to 2^40: refused, and the counter still takes a sketch
    c = kmlib.Counter(k=5, canonical=False)
    for words in (0, 1, 32, 65, 96, (1 << 40) + 1, 1 << 41):
        _refused(E_ARG, lambda: c.set_sketch(words))
    c.set_sketch(64)
    # a second sketch, a filter, records of any kind
    for call in (lambda: c.set_sketch(64), lambda: c.set_filter(keys[:3]), lambda: c.add_records(keys[:3], ones),
                 lambda: c.add_jf(jf), lambda: c.set_records(keys[:3], ones), lambda: c.set_jf(jf)):
        _refused(E_STATE, call)
    c.add_bases(data + b"\n" + data)
    # nothing reads the table before the first pass has ended
    with open(tmp_path / "no.txt", "wb") as text_out:
        for call in (lambda: c.finish(2), lambda: c.finish(2, 9), c.records, c.histo, lambda: c.dump(text_out),
                     lambda: c.write_jf(str(tmp_path / "no.jf"))):
            _refused(E_STATE, call)
    assert not os.path.exists(tmp_path / "no.jf") and os.path.getsize(tmp_path / "no.txt") == 0
    _refused(E_STATE, lambda: c.add_records(keys[:3], ones))
    assert c.stats()["kmers"] == 0 and c.sketch_stats()["kmers_noted"] == 2 * (len(data) - 4)
    c.sketch_done()
    for call in (c.sketch_done, lambda: c.set_sketch(64), lambda: c.set_filter(keys[:3]),
                 lambda: c.add_records(keys[:3], ones)):
        _refused(E_STATE, call)
    c.add_bases(data + b"\n" + data)
    c.finish(2).close()
    assert records_dict(c) == {key: 2 * n for key, n in as_dict(tc.model(data, 5, False)).items()}
    _refused(E_STATE, c.sketch_done)
    c.close()


def test_other_text_in_the_second_pass_is_counted_for_the_admitted_keys():
    rng = np.random.default_rng(71)
    first = tc.random_bases(rng, 600).tobytes()
    second = first[100:400] + b"\n" + tc.random_bases(rng, 300).tobytes()
    words = 1 << 16                                        # roomy: nothing but the keys seen twice is admitted
    seen = first + b"\n" + first
    brute, S, upper, _ = solid_model(seen, 31, True, words)
    assert upper == S == set(brute)
    rec, _, _ = solid(words, bases(seen), bases(second), 0)
    assert rec == {key: n for key, n in as_dict(tc.model(second, 31, True)).items() if key in S} and len(rec) == 270


# ------------------------------------------------------------------ 8: the command line
def _count(argv):
    err = io.StringIO()
    parser = cli.build_parser()
    args = cli.parse_args(["count"] + argv, parser)
    del args._cmd
    cli.main_count(args, err=err)
    return dict(line[1:].split(":") for line in err.getvalue().splitlines() if line.startswith("#"))


def _dump(path):
    with open(path + ".txt", "wb") as out:
        kc.dump_file(path, out=out, fmt="column")
    with open(path + ".txt", "rb") as fh:
        return fh.read()


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_command_line(tmp_path, monkeypatch):
    import gzip
    from oracle import jf_reader as jr
    monkeypatch.chdir(tmp_path)
    reads = tc.make_reads(81, 3000)
    with gzip.open("r.fq.gz", "wb") as fh:
        fh.write(tc.as_fastq(reads, np.random.default_rng(82)))
    full = as_dict(tc.model(b"\n".join(reads), 31, True))
    want = {key: n for key, n in full.items() if n >= 2}
    n = str(len(full))

    lines = _count(["--solid", n, "-m", "31", "-C", "-o", "a.jf", "--histo", "a.histo", "--dump", "a.dump", "r.fq.gz"])
    plain_lines = _count(["-L", "2", "-m", "31", "-C", "-o", "b.jf", "--histo", "b.histo", "--dump", "b.dump", "r.fq.gz"])
    text = _dump("a.jf")
    assert text == _dump("b.jf") and len(text.splitlines()) == len(want)
    assert _read("a.histo") == _read("b.histo") and _read("a.dump") == _read("b.dump") == text
    rec = jr.read_jf("a.jf")
    assert dict(zip(rec["keys"].tolist(), rec["counts"].tolist())) == want
    cmdline = rec["header"]["cmdline"]
    assert cmdline[cmdline.index("--solid") + 1] == n and cmdline[cmdline.index("-L") + 1] == "2"
    assert "--solid" not in jr.read_jf("b.jf")["header"]["cmdline"]
    assert lines["lower_count"] == "2" and int(lines["sketch_words"]) == kmlib.sketch_words(len(full))
    assert (lines["bases"], lines["kmers"]) == (plain_lines["bases"], plain_lines["kmers"])
    assert len(want) <= int(lines["distinct"]) < int(plain_lines["distinct"]) == len(full)
    assert 0 < int(lines["sketch_bits_2"]) < int(lines["sketch_bits_1"])
    assert sum(want.values()) <= int(lines["kmers_admitted"]) < int(lines["kmers"])
    assert not {"lower_count", "sketch_words", "kmers_admitted"} & set(plain_lines)

    _count(["--solid", n, "-m", "31", "-C", "--jellyfish-order", "-o", "aj.jf", "r.fq.gz"])
    _count(["-L", "2", "-m", "31", "-C", "--jellyfish-order", "-o", "bj.jf", "r.fq.gz"])
    assert _dump("aj.jf") == _dump("bj.jf") and sorted(_dump("aj.jf").splitlines()) == sorted(text.splitlines())

    assert _count(["-L", "1", "--solid", n, "-m", "31", "-C", "-o", "c.jf", "r.fq.gz"])["lower_count"] == "2"
    assert _dump("c.jf") == text
    assert _count(["-L", "5", "--solid", n, "-m", "31", "-C", "-o", "d.jf", "r.fq.gz"])["lower_count"] == "5"
    _count(["-L", "5", "-m", "31", "-C", "-o", "e.jf", "r.fq.gz"])
    assert _dump("d.jf") == _dump("e.jf") and 0 < len(_dump("d.jf").splitlines()) < len(want)

    _count(["--solid", n, "-Q", ">", "-s", "1000", "-m", "31", "-C", "-o", "q.jf", "r.fq.gz"])
    _count(["-L", "2", "-Q", ">", "-m", "31", "-C", "-o", "p.jf", "r.fq.gz"])
    assert _dump("q.jf") == _dump("p.jf") != text

    env = dict(os.environ, PYTHONPATH=tc.ROOT, KM_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, "-m", "km_amd", "count", "--solid", n, "-m", "31", "-C", "-o", "s.jf", "r.fq.gz"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "#lower_count:2" in res.stderr and "#kmers_admitted:" in res.stderr, res.stderr
    assert _dump("s.jf") == text
