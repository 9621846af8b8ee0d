"""Filtered counting on the GPU (km_counter_set_filter, Counter.set_filter, count_files(only=), `count --if`).

Every comparison is exact and covers the full record set.  The oracle for counts is test_count_filter_cpu.filtered_model
(plain Python, written from the definition, checked there against brute force); the unfiltered counter on the same GPU
is a second one."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import test_count as tc
from km_amd import cli
from km_amd import count as kc
from km_amd import lib as kmlib
from oracle import jf_reader as jr
from test_count_filter_cpu import canonical_key, filtered_model, revcomp_key

pytestmark = pytest.mark.gpu

ROOT = tc.ROOT
E_ARG, E_STATE = 4, 7
ALLT = (1 << 64) - 1
ACGT = np.frombuffer(b"ACGT", np.uint8)
CASES = [(2, False), (5, True), (5, False), (31, True), (32, True), (32, False)]


def records_dict(counter):
    keys, counts = counter.records()
    out = dict(zip(keys.tolist(), counts.tolist()))
    assert len(out) == keys.size                            # (no key twice)
    return out


def filtered(data, k, canonical, keys, lower=0, feed=None):
    """One filtered counter over `data` -> (records dict, stats, filter_stats, Database)."""
    c = kmlib.Counter(k=k, canonical=canonical)
    c.set_filter(np.array(keys, np.uint64))
    (feed or (lambda counter: counter.add_bases(data)))(c)
    stats, fs = c.stats(), c.filter_stats()
    db = c.finish(lower)
    rec = records_dict(c)
    c.close()
    return rec, stats, fs, db


def noisy_text(rng, n):
    """Random bases, some lower case, with Ns and newlines."""
    t = np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, n)].copy()
    t[rng.integers(0, n, n // 60)] = ord("N")
    t[rng.integers(0, n, n // 80)] = ord("\n")
    return t.tobytes()


def mers_text(keys, k):
    """Every key planted once, an N behind each."""
    keys = np.asarray(keys, np.uint64)
    shifts = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    rows = np.full((keys.size, k + 1), ord("N"), np.uint8)
    rows[:, :k] = ACGT[((keys[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)]
    return rows.tobytes()


def slots_for(distinct):
    s = 64
    while s < 2 * distinct:
        s <<= 1
    return s


# ------------------------------------------------------------------ 1: the model, every representation
@pytest.mark.parametrize("k,canonical", CASES)
def test_records_equal_the_model(k, canonical):
    rng = np.random.default_rng(100 + 2 * k + canonical)
    data = noisy_text(rng, 3000)
    present = tc.model(data, k, canonical)[0].tolist()
    assert present
    chosen = present[::2]
    space, occurs = 4 ** k, set(present)
    absent = set()
    for key in rng.integers(0, min(space, 1 << 63), 4 * len(chosen) + 64).tolist():
        if canonical_key(key, k, canonical) not in occurs and len(absent) < len(chosen):
            absent.add(canonical_key(key, k, canonical))
    keys = chosen + sorted(absent) + chosen[:7] + chosen[:3]
    if canonical:                                           # some by the other strand
        keys = [revcomp_key(key, k) if i % 3 == 0 else key for i, key in enumerate(keys)]
    keys = [keys[i] for i in rng.permutation(len(keys))]
    want = filtered_model(data, k, canonical, keys)
    assert sum(want.values()) > 0 and (len(absent) == 0 or 0 in want.values())

    rec, stats, fs, db = filtered(data, k, canonical, keys, lower=0)
    assert rec == want
    assert fs["kmers_hit"] == sum(want.values()) and fs["n_keys"] == len(want) == stats["distinct"]
    assert stats["slots"] == slots_for(len(want)) and stats["n_grow"] == 0 and fs["tier"] == "lds"
    order = sorted(want)
    assert db.info.n_records == len(want)
    assert db.query(np.array(order, np.uint64)).tolist() == [want[key] for key in order]
    db.close()

    plain = kmlib.Counter(k=k, canonical=canonical)
    plain.add_bases(data)
    st = plain.stats()
    plain.close()
    assert (stats["bases"], stats["kmers"]) == (st["bases"], st["kmers"])

    rec, _, _, db = filtered(data, k, canonical, keys, lower=1)
    assert rec == {key: n for key, n in want.items() if n}
    db.close()


# ------------------------------------------------------------------ 2: the all-T k-mer of a non-canonical k = 32 counter
def test_all_t_kmer_in_and_out_of_the_filter():
    with_t = b"T" * 40 + b"\nACGT" + b"T" * 32 + b"\n" + b"A" * 33
    without = b"A" * 33 + b"\nGGGT" + b"T" * 30 + b"\n"
    acgt_t = int(tc.model(b"ACGT" + b"T" * 28, 32, False)[0][0])
    # in the filter and in the text
    keys = [ALLT, 0, acgt_t]
    want = filtered_model(with_t, 32, False, keys)
    assert want[ALLT] == 9 + 2 and want[0] == 2             # (T^40; TT^32 behind ACG; A^33)
    rec, stats, fs, db = filtered(with_t, 32, False, keys)
    assert rec == want and fs["kmers_hit"] == sum(want.values()) and stats["distinct"] == 3
    assert db.query(np.array(keys, np.uint64)).tolist() == [want[key] for key in keys]
    db.close()
    # in the filter, not in the text: listed with 0 at lower_count 0, not listed at 1, and the database answers 0
    want = filtered_model(without, 32, False, keys)
    assert want == {ALLT: 0, 0: 2, acgt_t: 0}
    rec, stats, fs, db = filtered(without, 32, False, keys)
    assert rec == want and stats["distinct"] == 3 and fs["kmers_hit"] == 2
    assert db.query(np.array(keys, np.uint64)).tolist() == [0, 2, 0]
    db.close()
    rec, _, _, db = filtered(without, 32, False, keys, lower=1)
    assert rec == {0: 2}
    db.close()
    # not in the filter: its windows are seen and not counted
    rec, stats, fs, db = filtered(with_t, 32, False, [0, acgt_t])
    assert rec == {0: 2, acgt_t: 1} and fs["kmers_hit"] == 3 and stats["distinct"] == 2
    assert stats["kmers"] == int(tc.model(with_t, 32, False)[1].sum())
    db.close()
    # a canonical counter stores T^32 as A^32
    rec, _, _, db = filtered(with_t, 32, True, [ALLT])
    assert rec == filtered_model(with_t, 32, True, [ALLT]) == {0: 13}
    db.close()


# ------------------------------------------------------------------ 3: every key of k = 5
@pytest.mark.parametrize("canonical", [False, True])
def test_every_key_of_k5_fills_the_table_to_its_limit(canonical):
    rng = np.random.default_rng(7)
    data = noisy_text(rng, 20_000)
    keys = np.arange(1024, dtype=np.uint64)
    distinct = 512 if canonical else 1024
    rec, stats, fs, db = filtered(data, 5, canonical, keys, lower=1)
    db.close()
    assert stats["distinct"] == fs["n_keys"] == distinct and stats["slots"] == 2 * distinct and stats["n_grow"] == 0
    plain, st, db = tc.count_bases(data, 5, canonical)
    db.close()
    assert rec == dict(zip(plain[0].tolist(), plain[1].tolist()))
    assert (stats["bases"], stats["kmers"]) == (st["bases"], st["kmers"]) and fs["kmers_hit"] == st["kmers"]


# ------------------------------------------------------------------ 4: seams of a lane and of the text
@pytest.mark.parametrize("k", [31, 2])
def test_every_offset_in_a_lane_and_past_the_end_of_the_text(k):
    rng = np.random.default_rng(9)
    mer = b"GA" if k == 2 else ACGT[rng.integers(0, 4, k)].tobytes()
    key = int(tc.model(mer, k, False)[0][0])
    n = 2 * 32 + 9
    c = kmlib.Counter(k=k, canonical=False)
    c.set_filter(np.array([key], np.uint64))
    buf = bytearray(n)
    total = 0
    for off in range(2 * 32 + k + 1):
        buf[:] = b"N" * n
        piece = mer[:max(0, n - off)]
        buf[off:off + len(piece)] = piece
        assert len(buf) == n
        c.add_bases(bytes(buf))
        total += 1 if off + k <= n else 0
        assert filtered_model(bytes(buf), k, False, [key])[key] == (1 if off + k <= n else 0)
        assert c.filter_stats()["kmers_hit"] == total, off
    c.finish(0).close()
    assert records_dict(c) == {key: total}
    c.close()


@pytest.mark.parametrize("k", [31, 2])
def test_a_kmer_across_two_add_text_calls_counts_once(k):
    rng = np.random.default_rng(10)
    mer = b"GA" if k == 2 else ACGT[rng.integers(0, 4, k)].tobytes()
    key = int(tc.model(mer, k, False)[0][0])
    c = kmlib.Counter(k=k, canonical=False)
    c.set_filter(np.array([key], np.uint64))
    total = 0
    for split in range(1, k):
        first = b">r%d\nNN" % split + mer[:split] + b"\n"
        assert c.add_text(first, final=False) == len(first)
        assert c.filter_stats()["kmers_hit"] == total        # (enqueues what is staged: the rest arrives in a new piece)
        second = mer[split:] + b"NN\n"
        assert c.add_text(second, final=True) == len(second)
        total += 1
        assert c.filter_stats()["kmers_hit"] == total, split
    assert c.stats()["kmers"] == total
    c.finish(0).close()
    assert records_dict(c) == {key: total}
    c.close()


# ------------------------------------------------------------------ 5: the edge between the tiers
def _edge_keys(n):
    rng = np.random.default_rng(11)
    keys = np.unique(jr.canonical_np(rng.integers(0, 1 << 62, 2 * n + 64, dtype=np.uint64), 31))
    keys = keys[rng.permutation(keys.size)][:n]
    assert keys.size == n
    return keys


def test_tier_edge(monkeypatch):
    probe = kmlib.Counter(k=31)
    lds_keys = probe.filter_stats()["lds_keys"]
    assert probe.filter_stats()["tier"] == "none"
    probe.close()
    assert lds_keys == 4096
    all_keys = _edge_keys(lds_keys + 1)
    for n, tier in ((lds_keys - 1, "lds"), (lds_keys, "lds"), (lds_keys + 1, "hbm")):
        keys = all_keys[:n]
        data = mers_text(keys, 31)
        # the filter: every second key as planted, the rest by the other strand, and as many again that are absent
        given = np.where(np.arange(n) % 2 == 0, keys, jr.revcomp_np(keys, 31))
        want = filtered_model(data, 31, True, given.tolist())
        assert len(want) == n and set(want.values()) == {1}
        rec, stats, fs, db = filtered(data, 31, True, given)
        db.close()
        assert fs["tier"] == tier and fs["n_keys"] == n and stats["slots"] == slots_for(n)
        assert rec == want
        if n == lds_keys:
            monkeypatch.setenv("KM_COUNT_FILTER_LDS", "0")
            rec2, stats2, fs2, db = filtered(data, 31, True, given)
            db.close()
            monkeypatch.delenv("KM_COUNT_FILTER_LDS")
            assert fs2["tier"] == "hbm" and rec2 == rec and stats2 == stats


# ------------------------------------------------------------------ 6: trips of one block
def test_one_block_makes_five_trips(monkeypatch):
    rng = np.random.default_rng(12)
    data = noisy_text(rng, 40_000)                          # 1 250 lanes: five trips of one 256-lane block
    keys = tc.model(data, 31, True)[0][::10]                # (few enough for the LDS tier)
    want = filtered_model(data, 31, True, keys.tolist())
    default, stats, fs, db = filtered(data, 31, True, keys)
    db.close()
    assert fs["tier"] == "lds"
    for lds in ("1", "0"):
        monkeypatch.setenv("KM_COUNT_FILTER_BLOCKS", "1")
        monkeypatch.setenv("KM_COUNT_FILTER_LDS", lds)
        one, stats1, fs1, db = filtered(data, 31, True, keys)
        db.close()
        monkeypatch.delenv("KM_COUNT_FILTER_BLOCKS")
        monkeypatch.delenv("KM_COUNT_FILTER_LDS")
        assert one == default == want and stats1 == stats and fs1["kmers_hit"] == fs["kmers_hit"] == sum(want.values())
        assert fs1["tier"] == ("lds" if lds == "1" else "hbm")


# ------------------------------------------------------------------ 7: the three feeds agree
def test_the_three_feeds_agree(monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "65536")     # several pieces per feed
    reads = tc.make_reads(13, 2000)
    rng = np.random.default_rng(14)
    text = tc.as_fastq(reads, rng)
    long_reads = [r for r in reads if len(r) >= 100]
    keys = np.concatenate([tc.model(long_reads[0], 31, True)[0], tc.model(long_reads[1], 31, True)[0]])
    assert keys.size > 60
    key_set = sorted(set(keys.tolist()))

    def restricted(counter):
        db = counter.finish(1)
        db.close()
        got = records_dict(counter)
        counter.close()
        return {key: got.get(key, 0) for key in key_set}

    plain = kmlib.Counter(k=31)
    plain.add_text(text, final=True)
    want = restricted(plain)
    assert sum(want.values()) > 0
    masked = kmlib.Counter(k=31)
    masked.add_fastq(text, final=True, min_qual_char=">")
    want_masked = restricted(masked)
    assert want_masked != want

    def one_call(c):
        assert c.add_text(text, final=True) == len(text)

    def small_calls(c):
        pos, tail = 0, b""
        while pos < len(text):
            step = int(rng.integers(1, 20_000))
            buf = tail + text[pos:pos + step]
            pos += step
            used = c.add_text(buf, final=False)
            tail = buf[used:]
        c.add_text(tail, final=True)

    def fastq(q):
        def feed(c):
            half = kmlib.fastq_cut(text[:len(text) // 2])
            assert c.add_fastq(text[:half], final=False, min_qual_char=q) == half
            c.add_fastq(text[half:], final=True, min_qual_char=q)
        return feed

    fresh = kmlib.Counter(k=31)
    fresh.set_filter(keys)
    at_start = fresh.stats()
    fresh.close()
    assert at_start["slots"] == slots_for(len(key_set)) and at_start["n_grow"] == 0 and at_start["kmers"] == 0
    for feed, expect in ((one_call, want), (small_calls, want), (fastq(0), want), (fastq(">"), want_masked)):
        rec, stats, fs, db = filtered(None, 31, True, keys, feed=feed)
        db.close()
        assert rec == expect
        assert (stats["slots"], stats["n_grow"], stats["distinct"]) == (
            at_start["slots"], at_start["n_grow"], at_start["distinct"])
        assert fs["kmers_hit"] == sum(expect.values())


# ------------------------------------------------------------------ 8: the empty filter
def test_empty_filter_counts_nothing():
    data = noisy_text(np.random.default_rng(15), 3000)
    rec, stats, fs, db = filtered(data, 31, True, [])
    assert rec == {} and db.info.n_records == 0
    assert fs["n_keys"] == 0 and fs["kmers_hit"] == 0 and fs["tier"] == "lds"
    assert stats["kmers"] == int(tc.model(data, 31, True)[1].sum()) > 0
    assert stats["distinct"] == 0 and stats["slots"] == 64 and stats["n_grow"] == 0
    db.close()


# ------------------------------------------------------------------ 9: state
def _refused(code, call):
    with pytest.raises(kmlib.KmError) as e:
        call()
    assert e.value.code == code, e.value


def test_state_and_argument_errors_leave_the_counter_usable(tmp_path):
    data = b"ACGTACGTTGCATGCAACGT"
    keys = tc.model(data, 5, False)[0]
    jf = str(tmp_path / "k5.jf")
    kc.write_records(jf, keys, np.ones(keys.size, np.uint32), 5, False)
    # a counter that has been fed refuses a filter, and goes on counting everything
    c = kmlib.Counter(k=5, canonical=False)
    c.add_bases(data)
    _refused(E_STATE, lambda: c.set_filter(keys[:2]))
    c.add_bases(data)
    assert c.filter_stats()["tier"] == "none"
    c.finish().close()
    assert tc.same(tc.sorted_records(c), tc.model(data + b"\n" + data, 5, False))
    c.close()
    # a key that is no k-mer of this k: refused, and the counter still takes a filter
    c = kmlib.Counter(k=5, canonical=False)
    _refused(E_ARG, lambda: c.set_filter(np.array([3, 1024], np.uint64)))
    _refused(E_ARG, lambda: c.set_filter(np.array([ALLT], np.uint64)))
    c.set_filter(keys[:3])
    # a second filter, and records of any kind
    ones = np.ones(3, np.uint32)
    for call in (lambda: c.set_filter(keys[:3]), lambda: c.add_records(keys[:3], ones), lambda: c.add_jf(jf),
                 lambda: c.set_records(keys[:3], ones), lambda: c.set_jf(jf)):
        _refused(E_STATE, call)
    c.add_bases(data)
    _refused(E_STATE, lambda: c.add_records(keys[:3], ones))
    c.finish(0).close()
    assert records_dict(c) == filtered_model(data, 5, False, keys[:3].tolist())
    c.close()


# ------------------------------------------------------------------ 10: the command line
def _count(argv):
    err = io.StringIO()
    parser = cli.build_parser()
    args = cli.parse_args(["count"] + argv, parser)
    del args._cmd
    cli.main_count(args, err=err)
    return err.getvalue()


def _file_records(path):
    rec = jr.read_jf(str(path))
    assert rec["k"] == 31 and rec["canonical"] is True
    return dict(zip(rec["keys"].tolist(), rec["counts"].tolist())), rec


def test_command_line(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    names = sorted(os.listdir(tc.CATALOG))[:2]
    targets = [os.path.join(tc.CATALOG, f) for f in names]
    reads = tc.make_reads(16, 3000)
    with open("reads.fq", "wb") as fh:
        fh.write(tc.as_fastq(reads, np.random.default_rng(17)))
    target_keys = sorted(set(kc.query_keys(31, True, seq_files=targets).tolist()))
    full = dict(zip(*(a.tolist() for a in tc.model(b"\n".join(reads), 31, True))))
    want = {key: full.get(key, 0) for key in target_keys}
    assert 0 in want.values() or len(want) > 100

    if_args = [a for t in targets for a in ("--if", t)]
    err = _count(if_args + ["-m", "31", "-C", "-L", "0", "-o", "f.jf", "reads.fq"])
    got, rec = _file_records("f.jf")
    assert got == want
    assert rec["header"]["cmdline"][:2] == ["km_amd", "count"]
    for t in targets:
        at = rec["header"]["cmdline"].index(t)
        assert rec["header"]["cmdline"][at - 1] == "--if"
    lines = dict(line[1:].split(":") for line in err.splitlines() if line.startswith("#"))
    assert int(lines["filter_kmers"]) == len(want) and int(lines["kmers_hit"]) == sum(want.values())
    assert lines["filter_tier"] in ("lds", "hbm")
    assert lines["filter_tier"] == ("lds" if len(want) <= 4096 else "hbm")
    assert int(lines["kmers"]) == sum(full.values()) and int(lines["n_grow"]) == 0

    _count(if_args + ["-m", "31", "-C", "-o", "f1.jf", "reads.fq"])                     # -L 1 drops the zeros
    assert _file_records("f1.jf")[0] == {key: n for key, n in want.items() if n}

    _count(["-m", "31", "-C", "-o", "small.jf"] + targets)                              # the set as a table
    assert sorted(_file_records("small.jf")[0]) == target_keys
    _count(["--if", "small.jf", "-m", "31", "-C", "-L", "0", "-o", "g.jf", "reads.fq"])
    assert _file_records("g.jf")[0] == want

    _count(if_args + ["-m", "31", "-C", "-L", "0", "-o", "d.jf", "--dump", "d.txt", "reads.fq"])
    with open("dumped.txt", "wb") as out:
        kc.dump_file("d.jf", out=out, fmt="column")
    with open("d.txt", "rb") as a, open("dumped.txt", "rb") as b:
        text = a.read()
        assert text == b.read()
    assert len(text.splitlines()) == len(want)

    _count(if_args + ["-m", "31", "-C", "-L", "0", "--jellyfish-order", "-o", "j.jf", "reads.fq"])
    assert _file_records("j.jf")[0] == want

    env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, "-m", "km_amd", "count", "--if", "small.jf", "-m", "21", "-C", "-o", "bad.jf",
                          "reads.fq"], cwd=tmp_path, capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 1 and res.stderr.splitlines()[-1].startswith("ERROR: count:") and "k=31" in res.stderr
    assert not os.path.exists("bad.jf")
    for bad in ("missing.fa", "reads.fq"):                  # a missing file, a foreign one
        with pytest.raises(SystemExit) as e:
            _count(["--if", bad, "-m", "31", "-C", "-o", "bad.jf", "reads.fq"])
        assert str(e.value.code).startswith("ERROR: count:") and not os.path.exists("bad.jf")
