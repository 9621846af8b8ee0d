"""`compare` on the GPU (km_counter_mark_records, km_counter_mark_jf, km_counter_cooccurrence,
km_amd.count.compare_files, `python -m km_amd compare`).

Every comparison is exact, against compare_model of tests/test_compare_cpu.py: Python sets from the rule of
include/kmgpu.h, no code shared with the kernels.  Sets are read with oracle.jf_reader or built from arrays.  The
semantics are this project's own."""
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from km_amd import count as kc
from km_amd import lib as kmlib
from oracle import jf_reader as jr
import test_merge as tm
from test_compare_cpu import compare_model, same_result

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JF_DIR = os.path.join(HERE, "data", "jf")
FIXTURES = sorted(f for f in os.listdir(JF_DIR) if f.endswith(".jf"))
TOP = 0xFFFFFFFF
ALL_T = 0xFFFFFFFFFFFFFFFF
STATE, CAPACITY, ARG = 7, 8, 4


def compared(inputs, k=31, canonical=True, lower=1, upper=TOP, expected_distinct=0):
    """The inputs, one mark_records call each, through a counter of their own -> (result, stats)."""
    c = kmlib.Counter(k=k, canonical=canonical, expected_distinct=expected_distinct)
    try:
        for keys, counts in inputs:
            c.mark_records(keys, counts, lower, upper)
        return c.cooccurrence(), c.stats()
    finally:
        c.close()


def ones(keys):
    keys = np.asarray(keys, np.uint64)
    return keys, np.ones(keys.size, np.uint32)


# ------------------------------------------------------------------ 1. the five real tables
@functools.lru_cache(maxsize=None)
def real_inputs():
    assert len(FIXTURES) == 5
    out = []
    for name in FIXTURES:
        rec = jr.read_jf(os.path.join(JF_DIR, name))
        out.append((rec["keys"], rec["counts"]))
    return out


def test_the_five_real_tables_through_compare_files():
    paths = [os.path.join(JF_DIR, name) for name in FIXTURES]
    for lower, upper in ((1, TOP), (2, TOP), (1, 5)):
        want = compare_model(real_inputs(), lower, upper)
        result, stats = kc.compare_files(paths, lower_count=lower, upper_count=upper)
        assert same_result(result, want), (lower, upper)
        assert result["records"] == [keys.size for keys, _ in real_inputs()]
        passed = sum(int(np.count_nonzero((counts >= max(lower, 1)) & (counts <= upper))) for _, counts in real_inputs())
        assert stats["records_in"] == passed and stats["k"] == 31 and stats["distinct"] == want["union"]
    assert want["union"] > 0 and sum(want["in_exactly"][2:]) > 0          # the tables do overlap: the check is not idle


def test_the_five_real_tables_through_the_command(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system")
    for name in FIXTURES:
        shutil.copy(os.path.join(JF_DIR, name), tmp_path / name)

    def km(*args):
        res = subprocess.run([sys.executable, "-m", "km_amd", "compare"] + list(args), cwd=tmp_path, capture_output=True,
                             text=True, timeout=300, env=env)
        assert res.returncode == 0, res.stderr
        return res

    want = dict(compare_model(real_inputs()), records=[keys.size for keys, _ in real_inputs()])
    res = km(*FIXTURES)
    assert res.stdout == kc.format_compare(FIXTURES, want, "pairs") and len(res.stdout.splitlines()) == 1 + 10
    # one row written out by hand: the only pair of the five that shares k-mers, 685 of them (the record count of
    # `merge --min` of the two files, DESIGN.md §10 "Set operations"); 685 / (1604 + 2560 - 685), 685 / 1604, 685 / 2560
    assert res.stdout.splitlines()[8] == "03H112_IandI.jf\t03H116_ITD.jf\t1604\t2560\t685\t0.196896\t0.427057\t0.267578"
    err = dict(line[1:].split(":") for line in res.stderr.splitlines() if line.startswith("#"))
    assert (int(err["inputs"]), int(err["union"]), int(err["core"])) == (5, want["union"], want["in_exactly"][5])
    assert int(err["records_in"]) == sum(int(np.count_nonzero(counts)) for _, counts in real_inputs())
    assert int(err["slots"]) >= 2 * want["union"] and int(err["n_grow"]) >= 0
    assert km("--matrix", "jaccard", *FIXTURES).stdout == kc.format_compare(FIXTURES, want, "jaccard")
    assert km("--matrix", "shared", "-o", "m.tsv", *FIXTURES).stdout == ""
    assert (tmp_path / "m.tsv").read_text() == kc.format_compare(FIXTURES, want, "shared")
    res = km("--summary", "s.tsv", "--spectrum", "p.tsv", *FIXTURES)
    assert res.stdout == kc.format_compare(FIXTURES, want, "pairs")
    assert (tmp_path / "s.tsv").read_text() == kc.format_compare(FIXTURES, want, "summary")
    assert (tmp_path / "p.tsv").read_text() == kc.format_compare(FIXTURES, want, "spectrum")
    # the cut, and a file given twice: Jaccard 1.000000 with itself
    cut = dict(compare_model([real_inputs()[0], real_inputs()[1], real_inputs()[0]], 3, 50),
               records=[real_inputs()[i][0].size for i in (0, 1, 0)])
    names = [FIXTURES[0], FIXTURES[1], FIXTURES[0]]
    res = km("-L", "3", "-U", "50", *names)
    assert res.stdout == kc.format_compare(names, cut, "pairs")
    twice = res.stdout.splitlines()[2].split("\t")
    assert twice[:2] == [FIXTURES[0], FIXTURES[0]] and twice[5:] == ["1.000000", "1.000000", "1.000000"] and int(twice[4]) > 0
    # one input is legal and gives no pair rows
    assert km(FIXTURES[2]).stdout == "a\tb\tdistinct_a\tdistinct_b\tshared\tjaccard\tcontain_a\tcontain_b\n"


# ------------------------------------------------------------------ 2. every pair at once
@functools.lru_cache(maxsize=None)
def universe_inputs():
    """32 inputs over 4 096 random keys: input i holds a key with probability (i + 1) / 33."""
    rng = np.random.default_rng(3233)
    pool = np.unique(tm.random_keys(rng, 4200, 31))[:4096]
    assert pool.size == 4096
    inputs = []
    for i in range(32):
        keys = rng.permutation(pool[rng.random(4096) < (i + 1) / 33])
        inputs.append((keys, rng.integers(1, 1000, keys.size).astype(np.uint32)))
    return inputs


@functools.lru_cache(maxsize=None)
def universe_model(n):
    return compare_model(universe_inputs()[:n])


@pytest.mark.parametrize("n", [1, 2, 31, 32])
def test_every_pair_at_once(n):
    want = universe_model(n)
    if n == 32:                                      # the 528 values mostly differ: a swapped pair would show
        assert len({want["shared"][i][j] for i in range(32) for j in range(i + 1)}) > 264
    c = kmlib.Counter(k=31)
    try:
        for keys, counts in universe_inputs()[:n]:
            c.mark_records(keys, counts)
        got = c.cooccurrence()
        assert same_result(got, want)
        if n == 32:
            with pytest.raises(kmlib.KmError) as e:
                c.mark_records(*universe_inputs()[0])
            assert e.value.code == CAPACITY
            with pytest.raises(kmlib.KmError) as e:
                c.mark_jf(os.path.join(JF_DIR, FIXTURES[0]))
            assert e.value.code == CAPACITY
            assert same_result(c.cooccurrence(), want)
    finally:
        c.close()


# ------------------------------------------------------------------ 3. the smallest tables
# A table of 64 slots is one trip of wave 0 of block 0: waves 1 .. 3 leave the loop at once and meet the others only at
# the block's barriers outside it.  128 slots: two waves make a trip, two none.
def test_one_key_in_a_table_of_64_slots():
    inputs = [ones([12345]), ones([12345]), ones([])]
    got, stats = compared(inputs, expected_distinct=1)
    assert stats["slots"] == 64 and same_result(got, compare_model(inputs))
    assert got["union"] == 1 and got["shared"].tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 0]]


def test_twenty_keys_in_64_slots_with_an_empty_input_between():
    rng = np.random.default_rng(20)
    keys = np.unique(tm.random_keys(rng, 30, 31))[:20]
    inputs = [ones(keys[:10]), ones(keys[5:15]), ones([]), ones(keys[10:])]
    got, stats = compared(inputs, expected_distinct=20)
    want = compare_model(inputs)
    assert stats["slots"] == 64 and stats["n_grow"] == 0 and same_result(got, want)
    assert want["union"] == 20 and want["shared"][2] == [0, 0, 0, 0] and want["shared"][1][0] == 5 and want["private"] == [5, 0, 0, 5]


def test_forty_keys_in_128_slots():
    rng = np.random.default_rng(40)
    keys = np.unique(tm.random_keys(rng, 50, 31))[:40]
    inputs = [ones(keys[:20]), ones(keys[10:30]), ones(keys[20:])]
    got, stats = compared(inputs, expected_distinct=40)
    assert stats["slots"] == 128 and stats["n_grow"] == 0 and same_result(got, compare_model(inputs))
    assert got["union"] == 40 and got["in_exactly"].tolist() == [0, 20, 20, 0]


def test_all_inputs_empty():
    for slots_for in (1, 0):                                             # 64 slots, and the default table
        got, _ = compared([ones([])] * 3, expected_distinct=slots_for)
        assert same_result(got, compare_model([ones([])] * 3))
        assert got["union"] == 0 and not got["shared"].any() and not got["in_exactly"].any() and not got["private"].any()
    got, _ = compared([])                                                # no input at all
    assert got["n_inputs"] == 0 and got["union"] == 0 and got["shared"].shape == (0, 0)


# ------------------------------------------------------------------ 4. pieces and growth
@functools.lru_cache(maxsize=None)
def growing_inputs():
    """Input 0: 3 000 keys in a table sized for them (8 192 slots); inputs 1 and 2: 300 of those and 2 700 new keys each."""
    rng = np.random.default_rng(44)
    pool = np.unique(tm.random_keys(rng, 9000, 31))[:8400]
    inputs = []
    for i in range(3):
        keys = rng.permutation(pool[2700 * i:2700 * i + 3000])
        inputs.append((keys, rng.integers(1, 100, keys.size).astype(np.uint32)))
    return inputs


@functools.lru_cache(maxsize=None)
def growing_default():
    return compared(growing_inputs(), expected_distinct=3000)


@pytest.mark.parametrize("stage", [256, 1024])
def test_masks_survive_growth_between_pieces(monkeypatch, stage):
    want = compare_model(growing_inputs())
    assert want["shared"][1][0] == 300 and want["shared"][2][1] == 300 and want["union"] == 8400
    default, default_stats = growing_default()
    assert same_result(default, want) and default_stats["n_grow"] > 0
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))
    got, stats = compared(growing_inputs(), expected_distinct=3000)
    assert stats["n_grow"] > 0 and stats["slots"] >= 2 * 8400
    assert same_result(got, want)
    for key in ("shared", "in_exactly", "private"):
        assert np.array_equal(got[key], default[key]), key


# ------------------------------------------------------------------ 5. record widths and the key without a slot
@pytest.mark.parametrize("k,counter_len", [(5, 1), (11, 2), (13, 3), (17, 4), (21, 1), (25, 2)])
def test_record_widths(tmp_path, k, counter_len):
    rng = np.random.default_rng(100 * k + counter_len)
    space = 1 << (2 * k)
    pool = np.unique(rng.integers(0, space, 600, dtype=np.uint64))[:300]
    inputs, paths = [], []
    for i in range(3):
        keys = np.sort(pool[rng.random(pool.size) < 0.6])
        counts = rng.integers(0, 1 << (8 * counter_len), keys.size, dtype=np.uint64).astype(np.uint32)
        counts[:3] = 0                                                   # absent records
        inputs.append((keys, counts))
        paths.append(tm.write_file(tmp_path / ("w%d.jf" % i), keys, counts, k, counter_len=counter_len))
    info = kmlib.jf_file_info(paths[0])
    assert info["key_bytes"] == (2 * k + 7) // 8 < 8 and info["counter_len"] == counter_len
    for lower, upper in ((1, TOP), (2, 200)):
        result, _ = kc.compare_files(paths, lower_count=lower, upper_count=upper)
        assert same_result(result, compare_model(inputs, lower, upper)), (lower, upper)


def test_all_t_of_a_non_canonical_k32_table(tmp_path):
    rng = np.random.default_rng(32)
    others = np.unique(tm.random_keys(rng, 90, 32))[:80]
    others = others[others != np.uint64(ALL_T)]
    def with_all_t(keys, count):
        keys = np.concatenate([keys, np.array([ALL_T], np.uint64)])
        return keys, np.concatenate([np.full(keys.size - 1, 7, np.uint32), np.array([count], np.uint32)])
    inputs = [with_all_t(others[:50], 5), with_all_t(others[30:], 1), with_all_t(others[10:40], 9), (others[:5], np.full(5, 7, np.uint32))]
    without = [(keys[keys != np.uint64(ALL_T)], counts[keys != np.uint64(ALL_T)]) for keys, counts in inputs]
    want, base = compare_model(inputs, 2), compare_model(without, 2)
    # T^32 is in inputs 0 and 2, and in input 1 only below the cut: it shows in all four numbers
    assert want["shared"][0][0] == base["shared"][0][0] + 1 and want["shared"][2][0] == base["shared"][2][0] + 1
    assert want["shared"][1] == base["shared"][1] and want["union"] == base["union"] + 1
    assert want["in_exactly"][2] == base["in_exactly"][2] + 1 and want["private"] == base["private"]
    got, _ = compared(inputs, k=32, canonical=False, lower=2)
    assert same_result(got, want)
    paths = [tm.write_file(tmp_path / ("t%d.jf" % i), *inp, 32, canonical=False) for i, inp in enumerate(inputs)]
    result, _ = kc.compare_files(paths, lower_count=2)
    assert same_result(result, want)
    # alone in one input it is private to it, and with nothing else in any input it is the whole union
    alone = [(np.array([ALL_T], np.uint64), np.array([3], np.uint32)), ones([])]
    got, _ = compared(alone, k=32, canonical=False, expected_distinct=1)
    assert same_result(got, compare_model(alone)) and got["private"].tolist() == [1, 0] and got["union"] == 1


# ------------------------------------------------------------------ 6. cuts
def test_cuts_are_per_record_and_membership_is_idempotent():
    rng = np.random.default_rng(6)
    pool = np.unique(tm.random_keys(rng, 700, 31))[:600]
    inputs = []
    for i in range(4):
        keys = rng.permutation(pool[rng.random(pool.size) < 0.5])
        counts = rng.choice(np.array([0, 1, 2, 3, 50, 100, 101, TOP], np.uint32), keys.size)
        inputs.append((keys, counts))
    # a key with two records in input 0, one passing the cut and one not: present; and the other way round in input 1
    two = pool[0]
    inputs[0] = (np.concatenate([inputs[0][0][inputs[0][0] != two], [two, two]]).astype(np.uint64),
                 np.concatenate([inputs[0][1][inputs[0][0] != two], [1, 60]]).astype(np.uint32))
    inputs[1] = (np.concatenate([inputs[1][0][inputs[1][0] != two], [two, two]]).astype(np.uint64),
                 np.concatenate([inputs[1][1][inputs[1][0] != two], [0, 101]]).astype(np.uint32))
    for lower, upper in ((3, 100), (1, TOP), (0, TOP), (2, 2), (101, TOP), (5, 4)):
        want = compare_model(inputs, lower, upper)
        got, _ = compared(inputs, lower=lower, upper=upper)
        assert same_result(got, want), (lower, upper)
    want = compare_model(inputs, 3, 100)
    assert want["shared"][0][0] == len({k for k, c in zip(inputs[0][0].tolist(), inputs[0][1].tolist()) if 3 <= c <= 100})
    assert two in set(inputs[0][0][(inputs[0][1] >= 3) & (inputs[0][1] <= 100)].tolist())
    assert compare_model(inputs, 5, 4)["union"] == 0
    # the same records twice within one call change nothing
    doubled = [(np.concatenate([keys, keys]), np.concatenate([counts, counts])) for keys, counts in inputs]
    got, _ = compared(doubled, lower=3, upper=100)
    assert same_result(got, want)


# ------------------------------------------------------------------ 7. state rules
def test_mark_and_the_other_feeds_do_not_mix(tmp_path):
    keys, counts = ones(np.arange(1, 40, dtype=np.uint64))
    feeds = {"text": lambda c: c.add_bases(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGT"),
             "sum": lambda c: c.add_records(keys, counts), "set": lambda c: c.set_records(keys, counts)}
    good = tm.write_file(tmp_path / "good.jf", keys, counts, 31)
    for name, feed in feeds.items():
        c = kmlib.Counter(k=31)
        try:
            feed(c)
            for call in (lambda: c.mark_records(keys, counts), lambda: c.mark_jf(good), c.cooccurrence):
                with pytest.raises(kmlib.KmError) as e:
                    call()
                assert e.value.code == STATE, name
            feed(c)                                                      # the refusals changed nothing
        finally:
            c.close()
    c = kmlib.Counter(k=31)
    try:
        c.mark_records(keys, counts)
        calls = [lambda: c.add_bases(b"ACGT" * 10), lambda: c.add_text(b">r\nACGT\n", final=True),
                 lambda: c.add_fastq(b"@r\nACGT\n+\nIIII\n", final=True), lambda: c.add_records(keys, counts),
                 lambda: c.add_jf(good), lambda: c.set_records(keys, counts), lambda: c.set_jf(good, op="subtract")]
        for i, call in enumerate(calls):
            with pytest.raises(kmlib.KmError) as e:
                call()
            assert e.value.code == STATE, i
        c.mark_records(keys[:10], counts[:10])
        assert same_result(c.cooccurrence(), compare_model([(keys, counts), (keys[:10], counts[:10])]))
    finally:
        c.close()


def test_a_mark_counter_has_no_counts_to_read_and_stays_usable(tmp_path):
    rng = np.random.default_rng(7)
    pool = np.unique(tm.random_keys(rng, 500, 31))[:400]
    inputs = [ones(rng.permutation(pool)[:250]) for _ in range(3)]
    other_k = tm.write_file(tmp_path / "k21.jf", [1, 2], [1, 1], 21)
    other_strand = tm.write_file(tmp_path / "nc.jf", [1, 2], [1, 1], 31, canonical=False)
    c, plain = kmlib.Counter(k=31), kmlib.Counter(k=31)
    try:
        assert same_result(c.cooccurrence(), compare_model([]))
        c.mark_records(*inputs[0])
        assert same_result(c.cooccurrence(), compare_model(inputs[:1]))
        with open(tmp_path / "dump.txt", "wb") as fh:
            reads = [(c.finish, "km_counter_finish "), (lambda: c.finish(1, 100), "km_counter_finish_range "),
                     (c.records, "km_counter_records "), (c.n_records, "km_counter_records "),
                     (lambda: c.write_jf(str(tmp_path / "out.jf")), "km_counter_write_jf "), (c.histo, "km_counter_histo "),
                     (lambda: c.dump(fh, fmt="column"), "km_counter_dump ")]
            for i, (call, named) in enumerate(reads):
                with pytest.raises(kmlib.KmError) as e:
                    call()
                assert e.value.code == STATE and "mark" in str(e.value) and named in str(e.value), i
        assert not (tmp_path / "out.jf").exists() and (tmp_path / "dump.txt").read_bytes() == b""
        for path in (other_k, other_strand, str(tmp_path / "no_such.jf")):  # a refused file is no input
            with pytest.raises(kmlib.KmError) as e:
                c.mark_jf(path)
            assert e.value.code in (ARG, 1) and (e.value.code == 1) == path.endswith("no_such.jf")
            with pytest.raises(kmlib.KmError) as f:
                plain.add_jf(path)
            assert str(f.value) == str(e.value)                          # the message km_counter_add_jf gives
        c.mark_records(*inputs[1])
        between = c.cooccurrence()
        assert same_result(between, compare_model(inputs[:2]))
        again = c.cooccurrence()                                         # the table is left as it was
        assert same_result(again, compare_model(inputs[:2]))
        c.mark_records(*inputs[2])
        assert same_result(c.cooccurrence(), compare_model(inputs))
        assert c.merge_stats()["records_in"] == 750 and c.stats()["distinct"] == compare_model(inputs)["union"]
    finally:
        c.close()
        plain.close()


def test_timed_runs_change_nothing_and_report_something(monkeypatch):
    want = universe_model(2)
    monkeypatch.delenv("KM_COUNT_TIME_MERGE", raising=False)
    untimed = kmlib.Counter(k=31)
    monkeypatch.setenv("KM_COUNT_TIME_MERGE", "1")
    timed = kmlib.Counter(k=31)
    try:
        for c in (untimed, timed):
            for keys, counts in universe_inputs()[:2]:
                c.mark_records(keys, counts)
        a, b = untimed.cooccurrence(), timed.cooccurrence()
        assert same_result(a, want) and same_result(b, want)
        assert a["kernel_ms"] == 0 and untimed.merge_stats()["kernel_ms"] == 0
        assert b["kernel_ms"] > 0 and timed.merge_stats()["kernel_ms"] > 0
        assert timed.cooccurrence()["kernel_ms"] > b["kernel_ms"]          # a time of its own, which only grows
    finally:
        untimed.close()
        timed.close()
