"""Set operations over tables that already exist (km_counter_set_records, km_counter_set_jf, km_counter_finish_range,
km_amd.count.merge_files(mode="intersect" | "subtract"), `python -m km_amd merge --min | --subtract | -U`).

Every comparison is exact.  The model is written here from the definitions and shares no code with the kernels:
  intersect  the keys present, with count > 0, in every input; the count is the minimum over all their records;
  subtract   the records of the first input whose key occurs, with count > 0, in no later input; the count is the first
             input's, a key repeated inside it summed and clipped at 2^32 - 1;
a record with count 0 is absent, an input without records is an input, the cut lower <= count <= upper comes last.
The definitions are this project's own: no run of `jellyfish merge --min` stands behind them."""
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from km_amd import cli
from km_amd import count as kc
from km_amd import lib as kmlib
from oracle import jf_reader as jr
import test_merge as tm
from test_merge import fixture, random_keys, same, write_file

JF_DIR = tm.JF_DIR
ROOT = tm.ROOT
IANDI, ITD, NPM1 = "03H112_IandI.jf", "03H116_ITD.jf", "02H025_NPM1.jf"
TOP = 0xFFFFFFFF
ALL_T = 0xFFFFFFFFFFFFFFFF
STATE, ARG = 7, 4                                                       # KM_E_STATE, KM_E_ARG


# ------------------------------------------------------------------ the model
def set_model(inputs, op, lower=1, upper=TOP):
    """inputs: (keys, counts) per input, in order -> (keys ascending, counts) of the set operation after the cuts."""
    def present(keys, counts, combine):
        acc = {}
        for key, c in zip(np.asarray(keys, np.uint64).tolist(), np.asarray(counts, np.uint32).tolist()):
            if c:
                acc[key] = combine(acc[key], c) if key in acc else c
        return acc
    if op == "intersect":
        acc = present(*inputs[0], min)
        for later in inputs[1:]:
            there = present(*later, min)
            acc = {key: min(c, there[key]) for key, c in acc.items() if key in there}
    else:
        acc = present(*inputs[0], lambda a, b: min(a + b, TOP))
        for later in inputs[1:]:
            there = present(*later, min)
            acc = {key: c for key, c in acc.items() if key not in there}
    items = sorted((key, c) for key, c in acc.items() if lower <= c <= upper)
    return (np.array([key for key, _ in items], np.uint64), np.array([c for _, c in items], np.uint32))


def arrays(pairs):
    return (np.array([p[0] for p in pairs], np.uint64), np.array([p[1] for p in pairs], np.uint32))


def on_gpu(feed, k=31, canonical=True, lower=1, upper=TOP, expected_distinct=0):
    """feed(counter) feeds; -> (keys ascending, counts, stats before the cut)."""
    c = kmlib.Counter(k=k, canonical=canonical, expected_distinct=expected_distinct)
    try:
        feed(c)
        stats = c.stats()
        c.finish(lower, upper).close()
        keys, counts = c.records()
    finally:
        c.close()
    order = np.argsort(keys, kind="stable")
    return keys[order], counts[order], stats


def set_records_on_gpu(inputs, op, **kw):
    return on_gpu(lambda c: [c.set_records(keys, counts, op=op) for keys, counts in inputs], **kw)[:2]


def set_files_on_gpu(paths, op, **kw):
    return on_gpu(lambda c: [c.set_jf(p, op=op) for p in paths], **kw)[:2]


# ------------------------------------------------------------------ CPU
def test_parser_accepts_the_set_flags_and_refuses_their_combinations(capsys):
    args = cli.parse_args(["merge", "a.jf"])
    assert (args.min, args.subtract, args.max, args.upper_count, args.lower_count) == (False, False, False, None, 1)
    args = cli.parse_args(["merge", "--min", "-U", "7", "-L", "2", "a.jf", "b.jf"])
    assert (args.min, args.subtract, args.max, args.upper_count, args.lower_count) == (True, False, False, 7, 2)
    args = cli.parse_args(["merge", "--subtract", "--upper-count", "4294967295", "a.jf", "b.jf"])
    assert (args.min, args.subtract, args.max, args.upper_count) == (False, True, False, TOP)
    args = cli.parse_args(["merge", "--max", "-U", "0", "a.jf"])
    assert (args.max, args.upper_count) == (True, 0)
    for flags in (["--min", "--subtract"], ["--min", "--max"], ["--subtract", "--max"], ["--min", "--subtract", "--max"],
                  ["-U", "4294967296"], ["-U", "-1"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["merge"] + flags + ["a.jf", "b.jf"])
        assert e.value.code == 2, flags
    capsys.readouterr()


@pytest.mark.parametrize("mode", ["intersect", "subtract"])
def test_merge_files_refuses_a_mismatch_before_any_counter(tmp_path, mode):
    a = write_file(tmp_path / "a.jf", [1, 2], [3, 4], 31)
    b = write_file(tmp_path / "b.jf", [1, 2], [3, 4], 21)
    c = write_file(tmp_path / "c.jf", [1, 2], [3, 4], 31, canonical=False)
    for other in (b, c):
        with pytest.raises(ValueError) as e:                            # (raised without a GPU: no counter exists yet)
            kc.merge_files([a, a, other], mode=mode)
        assert other in str(e.value) and a in str(e.value) and "k=31" in str(e.value)
    with pytest.raises(ValueError):
        kc.merge_files([], mode=mode)


def test_argument_errors_without_a_counter():
    lib = kmlib.load()
    keys, counts = np.zeros(2, np.uint64), np.ones(2, np.uint32)
    out = kmlib.C.c_void_p()
    assert lib.km_counter_set_records(None, kmlib.ptr(keys), kmlib.ptr(counts), 2, 0) == ARG
    assert lib.km_counter_set_jf(None, b"x.jf", 0, None) == ARG
    assert lib.km_counter_finish_range(None, 1, 2, kmlib.C.byref(out)) == ARG
    assert kmlib.SET_OPS == {"intersect": 0, "subtract": 1}


def test_the_model_on_hand_written_cases():
    a = arrays([(5, 3), (9, 7), (9, 2), (11, 0), (20, TOP), (20, 5), (30, 4)])
    b = arrays([(9, 6), (9, 0), (5, 0), (20, 9), (40, 1)])
    c = arrays([(20, 8), (9, 1), (30, 2)])
    none = arrays([])

    def pairs(got):
        return list(zip(got[0].tolist(), got[1].tolist()))
    # one input: a filter; zero counts are absent; repeats: the min, or the clipped sum
    assert pairs(set_model([a], "intersect")) == [(5, 3), (9, 2), (20, 5), (30, 4)]
    assert pairs(set_model([a], "subtract")) == [(5, 3), (9, 9), (20, TOP), (30, 4)]
    # two and three inputs; 5 is in b with count 0 only: absent there
    assert pairs(set_model([a, b], "intersect")) == [(9, 2), (20, 5)]
    assert pairs(set_model([a, b], "subtract")) == [(5, 3), (30, 4)]
    assert pairs(set_model([a, b, c], "intersect")) == [(9, 1), (20, 5)]
    assert pairs(set_model([a, c, b], "intersect")) == [(9, 1), (20, 5)]
    assert pairs(set_model([a, b, c], "subtract")) == [(5, 3)]
    # 30 is in a and c but not in b: dead whatever comes later
    assert 30 not in set_model([a, b, c], "intersect")[0] and 30 in set_model([a, c], "intersect")[0]
    # an input without records is an input
    assert pairs(set_model([a, none], "intersect")) == [] and pairs(set_model([none, a], "intersect")) == []
    assert pairs(set_model([a, none], "subtract")) == pairs(set_model([a], "subtract"))
    assert pairs(set_model([none, a], "subtract")) == []
    # the cuts come last, on both sides
    assert pairs(set_model([a], "subtract", lower=4, upper=9)) == [(9, 9), (30, 4)]
    assert pairs(set_model([a], "intersect", lower=3, upper=4)) == [(5, 3), (30, 4)]
    assert pairs(set_model([a], "intersect", lower=4, upper=3)) == []
    got = set_model([a], "intersect")
    assert (got[0].dtype, got[1].dtype) == (np.uint64, np.uint32)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_the_real_files(tmp_path):
    iandi, itd, npm1 = fixture(IANDI), fixture(ITD), fixture(NPM1)
    p_iandi, p_itd = os.path.join(JF_DIR, IANDI), os.path.join(JF_DIR, ITD)
    for paths, inputs, op, size in (([p_iandi, p_itd], [iandi, itd], "intersect", 685),
                                    ([p_iandi, p_itd], [iandi, itd], "subtract", 919),
                                    ([p_itd, p_iandi], [itd, iandi], "subtract", 1875)):
        want = set_model(inputs, op)
        assert want[0].size == size
        assert same(set_files_on_gpu(paths, op), want), (op, size)
        db, stats = kc.merge_files(paths, mode=op)                     # sized from the first file only
        answer = db.query(np.concatenate([want[0], inputs[1][0]]))
        db.close()
        assert np.array_equal(answer[:size], want[1])
        assert np.array_equal(answer[size:] > 0, np.isin(inputs[1][0], want[0]))
        assert (stats["mode"], stats["records_out"], stats["k"], stats["canonical"]) == (op, size, 31, True)
        assert stats["distinct"] == inputs[0][0].size and stats["slots"] // 2 < 2 * inputs[0][0].size
        assert stats["records_in"] == inputs[0][0].size + inputs[1][0].size
    # all five intersected: nothing, and the empty result is a valid file
    all_paths = [os.path.join(JF_DIR, f) for f in tm.FIXTURES]
    all_inputs = [fixture(f) for f in tm.FIXTURES]
    assert set_model(all_inputs, "intersect")[0].size == 0
    db, stats, counter = kc.merge_files(all_paths, mode="intersect", keep_counter=True)
    try:
        out = str(tmp_path / "none.jf")
        counter.write_jf(out)
        assert counter.records()[0].size == 0 and stats["records_out"] == 0 and db.info.n_records == 0
    finally:
        counter.close()
        db.close()
    rec = jr.read_jf(out)
    assert (rec["k"], rec["canonical"], rec["keys"].size) == (31, True, 0)
    assert kmlib.jf_file_info(out)["n_records"] == 0
    # NPM1 minus the other four: all of it
    others = [f for f in tm.FIXTURES if f != NPM1]
    want = set_model([npm1] + [fixture(f) for f in others], "subtract")
    assert want[0].size == npm1[0].size == 1938
    got = set_files_on_gpu([os.path.join(JF_DIR, NPM1)] + [os.path.join(JF_DIR, f) for f in others], "subtract")
    assert same(got, want)


@pytest.mark.gpu
def test_gpu_dead_stays_dead_and_duplicates():
    rng = np.random.default_rng(90)
    x, y, z, w = (np.uint64(v) for v in (0x1111222233334444, 0x0ABCDEF012345678, 0x2222000011110000, 0x77))
    filler = np.unique(random_keys(rng, 400, 31))[:300]
    fc = rng.integers(1, 1000, (3, 300)).astype(np.uint32)
    one = arrays([(x, 9), (y, 8), (z, 50), (z, 40), (w, 5)])
    two = arrays([(y, 7), (y, 3), (z, 60), (z, 45), (z, 0), (w, 0)])   # x missing; w present with count 0 only
    three = arrays([(x, 9), (z, 41), (z, 44), (w, 0)])                  # y missing; w again with count 0 only
    inputs = [(np.concatenate([one[0], filler]), np.concatenate([one[1], fc[0]])),
              (np.concatenate([two[0], filler[:200]]), np.concatenate([two[1], fc[1][:200]])),
              (np.concatenate([three[0], filler[100:]]), np.concatenate([three[1], fc[2][100:]]))]
    want = set_model(inputs, "intersect")
    got = dict(zip(*(a.tolist() for a in set_records_on_gpu(inputs, "intersect"))))
    assert int(x) not in got and int(y) not in got and int(w) not in got and got[int(z)] == 40
    assert got == dict(zip(want[0].tolist(), want[1].tolist())) and len(got) == 101
    want = set_model(inputs, "subtract")
    got = set_records_on_gpu(inputs, "subtract")
    assert same(got, want) and got[0].tolist() == [int(w)] and got[1].tolist() == [5]
    # inputs 2..N in every order, four inputs, the first with 20 keys of its own: the same records
    own = np.unique(random_keys(rng, 30, 31))[:20]
    inputs[0] = (np.concatenate([inputs[0][0], own]), np.concatenate([inputs[0][1], fc[1][:20]]))
    inputs.append((np.concatenate([arrays([(z, 43), (x, 1)])[0], filler[50:250]]),
                   np.concatenate([arrays([(z, 43), (x, 1)])[1], fc[0][50:250]])))
    for op in ("intersect", "subtract"):
        first = set_model(inputs, op)
        assert first[0].size == (101 if op == "intersect" else 21)      # (w and the 20)
        for order in itertools.permutations(inputs[1:]):
            assert same(set_records_on_gpu([inputs[0]] + list(order), op), first), op
    # many records of few keys in every input: contention on the count cell and the spare word
    keys = random_keys(rng, 40, 31)
    inputs = []
    for i in range(3):
        pick = keys[:35] if i == 1 else keys[5:] if i == 2 else keys
        ks = pick[rng.integers(0, pick.size, 20_000)]
        inputs.append((ks, rng.integers(0, 1 << 30, ks.size).astype(np.uint32)))
    for op in ("intersect", "subtract"):
        assert same(set_records_on_gpu(inputs, op), set_model(inputs, op)), op


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["intersect", "subtract"])
def test_gpu_piece_boundaries(tmp_path, monkeypatch, op):
    rng = np.random.default_rng(91)
    real = [os.path.join(JF_DIR, IANDI), os.path.join(JF_DIR, ITD)]
    want = set_model([fixture(IANDI), fixture(ITD)], op)
    # k = 21: 6 + 4 bytes, 25 per piece of 256 bytes with 6 left over; 1 013 and 537 records, half of the second shared
    k1 = np.unique(random_keys(rng, 1100, 21))[:1013]
    k2 = np.concatenate([rng.permutation(k1)[:270], np.unique(random_keys(rng, 300, 21))[:267]])
    c1 = rng.integers(1, 1 << 32, k1.size, dtype=np.uint64).astype(np.uint32)
    c2 = rng.integers(1, 1 << 32, k2.size, dtype=np.uint64).astype(np.uint32)
    made = [write_file(tmp_path / "a21.jf", k1, c1, 21), write_file(tmp_path / "b21.jf", k2, c2, 21)]
    want21 = set_model([(k1, c1), (k2, c2)], op)
    assert kmlib.jf_file_info(made[0])["key_bytes"] == 6 and k1.size % 25 and k2.size % 25
    assert fixture(IANDI)[0].size % 21 and fixture(ITD)[0].size % 21    # the last piece of each is short
    assert want21[0].size >= 270 and want[0].size > 0
    default = set_files_on_gpu(real, op), set_files_on_gpu(made, op, k=21)
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "256")
    small = set_files_on_gpu(real, op), set_files_on_gpu(made, op, k=21)
    assert same(small[0], default[0]) and same(small[0], want)
    assert same(small[1], default[1]) and same(small[1], want21)


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["intersect", "subtract"])
def test_gpu_growth_ends_with_the_first_input(monkeypatch, op):
    """A counter made for 16 keys has 64 slots: 1 000 keys in the first input, in pieces of 85 records, make it double
    several times between pieces, which carries the counts of intersect (kept complemented) and the zero spare words
    through k_count_rehash; the 5 000 keys of the second input, 4 500 of them new, find a table that stays as it is."""
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "1024")
    rng = np.random.default_rng(92)
    pool = np.unique(random_keys(rng, 6000, 31))[:5500]
    first = (pool[:1000], rng.integers(1, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32))
    second_keys = rng.permutation(np.concatenate([pool[:500], pool[1000:]]))
    second = (second_keys, rng.integers(1, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32))
    seen = []

    def feed(c):
        c.set_records(*first, op=op)
        seen.append(c.stats())
        c.set_records(*second, op=op)
        seen.append(c.stats())
    keys, counts, _ = on_gpu(feed, expected_distinct=16)
    assert seen[0]["n_grow"] > 0 and seen[0]["slots"] >= 2048 and seen[0]["distinct"] == 1000
    assert (seen[1]["slots"], seen[1]["n_grow"], seen[1]["distinct"]) == (seen[0]["slots"], seen[0]["n_grow"], 1000)
    want = set_model([first, second], op)
    assert same((keys, counts), want) and want[0].size == 500


@pytest.mark.gpu
def test_gpu_record_widths_and_the_empty_mark(tmp_path):
    rng = np.random.default_rng(93)

    def counts32(n):
        return rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for op in ("intersect", "subtract"):
        # k = 5, not canonical: 2 key bytes, 4 count bytes; all 1 024 keys in the first input
        keys = rng.permutation(np.arange(1024, dtype=np.uint64))
        inputs = [(keys, counts32(1024)), (keys[::-1][:700], counts32(700)), (keys[300:], counts32(724))]
        paths = [write_file(tmp_path / ("k5_%d.jf" % i), *inp, 5, canonical=False) for i, inp in enumerate(inputs)]
        want = set_model(inputs, op)
        assert same(set_files_on_gpu(paths, op, k=5, canonical=False), want) and want[0].size > 0
        # k = 31 with 1 and 2 count bytes (9- and 10-byte records)
        keys = np.unique(random_keys(rng, 700, 31))[:600]
        inputs = [(keys, rng.integers(1, 256, 600).astype(np.uint32)),
                  (keys[100:], rng.integers(1, 65536, 500).astype(np.uint32))]
        paths = [write_file(tmp_path / "cb1.jf", *inputs[0], 31, counter_len=1),
                 write_file(tmp_path / "cb2.jf", *inputs[1], 31, counter_len=2)]
        assert [kmlib.jf_file_info(p)["counter_len"] for p in paths] == [1, 2]
        for order in ((0, 1), (1, 0)):
            want = set_model([inputs[i] for i in order], op)
            assert same(set_files_on_gpu([paths[i] for i in order], op), want), (op, order)
    # k = 32, not canonical: the key 2^64 - 1 (T^32, the table's empty mark) has cells of its own
    base = np.unique(np.concatenate([random_keys(rng, 300, 32), np.array([0], np.uint64)]))
    base = base[base != np.uint64(ALL_T)]

    def k32_input(all_t_count):
        """All of `base` but a random tenth, shuffled; T^32 with the given count (None: not there)."""
        keys = rng.permutation(base)[:270]
        counts = rng.integers(1, 1000, keys.size).astype(np.uint32)
        if all_t_count is not None:
            at = int(rng.integers(0, keys.size))
            keys = np.insert(keys, at, np.uint64(ALL_T))
            counts = np.insert(counts, at, np.uint32(all_t_count))
        return keys, counts

    def k32(inputs, op, **kw):
        paths = [write_file(tmp_path / ("k32_%d.jf" % i), *inp, 32, canonical=False) for i, inp in enumerate(inputs)]
        got = set_files_on_gpu(paths, op, k=32, canonical=False, **kw)
        assert same(got, set_model(inputs, op, **{k: v for k, v in kw.items() if k in ("lower", "upper")}))
        return dict(zip(got[0].tolist(), got[1].tolist()))
    # in all inputs: kept, with the minimum; twice in one input: still one input
    assert k32([k32_input(0xFFFFFF00), k32_input(0x200), k32_input(TOP)], "intersect")[ALL_T] == 0x200
    assert k32([k32_input(TOP)], "intersect")[ALL_T] == TOP
    twice = k32_input(7)
    twice = (np.append(twice[0], np.uint64(ALL_T)), np.append(twice[1], np.uint32(3)))
    assert k32([twice, k32_input(5)], "intersect")[ALL_T] == 3
    assert k32([k32_input(5), twice], "intersect")[ALL_T] == 3
    # in all inputs but one, whichever: absent; present with count 0 is absent
    for missing in range(3):
        inputs = [k32_input(None if i == missing else 10 + i) for i in range(3)]
        assert ALL_T not in k32(inputs, "intersect"), missing
    assert ALL_T not in k32([k32_input(4), k32_input(0), k32_input(4)], "intersect")
    assert ALL_T not in k32([k32_input(4), twice, k32_input(None), twice], "intersect")     # dead stays dead
    # the cut applies to it
    assert ALL_T not in k32([k32_input(4), k32_input(9)], "intersect", lower=5)
    assert ALL_T not in k32([k32_input(4000), k32_input(9000)], "intersect", upper=999)
    # subtract: in the first input only: kept (repeats summed and clipped); also in a later input: removed
    assert k32([k32_input(77), k32_input(None), k32_input(None)], "subtract")[ALL_T] == 77
    assert k32([twice, k32_input(None)], "subtract")[ALL_T] == 10
    big = (np.append(twice[0], np.uint64(ALL_T)), np.append(twice[1], np.uint32(0xFFFFFFFA)))
    assert k32([big], "subtract")[ALL_T] == TOP
    assert ALL_T not in k32([k32_input(77), k32_input(None), k32_input(1)], "subtract")
    assert ALL_T not in k32([k32_input(None), k32_input(77)], "subtract")
    assert k32([k32_input(77), k32_input(0)], "subtract")[ALL_T] == 77   # a zero count removes nothing
    # zero-count records in a later input of subtract remove nothing, in the first input they are not there
    keys = np.unique(random_keys(rng, 500, 31))[:400]
    first = (keys, rng.integers(0, 3, 400).astype(np.uint32))
    later = (keys[::-1].copy(), rng.integers(0, 2, 400).astype(np.uint32))
    want = set_model([first, later], "subtract")
    paths = [write_file(tmp_path / "z0.jf", *first, 31), write_file(tmp_path / "z1.jf", *later, 31)]
    assert same(set_files_on_gpu(paths, "subtract"), want) and 50 < want[0].size < 250
    assert same(set_files_on_gpu(paths, "intersect"), set_model([first, later], "intersect"))


@pytest.mark.gpu
def test_gpu_cuts_on_both_sides():
    rng = np.random.default_rng(94)
    keys = np.unique(random_keys(rng, 900, 31))[:800]
    inputs = [(keys, rng.integers(1, 40, 800).astype(np.uint32)),
              (keys[200:], rng.integers(1, 40, 600).astype(np.uint32))]
    cuts = ((1, TOP), (5, 20), (20, 20), (0, 7), (21, 20), (TOP, 0), (1, 1))
    for op in ("intersect", "subtract"):
        sizes = set()
        for lower, upper in cuts:
            want = set_model(inputs, op, lower=lower, upper=upper)
            assert same(set_records_on_gpu(inputs, op, lower=lower, upper=upper), want), (op, lower, upper)
            assert upper >= lower or want[0].size == 0
            sizes.add(want[0].size)
        assert len(sizes) >= 4
    # a sum counter, and one with T^32 on either side of the cut
    for lower, upper in cuts:
        want = tm.merged_model(inputs, "sum", lower=lower)
        want = (want[0][want[1] <= upper], want[1][want[1] <= upper])
        got = on_gpu(lambda c: [c.add_records(*inp) for inp in inputs], lower=lower, upper=upper)[:2]
        assert same(got, want), (lower, upper)
    k32 = (np.array([ALL_T, 5, ALL_T, 9], np.uint64), np.array([30, 2, 40, 71], np.uint32))
    for (lower, upper), kept in (((1, 70), [5, ALL_T]), ((1, 69), [5]), ((70, 70), [ALL_T]), ((71, TOP), [9])):
        got = on_gpu(lambda c: c.add_records(*k32), k=32, canonical=False, lower=lower, upper=upper)
        assert got[0].tolist() == kept, (lower, upper)
    # a counter fed from reads
    reads = tm.make_reads(94, 300)
    full = tm.counted_model(reads, 31)
    assert int(full[1].max()) > 6
    for lower, upper in ((1, TOP), (2, 6), (1, 1), (3, 2)):
        keep = (full[1] >= lower) & (full[1] <= upper)
        got = on_gpu(lambda c: c.add_bases(b"\n".join(reads)), lower=lower, upper=upper)[:2]
        assert same(got, (full[0][keep], full[1][keep])), (lower, upper)


@pytest.mark.gpu
def test_gpu_state_rules(tmp_path):
    rng = np.random.default_rng(95)
    keys = np.unique(random_keys(rng, 300, 31))[:256]
    counts = np.arange(1, 257, dtype=np.uint32)
    good = write_file(tmp_path / "good.jf", keys, counts, 31)
    half = write_file(tmp_path / "half.jf", keys[:128], counts[:128] + np.uint32(1000), 31)
    other_k = write_file(tmp_path / "k21.jf", keys & np.uint64((1 << 42) - 1), counts, 21)
    other_c = write_file(tmp_path / "noncanonical.jf", keys, counts, 31, canonical=False)
    empty = write_file(tmp_path / "empty.jf", [], [], 31)
    fastq = b"@r\n" + b"ACGT" * 10 + b"\n+\n" + b"I" * 40 + b"\n"

    def refused(call, code, named):
        with pytest.raises(kmlib.KmError) as e:
            call()
        assert e.value.code == code and all(word in str(e.value) for word in named), str(e.value)

    for op, other in (("intersect", "subtract"), ("subtract", "intersect")):
        c = kmlib.Counter(k=31, canonical=True)
        # refused before the first input: the counter is still nobody's
        refused(lambda: c.set_records(keys, counts, op=2), ARG, ["op 2"])
        refused(lambda: c.set_jf(good, op=-1), ARG, ["op -1"])
        refused(lambda: c.set_jf(other_k, op=op), ARG, [other_k, "k=21", "k=31"])
        refused(lambda: c.set_jf(other_c, op=op), ARG, [other_c, "canonical=0", "canonical=1"])
        refused(lambda: c.set_jf(str(tmp_path / "no_such.jf"), op=op), 1, ["no_such.jf"])
        assert c.set_jf(good, op=op) == 256 and c.stats()["distinct"] == 256
        for call, code, named in ((lambda: c.add_bases(b"ACGT" * 20), STATE, ["set operation", op]),
                                  (lambda: c.add_text(b">r\n" + b"ACGT" * 20 + b"\n", final=True), STATE, ["set operation"]),
                                  (lambda: c.add_fastq(fastq, final=True), STATE, ["set operation"]),
                                  (lambda: c.add_records(keys, counts), STATE, ["set operation"]),
                                  (lambda: c.add_jf(good, mode="max"), STATE, ["set operation"]),
                                  (lambda: c.set_records(keys, counts, op=other), STATE, [op, other]),
                                  (lambda: c.set_jf(good, op=other), STATE, [op, other]),
                                  (lambda: c.set_records(keys, counts, op=5), ARG, ["op 5"]),
                                  (lambda: c.set_jf(other_k, op=op), ARG, ["k=21"]),
                                  (lambda: c.set_jf(str(tmp_path / "no_such.jf"), op=op), 1, ["no_such.jf"]),
                                  (lambda: c.histo(), STATE, ["set operation", "finish"])):
            refused(call, code, named)
            assert c.stats()["distinct"] == 256
        # none of the refused calls was an input: the next valid one is the second, and the result says so
        assert c.set_jf(half, op=op) == 128
        assert c.merge_stats()["records_in"] == 256 + 128
        c.finish(1).close()
        got = c.records()
        order = np.argsort(got[0])
        want = set_model([(keys, counts), (keys[:128], counts[:128] + np.uint32(1000))], op)
        assert same((got[0][order], got[1][order]), want) and want[0].size == 128
        base, bins, hs = c.histo()                                      # after finish: the kept records
        assert hs["distinct"] == 128 and hs["total"] == int(want[1].sum(dtype=np.uint64))
        refused(lambda: c.set_jf(good, op=op), STATE, ["finished"])
        refused(lambda: c.set_records(keys, counts, op=op), STATE, ["finished"])
        c.close()
    # an empty input is an input: intersect then yields nothing, subtract loses nothing (or has nothing to lose)
    for feeds, op, size in (([good, empty], "intersect", 0), ([empty, good], "intersect", 0), ([good, empty], "subtract", 256),
                            ([empty, good], "subtract", 0), ([good, good], "intersect", 256)):
        assert set_files_on_gpu(feeds, op)[0].size == size, (feeds, op)
    none = (np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    assert set_records_on_gpu([(keys, counts), none], "intersect")[0].size == 0
    assert set_records_on_gpu([(keys, counts), none], "subtract")[0].size == 256
    # a counter that has taken text, FASTQ or sum / max records refuses the set calls and goes on as it was
    for take in (lambda c: c.add_bases(b"ACGT" * 20), lambda c: c.add_text(b">r\n" + b"ACGT" * 20 + b"\n", final=True),
                 lambda c: c.add_fastq(fastq, final=True), lambda c: c.add_records(keys, counts),
                 lambda c: c.add_jf(good, mode="max")):
        c = kmlib.Counter(k=31, canonical=True)
        take(c)
        before = c.stats()
        refused(lambda: c.set_records(keys, counts), STATE, ["text, FASTQ or sum / max records"])
        refused(lambda: c.set_jf(good, op="subtract"), STATE, ["text, FASTQ or sum / max records"])
        assert c.stats() == before
        c.add_records(keys[:1], counts[:1])                              # the next valid call works
        c.histo()
        c.finish().close()
        assert c.records()[0].size == before["distinct"] + (0 if before["kmers"] == 0 else 1)
        c.close()


@pytest.mark.gpu
def test_gpu_through_the_tool(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system")
    for name in (IANDI, ITD):
        shutil.copy(os.path.join(JF_DIR, name), tmp_path / name)

    def km(*args):
        res = subprocess.run([sys.executable, "-m", "km_amd"] + list(args), cwd=tmp_path, capture_output=True,
                             text=True, timeout=300, env=env)
        assert res.returncode == 0, res.stderr
        return res

    def tags(res):
        return dict(line[1:].split(":") for line in res.stderr.splitlines() if line.startswith("#"))
    inputs = [fixture(IANDI), fixture(ITD)]
    res = km("merge", "--min", "-U", "40", "-L", "3", "--jellyfish-order", "--dump", "d.txt", "-o", "out.jf", IANDI, ITD)
    want = set_model(inputs, "intersect", lower=3, upper=40)
    assert 0 < want[0].size < set_model(inputs, "intersect", lower=3)[0].size
    assert want[0].size < set_model(inputs, "intersect", upper=40)[0].size
    stats = tags(res)
    assert set(stats) == {"distinct", "slots", "n_grow", "records_in", "mode", "records_out"}
    assert (stats["mode"], int(stats["records_out"]), int(stats["distinct"])) == ("intersect", want[0].size, inputs[0][0].size)
    rec = jr.read_jf(str(tmp_path / "out.jf"))
    order = np.argsort(rec["keys"])
    assert (rec["k"], rec["canonical"]) == (31, True) and same((rec["keys"][order], rec["counts"][order]), want)
    assert rec["header"]["cmdline"] == ["km_amd", "merge", "-L", "3", "-U", "40", "--min", "--jellyfish-order", "-o",
                                        "out.jf", IANDI, ITD]
    m = rec["header"]["matrix1"]
    pos = tm.model_pos(rec["keys"], np.array(m["columns"], np.uint64), m["r"])
    assert np.array_equal(np.lexsort((rec["keys"], pos)), np.arange(rec["keys"].size))
    assert (tmp_path / "d.txt").read_text() == km("dump", "-c", "out.jf").stdout
    assert len((tmp_path / "d.txt").read_text().splitlines()) == want[0].size
    # subtract, the plain writer
    res = km("merge", "--subtract", "-o", "sub.jf", IANDI, ITD)
    want = set_model(inputs, "subtract")
    stats = tags(res)
    assert (stats["mode"], int(stats["records_out"])) == ("subtract", 919) and want[0].size == 919
    rec = jr.read_jf(str(tmp_path / "sub.jf"))
    assert same((rec["keys"], rec["counts"]), want)
    assert rec["header"]["cmdline"] == ["km_amd", "merge", "-L", "1", "--subtract", "-o", "sub.jf", IANDI, ITD]
    # -U on the modes that were there before; without it their stderr and their file are what they were
    res = km("merge", "-U", "12", "--max", "-o", "x.jf", IANDI, ITD)
    full = tm.merged_model(inputs, "max")
    rec = jr.read_jf(str(tmp_path / "x.jf"))
    assert same((rec["keys"], rec["counts"]), (full[0][full[1] <= 12], full[1][full[1] <= 12]))
    assert 0 < rec["keys"].size < full[0].size and "records_out" not in tags(res)
    res = km("merge", "-o", "m.jf", IANDI, ITD)
    want = tm.merged_model(inputs, "sum")
    stats = tags(res)
    assert [line.split(":")[0] for line in res.stderr.splitlines() if line.startswith("#")] == [
        "#distinct", "#slots", "#n_grow", "#records_in", "#mode"]
    assert (stats["mode"], int(stats["distinct"])) == ("sum", want[0].size)
    kc.write_records(str(tmp_path / "model.jf"), want[0], want[1], 31, True,
                     cmdline=["km_amd", "merge", "-L", "1", "-o", "m.jf", IANDI, ITD])
    assert (tmp_path / "m.jf").read_bytes() == (tmp_path / "model.jf").read_bytes()
    # the exclusions end with status 2 before anything runs
    bad = subprocess.run([sys.executable, "-m", "km_amd", "merge", "--min", "--subtract", IANDI, ITD], cwd=tmp_path,
                         capture_output=True, text=True, timeout=300, env=env)
    assert bad.returncode == 2 and "exclude" in bad.stderr
