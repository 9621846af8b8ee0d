"""The count histogram and the table statistics on the GPU (km_counter_histo, km_jf_histo, Counter.histo,
km_amd.count.histo_file, `python -m km_amd histo` / `stats`, `count --histo`, `merge --histo`).

Every comparison is exact.  The model is a numpy restatement of the definition in include/kmgpu.h and shares nothing
with the kernels: filter by the cut, np.bincount of bin(c), four reductions.  The definition is this project's reading
of `jellyfish histo` / `jellyfish stats`: no run of Jellyfish stands behind it.  The parts that need no GPU are in
tests/test_histo_cpu.py."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from km_amd import cli
from km_amd import count as kc
from km_amd import lib as kmlib
from oracle import jf_reader as jr
import test_count as tc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JF_DIR = os.path.join(HERE, "data", "jf")
FIXTURES = sorted(f for f in os.listdir(JF_DIR) if f.endswith(".jf"))
TOP = 0xFFFFFFFF
ALL_T = 0xFFFFFFFFFFFFFFFF
W = 4096                     # histo_kernel.h: HISTO_W, the bins a block holds in LDS

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the model
def model(counts, low=1, high=10000, increment=1, lower_count=1, upper_count=TOP):
    """-> (base, bins uint64[n_bins], stats) of the counts that pass the cut."""
    c = np.asarray(counts).astype(np.int64)
    c = c[(c >= max(lower_count, 1)) & (c <= upper_count)]
    base = (1 if increment >= low else low - increment) if low > 1 else 1
    ceil = high + increment
    n_bins = (ceil + increment - base) // increment
    b = np.where(c < base, 0, np.where(c > ceil, n_bins - 1, (np.maximum(c, base) - base) // increment))
    bins = np.bincount(b, minlength=n_bins).astype(np.uint64)
    stats = {"unique": int((c == 1).sum()), "distinct": int(c.size), "total": int(c.sum()),
             "max_count": int(c.max()) if c.size else 0}
    return base, bins, stats


def agree(got, want):
    """got: what Counter.histo / histo_file return (a file's stats carry k and n_records too)."""
    stats = {key: got[2][key] for key in ("unique", "distinct", "total", "max_count")}
    return got[0] == want[0] and got[1].dtype == np.uint64 and np.array_equal(got[1], want[1]) and stats == want[2]


def write_file(path, keys, counts, k, canonical=True, counter_len=4):
    """A `binary/sorted`-framed file with records in the order given: ceil(2k / 8) key bytes, counter_len count
    bytes."""
    keys = np.asarray(keys, np.uint64)
    counts = np.asarray(counts, np.uint32)
    assert counter_len == 4 or not counts.size or int(counts.max()) < 1 << (8 * counter_len)
    header = {"alignment": 8, "canonical": bool(canonical), "cmdline": ["test_histo"], "counter_len": counter_len,
              "format": "binary/sorted", "key_len": 2 * k, "size": 16, "val_len": 8 * counter_len}
    text = json.dumps(header, separators=(",", ":")).encode("ascii")
    text += b"\0" * ((-(9 + len(text))) % 8)
    kb = (2 * k + 7) // 8
    rec = np.zeros((keys.size, kb + counter_len), np.uint8)
    for b in range(kb):
        rec[:, b] = ((keys >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8)
    for b in range(counter_len):
        rec[:, kb + b] = ((counts >> np.uint32(8 * b)) & np.uint32(0xFF)).astype(np.uint8)
    with open(path, "wb") as fh:
        fh.write(b"%09d" % len(text) + text + rec.tobytes())
    return str(path)


def distinct_keys(rng, n, k=31):
    keys = np.unique(rng.integers(0, (1 << (2 * k)) - 1, n + n // 8 + 16, dtype=np.uint64))
    assert keys.size >= n
    return rng.permutation(keys)[:n]


def three_ways(tmp_path, keys, counts, variants, k=31):
    """Distinct keys with counts > 0 through the three kernels — the records of a file, the table of a live counter,
    the kept counts of a finished one — each against the model, for every dict of arguments in `variants`."""
    path = write_file(tmp_path / "three.jf", keys, counts, k)
    c = kmlib.Counter(k=k, canonical=True)
    try:
        c.add_records(keys, counts)
        for kw in variants:
            want = model(counts, **kw)
            assert agree(kc.histo_file(path, **kw), want), ("file", kw)
            assert agree(c.histo(**kw), want), ("table", kw)
        c.finish(1).close()
        for kw in variants:
            assert agree(c.histo(**kw), model(counts, **kw)), ("counts", kw)
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def catalog_reads():
    return tuple(tc.make_reads(90, 20_000))


def as_fasta(reads):
    return b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads))


# ------------------------------------------------------------------ files
@functools.lru_cache(maxsize=None)
def fixture_counts(name):
    return jr.read_jf(os.path.join(JF_DIR, name))["counts"]


LAYOUTS = [{}, {"high": 100}, {"low": 50, "high": 400, "increment": 25}]
CUTS = [{}, {"lower_count": 2}, {"lower_count": 5}, {"upper_count": 100}, {"lower_count": 5, "upper_count": 100}]


@pytest.mark.parametrize("name", FIXTURES)
def test_the_shipped_files(name, monkeypatch):
    path = os.path.join(JF_DIR, name)
    counts = fixture_counts(name)
    assert counts.size >= 200
    got = {}
    for stage in (None, "256"):                                         # 21 records per piece against one piece
        if stage:
            monkeypatch.setenv("KM_COUNT_STAGE_BYTES", stage)
        for i, lay in enumerate(LAYOUTS):
            for j, cut in enumerate(CUTS):
                res = kc.histo_file(path, **lay, **cut)
                assert agree(res, model(counts, **lay, **cut)), (stage, lay, cut)
                assert (res[2]["k"], res[2]["n_records"]) == (31, counts.size)
                got[stage, i, j] = res
    assert all(np.array_equal(got[None, i, j][1], got["256", i, j][1]) for i in range(3) for j in range(5))
    assert kmlib.histo_kernel_ms() > 0


def test_the_last_bin_collects():
    counts = np.concatenate([fixture_counts(f) for f in FIXTURES])
    assert int(counts.max()) > 8000                                     # far above -h 100
    name = max(FIXTURES, key=lambda f: int(fixture_counts(f).max()))
    base, bins, stats = kc.histo_file(os.path.join(JF_DIR, name), high=100)
    c = fixture_counts(name)
    assert bins.size == 101 and int(bins[-1]) == int((c >= 101).sum()) > 0 and stats["max_count"] == int(c.max())


def test_synthetic_files(tmp_path):
    rng = np.random.default_rng(91)
    # k = 21: 6 key bytes, 1 and 2 count bytes (7- and 8-byte records, read by bytes)
    keys = distinct_keys(rng, 1013, 21)
    for cb, top in ((1, 256), (2, 65536)):
        counts = rng.integers(0, top, keys.size).astype(np.uint32)
        counts[:4] = (1, top - 1, 2, 0)
        p = write_file(tmp_path / ("k21_%d.jf" % cb), keys, counts, 21, counter_len=cb)
        assert kmlib.jf_file_info(p)["key_bytes"] == 6 and kmlib.jf_file_info(p)["counter_len"] == cb
        for kw in ({}, {"high": 100}, {"low": 50, "high": 400, "increment": 25, "lower_count": 3}):
            res = kc.histo_file(p, **kw)
            assert agree(res, model(counts, **kw)), (cb, kw)
            assert (res[2]["k"], res[2]["n_records"]) == (21, 1013)
    # k = 32 with the key ~0: keys are not decoded, it is a record like any other
    keys = np.concatenate([distinct_keys(rng, 300, 32), np.array([ALL_T], np.uint64)])
    counts = rng.integers(1, 50, keys.size).astype(np.uint32)
    counts[-1] = 0xFFFFFF00
    p = write_file(tmp_path / "k32.jf", keys, counts, 32, canonical=False)
    res = kc.histo_file(p)
    assert agree(res, model(counts)) and res[2]["max_count"] == 0xFFFFFF00 and int(res[1][-1]) == 1
    # records with count 0 are no keys, whatever lower_count says; 401 records: a tail of one behind 100 quads
    keys = distinct_keys(rng, 401)
    counts = rng.integers(1, 100, keys.size).astype(np.uint32)
    counts[::3] = 0
    p = write_file(tmp_path / "zeros.jf", keys, counts, 31)
    for lower in (0, 1, 2):
        res = kc.histo_file(p, lower_count=lower)
        assert agree(res, model(counts, lower_count=lower)) and res[2]["n_records"] == 401
    assert kc.histo_file(p, lower_count=0)[2]["distinct"] == 401 - 134
    # 1, 2 and 3 records: only the tail
    for n in (1, 2, 3):
        p = write_file(tmp_path / ("n%d.jf" % n), keys[:n], [7, 1, 9][:n], 31)
        assert agree(kc.histo_file(p), model([7, 1, 9][:n]))
    # a file without records: zeros without a launch
    p = write_file(tmp_path / "none.jf", [], [], 31)
    res = kc.histo_file(p, high=50)
    assert agree(res, model([], high=50)) and res[1].size == 51 and res[2]["n_records"] == 0
    assert kmlib.histo_kernel_ms() == 0.0


@pytest.mark.parametrize("k, counter_len, sizes", [(21, 2, (32, 96, 97)), (31, 4, (21, 63, 64))])
def test_where_a_piece_ends_with_the_buffer(tmp_path, monkeypatch, k, counter_len, sizes):
    """256-byte staging.  k = 21 with 2 count bytes: records of 8 bytes, 32 to a piece, which fills the buffer to its
    last byte; k = 31: records of 12 bytes, 21 to a piece, 252 of the 256 bytes.  Files of one full piece, of three,
    and of three and one record more, through every user of the shared path: jf_histo of the file, add_jf of it twice
    into a counter, histo(), finish(), write_jf, jf_histo of what was written; on a pool stream and on the caller's."""
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "256")
    rng = np.random.default_rng(94)
    assert 256 // ((2 * k + 7) // 8 + counter_len) == sizes[0]
    stream = kmlib.stream_create()
    try:
        for n in sizes:
            keys = distinct_keys(rng, n, k)
            counts = rng.integers(1, 65536, n).astype(np.uint32)
            counts[0], counts[-1] = 1, 65535
            order = np.argsort(keys, kind="stable")
            twice = (keys[order], counts[order] * np.uint32(2))
            path = write_file(tmp_path / ("in_%d.jf" % n), keys, counts, k, canonical=False, counter_len=counter_len)
            got = {}
            for st in (None, stream):
                first = kmlib.jf_histo(path, stream=st)
                assert agree(first, model(counts)) and (first[2]["k"], first[2]["n_records"]) == (k, n), (n, st)
                out = str(tmp_path / ("out_%d.jf" % n))
                c = kmlib.Counter(k=k, canonical=False)
                try:
                    assert c.add_jf(path) == n and c.add_jf(path) == n
                    assert agree(c.histo(), model(twice[1])), (n, st)
                    c.finish().close()
                    c.write_jf(out)
                    assert tc.same(tc.sorted_records(c), twice), (n, st)
                finally:
                    c.close()
                second = kmlib.jf_histo(out, stream=st)
                assert agree(second, model(twice[1])) and (second[2]["k"], second[2]["n_records"]) == (k, n), (n, st)
                got[st] = (first, second)
            for a, b in zip(got[None], got[stream]):
                assert np.array_equal(a[1], b[1]) and a[2] == b[2], n
    finally:
        kmlib.stream_destroy(stream)


# ------------------------------------------------------------------ hot bins, cold bins, the edge of the LDS image
@pytest.mark.parametrize("rounds", [None, "1", "2", "8"])                 # None: the depth compiled in, 0
def test_hot_and_cold_bins_at_any_number_of_rounds(tmp_path, monkeypatch, rounds):
    if rounds is not None:
        monkeypatch.setenv("KM_HISTO_ROUNDS", rounds)
    rng = np.random.default_rng(92)
    keys = distinct_keys(rng, 70_000)
    hot = np.ones(keys.size, np.uint32)                                 # every lane of every wave on one bin
    three_ways(tmp_path, keys, hot, [{}, {"lower_count": 2}])
    cold = (np.arange(keys.size) % 64 * 37 + 3).astype(np.uint32)       # no two lanes of a wave share a bin
    assert np.unique(cold).size == 64
    three_ways(tmp_path, keys, cold, [{}, {"increment": 37}, {"low": 0, "high": 0, "increment": 5}])
    mixed = rng.choice(np.array([1, 1, 1, 1, 2, 2, 3, 40, 5000, 20000, TOP], np.uint32), keys.size)
    three_ways(tmp_path, keys, mixed, [{}, {"high": 100}, {"upper_count": 5000}])


def test_the_edge_of_the_lds_image(tmp_path):
    rng = np.random.default_rng(93)
    edge = np.array([1, 2, W - 2, W - 1, W, W + 1, W + 2, 2 * W, TOP - 1, TOP], np.uint32)
    counts = np.repeat(edge, np.arange(1, edge.size + 1) * 7)           # every value its own multiplicity
    keys = distinct_keys(rng, counts.size)
    variants = [{"high": high} for high in (W - 2, W - 1, W)]           # n_bins = W - 1, W, W + 1
    assert [kmlib.histo_layout(1, v["high"], 1)[1] for v in variants] == [W - 1, W, W + 1]
    variants += [{"high": 3 * W}, {"high": 2 * W, "increment": 2}, {"low": W, "high": 2 * W, "increment": 1}]
    three_ways(tmp_path, keys, counts, variants)
    one = [{"low": 0, "high": 0, "increment": 5}, {"low": 0, "high": 0, "increment": 2 ** 40}]
    assert [kmlib.histo_layout(v["low"], v["high"], v["increment"]) for v in one] == [(1, 1), (1, 1)]   # n_bins = 1
    three_ways(tmp_path, keys, counts, one)
    three_ways(tmp_path, keys, counts, [{"low": 2 ** 33, "high": 2 ** 34, "increment": 2 ** 20}])   # every count below base


# ------------------------------------------------------------------ a live counter
@pytest.mark.parametrize("k, canonical", [(31, True), (5, False)])
def test_a_live_counter(k, canonical):
    reads = catalog_reads()
    first, second = as_fasta(reads[:12_000]), as_fasta(reads[12_000:])
    so_far = tc.model(b"\n".join(reads[:12_000]), k, canonical)[1]
    whole_keys, whole = tc.model(b"\n".join(reads), k, canonical)
    # histo() before finish enqueues what is staged, as stats() does: WHEN the table doubles (slots, n_grow) follows
    # the pieces, what it holds does not.  `plain` is never asked anything, `asked` calls stats() where c calls histo().
    content = ("bases", "kmers", "distinct")
    plain = kmlib.Counter(k=k, canonical=canonical)
    asked = kmlib.Counter(k=k, canonical=canonical)
    c = kmlib.Counter(k=k, canonical=canonical)
    try:
        for ctr in (plain, asked, c):
            assert ctr.add_text(first, final=True) == len(first)
        asked.stats()
        assert agree(c.histo(), model(so_far))
        assert agree(c.histo(lower_count=2), model(so_far, lower_count=2))
        for ctr in (plain, asked, c):
            assert ctr.add_text(second, final=True) == len(second)
        assert agree(c.histo(), model(whole))
        assert agree(c.histo(high=100, lower_count=2), model(whole, high=100, lower_count=2))
        assert c.stats() == asked.stats()
        assert [c.stats()[key] for key in content] == [plain.stats()[key] for key in content]
        assert c.stats()["distinct"] == whole.size and c.stats()["kmers"] == int(whole.sum(dtype=np.uint64))
        db, db_plain = c.finish(lower_count=2), plain.finish(lower_count=2)
        try:
            a, b = db.info, db_plain.info
            assert (a.n_records, a.n_slots, a.n_groups) == (b.n_records, b.n_slots, b.n_groups)
            assert a.n_records == int((whole >= 2).sum())
            assert np.array_equal(db.query(whole_keys), db_plain.query(whole_keys))
            assert np.array_equal(db.query(whole_keys), np.where(whole >= 2, whole, 0))
        finally:
            db.close()
            db_plain.close()
        assert tc.same(tc.sorted_records(c), tc.sorted_records(plain))
        assert tc.same(tc.sorted_records(c), tc.cut(whole_keys, whole, 2)) and c.stats() == asked.stats()
        assert agree(c.histo(), model(whole, lower_count=2))             # after finish: the kept records
        assert agree(c.histo(lower_count=5, high=100), model(whole, lower_count=5, high=100))
        assert agree(c.histo(lower_count=1), model(whole, lower_count=2))
    finally:
        c.close()
        plain.close()
        asked.close()


def test_all_t_of_a_k32_table_is_counted_once():
    rng = np.random.default_rng(94)
    data = b"T" * 40 + b"\n" + b"\n".join(tc.random_bases(rng, 90).tobytes() for _ in range(50)) + b"\n" + b"T" * 33
    keys, counts = tc.model(data, 32, False)
    assert int(keys[-1]) == ALL_T and int(counts[-1]) == 11
    c = kmlib.Counter(k=32, canonical=False)
    try:
        c.add_bases(data)
        for kw in ({}, {"lower_count": 2}, {"lower_count": 12}, {"upper_count": 10}, {"high": 5}):
            assert agree(c.histo(**kw), model(counts, **kw)), kw
        assert c.histo()[2]["max_count"] == 11 and int(c.histo()[1][10]) == 1
        c.finish(1).close()
        for kw in ({}, {"lower_count": 2}, {"lower_count": 12}, {"upper_count": 10}, {"high": 5}):
            assert agree(c.histo(**kw), model(counts, **kw)), kw
    finally:
        c.close()


def test_a_grown_counter_and_an_empty_one():
    rng = np.random.default_rng(95)
    keys = distinct_keys(rng, 70_000)
    counts = rng.integers(1, 12_000, keys.size).astype(np.uint32)
    c = kmlib.Counter(k=31, canonical=True)                              # 65 536 slots: has to grow
    try:
        c.add_records(keys, counts)
        assert agree(c.histo(), model(counts)) and c.stats()["n_grow"] >= 1
        c.add_records(keys[:100], counts[:100])                          # the counter takes more afterwards
        more = counts.astype(np.int64)
        more[:100] *= 2
        assert agree(c.histo(), model(more))
    finally:
        c.close()
    c = kmlib.Counter(k=31, canonical=True)
    try:
        assert agree(c.histo(high=7), model([], high=7))
        c.finish(1).close()
        assert agree(c.histo(high=7), model([], high=7))
        assert c.histo()[1].size == 10001
    finally:
        c.close()


def test_errors_on_a_counter():
    c = kmlib.Counter(k=31, canonical=True)
    try:
        data = b"ACGT" * 20
        counts = tc.model(data, 31, True)[1]
        c.add_bases(data)
        for kw, code in (({"increment": 0}, 4), ({"low": 3, "high": 2}, 4), ({"high": 2 ** 40}, 4)):
            with pytest.raises(kmlib.KmError) as e:
                c.histo(**kw)
            assert e.value.code == code
        bins = np.zeros(5, np.uint64)
        assert c._lib.km_counter_histo(c._c, 1, 10000, 1, 1, TOP, kmlib.ptr(bins), 5, None) == 8    # KM_E_CAPACITY
        st = kmlib.HistoStats()
        assert c._lib.km_counter_histo(c._c, 1, 10000, 1, 1, TOP, None, 0, st) == 0                 # bins may be NULL
        assert (st.distinct, st.total, st.max_count) == (counts.size, 50, int(counts.max()))
        assert c._lib.km_counter_histo(c._c, 1, 4, 1, 1, TOP, kmlib.ptr(bins), 5, None) == 0        # and so may stats
        assert bins.tolist() == model(counts, high=4)[1].tolist() == [0, 0, 0, 0, counts.size]
        assert agree(c.histo(), model(counts))
    finally:
        c.close()
    c = kmlib.Counter(k=31, canonical=True)                              # a FASTQ error stays with the counter
    try:
        c.add_fastq(b"@r0\nACGTACGT\n+\nIIII\n", final=True)
        for _ in range(2):
            with pytest.raises(kmlib.KmError) as e:
                c.histo()
            assert e.value.code == 2 and "quality line" in str(e.value)
    finally:
        c.close()


# ------------------------------------------------------------------ statistics
def test_statistics_beyond_32_bits():
    rng = np.random.default_rng(96)
    keys = distinct_keys(rng, 4096 + 3)
    counts = np.full(keys.size, 1 << 31, np.uint32)
    counts[-3:] = (1, 1, TOP)
    c = kmlib.Counter(k=31, canonical=True)
    try:
        c.add_records(keys, counts)
        for after in (False, True):
            if after:
                c.finish(1).close()
            _, bins, st = c.histo()
            assert st == {"unique": 2, "distinct": 4099, "total": 4096 * 2 ** 31 + 2 + TOP, "max_count": TOP}
            assert st["total"] > 2 ** 43 and int(bins[-1]) == 4097 and int(bins[0]) == 2
            st = c.histo(lower_count=2)[2]                               # the cut excludes count 1: no unique key
            assert st == {"unique": 0, "distinct": 4097, "total": 4096 * 2 ** 31 + TOP, "max_count": TOP}
            st = c.histo(upper_count=TOP - 1)[2]
            assert st == {"unique": 2, "distinct": 4098, "total": 4096 * 2 ** 31 + 2, "max_count": 1 << 31}
            assert c.histo(lower_count=2, upper_count=5)[2] == {"unique": 0, "distinct": 0, "total": 0, "max_count": 0}
    finally:
        c.close()


# ------------------------------------------------------------------ command line
def test_count_and_merge_write_the_histogram_of_their_file(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _, reads = tc.itd_reads(depth=30)
    with open("reads.fa", "wb") as fh:
        fh.write(as_fasta(reads))
    cli.main(["count", "-m", "31", "-C", "-L", "2", "--histo", "h.txt", "-o", "out.jf", "reads.fa"])
    cli.main(["count", "-m", "31", "-C", "-L", "2", "-o", "plain.jf", "reads.fa"])
    capsys.readouterr()
    kept = jr.read_jf("out.jf")["counts"]
    want = kc.format_histo(1, 1, model(kept)[1])
    assert open("h.txt").read() == want and want.count("\n") > 5 and not want.startswith("1 ")
    plain = jr.read_jf("plain.jf")                                       # without the option: the same records
    assert np.array_equal(plain["keys"], jr.read_jf("out.jf")["keys"]) and np.array_equal(plain["counts"], kept)
    assert kept.size > 100 and not os.path.exists("mer_counts.jf")
    # the tool itself, as a process: the same bytes on its standard output
    env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, "-m", "km_amd", "histo", "out.jf"], cwd=tmp_path, capture_output=True,
                         timeout=300, env=env)
    assert res.returncode == 0, res.stderr
    assert res.stdout == want.encode()
    cli.main(["histo", "-o", "again.txt", "out.jf"])
    assert open("again.txt").read() == want
    # merge likewise
    paths = [os.path.join(JF_DIR, f) for f in FIXTURES[:2]]
    cli.main(["merge", "-L", "3", "--histo", "mh.txt", "-o", "m.jf"] + paths)
    capsys.readouterr()
    cli.main(["histo", "m.jf"])
    printed = capsys.readouterr().out
    merged = jr.read_jf("m.jf")["counts"]
    assert open("mh.txt").read() == printed == kc.format_histo(1, 1, model(merged)[1]) and int(merged.min()) >= 3


def test_stats_and_full_histogram_of_a_shipped_file(tmp_path, capsys):
    path = os.path.join(JF_DIR, FIXTURES[0])
    counts = fixture_counts(FIXTURES[0])
    cli.main(["stats", path])
    st = model(counts)[2]
    assert capsys.readouterr().out == "Unique:    %d\nDistinct:  %d\nTotal:     %d\nMax_count: %d\n" % (
        st["unique"], st["distinct"], st["total"], st["max_count"])
    cli.main(["stats", "-L", "5", "-U", "100", "-o", str(tmp_path / "s.txt"), path])
    st = model(counts, lower_count=5, upper_count=100)[2]
    assert open(tmp_path / "s.txt").read() == "Unique:    0\nDistinct:  %d\nTotal:     %d\nMax_count: %d\n" % (
        st["distinct"], st["total"], st["max_count"]) and capsys.readouterr().out == ""
    cli.main(["histo", "-h", "20", "-l", "4", "-i", "2", "-f", path])
    lines = capsys.readouterr().out.splitlines()
    base, bins, _ = model(counts, low=4, high=20, increment=2)
    assert lines == ["%d %d" % (base + 2 * i, n) for i, n in enumerate(bins.tolist())] and len(lines) == 11
    cli.main(["histo", "-h", "20", "-l", "4", "-i", "2", path])
    assert capsys.readouterr().out.splitlines() == [ln for ln in lines if not ln.endswith(" 0")]
