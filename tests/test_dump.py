"""`dump` and `query` on the GPU (km_dump_text, km_jf_dump, km_counter_dump, kmjf_query_text, km_amd.count.dump_file /
query_file, `python -m km_amd dump` / `query`, `count --dump`, `merge --dump`).

Every comparison is byte-exact against the model of tests/test_dump_cpu.py, which is written from the rule of
include/kmgpu.h alone and shares nothing with csrc/dump_text.h.  The rule is this project's reading of `jellyfish dump`
and `jellyfish query`: no run of Jellyfish stands behind it.  The parts that need no GPU are in tests/test_dump_cpu.py."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from km_amd import cli
from km_amd import common
from km_amd import count as kc
from km_amd import kmer as km
from km_amd import lib as kmlib
from oracle import jf_reader as jr
from oracle import km_oracle as ko
import test_count as tc
import test_dump_cpu as td

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JF_DIR = os.path.join(HERE, "data", "jf")
CATALOG = os.path.join(HERE, "data", "catalog", "GRCh38")
FIXTURES = sorted(f for f in os.listdir(JF_DIR) if f.endswith(".jf"))
NPM1 = os.path.join(JF_DIR, "02H025_NPM1.jf")
TOP = 0xFFFFFFFF
ALL_T = 0xFFFFFFFFFFFFFFFF
KM_E_IO, KM_E_STATE, KM_E_CAPACITY = 1, 7, 8
T = 256                      # dump_kernel.h: DUMP_TILE, the records of one block
FORMATS = td.FORMATS
model = td.model

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers
def distinct_keys(rng, n, k):
    """n distinct keys of k bases in a seeded random order (every key of a small k when n asks for more)."""
    space = 1 << (2 * k)
    if space <= 4 * n:
        keys = rng.permutation(np.arange(space, dtype=np.uint64))
        assert keys.size >= n
        return keys[:n]
    keys = np.unique(rng.integers(0, space - 1, n + n // 8 + 16, dtype=np.uint64))
    assert keys.size >= n
    return rng.permutation(keys)[:n]


def digit_cycle(n, start=0):
    """Counts that cycle through the ten digit lengths 1..10, so lines, and with them tile offsets, take every length
    and every residue mod 16: 7, 42, 420, .., 4 200 000 000."""
    by_len = np.array([7, 42, 420, 4200, 42000, 420000, 4200000, 42000000, 420000000, 4200000000], np.uint64)
    return by_len[(np.arange(n) + start) % 10].astype(np.uint32)


def write_file(path, keys, counts, k, canonical=True, counter_len=4):
    """A `binary/sorted`-framed file with records in the order given: ceil(2k / 8) key bytes, counter_len count
    bytes."""
    keys = np.asarray(keys, np.uint64)
    counts = np.asarray(counts, np.uint32)
    assert counter_len == 4 or not counts.size or int(counts.max()) < 1 << (8 * counter_len)
    header = {"alignment": 8, "canonical": bool(canonical), "cmdline": ["test_dump"], "counter_len": counter_len,
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


def through_pipe(call):
    """call(write end as a file object) while a thread reads the pipe to its end -> (what call returned, the bytes)."""
    r, w = os.pipe()
    got = []
    reader = threading.Thread(target=lambda: got.append(os.fdopen(r, "rb").read()))
    reader.start()
    try:
        with os.fdopen(w, "wb") as fh:
            res = call(fh)
    finally:
        reader.join()
    return res, got[0]


def dump_raw(keys, counts, k, fmt, lower, upper, cap, guard=64):
    """km_dump_text itself with a buffer of `cap` bytes and `guard` bytes of 0xA5 behind it -> (code, len, buffer)."""
    keys = np.ascontiguousarray(keys, np.uint64)
    counts = np.ascontiguousarray(counts, np.uint32)
    buf = np.full(cap + guard, 0xA5, np.uint8)
    ln = C.c_uint64()
    rc = kmlib.load().km_dump_text(0, kmlib.ptr(keys), kmlib.ptr(counts), keys.size, k, kmlib.DUMP_FORMATS[fmt], lower,
                                   upper, kmlib.ptr(buf), cap, C.byref(ln), None)
    return rc, int(ln.value), buf


# ------------------------------------------------------------------ shapes through dump_text
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 10 * T + 3])
def test_shapes(n):
    rng = np.random.default_rng(1000 + n)
    keys = distinct_keys(rng, n, 31)
    counts = digit_cycle(n, start=n)
    for fmt in FORMATS:
        assert kmlib.dump_text(keys, counts, 31, fmt) == model(keys, counts, 31, fmt), fmt
    if n:
        assert kmlib.dump_kernel_ms() > 0


@pytest.mark.parametrize("k", range(2, 33))
def test_every_k(k):
    rng = np.random.default_rng(k)
    n = T + 1
    top = (1 << (2 * k)) - 1
    if (1 << (2 * k)) >= n:
        keys = distinct_keys(rng, n, k)
        keys[np.flatnonzero((keys == 0) | (keys == top))] = 1       # the two named keys appear once each, below
    else:
        keys = rng.integers(0, top + 1, n, dtype=np.uint64)         # (k < 5: fewer keys than records; they repeat)
    keys[3], keys[T] = 0, top                                       # in the first tile, and alone in the second
    counts = digit_cycle(n, start=k)
    for fmt in FORMATS:
        assert kmlib.dump_text(keys, counts, k, fmt) == model(keys, counts, k, fmt), fmt


def test_the_count_filter():
    rng = np.random.default_rng(5)
    n = 3 * T + 7
    keys = distinct_keys(rng, n, 31)
    for name, counts, lower, upper in [
        ("the middle tile dropped", np.where((np.arange(n) // T) == 1, 5, digit_cycle(n)), 6, TOP),
        ("the first tile dropped", np.where(np.arange(n) < T, 3, 1000 + np.arange(n)), 4, TOP),
        ("the last record dropped", np.where(np.arange(n) == n - 1, 99, 12), 0, 50),
        ("only the last record kept", np.where(np.arange(n) == n - 1, 99, 12), 50, TOP),
        ("everything dropped", digit_cycle(n), 4200000001, TOP),
        ("lower above upper", digit_cycle(n), 43, 42),
        ("one value kept", digit_cycle(n), 42, 42),
    ]:
        counts = np.asarray(counts, np.uint32)
        for fmt in FORMATS:
            want = model(keys, counts, 31, fmt, lower, upper)
            assert kmlib.dump_text(keys, counts, 31, fmt, lower, upper) == want, (name, fmt)
        if name in ("everything dropped", "lower above upper"):
            assert want == b""
    # zero counts: printed by default, dropped from lower = 1 on
    counts = np.where(np.arange(n) % 3 == 0, 0, digit_cycle(n)).astype(np.uint32)
    with_zeros = kmlib.dump_text(keys, counts, 31, "column")
    assert with_zeros == model(keys, counts, 31, "column") and with_zeros.count(b" 0\n") == (n + 2) // 3
    assert kmlib.dump_text(keys, counts, 31, "column", 1) == model(keys, counts, 31, "column", 1)
    assert kmlib.dump_text(keys, counts, 31, "column", 1).count(b" 0\n") == 0


def test_the_filter_through_a_file(tmp_path):
    """records_out and bytes_out of a dump that keeps nothing, and of one that keeps a part."""
    rng = np.random.default_rng(6)
    n = 2 * T + 5
    keys, counts = distinct_keys(rng, n, 31), digit_cycle(n)
    path = write_file(tmp_path / "f.jf", keys, counts, 31)
    out = tmp_path / "out.txt"
    st = kc.dump_file(path, out=str(out), fmt="column", lower_count=4200000001)
    assert out.read_bytes() == b"" and (st["records_in"], st["records_out"], st["bytes_out"]) == (n, 0, 0)
    st = kc.dump_file(path, out=str(out), fmt="column", lower_count=5, upper_count=4)
    assert out.read_bytes() == b"" and (st["records_in"], st["records_out"], st["bytes_out"]) == (n, 0, 0)
    st = kc.dump_file(path, out=str(out), fmt="tab", lower_count=42, upper_count=42000)
    want = model(keys, counts, 31, "tab", 42, 42000)
    kept = int(((counts >= 42) & (counts <= 42000)).sum())
    assert out.read_bytes() == want and (st["records_in"], st["records_out"], st["bytes_out"]) == (n, kept, len(want))
    empty = write_file(tmp_path / "empty.jf", keys[:0], counts[:0], 31)
    st = kc.dump_file(empty, out=str(out))
    assert out.read_bytes() == b"" and (st["records_in"], st["records_out"], st["pieces"]) == (0, 0, 0)


def test_capacity():
    rng = np.random.default_rng(8)
    n = T + 9
    keys, counts = distinct_keys(rng, n, 31), digit_cycle(n)
    for fmt in FORMATS:
        want = model(keys, counts, 31, fmt)
        rc, ln, buf = dump_raw(keys, counts, 31, fmt, 0, TOP, len(want) - 1)
        assert rc == KM_E_CAPACITY and ln == len(want)
        msg = kmlib.load().km_last_error().decode()
        assert str(len(want)) in msg and str(len(want) - 1) in msg
        assert (buf == 0xA5).all()                                   # nothing was written
        rc, ln, buf = dump_raw(keys, counts, 31, fmt, 0, TOP, len(want))
        assert rc == 0 and ln == len(want) and buf[:ln].tobytes() == want
        assert (buf[ln:] == 0xA5).all()                              # the guard bytes behind the buffer
        rc, ln, buf = dump_raw(keys, counts, 31, fmt, 0, TOP, len(want) + 100)
        assert rc == 0 and ln == len(want) and buf[:ln].tobytes() == want and (buf[ln:] == 0xA5).all()
    ln = C.c_uint64()                                                # out == NULL asks for the length alone
    assert kmlib.load().km_dump_text(0, kmlib.ptr(keys), kmlib.ptr(counts), n, 31, 1, 0, TOP, None, 0, C.byref(ln), None) == 0
    assert ln.value == len(model(keys, counts, 31, "column"))


# ------------------------------------------------------------------ files
@pytest.mark.parametrize("counter_len", [1, 2, 4])
@pytest.mark.parametrize("k", [4, 17, 31])
def test_files_of_every_record_width(tmp_path, monkeypatch, k, counter_len):
    """key_bytes 1, 5, 8 and counter_len 1, 2, 4, records in shuffled order (k = 4 has 256 keys: they repeat, which a
    dump does not mind), at three staging sizes.  256: a handful of records per piece.  4096: pieces of less than a
    tile.  One byte less than 6 000 records: pieces of several tiles and a part, ending mid-tile.  In all three the
    text cap, bytes / (k + 13), decides the piece size, not the input buffer."""
    rng = np.random.default_rng(100 * k + counter_len)
    n = 4000
    keys = rng.permutation(np.resize(distinct_keys(rng, min(n, 1 << (2 * k)), k), n))
    counts = (digit_cycle(n) % (1 << (8 * counter_len))).astype(np.uint32) if counter_len < 4 else digit_cycle(n)
    counts[5] = 0
    path = write_file(tmp_path / "in.jf", keys, counts, k, canonical=False, counter_len=counter_len)
    rec = (2 * k + 7) // 8 + counter_len
    out = tmp_path / "out.txt"
    for i, stage in enumerate((256, 4096, 6000 * rec - 1)):
        monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))
        per = stage // (k + 13)
        assert per < stage // rec and per % T != 0 and (per > 2 * T) == (i == 2)
        fmt = FORMATS[(i + k) % 3]
        want = model(keys, counts, k, fmt)
        st = kc.dump_file(path, out=str(out), fmt=fmt)
        assert out.read_bytes() == want, (stage, fmt)
        assert st == {"records_in": n, "records_out": n, "bytes_out": len(want), "pieces": -(-n // per)}
        assert st["pieces"] > 1
        st, got = through_pipe(lambda fh: kc.dump_file(path, out=fh, fmt=fmt, lower_count=1))
        want = model(keys, counts, k, fmt, 1)
        assert got == want and (st["records_out"], st["bytes_out"]) == (int((counts >= 1).sum()), len(want))
        assert 0 < st["records_out"] < n


def test_a_file_object_is_flushed_first(tmp_path):
    keys, counts = np.arange(10, dtype=np.uint64), np.arange(10, dtype=np.uint32)
    path = write_file(tmp_path / "in.jf", keys, counts, 31)
    with open(tmp_path / "out.txt", "w") as fh:
        fh.write("# written by Python first\n")
        kc.dump_file(path, out=fh, fmt="column")
    assert (tmp_path / "out.txt").read_bytes() == b"# written by Python first\n" + model(keys, counts, 31, "column")


@pytest.mark.parametrize("name", FIXTURES)
def test_the_shipped_files(tmp_path, name):
    path = os.path.join(JF_DIR, name)
    want = jr.read_jf(path)
    k = want["k"]
    out = tmp_path / "out.txt"
    st = kc.dump_file(path, out=str(out), fmt="column")
    lines = out.read_bytes().split(b"\n")
    assert lines[-1] == b"" and st["records_out"] == len(lines) - 1 == len(want["keys"])
    mers, counts = zip(*(ln.split(b" ") for ln in lines[:-1]))
    assert all(len(m) == k for m in mers)
    assert np.array_equal(np.array([km.pack_str(m.decode()) for m in mers], np.uint64), want["keys"])    # and their order
    assert np.array_equal(np.array([int(c) for c in counts], np.uint32), want["counts"])
    kc.dump_file(path, out=str(out))
    assert out.read_bytes() == model(want["keys"], want["counts"], k, "fasta")
    _, _, stats = kc.histo_file(path, lower_count=0)
    kc.dump_file(path, out=str(out), fmt="column", lower_count=1)
    assert stats["distinct"] == out.read_bytes().count(b"\n")


# ------------------------------------------------------------------ a finished counter
def counter_dump(c, **kw):
    return through_pipe(lambda fh: c.dump(fh, **kw))


def test_counter_dump(tmp_path, monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "8192")              # 186 records of k = 31 to a piece
    rng = np.random.default_rng(11)
    n = 5 * T + 3
    keys, counts = distinct_keys(rng, n, 31), digit_cycle(n)
    counts[::7] = 1
    c = kmlib.Counter(k=31, canonical=True)
    try:
        c.add_records(keys, counts)
        with open(os.devnull, "wb") as null, pytest.raises(kmlib.KmError) as e:         # finish comes first
            c.dump(null)
        assert e.value.code == KM_E_STATE
        db = c.finish(2)
        rk, rc = c.records()
        assert rk.size == int((counts >= 2).sum())
        for fmt in FORMATS:
            st, got = counter_dump(c, fmt=fmt)
            want = model(rk, rc, 31, fmt)
            assert got == want, fmt
            assert st == {"records_in": rk.size, "records_out": rk.size, "bytes_out": len(want), "pieces": -(-rk.size // 186)}
        st, got = counter_dump(c, fmt="column", lower_count=420, upper_count=42000)
        assert got == model(rk, rc, 31, "column", 420, 42000) and st["records_in"] == rk.size
        # the counter is as usable as before
        c.write_jf(str(tmp_path / "out.jf"))
        back = jr.read_jf(str(tmp_path / "out.jf"))
        order = np.argsort(rk, kind="stable")
        assert np.array_equal(np.sort(back["keys"]), rk[order]) and back["counts"].sum() == rc.sum()
        _, _, stats = c.histo()
        assert stats["distinct"] == rk.size and stats["total"] == int(rc.sum(dtype=np.uint64))
        assert tc.same(c.records(), (rk, rc))
        assert counter_dump(c, fmt="tab")[1] == model(rk, rc, 31, "tab")
        db.close()
    finally:
        c.close()


def test_counter_dump_of_an_empty_counter():
    c = kmlib.Counter(k=21)
    try:
        c.finish(1).close()
        st, got = counter_dump(c)
        assert got == b"" and st == {"records_in": 0, "records_out": 0, "bytes_out": 0, "pieces": 0}
    finally:
        c.close()


def test_counter_dump_k32_noncanonical_with_all_t():
    c = kmlib.Counter(k=32, canonical=False)
    try:
        c.add_bases(b"T" * 40 + b"N" + b"ACGT" * 10)
        c.finish(1).close()
        rk, rc = c.records()
        assert ALL_T in rk.tolist() and int(rc[rk == ALL_T][0]) == 9
        st, got = counter_dump(c, fmt="column")
        assert got == model(rk, rc, 32, "column") and b"T" * 32 + b" 9\n" in got
        assert st["records_out"] == rk.size
    finally:
        c.close()


# ------------------------------------------------------------------ count --dump
@functools.lru_cache(maxsize=None)
def some_reads():
    return tuple(tc.make_reads(91, 4000))


@pytest.mark.parametrize("jellyfish_order", [False, True])
def test_count_dump_round_trip(tmp_path, jellyfish_order):
    reads = some_reads()
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    out_jf, out_txt, again = tmp_path / "out.jf", tmp_path / "out.txt", tmp_path / "again.txt"
    argv = ["count", "-m", "21", "-C", "-L", "2", "--dump", str(out_txt), "-o", str(out_jf)]
    cli.main(argv + (["--jellyfish-order"] if jellyfish_order else []) + [str(fa)])
    keys, counts = tc.cut(*tc.model(b"\n".join(reads), 21, True), 2)
    want = model(keys, counts, 21, "column")                        # (sorted by key, as the model's records are)
    text = out_txt.read_bytes()
    assert sorted(text.splitlines()) == sorted(want.splitlines()) and len(text) == len(want)
    rec = jr.read_jf(str(out_jf))
    assert text == model(rec["keys"], rec["counts"], 21, "column")   # the lines come in the file's order
    if not jellyfish_order:
        assert text == want
    else:
        assert text != want                                          # (Jellyfish's order is not the key order)
    cli.main(["dump", "-c", "-o", str(again), str(out_jf)])
    assert again.read_bytes() == text                                # `dump -c out.jf`: the same bytes
    # merge --dump of the one file, written in the same mode: the same bytes again
    cli.main(["merge", "--dump", str(tmp_path / "m.txt"), "-o", str(tmp_path / "m.jf")]
             + (["--jellyfish-order"] if jellyfish_order else []) + [str(out_jf)])
    if not jellyfish_order:
        assert (tmp_path / "m.txt").read_bytes() == text
    else:                                                            # (its header's matrix is sized anew: compare by file)
        cli.main(["dump", "-c", "-o", str(again), str(tmp_path / "m.jf")])
        assert (tmp_path / "m.txt").read_bytes() == again.read_bytes()
        assert sorted(again.read_bytes().splitlines()) == sorted(text.splitlines())


# ------------------------------------------------------------------ query
def query_text(db, kmers):
    return through_pipe(lambda fh: db.query_text(kmers, fh))


def test_query_every_record_both_strands_and_absent_kmers(monkeypatch):
    rec = jr.read_jf(NPM1)
    k = rec["k"]
    assert rec["canonical"]
    rng = np.random.default_rng(13)
    absent = np.setdiff1d(jr.canonical_np(rng.integers(0, 1 << 62, 500, dtype=np.uint64), k), rec["keys"])
    asked = np.concatenate([rec["keys"], km.revcomp(rec["keys"], k), absent, rec["keys"][:40], rec["keys"][:40]])
    asked = rng.permutation(asked)
    db = kmlib.Database.open(NPM1)
    try:
        db.upload(0)
        counts = db.query(asked)
        assert (counts[np.isin(asked, absent)] == 0).all() and (counts > 0).sum() == 2 * rec["keys"].size + 80
        st, got = query_text(db, asked)
        assert got == model(asked, counts, k, "column")              # as given, in the order given, duplicates too
        assert st["records_in"] == st["records_out"] == asked.size and st["bytes_out"] == len(got)
        # three upload pieces: 8 * 1024 bytes take 1024 k-mers, the text cap of k = 31 is 8192 // 44 = 186
        monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "8192")
        st, small = query_text(db, asked)
        assert small == got and st["pieces"] == -(-asked.size // 186) >= 3
        assert query_text(db, asked[:0]) == ({"records_in": 0, "records_out": 0, "bytes_out": 0, "pieces": 0}, b"")
    finally:
        db.close()


def test_query_file_prints_the_canonical_mer(tmp_path):
    rec = jr.read_jf(NPM1)
    k = rec["k"]
    key, count = int(rec["keys"][17]), int(rec["counts"][17])
    fwd = km.unpack(key, k)
    rev = km.unpack(int(km.revcomp(np.array([key], np.uint64), k)[0]), k)
    assert fwd != rev and fwd < rev
    out = tmp_path / "q.txt"
    st = kc.query_file(NPM1, mers=[rev, fwd.lower(), "A" * k], out=str(out))
    db = kmlib.Database.open(NPM1)
    try:
        zero = int(db.upload(0).query(np.zeros(1, np.uint64))[0])
    finally:
        db.close()
    assert out.read_text() == "%s %d\n%s %d\n%s %d\n" % (fwd, count, fwd, count, "A" * k, zero)
    assert st["records_out"] == 3
    # a database that is not canonical prints what was asked
    path = write_file(tmp_path / "nc.jf", [key], [count], k, canonical=False)
    kc.query_file(path, mers=[rev, fwd], out=str(out))
    assert out.read_text() == "%s 0\n%s %d\n" % (rev, fwd, count)


@pytest.mark.parametrize("target, db", [("DNMT3A_R882_exon_23.fa", "02H033_DNMT3A_sub.jf"),
                                        ("FLT3-TKD_exon_20.fa", "05H094_FLT3-TKD_del.jf"),
                                        ("MYC_T58A_P59R_exon2.fa", "02H025_NPM1.jf")])
def test_query_sequence_against_min_cov(tmp_path, target, db):
    """Catalog targets of one FASTA record (min_cov joins the records of a file, `query -s` takes them one by one)
    against the table of their own sample, and one against a foreign table, where nearly every count is 0."""
    fa, db = os.path.join(CATALOG, target), os.path.join(JF_DIR, db)
    seq = ko.read_fasta_concat(fa)
    total, length, lo, hi, mean, kmer_nb, kmer_nb_0 = common.get_cov(db, seq)
    common.close(db)
    out = tmp_path / "q.txt"
    cli.main(["query", "-s", fa, "-o", str(out), db])
    counts = np.array([int(ln.split()[1]) for ln in out.read_text().splitlines()], np.int64)
    assert counts.size == kmer_nb == length - 31 + 1
    assert (int(counts.sum()), int(counts.min()), int(counts.max()), int((counts == 0).sum())) == (total, lo, hi, kmer_nb_0)
    mers = [ln.split()[0] for ln in out.read_text().splitlines()]
    want = jr.canonical_np(km.sliding_kmers(km.encode(seq), 31), 31)
    assert mers == [km.unpack(x, 31) for x in want.tolist()]


def test_query_sequence_takes_the_records_of_a_file_one_by_one(tmp_path):
    """The NPM1 target has two records, of 27 and 53 bases: no k-mer spans them, so the 23 windows of the second."""
    fa = os.path.join(CATALOG, "NPM1_4ins_exons_10-11utr.fa")
    second = open(fa).read().split(">")[2].split("\n", 1)[1].replace("\n", "")
    assert len(second) == 53
    res = common.get_cov(NPM1, second)
    common.close(NPM1)
    out = tmp_path / "q.txt"
    cli.main(["query", "-s", fa, "-o", str(out), NPM1])
    counts = np.array([int(ln.split()[1]) for ln in out.read_text().splitlines()], np.int64)
    assert counts.size == res[5] == 23 and (int(counts.sum()), int(counts.min()), int(counts.max())) == res[0:1] + res[2:4]


# ------------------------------------------------------------------ the command line, its descriptor 1 the library's
def run_cli(args, **kw):
    env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system", **kw.pop("env", {}))
    return subprocess.run([sys.executable, "-m", "km_amd"] + args, capture_output=True, timeout=300, env=env, **kw)


def test_cli_dump_and_query_to_standard_output():
    rec = jr.read_jf(NPM1)
    res = run_cli(["dump", "-c", NPM1])
    assert res.returncode == 0, res.stderr
    assert res.stdout == model(rec["keys"], rec["counts"], 31, "column")
    res = run_cli(["dump", "-c", "-t", "-L", "10", "-U", "1000", NPM1])
    assert res.returncode == 0 and res.stdout == model(rec["keys"], rec["counts"], 31, "tab", 10, 1000)
    first = res.stdout.split(b"\n")[0].split(b"\t")
    res = run_cli(["query", NPM1, first[0].decode()])
    assert res.returncode == 0 and res.stdout == first[0] + b" " + first[1] + b"\n"      # `query` of a dumped mer: its count
    res = run_cli(["dump", "-t", NPM1])
    assert res.returncode == 2 and res.stdout == b""


def test_a_reader_that_goes_away(tmp_path):
    """The read end of the pipe is closed while the library writes: the call ends with KM_E_IO (the command with a
    message and a non-zero status), nothing hangs, and the next call on the same streams works."""
    rng = np.random.default_rng(17)
    n = 20000                                                        # 700 KB of text: far beyond a pipe's buffer
    keys, counts = distinct_keys(rng, n, 31), digit_cycle(n)
    path = write_file(tmp_path / "big.jf", keys, counts, 31)
    env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system", KM_COUNT_STAGE_BYTES="256")
    proc = subprocess.Popen([sys.executable, "-m", "km_amd", "dump", "-c", path], stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, env=env)
    head = proc.stdout.read(44)
    proc.stdout.close()
    err = proc.stderr.read()
    assert proc.wait(timeout=120) == 1 and b"ERROR: dump" in err and b"writing the text failed" in err, err
    assert head == model(keys[:2], counts[:2], 31, "column")[:44]
    # in this process (Python ignores SIGPIPE): the code, and the library goes on
    r, w = os.pipe()
    os.close(r)
    try:
        with pytest.raises(kmlib.KmError) as e:
            kmlib.jf_dump(path, w, fmt="column")
        assert e.value.code == KM_E_IO
    finally:
        os.close(w)
    out = tmp_path / "out.txt"
    kc.dump_file(path, out=str(out), fmt="column")
    assert out.read_bytes() == model(keys, counts, 31, "column")
