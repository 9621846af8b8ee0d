"""`dump` and `query`, the parts that need no GPU: the model of the text rule against literal strings, the sanitizer
build of csrc/dump_text.h, what the five C entry points refuse before any device work, the argument parser, and the
host-side k-mer extraction of `query`.  The GPU side is tests/test_dump.py, which takes its model from here.

The model is written from the rule of include/kmgpu.h alone (km_amd.kmer.unpack and %d, the same vectorised) and shares
nothing with csrc/dump_text.h.  The rule is this project's reading of `jellyfish dump` / `jellyfish query`: no run of
Jellyfish stands behind it."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from km_amd import cli
from km_amd import count as kc
from km_amd import kmer as km
from km_amd import lib as kmlib

HERE = os.path.dirname(os.path.abspath(__file__))
JF_DIR = os.path.join(HERE, "data", "jf")
CATALOG = os.path.join(HERE, "data", "catalog", "GRCh38")
NPM1 = os.path.join(JF_DIR, "02H025_NPM1.jf")
TOP = 0xFFFFFFFF
KM_E_IO, KM_E_FORMAT, KM_E_ARG, KM_E_STATE, KM_E_CAPACITY = 1, 2, 4, 7, 8
FORMATS = ("fasta", "column", "tab")


# ------------------------------------------------------------------ the model
def model_slow(keys, counts, k, fmt="fasta", lower=0, upper=TOP):
    """The rule, record by record: km.unpack and %d."""
    out = []
    for key, c in zip(np.asarray(keys, np.uint64).tolist(), np.asarray(counts, np.uint32).tolist()):
        if not lower <= c <= upper:
            continue
        mer = km.unpack(key, k)
        out.append(">%d\n%s\n" % (c, mer) if fmt == "fasta" else "%s%s%d\n" % (mer, "\t" if fmt == "tab" else " ", c))
    return "".join(out).encode("ascii")


def model(keys, counts, k, fmt="fasta", lower=0, upper=TOP):
    """The same for many records: the letters of all mers as one numpy table, one %-format per line."""
    keys = np.asarray(keys, np.uint64)
    counts = np.asarray(counts, np.uint32)
    keep = (counts.astype(np.int64) >= lower) & (counts.astype(np.int64) <= upper)
    keys, counts = keys[keep], counts[keep]
    shifts = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    letters = np.frombuffer(b"ACGT", np.uint8)[((keys[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)]
    blob = letters.tobytes()
    mers = [blob[i * k:(i + 1) * k] for i in range(keys.size)]
    if fmt == "fasta":
        return b"".join(b">%d\n%s\n" % (c, m) for c, m in zip(counts.tolist(), mers))
    sep = b"\t" if fmt == "tab" else b" "
    return b"".join(b"%s%s%d\n" % (m, sep, c) for c, m in zip(counts.tolist(), mers))


def test_model_against_literal_strings():
    keys, counts = [0b0111], [9]
    assert model_slow(keys, counts, 2, "fasta") == b">9\nCT\n"
    assert model_slow(keys, counts, 2, "column") == b"CT 9\n"
    assert model_slow(keys, counts, 2, "tab") == b"CT\t9\n"
    t32 = b"T" * 32
    every = ([2 ** 64 - 1] * 4, [0, 9, 10, TOP])
    assert model_slow(*every, 32, "fasta") == b">0\n" + t32 + b"\n>9\n" + t32 + b"\n>10\n" + t32 + b"\n>4294967295\n" + t32 + b"\n"
    assert model_slow(*every, 32, "column") == t32 + b" 0\n" + t32 + b" 9\n" + t32 + b" 10\n" + t32 + b" 4294967295\n"
    assert model_slow(*every, 32, "tab") == t32 + b"\t0\n" + t32 + b"\t9\n" + t32 + b"\t10\n" + t32 + b"\t4294967295\n"
    # the filter: lower <= count <= upper, a zero count is printed by default, lower > upper prints nothing
    assert model_slow(*every, 32, "column", lower=1) == t32 + b" 9\n" + t32 + b" 10\n" + t32 + b" 4294967295\n"
    assert model_slow(*every, 32, "column", lower=9, upper=10) == t32 + b" 9\n" + t32 + b" 10\n"
    assert model_slow(*every, 32, "column", lower=10, upper=9) == b""
    # bits above 2k are ignored
    assert model_slow([0b110111], [1], 2, "column") == b"CT 1\n"
    rng = np.random.default_rng(7)
    for k in (2, 5, 17, 31, 32):
        keys = rng.integers(0, 2 ** 63, 300, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 300, dtype=np.uint64)
        counts = (10 ** rng.integers(0, 10, 300) * rng.integers(0, 10, 300)).clip(0, TOP).astype(np.uint32)
        for fmt in FORMATS:
            assert model(keys, counts, k, fmt) == model_slow(keys, counts, k, fmt)
            assert model(keys, counts, k, fmt, 5, 5000) == model_slow(keys, counts, k, fmt, 5, 5000)


def test_text_rule_under_the_sanitizers(tmp_path):
    """csrc/dump_text.h built for the CPU with AddressSanitizer + UBSan (tests/host/dump_text.cpp): the host writer for
    every k in 2..32, every digit count 1..10 and the three formats against snprintf, into buffers of exactly the
    line's length between guard bytes; the worst case k + 13."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "dump_text")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "host", "dump_text.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert proc.returncode == 0 and "DUMP TEXT OK" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in proc.stderr and "runtime error" not in proc.stderr, proc.stderr[-3000:]


def test_refusals_come_before_any_device_work(tmp_path):
    """No GPU is needed for any of these: each fails with its code on a machine without one."""
    import ctypes as C
    lib = kmlib.load()
    keys, counts = np.arange(4, dtype=np.uint64), np.ones(4, np.uint32)
    out = np.zeros(256, np.uint8)
    ln = C.c_uint64()
    pk, pc, po = kmlib.ptr(keys), kmlib.ptr(counts), kmlib.ptr(out)
    null = os.open(os.devnull, os.O_WRONLY)
    try:
        # km_dump_text
        assert lib.km_dump_text(0, pk, pc, 4, 31, 1, 0, TOP, po, out.size, None, None) == KM_E_ARG
        assert lib.km_dump_text(0, None, pc, 4, 31, 1, 0, TOP, po, out.size, C.byref(ln), None) == KM_E_ARG
        assert lib.km_dump_text(0, pk, None, 4, 31, 1, 0, TOP, po, out.size, C.byref(ln), None) == KM_E_ARG
        assert lib.km_dump_text(0, pk, pc, 4, 31, 1, 0, TOP, None, out.size, C.byref(ln), None) == KM_E_ARG
        assert lib.km_dump_text(0, pk, pc, 4, 31, 7, 0, TOP, po, out.size, C.byref(ln), None) == KM_E_ARG
        assert b"7" in lib.km_last_error()
        assert lib.km_dump_text(0, pk, pc, 4, 31, -1, 0, TOP, po, out.size, C.byref(ln), None) == KM_E_ARG
        for k in (1, 33, 0, -5):
            assert lib.km_dump_text(0, pk, pc, 4, k, 1, 0, TOP, po, out.size, C.byref(ln), None) == KM_E_ARG
            assert str(k).encode() in lib.km_last_error()
        assert lib.km_dump_text(-1, pk, pc, 4, 31, 1, 0, TOP, po, out.size, C.byref(ln), None) == KM_E_ARG
        assert not out.any()
        for fmt in ("fasta", "column", "tab"):
            for k in (1, 33):
                with pytest.raises(kmlib.KmError) as e:
                    kmlib.dump_text(keys, counts, k, fmt)
                assert e.value.code == KM_E_ARG
        with pytest.raises(kmlib.KmError) as e:
            kmlib.dump_text(keys, counts, 31, 7)
        assert e.value.code == KM_E_ARG
        # km_jf_dump
        path = os.fsencode(NPM1)
        assert lib.km_jf_dump(0, None, null, 1, 0, TOP, None, None) == KM_E_ARG
        assert lib.km_jf_dump(0, path, null, 7, 0, TOP, None, None) == KM_E_ARG
        assert lib.km_jf_dump(-1, path, null, 1, 0, TOP, None, None) == KM_E_ARG
        assert lib.km_jf_dump(0, path, 987654, 1, 0, TOP, None, None) == KM_E_IO
        assert b"987654" in lib.km_last_error()
        closed = os.dup(null)
        os.close(closed)
        assert lib.km_jf_dump(0, path, closed, 1, 0, TOP, None, None) == KM_E_IO
        assert lib.km_jf_dump(0, os.fsencode(str(tmp_path / "no_such.jf")), null, 1, 0, TOP, None, None) == KM_E_IO
        assert lib.km_jf_dump(0, os.fsencode(os.path.join(CATALOG, "IDH1_R132.fa")), null, 1, 0, TOP, None, None) == KM_E_FORMAT
        # km_counter_dump, kmjf_query_text, km_dump_kernel_ms
        assert lib.km_counter_dump(None, null, 1, 0, TOP, None) == KM_E_ARG
        assert lib.kmjf_query_text(None, pk, 4, null, None, None) == KM_E_ARG
        assert lib.km_dump_kernel_ms(None) == KM_E_ARG
        db = kmlib.Database.from_records(keys, counts, 31)
        try:
            assert lib.kmjf_query_text(db._h, None, 4, null, None, None) == KM_E_ARG
            assert lib.kmjf_query_text(db._h, pk, 4, 987654, None, None) == KM_E_IO
            assert lib.kmjf_query_text(db._h, pk, 4, null, None, None) == KM_E_STATE        # not uploaded
        finally:
            db.close()
    finally:
        os.close(null)
    # the Python layer: the same codes, and a file this call created is removed again
    made = tmp_path / "made.txt"
    with pytest.raises(kmlib.KmError) as e:
        kc.dump_file(str(tmp_path / "no_such.jf"), out=str(made))
    assert e.value.code == KM_E_IO and not made.exists()
    with pytest.raises(kmlib.KmError) as e:
        kc.dump_file(os.path.join(CATALOG, "IDH1_R132.fa"), out=str(made), fmt="column")
    assert e.value.code == KM_E_FORMAT and not made.exists()
    with pytest.raises(kmlib.KmError) as e:
        kc.dump_file(NPM1, out=str(made), fmt=7)
    assert e.value.code == KM_E_ARG and not made.exists()
    # a file that was there before the call is neither removed nor, for a bad input, emptied
    made.write_text("kept\n")
    for bad in (str(tmp_path / "no_such.jf"), os.path.join(CATALOG, "IDH1_R132.fa")):
        with pytest.raises(kmlib.KmError):
            kc.dump_file(bad, out=str(made))
        assert made.read_text() == "kept\n"
    with pytest.raises(kmlib.KmError):
        kc.dump_file(NPM1, out=str(made), fmt=7)
    assert made.exists()


def test_parser_accepts_dump_and_query():
    a = cli.parse_args(["dump", "x.jf"])
    assert (a.column, a.tab, a.lower_count, a.upper_count, a.output, a.db) == (False, False, 0, TOP, None, "x.jf")
    a = cli.parse_args(["dump", "-c", "-t", "-L", "2", "-U", "9", "-o", "d.txt", "x.jf"])
    assert (a.column, a.tab, a.lower_count, a.upper_count, a.output, a.db) == (True, True, 2, 9, "d.txt", "x.jf")
    a = cli.parse_args(["dump", "-U", "4294967295", "-c", "x.jf"])
    assert (a.column, a.tab, a.upper_count) == (True, False, TOP)
    a = cli.parse_args(["query", "x.jf", "ACGT", "TTTT"])
    assert (a.db, a.mers, a.sequence, a.output) == ("x.jf", ["ACGT", "TTTT"], [], None)
    a = cli.parse_args(["query", "-s", "a.fa", "-s", "b.fa.gz", "-o", "q.txt", "x.jf"])
    assert (a.db, a.mers, a.sequence, a.output) == ("x.jf", [], ["a.fa", "b.fa.gz"], "q.txt")
    a = cli.parse_args(["query", "-s", "a.fa", "x.jf", "ACGT"])
    assert (a.mers, a.sequence) == (["ACGT"], ["a.fa"])
    for bad in (["dump", "-t", "x.jf"], ["dump", "-L", "-1", "x.jf"], ["dump", "-U", "4294967296", "x.jf"],
                ["dump", "-c", "-L", "x", "x.jf"], ["dump"], ["query", "x.jf"], ["query"], ["query", "-o", "q.txt", "x.jf"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(bad)
        assert e.value.code == 2, bad
    assert cli.parse_args(["count", "--dump", "d.txt", "-o", "o.jf", "r.fq"]).dump == "d.txt"
    assert cli.parse_args(["merge", "--dump", "d.txt", "a.jf", "b.jf"]).dump == "d.txt"
    assert cli.parse_args(["count", "r.fq"]).dump is None and cli.parse_args(["merge", "a.jf"]).dump is None


@pytest.mark.parametrize("mers, named", [
    (["A" * 30], "A" * 30),                                         # one letter short of the file's k = 31
    (["A" * 31, "C" * 32], "C" * 32),
    (["A" * 15 + "N" + "A" * 15], "A" * 15 + "N" + "A" * 15),
    (["ACGT" * 7 + "ACG", "acgt" * 7 + "ac-"], "ac-"),
])
def test_query_names_a_bad_mer_before_the_table_is_loaded(mers, named):
    """No GPU here, so a table that was loaded would fail otherwise; the message names the mer and its position."""
    with pytest.raises(SystemExit) as e:
        kc.query_file(NPM1, mers=mers)
    assert named in str(e.value) and "argument %d" % len(mers) in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(["query", NPM1] + mers)
    assert named in str(e.value)


# ------------------------------------------------------------------ the k-mers `query` looks up
_COMP = str.maketrans("ACGT", "TGCA")


def windows_by_hand(records, k, canonical):
    keys = []
    for seq in records:
        seq = seq.upper()
        for i in range(len(seq) - k + 1):
            w = seq[i:i + k]
            if set(w) <= set("ACGT"):
                key = km.pack_str(w)
                keys.append(min(key, km.pack_str(w.translate(_COMP)[::-1])) if canonical else key)
    return np.array(keys, np.uint64)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [5, 31, 32])
def test_query_keys_on_the_host(tmp_path, k, canonical):
    rng = np.random.default_rng(k)
    long_a = "".join("ACGTacgt"[i] for i in rng.integers(0, 8, 300))           # lower case
    with_n = "".join("ACGT"[i] for i in rng.integers(0, 4, 120))
    with_n = with_n[:50] + "N" + with_n[51:90] + "nR" + with_n[92:]            # windows over N / n / R are skipped
    short = "ACGT"[:k - 1] if k <= 5 else "ACGTTGCA" * 3                        # shorter than k: no window
    assert len(short) < k
    one = tmp_path / "one.fa"
    one.write_text(">a two lines\n%s\n%s\n>short\n%s\n>b\n%s\n" % (long_a[:137], long_a[137:], short, with_n))
    two = tmp_path / "two.fa.gz"
    with gzip.open(two, "wt") as fh:
        fh.write("ignored before the first header\n>c\r\n%s\r\n\r\n%s\r\n" % (with_n[:60], with_n[60:]))
    mers = [long_a[7:7 + k], "T" * k, "a" * k, long_a[7:7 + k]]
    got = kc.query_keys(k, canonical, mers=mers, seq_files=[str(one), str(two)])
    want = np.concatenate([windows_by_hand([long_a, short, with_n], k, canonical),
                           windows_by_hand([with_n], k, canonical), windows_by_hand(mers, k, canonical)])
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    n_seq = want.size - len(mers)
    assert n_seq < (300 - k + 1) + 2 * (120 - k + 1)                           # some windows were skipped
    # the order: -s files as given, then the mers; either alone
    assert np.array_equal(kc.query_keys(k, canonical, seq_files=[str(two), str(one)]),
                          np.concatenate([want[n_seq - windows_by_hand([with_n], k, canonical).size:n_seq],
                                          want[:n_seq - windows_by_hand([with_n], k, canonical).size]]))
    assert np.array_equal(kc.query_keys(k, canonical, mers=mers), want[n_seq:])
    assert kc.query_keys(k, canonical).size == 0
    if canonical:
        assert int(got[-3]) == 0 and int(got[-2]) == 0                          # T^k and a^k both print as A^k
    else:
        assert km.unpack(int(got[-3]), k) == "T" * k
