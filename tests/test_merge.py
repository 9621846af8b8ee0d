"""Merging tables that already exist (km_jf_file_info, km_counter_add_records, km_counter_add_jf,
km_amd.count.merge_files, `python -m km_amd merge`).

Every comparison is exact.  The model is written here from the definition and shares no code with the kernels: a
dict per key; the counts of one key are summed and the sum clipped at 2^32 - 1, or their maximum is taken; records
with count 0 are dropped; the cut at lower_count comes last.  Files are read back with oracle.jf_reader.  The
semantics are this project's own: no run of `jellyfish merge` stands behind them."""
import json
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
from oracle import km_oracle as ko
import test_count_quality as tq

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JF_DIR = os.path.join(HERE, "data", "jf")
FIXTURES = sorted(f for f in os.listdir(JF_DIR) if f.endswith(".jf"))
CATALOG = os.path.join(HERE, "data", "catalog", "GRCh38")
ITD, TKD = "03H116_ITD.jf", "05H094_FLT3-TKD_del.jf"
TOP = 0xFFFFFFFF
ALL_T = 0xFFFFFFFFFFFFFFFF
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


# ------------------------------------------------------------------ the model
def merged_model(inputs, mode, lower=1):
    """inputs: (keys, counts) per file or call, in order -> (keys ascending, counts) of the merged table."""
    acc = {}
    for keys, counts in inputs:
        for key, c in zip(np.asarray(keys, np.uint64).tolist(), np.asarray(counts, np.uint32).tolist()):
            if c == 0:
                continue
            acc[key] = min(acc.get(key, 0) + c, TOP) if mode == "sum" else max(acc.get(key, 0), c)
    items = sorted((key, c) for key, c in acc.items() if c >= lower)
    return (np.array([key for key, _ in items], np.uint64), np.array([c for _, c in items], np.uint32))


def model_pos(keys, columns, size_log2):
    """Jellyfish's position of a key under a header's matrix (the definition tests/test_jf_order.py pins)."""
    keys = np.asarray(keys, np.uint64)
    columns = np.asarray(columns, np.uint64)
    c = columns.size
    pos = np.zeros(keys.size, np.uint64)
    for i in range(c):
        bit = ((keys >> np.uint64(i)) & np.uint64(1)).astype(bool)
        pos ^= np.where(bit, columns[c - 1 - i], np.uint64(0))
    return pos & np.uint64((1 << size_log2) - 1)


def write_file(path, keys, counts, k, canonical=True, counter_len=4):
    """A `binary/sorted`-framed file with records in the order given: ceil(2k / 8) key bytes, counter_len count
    bytes."""
    keys = np.asarray(keys, np.uint64)
    counts = np.asarray(counts, np.uint32)
    assert counter_len == 4 or not counts.size or int(counts.max()) < 1 << (8 * counter_len)
    header = {"alignment": 8, "canonical": bool(canonical), "cmdline": ["test_merge"], "counter_len": counter_len,
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


def fixture(name):
    rec = jr.read_jf(os.path.join(JF_DIR, name))
    return rec["keys"], rec["counts"]


def merged_on_gpu(feed, k=31, canonical=True, lower=1, expected_distinct=0):
    """feed(counter) adds; -> (keys ascending, counts, stats before the cut, merge_stats)."""
    c = kmlib.Counter(k=k, canonical=canonical, expected_distinct=expected_distinct)
    try:
        feed(c)
        stats, merge = c.stats(), c.merge_stats()
        c.finish(lower).close()
        keys, counts = c.records()
    finally:
        c.close()
    order = np.argsort(keys, kind="stable")
    return keys[order], counts[order], stats, merge


def same(got, want):
    return (got[0].dtype, got[1].dtype) == (np.uint64, np.uint32) and np.array_equal(got[0], want[0]) and \
        np.array_equal(got[1], want[1])


def random_keys(rng, n, k):
    return rng.integers(0, (1 << (2 * k)) - 1, n, dtype=np.uint64, endpoint=True)


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", FIXTURES)
def test_file_info_equals_the_header_of_the_real_files(name):
    path = os.path.join(JF_DIR, name)
    rec = jr.read_jf(path)
    info = kmlib.jf_file_info(path)
    hdr = rec["header"]
    assert info == {"k": hdr["key_len"] // 2, "canonical": bool(hdr["canonical"]), "n_records": rec["keys"].size,
                    "key_bytes": (hdr["key_len"] + 7) // 8, "counter_len": hdr["counter_len"]}
    assert info["n_records"] >= 200 and (info["k"], info["key_bytes"], info["counter_len"]) == (31, 8, 4)


def test_file_info_of_written_files_and_bad_files(tmp_path):
    p = write_file(tmp_path / "k5.jf", [1, 2, 3], [7, 0, 9], 5, canonical=False, counter_len=2)
    assert kmlib.jf_file_info(p) == {"k": 5, "canonical": False, "n_records": 3, "key_bytes": 2, "counter_len": 2}
    assert kmlib.jf_file_info(write_file(tmp_path / "none.jf", [], [], 21))["n_records"] == 0
    lib = kmlib.load()
    assert lib.km_jf_file_info(None, None, None, None, None, None) == 4
    assert lib.km_jf_file_info(os.fsencode(p), None, None, None, None, None) == 0        # any output may be NULL
    raw = open(os.path.join(JF_DIR, FIXTURES[0]), "rb").read()
    bad = {"truncated.jf": raw[:200], "text.jf": b"@r0\nACGT\n+\nIIII\n" * 40, "short.jf": b"0000", "empty.jf": b""}
    codes = {}
    for name, data in bad.items():
        (tmp_path / name).write_bytes(data)
        with pytest.raises(kmlib.KmError) as opened:
            kmlib.Database.open(str(tmp_path / name))
        with pytest.raises(kmlib.KmError) as asked:
            kmlib.jf_file_info(str(tmp_path / name))
        assert asked.value.code == opened.value.code, name
        codes[name] = asked.value.code
    assert set(codes.values()) == {2}                                   # KM_E_FORMAT, all four
    with pytest.raises(kmlib.KmError) as asked:
        kmlib.jf_file_info(str(tmp_path / "no_such.jf"))
    with pytest.raises(kmlib.KmError) as opened:
        kmlib.Database.open(str(tmp_path / "no_such.jf"))
    assert asked.value.code == opened.value.code == 1


def test_merge_files_refuses_a_mismatch_before_any_counter(tmp_path):
    a = write_file(tmp_path / "a.jf", [1, 2], [3, 4], 31)
    b = write_file(tmp_path / "b.jf", [1, 2], [3, 4], 21)
    c = write_file(tmp_path / "c.jf", [1, 2], [3, 4], 31, canonical=False)
    for other in (b, c):
        with pytest.raises(ValueError) as e:                            # (raised without a GPU: no counter exists yet)
            kc.merge_files([a, a, other])
        assert other in str(e.value) and a in str(e.value) and "k=31" in str(e.value)
    with pytest.raises(ValueError):
        kc.merge_files([a], mode="min")
    with pytest.raises(ValueError):
        kc.merge_files([])
    with pytest.raises(kmlib.KmError) as e:                             # an unreadable input: the header's own error
        kc.merge_files([a, str(tmp_path / "no_such.jf")])
    assert e.value.code == 1


def test_parser_accepts_merge():
    p = cli.build_parser()
    args = p.parse_args(["merge", "a.jf"])
    assert (args.output, args.lower_count, args.max, args.jellyfish_order, args.inputs) == (
        "mer_counts_merged.jf", 1, False, False, ["a.jf"])
    args = p.parse_args(["merge", "-L", "3", "--max", "--jellyfish-order", "-o", "m.jf", "a.jf", "b.jf", "c.jf"])
    assert (args.output, args.lower_count, args.max, args.jellyfish_order, args.inputs) == (
        "m.jf", 3, True, True, ["a.jf", "b.jf", "c.jf"])
    with pytest.raises(SystemExit):
        p.parse_args(["merge"])


def test_argument_errors_without_a_counter():
    lib = kmlib.load()
    keys, counts = np.zeros(2, np.uint64), np.ones(2, np.uint32)
    assert lib.km_counter_add_records(None, kmlib.ptr(keys), kmlib.ptr(counts), 2, 0) == 4
    assert lib.km_counter_add_jf(None, b"x.jf", 0, None) == 4
    assert lib.km_counter_merge_stats(None, None, None) == 4


def test_piece_arithmetic_under_the_sanitizers(tmp_path):
    """csrc/merge_pieces.h built for the CPU with AddressSanitizer + UBSan (tests/host/merge_pieces.cpp): record
    sizes 3..12 at staging sizes of 256, 4 096 and 16 MiB, host arrays packed into 12-byte records, and read_exact
    over a temporary file: to its last byte, from an odd offset, nothing, one byte too many, a descriptor that cannot
    be read."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "merge_pieces")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "host", "merge_pieces.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert proc.returncode == 0 and "PIECES OK" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in proc.stderr and "runtime error" not in proc.stderr, proc.stderr[-3000:]


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sum", "max"])
def test_gpu_the_five_real_files_together(mode):
    paths = [os.path.join(JF_DIR, f) for f in FIXTURES]
    inputs = [fixture(f) for f in FIXTURES]
    want = merged_model(inputs, mode)
    assert want[0].size < sum(k.size for k, _ in inputs)                # the files share k-mers: something is combined

    def feed(c):
        assert [c.add_jf(p, mode=mode) for p in paths] == [k.size for k, _ in inputs]
    keys, counts, stats, merge = merged_on_gpu(feed)
    assert same((keys, counts), want)
    assert stats["distinct"] == want[0].size and (stats["bases"], stats["kmers"]) == (0, 0)
    assert merge["records_in"] == sum(int((c > 0).sum()) for _, c in inputs)
    # the cut comes last (these files were counted with -L 2: a cut at 2 would remove nothing)
    cut = merged_model(inputs, mode, lower=5)
    assert same(merged_on_gpu(feed, lower=5)[:2], cut) and 0 < cut[0].size < want[0].size
    # and through merge_files, which sizes the table from the largest input
    db, stats2 = kc.merge_files(paths, mode=mode)
    absent = jr.canonical_np(random_keys(np.random.default_rng(70), 50, 31), 31)
    absent = absent[~np.isin(absent, want[0])]
    answer = db.query(np.concatenate([want[0], absent]))
    db.close()
    assert np.array_equal(answer[:want[0].size], want[1]) and not answer[want[0].size:].any() and absent.size >= 45
    assert (stats2["distinct"], stats2["mode"], stats2["k"], stats2["canonical"]) == (want[0].size, mode, 31, True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sum", "max"])
def test_gpu_piece_boundaries(tmp_path, monkeypatch, mode):
    rng = np.random.default_rng(71)
    # two real files: 12-byte records, 21 per piece of 256 bytes with 4 bytes left over
    real = [os.path.join(JF_DIR, ITD), os.path.join(JF_DIR, TKD)]
    want = merged_model([fixture(ITD), fixture(TKD)], mode)
    # k = 21: 6 + 4 bytes, 25 per piece with 6 left over; 1 013 and 537 records, half of the second shared
    k1 = np.unique(random_keys(rng, 1100, 21))[:1013]
    k2 = np.concatenate([rng.permutation(k1)[:270], np.unique(random_keys(rng, 300, 21))[:267]])
    c1 = rng.integers(1, 1 << 32, k1.size, dtype=np.uint64).astype(np.uint32)
    c2 = rng.integers(1, 1 << 32, k2.size, dtype=np.uint64).astype(np.uint32)
    made = [write_file(tmp_path / "a21.jf", k1, c1, 21), write_file(tmp_path / "b21.jf", k2, c2, 21)]
    want21 = merged_model([(k1, c1), (k2, c2)], mode)
    assert kmlib.jf_file_info(made[0])["key_bytes"] == 6 and k1.size % 25 and k2.size % 25
    assert fixture(ITD)[0].size % 21 and fixture(TKD)[0].size % 21      # the last piece of each is short

    def run(paths, k):
        return merged_on_gpu(lambda c: [c.add_jf(p, mode=mode) for p in paths], k=k)[:2]
    default = run(real, 31), run(made, 21)
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "256")
    small = run(real, 31), run(made, 21)
    assert same(small[0], default[0]) and same(small[0], want)
    assert same(small[1], default[1]) and same(small[1], want21)


@pytest.mark.gpu
def test_gpu_record_widths(tmp_path):
    rng = np.random.default_rng(72)
    for mode in ("sum", "max"):
        # k = 5: 2 key bytes, 4 count bytes; all 1 024 keys, twice
        keys = rng.permutation(np.arange(1024, dtype=np.uint64))
        inputs = [(keys, rng.integers(1, 1 << 32, 1024, dtype=np.uint64).astype(np.uint32)),
                  (keys[::-1], rng.integers(1, 1 << 32, 1024, dtype=np.uint64).astype(np.uint32))]
        paths = [write_file(tmp_path / ("k5_%d.jf" % i), *inp, 5, canonical=False) for i, inp in enumerate(inputs)]
        got = merged_on_gpu(lambda c: [c.add_jf(p, mode=mode) for p in paths], k=5, canonical=False)
        assert same(got[:2], merged_model(inputs, mode)) and got[2]["distinct"] == 1024
        # k = 31 with 1 and 2 count bytes (9- and 10-byte records) into one counter
        keys = np.unique(random_keys(rng, 700, 31))[:600]
        inputs = [(keys, rng.integers(1, 256, 600).astype(np.uint32)),
                  (keys[100:], rng.integers(1, 65536, 500).astype(np.uint32))]
        paths = [write_file(tmp_path / "cb1.jf", *inputs[0], 31, counter_len=1),
                 write_file(tmp_path / "cb2.jf", *inputs[1], 31, counter_len=2)]
        assert [kmlib.jf_file_info(p)["counter_len"] for p in paths] == [1, 2]
        got = merged_on_gpu(lambda c: [c.add_jf(p, mode=mode) for p in paths])
        assert same(got[:2], merged_model(inputs, mode))
        # k = 32, not canonical: the key 2^64 - 1 (T^32, the table's empty mark) in both inputs
        inputs = []
        for n_all_t in (0xFFFFFF00, 0x200):
            keys = rng.permutation(np.unique(np.concatenate([random_keys(rng, 300, 32), np.array([ALL_T, 0], np.uint64)])))
            counts = rng.integers(1, 1000, keys.size).astype(np.uint32)
            counts[keys == np.uint64(ALL_T)] = n_all_t
            inputs.append((keys, counts))
        paths = [write_file(tmp_path / ("k32_%d.jf" % i), *inp, 32, canonical=False) for i, inp in enumerate(inputs)]
        want = merged_model(inputs, mode)
        got = merged_on_gpu(lambda c: [c.add_jf(p, mode=mode) for p in paths], k=32, canonical=False)
        assert same(got[:2], want) and got[2]["distinct"] == want[0].size
        assert int(want[0][-1]) == ALL_T and int(want[1][-1]) == (TOP if mode == "sum" else 0xFFFFFF00)
        # records with count 0 are skipped and claim no slot
        keys = np.unique(random_keys(rng, 500, 31))[:400]
        counts = rng.integers(1, 100, 400).astype(np.uint32)
        counts[::3] = 0
        p = write_file(tmp_path / "zeros.jf", keys, counts, 31)
        got = merged_on_gpu(lambda c: c.add_jf(p, mode=mode))
        want = merged_model([(keys, counts)], mode)
        assert same(got[:2], want) and want[0].size == 400 - 134
        assert got[2]["distinct"] == want[0].size and got[3]["records_in"] == want[0].size


@pytest.mark.gpu
@pytest.mark.parametrize("stage", [None, 4096])
def test_gpu_growth(tmp_path, monkeypatch, stage):
    """A default counter has 65 536 slots and fills them to a half: three inputs of 40 000 records from a pool of
    60 000 keys make it grow before the first piece (default staging) or between pieces of 341 records."""
    if stage:
        monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))
    rng = np.random.default_rng(73)
    pool = np.unique(random_keys(rng, 61_000, 31))[:60_000]
    inputs = []
    for i in range(3):
        keys = rng.permutation(pool)[:40_000]
        inputs.append((keys, rng.integers(1, 1 << 31, keys.size).astype(np.uint32)))
    paths = [write_file(tmp_path / ("g%d.jf" % i), *inp, 31) for i, inp in enumerate(inputs)]
    for mode in ("sum", "max"):
        want = merged_model(inputs, mode)
        keys, counts, stats, merge = merged_on_gpu(lambda c: [c.add_jf(p, mode=mode) for p in paths])
        assert same((keys, counts), want)
        assert stats["n_grow"] >= 1 and stats["distinct"] == want[0].size and stats["slots"] >= 2 * want[0].size
        assert merge["records_in"] == 120_000


@pytest.mark.gpu
def test_gpu_contention_and_saturation():
    key = np.uint64(0x123456789ABCDEF)

    def one(calls, mode):
        keys, counts, stats, _ = merged_on_gpu(
            lambda c: [c.add_records(np.full(n, key), np.full(n, v, np.uint32), mode=mode) for n, v in calls])
        assert keys.tolist() == [int(key)] and stats["distinct"] == 1
        return int(counts[0])
    assert one([(4096, 3)], "sum") == 12288
    assert one([(4096, 3)], "max") == 3
    assert one([(8, 0x40000000)], "sum") == TOP
    assert one([(8, 0x40000000)], "max") == 0x40000000
    assert one([(1, 0xFFFFFFF0), (1, 0x20)], "sum") == TOP
    assert one([(1, 0x20), (1, 0xFFFFFFF0)], "sum") == TOP
    assert one([(1, 0xFFFFFFF0), (1, 0x0F)], "sum") == TOP              # lands on the top exactly
    assert one([(1, 0xFFFFFFF0), (1, 0x0E)], "sum") == TOP - 1
    # many keys, each many times in one call, against the model
    rng = np.random.default_rng(74)
    keys = random_keys(rng, 50, 31)[rng.integers(0, 50, 20_000)]
    counts = rng.integers(0, 1 << 28, keys.size).astype(np.uint32)
    for mode in ("sum", "max"):
        got = merged_on_gpu(lambda c: c.add_records(keys, counts, mode=mode))
        assert same(got[:2], merged_model([(keys, counts)], mode))


def make_reads(seed, n_reads):
    """Reads of 30-150 nt from both strands of the nine catalog sequences, 1 % substitutions, 0.5 % N, mixed case
    (as tests/test_jf_order.py makes them)."""
    rng = np.random.default_rng(seed)
    seqs = [ko.read_fasta_concat(os.path.join(CATALOG, f)).encode() for f in sorted(os.listdir(CATALOG))]
    reads = []
    for _ in range(n_reads):
        s = seqs[int(rng.integers(len(seqs)))]
        ln = min(int(rng.integers(30, 151)), len(s))
        a = int(rng.integers(0, len(s) - ln + 1))
        r = s[a:a + ln]
        if rng.integers(2):
            r = r.translate(_COMP)[::-1]
        r = np.frombuffer(r, np.uint8).copy()
        sub = rng.random(ln) < 0.01
        r[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(sub.sum()))]
        r[rng.random(ln) < 0.005] = ord("N")
        r[rng.random(ln) < 0.2] |= 0x20
        reads.append(r.tobytes())
    return reads


def counted_model(reads, k, lower=1):
    """(keys sorted, counts) of the canonical k-mers of `reads`, from the definition: every window of k bases,
    either case; any other byte breaks a window, and so does a read's end."""
    code = np.full(256, 4, np.uint8)
    for ch, v in zip(b"ACGTacgt", (0, 1, 2, 3) * 2):
        code[ch] = v
    codes = code[np.frombuffer(b"\n".join(reads), np.uint8)]
    n = codes.size - k + 1
    keys, bad = np.zeros(n, np.uint64), np.zeros(n, bool)
    for j in range(k):
        c = codes[j:j + n]
        bad |= c > 3
        keys = (keys << np.uint64(2)) | (c & 3).astype(np.uint64)
    u, cnt = np.unique(jr.canonical_np(keys[~bad], k), return_counts=True)
    return u[cnt >= lower], cnt[cnt >= lower].astype(np.uint32)


@pytest.mark.gpu
def test_gpu_reads_and_records_on_one_counter(tmp_path):
    reads = make_reads(75, 1500)
    first, second, third = reads[:600], reads[600:1100], reads[1100:]
    p = write_file(tmp_path / "second.jf", *counted_model(second, 31), 31)
    fasta = b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(third))
    seen = {}

    def feed(c):
        c.add_bases(b"\n".join(first))                                  # stays staged: add_jf has to flush it first
        c.add_jf(p)
        assert c.add_text(fasta, final=True) == len(fasta)
        seen.update(c.stats())
    got = merged_on_gpu(feed)
    want = counted_model(reads, 31)
    assert same(got[:2], want)
    text_only = counted_model(first + third, 31)
    assert seen["kmers"] == int(text_only[1].sum(dtype=np.uint64)) and seen["distinct"] == want[0].size
    assert got[3]["records_in"] == counted_model(second, 31)[0].size


@pytest.mark.gpu
def test_gpu_every_producer_on_one_counter_at_the_smallest_staging(tmp_path, monkeypatch):
    """Text, FASTQ and records take turns on one counter whose staging buffers have the smallest size there is
    (256 bytes: no multiple of the 12-byte record), and the file leaves through the same two buffers.  Every call
    is a segment of its own: no k-mer spans two calls or two kinds."""
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "256")
    rng = np.random.default_rng(77)
    q = ord("5")
    reads = make_reads(77, 45)
    fasta = b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads))
    first = 3000                                                        # of the FASTA: what the calls before the last see
    acgt = np.frombuffer(b"ACGT", np.uint8)
    recs = [tq.record(b"q%d" % i, acgt[rng.integers(0, 4, 40)].tobytes(), tq.qualities(rng, 40).tobytes())
            for i in range(80)]
    fastq = b"".join(recs)
    fq_first = len(b"".join(recs[:60])) + 17                            # ends inside record 60
    bases = acgt[rng.integers(0, 4, 500)].tobytes()
    text_models = [counted_model(reads, 31), tq.model_fastq(fastq, q, 31, True), tq.model(bases, 31, True)]
    assert first + 100 < len(fasta) and max(len(r) for r in recs) < 256
    assert not same(text_models[1], tq.model_fastq(fastq, 0, 31, True)) and text_models[1][0].size > 100
    # records: keys the text has too, keys of their own, a fifth of them twice, some with count 0
    keys = np.concatenate([text_models[0][0][:30], jr.canonical_np(random_keys(rng, 50, 31), 31)])
    keys = np.concatenate([keys, keys[:20]])
    counts = rng.integers(1, 1000, keys.size).astype(np.uint32)
    counts[::9] = 0
    jf_keys = np.concatenate([text_models[1][0][:25], jr.canonical_np(random_keys(rng, 75, 31), 31)])
    jf_counts = rng.integers(1, 1000, jf_keys.size).astype(np.uint32)
    jf_counts[::11] = 0
    path = write_file(tmp_path / "in.jf", jf_keys, jf_counts, 31)
    assert keys.size == 100 and jf_keys.size == 100 and keys.size * 12 > 4 * 256
    want = merged_model(text_models + [(keys, counts), (jf_keys, jf_counts)], "sum")

    c = kmlib.Counter(k=31, canonical=True)
    try:
        pos, tail, calls = 0, b"", 0
        while pos < first:                                              # about a dozen pieces that overlap by k - 1
            buf = tail + fasta[pos:min(pos + 700, first)]
            pos += 700
            used = c.add_text(buf, final=False)
            tail, calls = buf[used:], calls + 1
        assert calls == 5 and 0 < len(tail) < 200
        used = c.add_fastq(fastq[:fq_first], final=False, min_qual_char=q)
        assert used == fq_first - 17
        c.add_records(keys, counts)
        c.add_bases(bases)                                              # its end stays staged
        assert c.add_jf(path) == 100
        assert c.add_fastq(fastq[used:], final=True, min_qual_char=q) == len(fastq) - used
        rest = tail + fasta[first:]
        assert c.add_text(rest, final=True) == len(rest)
        stats, merge = c.stats(), c.merge_stats()
        c.finish().close()
        got = c.records()
        out = str(tmp_path / "out.jf")
        c.write_jf(out)
    finally:
        c.close()
    order = np.argsort(got[0], kind="stable")
    assert same((got[0][order], got[1][order]), want)
    assert stats["kmers"] == sum(int(m[1].sum(dtype=np.uint64)) for m in text_models)
    assert stats["distinct"] == want[0].size
    assert merge["records_in"] == int((counts > 0).sum()) + int((jf_counts > 0).sum())
    rec = jr.read_jf(out)
    order = np.argsort(rec["keys"], kind="stable")
    assert (rec["k"], rec["canonical"]) == (31, True) and same((rec["keys"][order], rec["counts"][order]), want)
    assert os.path.getsize(out) > 40 * 256                              # the file left in many pieces


@pytest.mark.gpu
def test_gpu_timed_runs_change_nothing_and_report_something(monkeypatch):
    """KM_COUNT_TIME_FASTQ and KM_COUNT_TIME_MERGE put an event pair around every piece's kernels: the records stay
    what they are, an untimed run reports 0, a timed one a time that only grows.  No bound on the times."""
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")
    rng = np.random.default_rng(78)
    q = ord("+")
    text, _ = tq.small_text()
    keys = jr.canonical_np(random_keys(rng, 2000, 31), 31)
    counts = rng.integers(0, 1000, keys.size).astype(np.uint32)
    assert len(text) > 5 * 4096 and keys.size * 12 > 5 * 4096            # several spans each
    want = merged_model([tq.small_want(q, 31, True)] * 2 + [(keys, counts)] * 2, "sum")
    for time_fastq, time_merge in ((False, False), (True, False), (False, True), (True, True)):
        monkeypatch.delenv("KM_COUNT_TIME_FASTQ", raising=False)
        monkeypatch.delenv("KM_COUNT_TIME_MERGE", raising=False)
        if time_fastq:
            monkeypatch.setenv("KM_COUNT_TIME_FASTQ", "1")
        if time_merge:
            monkeypatch.setenv("KM_COUNT_TIME_MERGE", "1")
        c = kmlib.Counter(k=31, canonical=True)
        try:
            seen = []
            for _ in range(2):
                assert c.add_fastq(text, final=True, min_qual_char=q) == len(text)
                c.add_records(keys, counts)
                seen.append((c.fastq_kernel_ms(), c.merge_stats()["kernel_ms"]))
                assert (c.fastq_kernel_ms(), c.merge_stats()["kernel_ms"]) == seen[-1]   # no new piece: the same
            c.finish().close()
            assert c.fastq_kernel_ms() == seen[-1][0]                   # what was measured outlives the scratch
            got = c.records()
        finally:
            c.close()
        order = np.argsort(got[0], kind="stable")
        assert same((got[0][order], got[1][order]), want), (time_fastq, time_merge)
        for which, timed in ((0, time_fastq), (1, time_merge)):
            first, second = seen[0][which], seen[1][which]
            if timed:
                assert np.isfinite(first) and np.isfinite(second) and 0 < first <= second, (which, seen)
            else:
                assert first == 0.0 and second == 0.0, (which, seen)


@pytest.mark.gpu
def test_gpu_errors_leave_the_counter_as_it_was(tmp_path):
    rng = np.random.default_rng(76)
    keys = np.unique(random_keys(rng, 300, 31))[:256]
    counts = np.arange(1, 257, dtype=np.uint32)
    good = write_file(tmp_path / "good.jf", keys, counts, 31)
    other_k = write_file(tmp_path / "k21.jf", keys & np.uint64((1 << 42) - 1), counts, 21)
    other_c = write_file(tmp_path / "noncanonical.jf", keys, counts, 31, canonical=False)
    empty = write_file(tmp_path / "empty.jf", [], [], 31)
    c = kmlib.Counter(k=31, canonical=True)
    assert c.add_jf(good) == 256 and c.stats()["distinct"] == 256
    for call, code, named in ((lambda: c.add_records(keys + np.uint64(1), counts, mode=2), 4, ["mode 2"]),
                              (lambda: c.add_records(keys + np.uint64(1), counts, mode=-1), 4, ["mode -1"]),
                              (lambda: c.add_jf(good, mode=7), 4, ["mode 7"]),
                              (lambda: c.add_jf(other_k), 4, [other_k, "k=21", "k=31"]),
                              (lambda: c.add_jf(other_c), 4, [other_c, "canonical=0", "canonical=1"]),
                              (lambda: c.add_jf(str(tmp_path / "no_such.jf")), 1, ["no_such.jf"]),
                              (lambda: c.add_jf(os.path.join(CATALOG, "IDH1_R132.fa")), 2, [])):
        with pytest.raises(kmlib.KmError) as e:
            call()
        assert e.value.code == code and all(word in str(e.value) for word in named), str(e.value)
        assert c.stats()["distinct"] == 256
        c.add_records(keys[:1], counts[:1])                              # the next valid call works
        assert c.stats()["distinct"] == 256
    assert c.add_jf(empty) == 0                                          # KM_OK, nothing launched
    c.add_records(np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    assert c.merge_stats()["records_in"] == 256 + 7
    c.finish(1).close()
    got_keys, got_counts = c.records()
    want = merged_model([(keys, counts)] + [(keys[:1], counts[:1])] * 7, "sum")
    order = np.argsort(got_keys)
    assert same((got_keys[order], got_counts[order]), want)
    for call in (lambda: c.add_jf(good), lambda: c.add_records(keys, counts)):
        with pytest.raises(kmlib.KmError) as e:
            call()
        assert e.value.code == 7                                         # KM_E_STATE
    c.close()


@pytest.mark.gpu
def test_gpu_through_the_tools(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system")
    for name in (ITD, TKD):
        shutil.copy(os.path.join(JF_DIR, name), tmp_path / name)

    def km(*args):
        res = subprocess.run([sys.executable, "-m", "km_amd"] + list(args), cwd=tmp_path, capture_output=True,
                             text=True, timeout=300, env=env)
        assert res.returncode == 0, res.stderr
        return res

    inputs = [fixture(ITD), fixture(TKD)]
    err = km("merge", "-o", "m.jf", ITD, TKD).stderr
    km("merge", "--jellyfish-order", "-o", "j.jf", ITD, TKD)
    km("merge", "-L", "2", "--max", "-o", "x.jf", ITD, TKD)
    want = merged_model(inputs, "sum")
    stats = dict(line[1:].split(":") for line in err.splitlines() if line.startswith("#"))
    assert set(stats) == {"distinct", "slots", "n_grow", "records_in", "mode"} and stats["mode"] == "sum"
    assert int(stats["distinct"]) == want[0].size and int(stats["records_in"]) == sum(k.size for k, _ in inputs)
    rec = jr.read_jf(str(tmp_path / "m.jf"))
    assert (rec["k"], rec["canonical"]) == (31, True) and same((rec["keys"], rec["counts"]), want)
    assert rec["header"]["cmdline"] == ["km_amd", "merge", "-L", "1", "-o", "m.jf", ITD, TKD]
    cut = jr.read_jf(str(tmp_path / "x.jf"))
    want_max = merged_model(inputs, "max", lower=2)
    assert same((cut["keys"], cut["counts"]), want_max) and want_max[0].size > 0
    # Jellyfish's order: ascending (position, key) under the file's own matrix, the same records
    jf = jr.read_jf(str(tmp_path / "j.jf"))
    m = jf["header"]["matrix1"]
    pos = model_pos(jf["keys"], np.array(m["columns"], np.uint64), m["r"])
    assert np.array_equal(np.lexsort((jf["keys"], pos)), np.arange(jf["keys"].size))
    order = np.argsort(jf["keys"])
    assert same((jf["keys"][order], jf["counts"][order]), want) and not np.array_equal(jf["keys"], want[0])
    # find_mutation on the merged file: the oracle on the model's records, byte for byte
    cpu = ko.KmerDB(records={"k": 31, "canonical": True, "keys": want[0], "counts": want[1]}, cutoff=0.05, n_cutoff=5)
    for target in ("FLT3-ITD_exons_13-15", "FLT3-TKD_exon_20"):
        fa = os.path.join(CATALOG, target + ".fa")
        rows = ko.target_rows(ko.analyse_target(ko.read_fasta_concat(fa), target, cpu), "m.jf")
        body = [ln for ln in km("find_mutation", fa, "m.jf").stdout.splitlines() if not ln.startswith("#")]
        assert body[0].startswith("Database\t") and body[1:] == rows and len(rows) >= 1
