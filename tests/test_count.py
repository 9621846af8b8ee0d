"""Counting k-mers from reads (km_counter_*, km_amd.lib.Counter, km_amd.count, `python -m km_amd count`).

Every comparison is exact.  The model the GPU is compared against is written here from the definition: sliding
windows over the same bytes, a break at every byte outside ACGTacgt, 2-bit keys (first base most significant),
oracle.jf_reader.canonical_np for the canonical form, np.unique for the counts.  It shares no code with the
kernel or with the text stripper."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from km_amd import count as kc
from km_amd import lib as kmlib
from oracle import jf_reader as jr
from oracle import km_oracle as ko

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CATALOG = os.path.join(HERE, "data", "catalog", "GRCh38")
FLT3 = os.path.join(CATALOG, "FLT3-ITD_exons_13-15.fa")

_CODE = np.full(256, 4, np.uint8)
for _ch, _c in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
    _CODE[_ch] = _c
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


# ------------------------------------------------------------------ the model
def model(data, k, canonical):
    """(keys sorted, counts) of every window of k bases in `data` (bytes); any other byte is a break."""
    codes = _CODE[np.frombuffer(bytes(data), np.uint8)]
    n = codes.size - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    keys = np.zeros(n, np.uint64)
    bad = np.zeros(n, bool)
    for j in range(k):
        c = codes[j:j + n]
        bad |= c > 3
        keys = (keys << np.uint64(2)) | (c & 3).astype(np.uint64)
    keys = keys[~bad]
    if canonical:
        keys = jr.canonical_np(keys, k)
    u, c = np.unique(keys, return_counts=True)
    return u, c.astype(np.uint32)


def cut(keys, counts, lower):
    keep = counts >= lower
    return keys[keep], counts[keep]


def sorted_records(counter):
    keys, counts = counter.records()
    order = np.argsort(keys, kind="stable")
    return keys[order], counts[order]


def same(a, b):
    return a[0].dtype == b[0].dtype and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def catalog_sequences():
    return [ko.read_fasta_concat(os.path.join(CATALOG, f)).encode() for f in sorted(os.listdir(CATALOG))]


def make_reads(seed, n_reads=20_000):
    """Reads of 30-150 nt from both strands of the nine catalog sequences, 1 % substitutions, 0.5 % N, mixed
    case; some are shorter than k."""
    rng = np.random.default_rng(seed)
    seqs = catalog_sequences()
    assert len(seqs) == 9
    reads = []
    for _ in range(n_reads):
        s = seqs[int(rng.integers(9))]
        ln = min(int(rng.integers(30, 151)), len(s))
        a = int(rng.integers(0, len(s) - ln + 1))
        r = s[a:a + ln]
        if rng.integers(2):
            r = r.translate(_COMP)[::-1]
        r = np.frombuffer(r, np.uint8).copy()
        sub = rng.random(ln) < 0.01
        r[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(sub.sum()))]
        r[rng.random(ln) < 0.005] = ord("N")
        lower = rng.random(ln) < 0.2
        r[lower] |= 0x20
        reads.append(r.tobytes())
    return reads


def as_fastq(reads, rng, crlf=False):
    """4-line FASTQ whose quality lines are made of ACGT@>+ only."""
    nl = b"\r\n" if crlf else b"\n"
    qual = np.frombuffer(b"ACGT@>+", np.uint8)
    out = []
    for i, r in enumerate(reads):
        q = qual[rng.integers(0, qual.size, len(r))].tobytes()
        out.append(b"@read%d extra" % i + nl + r + nl + b"+" + nl + q + nl)
    return b"".join(out)


def random_bases(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]


# ------------------------------------------------------------------ CPU: file writer
@pytest.mark.parametrize("k", [31, 21, 5])
def test_write_records_round_trip(tmp_path, k):
    rng = np.random.default_rng(k)
    top = (1 << (2 * k)) - 1
    keys = np.unique(rng.integers(0, top, 5000 if k > 5 else 700, dtype=np.uint64, endpoint=True))
    counts = rng.integers(1, 1 << 32, keys.size, dtype=np.uint64).astype(np.uint32)
    counts[:3] = (1, 65535, 0xFFFFFFFF)
    p1, p2 = str(tmp_path / "a.jf"), str(tmp_path / "b.jf")
    perm = rng.permutation(keys.size)
    kc.write_records(p1, keys[perm], counts[perm], k, True)
    perm = rng.permutation(keys.size)
    kc.write_records(p2, keys[perm], counts[perm], k, True)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    rec = jr.read_jf(p1)
    assert rec["k"] == k and rec["canonical"] is True
    assert np.array_equal(rec["keys"], keys) and np.array_equal(rec["counts"], counts)
    assert rec["header"]["counter_len"] == 4 and rec["header"]["cmdline"][:2] == ["km_amd", "count"]
    db = kmlib.Database.open(p1)
    got_k, got_c = db.records()
    assert np.array_equal(got_k, keys) and np.array_equal(got_c, counts)
    assert db.info.k == k and db.info.canonical == 1 and db.info.n_records == keys.size
    db.close()
    kc.write_records(p2, keys, counts, k, False)
    assert jr.read_jf(p2)["canonical"] is False
    db = kmlib.Database.open(p2)
    assert db.info.canonical == 0
    db.close()


# ------------------------------------------------------------------ CPU: the text stripper alone
def test_strip_fasta_and_fastq_cases():
    fa = b">h1 some text\nACGTNN\nacgt\n\n>h2\r\nTT\r\nGG\r\n>h3 no sequence\n>h4\nA"
    assert kmlib.strip_text(fa)[0] == b"ACGTNNacgt\nTTGG\nA\n"
    fq = (b"@r1\nACGTNAC\n+\nACGT@>+\n"            # a quality line of bases and header characters
          b"@r2\r\nacgt\r\n+r2\r\n@>+A\r\n"           # \r\n, and a quality line that starts with '@'
          b"@r3\n\n+\n\n"                            # an empty sequence
          b"@r4\nGGGG\n+\nAAAA")                     # no newline at the end
    assert kmlib.strip_text(fq)[0] == b"ACGTNAC\nacgt\n\nGGGG\n"
    assert kmlib.strip_text(b"")[0] == b""
    assert kmlib.strip_text(b"\n\n>x\nAC\n")[0] == b"AC\n"


def test_strip_every_split_point_gives_the_same_stream():
    rng = np.random.default_rng(5)
    reads = [random_bases(rng, int(rng.integers(0, 60))).tobytes() for _ in range(80)]
    fq = as_fastq(reads[:14], rng) + as_fastq(reads[14:40], rng, crlf=True)
    fa = b"".join(b">rec %d\n" % i + b"\n".join(r[j:j + 17] for j in range(0, len(r), 17)) + b"\n"
                  for i, r in enumerate(reads))
    for text in (fq[:2048], fa[:2048]):
        assert len(text) == 2048
        whole = kmlib.strip_text(text)[0]
        assert whole.count(b"\n") > 10
        for at in range(len(text) + 1):
            first, used, st = kmlib.strip_text(text[:at], final=False)
            assert used <= at
            second, used2, _ = kmlib.strip_text(text[used:], final=True, state=st)
            assert used2 == len(text) - used
            assert first + second == whole, at


def test_strip_format_errors_name_the_offset():
    with pytest.raises(kmlib.KmError) as e:
        kmlib.strip_text(b"@r1\nACGT\n+\nIIII\n@r2\nACGT\nIIII\n@r3\nAC\n+\nII\n")
    assert e.value.code == 2 and "'+'" in str(e.value) and "offset 25" in str(e.value)
    # the same across two calls: the offset counts from the start of the stream
    first, used, st = kmlib.strip_text(b"@r1\nACGT\n+\nIIII\n@r2\nAC", final=False)
    assert (first, used) == (b"ACGT\n", 20)
    with pytest.raises(kmlib.KmError) as e:
        kmlib.strip_text(b"ACGT\nIIII\n", final=True, state=st)
    assert e.value.code == 2 and "offset 25" in str(e.value)
    with pytest.raises(kmlib.KmError) as e:
        kmlib.strip_text(b"@r1\nACGT\n")                      # the stream ends where the '+' line should be
    assert e.value.code == 2 and "offset 9" in str(e.value)
    with pytest.raises(kmlib.KmError) as e:
        kmlib.strip_text(b"ACGT\n")
    assert e.value.code == 2 and "offset 0" in str(e.value)


def test_argument_errors_before_any_hip_call():
    lib = kmlib.load()
    h = C.c_void_p()
    n = C.c_uint64()
    buf = np.frombuffer(b"ACGT", np.uint8)
    for k in (-1, 0, 1, 33, 64):
        assert lib.km_counter_create(0, k, 1, 0, C.byref(h)) == 3
    assert lib.km_counter_create(0, 31, 1, 0, None) == 4
    assert lib.km_counter_create(-1, 31, 1, 0, C.byref(h)) == 4
    assert lib.km_counter_add_bases(None, kmlib.ptr(buf), 4) == 4
    assert lib.km_counter_add_text(None, kmlib.ptr(buf), 4, 1, C.byref(n)) == 4
    assert lib.km_counter_stats(None, None) == 4
    assert lib.km_counter_finish(None, 1, C.byref(h)) == 4
    assert lib.km_counter_records(None, None, None, 0, C.byref(n)) == 4
    assert lib.km_counter_destroy(None) == 0
    st = kmlib.TextState()
    out = np.zeros(8, np.uint8)
    assert lib.km_text_strip(None, kmlib.ptr(buf), 4, 1, kmlib.ptr(out), 8, C.byref(n), C.byref(n)) == 4
    assert lib.km_text_strip(C.byref(st), kmlib.ptr(buf), 4, 1, None, 8, C.byref(n), C.byref(n)) == 4
    assert lib.km_text_strip(C.byref(st), kmlib.ptr(buf), 4, 1, kmlib.ptr(out), 4, C.byref(n), C.byref(n)) == 8
    with pytest.raises(ValueError):
        kc.write_records(os.devnull, np.zeros(2, np.uint64), np.zeros(3, np.uint32), 31, True)


# ------------------------------------------------------------------ GPU 1: counts equal the model
def count_bases(data, k, canonical, lower=1, **kw):
    c = kmlib.Counter(k=k, canonical=canonical, **kw)
    c.add_bases(data)
    stats = c.stats()
    db = c.finish(lower)
    rec = sorted_records(c)
    c.close()
    return rec, stats, db


@pytest.mark.gpu
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [31, 21, 32])
def test_gpu_reads_equal_the_model(k, canonical):
    data = b"\n".join(make_reads(41))
    want = model(data, k, canonical)
    got, stats, db = count_bases(data, k, canonical)
    assert same(got, want)
    assert stats["kmers"] == int(want[1].sum(dtype=np.uint64)) and stats["distinct"] == want[0].size
    assert stats["bases"] == int((_CODE[np.frombuffer(data, np.uint8)] < 4).sum())
    assert db.info.n_records == want[0].size
    db.close()


@pytest.mark.gpu
def test_gpu_k32_noncanonical_counts_the_all_t_kmer():
    """T^32 has the key ~0, the table's empty marker: it is counted beside the table."""
    data = b"T" * 40 + b"\nACGT" + b"T" * 32 + b"\n" + b"A" * 33
    for canonical in (False, True):
        want = model(data, 32, canonical)
        got, stats, db = count_bases(data, 32, canonical)
        assert same(got, want) and stats["distinct"] == want[0].size
        assert np.array_equal(db.query(want[0]), want[1])
        db.close()
    assert int(model(data, 32, False)[0][-1]) == 0xFFFFFFFFFFFFFFFF


@pytest.mark.gpu
def test_gpu_k5_every_key_and_counts_above_the_16_bit_escape():
    rng = np.random.default_rng(42)
    data = np.concatenate([random_bases(rng, 2_800_000), np.full(200_000, ord("A"), np.uint8)]).tobytes()
    want = model(data, 5, True)
    assert want[0].size == 512 and int(want[1].min()) >= 1000 and int(want[1].max()) >= 65_535
    got, stats, db = count_bases(data, 5, True)
    assert same(got, want)
    assert np.array_equal(db.query(want[0]), want[1])
    assert np.array_equal(db.query(jr.revcomp_np(want[0], 5)), want[1])
    db.close()


@pytest.mark.gpu
def test_gpu_one_call_many_calls_and_fastq_blocks_agree(monkeypatch):
    reads = make_reads(43)
    want = model(b"\n".join(reads), 31, True)
    one, _, db = count_bases(b"\n".join(reads), 31, True)
    db.close()
    many = kmlib.Counter(k=31)
    for i in range(0, len(reads), 20):                      # 1 000 calls
        many.add_bases(b"\n".join(reads[i:i + 20]))
    many.finish().close()
    rng = np.random.default_rng(44)
    text = as_fastq(reads, rng)
    blocks = kmlib.Counter(k=31)
    pos, tail = 0, b""
    while pos < len(text):
        step = int(rng.integers(1, 200_000))
        buf = tail + text[pos:pos + step]
        pos += step
        used = blocks.add_text(buf, final=False)
        tail = buf[used:]
    blocks.add_text(tail, final=True)
    blocks.finish().close()
    # and with a staging buffer of 4 kB: hundreds of pieces, reads across every cut
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")
    small, _, db = count_bases(b"\n".join(reads), 31, True)
    db.close()
    for got in (one, sorted_records(many), sorted_records(blocks), small):
        assert same(got, want)
    many.close()
    blocks.close()


@pytest.mark.gpu
def test_gpu_growth_and_a_generous_size_give_the_same_records():
    rng = np.random.default_rng(45)
    data = random_bases(rng, 1_500_000)
    data[rng.integers(0, data.size, 3000)] = ord("\n")
    data = data.tobytes()
    want = model(data, 31, True)
    assert want[0].size > 1_000_000
    grown, stats, db = count_bases(data, 31, True, expected_distinct=0)
    db.close()
    assert stats["n_grow"] >= 3 and same(grown, want)
    roomy, stats, db = count_bases(data, 31, True, expected_distinct=4_000_000)
    db.close()
    assert stats["n_grow"] == 0 and stats["slots"] == 1 << 23 and same(roomy, want)


@pytest.mark.gpu
def test_gpu_input_larger_than_one_staging_buffer():
    """17 M bytes through 16 MiB staging buffers: two pieces, with a read lying across the cut."""
    rng = np.random.default_rng(46)
    stage = 16 << 20
    data = random_bases(rng, 17_000_000)
    data[rng.integers(0, data.size, 170_000)] = ord("\n")
    data[stage - 60:stage + 60] = random_bases(rng, 120)
    data = data.tobytes()
    want = model(data, 31, True)
    got, stats, db = count_bases(data, 31, True)
    db.close()
    assert same(got, want)
    assert stats["kmers"] == int(want[1].sum(dtype=np.uint64))
    assert stats["bases"] == int((_CODE[np.frombuffer(data, np.uint8)] < 4).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("lower", [1, 2, 5])
def test_gpu_lower_count(lower):
    data = b"\n".join(make_reads(47, 5000))
    want = cut(*model(data, 31, True), lower)
    got, stats, db = count_bases(data, 31, True, lower=lower)
    assert same(got, want) and db.info.n_records == want[0].size
    assert stats["distinct"] == model(data, 31, True)[0].size
    db.close()


@pytest.mark.gpu
def test_gpu_call_order_is_checked():
    c = kmlib.Counter(k=31)
    c.add_bases(b"")
    assert c.add_text(b"", final=False) == 0
    assert c.stats()["kmers"] == 0
    with pytest.raises(kmlib.KmError) as e:
        c.records()
    assert e.value.code == 7
    db = c.finish()
    assert db.info.n_records == 0
    for call in (lambda: c.add_bases(b"ACGT"), lambda: c.add_text(b">x\nAC\n"), lambda: c.finish()):
        with pytest.raises(kmlib.KmError) as e:
            call()
        assert e.value.code == 7
    assert c.records()[0].size == 0
    db.close()
    c.close()


# ------------------------------------------------------------------ GPU 2: finish gives a working database
@pytest.mark.gpu
@pytest.mark.parametrize("canonical", [True, False])
def test_gpu_finish_gives_a_working_database(canonical):
    data = b"\n".join(make_reads(48))
    want = model(data, 31, canonical)
    _, _, db = count_bases(data, 31, canonical)
    assert db.info.n_records == want[0].size and db.info.k == 31 and db.info.canonical == int(canonical)
    assert np.array_equal(db.query(want[0]), want[1])
    if canonical:
        assert np.array_equal(db.query(jr.revcomp_np(want[0], 31)), want[1])
    rng = np.random.default_rng(49)
    absent = rng.integers(0, 1 << 62, 10_000, dtype=np.uint64)
    probe = jr.canonical_np(absent, 31) if canonical else absent
    absent = absent[~np.isin(probe, want[0])]
    assert absent.size > 9_990 and not db.query(absent).any()
    db.close()


# ------------------------------------------------------------------ GPU 3 + 4: end to end against the oracle
def itd_reads(seed=50, depth=120, read_len=100, fraction=0.3):
    """Reads tiling the FLT3 target at a seeded depth; a fraction carries a 30-nt tandem duplication."""
    rng = np.random.default_rng(seed)
    ref = ko.read_fasta_concat(FLT3)
    p = 150
    itd = ref[:p + 30] + ref[p:p + 30] + ref[p + 30:]
    pad = "".join("ACGT"[i] for i in rng.integers(0, 4, 200))
    reads = []
    for _ in range(depth * (len(ref) + 2 * read_len) // read_len):
        src = pad[:100] + (itd if rng.random() < fraction else ref) + pad[100:]
        a = int(rng.integers(0, len(src) - read_len + 1))
        r = src[a:a + read_len]
        if rng.integers(2):
            r = r.encode().translate(_COMP)[::-1].decode()
        reads.append(r.encode())
    return ref, reads


def oracle_rows(ref, reads, db_name):
    keys, counts = cut(*model(b"\n".join(reads), 31, True), 2)
    cpu = ko.KmerDB(records={"k": 31, "canonical": True, "keys": keys, "counts": counts}, cutoff=0.05, n_cutoff=5)
    rows = ko.target_rows(ko.analyse_target(ref, "FLT3-ITD_exons_13-15", cpu), db_name)
    assert any(r.split("\t")[2] == "ITD" for r in rows), rows
    return rows, keys


@pytest.mark.gpu
def test_gpu_counted_database_through_batchfinder_equals_the_oracle():
    from km_amd.finder import BatchFinder
    from km_amd.jellyfish import Jellyfish
    ref, reads = itd_reads()
    want, keys = oracle_rows(ref, reads, "counted.jf")
    c = kmlib.Counter(k=31, canonical=True)
    c.add_text(as_fastq(reads, np.random.default_rng(51)), final=True)
    db = c.finish(2)
    c.close()
    assert db.info.n_records == keys.size
    jf = Jellyfish("counted.jf", cutoff=0.05, n_cutoff=5, device=0, db=db)
    rows = BatchFinder(jf).rows([("FLT3-ITD_exons_13-15", ref)])[0]
    assert rows == want
    db.close()


@pytest.mark.gpu
def test_gpu_cli_count_then_find_mutation(tmp_path):
    ref, reads = itd_reads()
    fq = tmp_path / "reads.fq.gz"
    with gzip.open(fq, "wb") as fh:
        fh.write(as_fastq(reads, np.random.default_rng(52)))
    env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, "-m", "km_amd", "count", "-m", "31", "-C", "-L", "2", "-o", "x.jf",
                          "reads.fq.gz"], cwd=tmp_path, capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stderr
    full = model(b"\n".join(reads), 31, True)
    stats = dict(line[1:].split(":") for line in res.stderr.splitlines() if line.startswith("#"))
    assert int(stats["kmers"]) == int(full[1].sum(dtype=np.uint64)) and int(stats["distinct"]) == full[0].size
    assert set(stats) == {"bases", "kmers", "distinct", "slots", "n_grow"}
    want, keys = oracle_rows(ref, reads, "x.jf")
    rec = jr.read_jf(str(tmp_path / "x.jf"))
    assert rec["k"] == 31 and rec["canonical"] is True and np.array_equal(rec["keys"], keys)
    assert np.array_equal(rec["counts"], cut(*full, 2)[1])
    res = subprocess.run([sys.executable, "-m", "km_amd", "find_mutation", FLT3, "x.jf"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stderr
    body = [ln for ln in res.stdout.splitlines() if not ln.startswith("#")]
    assert body[1:] == want and body[0].startswith("Database\t")
    # the file loaded straight into HBM and the database counted in memory have the same table
    c = kmlib.Counter(k=31)
    c.add_bases(b"\n".join(reads))
    mem = c.finish(2)
    c.close()
    disk = kmlib.Database.load(str(tmp_path / "x.jf"))
    for field in ("k", "canonical", "n_records", "n_slots", "n_groups", "table_bytes", "max_probe"):
        assert getattr(mem.info, field) == getattr(disk.info, field), field
    mem.close()
    disk.close()
