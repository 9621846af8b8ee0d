"""Files in Jellyfish's own record order (km_jf_*, km_counter_write_jf, km_amd.count.write_jellyfish,
`python -m km_amd count --jellyfish-order`).

Every comparison is exact.  The model is written here from the definition and shares no code with the kernels:
pos(key) = XOR over the set bits i of key of columns[c - 1 - i], masked with size - 1; the order is
np.lexsort((key, pos)); a record is ceil(2k / 8) little-endian key bytes and 4 count bytes, as oracle.jf_reader
reads them.  The rule itself is pinned on the five files real Jellyfish 2.2.3 wrote (tests/data/jf); those have no
two records with one position, so the tie-break (ascending key) is this project's reading of Jellyfish, not a
pinned fact."""
import ctypes as C
import json
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
JF_DIR = os.path.join(HERE, "data", "jf")
FIXTURES = sorted(f for f in os.listdir(JF_DIR) if f.endswith(".jf"))
CATALOG = os.path.join(HERE, "data", "catalog", "GRCh38")
FLT3 = os.path.join(CATALOG, "FLT3-ITD_exons_13-15.fa")
HEADER_KEYS = {"alignment", "canonical", "cmdline", "counter_len", "format", "key_len", "matrix1", "max_reprobe",
               "reprobes", "size", "val_len"}
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


# ------------------------------------------------------------------ the model
def model_pos(keys, columns, size_log2):
    keys = np.asarray(keys, np.uint64)
    columns = np.asarray(columns, np.uint64)
    c = columns.size
    pos = np.zeros(keys.size, np.uint64)
    for i in range(c):
        bit = ((keys >> np.uint64(i)) & np.uint64(1)).astype(bool)
        pos ^= np.where(bit, columns[c - 1 - i], np.uint64(0))
    return pos & np.uint64((1 << size_log2) - 1)


def record_bytes(keys, counts, k):
    kb = (2 * k + 7) // 8
    rec = np.zeros((len(keys), kb + 4), np.uint8)
    for b in range(kb):
        rec[:, b] = ((keys >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8)
    for b in range(4):
        rec[:, kb + b] = ((counts >> np.uint32(8 * b)) & np.uint32(0xFF)).astype(np.uint8)
    return rec


def model(keys, counts, columns, k, size_log2):
    """(records uint8[n, rec], pos[n]) in file order."""
    keys = np.asarray(keys, np.uint64)
    counts = np.asarray(counts, np.uint32)
    pos = model_pos(keys, columns, size_log2)
    order = np.lexsort((keys, pos))
    return record_bytes(keys[order], counts[order], k), pos[order]


def gf2_rank(columns):
    basis, rank = {}, 0
    for v in (int(x) for x in columns):
        while v:
            b = v.bit_length() - 1
            if b not in basis:
                basis[b] = v
                rank += 1
                break
            v ^= basis[b]
    return rank


def read_fixture(name):
    path = os.path.join(JF_DIR, name)
    rec = jr.read_jf(path)
    raw = open(path, "rb").read()
    _, off = jr.parse_header(raw)
    m = rec["header"]["matrix1"]
    assert (m["r"], m["c"], rec["header"]["size"], rec["k"]) == (32, 62, 1 << 32, 31)
    return rec, np.array(m["columns"], np.uint64), raw[off:]


def distinct_keys(rng, n, k):
    top = (1 << (2 * k)) - 1
    keys = np.unique(rng.integers(0, top, n + n // 4 + 16, dtype=np.uint64, endpoint=True))
    assert keys.size >= n
    return rng.permutation(keys)[:n]


def any_counts(rng, n):
    counts = rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    counts[:3] = (0xFFFFFFFF, 65535, 65536)[:min(n, 3)]
    return counts


def check_against_model(keys, counts, columns, k, size_log2):
    want, want_pos = model(keys, counts, columns, k, size_log2)
    got, pos = kmlib.jf_sort_records(columns, k, size_log2, keys, counts, want_pos=True)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(pos, want_pos)
    assert np.array_equal(got, want)
    return got


# ------------------------------------------------------------------ CPU
def test_matrix_is_deterministic_and_of_full_rank():
    for k, r in ((31, 32), (32, 64), (5, 10), (21, 4), (2, 1)):
        a = kmlib.jf_matrix(k, r, seed=7)
        assert a.dtype == np.uint64 and a.size == 2 * k
        assert np.array_equal(a, kmlib.jf_matrix(k, r, seed=7))
        assert not np.array_equal(a, kmlib.jf_matrix(k, r, seed=8))
        assert all(int(x) >> r == 0 for x in a)
        assert gf2_rank(a) == r
    assert np.array_equal(kmlib.jf_matrix(31, 32), kmlib.jf_matrix(31, 32, seed=0))


def test_argument_errors_before_any_hip_call():
    lib = kmlib.load()
    cols = np.zeros(64, np.uint64)
    for k in (-1, 0, 1, 33):
        assert lib.km_jf_matrix(k, 4, 0, kmlib.ptr(cols)) == 3
    for k, r in ((31, 0), (31, 63), (2, 5), (5, -1)):
        assert lib.km_jf_matrix(k, r, 0, kmlib.ptr(cols)) == 4
    assert lib.km_jf_matrix(31, 32, 0, None) == 4
    keys, counts, out = np.zeros(2, np.uint64), np.zeros(2, np.uint32), np.zeros(24, np.uint8)
    args = (kmlib.ptr(keys), kmlib.ptr(counts), 2, kmlib.ptr(out), None, None)
    assert lib.km_jf_sort_records(0, None, 31, 32, *args) == 4
    assert lib.km_jf_sort_records(0, kmlib.ptr(cols), 33, 32, *args) == 3
    assert lib.km_jf_sort_records(0, kmlib.ptr(cols), 31, 63, *args) == 4
    assert lib.km_jf_sort_records(-1, kmlib.ptr(cols), 31, 32, *args) == 4
    assert lib.km_jf_sort_records(0, kmlib.ptr(cols), 31, 32, None, kmlib.ptr(counts), 2, kmlib.ptr(out), None, None) == 4
    assert lib.km_jf_sort_records(0, kmlib.ptr(cols), 31, 32, kmlib.ptr(keys), kmlib.ptr(counts), 1 << 32,
                                  kmlib.ptr(out), None, None) == 4
    assert lib.km_jf_sort_records(0, kmlib.ptr(cols), 31, 32, None, None, 0, None, None, None) == 0   # no launch
    assert lib.km_jf_sort_stats(None) == 4
    assert lib.km_counter_write_jf(None, b"x.jf", None, 0) == 4
    for k in (-1, 0, 33):                                    # the wrapper leaves the verdict on k to the library
        with pytest.raises(kmlib.KmError) as e:
            kmlib.jf_matrix(k, 4)
        assert e.value.code == 3
    ln, s = C.c_uint64(), C.c_int()
    for bad in (b"", b"[", b"km_amd count", b'["km_amd"', b'"km_amd"]'):      # cmdline_json: an array's brackets
        assert lib.km_jf_header(31, 1, 10, 0, bad, None, 0, C.byref(ln), kmlib.ptr(cols), C.byref(s)) == 4
    assert lib.km_jf_header(31, 1, 10, 0, b"[]", None, 0, C.byref(ln), kmlib.ptr(cols), C.byref(s)) == 0


def test_header_is_a_function_of_its_arguments():
    text, columns, r = kmlib.jf_header(31, True, 1000, cmdline=["km_amd", "count", "a b"], seed=3)
    assert len(text) % 8 == 0 and int(text[:9]) == len(text) - 9
    hdr, off = jr.parse_header(text)
    assert off == len(text) and set(hdr) == HEADER_KEYS
    assert r == 11 and hdr["size"] == 2048 and hdr["key_len"] == 62 and hdr["canonical"] is True
    assert hdr["matrix1"] == {"c": 62, "r": 11, "columns": [int(x) for x in kmlib.jf_matrix(31, 11, seed=3)]}
    assert np.array_equal(columns, kmlib.jf_matrix(31, 11, seed=3))
    assert hdr["cmdline"] == ["km_amd", "count", "a b"] and hdr["format"] == "binary/sorted"
    real = jr.read_jf(os.path.join(JF_DIR, FIXTURES[0]))["header"]
    for key in ("alignment", "counter_len", "max_reprobe", "reprobes", "val_len"):
        assert hdr[key] == real[key], key
    assert set(real) - set(hdr) == {"hostname", "pwd", "time", "exe_path"}
    body = text[9:].rstrip(b"\0").decode()
    assert body == json.dumps(hdr, separators=(",", ":"), sort_keys=True)
    assert kmlib.jf_header(31, True, 1000, cmdline=["km_amd", "count", "a b"], seed=3)[0] == text
    assert jr.parse_header(kmlib.jf_header(31, False, 0)[0])[0]["size"] == 16
    small = jr.parse_header(kmlib.jf_header(2, False, 16)[0])[0]              # capped at 4^k
    assert small["size"] == 16 and small["matrix1"]["r"] == 4 and small["cmdline"] == ["km_amd", "count"]


@pytest.mark.parametrize("name", FIXTURES)
def test_model_reproduces_the_order_of_real_jellyfish_files(name):
    """The pin of the rule (passes without the feature): with the file's own matrix and size the model puts the
    shuffled records back into the file's order, and the other column order does not."""
    rec, columns, area = read_fixture(name)
    n = rec["keys"].size
    assert n >= 200
    perm = np.random.default_rng(1).permutation(n)
    got, pos = model(rec["keys"][perm], rec["counts"][perm], columns, 31, 32)
    assert got.tobytes() == area
    assert np.all(pos[1:] > pos[:-1])                       # strictly: these files do not pin the tie-break
    other = model_pos(rec["keys"], columns[::-1], 32)
    assert not np.all(other[1:] >= other[:-1])


# ------------------------------------------------------------------ GPU: the sort alone
@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_gpu_real_files_round_trip(name):
    rec, columns, area = read_fixture(name)
    perm = np.random.default_rng(2).permutation(rec["keys"].size)
    got, pos = kmlib.jf_sort_records(columns, 31, 32, rec["keys"][perm], rec["counts"][perm], want_pos=True)
    assert got.tobytes() == area
    assert np.all(pos[1:] > pos[:-1])
    assert np.array_equal(pos, model_pos(rec["keys"], columns, 32))


@pytest.mark.gpu
def test_gpu_ties_are_ordered_by_key():
    rng = np.random.default_rng(3)
    keys = np.unique(jr.canonical_np(distinct_keys(rng, 700, 31), 31))[:600]
    keys = rng.permutation(keys)
    assert keys.size == 600
    columns = kmlib.jf_matrix(31, 6, seed=1)
    assert np.unique(model_pos(keys, columns, 6), return_counts=True)[1].min() >= 2     # every position is shared
    check_against_model(keys, any_counts(rng, 600), columns, 31, 6)
    # 5 000 keys at k = 5: only 1 024 exist, so keys repeat; records of one key carry one count (a function of the
    # key), which makes the expected bytes a function of the input
    keys = rng.integers(0, 1024, 5000, dtype=np.uint64)
    counts = ((keys * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    got = check_against_model(keys, counts, kmlib.jf_matrix(5, 8, seed=2), 5, 8)
    assert got.shape == (5000, 6)


@pytest.mark.gpu
def test_gpu_many_buckets_and_any_arrival_order():
    rng = np.random.default_rng(4)
    n = 1 << 20
    keys = distinct_keys(rng, n, 21)
    counts = any_counts(rng, n)
    assert (counts >= 65535).sum() > n // 2
    columns = kmlib.jf_matrix(21, 21, seed=5)
    first = check_against_model(keys, counts, columns, 21, 21)
    stats = kmlib.jf_sort_stats()
    assert stats["buckets"] > 1 and stats["oversized"] == 0 and 0 < stats["largest"] <= 2048
    for _ in range(2):
        perm = rng.permutation(n)
        again = kmlib.jf_sort_records(columns, 21, 21, keys[perm], counts[perm])
        assert np.array_equal(again, first)


@pytest.mark.gpu
def test_gpu_oversized_buckets_are_exact():
    rng = np.random.default_rng(6)
    keys = distinct_keys(rng, 20_000, 31)
    counts = any_counts(rng, keys.size)
    columns = kmlib.jf_matrix(31, 32, seed=9) & np.uint64(0xF)         # only the low 4 rows are non-zero
    assert columns.any()
    check_against_model(keys, counts, columns, 31, 32)
    stats = kmlib.jf_sort_stats()
    assert stats["oversized"] >= 1 and stats["largest"] == 20_000 and stats["buckets"] > 1
    # the all-zero matrix: every position is 0, the order is the keys' own
    keys, counts = keys[:9000], counts[:9000]
    got = check_against_model(keys, counts, np.zeros(62, np.uint64), 31, 32)
    assert kmlib.jf_sort_stats()["oversized"] >= 1
    order = np.argsort(keys)
    assert np.array_equal(got, record_bytes(np.sort(keys), counts[order], 31))


@pytest.mark.gpu
def test_gpu_edges():
    rng = np.random.default_rng(7)
    columns = kmlib.jf_matrix(31, 32, seed=1)
    for n in (0, 1, 2):
        keys = distinct_keys(rng, 8, 31)[:n]
        got = check_against_model(keys, any_counts(rng, 8)[:n], columns, 31, 32)
        assert got.shape == (n, 12)
    # k = 32, not canonical, with the all-T key: 64 columns, 8 key bytes
    keys = np.unique(np.concatenate([rng.integers(0, 1 << 63, 3000, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                                     np.array([0xFFFFFFFFFFFFFFFF, 0], np.uint64)]))
    keys = rng.permutation(keys)
    assert int(keys.max()) == 0xFFFFFFFFFFFFFFFF
    for r in (64, 40):
        got = check_against_model(keys, any_counts(rng, keys.size), kmlib.jf_matrix(32, r, seed=r), 32, r)
        assert got.shape[1] == 12
    # k = 29: 58 bits are 8 key bytes; k = 13: 26 bits are 4
    for k, rec in ((29, 12), (13, 8)):
        keys = distinct_keys(rng, 3000, k)
        got = check_against_model(keys, any_counts(rng, keys.size), kmlib.jf_matrix(k, 20, seed=k), k, 20)
        assert got.shape == (3000, rec)


# ------------------------------------------------------------------ GPU: the counter's own writer
def make_reads(seed, n_reads):
    """Reads of 30-150 nt from both strands of the nine catalog sequences, 1 % substitutions, 0.5 % N, mixed case
    (as tests/test_count.py makes them)."""
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


def counted_model(reads, k, lower):
    """(keys sorted, counts) of the canonical k-mers that occur at least `lower` times in `reads`, from the
    definition: every window of k bases, either case; any other byte breaks a window, and so does a read's end."""
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


def jellyfish_lookup(keys, counts, pos, key, p):
    """Jellyfish's query of a binary/sorted file, restated: an interpolated binary search by (pos, key)."""
    lo, hi = 0, len(keys)
    while lo < hi:
        plo, phi = int(pos[lo]), int(pos[hi - 1])
        if p < plo or p > phi:
            return None
        mid = (lo + hi) // 2 if phi == plo else lo + (p - plo) * (hi - 1 - lo) // (phi - plo)
        at = (int(pos[mid]), int(keys[mid]))
        if at == (p, key):
            return int(counts[mid])
        if at < (p, key):
            lo = mid + 1
        else:
            hi = mid
    return None


@pytest.mark.gpu
def test_gpu_counter_writes_the_file_natively(tmp_path, monkeypatch):
    monkeypatch.setenv("KM_COUNT_STAGE_BYTES", "4096")          # the file leaves the device in many pieces
    c = kmlib.Counter(k=31, canonical=True)
    reads = make_reads(61, 2000)
    c.add_bases(b"\n".join(reads))
    with pytest.raises(kmlib.KmError) as e:
        c.write_jf(str(tmp_path / "early.jf"))
    assert e.value.code == 7
    mem = c.finish(2)
    keys, counts = c.records()
    # the records are the ones the reads hold (the catalog is about 1.4 kb, so its k-mers and the repeated
    # errors come to some 2 000), and at 12 bytes each they fill more than four staging buffers of 4 096 bytes
    want_keys, want_counts = counted_model(reads, 31, 2)
    order = np.argsort(keys)
    assert np.array_equal(keys[order], want_keys) and np.array_equal(counts[order], want_counts)
    assert keys.size * 12 > 4 * 4096
    with pytest.raises(kmlib.KmError) as e:                     # a path that cannot be created: KM_E_IO
        c.write_jf(str(tmp_path / "no_such_dir" / "x.jf"))
    assert e.value.code == 1 and not (tmp_path / "no_such_dir").exists()
    native, host = str(tmp_path / "native.jf"), str(tmp_path / "host.jf")
    c.write_jf(native, cmdline=["km_amd", "count", "x"], seed=5)
    c.close()
    kc.write_jellyfish(host, keys, counts, 31, True, cmdline=["km_amd", "count", "x"], seed=5)
    raw = open(native, "rb").read()
    assert raw == open(host, "rb").read()
    hdr, off = jr.parse_header(raw)
    r = max(4, int(2 * keys.size - 1).bit_length())             # size: the power of two >= max(16, 2n)
    assert set(hdr) == HEADER_KEYS and hdr["size"] == 1 << r and hdr["matrix1"]["r"] == r
    assert hdr["matrix1"]["columns"] == [int(x) for x in kmlib.jf_matrix(31, r, seed=5)]
    columns = np.array(hdr["matrix1"]["columns"], np.uint64)
    want, want_pos = model(keys, counts, columns, 31, r)
    assert raw[off:] == want.tobytes()
    # every reader of the project loads it
    rng = np.random.default_rng(62)
    absent = jr.canonical_np(rng.integers(0, 1 << 62, 1000, dtype=np.uint64), 31)
    absent = absent[~np.isin(absent, keys)]
    probe = np.concatenate([keys, absent])
    answer = mem.query(probe)
    assert np.array_equal(answer[:keys.size], counts) and not answer[keys.size:].any()
    opened = kmlib.Database.open(native)
    opened.upload(0)
    loaded = kmlib.Database.load(native)
    assert np.array_equal(opened.query(probe), answer) and np.array_equal(loaded.query(probe), answer)
    for db in (mem, opened, loaded):
        db.close()
    # and so would Jellyfish: its lookup finds every key and misses the absent ones
    rec = jr.read_jf(native)
    pos = model_pos(rec["keys"], columns, r)
    assert np.array_equal(pos, want_pos)
    count_of = dict(zip(keys.tolist(), counts.tolist()))
    for key, p in zip(rec["keys"].tolist(), pos.tolist()):
        assert jellyfish_lookup(rec["keys"], rec["counts"], pos, key, p) == count_of[key]
    for key, p in zip(absent.tolist(), model_pos(absent, columns, r).tolist()):
        assert jellyfish_lookup(rec["keys"], rec["counts"], pos, key, p) is None
    assert absent.size >= 990


@pytest.mark.gpu
def test_gpu_cli_jellyfish_order(tmp_path):
    rng = np.random.default_rng(63)
    reads = make_reads(64, 2000)
    qual = np.frombuffer(b"ACGT@>+", np.uint8)
    text = b"".join(b"@r%d\n" % i + r + b"\n+\n" + qual[rng.integers(0, 7, len(r))].tobytes() + b"\n"
                    for i, r in enumerate(reads))
    for d in ("one", "two", "plain"):
        (tmp_path / d).mkdir()
        (tmp_path / d / "reads.fq").write_bytes(text)
    env = dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system")

    def km(cwd, *args):
        res = subprocess.run([sys.executable, "-m", "km_amd"] + list(args), cwd=tmp_path / cwd, capture_output=True,
                             text=True, timeout=300, env=env)
        assert res.returncode == 0, res.stderr
        return res.stdout

    base = ["count", "-m", "31", "-C", "-L", "2"]
    km("one", *base, "--jellyfish-order", "-o", "a.jf", "reads.fq")
    km("two", *base, "--jellyfish-order", "-o", "a.jf", "reads.fq")
    km("plain", *base, "-o", "a.jf", "reads.fq")
    raw = (tmp_path / "one" / "a.jf").read_bytes()
    assert raw == (tmp_path / "two" / "a.jf").read_bytes()
    hdr, off = jr.parse_header(raw)
    assert set(hdr) == HEADER_KEYS
    assert hdr["cmdline"] == ["km_amd", "count", "-m", "31", "-C", "-L", "2", "-s", "0", "--jellyfish-order", "-o",
                              "a.jf", "reads.fq"]
    rec = jr.read_jf(str(tmp_path / "one" / "a.jf"))
    want, _ = model(rec["keys"], rec["counts"], np.array(hdr["matrix1"]["columns"], np.uint64), 31,
                    hdr["matrix1"]["r"])
    assert raw[off:] == want.tobytes() and hdr["size"] == 1 << hdr["matrix1"]["r"] >= 2 * rec["keys"].size
    # without the flag: the bytes write_records gives for the same records
    again = str(tmp_path / "again.jf")
    kc.write_records(again, rec["keys"], rec["counts"], 31, True,
                     cmdline=["km_amd", "count", "-m", "31", "-C", "-L", "2", "-s", "0", "-o", "a.jf", "reads.fq"])
    plain = (tmp_path / "plain" / "a.jf").read_bytes()
    assert plain == open(again, "rb").read() and plain != raw
    rows = [[ln for ln in km(d, "find_mutation", FLT3, "a.jf").splitlines() if not ln.startswith("#")]
            for d in ("one", "plain")]
    assert rows[0] == rows[1] and len(rows[0]) >= 2 and rows[0][0].startswith("Database\t")
