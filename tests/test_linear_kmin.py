"""`km linear_kmin` (km/tools/linear_kmin.py): the km_linear_kmin export, its binding and the CLI subcommand.

The answers are pinned three ways: tests/golden/linear_kmin.json (the unmodified reference on real files,
tests/golden/make_golden_kmin.py), an independent model written from the reference's definition (below: the
smallest unique k by binary search over k-mer sets, then the reference's forward / backward neighbour counts),
and, on the GPU, the kernel's own R against the model's.  The model never uses the closed form the library
relies on."""
import contextlib
import io
import json
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

from km_amd import cli
from km_amd import lib as kmlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "linear_kmin.json")))["cases"]


# ------------------------------------------------------------------ the model
def _exact_ids(s, k):
    """The k-mers of s as the reference slices them (any k, negative included)."""
    return [s[i:i + k] for i in range(len(s) - k + 1)]


class _Hashed:
    """k-mer identities of a long target as 64-bit polynomial hashes (one prefix sum, wrapping arithmetic)."""
    B = np.uint64(0x9E3779B97F4A7C15)

    def __init__(self, s):
        c = np.frombuffer(s.encode("ascii"), np.uint8).astype(np.uint64) + np.uint64(1)
        binv = np.uint64(pow(int(self.B), -1, 1 << 64))
        with np.errstate(over="ignore"):
            self.bpow = np.concatenate([[np.uint64(1)], np.cumprod(np.full(len(s), self.B, np.uint64))])
            ipow = np.concatenate([[np.uint64(1)], np.cumprod(np.full(len(s), binv, np.uint64))])
            self.q = np.concatenate([[np.uint64(0)], np.cumsum(c * ipow[:-1])])

    def ids(self, k, first, count):
        i = np.arange(first, first + count)
        with np.errstate(over="ignore"):
            return (self.q[i + k] - self.q[i]) * self.bpow[i]


def _unique(s, k, h):
    n = len(s)
    if h is None or k <= 0:
        m = _exact_ids(s, k)
        return len(set(m)) == len(m)
    return np.unique(h.ids(k, 0, n - k + 1)).size == n - k + 1


def _linear(s, k, h):
    """The reference's neighbour counts (linear_kmin.py:21-43) with dicts of (k-1)-mer prefixes / suffixes."""
    if h is None or k <= 0:
        mers = _exact_ids(s, k)
        pre, suf = [m[:-1] for m in mers], [m[1:] for m in mers]
        npre, nsuf = {}, {}
        for p, q in zip(pre, suf):
            npre[p] = npre.get(p, 0) + 1
            nsuf[q] = nsuf.get(q, 0) + 1
        for p, q in zip(pre, suf):
            self_loop = p == q
            if npre.get(q, 0) - self_loop > 1 or nsuf.get(p, 0) - self_loop > 1:
                return False
        return True
    m = len(s) - k + 1
    pre, suf = h.ids(k - 1, 0, m), h.ids(k - 1, 1, m)
    up, cp = np.unique(pre, return_counts=True)
    us, cs = np.unique(suf, return_counts=True)

    def count(keys, vals, cnt):
        j = np.minimum(np.searchsorted(keys, vals), keys.size - 1)
        return np.where(keys[j] == vals, cnt[j], 0)

    self_loop = (pre == suf).astype(np.int64)
    return bool(((count(up, suf, cp) - self_loop <= 1) & (count(us, pre, cs) - self_loop <= 1)).all())


def model(s, start):
    """(k, R): what km/tools/linear_kmin.py prints for s and start, and the longest repeated substring."""
    n = len(s)
    h = _Hashed(s) if n > 3000 else None
    lo, hi = 1, max(n, 1)              # smallest unique k >= 1 (k = n leaves one k-mer)
    while lo < hi:
        mid = (lo + hi) // 2
        if _unique(s, mid, h):
            hi = mid
        else:
            lo = mid + 1
    R = lo - 1 if n else 0
    if start - 1 >= n:
        return start - 1, R
    for k in range(start, 1):          # k <= 0: sliced as the reference slices
        if _unique(s, k, None) and _linear(s, k, None):
            return k, R
    for k in range(max(start, lo), n + 1):
        if _linear(s, k, h):
            return k, R
    return n, R


# ------------------------------------------------------------------ golden cases through the CLI
def _write_files(case, where):
    if case["files"] is None:
        return [os.path.join(HERE, p) for p in case["paths"]]
    for name, text in case["files"].items():
        with open(os.path.join(where, name), "w") as fh:
            fh.write(text)
    return [os.path.join(where, p) for p in case["paths"]]


def _run_cli(argv, out):
    """cli.main with stdout captured; (stdout, exception or None)."""
    err = None
    with contextlib.redirect_stdout(out):
        try:
            cli.main(argv)
        except (Exception, SystemExit) as e:   # noqa: BLE001
            err = e
    return out.getvalue(), err


def _argv(case, paths):
    return ["linear_kmin"] + ([] if case["start"] is None else ["-s", str(case["start"])]) + paths


def _check_case(case, tmp_path):
    d = tmp_path / ("c%d" % id(case))
    d.mkdir()
    out, err = _run_cli(_argv(case, _write_files(case, str(d))), io.StringIO())
    assert out == case["stdout"], case["paths"]
    if case["error"] is None:
        assert err is None, err
    else:
        assert type(err).__name__ == case["error"]["type"] and str(err) == case["error"]["message"]


@pytest.fixture
def model_gpu(monkeypatch):
    """km_amd.lib.linear_kmin replaced by the model: the CLI runs with no GPU."""
    calls = []

    def stub(seqs, start=10, device=0, stream=None, detail=False):
        calls.append(len(seqs))
        assert all(isinstance(s, str) and s == s.upper() for s in seqs)
        return np.array([model(s, start)[0] for s in seqs], np.int32)

    monkeypatch.setattr(kmlib, "linear_kmin", stub)
    return calls


def test_model_equals_every_golden(model_gpu, tmp_path):
    """The model + the CLI's file reading reproduce every reference run (stdout, and the exception where
    it raised) — 99 fixture x start cases, 200 synthetic targets, the two fixture lists, the header errors."""
    kinds = set()
    for case in GOLD:
        _check_case(case, tmp_path)
        kinds.add(case["kind"])
    assert len(GOLD) >= 300 and {"fixture", "fixture_list", "error", "prefix_suffix", "tandem"} <= kinds
    assert max(model_gpu) == 9          # a file list is one call


def test_flt3_fixture_is_ten_from_five():
    """km/tests/test_main.py:563-579: FLT3-ITD from -s 5 gives 10 (R = 8)."""
    seq = cli.read_target_records(os.path.join(HERE, "data", "catalog", "GRCh38", "FLT3-ITD_exons_13-15.fa"))
    assert model(seq, 5) == (10, 8)


def test_cli_flags_and_rows(model_gpu, tmp_path):
    """-s / --start (nargs='?', default 10), file order kept, the name column is splitext(basename)."""
    files = []
    for name, seq in (("z.b.fa", "ACGTACGTTTGA" * 3), ("a.fasta", "AC" * 30), ("m", "acgtnnnnACGT")):
        p = tmp_path / name
        p.write_text(">x\n%s\n" % seq)
        files.append(str(p))
    want = [model(s, st)[0] for st in (10, 3) for s in ("ACGTACGTTTGA" * 3, "AC" * 30, "ACGTNNNNACGT")]
    for argv, ks in ((files, want[:3]), (["-s", "3"] + files, want[3:]), (["--start", "3"] + files, want[3:])):
        out, err = _run_cli(["linear_kmin"] + argv, io.StringIO())
        assert err is None
        assert out == "target_name\tlinear_kmin\n" + "".join(
            "%s\t%d\n" % (n, k) for n, k in zip(("z.b", "a", "m"), ks))
    assert model_gpu == [3, 3, 3]
    # a directory argument lists the directory
    out, err = _run_cli(["linear_kmin", str(tmp_path)], io.StringIO())
    by_file = dict(zip(("z.b.fa", "a.fasta", "m"), want[:3]))
    assert err is None and out.split("\n")[1:-1] == [
        "%s\t%d" % (os.path.splitext(f)[0], by_file[f]) for f in os.listdir(tmp_path)]
    # `-s` with no value: the reference's `start - 1` on None, after the header
    out, err = _run_cli(["linear_kmin"] + files + ["-s"], io.StringIO())
    assert isinstance(err, TypeError) and out == "target_name\tlinear_kmin\n"
    assert str(err) == "unsupported operand type(s) for -: 'NoneType' and 'int'"
    # no target at all: the reference indexes an empty list
    out, err = _run_cli(["linear_kmin"], io.StringIO())
    assert isinstance(err, IndexError) and out == "target_name\tlinear_kmin\n"


def test_cli_header_errors_after_earlier_rows(model_gpu, tmp_path):
    """A file that fails to read: the rows of the files before it, then the reference's exception."""
    good = tmp_path / "good.fa"
    good.write_text("text before the header\n>g|a=b\n>merged\nacgtacgtac\n\nTTGCA\n")
    assert cli.read_target_records(str(good)) == "ACGTACGTACTTGCA"
    for text, etype, msg in ((">h|nofield\nACGT\n", ValueError, "not enough values to unpack (expected 2, got 1)"),
                             (">h=1\nACGT\n", ValueError, "too many values to unpack (expected 2)"),
                             (">h\nACGT\n>h2\n", RuntimeError, "generator raised StopIteration")):
        bad = tmp_path / "bad.fa"
        bad.write_text(text)
        out, err = _run_cli(["linear_kmin", str(good), str(bad), str(good)], io.StringIO())
        assert type(err) is etype and str(err) == msg
        assert out == "target_name\tlinear_kmin\ngood\t%d\n" % model("ACGTACGTACTTGCA", 10)[0]


def test_cli_refuses_non_ascii_targets(model_gpu, tmp_path):
    """Bytes are compared, so a target with a non-ASCII letter exits with a message."""
    good = tmp_path / "good.fa"
    good.write_text(">g\nACGTTGCA\n")
    bad = tmp_path / "bad.fa"
    bad.write_text(">b\nACGÉT\n", encoding="utf-8")
    out, err = _run_cli(["linear_kmin", str(good), str(bad)], io.StringIO())
    assert isinstance(err, SystemExit) and "ASCII" in str(err.code) and "bad.fa" in str(err.code)
    assert out == "target_name\tlinear_kmin\ngood\t%d\n" % model("ACGTTGCA", 10)[0]


def test_km_linear_kmin_refuses_bad_arguments_without_touching_a_gpu():
    """KM_E_ARG before any HIP call: NULL pointers, decreasing offsets, a target longer than 2^31 - 1;
    no target at all is KM_OK without a launch."""
    lib = kmlib.load()
    bases = np.frombuffer(b"ACGTACGT", np.uint8)
    k = np.zeros(2, np.int32)
    ok = np.array([0, 4, 8], np.uint64)
    P = kmlib.ptr
    assert lib.km_linear_kmin(0, P(bases), None, 2, 10, P(k), None, None, None) == 4
    assert lib.km_linear_kmin(0, P(bases), P(ok), 2, 10, None, None, None, None) == 4
    assert lib.km_linear_kmin(0, None, P(ok), 2, 10, P(k), None, None, None) == 4
    assert lib.km_linear_kmin(0, P(bases), P(np.array([0, 5, 4], np.uint64)), 2, 10, P(k), None, None, None) == 4
    assert lib.km_linear_kmin(0, P(bases), P(np.array([0, 4, 4 + (1 << 31)], np.uint64)), 2, 10, P(k), None, None,
                              None) == 4
    assert b"2^31" in lib.km_last_error()
    assert lib.km_linear_kmin(0, None, P(np.zeros(1, np.uint64)), 0, 10, P(k), None, None, None) == 0
    assert kmlib.linear_kmin([], 10).shape == (0,)


# ------------------------------------------------------------------ GPU
def _golden_targets(tmp_path):
    """(sequence, start, k) of every golden row that has one, through the CLI's reader."""
    out = []
    for i, case in enumerate(GOLD):
        d = tmp_path / ("g%d" % i)
        d.mkdir()
        paths = _write_files(case, str(d))
        rows = case["stdout"].split("\n")[1:-1]
        start = 10 if case["start"] is None else case["start"]
        for p, row in zip(paths, rows):
            out.append((cli.read_target_records(p), start, int(row.split("\t")[1])))
    return out


@pytest.mark.gpu
def test_gpu_equals_every_golden(tmp_path):
    rows = _golden_targets(tmp_path)
    for start in sorted({st for _, st, _ in rows}):
        part = [(s, k) for s, st, k in rows if st == start]
        kmin, rep, _flag = kmlib.linear_kmin([s for s, _ in part], start, detail=True)
        assert kmin.tolist() == [k for _, k in part], start
        assert rep.tolist() == [model(s, start)[1] for s, _ in part]
    assert len(rows) > 300


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _check_against_model(seqs, start):
    kmin, rep, _flag = kmlib.linear_kmin(seqs, start, detail=True)
    for i, s in enumerate(seqs):
        assert (int(kmin[i]), int(rep[i])) == model(s, start), (i, len(s))
    return kmin, rep


@pytest.mark.gpu
def test_gpu_catalog_of_short_targets_with_planted_repeats():
    """10 000 x 500 nt, each with a 20-60 nt stretch copied to a second place."""
    rng = random.Random(11)
    seqs = []
    for _ in range(10_000):
        s = list(_rand(rng, 500))
        r = rng.randint(20, 60)
        a = rng.randint(0, 500 - 2 * r)
        b = rng.randint(a + r, 500 - r)             # copy and source do not overlap
        s[b:b + r] = s[a:a + r]
        seqs.append("".join(s))
    _kmin, rep = _check_against_model(seqs, 10)
    assert int(rep.min()) >= 20 and int(rep.max()) >= 59


@pytest.mark.gpu
def test_gpu_one_call_mixes_every_size():
    """Lengths 0, 1, 2, 3, 64, 65 and 500 nt .. 50 kb in ONE call: short and long work units share a launch."""
    rng = random.Random(12)
    lens = [0, 1, 2, 3, 64, 65, 66, 127, 128, 129] + [rng.choice([500, 1000, 5000, 20_000, 50_000]) for _ in range(40)]
    rng.shuffle(lens)
    seqs = [_rand(rng, n, rng.choice(["ACGT", "ACGTN", "AC", "A"])) if n < 100 else _rand(rng, n) for n in lens]
    for start in (10, 1, 0):
        _check_against_model(seqs, start)


@pytest.mark.gpu
def test_gpu_adversarial_targets():
    rng = random.Random(13)
    letters = "ACDEFGHIKLMNPQRSTVWY"
    # order-2 de Bruijn sequence over 20 letters (every 2-mer once): R = 1 with ~400 tied runs
    db = []
    a = [0] * 40

    def gen(t, p):
        if t > 2:
            if 2 % p == 0:
                db.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            gen(t + 1, p)
            for j in range(a[t - p] + 1, 20):
                a[t] = j
                gen(t + 1, t)
    gen(1, 1)
    debruijn = "".join(letters[i] for i in db) + letters[db[0]]
    assert len(debruijn) == 401
    random300 = _rand(rng, 300_000)
    seqs = {
        "debruijn": debruijn,
        "homopolymer": "A" * 100_000,
        "period2": "AC" * 50_000,
        "period3": "ACG" * 33_334,
        "planted_end": random300[:-5000] + random300[100_000:105_000],
        "prefix_is_suffix": "ACGTTGCATTAGGC" + _rand(rng, 2000, "ACGT") + "ACGTTGCATTAGGC",
    }
    names = list(seqs)
    kmin, rep, flag = kmlib.linear_kmin([seqs[n] for n in names], 10, detail=True)
    got = {n: (int(k), int(r), int(f)) for n, k, r, f in zip(names, kmin, rep, flag)}
    for n in names:
        assert got[n][:2] == model(seqs[n], 10), n
    assert got["debruijn"][1] == 1 and got["homopolymer"][1] == 99_999
    assert got["period2"][1] == 99_998 and got["period3"][1] == len(seqs["period3"]) - 3
    assert got["planted_end"][1] >= 5000
    # the longest repeat is only the target's first bases = its last: exempt, so k = R + 1
    assert got["prefix_is_suffix"] == (15, 14, 0)


@pytest.mark.gpu
def test_gpu_results_are_deterministic_across_calls_and_streams():
    rng = random.Random(14)
    seqs = [_rand(rng, rng.randint(0, 3000)) for _ in range(300)]
    a = kmlib.linear_kmin(seqs, 10, detail=True)
    b = kmlib.linear_kmin(seqs, 10, detail=True)
    st = kmlib.stream_create(0)
    try:
        c = kmlib.linear_kmin(seqs, 10, stream=st, detail=True)
    finally:
        kmlib.stream_destroy(st)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)


@pytest.mark.gpu
def test_gpu_staging_in_chunks_gives_the_same_results(monkeypatch):
    """A call whose text exceeds the staging size is staged and launched chunk by chunk (KM_KMIN_STAGE_BYTES
    lowers the 256 MB default): same k, R and flag as one launch, a target longer than a chunk alone in its own."""
    rng = random.Random(15)
    seqs = [_rand(rng, rng.choice([0, 1, 2, 70, 500, 3000])) for _ in range(400)]
    seqs[123] = _rand(rng, 40_000)
    one = kmlib.linear_kmin(seqs, 10, detail=True)
    monkeypatch.setenv("KM_KMIN_STAGE_BYTES", "20000")
    chunked = kmlib.linear_kmin(seqs, 10, detail=True)
    for x, y in zip(one, chunked):
        assert np.array_equal(x, y)
    assert (int(one[0][123]), int(one[1][123])) == model(seqs[123], 10)


@pytest.mark.gpu
def test_gpu_cli_end_to_end_matches_reference_stdout():
    """`python -m km_amd linear_kmin` on the fixture file lists: byte-identical to the reference's stdout."""
    n = 0
    for case in GOLD:
        if case["kind"] != "fixture_list":
            continue
        res = subprocess.run([sys.executable, "-m", "km_amd"] + _argv(case, case["paths"]), cwd=HERE,
                             capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, PYTHONPATH=ROOT, KM_HIP_RUNTIME="system"))
        assert res.returncode == 0, res.stderr
        assert res.stdout == case["stdout"]
        n += 1
    assert n == 2


@pytest.mark.gpu
def test_gpu_plain_c_consumer(tmp_path):
    """tests/c_abi/linear_kmin.c: gcc-built, no Python in the process, same rows as the reference."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "linear_kmin_c")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "c_abi", "linear_kmin.c"), "-L", os.path.join(ROOT, "km_amd"),
                           "-lkmgpu", "-Wl,-rpath," + os.path.join(ROOT, "km_amd"), "-o", exe])
    for case in GOLD:
        if case["kind"] != "fixture_list":
            continue
        start = "10" if case["start"] is None else str(case["start"])
        res = subprocess.run([exe, start] + case["paths"], capture_output=True, text=True, cwd=HERE, timeout=120)
        assert res.returncode == 0, res.stderr
        assert res.stdout == case["stdout"]
