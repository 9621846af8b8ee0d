"""The scan on the GPU: Database.cov_seqs / scan_text (kmjf_cov_seqs, kmjf_scan_text), common.get_cov / get_cov_many /
cov_many over them, `python -m km_amd cov` and `query -s`.

Every comparison is exact, integers equal and text byte-identical, against model_cov / model_text of
tests/test_scan_cpu.py, which are written from the rule of include/kmgpu.h and pinned there to the reference's answers.
The sizes are the ends of what a lane (32 window starts), a wave (2 048) and a block (8 192) own, with and without the
k - 1 bytes a lane reads from its neighbour."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from km_amd import cli
from km_amd import common
from km_amd import count as kc
from km_amd import lib as kmlib
import test_dump as tdump
import test_scan_cpu as sc

HERE = os.path.dirname(os.path.abspath(__file__))
JF_DIR = os.path.join(HERE, "data", "jf")
CATALOG = os.path.join(HERE, "data", "catalog", "GRCh38")
NPM1 = os.path.join(JF_DIR, "02H025_NPM1.jf")
IANDI = os.path.join(JF_DIR, "03H112_IandI.jf")
NONE = 0xFFFFFFFF
KM_E_IO, KM_E_ARG, KM_E_STATE = 1, 4, 7
EDGES = (31, 32, 33, 2047, 2048, 2049, 8191, 8192, 8193)
COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")

pytestmark = pytest.mark.gpu

model_cov, model_text, random_bases = sc.model_cov, sc.model_text, sc.random_bases


# ------------------------------------------------------------------ helpers
def make_db(table, k, canonical):
    keys = np.fromiter(table.keys(), np.uint64, len(table))
    counts = np.fromiter(table.values(), np.uint32, len(table))
    return kmlib.Database.from_records(keys, counts, k, canonical).upload(0)


def cells(cov):
    return [tuple(int(c[f]) for f in ("total", "n_kmers", "n_zero", "n_skipped", "n_nonbase", "min", "max")) for c in cov]


def scan_text(db, seqs):
    return tdump.through_pipe(lambda fh: db.scan_text(seqs, fh))


def check(db, seqs, table, k, canonical, ctx=None, model=None):
    """cov_seqs and scan_text of the batch against the model (computed here, or as given: (cells, text)) -> (cells,
    text, stats of scan_text)."""
    want, want_text = model or (model_cov(seqs, table, k, canonical), model_text(seqs, table, k, canonical))
    got = cells(db.cov_seqs(seqs))
    assert got == want, (ctx, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5])
    st, text = scan_text(db, seqs)
    assert text == want_text, ctx
    assert st["records_in"] == sc.n_windows(seqs, k) and st["records_out"] == text.count(b"\n") == sum(c[1] for c in want), ctx
    assert st["bytes_out"] == len(text), ctx
    return got, text, st


def table_of(seqs, k, canonical, seed):
    return sc.a_tenth_of_the_kmers(seqs, k, canonical, np.random.default_rng(seed))


def tiny_batch(k, seed=21, long_ones=(10000, 10000, 10000)):
    """5 000 sequences of 0 .. k + 2 bases, a few long ones mixed in: several sequences, empty ones among them, end
    inside one lane's 32 starts."""
    rng = np.random.default_rng(seed + k)
    seqs = [random_bases(rng, int(n)) for n in rng.integers(0, k + 3, 5000)]
    for i, n in enumerate(long_ones):
        seqs[700 + 1300 * i] = random_bases(rng, n)
    return seqs


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("k", [31, 5])
def test_lengths_of_one_sequence(k):
    rng = np.random.default_rng(k)
    lengths = [0, 1, k - 1, k, k + 1, 32, 33, 32 + k - 1, 2047, 2048, 2049, 2048 + k - 1, 8191, 8192, 8193, 3 * 8192 + 5]
    seqs = [random_bases(rng, n) for n in lengths]
    table = table_of(seqs, k, True, k)
    db = make_db(table, k, True)
    try:
        alone = []
        for n, seq in zip(lengths, seqs):
            alone.append(check(db, [seq], table, k, True, n))
            assert alone[-1][0][0][1] == max(0, n - k + 1)
        # all in one batch: the cells and the lines of the sixteen, one after the other
        check(db, seqs, table, k, True, "all in one batch", ([a[0][0] for a in alone], b"".join(a[1] for a in alone)))
        assert kmlib.scan_kernel_ms() > 0
    finally:
        db.close()


@pytest.mark.parametrize("k", [31, 5])
def test_boundaries_at_every_edge(k):
    """A sequence that starts, and one that ends, at each end of a lane's, a wave's and a block's range."""
    rng = np.random.default_rng(100 + k)
    batches = []
    for at in EDGES:
        batches.append(("starts at", at, [random_bases(rng, at), random_bases(rng, k + 3), random_bases(rng, 70)]))
        batches.append(("ends at", at, [random_bases(rng, 7), random_bases(rng, at - 7), random_bases(rng, 2 * k)]))
        batches.append(("empty ones at", at, [random_bases(rng, at), b"", b"", random_bases(rng, k), b""]))
    table = table_of([s for _, _, b in batches for s in b], k, False, k)
    db = make_db(table, k, False)
    try:
        for name, at, seqs in batches:
            assert name == "ends at" or len(seqs[0]) == at
            assert name != "ends at" or len(seqs[0]) + len(seqs[1]) == at
            check(db, seqs, table, k, False, (name, at))
    finally:
        db.close()


@pytest.mark.parametrize("k", [31, 5])
def test_many_tiny_sequences(k):
    seqs = tiny_batch(k)
    table = table_of(seqs, k, True, k)
    db = make_db(table, k, True)
    try:
        got, _, _ = check(db, seqs, table, k, True)
        short = [c for s, c in zip(seqs, got) if len(s) < k]
        assert len(short) > 1000 and all(c == (0, 0, 0, 0, 0, NONE, 0) for c in short)
        assert sum(1 for s in seqs if not s) > 50 and sum(1 for c in got if c[1] > 9000) == 3
    finally:
        db.close()


@pytest.mark.parametrize("k", [31, 5])
def test_non_bases(k):
    rng = np.random.default_rng(200 + k)
    every_kth = bytearray(random_bases(rng, 40 * k))
    every_kth[::k] = b"N" * len(every_kth[::k])
    body = random_bases(rng, 100)
    cases = {
        "N first and last": [b"N" + body + b"N"],
        "N at every k-th byte": [bytes(every_kth)],
        "N in a sequence shorter than k": [b"ACNG"[: k - 1], body],
        "lower case": [body.lower(), body[:50] + body[50:].lower()],
        "N on both sides of a boundary": [body + b"N", b"N" + body[::-1], body],
        "other bytes": [body[:40] + b"-" + body[40:60] + b"\x00\xff" + body[60:], b"NNNN", b"*"],
    }
    table = table_of([s.upper() for b in cases.values() for s in b], k, True, k)
    db = make_db(table, k, True)
    try:
        for name, seqs in cases.items():
            got, text, st = check(db, seqs, table, k, True, name)
            if name == "N first and last":
                assert got[0][3:5] == (2, 2) and got[0][1] == 102 - k + 1 - 2
            if name == "N at every k-th byte":
                assert got[0][1] == 0 and got[0][3] == 40 * k - k + 1 and got[0][4] == 40 and text == b""
            if name == "N in a sequence shorter than k":
                assert got[0] == (0, 0, 0, 0, 1, NONE, 0)
            if name == "lower case":
                assert got[0] == cells(db.cov_seqs([body]))[0] and got[0][3:5] == (0, 0)
                assert text[: len(text) // 2] == text[len(text) // 2:] and text == text.upper()
            if name == "N on both sides of a boundary":
                assert [c[3:5] for c in got] == [(1, 1), (1, 1), (0, 0)] and got[0][1] == got[1][1] == got[2][1]
    finally:
        db.close()


def test_counts_around_the_escape_and_beyond_32_bits():
    k = 31
    rng = np.random.default_rng(300)
    unit = random_bases(rng, 60)
    seqs = [unit + unit + unit + unit, random_bases(rng, 500)]
    keys = sorted({w[0] for s in seqs for w in sc.windows(s, k, True)})
    assert len(keys) > 400
    table = {key: c for key, c in zip(keys, [NONE, 65534, 65535, 65536, 1, 65535, NONE - 1] * 100)}
    top = sc.windows(unit, k, True).__next__()[0]
    table[top] = NONE                                     # the first window of the unit: four times in seqs[0]
    db = make_db(table, k, True)
    try:
        got, text, _ = check(db, seqs, table, k, True)
        assert got[0][0] > 4 * NONE > 1 << 32 and got[0][6] == NONE
        for c in (65534, 65535, 65536, NONE):
            assert b" %d\n" % c in text
    finally:
        db.close()


def test_canonical_and_non_canonical_tables():
    k = 31
    rng = np.random.default_rng(400)
    seqs = [random_bases(rng, 300), random_bases(rng, 40), random_bases(rng, 2100)]
    flipped = [s.translate(COMPLEMENT)[::-1] for s in seqs]
    table = table_of(seqs, k, True, 400)                  # canonical keys; the same records in both tables
    for canonical in (True, False):
        db = make_db(table, k, canonical)
        try:
            got, text, _ = check(db, seqs, table, k, canonical, canonical)
            back, _, _ = check(db, flipped, table, k, canonical, canonical)
            if canonical:
                assert back == got and got[0][1] > got[0][2] > 0
            else:
                mers = [ln.split(b" ")[0] for ln in text.splitlines()]
                assert mers == [s[i:i + k] for s in seqs for i in range(len(s) - k + 1)]      # printed as given
                assert back != got
        finally:
            db.close()


# ------------------------------------------------------------------ pieces
@pytest.mark.parametrize("k", [31, 5])
def test_pieces(monkeypatch, k):
    """The same batch at three staging sizes: identical statistics and text.  At 256 the 30 000-base sequence spans
    more than a hundred pieces, and a piece of k = 31 stages more overlap (30 bytes) than it owns starts (5 in text
    mode)."""
    seqs = tiny_batch(k, seed=33)
    seqs.insert(2500, random_bases(np.random.default_rng(34), 30000))
    table = table_of(seqs, k, True, 35)
    total = sum(len(s) for s in seqs)
    db = make_db(table, k, True)
    try:
        seen = {}
        model = (model_cov(seqs, table, k, True), model_text(seqs, table, k, True))
        for stage in (256, 4096, None):
            if stage is None:
                monkeypatch.delenv("KM_COUNT_STAGE_BYTES", raising=False)
            else:
                monkeypatch.setenv("KM_COUNT_STAGE_BYTES", str(stage))
            seen[stage] = check(db, seqs, table, k, True, stage, model)
            if stage is not None:                        # a piece's starts: its bytes less the overlap, and lines that fit
                assert seen[stage][2]["pieces"] == -(-total // min(stage - (k - 1), stage // (k + 13))), stage
        assert seen[256][:2] == seen[4096][:2] == seen[None][:2]
        assert seen[None][2]["pieces"] == 1 and 3 <= seen[4096][2]["pieces"] < seen[256][2]["pieces"]
        assert 30000 // 256 > 100
    finally:
        db.close()


# ------------------------------------------------------------------ the reference's answers through the scan
@functools.lru_cache(maxsize=None)
def golden(name):
    with open(os.path.join(HERE, "golden", name)) as fh:
        return json.load(fh)


def test_get_cov_against_the_golden_tuples(monkeypatch):
    from oracle import km_oracle as ko
    monkeypatch.chdir(HERE)
    try:
        for g in golden("fixtures_children.json")["min_cov"]:
            got = common.get_cov(g["db"], ko.read_fasta_concat(g["target"]))
            assert list(got) == g["cov"] and isinstance(got[4], float) and all(isinstance(x, int) for x in got[:4] + got[5:])
        seq = ko.read_fasta_concat("./data/catalog/GRCh38/FLT3-ITD_exons_13-15.fa")
        r = common.get_cov("./data/jf/03H112_IandI.jf", seq)
        assert r[:4] == (275596, 345, 618, 1368) and "%.2f" % r[4] == "874.91" and r[5:] == (315, 0)
    finally:
        common.close_all()


def test_get_cov_many_against_the_exclusion_column(monkeypatch):
    monkeypatch.chdir(HERE)
    mat = golden("sample_matrix.json")
    try:
        for case in mat["exclu"]:
            stream = [t for t in mat["targets"] if t["target"] == case["target"]][0]["stream"]
            seqs = []
            for line in stream:
                tok = line.split("\t")
                if line.startswith("#") or "vs_ref" not in line or tok[0] == "Database" or len(tok) <= 1:
                    continue
                if int(tok[6]) < 1:                      # find_report's -m 1 filter
                    continue
                seqs.append(tok[8])
            want = [ln.split("\t")[10] for ln in case["find_report"][1:]]
            assert len(seqs) == len(want) and len(seqs) >= 2
            many = common.get_cov_many(case["exclu"], seqs)
            assert [str(r[2]) for r in many] == want
            table, k, canonical = sc.file_table(case["exclu"])
            assert many == [sc.cov_tuple(s, c) for s, c in zip(seqs, model_cov(seqs, table, k, canonical))]
            raw = common.cov_many(case["exclu"], seqs)
            assert cells(raw) == model_cov(seqs, table, k, canonical)
    finally:
        common.close_all()


def test_the_exceptions_stay_the_reference_s():
    good, short = "ACGT" * 20, "ACGT" * 5
    try:
        for call in (lambda: common.get_cov(NPM1, good[:40] + "N" + good[41:]),
                     lambda: common.get_cov(NPM1, "ACGN"),                       # shorter than k: still the letter
                     lambda: common.get_cov_many(NPM1, [short, good, "ACGTN"]),   # ... before the short one in front
                     lambda: common.get_cov_many(NPM1, [good, "AC-T"])):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == "non-ACGT character in sequence"
        for call in (lambda: common.get_cov(NPM1, short), lambda: common.get_cov(NPM1, ""),
                     lambda: common.get_cov_many(NPM1, [good, short, good])):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == "min() arg is an empty sequence"
        assert common.get_cov_many(NPM1, []) == []
        assert common.get_cov(NPM1, good.lower()) == common.get_cov(NPM1, good)
        raw = common.cov_many(NPM1, [short, "ACGTN", good])                      # the raw cells raise nothing
        assert cells(raw)[0] == (0, 0, 0, 0, 0, NONE, 0) and cells(raw)[1] == (0, 0, 0, 0, 1, NONE, 0) and raw["n_kmers"][2] == 50
    finally:
        common.close_all()


# ------------------------------------------------------------------ the commands
def test_cli_cov(tmp_path):
    res = tdump.run_cli(["cov", "-t", CATALOG, NPM1, IANDI])
    assert res.returncode == 0, res.stderr
    files = cli.list_target_files([CATALOG])
    want = sc.cov_rows([NPM1, IANDI], files)
    assert res.stdout.decode() == want
    rows = [ln.split("\t") for ln in want.splitlines()]
    npm1 = [r for r in rows if r[0] == NPM1 and r[1] == "NPM1_4ins_exons_10-11utr"]
    assert [r[2:5] + r[8:] for r in npm1] == [["1", "0", "27", "0", "0", "0"], ["2", npm1[1][3], "53", "23", "0", "0"]]
    assert npm1[0][5:8] == ["NA", "NA", "NA"] and int(npm1[1][3]) > 0
    assert len(rows) == 1 + 2 * sum(len(sc.fasta_records(f)) for f in files)
    out = tmp_path / "cov.tsv"
    res = tdump.run_cli(["cov", "-o", str(out), "-t", os.path.join(CATALOG, "NPM1_4ins_exons_10-11utr.fa"), NPM1])
    assert res.returncode == 0 and res.stdout == b"" and out.read_text() == sc.cov_rows([NPM1], [files[[os.path.basename(f) for f in files].index("NPM1_4ins_exons_10-11utr.fa")]])
    res = tdump.run_cli(["cov", "-t", str(tmp_path / "missing.fa"), "-o", str(tmp_path / "no.tsv"), NPM1])
    assert res.returncode != 0 and res.stdout == b"" and not (tmp_path / "no.tsv").exists()


def test_cli_query_sequence_and_mers(tmp_path):
    table, k, canonical = sc.file_table(NPM1)
    rng = np.random.default_rng(500)
    inside = sc.fasta_records(os.path.join(CATALOG, "NPM1_4ins_exons_10-11utr.fa"))[1]
    records = [inside + random_bases(rng, 40), b"ACGTACGT", inside[:40] + b"NN" + inside[10:] + b"n"]
    fa = tmp_path / "three.fa"
    fa.write_bytes(b"ignored before the first header\n" + b"".join(b">r%d\n%s\n%s\n" % (i, r[:30], r[30:]) for i, r in enumerate(records)))
    mers = [inside[3:3 + k].decode(), "A" * k, inside[5:5 + k].decode().lower()]
    want = model_text(records, table, k, canonical) + model_text([m.encode() for m in mers], table, k, canonical)
    cov = model_cov(records, table, k, canonical)          # the second record has no window, the third skips k + 2
    assert cov[1][1] == 0 and cov[2][3:5] == (k + 2, 3) and want.count(b"\n") == sum(c[1] for c in cov) + 3
    assert b" 0\n" in want and want.count(b" 0\n") < want.count(b"\n") // 2
    res = tdump.run_cli(["query", "-s", str(fa), NPM1] + mers)
    assert res.returncode == 0, res.stderr
    assert res.stdout == want
    # in this process: the same bytes to a file, and the scan kernels really ran
    out = tmp_path / "q.txt"
    st = kc.query_file(NPM1, mers=mers, seq_files=[str(fa), str(fa)], out=str(out))
    assert kmlib.scan_kernel_ms() > 0
    twice = model_text(records + records, table, k, canonical) + model_text([m.encode() for m in mers], table, k, canonical)
    assert out.read_bytes() == twice
    assert st["records_out"] == twice.count(b"\n") and st["records_in"] == 2 * sc.n_windows(records, k) + 3 and st["bytes_out"] == len(twice)


# ------------------------------------------------------------------ refusals
def test_error_paths(tmp_path):
    lib = kmlib.load()
    text = np.frombuffer(b"ACGT" * 20, np.uint8)
    off = np.array([0, 40, 80], np.uint64)
    out = np.zeros(2, kmlib.COV_DTYPE)
    db = kmlib.Database.open(NPM1)
    try:
        with open(os.devnull, "wb") as null:
            with pytest.raises(kmlib.KmError) as e:                          # before the upload
                db.cov_seqs([b"ACGT" * 10])
            assert e.value.code == KM_E_STATE
            with pytest.raises(kmlib.KmError) as e:
                db.scan_text([b"ACGT" * 10], null)
            assert e.value.code == KM_E_STATE
            db.upload(0)
            down = np.array([0, 50, 40], np.uint64)
            assert lib.kmjf_cov_seqs(db._h, kmlib.ptr(text), kmlib.ptr(down), 2, kmlib.ptr(out), None) == KM_E_ARG
            assert "ascend" in lib.km_last_error().decode()
            assert lib.kmjf_scan_text(db._h, kmlib.ptr(text), kmlib.ptr(down), 2, null.fileno(), None, None) == KM_E_ARG
            assert lib.kmjf_cov_seqs(db._h, None, kmlib.ptr(off), 2, kmlib.ptr(out), None) == KM_E_ARG
            assert lib.kmjf_cov_seqs(db._h, kmlib.ptr(text), None, 2, kmlib.ptr(out), None) == KM_E_ARG
            assert lib.kmjf_cov_seqs(db._h, kmlib.ptr(text), kmlib.ptr(off), 2, None, None) == KM_E_ARG
            assert lib.kmjf_cov_seqs(None, kmlib.ptr(text), kmlib.ptr(off), 2, kmlib.ptr(out), None) == KM_E_ARG
            ms = C.c_float()
            assert lib.km_scan_kernel_ms(None) == KM_E_ARG and lib.km_scan_kernel_ms(C.byref(ms)) == 0
            # nothing to do: KM_OK, and nothing is touched
            out[:] = 7
            assert lib.kmjf_cov_seqs(db._h, None, None, 0, None, None) == 0
            assert lib.kmjf_cov_seqs(db._h, None, kmlib.ptr(np.array([5, 5, 5], np.uint64)), 2, kmlib.ptr(out), None) == 0
            assert (out["total"] == 7).all() and (out["max"] == 7).all()
            st = kmlib.DumpStats()
            assert lib.kmjf_scan_text(db._h, None, None, 0, null.fileno(), C.byref(st), None) == 0 and st.pieces == 0
            assert db.cov_seqs([]).size == 0 and cells(db.cov_seqs([b"", b""])) == [(0, 0, 0, 0, 0, NONE, 0)] * 2
            assert db.scan_text([], null) == {"records_in": 0, "records_out": 0, "bytes_out": 0, "pieces": 0}
        # a descriptor that is not open, and a reader that has gone away: KM_E_IO, and the library goes on
        r, w = os.pipe()
        os.close(r)
        try:
            with pytest.raises(kmlib.KmError) as e:
                db.scan_text([random_bases(np.random.default_rng(1), 200000)], w)
            assert e.value.code == KM_E_IO and "writing the text failed" in str(e.value)
        finally:
            os.close(w)
        with pytest.raises(kmlib.KmError) as e:
            db.scan_text([b"ACGT" * 10], w)
        assert e.value.code == KM_E_IO
        table, k, canonical = sc.file_table(NPM1)
        check(db, [b"ACGT" * 10, b"ACG"], table, k, canonical)
    finally:
        db.close()
