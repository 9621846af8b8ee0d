"""Low-complexity k-mers and every k from 2 to 32: homopolymers, microsatellites, palindromes, a k-mer beside its
own reverse complement, tables over the whole key space, every key width of a `.jf` file — the table, the walk and
the graph stage against plain models (a dict; oracle/km_oracle.py; oracle/km_oracle.c).  Every input is judged on the
oracle's side first: what a case is meant to show is asserted from the oracle's results alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

from km_amd import kmer as km
from km_amd import lib as kmlib
from km_amd import report, synth
from km_amd.finder import BatchFinder
from km_amd.jellyfish import Jellyfish
from oracle import c_oracle
from oracle import km_oracle as ko

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U32 = 0xFFFFFFFF
EDGE_COUNTS = np.array([0, 1, 4, 5, 6, 65534, 65535, 65536, U32], dtype=np.uint32)
WALK_KS = (11, 12, 16, 17, 21, 31, 32)


# ------------------------------------------------------------------ models
def _key_space(k):
    return np.arange(1 << (2 * k), dtype=np.uint64)


def _lookup(table, x, k, canonical):
    """km/utils/Jellyfish.py:47-53: the canonical form is looked up iff the table is canonical."""
    x = np.asarray(x, dtype=np.uint64)
    if canonical:
        x = km.canonical(x, k)
    return np.array([table.get(v, 0) for v in x.tolist()], dtype=np.uint32)


def _children_model(query, x, k, ratio, count, forward):
    """km/utils/Jellyfish.py:55-72 for an array of k-mers: (mask, counts4)."""
    x = np.asarray(x, dtype=np.uint64)
    kmask = np.uint64((1 << (2 * k)) - 1)
    kids = []
    for c in range(4):
        if forward:
            kids.append(((x << np.uint64(2)) & kmask) | np.uint64(c))
        else:
            kids.append((x >> np.uint64(2)) | np.uint64(c << (2 * (k - 1))))
    c4 = np.stack([query(kid) for kid in kids], axis=1)
    total = c4.astype(np.int64).sum(axis=1)
    floor = np.maximum(total.astype(np.float64) * float(ratio), float(count))
    keep = c4.astype(np.float64) >= floor[:, None]
    mask = (keep * np.array([1, 2, 4, 8])).sum(axis=1).astype(np.uint8)
    return mask, c4


def _dense_query(keys, counts, k, canonical):
    """Vector form of the dict model for a table inside a small key space."""
    dense = np.zeros(1 << (2 * k), dtype=np.uint32)
    dense[np.asarray(keys, dtype=np.int64)] = counts

    def query(x):
        x = np.asarray(x, dtype=np.uint64)
        return dense[(km.canonical(x, k) if canonical else x).astype(np.int64)]
    return query


def _check_lookups(db, query, probes, k):
    assert np.array_equal(db.query(probes), query(probes))
    for ratio, count in ((0.05, 5), (0.0, 0)):
        for forward in (True, False):
            mask, c4 = db.children(probes, ratio, count, forward)
            want_mask, want_c4 = _children_model(query, probes, k, ratio, count, forward)
            assert np.array_equal(c4, want_c4), (k, ratio, count, forward)
            assert np.array_equal(mask, want_mask), (k, ratio, count, forward)


# ------------------------------------------------------------------ B1: the whole key space
def _whole_space_records(k, canonical):
    """Every (canonical) key with edge and random counts, zero among them; for a canonical table also up to 300
    non-canonical keys whose count differs from their canonical form's: records that no query may reach."""
    rng = np.random.default_rng(9100 + 2 * k + canonical)
    space = _key_space(k)
    rc = km.revcomp(space, k)
    keys = space[space <= rc] if canonical else space
    counts = rng.integers(1, 70_000, size=keys.size).astype(np.uint32)
    edge = rng.random(keys.size) < 0.5
    counts[edge] = rng.choice(EDGE_COUNTS, size=int(edge.sum()))
    at = {int(x): i for i, x in enumerate(keys.tolist())}
    counts[at[0]] = 65536                                            # the homopolymer A^k: an escaped count
    n_pal = int((space == rc).sum())
    if k % 2 == 0:
        counts[at[km.pack_str("AT" * (k // 2))]] = U32               # a palindrome with an escaped count
        counts[at[km.pack_str("CG" * (k // 2))]] = 0                 # ... and one that is stored with count zero
    assert (counts == 0).any() and (counts >= 65535).any()
    n_hidden = 0
    if canonical:
        hidden = space[space > rc]
        hidden = hidden[rng.permutation(hidden.size)[:300]]
        canon_count = counts[[at[int(x)] for x in rc[hidden.astype(np.int64)].tolist()]]
        hidden_count = (canon_count.astype(np.uint64) + np.uint64(7)).astype(np.uint32)
        hidden_count[hidden_count == 0] = 3                          # (never zero: a dropped record would hide a leak)
        assert (hidden_count != canon_count).all()
        n_hidden = hidden.size
        order = rng.permutation(keys.size + hidden.size)             # the hidden records anywhere among the others
        keys = np.concatenate([keys, hidden])[order]
        counts = np.concatenate([counts, hidden_count])[order]
    return keys, counts, n_pal, n_hidden


@gpu
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", range(2, 9))
def test_whole_key_space_lookups_and_children(k, canonical):
    keys, counts, n_pal, n_hidden = _whole_space_records(k, canonical)
    stored_canonical = keys[keys <= km.revcomp(keys, k)]
    pal = int((stored_canonical == km.revcomp(stored_canonical, k)).sum())
    assert pal == n_pal == (4 ** (k // 2) if k % 2 == 0 else 0)      # the one-orientation branch runs iff k is even
    if canonical:
        assert n_hidden == min(300, (4 ** k - n_pal) // 2) and keys.size == (4 ** k + n_pal) // 2 + n_hidden
    table = dict(zip(keys.tolist(), counts.tolist()))
    assert len(table) == keys.size
    db = kmlib.Database.from_records(keys, counts, k, canonical).upload(0)
    space = _key_space(k)
    want = _lookup(table, space, k, canonical)
    query = _dense_query(keys[keys <= km.revcomp(keys, k)] if canonical else keys,
                         counts[keys <= km.revcomp(keys, k)] if canonical else counts, k, canonical)
    assert np.array_equal(query(space), want)                        # the vector model is the dict model
    _check_lookups(db, query, space, k)
    db.close()


@gpu
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [2, 5, 16, 31, 32])
def test_empty_and_one_record_tables(k, canonical):
    rng = np.random.default_rng(9200 + k)
    top = (1 << (2 * k)) - 1
    probes = np.unique(np.concatenate([rng.integers(0, top, size=200, dtype=np.uint64, endpoint=True),
                                       np.array([0, top], dtype=np.uint64)]))
    empty = kmlib.Database.empty(k, canonical).upload(0)
    assert empty.info.k == k and not empty.query(probes).any()
    for forward in (True, False):
        mask, c4 = empty.children(probes, 0.05, 5, forward)
        assert not mask.any() and not c4.any()
        mask, c4 = empty.children(probes, 0.0, 0, forward)           # a floor of zero keeps every child, present or not
        assert (mask == 15).all() and not c4.any()
    empty.close()
    seq = "ACGTTGCATCGGATACCTGAGTCAAGCTTAGCGA"[:k]
    key = km.pack_str(seq)
    if canonical:
        key = int(km.canonical(np.array([key], dtype=np.uint64), k)[0])
    for cnt in (1, 7, 65535, U32):
        one = kmlib.Database.from_records(np.array([key], np.uint64), np.array([cnt], np.uint32), k, canonical).upload(0)
        table = {key: cnt}
        near = np.array([key, int(km.revcomp(np.array([key], np.uint64), k)[0]), key ^ 1, key ^ 2,
                         (key >> 2), ((key << 2) & top), (key >> 2) | (3 << (2 * (k - 1))), ((key << 2) & top) | 3],
                        dtype=np.uint64)
        ask = np.unique(np.concatenate([probes, near]))

        def query(x):
            return _lookup(table, x, k, canonical)
        assert int(one.query(np.array([key], np.uint64))[0]) == cnt
        _check_lookups(one, query, ask, k)
        one.close()


# ------------------------------------------------------------------ B2: every key width through the file path
def _file_records(k):
    rng = np.random.default_rng(9300 + k)
    if 4 ** k <= 6000:
        keys = _key_space(k)
    else:
        top = (1 << (2 * k)) - 1
        keys = rng.integers(0, top, size=6000, dtype=np.uint64, endpoint=True)
    keys = np.unique(km.canonical(keys, k))
    counts = rng.integers(1, 5000, size=keys.size).astype(np.uint32)
    edge = rng.random(keys.size) < 0.1
    counts[edge] = rng.choice(EDGE_COUNTS, size=int(edge.sum()))
    top = (1 << (2 * k)) - 1
    absent = rng.integers(0, top, size=2000, dtype=np.uint64, endpoint=True)
    return keys, counts, absent


@gpu
@pytest.mark.parametrize("chunk_kb", [None, 16])
@pytest.mark.parametrize("ks", [range(2, 12), range(12, 22), range(22, 33)], ids=["k2-11", "k12-21", "k22-32"])
def test_every_key_width_through_the_file_path(ks, chunk_kb, tmp_path, monkeypatch):
    """Key bytes 1 .. 8 (k = 2 .. 32): the unpack kernel of the direct ingestion, the host reader and from_records
    must build the same table; with 16 KB chunks a file crosses the two pinned buffers several times."""
    if chunk_kb:
        monkeypatch.setenv("KM_LOAD_CHUNK_KB", str(chunk_kb))
    widths = set()
    for k in ks:
        keys, counts, absent = _file_records(k)
        widths.add((2 * k + 7) // 8)
        path = str(tmp_path / ("k%d.jf" % k))
        synth.write_jf(path, keys, counts, k)
        table = dict(zip(keys.tolist(), counts.tolist()))
        ask = np.concatenate([keys, km.revcomp(keys, k), absent])
        want = _lookup(table, ask, k, True)
        assert np.array_equal(want[:keys.size], counts) and np.array_equal(want[keys.size:2 * keys.size], counts)
        if k >= 12:
            assert int((want[2 * keys.size:] == 0).sum()) > 1900     # (the absent keys are absent)
        for how in ("load", "open", "records"):
            if how == "load":
                db = kmlib.Database.load(path, 0)
            elif how == "open":
                db = kmlib.Database.open(path).upload(0)
            else:
                db = kmlib.Database.from_records(keys, counts, k).upload(0)
            assert db.info.k == k and db.info.canonical
            assert np.array_equal(db.query(ask), want), (k, how)
            db.close()
    assert widths == set(range((2 * ks[0] + 7) // 8, (2 * ks[-1] + 7) // 8 + 1))


# ------------------------------------------------------------------ walk comparisons
def _run(db, seqs, ratio=0.05, count=5, steps=500, branchs=10, nodes=10000, flags=0, stream=None):
    b = kmlib.Batch(db, ratio=ratio, count=count, max_stack=steps, max_break=branchs, max_node=nodes,
                    max_targets=max(64, len(seqs)), max_total_bases=max(1 << 14, sum(len(s) for s in seqs)))
    b.set_targets(seqs)
    if flags:
        b.run(kmlib.KM_STAGE_WALK | kmlib.KM_STAGE_GRAPH | flags, stream)
        r = {key: (np.array(val) if isinstance(val, np.ndarray) else val) for key, val in b.result().items()}
    else:
        b.run()
        r = b.fetch()
    b.close()
    return r


def _target(r, t, k):
    a, e = int(r["node_off"][t]), int(r["node_off"][t + 1])
    p0, p1 = int(r["path_off"][t]), int(r["path_off"][t + 1])
    return {"status": int(r["status"][t]), "n_ref": int(r["n_ref"][t]), "kmers": r["node_kmer"][a:e].tolist(),
            "counts": r["node_count"][a:e].tolist(), "probes": int(r["probes"][t]),
            "paths": [kmlib.expand_path(r, p).tolist() for p in range(p0, p1)],
            "min_cov": r["path_min_cov"][p0:p1].tolist()}


def _c_want(co, seq, **prm):
    w = co.analyse(km.encode(seq), **prm)
    return {"status": w["status"], "kmers": w["kmers"].tolist(), "counts": w["counts"].tolist(),
            "probes": w["probes"], "paths": w["paths"], "min_cov": w["min_cov"]}


def _equal(got, want, ctx):
    assert got["status"] == want["status"], ctx
    if want["status"] != kmlib.T_OK:
        return
    for field in ("kmers", "counts", "probes", "paths", "min_cov"):
        assert got[field] == want[field], (ctx, field)


def _against_c(db, co, k, seqs, ctx, steps=500, branchs=10, nodes=10000, ratio=0.05, count=5, wants=None):
    r = _run(db, seqs, ratio, count, steps, branchs, nodes)
    out = []
    for t, seq in enumerate(seqs):
        want = wants[t] if wants else _c_want(co, seq, ratio=ratio, count=count, max_stack=steps, max_break=branchs,
                                              max_node=nodes)
        _equal(_target(r, t, k), want, (ctx, t, steps, branchs, nodes))
        out.append(want)
    return r, out


def _py_want(py, seq, name, k, steps=500, branchs=10, nodes=10000):
    try:
        w = ko.analyse_target(seq, name, py, steps, branchs, nodes)
    except ko.NodeLimit:
        return {"status": kmlib.T_NODE_LIMIT}
    return {"status": 0, "kmers": [km.pack_str(x) for x in w["kmers"]], "counts": w["counts"], "probes": w["probes"],
            "paths": [list(p) for p in w["paths"]], "min_cov": w["min_cov"], "res": w}


# ------------------------------------------------------------------ B3: the walk at every k
def _sweep_case(k, canonical):
    if k >= 11:
        case = synth.make_case(n_targets=12, length=2 * k + 60, k=k, n_keys=5000, seed=500 + k, variant_frac=0.8,
                               branch_noise_frac=0.02, canonical=canonical)
        return case["keys"], case["counts"], [km.decode(r) for r in case["targets"]]
    case = synth.small_k_case(k, canonical)
    return case["keys"], case["counts"], case["targets"]


def _limit_for(k, seqs):
    """max_node of the node-limit run: n_ref + 3 (of the median target where the lengths differ)."""
    return sorted(len(s) - k + 1 for s in seqs)[len(seqs) // 2] + 3


def _sweep_oracle(k):
    """Per `canonical`: records, targets, the C oracle's results at the default budgets and with max_node = n_ref + 3;
    asserts — from the oracle alone — that the inputs show what the sweep is for."""
    out = []
    n_multi = n_limit = n_targets = 0
    for canonical in (True, False):
        keys, counts, seqs = _sweep_case(k, canonical)
        assert len(np.unique(keys)) == keys.size
        for s in seqs:
            assert not synth.has_repeated_kmer(s, k) and len(s) <= 200
        co = c_oracle.COracle(keys, counts, k, canonical)
        wants = [_c_want(co, s) for s in seqs]
        assert all(w["status"] == 0 for w in wants), (k, canonical)
        limit = _limit_for(k, seqs)
        tight = [_c_want(co, s, max_node=limit) for s in seqs]
        assert {w["status"] for w in tight} <= {kmlib.T_OK, kmlib.T_NODE_LIMIT}
        n_multi += sum(len(w["paths"]) > 1 for w in wants)
        n_limit += sum(w["status"] == kmlib.T_NODE_LIMIT for w in tight)
        n_targets += len(seqs)
        out.append((canonical, keys, counts, seqs, co, wants, limit, tight))
    assert n_targets == 24 and 4 * n_multi >= n_targets, (k, n_multi)
    return out, n_multi, n_limit


@pytest.mark.parametrize("k", range(2, 33))
def test_sweep_inputs_branch_at_every_k(k):
    """CPU: what test_walk_at_every_k rests on, from the C oracle alone (status 0 everywhere, a quarter of the targets
    with several paths, the node limit met)."""
    _, n_multi, n_limit = _sweep_oracle(k)
    assert n_limit >= 1, k


@gpu
@pytest.mark.parametrize("k", range(2, 33))
def test_walk_at_every_k(k):
    """Statuses, node k-mers, node counts, logical probes, paths in order and min coverages against the C oracle,
    canonical and not, at the default budgets and with max_node = n_ref + 3."""
    cases, _, n_limit = _sweep_oracle(k)
    assert n_limit >= 1
    for canonical, keys, counts, seqs, co, wants, limit, tight in cases:
        db = kmlib.Database.from_records(keys, counts, k, canonical).upload(0)
        _against_c(db, co, k, seqs, (k, canonical), wants=wants)
        _against_c(db, co, k, seqs, (k, canonical, "limit"), nodes=limit, wants=tight)
        db.close()


# ------------------------------------------------------------------ B4: structured walks
def _tables(case, canonical=True):
    k = case["k"]
    keys, counts = synth.reads_to_records(case["reads"], k, canonical)
    co = c_oracle.COracle(keys, counts, k, canonical)
    py = ko.KmerDB(None, 0.05, 5, records={"k": k, "canonical": canonical, "keys": keys, "counts": counts})
    return keys, counts, co, py


def _oracle_side(case, c, p):
    """What each structured case is meant to show, on the oracles' results (C == Python first)."""
    k, T = case["k"], case["target"]
    n_ref = len(T) - k + 1
    assert c["status"] == p["status"] == 0, case["name"]
    for field in ("kmers", "counts", "probes", "paths", "min_cov"):
        assert c[field] == p[field], (case["name"], field)
    name = case["name"]
    nodes = [km.unpack(x, k) for x in c["kmers"]]
    assert len(set(nodes)) == len(nodes)
    if name.startswith("rep_"):
        unit = name.split("_")[1]
        assert len(nodes) > n_ref                                    # the repeat was entered
        rot = {(unit * k)[i:i + k] for i in range(len(unit))}
        assert rot <= set(nodes[n_ref:]) | set(nodes[:n_ref]) and rot & set(nodes[n_ref:])   # ... and circled
        if len(unit) == 2 and k % 2 == 1 and unit in ("AT", "TA"):   # one record serves both nodes of the 2-cycle
            a, b = sorted(rot)
            assert synth.revcomp_str(a) == b
    elif name.startswith("inv"):
        assert len(c["paths"]) >= 2
        strings = set(nodes)
        assert sum(synth.revcomp_str(x) in strings for x in nodes) >= 2 * k   # k-mers beside their reverse complement
    elif name.startswith("hairpin"):
        strings = set(nodes)
        assert all(synth.revcomp_str(x) in strings for x in nodes[:n_ref])
        mid = (len(T) - k) // 2
        doubled = [x for i, x in enumerate(c["counts"][:n_ref]) if not (k % 2 == 0 and i == mid)]
        assert set(doubled) == {100}                                 # every count doubled ...
        if k % 2 == 0:                                               # ... but the centre k-mer's: it is its own reverse complement
            assert nodes[mid] == synth.revcomp_str(nodes[mid]) and c["counts"][mid] == 50
        assert c["paths"] == [list(range(n_ref))]
    elif name.startswith("enddup"):
        ref = list(range(n_ref))
        assert c["paths"][0] == ref and len(c["paths"]) == 2 and c["paths"][1][:n_ref] == ref
        assert len(c["paths"][1]) == n_ref + k + 5 and c["min_cov"] == [90, 30]


def _structured(k):
    out = []
    for case in synth.structured_cases(k):
        keys, counts, co, py = _tables(case)
        c = _c_want(co, case["target"])
        p = _py_want(py, case["target"], case["name"], k)
        _oracle_side(case, c, p)
        out.append((case, keys, counts, co, py, c, p))
    return out


@pytest.mark.parametrize("k", WALK_KS)
def test_structured_inputs_show_what_they_are_for(k):
    """CPU: the two oracles agree on every structured case, and each case shows its structure."""
    _structured(k)


@gpu
@pytest.mark.parametrize("k", WALK_KS)
def test_structured_walks(k):
    """Repeats entered from the target and never left (homopolymers, (AT)n, (CG)n), an inversion, a hairpin target, a
    duplication reaching the target's end: the GPU against both oracles; the repeats again under stack, break and
    node budgets that cut the circling walk at every early length."""
    for case, keys, counts, co, py, c, p in _structured(k):
        T, name = case["target"], case["name"]
        db = kmlib.Database.from_records(keys, counts, k).upload(0)
        assert np.array_equal(db.query(keys), counts)
        _against_c(db, co, k, [T], name, wants=[c])                  # (c == p was asserted on the oracle's side)
        if name.startswith("rep_"):
            n_ref = len(T) - k + 1
            for steps in (1, 2, 3, 4, 5, 6, 63, 64, 65, 66):
                _, w = _against_c(db, co, k, [T], name, steps=steps)
                _equal(w[0], _py_want(py, T, name, k, steps=steps), (name, "py", steps))
            for branchs in (0, 1, 2):
                _, w = _against_c(db, co, k, [T], name, branchs=branchs)
                _equal(w[0], _py_want(py, T, name, k, branchs=branchs), (name, "py", branchs))
            for nodes in (n_ref, n_ref + 1, n_ref + 5):
                _, w = _against_c(db, co, k, [T], name, nodes=nodes)
                _equal(w[0], _py_want(py, T, name, k, nodes=nodes), (name, "py", nodes))
        db.close()


@gpu
@pytest.mark.parametrize("k", [11, 21, 31, 32])
def test_prefix_path_order_in_all_three_reports(k):
    """The duplication reaching the target's end through the three reports: the oracle's rows, the Python report of
    the GPU result and the native report of the GPU result — rows in the reports' own order, cluster numbers
    included."""
    case = synth.end_duplication_case(k)
    keys, counts, co, py = _tables(case)
    want = ko.analyse_target(case["target"], case["name"], py)
    assert [len(x) for x in want["paths"]] == [want["n_ref"], want["n_ref"] + k + 5]
    db = kmlib.Database.from_records(keys, counts, k).upload(0)
    jf = Jellyfish("mem.jf", cutoff=0.05, n_cutoff=5, db=db)
    finder = BatchFinder(jf)
    targets = [(case["name"], case["target"])]
    res = finder.analyse(targets)[0]
    assert [p.tolist() for p in res.paths] == [list(p) for p in want["paths"]]
    rows = ko.target_rows(want, "mem.jf")
    assert len(rows) == 3 and sum("cluster 1 n=1" in r for r in rows) == 1
    assert report.target_rows(res, "mem.jf") == rows
    assert finder.rows(targets) == [rows]
    db.close()


STATUS_TARGETS = ("A" * 30, "AT" * 15)


@gpu
@pytest.mark.parametrize("k", WALK_KS)
def test_statuses_of_degenerate_targets(k):
    """Homopolymer and (AT)n targets (a repeated k-mer), a target shorter than k, one of exactly k bases (one node,
    one path) and one of k + 1: the C oracle's statuses and results."""
    rng = np.random.default_rng(9500 + k)
    base = synth.unique_kmer_seq(rng, k + 1, k)
    seqs = list(STATUS_TARGETS) + ["A" * (k + 2), "AT" * k, base[:k - 1], base[:k], base]
    keys, counts = synth.records_from_reads([(base, 50), ("A" * (k + 2), 20), ("AT" * k, 20)], k)
    co = c_oracle.COracle(keys, counts, k, True)
    wants = [_c_want(co, s) for s in seqs]
    st = [w["status"] for w in wants]
    short = kmlib.T_EMPTY if k > 30 else kmlib.T_REPEAT_KMER         # "A" * 30 has no 31-mer
    assert st == [short, short, kmlib.T_REPEAT_KMER, kmlib.T_REPEAT_KMER, kmlib.T_EMPTY, kmlib.T_OK, kmlib.T_OK]
    assert wants[5]["paths"] == [[0]] and len(wants[5]["kmers"]) == 1
    assert wants[6]["paths"] == [[0, 1]] and len(wants[6]["kmers"]) == 2
    db = kmlib.Database.from_records(keys, counts, k).upload(0)
    _against_c(db, co, k, seqs, ("status", k), wants=wants)
    db.close()


@gpu
@pytest.mark.parametrize("k", WALK_KS)
def test_homopolymer_node_between_two_target_kmers(k):
    """One more base in a run of k - 1 equal ones of the target: the only discovered node is c^k, a one-node bubble
    whose k-mer is behind its own suffix.  No path goes through it twice: the reference's graph has no edge from a
    node to itself (the epilogue of k_dfs once took that for a looped tandem duplication)."""
    for base in "ACGT":
        case = synth.homopolymer_insertion_case(k, base)
        keys, counts, co, py = _tables(case)
        c = _c_want(co, case["target"])
        p = _py_want(py, case["target"], case["name"], k)
        for field in ("status", "kmers", "counts", "probes", "paths", "min_cov"):
            assert c[field] == p[field], (case["name"], field)
        n_ref = len(case["target"]) - k + 1
        a = case["target"].index(base * (k - 1)) - 1
        assert c["kmers"][n_ref:] == [km.pack_str(base * k)]
        assert c["paths"] == sorted([list(range(n_ref)), list(range(a + 1)) + [n_ref] + list(range(a + 1, n_ref))])
        db = kmlib.Database.from_records(keys, counts, k).upload(0)
        _against_c(db, co, k, [case["target"]], case["name"], wants=[c])
        db.close()


def _all_t_case():
    k = 32
    rng = np.random.default_rng(9600)
    while True:
        T = synth.random_seq(rng, k + 5) + "T" * 6 + synth.random_seq(rng, k + 7)
        if not synth.has_repeated_kmer(T, k):
            break
    reads = [(T, 50), (T[:k + 5 + 6] + "T" * (k + 4), 30)]
    return T, reads


@gpu
def test_all_t_key_of_a_non_canonical_k32_table():
    """T^32 is the key with every bit set: the marker of an empty slot in the counter's table means nothing to the
    finder's, neither as a record nor as a node of the walk."""
    k = 32
    T, reads = _all_t_case()
    keys, counts = synth.reads_to_records(reads, k, canonical=False)
    all_t = np.uint64(0xFFFFFFFFFFFFFFFF)
    assert all_t in keys and int(counts[keys == all_t][0]) == 30 * 11       # 6 + k + 4 bases of T: 11 windows
    co = c_oracle.COracle(keys, counts, k, False)
    py = ko.KmerDB(None, 0.05, 5, records={"k": k, "canonical": False, "keys": keys, "counts": counts})
    c = _c_want(co, T)
    p = _py_want(py, T, "allT", k)
    for field in ("status", "kmers", "counts", "probes", "paths", "min_cov"):
        assert c[field] == p[field], field
    assert int(all_t) in c["kmers"][len(T) - k + 1:]                 # the walk reaches T^32 ...
    assert c["counts"][c["kmers"].index(int(all_t))] == 330
    db = kmlib.Database.from_records(keys, counts, k, False).upload(0)
    assert np.array_equal(db.query(keys), counts)
    mask, c4 = db.children(np.array([all_t], np.uint64), 0.05, 5, True)
    assert int(mask[0]) == 8 and c4[0].tolist() == [0, 0, 0, 330]    # ... whose only child is itself
    _against_c(db, co, k, [T], "allT", wants=[c])
    for steps in (1, 5, 40):
        _against_c(db, co, k, [T], "allT", steps=steps)
    db.close()


# ------------------------------------------------------------------ B4 again: speculation off, 16-bit delivery
_FIELDS = ("status", "n_ref", "probes", "node_off", "node_kmer", "node_count", "path_off", "run_off", "run_start",
           "run_len", "path_len", "path_min_cov")


def _structured_batches():
    """(k, name, canonical, keys, counts, target) of every structured case, the all-T one included."""
    for k in WALK_KS:
        for case in synth.structured_cases(k):
            keys, counts = synth.records_from_reads(case["reads"], k)
            yield k, case["name"], True, keys, counts, case["target"]
    T, reads = _all_t_case()
    keys, counts = synth.reads_to_records(reads, 32, canonical=False)
    yield 32, "allT", False, keys, counts, T


_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(here)r]
import numpy as np
import test_structured_kmers as me
from km_amd import lib as kmlib
out = {}
for k, name, canonical, keys, counts, seq in me._structured_batches():
    db = kmlib.Database.from_records(keys, counts, k, canonical).upload(0)
    r = me._run(db, [seq])
    for field in me._FIELDS:
        out[name + "_" + field] = r[field]
    db.close()
np.savez(%(out)r, **out)
"""


@gpu
def test_structured_walks_without_speculation_and_with_sixteen_bit_counts(tmp_path):
    """Every structured case once more: the same arrays with the chain speculation off (KM_SPECULATE=0 is read once
    per process: a child process) and the same results through the 16-bit delivery of the node counts."""
    mine = {}
    st = kmlib.stream_create(0)
    lean = kmlib.KM_RUN_DELIVER | kmlib.KM_DELIVER_LEAN
    for k, name, canonical, keys, counts, seq in _structured_batches():
        co = c_oracle.COracle(keys, counts, k, canonical)
        db = kmlib.Database.from_records(keys, counts, k, canonical).upload(0)
        mine[name], wants = _against_c(db, co, k, [seq], name)
        assert wants[0]["status"] == 0
        v32 = _run(db, [seq], flags=lean, stream=st)
        v16 = _run(db, [seq], flags=lean | kmlib.KM_DELIVER_COUNT16, stream=st)
        assert "node_count16" in v16 and "node_count16" not in v32
        for key in ("status", "n_ref", "probes", "node_off", "node_count", "extra_off", "extra_kmer", "path_off",
                    "run_off", "run_start", "run_len", "path_len", "path_min_cov", "ref_max_cov"):
            assert np.array_equal(v16[key], v32[key]), (name, key)
        assert np.array_equal(v32["path_min_cov"], mine[name]["path_min_cov"]), name      # (a lean delivery skips the nodes
        if len(v32["node_count"]):                                                          # of a target with one path)
            assert np.array_equal(v32["node_count"], mine[name]["node_count"]), name
        assert kmlib.report_rows(v16, [name], [seq], k, "mem.jf") == kmlib.report_rows(v32, [name], [seq], k, "mem.jf")
        db.close()
    kmlib.stream_destroy(st)
    out = str(tmp_path / "spec_off.npz")
    subprocess.check_call([sys.executable, "-c", _CHILD % {"root": os.path.dirname(HERE), "here": HERE, "out": out}],
                          env=dict(os.environ, KM_SPECULATE="0"))
    off = np.load(out)
    assert len(mine) == 9 * len(WALK_KS) + 1
    for name, r in mine.items():
        for field in _FIELDS:
            assert np.array_equal(r[field], off[name + "_" + field]), (name, field)
