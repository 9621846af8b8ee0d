"""One batch workspace reused across changing target sets and run modes, as the product uses it: km_amd/cli.py feeds
one BatchFinder catalog chunk after chunk, bench.py and tools/kmclient.cpp set new targets before every step.  A
workspace carries state from one set to the next (the k_dfs / k_graph grids, the armed device large tier, the node
layout moved by the large tier, a captured hipGraph, the first delivery copy's size, the pinned buffer, the 16-bit
count form); every step here must give what a fresh workspace gives for that set, and the fresh results are checked
against the plain-C oracle.  Consecutive sets of the sequence are checked to give different results, so a stale
replay or a stale delivery cannot pass."""
import io

import numpy as np
import pytest

from km_amd import kmer as km
from km_amd import lib as kmlib
from km_amd import synth
from km_amd.finder import BatchFinder
from km_amd.jellyfish import Jellyfish
from oracle import km_oracle as ko

pytestmark = pytest.mark.gpu

K = 31
MAX_TARGETS, MAX_BASES = 500, 150_000
BOTH = kmlib.KM_STAGE_WALK | kmlib.KM_STAGE_GRAPH
DELIVER = BOTH | kmlib.KM_RUN_DELIVER
_R4_FIELDS = ("status", "n_ref", "probes", "node_off", "node_kmer", "node_count", "path_off", "run_off", "run_start",
              "run_len", "path_len", "path_min_cov")
_VIEW_FIELDS = ("status", "n_ref", "probes", "path_off", "run_off", "run_start", "run_len", "path_len", "path_min_cov",
                "extra_off", "extra_kmer", "ref_max_cov")


def _seqs(case, lengths=None):
    out = [km.decode(r) for r in case["targets"]]
    return out if lengths is None else [s[:L] for s, L in zip(out, lengths)]


def _make_sets():
    light = synth.make_case(n_targets=500, length=300, n_keys=40_000, seed=9101, variant_frac=0.04, exact_pad=False)
    heavy = synth.make_case(n_targets=500, length=300, n_keys=40_000, seed=9102, variant_frac=0.9,
                            variants_per_target=(1, 3), hom_frac=0.3, branch_noise_frac=0.05, exact_pad=False)
    twin = synth.make_case(n_targets=500, length=300, n_keys=40_000, seed=9103, variant_frac=0.04, exact_pad=False)
    big = synth.make_case(n_targets=10, length=3000, n_keys=30_000, seed=9104, variant_frac=0.6,
                          variants_per_target=(1, 2), exact_pad=False)
    small = synth.make_case(n_targets=50, length=300, n_keys=20_000, seed=9105, variant_frac=0.4, exact_pad=False)
    dups = synth.make_case(n_targets=60, length=700, n_keys=40_000, seed=9106, variant_frac=0.6,
                           variants_per_target=(1, 11), kinds=("ins", "dup", "snv"), vaf=(0.3, 0.5), exact_pad=False)
    hot = synth.make_case(n_targets=300, length=250, n_keys=30_000, seed=9107, variant_frac=0.3,
                          cov=(80_000, 400_000), exact_pad=False)
    full = synth.make_case(n_targets=500, length=350, n_keys=40_000, seed=9108, variant_frac=0.3, exact_pad=False)
    cases = [light, heavy, twin, big, small, dups, hot, full]
    keys = np.concatenate([c["keys"] for c in cases])
    counts = np.concatenate([c["counts"] for c in cases])
    keys, first = np.unique(keys, return_index=True)
    counts = counts[first]

    long_seqs = []
    for i, s in enumerate(_seqs(big, [2200 + 80 * i for i in range(10)])):
        long_seqs += [s] + _seqs({"targets": small["targets"][3 * i:3 * i + 3]})
    plain = _seqs({"targets": small["targets"][30:50]})
    rep = plain[0][:150] + plain[0][60:100] + plain[0][150:]
    errors = plain[1:8] + [plain[8][:20]] + plain[9:14] + [plain[14][:100] + "N" + plain[14][101:]] + plain[15:18] \
        + [rep] + plain[18:20]
    sets = {
        "light": _seqs(light),
        "heavy": _seqs(heavy),
        "twin": _seqs(twin),
        "long": long_seqs,
        "dups": _seqs(dups),
        "hot": _seqs(hot),
        "tiny": [_seqs(light)[7][:K]],
        "empty": [],
        "errors": errors,
        "full": _seqs(full, [250 if i % 2 else 350 for i in range(500)]),
    }
    assert len(sets["full"]) == MAX_TARGETS and sum(len(s) for s in sets["full"]) == MAX_BASES
    assert len(sets["twin"]) == len(sets["light"]) and [len(s) for s in sets["twin"]] == [len(s) for s in sets["light"]]
    assert len(sets["long"]) == 40 and sum(len(s) > 2000 for s in sets["long"]) == 10
    hot_c = counts[np.searchsorted(keys, np.unique(km.canonical(km.sliding_kmers(hot["targets"], K).ravel(), K)))]
    assert int((hot_c >= 0xFFFF).sum()) > 4 * 2048
    return keys, counts, sets


def _fresh(db, co, name, seqs):
    """What a workspace that has never seen another set gives for `seqs`, checked against the C oracle."""
    b = kmlib.Batch(db, max_targets=MAX_TARGETS, max_total_bases=MAX_BASES)
    b.set_targets(seqs)
    b.run()
    f = b.fetch()
    b.run(DELIVER)
    v = b.result()
    for key in ("status", "n_ref", "probes", "node_off", "node_count", "path_off", "run_off", "run_start", "run_len",
                "path_len", "path_min_cov"):
        assert np.array_equal(np.asarray(v[key]), f[key]), (name, key)
    for key in ("extra_off", "extra_kmer", "ref_max_cov"):
        f[key] = np.array(v[key])
    b.close()
    n = len(seqs)
    noff, poff = f["node_off"].astype(np.int64), f["path_off"].astype(np.int64)
    # the delivery's own fields, from the fetched arrays
    tid = np.repeat(np.arange(n), np.diff(noff))
    own = np.arange(int(noff[-1])) - noff[tid] < f["n_ref"].astype(np.int64)[tid]
    assert np.array_equal(f["node_kmer"][~own], f["extra_kmer"]), name
    for t in np.nonzero(f["ref_max_cov"] != 0xFFFFFFFF)[0]:
        assert poff[t + 1] - poff[t] == 1 and int(f["ref_max_cov"][t]) == int(f["node_count"][noff[t]:noff[t + 1]].max())
    every = 1 if name in ("tiny", "errors") else 5
    for t in range(0, n, every):
        if "N" in seqs[t]:
            assert int(f["status"][t]) == kmlib.T_BAD_BASE
            continue
        want = co.analyse(km.encode(seqs[t]))
        assert int(f["status"][t]) == want["status"], (name, t)
        if want["status"] != 0:
            continue
        assert np.array_equal(f["node_kmer"][noff[t]:noff[t + 1]], want["kmers"]), (name, t)
        assert np.array_equal(f["node_count"][noff[t]:noff[t + 1]], want["counts"]), (name, t)
        assert int(f["probes"][t]) == want["probes"], (name, t)
        assert [kmlib.expand_path(f, p).tolist() for p in range(poff[t], poff[t + 1])] == want["paths"], (name, t)
        assert f["path_min_cov"][poff[t]:poff[t + 1]].tolist() == want["min_cov"], (name, t)
    names = ["%s_%d" % (name, i) for i in range(n)]
    f["_names"] = names
    f["_rows"] = kmlib.report_rows(f, names, seqs, K, "mem.jf") if n else []
    return f


def _differ(a, b):
    return not all(np.array_equal(a[key], b[key]) for key in ("status", "node_off", "node_count", "path_off",
                                                             "run_start", "path_min_cov"))


def _check_fetch(got, want, tag):
    for key in _R4_FIELDS:
        assert np.array_equal(got[key], want[key]), (tag, key)


def _check_view(v, want, tag, lean=False, walk_only=False):
    if walk_only:
        for key in ("status", "n_ref", "probes", "node_off", "node_count", "extra_off", "extra_kmer"):
            assert np.array_equal(np.asarray(v[key]), want[key]), (tag, key)
        assert int(np.asarray(v["path_off"])[-1]) == 0, tag
        return
    for key in _VIEW_FIELDS:
        assert np.array_equal(np.asarray(v[key]), want[key]), (tag, key)
    nc = np.asarray(v["node_count"])
    if lean:
        bare = want["ref_max_cov"] != 0xFFFFFFFF
        got_len = np.diff(np.asarray(v["node_off"]).astype(np.int64))
        want_len = np.diff(want["node_off"].astype(np.int64))
        assert (got_len[bare] == 0).all() and np.array_equal(got_len[~bare], want_len[~bare]), tag
        assert np.array_equal(nc, want["node_count"][np.repeat(~bare, want_len)]), tag
    else:
        assert np.array_equal(np.asarray(v["node_off"]), want["node_off"]), tag
        assert np.array_equal(nc, want["node_count"]), tag
    if "node_count16" in v:
        assert np.array_equal(np.asarray(v["node_count16"]), np.minimum(nc, 0xFFFF).astype(np.uint16)), tag


# (set, mode): `reject` keeps the set of the step before, `inflight` starts an un-awaited delivered run of the
# previous set right before the new set is given
SEQUENCE = [
    ("light", "fetch"), ("heavy", "fetch"), ("light", "lean"), ("long", "deliver"), ("light", "c16"),
    ("dups", "fetch"), ("light", "deliver"), ("hot", "c16"), ("light", "c16"), ("light", "graph"),
    ("twin", "graph"), ("heavy", "serial"), ("empty", "fetch"), ("long", "lean"), ("tiny", "deliver"),
    ("heavy", "walk"), ("errors", "fetch"), ("light", "dev"), ("long", "fetch"), ("full", "lean"),
    ("full", "reject"), ("dups", "graph"), ("heavy", "inflight"), ("errors", "lean"), ("light", "walk"),
    ("hot", "fetch"), ("tiny", "c16"), ("long", "graph"), ("empty", "deliver"), ("twin", "c16"),
    ("light", "inflight"), ("heavy", "lean"), ("dups", "dev"), ("light", "serial"), ("light", "reject"),
    ("full", "c16"), ("heavy", "graph"), ("tiny", "fetch"), ("errors", "c16"), ("twin", "lean"),
    ("hot", "deliver"), ("long", "inflight"), ("full", "fetch"), ("tiny", "walk"), ("dups", "c16"),
    ("twin", "dev"), ("heavy", "deliver"), ("empty", "lean"), ("light", "fetch"),
]


def _covers(seq):
    pairs = set()
    for (a, _ma), (b, mb) in zip(seq, seq[1:]):
        pairs.add((a, b, mb))
    return pairs


def test_sequence_covers_every_transition():
    pairs = _covers(SEQUENCE)
    trans = {(a, b) for a, b, _m in pairs}
    modes = {m for _s, m in SEQUENCE}
    assert len(SEQUENCE) >= 40
    assert modes == {"fetch", "deliver", "lean", "c16", "graph", "serial", "walk", "dev", "inflight", "reject"}
    for need in [("light", "heavy"), ("heavy", "light"), ("long", "light"), ("dups", "light"), ("long", "full"),
                 ("heavy", "empty"), ("empty", "long"), ("long", "tiny"), ("tiny", "heavy"),
                 ("heavy", "errors"), ("errors", "light")]:
        assert need in trans, need
    assert ("hot", "light", "c16") in pairs and ("light", "twin", "graph") in pairs
    rejects = [i for i, (_s, m) in enumerate(SEQUENCE) if m == "reject"]
    assert all(SEQUENCE[i][0] == SEQUENCE[i - 1][0] for i in rejects)


@pytest.fixture(scope="module")
def world():
    keys, counts, sets = _make_sets()
    db = kmlib.Database.from_records(keys, counts, K).upload(0)
    from oracle import c_oracle
    co = c_oracle.COracle(keys, counts, K)
    fresh = {name: _fresh(db, co, name, seqs) for name, seqs in sets.items()}
    yield {"db": db, "sets": sets, "fresh": fresh, "keys": keys, "counts": counts}
    db.close()


def _rows_equal(res, name, world, tag):
    seqs = world["sets"][name]
    if not seqs:
        return
    w = world["fresh"][name]
    assert kmlib.report_rows(res, w["_names"], seqs, K, "mem.jf") == w["_rows"], tag


def _copy(view):
    return {key: (np.array(val) if isinstance(val, np.ndarray) else val) for key, val in view.items()}


def test_one_workspace_through_the_sequence(world):
    sets, fresh = world["sets"], world["fresh"]
    for (a, _ma), (b, mb) in zip(SEQUENCE, SEQUENCE[1:]):
        if a != b:
            assert _differ(fresh[a], fresh[b]), (a, b)
    import torch
    st = kmlib.stream_create(0)
    bt = kmlib.Batch(world["db"], max_targets=MAX_TARGETS, max_total_bases=MAX_BASES)
    cur = None
    for i, (name, mode) in enumerate(SEQUENCE):
        tag = (i, name, mode)
        want = fresh[name]
        if mode == "reject":
            assert name == cur
            blob, offs = kmlib.pack_sequences(sets["light"])
            bad = offs.copy()
            bad[2], bad[3] = bad[3], bad[2]                    # one decreasing offset, the total within capacity
            with pytest.raises(kmlib.KmError):
                bt.set_targets_packed(blob, bad)
            over = sets["full"][:-1] + [sets["full"][-1] + "A"]  # one base over capacity
            with pytest.raises(kmlib.KmError):
                bt.set_targets(over)
            assert bt.n_targets == len(sets[cur])
            bt.run()
            got = bt.fetch()
            _check_fetch(got, want, tag)
            _rows_equal(got, name, world, tag)
            continue
        if mode == "inflight":
            bt.run(DELIVER, st)                               # never awaited: set_targets waits for it
        if mode == "dev":
            blob, offs = kmlib.pack_sequences(sets[name])
            d_blob = torch.from_numpy(np.concatenate([np.zeros(5, np.uint8), blob])).to("cuda")
            torch.cuda.synchronize()
            bt.set_targets_dev(d_blob.data_ptr(), offs + np.uint64(5), st)
            del d_blob
        else:
            bt.set_targets(sets[name])
        cur = name
        if mode in ("fetch", "inflight"):
            bt.run()
            got = bt.fetch()
            _check_fetch(got, want, tag)
        elif mode == "serial":
            bt.run(BOTH | kmlib.KM_RUN_SERIAL | kmlib.KM_RUN_TIMED, st)
            got = bt.fetch()
            assert all(x >= 0 for x in bt.timings())
            _check_fetch(got, want, tag)
        elif mode == "walk":
            bt.run(kmlib.KM_STAGE_WALK | kmlib.KM_RUN_DELIVER, st)
            _check_view(bt.result(), want, tag, walk_only=True)
            continue
        elif mode == "graph":
            for rep in range(2):
                bt.run(DELIVER | kmlib.KM_RUN_HIPGRAPH, st)
                got = _copy(bt.result())
                _check_view(got, want, tag + (rep,))
        else:
            flags = {"deliver": DELIVER, "dev": DELIVER, "lean": DELIVER | kmlib.KM_DELIVER_LEAN,
                     "c16": DELIVER | kmlib.KM_DELIVER_LEAN | kmlib.KM_DELIVER_COUNT16}[mode]
            bt.run(flags, st)
            got = _copy(bt.result())
            _check_view(got, want, tag, lean=bool(flags & kmlib.KM_DELIVER_LEAN))
            if mode == "c16" and name == "hot":
                assert "node_count16" not in got, tag       # > 2048 counts beyond 16 bits: the 32-bit form
            if mode == "c16" and name == "light":
                assert "node_count16" in got, tag
        _rows_equal(got, name, world, tag)
    bt.close()
    kmlib.stream_destroy(st)


def test_pump_across_set_changes(world):
    """Three batches in flight on three streams, new targets between two pumps (batch q takes set q+1)."""
    sets, fresh = world["sets"], world["fresh"]
    order = ["light", "heavy", "twin"]
    flags = DELIVER | kmlib.KM_DELIVER_LEAN
    batches = [kmlib.Batch(world["db"], max_targets=MAX_TARGETS, max_total_bases=MAX_BASES) for _ in order]
    streams = [kmlib.stream_create(0) for _ in order]
    for b, name in zip(batches, order):
        b.set_targets(sets[name])
    kmlib.pump(batches, streams, 7, flags)
    for b, name in zip(batches, order):
        _check_fetch(b.fetch(), fresh[name], ("pump 1", name))
    for q, b in enumerate(batches):
        b.set_targets(sets[order[(q + 1) % 3]])
    kmlib.pump(batches, streams, 5, flags)
    for q, b in enumerate(batches):
        name = order[(q + 1) % 3]
        got = b.fetch()
        _check_fetch(got, fresh[name], ("pump 2", name))
        _rows_equal(got, name, world, ("pump 2", name))
        b.close()
    for st in streams:
        kmlib.stream_destroy(st)


def test_finder_entry_points_reuse_one_workspace(world):
    """BatchFinder.rows and BatchFinder.write_rows over catalog chunks of different sizes on one finder: the workspace
    of the first (largest) chunk serves all of them, and every target prints what the reference prints."""
    sets = world["sets"]
    chunks = [[("heavy_%d" % i, s) for i, s in enumerate(sets["heavy"][:150])],
              [("light_%d" % i, s) for i, s in enumerate(sets["light"][:60])],
              [("long_%d" % i, s) for i, s in enumerate(sets["long"][:16])],
              [("tiny_0", sets["tiny"][0])],
              [("twin_%d" % i, s) for i, s in enumerate(sets["twin"][:40])]]
    db_cpu = ko.KmerDB(None, cutoff=0.05, n_cutoff=5,
                       records={"k": K, "canonical": True, "keys": world["keys"], "counts": world["counts"]})
    want = [[ko.target_rows(ko.analyse_target(seq, name, db_cpu), "mem.jf") for name, seq in c] for c in chunks]
    assert sum(len(r) > 1 for c in want for r in c) > 60
    jf = Jellyfish("mem.jf", cutoff=0.05, n_cutoff=5, db=world["db"])
    finder = BatchFinder(jf)
    ws = None
    for c, w in zip(chunks, want):
        assert finder.rows(c) == w
        ws = ws or finder._batch
        assert finder._batch is ws
    for c, w in zip(chunks, want):
        out = io.StringIO()
        finder.write_rows(c, out)
        assert out.getvalue() == "".join(r + "\n" for rows in w for r in rows)
        assert finder._batch is ws
    ws.close()


def test_cli_find_mutation_over_several_batches(tmp_path, monkeypatch):
    """`km find_mutation` over 150 targets in batches of 40 (one workspace, four target sets) prints what the reference
    prints: a clean catalog; one whose last batch has a repeated k-mer (no row at all, the reference's ValueError); and
    one where a single target of the third batch hits -n/--nodes (every row before it, then the reference's exit)."""
    import argparse

    from km_amd import cli
    case = synth.make_case(n_targets=149, length=200, n_keys=30_000, seed=9201, variant_frac=0.5,
                           variants_per_target=(1, 2), exact_pad=False)
    big = synth.make_case(n_targets=1, length=700, n_keys=2_000, seed=9202, variant_frac=1.0, exact_pad=False)
    keys, first = np.unique(np.concatenate([case["keys"], big["keys"]]), return_index=True)
    counts = np.concatenate([case["counts"], big["counts"]])[first]
    jf_path = str(tmp_path / "cat.jf")
    synth.write_jf(jf_path, keys, counts, K)
    seqs = _seqs(case)
    seqs.insert(85, _seqs(big)[0])                      # the third batch (targets 80-119) holds the long target
    files = []
    for t, s in enumerate(seqs):
        path = str(tmp_path / ("t%03d.fa" % t))
        with open(path, "w") as fh:
            fh.write(">t%03d\n%s\n" % (t, s))
        files.append(path)
    monkeypatch.setattr(cli, "CHUNK", 40)
    assert cli.CHUNK < len(files) <= cli.STREAM_ABOVE    # rows are held back until every batch has passed

    def run_cli(nodes):
        p = argparse.ArgumentParser()
        cli.add_find_mutation_args(p)
        out = io.StringIO()
        exc = None
        try:
            cli.main_find_mut(p.parse_args(["-n", str(nodes)] + files + [jf_path]), out=out, err=io.StringIO())
        except (SystemExit, Exception) as e:           # noqa: B902 — how the run ends is part of the check
            exc = e
        return out.getvalue().splitlines(), exc

    want, err = ko.run_find_mutation(files, jf_path, nodes=10000)
    assert err is None and len(want) > want.index(ko.HEADER) + 1 + len(files) + 30     # variant rows beside the references
    lines, exc = run_cli(10000)
    assert exc is None and lines[-1].startswith("#Elapsed time:")
    assert lines[:-1] == want
    # -n 600: only the 700 nt target (670 k-mers) exceeds it
    want_n, err_n = ko.run_find_mutation(files, jf_path, nodes=600)
    assert err_n == "ERROR: Node query count limit exceeded: max=600"
    lines, exc = run_cli(600)
    assert isinstance(exc, SystemExit) and str(exc.code) == err_n
    assert lines == want_n
    # a repeated k-mer in the last batch: the reference raises before its first row
    s = seqs[140]
    with open(files[140], "w") as fh:
        fh.write(">t140\n%s\n" % (s[:120] + s[40:80] + s[120:]))
    with pytest.raises(ValueError) as ref_exc:
        ko.run_find_mutation(files, jf_path)
    lines, exc = run_cli(10000)
    assert isinstance(exc, ValueError) and str(exc) == str(ref_exc.value)
    assert lines == want[:want.index(ko.HEADER) + 1]
