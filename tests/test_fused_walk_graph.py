"""k_dfs and k_graph_pure in one launch (graph_kernel.h: k_dfs_pure).  The default walk + graph run launches the walk of
the flagged targets and the pure-chain pass over the unflagged ones as one kernel; KM_RUN_SERIAL launches them one
after the other, as every run did before.  The pure-chain blocks run while k_dfs stores statuses and its epilogue
stores per-target results, so they may touch nothing of a flagged target, and every word a flagged target delivers
must be written by k_dfs or k_graph in every step — a reused workspace holds the last step's.

Every case runs the same batch both ways in one process and compares every array of fetch() and every field of
sizes(); the results are checked against a workspace that has seen nothing else and against the plain-C oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from km_amd import kmer as km
from km_amd import lib as kmlib
from km_amd import synth
from oracle import c_oracle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOTH = kmlib.KM_STAGE_WALK | kmlib.KM_STAGE_GRAPH
SERIAL = BOTH | kmlib.KM_RUN_SERIAL
_SIZE_FIELDS = ("n_targets", "n_paths", "n_nodes", "n_runs", "logical_probes", "table_fetches", "n_big_tier",
                "n_flagged", "seed_probes", "n_extra", "n_count_escapes")


def _merge(tables):
    """One table over several (keys, counts): the first one that has a key gives its count."""
    keys, first = np.unique(np.concatenate([t[0] for t in tables]), return_index=True)
    return keys, np.concatenate([t[1] for t in tables])[first]


def _seqs(case):
    return [km.decode(r) for r in case["targets"]]


def _take(b, flags=BOTH, stream=None):
    """Every array of fetch(), every field of sizes(), and the one per-target word the copying API does not show:
    the delivery's ref_max_cov (t_refmax), from a delivered run of the same kind."""
    b.run(flags, stream)
    r = b.fetch()
    s = b.sizes()
    r["_sizes"] = {f: int(getattr(s, f)) for f in _SIZE_FIELDS}
    b.run(flags | kmlib.KM_RUN_DELIVER, stream)
    r["ref_max_cov"] = np.array(b.result()["ref_max_cov"])
    return r


def _same(got, want, ctx):
    assert sorted(got) == sorted(want), ctx
    for key in want:
        if key == "_sizes":
            assert got[key] == want[key], (ctx, key, got[key], want[key])
        else:
            assert np.array_equal(got[key], want[key]), (ctx, key)


def _both_ways(b, ctx, stream=None):
    """The batch's current targets: the fused run, then the serial run; the fused result."""
    fused = _take(b, BOTH, stream)
    counts = b.debug_counts()
    serial = _take(b, SERIAL, stream)
    _same(fused, serial, (ctx, "fused vs serial"))
    assert b.debug_counts() == counts, ctx
    fused["_counts"] = counts
    return fused


def _against_oracle(r, co, seqs, which, ctx, **prm):
    noff, poff = r["node_off"].astype(np.int64), r["path_off"].astype(np.int64)
    for t in which:
        if set(seqs[t]) - set("ACGTacgt"):
            assert int(r["status"][t]) == kmlib.T_BAD_BASE and poff[t + 1] == poff[t], (ctx, t)
            continue
        want = co.analyse(km.encode(seqs[t]), **prm)
        assert int(r["status"][t]) == want["status"], (ctx, t)
        if want["status"] != kmlib.T_OK:
            assert poff[t + 1] == poff[t], (ctx, t)
            continue
        assert np.array_equal(r["node_kmer"][noff[t]:noff[t + 1]], want["kmers"]), (ctx, t)
        assert np.array_equal(r["node_count"][noff[t]:noff[t + 1]], want["counts"]), (ctx, t)
        assert int(r["probes"][t]) == want["probes"], (ctx, t)
        assert [kmlib.expand_path(r, p).tolist() for p in range(poff[t], poff[t + 1])] == want["paths"], (ctx, t)
        assert r["path_min_cov"][poff[t]:poff[t + 1]].tolist() == want["min_cov"], (ctx, t)
        bare = int(r["ref_max_cov"][t]) != 0xFFFFFFFF                 # one path, the maximum of the target's own counts
        assert not bare or (len(want["paths"]) == 1 and int(r["ref_max_cov"][t]) == int(want["counts"].max())), (ctx, t)


def _batch(db, seqs, **prm):
    b = kmlib.Batch(db, max_targets=max(1, len(seqs)), max_total_bases=max(64, sum(len(s) for s in seqs)), **prm)
    b.set_targets(seqs)
    return b


# ------------------------------------------------------------------ the mixed batch, the edges of the grid split
@pytest.mark.parametrize("k", [31, 21])
def test_mixed_batch(k):
    """300 targets of 300 nt, 40 % with a variant: k = 31 (its own instantiation) and k = 21 (the generic one)."""
    case = synth.make_case(n_targets=300, length=300, k=k, n_keys=55_000, seed=6100 + k, variant_frac=0.4,
                           exact_pad=False)
    db = kmlib.Database.from_records(case["keys"], case["counts"], k).upload(0)
    seqs = _seqs(case)
    b = _batch(db, seqs)
    r = _both_ways(b, ("mixed", k))
    flagged, _handed, _left = r["_counts"]
    assert 60 <= flagged <= 180 and r["_sizes"]["n_flagged"] == flagged
    _against_oracle(r, c_oracle.COracle(case["keys"], case["counts"], k), seqs, range(0, 300, 4), ("mixed", k))
    b.close()
    db.close()


def test_batch_whose_pure_chain_pass_needs_more_lds_than_the_walk():
    """A longest target of 512 k-mers: the pure-chain pass's table (the power of two >= 4 (n_ref + 2)) is then twice the
    walk's position table and its LDS the larger of the two — the one geometry at which a walk + graph run keeps
    two launches (batch_host.h: fuses_pure).  511 k-mers beside it, and 510, which is one launch again."""
    k = 31
    for length in (512 + k - 1, 511 + k - 1, 510 + k - 1):
        case = synth.make_case(n_targets=60, length=length, k=k, n_keys=40_000, seed=6150 + length, variant_frac=0.5,
                               exact_pad=False)
        db = kmlib.Database.from_records(case["keys"], case["counts"], k).upload(0)
        seqs = _seqs(case)
        b = _batch(db, seqs)
        r = _both_ways(b, ("lds", length))
        assert 15 <= r["_counts"][0] <= 45
        _against_oracle(r, c_oracle.COracle(case["keys"], case["counts"], k), seqs, range(0, 60, 3), ("lds", length))
        b.close()
        db.close()


@pytest.mark.parametrize("variant_frac,n_targets", [(0.0, 300), (1.0, 300), (0.0, 1), (1.0, 1)])
def test_edges_of_the_grid_split(variant_frac, n_targets):
    """No flagged target at all (every k_dfs block leaves at once), every target flagged (every pure-chain block
    does), and a batch of one target, flagged or not."""
    case = synth.make_case(n_targets=n_targets, length=300, k=31, n_keys=50_000, seed=6200 + n_targets,
                           variant_frac=variant_frac, vaf=(0.3, 0.6), exact_pad=False)
    db = kmlib.Database.from_records(case["keys"], case["counts"], 31).upload(0)
    seqs = _seqs(case)
    b = _batch(db, seqs)
    r = _both_ways(b, ("edge", variant_frac, n_targets))
    flagged = r["_counts"][0]
    if variant_frac == 0.0:
        assert flagged == 0
    else:
        assert flagged > 0.95 * n_targets
    co = c_oracle.COracle(case["keys"], case["counts"], 31)
    _against_oracle(r, co, seqs, range(0, n_targets, 5), ("edge", variant_frac, n_targets))
    again = _both_ways(b, ("edge again", variant_frac, n_targets))      # (the grid now follows the flagged count)
    _same(again, r, ("edge again", variant_frac, n_targets))
    b.close()
    db.close()


# ------------------------------------------------------------------ k_graph's list filled from both roles
def _shared_prefix_target(rng, k, length=200):
    """No k-mer twice, one (k-1)-mer twice (followed by different bases): not a pure chain."""
    while True:
        s = synth.random_seq(rng, length)
        p = s[20:20 + k - 1]
        a = "ACGT"[("ACGT".index(s[20 + k - 1]) + 1) % 4]
        t = s[:120] + p + a + s[120 + k:]
        if len(t) == length and not synth.has_repeated_kmer(t, k):
            return t


_LIST_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from km_amd import lib as kmlib
d = np.load(%(inp)r)
db = kmlib.Database.from_records(d["keys"], d["counts"], 31).upload(0)
seqs = [str(x) for x in d["seqs"]]
b = kmlib.Batch(db, max_targets=len(seqs), max_total_bases=sum(len(s_) for s_ in seqs))
b.set_targets(seqs)
both = kmlib.KM_STAGE_WALK | kmlib.KM_STAGE_GRAPH
def take(flags):
    b.run(flags)
    r = b.fetch()
    b.run(flags | kmlib.KM_RUN_DELIVER)
    r["ref_max_cov"] = np.array(b.result()["ref_max_cov"])
    return r
r = take(both)                                   # k_dfs and k_graph_pure in one launch
counts = np.array(b.debug_counts())
serial = take(both | kmlib.KM_RUN_SERIAL)        # ... and one after the other, in this process as well
assert sorted(r) == sorted(serial)
for key_ in r:
    assert np.array_equal(r[key_], serial[key_]), key_
assert np.array_equal(np.array(b.debug_counts()), counts)
np.savez(%(out)r, counts=counts, **{k_: v for k_, v in r.items() if isinstance(v, np.ndarray)})
"""


def test_unflagged_targets_that_are_not_pure_beside_flagged_ones_left_to_k_graph(tmp_path):
    """k_graph's work list filled from both roles of the one launch: unflagged targets the pure-chain pass hands over
    (a repeated (k-1)-mer; low-complexity targets with a repeated k-mer, which k_graph reports) and flagged targets
    the epilogue of k_dfs leaves (walks that circle a repeat, dead-end branches) among ordinary ones.  Then the same
    batch with the epilogue off (KM_EPILOGUE is read once per process: a child process, which runs it both ways too)."""
    k = 31
    keys, counts, seqs, special = _list_case()
    db = kmlib.Database.from_records(keys, counts, k).upload(0)
    b = _batch(db, seqs)
    r = _both_ways(b, "list")
    flagged, handed, left = r["_counts"]
    assert flagged >= 40 and handed >= 12 and left >= 6, r["_counts"]
    co = c_oracle.COracle(keys, counts, k)
    _against_oracle(r, co, seqs, sorted(set(special) | set(range(0, len(seqs), 3))), "list")
    assert sum(int(r["status"][t]) == kmlib.T_REPEAT_KMER for t in special) == 4
    b.close()
    db.close()
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "epi_off.npz")
    np.savez(inp, keys=keys, counts=counts, seqs=np.array(seqs))
    subprocess.check_call([sys.executable, "-c", _LIST_CHILD % {"root": os.path.dirname(HERE), "inp": inp, "out": out}],
                          env=dict(os.environ, KM_EPILOGUE="0"))
    off = np.load(out)
    assert off["counts"].tolist() == [flagged, handed, 0]               # (nothing left by an epilogue: there was none)
    for key, val in r.items():
        if isinstance(val, np.ndarray):
            assert np.array_equal(val, off[key]), key


def _list_case():
    k = 31
    rng = np.random.default_rng(6300)
    case = synth.make_case(n_targets=120, length=300, k=k, n_keys=40_000, seed=6301, variant_frac=0.5,
                           branch_noise_frac=0.03, exact_pad=False)
    reps = [synth.repeat_case(k, u) for u in synth.REPEAT_UNITS]
    tables = [(case["keys"], case["counts"])] + [synth.records_from_reads(c["reads"], k) for c in reps]
    keys, counts = _merge(tables)
    shared = [_shared_prefix_target(rng, k) for _ in range(12)]       # (their k-mers are not in the table: unflagged)
    low = ["A" * 60, "AT" * 40, "ACACACAC" * 9, "T" * 45]
    seqs = []
    for i, s in enumerate(_seqs(case)):
        seqs.append(s)
        if i % 10 == 0:
            seqs.append(shared[i // 10])
        if i % 20 == 5:
            seqs.append(reps[(i // 20) % len(reps)]["target"])
        if i % 30 == 7:
            seqs.append(low[i // 30])
    special = [t for t, s in enumerate(seqs) if s in shared or s in low or any(s == c["target"] for c in reps)]
    assert len(special) == 12 + 6 + 4
    return keys, counts, seqs, special


# ------------------------------------------------------------------ stale words on a reused workspace
def _insertion_reads(rng, k, length, ins_len, later_snv):
    """A target and reads with one insertion of ins_len bases (ins_len + k - 1 new nodes) and, on request, a
    substitution further on (one more flagged seed behind the insertion)."""
    while True:
        T = synth.unique_kmer_seq(rng, length, k)
        var = T[:80] + synth.random_seq(rng, ins_len) + T[80:]
        reads = [(T, 60), (var, 30)]
        if later_snv:
            p = length - 60
            reads.append((T[:p] + "ACGT"[("ACGT".index(T[p]) + 1) % 4] + T[p + 1:], 25))
        if not any(synth.has_repeated_kmer(s, k) for s, _c in reads):
            return T, reads


def test_reused_workspace_delivers_no_stale_word():
    """One workspace, three target sets in a row: flagged targets become unflagged and the reverse, and targets that
    k_dfs leaves with a status or to the large tier — a bad base, the node limit, more than 160 new nodes — take the
    place of answered ones and give it back.  Every step equals what a fresh workspace gives for that set."""
    k, n, max_node = 31, STALE_N, STALE_MAX_NODE
    keys, counts, sets = _stale_sets()
    db = kmlib.Database.from_records(keys, counts, k).upload(0)
    co = c_oracle.COracle(keys, counts, k)
    fresh = []
    for q, seqs in enumerate(sets):
        f = _batch(db, seqs, max_node=max_node)
        fresh.append(_both_ways(f, ("fresh", q)))
        f.close()
        _against_oracle(fresh[q], co, seqs, range(n), ("fresh", q), max_node=max_node)
        st = fresh[q]["status"]
        first = 10 + 30 * q
        assert int((st == kmlib.T_BAD_BASE).sum()) == 4 and int((st == kmlib.T_NODE_LIMIT).sum()) == 4
        assert fresh[q]["_sizes"]["n_big_tier"] >= 4                      # the 170-base insertions
        for j in range(4):
            assert int(st[first + 6 * j + j % 2]) == kmlib.T_NODE_LIMIT
            t = first + 6 * j + 2 + j % 2
            assert int(st[t]) == kmlib.T_OK and int(fresh[q]["node_off"][t + 1] - fresh[q]["node_off"][t]) > 270 + 160
    b = kmlib.Batch(db, max_node=max_node, max_targets=n, max_total_bases=max(sum(len(s) for s in seqs) for seqs in sets))
    for q in (0, 1, 2, 1, 0):
        b.set_targets(sets[q])
        got = _both_ways(b, ("reused", q))
        _same(got, fresh[q], ("reused vs fresh", q))
    b.close()
    db.close()


STALE_N, STALE_MAX_NODE = 120, 500


def _stale_sets():
    k, n = 31, STALE_N
    rng = np.random.default_rng(6400)
    var = synth.make_case(n_targets=n, length=300, k=k, n_keys=30_000, seed=6401, variant_frac=1.0,
                          variants_per_target=(1, 2), vaf=(0.3, 0.6), kinds=("snv", "del", "dup"), exact_pad=False)
    plain = synth.make_case(n_targets=n, length=300, k=k, n_keys=30_000, seed=6402, variant_frac=0.0, exact_pad=False)
    limit = [_insertion_reads(rng, k, 400, 110, True) for _ in range(4)]    # 370 + 140 nodes > max_node, then a seed
    large = [_insertion_reads(rng, k, 300, 170, False) for _ in range(4)]   # 200 new nodes: beyond the LDS tier
    keys, counts = _merge([(var["keys"], var["counts"]), (plain["keys"], plain["counts"])] +
                          [synth.records_from_reads(reads, k) for _T, reads in limit + large])
    flg, unf = _seqs(var), _seqs(plain)
    bad = [s[:100] + "N" + s[101:] for s in flg[:4]]

    def pattern(parity, specials_at):
        seqs = [flg[p] if p % 2 == parity else unf[p] for p in range(n)]
        for j in range(4):                                            # two of each kind where the other sets have a
            seqs[specials_at + 6 * j + j % 2] = limit[j][0]           # flagged target, two where they have an unflagged one
            seqs[specials_at + 6 * j + 2 + j % 2] = large[j][0]
            seqs[specials_at + 6 * j + 4 + j % 2] = bad[j]
        return seqs
    return keys, counts, [pattern(0, 10), pattern(1, 40), pattern(0, 70)]


# ------------------------------------------------------------------ more flagged targets than k_dfs blocks
def test_more_flagged_targets_than_dfs_blocks():
    """The grid of the k_dfs role follows the flagged count of the batch's last delivery; a set with many more flagged
    targets overflows it and block 0 hands the rest to the large tier — keyed on the number of k_dfs blocks, not on
    the launch's grid, which also holds the pure-chain blocks."""
    few = synth.make_case(n_targets=300, length=300, k=31, n_keys=40_000, seed=6501, variant_frac=0.04, exact_pad=False)
    many = synth.make_case(n_targets=300, length=300, k=31, n_keys=40_000, seed=6502, variant_frac=0.9,
                           variants_per_target=(1, 2), exact_pad=False)
    keys, counts = _merge([(few["keys"], few["counts"]), (many["keys"], many["counts"])])
    db = kmlib.Database.from_records(keys, counts, 31).upload(0)
    seq_few, seq_many = _seqs(few), _seqs(many)
    f = _batch(db, seq_many)
    want = _take(f)
    f.close()
    b = _batch(db, seq_few)
    _both_ways(b, "few")
    assert 2 <= b.debug_counts()[0] <= 40
    b.set_targets(seq_many)
    got = _take(b)                                   # ~80 k_dfs blocks for ~260 flagged targets
    assert b.debug_counts()[0] > 230 and got["_sizes"]["n_big_tier"] > 120
    serial = _take(b, SERIAL)                        # (this run's grid holds them all)
    again = _take(b)
    assert again["_sizes"]["n_big_tier"] == want["_sizes"]["n_big_tier"] < 20
    for r, tag in ((serial, "serial"), (again, "again")):
        _same(r, want, tag)
    got["_sizes"]["n_big_tier"] = want["_sizes"]["n_big_tier"]     # (the one figure that says which tier walked them)
    got["n_big_tier"] = want["n_big_tier"]
    _same(got, want, "overflow")
    _against_oracle(got, c_oracle.COracle(keys, counts, 31), seq_many, range(0, 300, 7), "overflow")
    b.close()
    db.close()


# ------------------------------------------------------------------ three batches in flight
def test_pump_three_batches_in_flight():
    """Three batches on three pool streams, 12 steps round robin: the fused launches of different batches overlap on
    the device; every batch ends with the results of a plain run."""
    cases = [synth.make_case(n_targets=200, length=260, k=31, n_keys=20_000, seed=6600 + i, variant_frac=0.3 + 0.2 * i,
                             exact_pad=False) for i in range(3)]
    keys, counts = _merge([(c["keys"], c["counts"]) for c in cases])
    db = kmlib.Database.from_records(keys, counts, 31).upload(0)
    batches, streams, want = [], [], []
    for c in cases:
        b = _batch(db, _seqs(c))
        want.append(_both_ways(b, "plain"))
        batches.append(b)
        streams.append(kmlib.stream_create(0))
    kmlib.pump(batches, streams, 12, BOTH | kmlib.KM_RUN_DELIVER)
    for b, w in zip(batches, want):
        assert np.array_equal(np.array(b.result()["ref_max_cov"]), w["ref_max_cov"])
        got = b.fetch()
        for key, val in got.items():
            assert np.array_equal(val, w[key]), key
        b.close()
    for st in streams:
        kmlib.stream_destroy(st)
    db.close()
