"""The graph stage where a bubble and the reference route it bypasses cost the same.

A deletion bubble of c edges (weight 1) bypasses b - a reference edges (weight 0.01f, added hop by hop in float32).
Around b - a = 100 c three pieces of code hand over to each other: the epilogue of k_dfs and step 2c of k_graph answer
the bubble in closed form while b - a + 10 <= 100 c, the frontier Dijkstra of k_graph (the only code of the large
tier) takes everything past that margin — and the shortest-path trees themselves flip a little further on, where the
float32 sums say so.  The cases here sit on both sides of each of those places and on the tie, by construction
(km_amd/synth.py: DistinctPool, crossover_case, tie_case): every (k-1)-mer is distinct on both strands, so the oracle
accepts every target and every bubble is exactly the one asked for — the CPU tests assert both, nothing is skipped.

Tiers: the LDS tier holds targets of up to 1 416 k-mers (test_margin_* asks tests/host/lds_tier_limit.hip), so a
crossover at c = k fits it for k <= 13 only.  The k = 11 sweep (1 278 k-mers a target) and the k = 13 one (1 398, cut
as short as its longest deletion allows) run there; the k = 15 sweep (1 706) and the k = 21 one (2 348) outgrow it by
their length and the k = 11 sweep with a 170-base insertion added to every target by its node count.

What a changed kernel would trip over: the margin + 10 -> + 0 in the epilogue of k_dfs gives the tie case of a sweep
the reference's trees (default and replayed runs); in 2c / 2c' of k_graph it gives the deletion-only cases of margin 0
and -1 the wrong graph log (KM_EPILOGUE=0 run); the guard `d == tref[cur]` of k_graph's chain loop taken away, in
either pass, flips prev[] / after[] where the nested case's outer bubble rejoins / leaves the reference
(test_nested_case_* shows on the CPU that it must).
"""
import functools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from km_amd import kmer as km
from km_amd import lib as kmlib
from km_amd import synth
from oracle import km_oracle as ko

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MARGINS = (12, 11, 10, 9, 8, 3, 1, 0, -1, -2, -5)          # 100 c - (b - a): both sides of the + 10 margin, the tie, both sides of the flip
MARGINS_K21 = (10, 1, 0, -1, -5)
LENGTH_K13 = 1410                                          # 4 k + the longest deletion (99 k + 5) + 4 k and a few bases
MARGINS_SOLO = (10, 9, 0, -1)                              # k = 11, the deletion alone in its target: step 2c of k_graph
FIELDS = ("status", "n_ref", "probes", "node_off", "node_kmer", "node_count", "path_off", "run_off", "run_start",
          "run_len", "path_len", "path_min_cov")
assert synth.CROSSOVER_MARGINS == MARGINS


# ------------------------------------------------------------------ cases and their oracle results, computed once
def _cpu_db(keys, counts, k):
    return ko.KmerDB(None, cutoff=0.05, n_cutoff=5, records={"k": k, "canonical": True, "keys": keys, "counts": counts})


@functools.lru_cache(maxsize=None)
def _cases(kind, k):
    """(cases, keys, counts) of one batch: every case from one pool, one table for all of them."""
    if kind == "sweep":
        cases = synth.crossover_sweep(k, MARGINS_K21 if k == 21 else MARGINS, solo=MARGINS_SOLO if k == 11 else (),
                                      nested=k in (11, 15), length=LENGTH_K13 if k == 13 else None)
    elif kind == "sweep_ins":                                    # + 170 inserted bases: 180 more walk nodes than the LDS tier keeps
        cases = synth.crossover_sweep(k, MARGINS, extra_ins=170, seed=1)
    else:
        pool = synth.DistinctPool(k, 31 * k + 5)
        cases = [synth.tie_case(pool, "ins3_%d" % k, "ins3"), synth.tie_case(pool, "snv2_%d" % k, "snv2")]
    keys, counts = synth.records_from_reads([r for c in cases for r in c["reads"]], k)
    return cases, keys, counts


@functools.lru_cache(maxsize=None)
def _python_wants(kind, k):
    cases, keys, counts = _cases(kind, k)
    cpu = _cpu_db(keys, counts, k)
    return [ko.analyse_target(c["target"], c["name"], cpu) for c in cases]      # (raises on a repeated k-mer: no skip)


@functools.lru_cache(maxsize=None)
def _c_wants(kind, k):
    from oracle import c_oracle
    cases, keys, counts = _cases(kind, k)
    co = c_oracle.COracle(keys, counts, k)
    out = []
    for c in cases:
        w = co.analyse(km.encode(c["target"]))
        assert w["status"] == 0, c["name"]
        w["kmers"] = [km.unpack(int(x), k) for x in w["kmers"]]
        w["counts"] = w["counts"].tolist()
        out.append(w)
    return out


def _bubble(kmers, n_ref, chain):
    """(a, b, c, nodes) of the bubble whose new k-mers are `chain`, read off a node list: a / b are the reference
    nodes the chain hangs off / rejoins, c its number of edges."""
    index = {m: i for i, m in enumerate(kmers)}
    assert len(index) == len(kmers)
    nodes = [index[m] for m in chain]
    assert all(i >= n_ref for i in nodes)
    assert all(x[1:] == y[:-1] for x, y in zip(chain, chain[1:]))
    a = [i for i in range(n_ref) if kmers[i][1:] == chain[0][:-1]]
    b = [i for i in range(n_ref) if kmers[i][:-1] == chain[-1][1:]]
    assert len(a) == 1 and len(b) == 1
    return a[0], b[0], len(nodes) + 1, nodes


def _assert_bubbles_as_asked(case, kmers, n_ref):
    """The walk found the haplotypes' new k-mers and nothing else; the deletion bubble has k - 1 nodes, c = k edges."""
    k = case["k"]
    asked = [m for chain in case["expect"].values() for m in chain]
    assert len(set(asked)) == len(asked)
    assert sorted(kmers[n_ref:]) == sorted(asked), case["name"]
    if "del" in case["expect"]:
        a, b, c, nodes = _bubble(kmers, n_ref, case["expect"]["del"])
        assert len(nodes) == k - 1 and c == k and a < b, case["name"]
        lo, hi = a, b
        if case["kind"] == "nested":
            lo, hi, c2, _ = _bubble(kmers, n_ref, case["expect"]["outer"])
            assert (b - a, c2, a - lo, hi - b) == (100 * k + 5, k + 1, 48, 49), case["name"]
        for tag in ("up", "in", "down"):
            if tag in case["expect"]:
                sa, sb, sc, _ = _bubble(kmers, n_ref, case["expect"][tag])
                assert sb - sa == k + 1 and sc == k + 1
                assert (sb <= lo) if tag == "up" else (a < sa and sb < b) if tag == "in" else (sa >= hi)


def _margin_and_outcome(case, want):
    """(100 c - (b - a), does the path through the downstream SNV run through the deletion bubble)."""
    a, b, c, nodes = _bubble(want["kmers"], want["n_ref"], case["expect"]["del"])
    down = _bubble(want["kmers"], want["n_ref"], case["expect"]["down"])[3]
    through = [p for p in want["paths"] if down[0] in p]
    assert len(through) == 1, case["name"]
    return 100 * c - (b - a), nodes[0] in through[0]


def _assert_coverage(cases, wants, margins):
    """Every margin of the set is hit, in order, and both outcomes occur: what the closed forms may answer stays on
    the reference, the far side runs through the bubble (where between 9 and -2 it flips is the float32 sums' say)."""
    seen = [_margin_and_outcome(c, w) for c, w in zip(cases, wants) if c["kind"] == "sweep"]
    solo = [(c, w) for c, w in zip(cases, wants) if c["kind"] == "solo"]         # the deletion-only cases behind them
    assert len(solo) in (0, len(MARGINS_SOLO))
    for (c, w), v in zip(solo, MARGINS_SOLO):
        a, b, n_edges, _ = _bubble(w["kmers"], w["n_ref"], c["expect"]["del"])
        assert 100 * n_edges - (b - a) == v and len(w["paths"]) == 2
    for c, w in zip(cases, wants):
        if c["kind"] == "nested":                               # the downstream SNV's path takes the inner bubble
            assert _margin_and_outcome(c, w) == (-5, True)
            outer = _bubble(w["kmers"], w["n_ref"], c["expect"]["outer"])[3]
            assert sum(outer[0] in p for p in w["paths"]) == 1
    assert [v for v, _ in seen] == list(margins)
    assert {o for _, o in seen} == {False, True}, seen
    assert not any(o for v, o in seen if v >= 10), seen        # (what the closed forms may answer is on the reference)
    assert all(o for v, o in seen if v <= -5), seen
    return seen


# ------------------------------------------------------------------ CPU: the generator
def _k1mers(seq, k):
    return [seq[i:i + k - 1] for i in range(len(seq) - k + 2)]


@pytest.mark.parametrize("k", [11, 12, 15, 21, 31])
def test_pool_keeps_every_k1mer_distinct_on_both_strands_and_off_its_own_reverse(k):
    pool = synth.DistinctPool(k, 5)
    seqs = [pool.grow(n) for n in (k - 1, k, 400, 37, 1500)]
    assert [len(s) for s in seqs] == [k - 1, k, 400, 37, 1500]
    mers = [m for s in seqs for m in _k1mers(s, k)]
    both = set(mers) | {synth.revcomp_str(m) for m in mers}
    assert len(both) == 2 * len(mers)                          # no repeat, no reverse-complement pair, no palindrome
    again = synth.DistinctPool(k, 5)
    assert [again.grow(n) for n in (k - 1, k, 400, 37, 1500)] == seqs          # deterministic
    # a haplotype that repeats a (k-1)-mer of another sequence is refused and changes nothing
    own = set(_k1mers(seqs[2], k))
    before = set(pool.seen)
    assert not pool.admit(own, seqs[2][:50] + seqs[4][100:160])
    assert pool.seen == before and own == set(_k1mers(seqs[2], k))
    if (k - 1) % 2 == 0:                                       # a (k-1)-mer that is its own reverse complement
        half = pool.grow(k - 1)[:(k - 1) // 2]
        assert not pool.admit(set(), half + synth.revcomp_str(half))


@pytest.mark.parametrize("kind,k", [("sweep", 11), ("sweep", 13), ("sweep", 15), ("sweep", 21), ("sweep_ins", 11), ("ties", 21), ("ties", 31)])
def test_oracle_accepts_every_target_and_every_bubble_is_the_one_asked_for(kind, k):
    cases, keys, counts = _cases(kind, k)
    cpu = _cpu_db(keys, counts, k)
    all_mers = []
    for c in cases:
        mers = ko.ref_kmers(c["target"], c["name"], k)                          # raises on a repeated k-mer
        nodes = ko.walk(mers, cpu)
        _assert_bubbles_as_asked(c, list(nodes.keys()), len(mers))
        all_mers += [m for seq, _ in c["reads"] for m in _k1mers(seq, k)]
    # the cases of a batch share a table: no (k-1)-mer of one occurs in another, on either strand
    fw = set(all_mers)
    assert not any(synth.revcomp_str(m) in fw for m in fw)
    for i, c in enumerate(cases):
        mine = {m for seq, _ in c["reads"] for m in _k1mers(seq, k)}
        for d in cases[i + 1:]:
            assert not mine & {m for seq, _ in d["reads"] for m in _k1mers(seq, k)}


@pytest.mark.parametrize("kind,k", [("sweep", 11), ("sweep", 13), ("sweep", 15), ("sweep", 21), ("sweep_ins", 11)])
def test_sweep_hits_every_margin_and_both_outcomes(kind, k):
    """On the C oracle's node lists and paths (the GPU tests assert the same on what they compare with)."""
    cases = _cases(kind, k)[0]
    seen = _assert_coverage(cases, _c_wants(kind, k), MARGINS_K21 if k == 21 else MARGINS)
    print(kind, k, seen)


def _same_as_python(want_c, want_py):
    return (want_c["kmers"] == want_py["kmers"] and want_c["counts"] == want_py["counts"] and
            want_c["probes"] == want_py["probes"] and want_c["paths"] == [list(p) for p in want_py["paths"]] and
            list(want_c["min_cov"]) == want_py["min_cov"])


@functools.lru_cache(maxsize=None)
def _k21_tie_python():
    cases, keys, counts = _cases("sweep", 21)
    i = MARGINS_K21.index(0)
    return i, ko.analyse_target(cases[i]["target"], cases[i]["name"], _cpu_db(keys, counts, 21))


def test_python_and_c_oracles_agree_on_the_k21_tie():
    i, want = _k21_tie_python()
    assert _same_as_python(_c_wants("sweep", 21)[i], want)


# ------------------------------------------------------------------ CPU: exact ties inside the walk's own nodes
def _dist_from_prev(w, prev, root):
    """dist[] of the oracle's Dijkstra, from its predecessor array: dist[j] was last written as w[i, j] + dist[i] with
    i = prev[j] final — the same float32 additions, hop by hop."""
    n = w.shape[0]
    dist = np.full(n, np.inf, dtype=np.float32)
    dist[root] = 0
    for j in range(n):
        chain = []
        while j != root and not np.isfinite(dist[j]) and prev[j] != -1:
            chain.append(j)
            j = int(prev[j])
        for x in reversed(chain):
            dist[x] = np.float32(w[prev[x], x]) + dist[prev[x]]
    return dist


def _tied_nodes(w, dist):
    """Nodes with two or more in-neighbours attaining the minimal fl(dist + w)."""
    out = []
    for j in range(w.shape[0]):
        ins = np.flatnonzero(np.isfinite(w[:, j]) & np.isfinite(dist))
        if ins.size >= 2:
            vals = (w[ins, j] + dist[ins]).astype(np.float32)
            if int((vals == vals.min()).sum()) >= 2:
                out.append((j, int((vals == vals.min()).sum())))
    return out


@pytest.mark.parametrize("k", [21, 31])
def test_tie_cases_really_tie(k):
    """The three-way split inside the insertion rejoins at a node with three in-neighbours at exactly equal float32
    distance (forward tree), and leaves from one with three successors at equal distance to the sink (backward)."""
    cases = _cases("ties", k)[0]
    wants = _python_wants("ties", k)
    want = wants[0]
    names = want["kmers"] + [ko.SOURCE, ko.SINK]
    n = len(names)
    w, _ = ko.build_graph(names, list(range(want["n_ref"])), 0, want["n_ref"] - 1)
    fwd = _dist_from_prev(w, ko.dijkstra_prev(w, n - 2), n - 2)
    bwd = _dist_from_prev(w.transpose(), ko.dijkstra_prev(w.transpose(), n - 1), n - 1)
    assert np.isfinite(fwd[:n - 2]).all() and np.isfinite(bwd[:n - 2]).all()
    tf, tb = _tied_nodes(w, fwd), _tied_nodes(w.transpose(), bwd)
    assert (3 in [c for _, c in tf]) and (3 in [c for _, c in tb]), (tf, tb)
    assert all(j >= want["n_ref"] for j, _ in tf + tb)                         # inside the walk's own nodes
    # insertion alone, its two substituted forms, the reference
    assert len(want["paths"]) == 4 and len(wants[1]["paths"]) == 3


# ------------------------------------------------------------------ CPU: the margin as arithmetic
@functools.lru_cache(maxsize=None)
def _host_program(name):
    """tests/host/<name>.hip, compiled once per session (host code only; hipcc is what builds the library).
    tests/test_lds_tier_edges.py uses it too."""
    import atexit
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    tmp = tempfile.mkdtemp(prefix="km_%s_" % name)
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, name)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", exe,
                           os.path.join(ROOT, "tests", "host", name + ".hip")])
    return exe


def _lds_tier_program():
    return _host_program("lds_tier_limit")


@functools.lru_cache(maxsize=None)
def _lds_tier_limit(k, max_break=10):
    largest, settled = map(int, subprocess.run([_lds_tier_program(), str(k), str(max_break)], capture_output=True,
                                               text=True, check=True, timeout=60).stdout.split())
    assert largest == settled                                   # (fitting is monotone: the bisection finds the largest)
    return largest


def _margins_in_the_kernels():
    """The margin as the three closed-form tests of the kernels spell it (one in the epilogue of k_dfs, 2c and 2c' of
    k_graph)."""
    import re
    with open(os.path.join(ROOT, "km_amd", "csrc", "walk_kernel.h")) as fh:
        epi = re.findall(r"\(b_node - a_here\) \+ (\d+) > 100ull \* \(e - s_node \+ 2\)", fh.read())
    with open(os.path.join(ROOT, "km_amd", "csrc", "graph_kernel.h")) as fh:
        twoc = re.findall(r"\(fb - fa\) \+ (\d+) <= 100ull \* \(m - n_ref \+ 1\)", fh.read())
    assert len(epi) == 1 and len(twoc) == 2, (epi, twoc)
    return [int(x) for x in epi + twoc]


def _tref(n):
    """tref[j] as batch_host.h accumulates it: acc += 0.01f from 0, (j + 1) terms."""
    t = np.cumsum(np.full(n, 0.01, dtype=np.float32), dtype=np.float32)
    acc = np.float32(0)
    for j in range(min(n, 3000)):                               # (cumsum adds one after the other, as the loop does)
        acc = np.float32(acc + np.float32(0.01))
        assert t[j] == acc
    return t


def _margin_violations(n_max, margin, max_stack=500):
    """Triples (n_ref, a, c) at which the reference route a -> b is NOT strictly cheaper than a bubble of c edges in
    float32 hop-by-hop sums although b - a + margin <= 100 c — in the forward tree (distances tref[] from the source)
    or in the backward one (the same sums from the sink: node j is at tref[n_ref - 1 - j]).  b is taken at the
    bound; a at 0, in the middle and at its largest."""
    tref = _tref(n_max + 2)
    bad = []
    n_ref = np.arange(2, n_max + 1)
    for c in range(2, max_stack + 2):
        span = np.minimum(100 * c - margin, n_ref - 1)          # b - a at the bound (or the longest there is)
        for pick in (0, 1, 2):
            a = (n_ref - 1 - span) * pick // 2                  # 0, middle, largest a with b <= n_ref - 1
            b = a + span
            ok = span >= 1
            via = tref[a].copy()
            for _ in range(c):                                  # c additions of 1.0f, one after the other
                via = via + np.float32(1.0)
            fwd = tref[b] < via
            # backward: dist_b[j] = tref[n_ref - 1 - j]; the bubble enters at b and reaches a after c hops
            via_b = tref[n_ref - 1 - b].copy()
            for _ in range(c):
                via_b = via_b + np.float32(1.0)
            bwd = tref[n_ref - 1 - a] < via_b
            for i in np.flatnonzero(ok & ~(fwd & bwd)).tolist():
                bad.append((int(n_ref[i]), int(a[i]), c))
    return bad


def test_margin_of_the_closed_forms_holds_in_float32_up_to_the_lds_tier_limit():
    """Both closed forms assume: whenever b - a + 10 <= 100 c the float32 sums keep the reference route strictly
    cheaper in both trees.  Checked for every n_ref the LDS tier accepts (the epilogue of k_dfs and 2c of k_graph run
    nowhere else), with the margin read from the three places of the headers that spell it.  With + 0 the same check
    fails: exact ties in real arithmetic, which the float32 sums decide either way."""
    limits = {k: _lds_tier_limit(k) for k in (11, 13, 15, 21, 31, 32)}
    n_max = max(limits.values())
    # tref[] stays below 64 there (a relative error below 2e-5 per hop, some 0.003 over 3 000 hops, against a margin
    # of 0.1); the sums through a bubble reach tref[a] + max_stack + 1
    assert 1000 < n_max < 4000, limits
    margins = _margins_in_the_kernels()
    assert len(set(margins)) == 1, margins
    assert _margin_violations(n_max, margins[0]) == []
    at_zero = _margin_violations(n_max, 0)
    assert at_zero, "a margin of 0 should fail somewhere: exact ties in real arithmetic"
    print("margin 0 fails at", len(at_zero), "triples, first", at_zero[:3])
    # the k = 11 sweep is meant for the LDS tier, the other sweeps for the large one
    assert len(_cases("sweep", 11)[0][0]["target"]) - 11 + 1 <= limits[11]
    assert len(_cases("sweep", 13)[0][0]["target"]) - 13 + 1 <= limits[13]
    assert len(_cases("sweep", 11)[0][-1]["target"]) - 11 + 1 <= limits[11]     # (the nested case)
    assert len(_cases("sweep", 15)[0][0]["target"]) - 15 + 1 > limits[15]
    assert len(_cases("sweep", 21)[0][0]["target"]) - 21 + 1 > limits[21]


def test_tref_shortcut_is_exact_only_where_the_distance_equals_tref():
    """k_graph copies tref[] along a reference chain only if the chain's head was reached at d == tref[cur]; otherwise
    it adds hop by hop.  Where the bubble is the cheaper route, b is reached at tref[a] + c != tref[b] and the
    oracle's own distances beyond b are NOT tref[]: taking the shortcut regardless would be wrong there.  Where the
    reference route wins they are tref[] bit for bit."""
    cases = _cases("sweep", 11)[0]
    wants = _python_wants("sweep", 11)
    for v in (10, -5):
        case, want = cases[MARGINS.index(v)], wants[MARGINS.index(v)]
        a, b, c, nodes = _bubble(want["kmers"], want["n_ref"], case["expect"]["del"])
        names = want["kmers"] + [ko.SOURCE, ko.SINK]
        n = len(names)
        w, _ = ko.build_graph(names, list(range(want["n_ref"])), 0, want["n_ref"] - 1)
        dist = _dist_from_prev(w, ko.dijkstra_prev(w, n - 2), n - 2)
        tref = _tref(want["n_ref"])
        assert (dist[:a + 1] == tref[:a + 1]).all()
        if v == 10:
            assert (dist[:want["n_ref"]] == tref).all()
        else:
            via = tref[a]
            for _ in range(c):
                via = np.float32(via + np.float32(1.0))
            assert dist[b] == via and via < tref[b]
            hop = via
            for j in range(b + 1, want["n_ref"]):               # the register loop of dependent adds
                hop = np.float32(hop + np.float32(0.01))
                assert dist[j] == hop
            assert (dist[b:want["n_ref"]] != tref[b:]).all()


@pytest.mark.parametrize("k", [11, 15])
def test_nested_case_is_decided_by_the_true_distances_past_the_inner_bubble(k):
    """Where the outer bubble rejoins the reference (b2) the oracle's winner is the reference edge from b2 - 1, reached
    through the inner bubble at a distance that is NOT tref[b2 - 1]; with tref[b2 - 1] in its place the outer bubble
    would win.  The same from the sink at a2.  So a chain loop of k_graph that copied tref[] without its guard
    `d == tref[cur]` gives another prev[b2] / after[a2], and other paths for the two SNVs."""
    cases = _cases("sweep", k)[0]
    case, want = cases[-1], _python_wants("sweep", k)[-1]
    assert case["kind"] == "nested"
    n_ref = want["n_ref"]
    a2, b2, c2, outer = _bubble(want["kmers"], n_ref, case["expect"]["outer"])
    names = want["kmers"] + [ko.SOURCE, ko.SINK]
    n = len(names)
    w, _ = ko.build_graph(names, list(range(n_ref)), 0, n_ref - 1)
    tref = _tref(n_ref)
    one, hop = np.float32(1.0), np.float32(0.01)
    prev = ko.dijkstra_prev(w, n - 2)
    dist = _dist_from_prev(w, prev, n - 2)
    assert prev[b2] == b2 - 1 and dist[b2 - 1] != tref[b2 - 1]
    assert np.float32(dist[b2 - 1] + hop) < np.float32(dist[outer[-1]] + one) < np.float32(tref[b2 - 1] + hop)
    after = ko.dijkstra_prev(w.transpose(), n - 1)
    back = _dist_from_prev(w.transpose(), after, n - 1)
    assert after[a2] == a2 + 1 and back[a2 + 1] != tref[n_ref - 1 - (a2 + 1)]
    assert np.float32(back[a2 + 1] + hop) < np.float32(back[outer[0]] + one) < np.float32(tref[n_ref - 2 - a2] + hop)
    # ... and the SNVs' paths show it: both run through the inner bubble, not the outer one
    inner = _bubble(want["kmers"], n_ref, case["expect"]["del"])[3]
    for tag in ("up", "down"):
        snv = _bubble(want["kmers"], n_ref, case["expect"][tag])[3]
        through = [p for p in want["paths"] if snv[0] in p]
        assert len(through) == 1 and inner[0] in through[0] and outer[0] not in through[0]


# ------------------------------------------------------------------ CPU: goldens from the unmodified reference
def _load_golden():
    with open(os.path.join(HERE, "golden", "crossover.json")) as fh:
        return json.load(fh)


def test_oracle_matches_the_reference_on_the_crossover_goldens():
    """tests/golden/crossover.json (make_golden.py --only crossover): the k = 11 cases of margin 10, 0 and -5, each
    alone with its own table, through the unmodified reference.  A case whose output moved with PYTHONHASHSEED is
    recorded as unstable and not compared."""
    import hashlib
    gold = _load_golden()
    assert [g["margin"] for g in gold["cases"]] == list(synth.CROSSOVER_GOLDEN)
    cases = _cases("sweep", 11)[0]
    compared = 0
    for g in gold["cases"]:
        case = cases[MARGINS.index(g["margin"])]
        keys, counts = synth.records_from_reads(case["reads"], 11)
        h = hashlib.md5(case["target"].encode())
        h.update(keys.tobytes())
        h.update(counts.tobytes())
        assert h.hexdigest() == g["input_md5"], "generator drifted; regenerate the goldens"
        if not g["stable_but_probes"]:
            continue
        res = ko.analyse_target(case["target"], case["name"], _cpu_db(keys, counts, 11))
        assert len(res["kmers"]) + 2 == g["num_k"]
        nodes = sorted([m, c] for m, c in zip(res["kmers"], res["counts"]))
        assert hashlib.md5(json.dumps(nodes).encode()).hexdigest() == g["nodes_md5"]
        assert res["probes"] in g["probes_seen"]
        allk = res["kmers"] + ["", ""]
        seqs = sorted(ko.spell(allk, p, True) for p in res["paths"])
        assert seqs == g["path_seqs"]
        by_seq = {ko.spell(allk, p, True): m for p, m in zip(res["paths"], res["min_cov"])}
        assert [by_seq[s] for s in seqs] == g["path_min_cov"]
        # its stripped-edge count is ours or ours - 1 (`if last_cur` skips whichever node its seed gave index 0)
        for removed, nonref in zip(g["removed_ref_edges"], g["nonref_edges"]):
            assert removed in (res["removed_ref_edges"], res["removed_ref_edges"] - 1)
            assert removed + nonref == res["removed_ref_edges"] + res["nonref_edges"]
        compared += 1
    assert compared >= 1


# ------------------------------------------------------------------ GPU
_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from km_amd import lib as kmlib
d = np.load(%(inp)r, allow_pickle=False)
k = int(d["k"])
db = kmlib.Database.from_records(d["keys"], d["counts"], k).upload(0)
seqs = [str(x) for x in d["seqs"]]
b = kmlib.Batch(db, max_targets=len(seqs), max_total_bases=sum(len(s_) for s_ in seqs))
b.set_targets(seqs)
b.run()
r = b.fetch()
removed, nonref, _loops, _n = b.graph_log(len(seqs))
np.savez(%(out)r, removed=removed, nonref=nonref, left=np.array(b.debug_counts()), n_big_tier=np.array(r["n_big_tier"]),
         **{k_: v for k_, v in r.items() if isinstance(v, np.ndarray)})
b.close()
db.close()
"""


def _child_run(tmp_path, tag, keys, counts, k, seqs, **env):
    inp, out = str(tmp_path / (tag + "_in.npz")), str(tmp_path / (tag + "_out.npz"))
    np.savez(inp, keys=keys, counts=counts, k=np.array(k), seqs=np.array(seqs))
    subprocess.check_call([sys.executable, "-c", _CHILD % {"root": ROOT, "inp": inp, "out": out}],
                          env=dict(os.environ, **env), timeout=300)
    r = dict(np.load(out))
    return r, (r["removed"], r["nonref"])


def _check_against_oracle(r, glog, wants, k, tag):
    """Everything test_gpu_parity._compare_with_oracle compares, on the fetched arrays, and the two numbers of the
    graph log where the oracle has them."""
    noff, poff = r["node_off"].astype(np.int64), r["path_off"].astype(np.int64)
    assert len(r["status"]) == len(wants)
    for t, want in enumerate(wants):
        assert int(r["status"][t]) == 0, (tag, t)
        assert int(r["n_ref"][t]) == want["n_ref"], (tag, t)
        assert [km.unpack(int(x), k) for x in r["node_kmer"][noff[t]:noff[t + 1]]] == want["kmers"], (tag, t)
        assert r["node_count"][noff[t]:noff[t + 1]].tolist() == list(want["counts"]), (tag, t)
        assert int(r["probes"][t]) == want["probes"], (tag, t)
        got = [kmlib.expand_path(r, p).tolist() for p in range(poff[t], poff[t + 1])]
        assert got == [list(p) for p in want["paths"]], (tag, t)
        assert r["path_min_cov"][poff[t]:poff[t + 1]].tolist() == list(want["min_cov"]), (tag, t)
        if glog is not None and "removed_ref_edges" in want:
            assert (int(glog[0][t]), int(glog[1][t])) == (want["removed_ref_edges"], want["nonref_edges"]), (tag, t)


def _three_ways(tmp_path, cases, keys, counts, k, wants, runs=1):
    """Default (`runs` times: the device's own large tier is armed by the first), captured and replayed, and with the
    epilogue of k_dfs off (a child process: the knob is read once): each against the oracle.  -> the first fetch."""
    seqs = [c["target"] for c in cases]
    db = kmlib.Database.from_records(keys, counts, k).upload(0)
    b = kmlib.Batch(db, max_targets=len(seqs), max_total_bases=sum(len(s_) for s_ in seqs))
    b.set_targets(seqs)
    first = None
    for i in range(runs):
        b.run()
        r = b.fetch()
        _check_against_oracle(r, b.graph_log(len(seqs))[:2], wants, k, "default run %d" % i)
        first = first or r
    both = kmlib.KM_STAGE_WALK | kmlib.KM_STAGE_GRAPH
    st = kmlib.stream_create(0)
    b.run(both | kmlib.KM_RUN_HIPGRAPH, st)
    b.run(both | kmlib.KM_RUN_HIPGRAPH, st)
    replay = b.fetch()
    _check_against_oracle(replay, b.graph_log(len(seqs))[:2], wants, k, "replayed")
    for name in FIELDS:
        assert np.array_equal(first[name], replay[name]), name
    flagged = b.debug_counts()[0]
    b.close()
    kmlib.stream_destroy(st)
    db.close()
    off, glog = _child_run(tmp_path, "epi_off", keys, counts, k, seqs, KM_EPILOGUE="0")
    assert int(off["left"][2]) == 0                             # (the epilogue was off there)
    _check_against_oracle(off, glog, wants, k, "KM_EPILOGUE=0")
    assert flagged == len(seqs)
    return first


@pytest.mark.gpu
@pytest.mark.parametrize("k", [11, 13, 15])
def test_crossover_sweep_matches_oracle(k, tmp_path):
    """One batch of eleven targets, 100 c - (b - a) from 12 down to -5 (a, b, c read off the oracle's node list; at
    k = 11 four more with the deletion alone, margins 10, 9, 0, -1: the one-bubble shape step 2c of k_graph answers;
    at k = 11 and 15 the nested case, whose answer needs the guard of the tref[] shortcut in both passes):
    status, node k-mers, counts, probes, paths in canonical order, minimum coverages and the graph log equal the
    Python oracle's — by default, replayed from a captured step, and with every flagged target through k_graph.
    k = 11 and 13 stay in the LDS tier (closed forms up to the margin, the frontier Dijkstra past it); the k = 15
    targets are longer than that tier holds and run in the large one."""
    cases, keys, counts = _cases("sweep", k)
    wants = _python_wants("sweep", k)
    for c, w in zip(cases, wants):
        _assert_bubbles_as_asked(c, w["kmers"], w["n_ref"])
    _assert_coverage(cases, wants, MARGINS)
    first = _three_ways(tmp_path, cases, keys, counts, k, wants, runs=2 if k == 15 else 1)
    if k in (11, 13):
        assert int(first["n_big_tier"]) == 0


@pytest.mark.gpu
def test_crossover_sweep_forced_into_the_large_tier(tmp_path):
    """The k = 11 sweep with a 170-base insertion haplotype near the end of every target: 180 more walk nodes than
    the LDS tier keeps per target, so walk and graph of every target run in the large tier (k_graph<BIG>: no closed
    form, always the general algorithm) — the host's on a workspace's first run, the device's own from the second,
    the host's alone with KM_BIG_DEVICE_OFF=1."""
    cases, keys, counts = _cases("sweep_ins", 11)
    wants = _python_wants("sweep_ins", 11)
    for c, w in zip(cases, wants):
        _assert_bubbles_as_asked(c, w["kmers"], w["n_ref"])
    _assert_coverage(cases, wants, MARGINS)
    first = _three_ways(tmp_path, cases, keys, counts, 11, wants, runs=2)
    assert int(first["n_big_tier"]) == len(cases)
    host, glog = _child_run(tmp_path, "host_tier", keys, counts, 11, [c["target"] for c in cases], KM_BIG_DEVICE_OFF="1")
    assert int(host["n_big_tier"]) == len(cases)
    _check_against_oracle(host, glog, wants, 11, "KM_BIG_DEVICE_OFF=1")


@pytest.mark.gpu
def test_crossover_in_the_large_tier_by_length_k21(tmp_path):
    """Targets of 2 368 bases take the large tier by their own length: margins 10, 1, 0, -1, -5 against the C oracle
    (the tie also against the Python oracle, graph log included), device tier and KM_BIG_DEVICE_OFF=1."""
    cases, keys, counts = _cases("sweep", 21)
    wants = [dict(w) for w in _c_wants("sweep", 21)]
    for c, w in zip(cases, wants):
        _assert_bubbles_as_asked(c, w["kmers"], w["n_ref"])
    _assert_coverage(cases, wants, MARGINS_K21)
    i, tie = _k21_tie_python()
    assert _same_as_python(wants[i], tie)
    wants[i] = tie
    _three_ways(tmp_path, cases, keys, counts, 21, wants, runs=2)
    host, glog = _child_run(tmp_path, "host_tier", keys, counts, 21, [c["target"] for c in cases], KM_BIG_DEVICE_OFF="1")
    _check_against_oracle(host, glog, wants, 21, "KM_BIG_DEVICE_OFF=1")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 31])
def test_exact_ties_inside_the_walks_own_nodes(k, tmp_path):
    """prev[] breaks ties by (dist, index): an insertion that splits three ways and rejoins at three equal float32
    distances, and two substitutions at one reference position — against the Python oracle, epilogue on and off,
    replayed."""
    cases, keys, counts = _cases("ties", k)
    wants = _python_wants("ties", k)
    for c, w in zip(cases, wants):
        _assert_bubbles_as_asked(c, w["kmers"], w["n_ref"])
    _three_ways(tmp_path, cases, keys, counts, k, wants)
