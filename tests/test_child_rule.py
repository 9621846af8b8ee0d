"""Jellyfish.get_child's keep rule (km/utils/Jellyfish.py:69-72) at its float64 edges, in every place
the library evaluates it.

The rule is ``count >= max(sum * ratio, n_cutoff)`` as Python evaluates it: a float64 product, Python's
``max`` and an exact int-against-float comparison.  The library turns it into an integer threshold
(device_common.h: threshold_of) and uses that in child_mask (32- and 64-bit sums), in slot_successor
(chain runs, with the thr_below shortcut), in k_children and in k_seed / k_dfs.  Everything here is
compared with ``_py_keep`` below — the rule in Python ints and floats, sharing nothing with the header
or with oracle/km_oracle.c — and every comparison is exact: integers and bit masks, no tolerances.

  1. the edge table, generated and asserted on the CPU;
  2. threshold_of / threshold_shortcut on the host (tests/host/child_rule_dump.hip) against the rule;
  3. k_children over databases constructed from the table (GPU);
  4. the same edges inside the walk: at a reference k-mer (k_seed), on a walked chain (k_dfs: dead end,
     branch), against oracle.km_oracle.analyse_target (GPU).
"""
import functools
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from km_amd import kmer as km
from km_amd import lib as kmlib
from oracle import km_oracle as ko

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = 0xFFFFFFFF


def _py_keep(counts, ratio, n_cutoff):
    """Which of the four children Jellyfish.get_child keeps."""
    threshold = max(sum(counts) * ratio, n_cutoff)
    return [c >= threshold for c in counts]


def _py_mask(counts, ratio, n_cutoff):
    return sum(1 << i for i, kept in enumerate(_py_keep(counts, ratio, n_cutoff)) if kept)


# ------------------------------------------------------------------ 1. the edge table
RATIO_LITERALS = ["0.0", "1e-9", "0.01", "0.05", "0.07", "0.1", "0.29", "0.3", "1/3", "0.5", "0.57", "0.999",
                  "1.0", "1.5"]
EXACT = {}                      # ratio.hex() -> the exact value of its literal
for _lit in RATIO_LITERALS:
    _fr = Fraction(_lit)
    EXACT[(_fr.numerator / _fr.denominator).hex()] = _fr
RATIOS = [float.fromhex(h) for h in EXACT]
assert RATIOS[4] == 0.07 and RATIOS[8] == 1 / 3 and RATIOS[1] == 1e-9
SUMS = (list(range(1, 301)) + list(range(400, 3001, 100)) + [65535 * m + d for m in (1, 2, 3, 4) for d in (-1, 0, 1)]
        + [2**30 - 1, 2**30, 2**30 + 1, 2**31 - 1, 2**31, 2**32 - 1, 2**32, 2**32 + 1, 2**34 - 5, 2**34 - 4])
SWEEP_CUTOFF = 1                # the ratio sweep's n_cutoff: a zero count is never kept, so the walk can use it
CUTOFFS = [-3, 0, 1, 5, 65535, 65536, 2**32 - 1, 2**32, 2**53 + 1]
CUTOFF_RATIOS = [0.0, 0.05]
COMPANIONS = [0, 7, 70000]
FIXED_PARAMS = [(0.0, 0), (0.05, 5), (0.3, 1), (1 / 3, 1), (0.5, 1), (1.0, 1)]
EXTRA_RATIOS = [-0.05, math.inf, math.nan]          # k_children (and the host harness) only


def _spread(total, edge, pos, others):
    """Four counts adding up to `total`: `edge` at `pos`, the rest over `others` (1 or 2) other children — over more
    where a count would pass 2^32 - 1.  None if that cannot be done."""
    rest = total - edge
    if not 0 <= edge <= F32 or rest < 0:
        return None
    parts = [rest - rest // 3, rest // 3, 0] if others == 2 else [rest, 0, 0]
    c = [0, 0, 0, 0]
    c[pos] = edge
    carry = 0
    for part, q in zip(parts, ((pos + 1) % 4, (pos + 3) % 4, (pos + 2) % 4)):
        v = part + carry
        carry = max(0, v - F32)
        c[q] = v - carry
    return None if carry else tuple(c)


def _make_table():
    table, pairs, cutoff_pairs = [], {}, {}

    def add(counts, ratio, n_cutoff):
        assert len(counts) == 4 and all(0 <= c <= F32 for c in counts)
        table.append((tuple(counts), ratio, n_cutoff))

    for ratio in RATIOS:
        for total in SUMS:
            t = total * ratio
            n_edges = 0
            for d in (-1, 0, 1):
                edge = math.ceil(t) + d
                if not 0 <= edge <= total:
                    continue
                for pos in range(4):
                    others = 1 + (pos + total) % 2
                    counts = _spread(total, edge, pos, others)
                    if counts is None:
                        continue
                    add(counts, ratio, SWEEP_CUTOFF)
                    n_edges += 1
                    if others == 1 and total - edge <= F32:
                        # a two-child triple: (the other child, the edge child) for the walk
                        pairs.setdefault((ratio.hex(), SWEEP_CUTOFF), {}).setdefault(total, {})[d] = (total - edge, edge)
            if n_edges == 0:                         # no edge count fits: the sum itself is still looked at
                add(_spread(total, total // 4, 0, 2), ratio, SWEEP_CUTOFF)
        # either side of the 32/64-bit split of child_mask, with an edge child beside the large count
        for big in (2**30 - 1, 2**30):
            edge = 0
            for _ in range(60):
                edge = math.ceil((big + edge) * ratio)
            for i, d in enumerate((-1, 0, 1)):
                if 0 <= edge + d <= big:
                    c = [0, 0, 0, 0]
                    c[i] = big
                    c[(i + 2) % 4] = edge + d
                    add(c, ratio, SWEEP_CUTOFF)
    for n_cutoff in CUTOFFS:
        for ratio in CUTOFF_RATIOS:
            for v in (n_cutoff - 1, n_cutoff, F32):
                if not 0 <= v <= F32:
                    continue
                for pos in range(4):
                    for comp in COMPANIONS:
                        c = [0, 0, 0, 0]
                        c[pos] = v
                        c[(pos + 1) % 4] = comp
                        add(c, ratio, n_cutoff)
                if v != F32:
                    for comp in COMPANIONS[1:]:
                        cutoff_pairs.setdefault((ratio.hex(), n_cutoff), {}).setdefault(comp, {})[v - n_cutoff] = (comp, v)
    fixed = [(0, 0, 0, 0), (F32,) * 4, (2**30 - 1, 7, 0, 5), (2**30, 7, 0, 5), (5, 2**30 - 1, 2**30 - 1, 2**30 - 1)]
    for v in (65535, 65534, 65536):
        fixed += [(v, 0, 0, 0), (0, 0, v, 0), (v, v, 0, 0), (0, v, 0, v), (v, v, v, v)]
    for ratio, n_cutoff in FIXED_PARAMS:
        for counts in fixed:
            add(counts, ratio, n_cutoff)
    extra = []
    for ratio in EXTRA_RATIOS:
        for n_cutoff in (-3, 0, 5):
            for counts in [(0, 0, 0, 0), (100, 7, 0, 0), (5, 4, 0, 0), (0, 65535, 65536, 1), (F32,) * 4, (0, 0, 2**30, 3)]:
                extra.append((counts, ratio, n_cutoff))
    return table, extra, pairs, cutoff_pairs


TABLE, EXTRA, PAIRS, CUTOFF_PAIRS = _make_table()
MASKS = [_py_mask(*t) for t in TABLE + EXTRA]


def _int_threshold(total, ratio, n_cutoff):
    """The smallest 32-bit count the rule keeps (None: it keeps none of them), by bisection over the rule itself."""
    thr = max(total * ratio, n_cutoff)
    if not F32 >= thr:
        return None
    lo, hi = -1, F32                                 # lo is dropped (or -1), hi is kept
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if mid >= thr:
            hi = mid
        else:
            lo = mid
    return hi


def test_edge_table_sits_on_the_edges():
    """The table is what it claims to be: triples where float64 and exact arithmetic part, children exactly at the
    threshold and one below it, and every size of answer."""
    assert 40_000 < len(TABLE) < 80_000, len(TABLE)
    assert ((0, 0, 0, 0), 0.0, 0) in TABLE and _py_mask((0, 0, 0, 0), 0.0, 0) == 15
    n_differ = n_at = n_below = 0
    popcounts = set()
    for counts, ratio, n_cutoff in TABLE:
        total = sum(counts)
        kept = _py_keep(counts, ratio, n_cutoff)
        exact = max(total * EXACT[ratio.hex()], n_cutoff)
        n_differ += kept != [c >= exact for c in counts]
        T = _int_threshold(total, ratio, n_cutoff)
        if T is not None:
            n_at += T in counts
            n_below += T - 1 in counts
        popcounts.add(sum(kept))
    assert n_differ >= 20 and n_at >= 20 and n_below >= 20, (n_differ, n_at, n_below)
    assert {0, 1, 2, 4} <= popcounts
    # the examples the rule is known by
    assert _py_keep((93, 7, 0, 0), 0.07, 1)[1] is False and _py_keep((95, 5, 0, 0), 0.05, 1)[1] is True
    assert any(r == 0.07 and sum(c) == 100 and 7 in c for c, r, _ in TABLE)
    assert any(r == 0.05 and sum(c) == 100 and 5 in c for c, r, _ in TABLE)
    # both sides of the 32/64-bit split of child_mask
    assert any(max(c) == 2**30 - 1 for c, _, _ in TABLE) and any(max(c) == 2**30 for c, _, _ in TABLE)
    for counts, ratio, n_cutoff in EXTRA:                # a product that is inf or NaN keeps nothing
        assert ratio < 0 or _py_mask(counts, ratio, n_cutoff) == 0


# ------------------------------------------------------------------ 2. threshold_of / threshold_shortcut on the host
@pytest.fixture(scope="module")
def rule_dump(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("child_rule") / "child_rule_dump")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "child_rule_dump.hip")],
                          stderr=subprocess.DEVNULL)

    def run(triples):
        """[(sum, ratio, n_cutoff)] -> [(T, none, below, thr_T)]"""
        text = "".join("%d %s %d\n" % (s, r.hex(), n) for s, r, n in triples)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-500:]
        rows = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
        assert len(rows) == len(triples)
        return rows
    return run


PROBES = (0, 65534, 65535, 65536, F32)


def _same_rule(total, ratio, n_cutoff, T, none, ctx):
    """Python keeps a count c iff not none and c >= T, for the counts where an integer threshold can be wrong."""
    thr = max(total * ratio, n_cutoff)
    for c in PROBES + (T - 1, T, T + 1):
        if 0 <= c <= F32:
            assert (c >= thr) == (not none and c >= T), (ctx, c)


def test_threshold_of_and_shortcut_equal_the_python_rule(rule_dump):
    """Every triple of the table through child_threshold and threshold_shortcut of device_common.h, on the host."""
    triples = [(sum(c), r, n) for c, r, n in TABLE + EXTRA]
    rows = rule_dump(triples)
    shortcut = {}
    for (total, ratio, n_cutoff), (T, none, below, thr_T) in zip(triples, rows):
        ctx = ("sum", total, "ratio", ratio, "n_cutoff", n_cutoff)
        _same_rule(total, ratio, n_cutoff, T, none, ctx + ("T", T, "none", none))
        if total < below:                            # the sums for which a chain run takes thr_T unseen
            _same_rule(total, ratio, n_cutoff, thr_T, 0, ctx + ("below", below, "thr_T", thr_T))
        seen = shortcut.setdefault((ratio.hex(), n_cutoff), (below, thr_T))
        assert seen == (below, thr_T), ctx
    # the last sum of every shortcut, and the first one past it (which must have another threshold)
    assert sum(below > 0 for below, _ in shortcut.values()) >= 20
    ends = []
    for (rhex, n_cutoff), (below, thr_T) in shortcut.items():
        if below > 0:
            ends.append((below - 1, float.fromhex(rhex), n_cutoff, thr_T, True))
            if below <= 1 << 36:
                ends.append((below, float.fromhex(rhex), n_cutoff, thr_T, False))
    for (total, ratio, n_cutoff, thr_T, inside), (T, none, _, _) in zip(ends, rule_dump([e[:3] for e in ends])):
        ctx = ("sum", total, "ratio", ratio, "n_cutoff", n_cutoff, "thr_T", thr_T)
        _same_rule(total, ratio, n_cutoff, T, none, ctx + ("T", T, "none", none))
        if inside:
            _same_rule(total, ratio, n_cutoff, thr_T, 0, ctx)
        else:
            assert (thr_T >= max(total * ratio, n_cutoff)) is False, ctx


# ------------------------------------------------------------------ 3. k_children on constructed quadruples
CHILD_DBS = [(15, True), (31, True), (32, True), (31, False), (32, False)]
ALL_TRIPLES = TABLE + EXTRA
COUNTS4 = np.array([t[0] for t in ALL_TRIPLES], dtype=np.uint32)
GROUPS = {}
for _i, (_c, _r, _n) in enumerate(ALL_TRIPLES):
    GROUPS.setdefault((_r.hex(), _n), []).append(_i)


def _children_of(parents, k, forward):
    """[n, 4] k-mers: parent[1:] + c (forward) or c + parent[:-1]."""
    kmask = np.uint64((1 << (2 * k)) - 1)
    base = np.arange(4, dtype=np.uint64)
    if forward:
        return ((parents[:, None] << np.uint64(2)) | base[None, :]) & kmask
    return (parents[:, None] >> np.uint64(2)) | (base[None, :] << np.uint64(2 * (k - 1)))


def _stored_keys(kids, k, canonical):
    return km.canonical(kids, k) if canonical else kids


def _parents(k, canonical, forward, all_t_at=None):
    """One random parent k-mer per triple such that the stored keys of all their children are distinct: parents whose
    children collide are drawn again (k = 15 leaves too little room for luck).  `all_t_at`: this parent is T...T."""
    rng = np.random.default_rng(9000 + 100 * k + 10 * canonical + forward)
    n = len(ALL_TRIPLES)
    top = 1 << (2 * k)
    parents = rng.integers(0, top, size=n, dtype=np.uint64)
    for _ in range(100):
        if all_t_at is not None:
            parents[all_t_at] = top - 1
        keys = _stored_keys(_children_of(parents, k, forward), k, canonical).reshape(-1)
        _, inverse, times = np.unique(keys, return_inverse=True, return_counts=True)
        again = (times[inverse.reshape(-1)] > 1).reshape(n, 4).any(axis=1)
        if all_t_at is not None:
            again[all_t_at] = False
        if not again.any():
            break
        parents[again] = rng.integers(0, top, size=int(again.sum()), dtype=np.uint64)
    return parents


@pytest.mark.gpu
@pytest.mark.parametrize("k,canonical", CHILD_DBS)
def test_k_children_keeps_what_python_keeps(k, canonical):
    """One parent per triple, its four children stored with the triple's counts, forward and backward: the mask,
    the four counts and every single query."""
    want_mask = np.array(MASKS, dtype=np.uint8)
    all_t_at = None
    if (k, canonical) == (32, False):                # its child T...T is the key ~0
        all_t_at = next(i for i, t in enumerate(ALL_TRIPLES) if t[0][3] > 0)
    for forward in (True, False):
        parents = _parents(k, canonical, forward, all_t_at)
        kids = _children_of(parents, k, forward)
        keys = _stored_keys(kids, k, canonical).reshape(-1)
        assert np.unique(keys).size == keys.size     # no two children share a record, across all parents
        counts = COUNTS4.reshape(-1)
        if all_t_at is not None:
            assert int(keys[4 * all_t_at + 3]) == 2**64 - 1 and int(counts[4 * all_t_at + 3]) > 0
        present = counts > 0
        order = np.argsort(keys[present])
        db = kmlib.Database.from_records(keys[present][order], counts[present][order], k, canonical).upload(0)
        try:
            assert (db.query(kids.reshape(-1)) == counts).all()
            for (rhex, n_cutoff), idx in GROUPS.items():
                idx = np.array(idx)
                mask, counts4 = db.children(parents[idx], float.fromhex(rhex), n_cutoff, forward)
                ctx = (k, canonical, forward, rhex, n_cutoff)
                assert (counts4 == COUNTS4[idx]).all(), ctx
                bad = np.nonzero(mask != want_mask[idx])[0]
                assert bad.size == 0, ctx + (ALL_TRIPLES[idx[bad[0]]], int(mask[bad[0]]), int(want_mask[idx[bad[0]]]))
        finally:
            db.close()


# ------------------------------------------------------------------ 4. the same edges inside the walk
WALK_KS = [11, 31, 32]
WALK_GROUPS = [(0.05, 1), (0.07, 1), (0.29, 1), (1 / 3, 1), (0.5, 1), (0.57, 1),
               (0.0, 5), (0.0, 65535), (0.05, 65535), (0.0, 65536)]
LONG_GROUP = (0.07, 1)           # this one also walks targets of the large tier (k >= 31: 4^11 k-mers leave no room
                                 # for two 2600-base targets that share no k-mer)
LONG_LENGTH = 2600
SCALED_SUMS = [2**30 - 1, 2**30, 2**30 + 1]


def _small_sums(ratio, n_cutoff):
    """Four sums below 65535 for a ratio: first those at which the float64 and the exact product part."""
    differ = []
    for total, by_d in sorted(PAIRS[(ratio.hex(), n_cutoff)].items()):
        if 20 <= total <= 300:
            exact = max(total * EXACT[ratio.hex()], n_cutoff)
            if any((b >= max(total * ratio, n_cutoff)) != (b >= exact) for _, b in by_d.values()):
                differ.append(total)
    sums = differ[-2:]
    for total in (300, 257, 100, 64):
        if total not in sums and len(sums) < 4:
            sums.append(total)
    return sums


def _group_cases(ratio, n_cutoff):
    """[(shape, regime, A, B, C, override)] of one (ratio, n_cutoff) from the table's two-child triples.
    seed: reads of the target carry A, of the variant B (the edge), decided at a reference k-mer;
    dead: B sits at the threshold and is kept, the 6th k-mer of the variant chain is set to `override`;
    chain: a second variant branches off the first 5 bases on, (B, C) is the edge pair."""
    cases = []
    if n_cutoff == SWEEP_CUTOFF:
        pairs = PAIRS[(ratio.hex(), n_cutoff)]
        for regime, sums in (("small", _small_sums(ratio, n_cutoff)), ("scaled", SCALED_SUMS)):
            for total in sums:
                by_d = pairs[total]
                assert sorted(by_d) == [-1, 0, 1]
                for d in (-1, 0, 1):
                    a, b = by_d[d]
                    cases.append(("seed", regime, a, b, None, None))
                    cases.append(("chain", regime, max(1, (a + b) // 4), a, b, None))
                a, b = by_d[0]
                cases.append(("dead", regime, a, b, None, n_cutoff - 1))
                cases.append(("dead", regime, a, b, None, n_cutoff))
    else:
        pairs = CUTOFF_PAIRS[(ratio.hex(), n_cutoff)]
        for rep in range(4):
            for comp, regime in ((7, "small"), (70000, "scaled")):
                by_d = pairs[comp]
                assert sorted(by_d) == [-1, 0]
                for d in (-1, 0):
                    a, b = by_d[d]
                    cases.append(("seed", regime, a, b, None, None))
                    cases.append(("chain", regime, max(1, (a + b) // 4), a, b, None))
                a, b = by_d[0]
                cases.append(("dead", regime, a, b, None, n_cutoff - 1 + rep % 2))
    return cases


def _other(base):
    return "ACGT"[("ACGT".index(base) + 1) % 4]


def _stored(seq, k):
    return km.canonical(km.sliding_kmers(km.encode(seq), k), k).tolist()


@functools.lru_cache(maxsize=None)
def _walk_batch(k, ratio, n_cutoff):
    """Targets, records and the oracle's answers of one batch.  Every target is drawn until neither it nor its
    variants repeat a stored k-mer, of their own or of an earlier case: each count is then exactly the constructed
    one, and no target has a repeated k-mer."""
    rng = np.random.default_rng(7000 + 1000 * k + n_cutoff % 1000 + int(ratio * 1000))
    cases = [(c, 4 * k + 20) for c in _group_cases(ratio, n_cutoff)]
    if (ratio, n_cutoff) == LONG_GROUP and k >= 31:
        by_d = PAIRS[(ratio.hex(), n_cutoff)][100]
        long_cases = [("chain", "long", 25, by_d[d][0], by_d[d][1], None) for d in (-1, 0)]
        cases = [(c, LONG_LENGTH) for c in long_cases] + cases       # (first: they need the most room)
    assert 40 <= len(cases) <= 100
    acc, targets, info = {}, [], []
    p = 2 * k
    for i, ((shape, regime, a, b, c, override), length) in enumerate(cases):
        for _ in range(10_000):
            target = km.decode(rng.integers(0, 4, length).astype(np.uint8))
            v1 = target[:p] + _other(target[p]) + target[p + 1:]
            reads = [(target, a), (v1, b)]
            marker = v1[k + 1:2 * k + 1]                                  # first k-mer of the variant chain
            if shape == "chain":
                v2 = v1[:p + 5] + _other(v1[p + 5]) + v1[p + 6:]
                reads.append((v2, c))
                marker = v2[k + 6:2 * k + 6]                              # first k-mer of the branch off the chain
            fresh = set()
            for seq, _ in reads:
                fresh.update(_stored(seq, k))
            n_ref = length - k + 1
            if len(fresh) == n_ref + k * (len(reads) - 1) and not (fresh & acc.keys()):
                break
        else:
            raise AssertionError("no collision-free target")
        assert len(set(target[j:j + k] for j in range(n_ref))) == n_ref   # no repeated k-mer
        for seq, cov in reads:
            for key in _stored(seq, k):
                acc[key] = acc.get(key, 0) + cov
        if override is not None:
            acc[_stored(v1[k + 6:2 * k + 6], k)[0]] = override            # the 6th k-mer of the variant chain
        targets.append(("%s_%s_%03d" % (shape, regime, i), target))
        info.append((shape, regime, marker))
    assert all(0 <= v <= F32 for v in acc.values())
    keys = np.array(sorted(x for x, v in acc.items() if v > 0), dtype=np.uint64)
    counts = np.array([acc[x] for x in keys.tolist()], dtype=np.uint32)
    cpu = ko.KmerDB(None, cutoff=ratio, n_cutoff=n_cutoff,
                    records={"k": k, "canonical": True, "keys": keys, "counts": counts})
    want = [ko.analyse_target(seq, name, cpu) for name, seq in targets]
    return targets, info, keys, counts, want


def _found(info, want):
    """{shape: [the variant's marker k-mer is a node of the oracle's walk, per case]}"""
    out = {}
    for (shape, _, marker), w in zip(info, want):
        out.setdefault(shape, []).append(marker in w["kmers"])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,n_cutoff", WALK_GROUPS)
@pytest.mark.parametrize("k", WALK_KS)
def test_walk_decides_the_edges_like_the_oracle(k, ratio, n_cutoff):
    """Constructed targets whose variant sits at T - 1, T or T + 1 of the branching k-mer — at a reference k-mer,
    behind a dead end at n_cutoff - 1 / n_cutoff on the walked chain, and at a branch on the chain — with counts
    below 65535 and far above: nodes, counts, probes and paths equal the Python oracle's."""
    from km_amd.finder import BatchFinder
    from km_amd.jellyfish import Jellyfish
    targets, info, keys, counts, want = _walk_batch(k, ratio, n_cutoff)
    # the edge is on the edge: each shape's variant is found in at least a third of its cases and missed in a third
    for shape, flags in _found(info, want).items():
        assert 3 * sum(flags) >= len(flags) and 3 * (len(flags) - sum(flags)) >= len(flags), (shape, flags)
    assert {i[1] for i in info} >= {"small", "scaled"} and {i[0] for i in info} == {"seed", "dead", "chain"}
    db = kmlib.Database.from_records(keys, counts, k).upload(0)
    try:
        assert (db.query(keys) == counts).all()
        finder = BatchFinder(Jellyfish("mem.jf", cutoff=ratio, n_cutoff=n_cutoff, db=db))
        got = finder.analyse(targets)
        for (name, _), g, w in zip(targets, got, want):
            assert not isinstance(g, Exception), (name, g)
            assert g.n_ref == w["n_ref"], name
            assert [km.unpack(x, k) for x in g.kmers] == w["kmers"], name
            assert g.counts.tolist() == w["counts"], name
            assert g.probes == w["probes"], name
            assert [p.tolist() for p in g.paths] == [list(p) for p in w["paths"]], name
            assert list(g.min_cov) == w["min_cov"], name
        if (ratio, n_cutoff) == LONG_GROUP and k >= 31:
            n_long = sum(len(seq) == LONG_LENGTH for _, seq in targets)
            assert n_long == 2 and finder.run_raw([seq for _, seq in targets])["n_big_tier"] > 0
    finally:
        db.close()
