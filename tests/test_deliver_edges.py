"""The delivery's second tries and the path half of k_out_pack (km_amd/csrc/deliver_kernel.h, result_host.h:
finish_result).  tests/test_deliver_chain.py covers a step that is delivered once; here a step is delivered again
because the escape list of the 16-bit counts overflowed, because the tail is larger than the buffer, or both, and the
tail is larger than the part copied along with region A.  Every expectation is the plain-C oracle's, target by target;
how often a step was delivered is read from totals[OT_SERIAL], which goes up by one per delivery.

The paths of a target are ranked by rle_less, which compares two run-length lists that may cut the same index
sequence at different places: it is compiled for the host (tests/host/rle_order.hip) and compared with Python's list
order, once more under AddressSanitizer and UBSan; on the GPU the ranks are pinned at 63, 64, 65, 127, 128 and 129 paths
of one target (the `i += 64` trips of the ranking loop).

Not reached: k_out_pack's loops for a path of more than 64 runs (the largest run count seen is 15).  Over
1 200 dense small-k tables with 24 targets each the oracle's longest path has 15 runs.  The directed construction —
walk-discovered nodes n_m .. n_1 that form a chain n_m -> .. -> n_1 but are registered one by one, each from a
reference k-mer x_i of its own, so that the chain is numbered against its direction and costs one run per node — does
not give such a path: x_i must end with the (k-1)-mer n_i begins with, which is the one n_(i+1) ends with, so the
graph has the edge n_(i+1) -> successor of x_i, and the reference route from there (0.01 per edge) is cheaper than
staying on the chain (1 per edge) unless more than 100 reference edges lie ahead per chain node kept: 6 300 k-mers for
64 nodes, far outside the LDS tier and these batches.  No oracle-accepted input found reaches those loops."""
import functools
import os
import re
import subprocess
import tempfile
import atexit
import shutil

import numpy as np
import pytest

from km_amd import kmer as km
from km_amd import lib as kmlib
from km_amd import synth
from oracle import c_oracle
from test_deliver_chain import (C16, DELIVER, K, LEAN, NOT_BARE, OT_NEEDS_HOST, OT_SERIAL, _check_against_oracle, _copy,
                                _totals)
from test_lds_tier_edges import FAST_EXTRA, _feature_case, _table, model_geometry, model_walk

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "km_amd", "csrc")
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------- the library's own arithmetic
def _source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


@functools.lru_cache(maxsize=None)
def _numbers():
    """The numbers the thresholds below are made of, read from the headers; the formulas they stand in are restated
    in lib_* below and their source lines are asserted to be there, so a change of either shows here."""
    deliver, batch, walk = _source("deliver_kernel.h"), _source("batch_host.h"), _source("walk_kernel.h")
    n = {"esc_cap": int(re.search(r"constexpr uint32_t OUT_ESC_CAP = (\d+);", deliver).group(1)),
         "ot_words": int(re.search(r"OT_WORDS = (\d+)", deliver).group(1)),
         "groups": int(re.search(r"constexpr uint32_t POOL_GROUPS = (\d+);", walk).group(1))}
    # batch_host.h, PathPools::alloc
    m = re.search(r"path_pool = small_pools \? 2 \* POOL_GROUPS : \(\(\(uint64_t\)n \* (\d+) \+ (\d+)\) / POOL_GROUPS \+ 1\) \* POOL_GROUPS;",
                  batch)
    n["path_per_target"], n["path_min"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"run_pool = small_pools \? 4 \* POOL_GROUPS : \(\(\(uint64_t\)n \* (\d+) \+ (\d+)\) / POOL_GROUPS \+ 1\) \* POOL_GROUPS;",
                  batch)
    n["run_per_target"], n["run_min"] = int(m.group(1)), int(m.group(2))
    # batch_host.h: layout_targets, ensure_out, km_batch_create, default_tail_bytes
    assert "b->out.tail_guess = 4 * total_ref + total_ref / 2 + (64u << 10);" in batch
    assert "const uint64_t cap = need + need / 8;" in batch
    assert "ensure_out(b, default_tail_bytes(b, max_total_bases + 16ull * max_targets, 16ull * max_targets))" in batch
    assert ("return out_align(4 * nodes) + out_align(8 * extra) + 2 * out_align(4 * b->paths.path_pool) +\n"
            "         out_align(8 * (b->paths.path_pool + 1)) + 2 * out_align(4 * b->paths.run_pool) + 256;") in batch
    assert "uint64_t guess = std::min<uint64_t>(oa.tail_cap, b->out.tail_guess);" in batch
    assert "oa.tail_cap = b->out.out_cap - L.a_bytes;" in batch
    assert "const uint32_t pg = t % POOL_GROUPS;" in _source("graph_kernel.h")
    return n


def _align(v, m=16):
    return (v + m - 1) // m * m


def lib_a_bytes(n):
    """batch_host.h: out_layout(n).a_bytes — region A of a delivery of n targets."""
    num = _numbers()
    o = 0
    for size in (8 * num["ot_words"], 4 * n, 4 * n, 8 * n, 8 * (n + 1), 8 * (n + 1), 4 * (n + 1), 4 * n,
                 8 * num["esc_cap"], 4 * num["esc_cap"]):
        o = _align(o + size, 64)
    return o


def lib_pools(max_targets):
    """batch_host.h: PathPools::alloc — (paths, runs) the pools of a new workspace hold."""
    num = _numbers()
    g = num["groups"]
    return (((max_targets * num["path_per_target"] + num["path_min"]) // g + 1) * g,
            ((max_targets * num["run_per_target"] + num["run_min"]) // g + 1) * g)


def lib_tail_cap(max_targets, max_total_bases, n_targets):
    """Bytes of tail the buffer km_batch_create made holds in a delivery of n_targets (batch_host.h: km_batch_create
    -> ensure_out -> out_cap = 9/8 need; enqueue_deliver: tail_cap = out_cap - a_bytes)."""
    path_pool, run_pool = lib_pools(max_targets)
    nodes, extra = max_total_bases + 16 * max_targets, 16 * max_targets
    tail = (_align(4 * nodes) + _align(8 * extra) + 2 * _align(4 * path_pool) + _align(8 * (path_pool + 1)) +
            2 * _align(4 * run_pool) + 256)
    need = lib_a_bytes(max_targets) + tail
    return need + need // 8 - lib_a_bytes(n_targets)


def lib_tail_guess(wants):
    """batch_host.h: layout_targets — the bytes of tail copied along with region A until a delivery has told better."""
    total_ref = sum(w["n_ref"] for w in wants)
    return 4 * total_ref + total_ref // 2 + 65536


def _runs(path):
    return 1 + sum(1 for a, b in zip(path[:-1], path[1:]) if b != a + 1)


def oracle_tail(wants, count_bytes=4):
    """deliver_kernel.h: k_out_pack — the tail of a full delivery of these answers, laid out with out_align.
    -> (bytes, offset of run_len, runs)."""
    nodes = sum(len(w["kmers"]) for w in wants)
    extra = sum(len(w["kmers"]) - w["n_ref"] for w in wants)
    paths = sum(len(w["paths"]) for w in wants)
    runs = sum(_runs(p) for w in wants for p in w["paths"])
    o = _align(count_bytes * nodes)
    o = _align(o + 8 * extra)
    o = _align(o + 4 * paths)
    o = _align(o + 4 * paths)
    o = _align(o + 8 * (paths + 1))
    o = _align(o + 4 * runs)
    off_rlen = o
    return _align(o + 4 * runs), off_rlen, runs


# ---------------------------------------------------------------------------- 3. rle_less on the CPU
@functools.lru_cache(maxsize=None)
def _rle_order(sanitize=False):
    """tests/host/rle_order.hip, compiled once per session (host code only; hipcc is what builds the library)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    tmp = tempfile.mkdtemp(prefix="km_rle_order_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "rle_order_san" if sanitize else "rle_order")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1" if sanitize else "-O2", "-std=c++17"] + extra +
                          ["-o", exe, os.path.join(HERE, "host", "rle_order.hip")])
    return exe


def _cut(seq, rng, p):
    """A run list of the index sequence `seq`: a run ends where the next index is not the successor, and with
    probability p anywhere else (p = 1: every run has length 1)."""
    runs = []
    for x in seq:
        if runs and x == runs[-1][0] + runs[-1][1] and not rng.random() < p:
            runs[-1][1] += 1
        else:
            runs.append([x, 1])
    return runs


def _expand(runs):
    return [s + i for s, n in runs for i in range(n)]


def _stretches(rng, n_stretches, longest=9):
    """An index sequence of n_stretches runs of consecutive indices that do not continue one another."""
    seq = []
    for _ in range(n_stretches):
        while True:
            s = int(rng.integers(0, 3000))
            if not seq or s != seq[-1] + 1:
                break
        seq += list(range(s, s + int(rng.integers(1, longest + 1))))
    return seq


def _rle_pairs():
    """(run list a, run list b, what the pair is) — the sequences are what is compared, the cuts are arbitrary."""
    rng = np.random.default_rng(5303)
    pairs = []
    ps = (0.0, 0.3, 1.0)
    for i in range(3000):
        a = _stretches(rng, 200 if i % 50 == 0 else 1 if i % 7 == 0 else int(rng.integers(1, 12)))
        kind = ("same", "inside", "first", "last", "prefix", "other")[i % 6]
        pa, pb = ps[int(rng.integers(0, 3))], ps[int(rng.integers(0, 3))]
        if kind == "same":                                     # one sequence, two cuts: neither is less
            ra, rb = _cut(a, rng, pa), _cut(a, rng, pb)
            assert _expand(ra) == _expand(rb) == a
        elif kind == "inside":
            # the first difference inside a run of a (uncut there) and at a run boundary of b: b leaves a's run early
            j = int(rng.integers(0, len(a)))
            b = a[:j] + [a[j] + int(rng.integers(1, 5)) * (1 if rng.random() < 0.5 or a[j] < 5 else -1)] + a[j + 1:]
            ra, rb = _cut(a, rng, 0.0), _cut(b, rng, pb)
        elif kind in ("first", "last"):
            j = 0 if kind == "first" else len(a) - 1
            b = list(a)
            b[j] += 1 if rng.random() < 0.5 or b[j] == 0 else -1
            ra, rb = _cut(a, rng, pa), _cut(b, rng, pb)
        elif kind == "prefix":
            b = a[:int(rng.integers(0, len(a)))]               # (the empty list too: no runs at all)
            ra, rb = _cut(a, rng, pa), _cut(b, rng, pb)
        else:
            ra, rb = _cut(a, rng, pa), _cut(_stretches(rng, int(rng.integers(1, 12))), rng, pb)
        pairs.append((ra, rb, kind) if i % 2 else (rb, ra, kind))
    # by hand: a run of one list against the same indices as single runs, a difference at the last index of a long run
    pairs += [([[5, 4]], [[5, 1], [6, 1], [7, 1], [8, 1]], "same"), ([[5, 4]], [[5, 2], [7, 1], [9, 1]], "inside"),
              ([[0, 200]], [[0, 199], [200, 1]], "last"), ([[0, 200]], [[0, 100], [100, 99]], "prefix"),
              ([[7, 1]], [[7, 1]], "same"), ([], [], "same"), ([], [[0, 1]], "prefix"),
              ([[10, 3], [20, 2]], [[10, 2], [12, 1], [20, 1], [21, 1], [3, 1]], "prefix")]
    return pairs


def test_rle_less_is_the_order_of_the_expanded_lists():
    """rle_less(a, b) and rle_less(b, a) against Python's `<` on the expanded index lists, a few thousand pairs: one
    sequence cut at different places (neither less), a first difference inside a run of one list and at a boundary of
    the other, at the first and at the last index, proper prefixes, single-run and 200-run lists, runs of length 1
    throughout.  The same input once more through a build with AddressSanitizer and UBSan (every list in a heap
    block of its own size: a read past a list's end stops it)."""
    pairs = _rle_pairs()
    kinds = {}
    for ra, rb, kind in pairs:
        kinds[kind] = kinds.get(kind, 0) + 1
    assert min(kinds[x] for x in ("same", "inside", "first", "last", "prefix", "other")) >= 400
    assert sum(len(ra) >= 200 or len(rb) >= 200 for ra, rb, _ in pairs) >= 50
    assert sum(len(ra) == 1 and len(rb) == 1 for ra, rb, _ in pairs) >= 20
    assert sum(all(n == 1 for _, n in ra) and len(ra) > 3 for ra, rb, _ in pairs) >= 300
    # (inside a run of one list, at a boundary of the other: the case the cuts are there for)
    n_inside = 0
    for ra, rb, kind in pairs:
        if kind == "inside":
            a, b = _expand(ra), _expand(rb)
            if len(a) != len(b):
                a, b, ra, rb = b, a, rb, ra
            j = next(i for i in range(len(a)) if a[i] != b[i])
            for runs, seq in ((ra, a), (rb, b)):
                starts = np.cumsum([0] + [n for _, n in runs]).tolist()
                n_inside += j not in starts
    assert n_inside >= 150
    text = "".join("%d %s\n" % (len(r), " ".join("%d %d" % (s, n) for s, n in r)) for ra, rb, _ in pairs for r in (ra, rb))
    want = ["%d %d" % (_expand(ra) < _expand(rb), _expand(rb) < _expand(ra)) for ra, rb, _ in pairs]
    assert {"0 0", "0 1", "1 0"} == set(want)
    for sanitize in (False, True):
        out = subprocess.run([_rle_order(sanitize)], input=text, capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert out.returncode == 0, out.stderr[-3000:]
        assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
        got = out.stdout.splitlines()
        assert len(got) == len(want)
        for (ra, rb, kind), g, w in zip(pairs, got, want):
            assert g == w, (kind, ra, rb)


# ---------------------------------------------------------------------------- 1. the escape list at its capacity
HOT_VALUES = (65_535, 65_536, 70_000, 2 ** 32 - 1)
ESC_N_REF = 500
# targets 0 .. 4: every k-mer hot (500 each); 5: its first 47; 6 and 7: one, in the middle / the last; 8: three;
# 9 .. 12: every k-mer hot and 13: its first 49, none of them 2^32 - 1 (a maximum that ref_max_cov cannot tell from NOT_BARE)
ESC_SETS = {2047: (5, 0, 1, 2, 3), 2048: (0, 6, 1, 5, 2, 3), 2049: (7, 0, 1, 6, 2, 3, 5), "all": (0, 1, 2, 3, 4), 3: (8,),
            "lean2049": (13, 9, 10, 11, 12)}
ESC_TARGETS = 14


@functools.lru_cache(maxsize=None)
def _escape_world():
    """Fourteen pure-reference targets of 500 k-mers, no k-mer twice in the batch, so a raised count changes no edge: every
    k-mer has one child in the table.  -> (keys, counts, seqs, the oracle's answers)."""
    case = synth.make_case(n_targets=ESC_TARGETS, length=ESC_N_REF + K - 1, n_keys=9000, seed=5201, variant_frac=0.0,
                           noise_frac=0.0, exact_pad=False)
    seqs = [km.decode(r) for r in case["targets"]]
    keys, counts = case["keys"].copy(), case["counts"].copy()
    kms = [km.canonical(km.sliding_kmers(km.encode(s), K), K) for s in seqs]
    assert np.unique(np.concatenate(kms)).size == ESC_TARGETS * ESC_N_REF
    order = np.argsort(keys)
    hot = [(t, pos) for t in range(5) for pos in range(ESC_N_REF)] + [(5, pos) for pos in range(47)]
    hot += [(6, ESC_N_REF // 2), (7, ESC_N_REF - 1), (8, 0), (8, ESC_N_REF // 2), (8, ESC_N_REF - 1)]
    below = [(t, pos) for t in range(9, 13) for pos in range(ESC_N_REF)] + [(13, pos) for pos in range(49)]
    for i, (t, pos) in enumerate(hot + below):
        at = order[np.searchsorted(keys[order], kms[t][pos])]
        assert keys[at] == kms[t][pos]
        counts[at] = HOT_VALUES[(i + i // 7) % 4] if i < len(hot) else HOT_VALUES[(i + i // 7) % 3]
    co = c_oracle.COracle(keys, counts, K)
    wants = [co.analyse(km.encode(s)) for s in seqs]
    for w in wants:                                            # pure reference: the bare path, no node of the walk's
        assert w["status"] == 0 and w["n_ref"] == ESC_N_REF == len(w["kmers"]) and w["paths"] == [list(range(ESC_N_REF))]
    return keys, counts, seqs, wants


def _escape_set(name):
    """-> (seqs, wants, all node counts of the set in delivery order, the indices of those >= 65535)."""
    _keys, _counts, seqs, wants = _escape_world()
    ts = ESC_SETS[name]
    all_counts = np.concatenate([wants[t]["counts"] for t in ts])
    return [seqs[t] for t in ts], [wants[t] for t in ts], all_counts, np.nonzero(all_counts >= 0xFFFF)[0]


def test_escape_sets_hold_exactly_n_hot_counts():
    """Before anything runs on the GPU: the oracle's counts of each target set hold exactly N values >= 65535, the
    four values are all there, and N sits on both sides of the list's capacity."""
    cap = _numbers()["esc_cap"]
    assert cap == 2048
    for name in ESC_SETS:
        _seqs, _wants, all_counts, big = _escape_set(name)
        assert big.size == {"all": len(all_counts), "lean2049": 2049}.get(name, name), name
        if name != 3:
            assert set(all_counts[big].tolist()) == set(HOT_VALUES[:3] if name == "lean2049" else HOT_VALUES), name
    assert len(_escape_set("all")[2]) == 2500 > cap + 1
    assert [n > cap for n in (2047, 2048, 2049)] == [False, False, True]


def _serial(bt):
    return int(_totals(bt.result())[OT_SERIAL])


def _rows(res, seqs):
    names = ["t%d" % i for i in range(len(seqs))]
    return kmlib.report_rows(res, names, seqs, K, "edges.jf")


@gpu
def test_escape_list_at_2047_2048_2049_and_every_count():
    keys, counts, _seqs, _wants = _escape_world()
    cap = _numbers()["esc_cap"]
    db = kmlib.Database.from_records(keys, counts, K).upload(0)
    st = kmlib.stream_create(0)
    bt = kmlib.Batch(db, max_targets=9, max_total_bases=9 * (ESC_N_REF + K - 1))
    top = 2 ** 32 - 1
    assert top == NOT_BARE
    state = {"serial": 0}

    def step(flags):
        """-> (a copy of the view, the step's sizes, how often it was delivered)"""
        bt.run(flags, st)
        sizes = bt.wait_result()
        view = _copy(bt.result())
        now = _serial(bt)
        state["serial"], delivered = now, now - state["serial"]
        return view, sizes, delivered

    def check16(name):
        seqs, wants, all_counts, big = _escape_set(name)
        bt.set_targets(seqs)
        v, sizes, delivered = step(DELIVER | C16)
        _check_against_oracle(v, wants, ("C16", name))
        if big.size <= cap:
            assert delivered == 1, (name, delivered)
            assert "node_count16" in v and sizes.n_count_escapes == big.size, name
            esc_node, esc_value = v["count_esc_node"].astype(np.int64), v["count_esc_value"]
            assert esc_node.size == big.size and (np.diff(esc_node) > 0).all(), name
            assert np.array_equal(esc_node, big) and np.array_equal(esc_value, all_counts[big]), name
            assert np.array_equal(v["node_count16"] == 0xFFFF, all_counts >= 0xFFFF), name
        else:
            assert delivered == 2, (name, delivered, "the 16-bit delivery must be thrown away and replaced")
            assert "node_count16" not in v and "count_esc_node" not in v and sizes.n_count_escapes == 0, name
            assert np.array_equal(v["node_count"], all_counts), name
        return v

    for name in (2047, 2048, 2049, 3, "all", 3):               # (3: the step behind one that overflowed)
        check16(name)
    # lean: the counts of bare-reference targets are not sent, so nothing escapes, whatever N is
    seqs, wants, all_counts, big = _escape_set("lean2049")
    bt.set_targets(seqs)
    v, sizes, delivered = step(DELIVER | LEAN | C16)
    assert delivered == 1 and sizes.n_count_escapes == 0 and "node_count16" in v and v["node_count"].size == 0
    _check_against_oracle(v, wants, "lean C16", lean=True)
    assert v["ref_max_cov"].tolist() == [int(w["counts"].max()) for w in wants] and set(v["ref_max_cov"].tolist()) == {70_000}
    # ... unless its maximum is 2^32 - 1: ref_max_cov then reads NOT_BARE, and such a target is delivered like one
    # that is not bare, counts and escapes and all
    seqs, wants, all_counts, big = _escape_set(2049)
    sent = np.concatenate([w["counts"] for w in wants if int(w["counts"].max()) == top])
    assert 0 < int((sent >= 0xFFFF).sum()) == 2047 and sum(int(w["counts"].max()) < top for w in wants) == 2
    bt.set_targets(seqs)
    v, sizes, delivered = step(DELIVER | LEAN | C16)
    assert delivered == 1 and sizes.n_count_escapes == 2047 and v["node_count"].size == sent.size
    _check_against_oracle(v, wants, "lean C16, saturated maxima", lean=True)
    assert v["ref_max_cov"].tolist() == [int(w["counts"].max()) for w in wants]
    assert np.array_equal(v["node_count"], sent) and np.array_equal(v["count_esc_value"], sent[sent >= 0xFFFF])
    # native reporting from the view, on both sides of the capacity; fetch() behind a 16-bit step
    for name in (2048, 2049):
        seqs, wants, all_counts, big = _escape_set(name)
        bt.set_targets(seqs)
        v, sizes, delivered = step(DELIVER | C16)
        assert delivered == (1 if name == 2048 else 2) and ("node_count16" in v) == (name == 2048)
        rows = _rows(v, seqs)
        f16 = bt.fetch()                                       # (a full delivery: one more behind a 16-bit one)
        now = _serial(bt)
        assert now - state["serial"] == (1 if name == 2048 else 0), name
        state["serial"] = now
        assert rows == _rows(f16, seqs) and all(isinstance(r, list) and len(r) == 1 for r in rows), name
    v, sizes, delivered = step(DELIVER)
    assert delivered == 1 and "node_count16" not in v
    plain = bt.fetch()
    assert set(plain) == set(f16)
    for key in plain:
        assert np.array_equal(plain[key], f16[key]), key
    assert np.array_equal(plain["node_count"], all_counts)
    bt.close()
    kmlib.stream_destroy(st)
    db.close()


# ---------------------------------------------------------------------------- 2. a tail beyond the guess, beyond the buffer
TAIL_N_REF = 60
N_GUESS, N_BUFFER, N_SMALL = 60, 640, 20


@functools.lru_cache(maxsize=None)
def _tail_world():
    """N_BUFFER targets of 60 k-mers, each with one insertion haplotype in the table that adds 135 .. 160 nodes to the
    walk: two paths and four runs per target, and a tail of some 2 KB each that is mostly walk-discovered k-mers.
    A second table has 2 049 counts of reference k-mers raised to >= 65535 (none of them the reference child at the
    branch, whose sibling starts the insertion: the walks stay what they are).
    -> dict(cases, seqs, keys, counts, wants, hot_counts, hot_wants)"""
    pool = synth.DistinctPool(K, 5302)
    cases = [_feature_case(pool, "ins%d" % i, TAIL_N_REF, [("ins", 105 + (7 * i) % 26)]) for i in range(N_BUFFER)]
    keys, counts = synth.records_from_reads([r for c in cases for r in c["reads"]], K)
    seqs = [c["target"] for c in cases]
    co = c_oracle.COracle(keys, counts, K)
    wants = [co.analyse(km.encode(s)) for s in seqs]
    hot_counts = counts.copy()
    n_hot = 0
    for c in cases:
        kms = km.canonical(km.sliding_kmers(km.encode(c["target"]), K), K)
        branch_child = c["feats"][0][1] - (K - 1)
        for pos in [p for p in range(6) if p != branch_child]:
            if n_hot < 2049:
                at = int(np.searchsorted(keys, kms[pos]))
                assert keys[at] == kms[pos]
                hot_counts[at] = HOT_VALUES[n_hot % 4]
                n_hot += 1
    assert n_hot == 2049
    co = c_oracle.COracle(keys, hot_counts, K)
    hot_wants = [co.analyse(km.encode(s)) for s in seqs]
    return {"cases": cases, "seqs": seqs, "keys": keys, "counts": counts, "wants": wants, "hot_counts": hot_counts,
            "hot_wants": hot_wants}


def _bases(seqs):
    return sum(len(s) for s in seqs)


def test_tail_thresholds_from_the_librarys_arithmetic():
    """Where the tails of the batches below sit: beyond tail_guess and inside the buffer (N_GUESS targets), beyond the
    buffer in both count widths (N_BUFFER), with 2 049 escapes in the second table; no pool group can overflow and
    every target stays in the LDS tier."""
    w = _tail_world()
    wants, hot_wants = w["wants"], w["hot_wants"]
    for x in wants + hot_wants:
        new = len(x["kmers"]) - x["n_ref"]
        assert x["status"] == 0 and x["n_ref"] == TAIL_N_REF and 100 < new <= FAST_EXTRA and len(x["paths"]) == 2
        assert sum(_runs(p) for p in x["paths"]) == 4
    assert [len(x["kmers"]) for x in wants] == [len(x["kmers"]) for x in hot_wants]
    assert {len(x["kmers"]) - x["n_ref"] for x in wants} == set(range(135, 161))
    # beyond the guess, inside the buffer: the second copy of finish_result fetches the rest
    tail, off_rlen, runs = oracle_tail(wants[:N_GUESS])
    guess = lib_tail_guess(wants[:N_GUESS])
    cap = lib_tail_cap(N_GUESS, _bases(w["seqs"][:N_GUESS]), N_GUESS)
    assert guess + 16384 < off_rlen and tail <= cap, (guess, off_rlen, tail, cap)      # (all of run_len is in the second copy)
    # beyond the buffer: nothing is packed, the buffer grows; the 16-bit form does not fit either
    cap = lib_tail_cap(N_BUFFER, _bases(w["seqs"]), N_BUFFER)
    tail32, tail16 = oracle_tail(wants)[0], oracle_tail(hot_wants, count_bytes=2)[0]
    assert tail16 > cap + 4096 and tail32 > tail16, (tail16, tail32, cap)
    # ... and the buffer that is grown for the 16-bit form (9/8 of region A + that tail + 4096) would not hold the 32-bit one
    grown = lib_a_bytes(N_BUFFER) + tail16 + 4096
    assert oracle_tail(hot_wants)[0] > grown + grown // 8 - lib_a_bytes(N_BUFFER)
    all_hot = np.concatenate([x["counts"] for x in hot_wants])
    assert int((all_hot >= 0xFFFF).sum()) == 2049 == _numbers()["esc_cap"] + 1
    assert int((np.concatenate([x["counts"] for x in wants]) >= 0xFFFF).sum()) == 0
    # the small batch beside it in the pump: inside its guess
    assert oracle_tail(wants[:N_SMALL])[0] <= lib_tail_guess(wants[:N_SMALL])
    # pool groups (group = target % 64, graph_kernel.h): a group's share of the pools against what its targets claim
    groups = _numbers()["groups"]
    path_pool, run_pool = lib_pools(N_BUFFER)
    assert _numbers()["path_min"] == 8192 and _numbers()["run_min"] == 32768
    per_group = -(-N_BUFFER // groups)
    assert 2 * per_group <= path_pool // groups and 4 * per_group <= run_pool // groups
    # the LDS tier: the geometry of a batch of these targets holds every walk
    geo = model_geometry(TAIL_N_REF)
    for counts in (w["counts"], w["hot_counts"]):
        table = _table(w["keys"], counts)
        for c in w["cases"][::7]:
            assert model_walk(c["target"], K, table, geo)["cause"] is None, c["name"]


def _delivered(bt, before):
    now = _serial(bt)
    return now, now - before


@gpu
def test_tail_beyond_the_guess_is_fetched_by_the_second_copy():
    w = _tail_world()
    seqs, wants = w["seqs"][:N_GUESS], w["wants"][:N_GUESS]
    tail, off_rlen, runs = oracle_tail(wants)
    db = kmlib.Database.from_records(w["keys"], w["counts"], K).upload(0)
    st = kmlib.stream_create(0)
    bt = kmlib.Batch(db, max_targets=N_GUESS, max_total_bases=_bases(seqs))
    bt.set_targets(seqs)
    serial, first = 0, None
    for i, flags in enumerate((DELIVER, DELIVER, DELIVER | C16, DELIVER | LEAN)):    # (the second: tail_guess has adapted)
        bt.run(flags, st)
        v = _copy(bt.result())
        tot = _totals(bt.result())
        serial, delivered = _delivered(bt, serial)
        assert delivered == 1 and int(tot[OT_NEEDS_HOST]) == 0, i
        if not flags & C16:
            assert int(tot[4]) == tail                         # (OT_TAIL_BYTES)
        _check_against_oracle(v, wants, ("beyond the guess", i), lean=bool(flags & LEAN))
        assert int(bt.wait_result().n_big_tier) == 0
        # run_len sits at the tail's end: all of it came with the second copy
        want_len = [n for x in wants for p in x["paths"] for n in _run_lengths(p)]
        assert v["run_len"].tolist() == want_len and len(want_len) == runs
        assert v["run_len"][-8:].tolist() == want_len[-8:]
        first = first or v
        for key in ("run_start", "run_len", "run_off", "extra_kmer", "node_count", "path_len", "path_min_cov"):
            assert np.array_equal(first[key], v[key]), (i, key)
    bt.close()
    kmlib.stream_destroy(st)
    db.close()


def _run_lengths(path):
    out = [1]
    for a, b in zip(path[:-1], path[1:]):
        if b == a + 1:
            out[-1] += 1
        else:
            out.append(1)
    return out


@gpu
def test_tail_beyond_the_buffer_is_delivered_twice_then_once():
    w = _tail_world()
    db = kmlib.Database.from_records(w["keys"], w["counts"], K).upload(0)
    st = kmlib.stream_create(0)
    bt = kmlib.Batch(db, max_targets=N_BUFFER, max_total_bases=_bases(w["seqs"]))
    bt.set_targets(w["seqs"])
    serial = 0
    for i, want_deliveries in enumerate((2, 1, 1)):
        bt.run(DELIVER, st)
        v = _copy(bt.result())
        tot = _totals(bt.result())
        serial, delivered = _delivered(bt, serial)
        assert delivered == want_deliveries, (i, delivered, "first step: the buffer must have been too small")
        assert int(tot[OT_NEEDS_HOST]) == 0 and int(tot[4]) == oracle_tail(w["wants"])[0]
        assert int(bt.wait_result().n_big_tier) == 0
        _check_against_oracle(v, w["wants"], ("beyond the buffer", i))
    bt.close()
    kmlib.stream_destroy(st)
    db.close()


@gpu
def test_tail_beyond_the_buffer_and_escape_overflow_in_one_step():
    """Three deliveries of one step: the 16-bit form does not fit the buffer (nothing packed, the buffer grows — for the
    32-bit form, which a step whose counts are sent as 16 bits may still need), the 16-bit form overflows its escape
    list, the 32-bit form arrives."""
    w = _tail_world()
    db = kmlib.Database.from_records(w["keys"], w["hot_counts"], K).upload(0)
    st = kmlib.stream_create(0)
    bt = kmlib.Batch(db, max_targets=N_BUFFER, max_total_bases=_bases(w["seqs"]))
    bt.set_targets(w["seqs"])
    bt.run(DELIVER | C16, st)
    v = _copy(bt.result())
    sizes = bt.wait_result()
    serial, delivered = _delivered(bt, 0)
    assert delivered == 3, delivered
    assert "node_count16" not in v and sizes.n_count_escapes == 0 and int(sizes.n_big_tier) == 0
    _check_against_oracle(v, w["hot_wants"], "both at once")
    assert int((v["node_count"] >= 0xFFFF).sum()) == 2049
    bt.run(DELIVER, st)
    v = _copy(bt.result())
    serial, delivered = _delivered(bt, serial)
    assert delivered == 1
    _check_against_oracle(v, w["hot_wants"], "the plain step behind it")
    bt.close()
    kmlib.stream_destroy(st)
    db.close()


@gpu
@pytest.mark.parametrize("pairing", ["paired", "unpaired"])
def test_tail_beyond_the_buffer_through_the_pump(pairing):
    """Two workspaces in flight: the large batch's first delivery does not fit and is repeated inside the pump, beside
    a small batch whose steps go on."""
    w = _tail_world()
    db = kmlib.Database.from_records(w["keys"], w["counts"], K).upload(0)
    streams = [kmlib.stream_create(0), kmlib.stream_create(0)]
    big = kmlib.Batch(db, max_targets=N_BUFFER, max_total_bases=_bases(w["seqs"]))
    small = kmlib.Batch(db, max_targets=N_SMALL, max_total_bases=_bases(w["seqs"][:N_SMALL]))
    big.set_targets(w["seqs"])
    small.set_targets(w["seqs"][:N_SMALL])
    how = kmlib.KM_PUMP_PAIRED if pairing == "paired" else kmlib.KM_PUMP_UNPAIRED
    kmlib.pump([big, small], streams, 4, DELIVER | LEAN | how)
    n_paired = big.paired_steps() + small.paired_steps()
    vb, vs = _copy(big.result()), _copy(small.result())
    assert _serial(big) == 3 and _serial(small) == 2           # two steps each; the large batch's first one twice
    _check_against_oracle(vb, w["wants"], "pump, large", lean=True)
    _check_against_oracle(vs, w["wants"][:N_SMALL], "pump, small", lean=True)
    kmlib.pump([big, small], streams, 2, DELIVER | how)
    assert _serial(big) == 4 and _serial(small) == 3
    _check_against_oracle(_copy(big.result()), w["wants"], "pump again, large")
    _check_against_oracle(_copy(small.result()), w["wants"][:N_SMALL], "pump again, small")
    print("paired steps of the first pump:", n_paired)
    assert n_paired == (3 if pairing == "paired" else 0)        # (k_seed ran as blocks of the other batch's walk launch)
    big.close()
    small.close()
    for s in streams:
        kmlib.stream_destroy(s)
    db.close()


# ---------------------------------------------------------------------------- 4. ranks at 63 .. 129 paths of one target
RANK_CANDIDATES = 24
# (k, seed of the table) -> {paths: which candidate target has that many}; found by a search over seeds 0 .. 599 with
# the C oracle.  The targets of one world share its table, so they run in one batch.
RANK_WORLDS = {(4, 252): {127: 21, 128: 0, 129: 3}, (5, 433): {64: 5, 65: 17}, (5, 503): {63: 21}}
RANK_MOST_PATHS = 160                                          # (more candidate edges than a short batch's ccap: another tier)


@functools.lru_cache(maxsize=None)
def _rank_world(k, seed):
    """A table that holds a random share (5 to 95 %) of all canonical k-mers, counts 30 .. 90 (one child is never
    below 5 % of its siblings' sum), and 24 candidate targets of 15 .. 60 k-mers that are walks inside it without a
    repeated k-mer.  Kept: those the oracle accepts with at most 160 walk-discovered nodes and 160 paths.
    -> dict(keys, counts, seqs, wants, index: candidate number -> place in seqs, causes: None for a target whose
    walk stays in the LDS tier)"""
    rng = np.random.default_rng(seed)
    space = np.arange(1 << (2 * k), dtype=np.uint64)
    rc = km.revcomp(space, k)
    frac = rng.uniform(0.05, 0.95)
    keep = (space <= rc) & (rng.random(space.size) < frac)
    keys = space[keep]
    counts = rng.integers(30, 91, size=keys.size).astype(np.uint32)
    present = np.zeros(space.size, dtype=bool)
    present[keys.astype(np.int64)] = True
    present |= present[rc.astype(np.int64)]
    mask = (1 << (2 * k)) - 1
    starts = np.flatnonzero(present)
    co = c_oracle.COracle(keys, counts, k)
    seqs, wants, index = [], [], {}
    for cand in range(RANK_CANDIDATES):
        n_ref = int(rng.integers(15, 61))
        seq = None
        for _try in range(20):
            x = int(starts[rng.integers(0, starts.size)])
            used = {x}
            codes = [(x >> (2 * (k - 1 - i))) & 3 for i in range(k)]
            while len(used) < n_ref:
                for b in rng.permutation(4).tolist():
                    y = ((x << 2) | b) & mask
                    if present[y] and y not in used:
                        break
                else:
                    break                                      # (a dead end: another start)
                used.add(y)
                codes.append(b)
                x = y
            if len(used) == n_ref:
                seq = "".join("ACGT"[c] for c in codes)
                break
        if seq is None:
            continue
        w = co.analyse(km.encode(seq))
        if w["status"] == 0 and len(w["kmers"]) - w["n_ref"] <= FAST_EXTRA and len(w["paths"]) <= RANK_MOST_PATHS:
            index[cand] = len(seqs)
            seqs.append(seq)
            wants.append(w)
    # which of them the walk's LDS tier hands to the large tier (tests/test_lds_tier_edges.py: the model)
    geo = model_geometry(max(x["n_ref"] for x in wants))
    table = _table(keys, counts)
    causes = [model_walk(s, k, table, geo)["cause"] for s in seqs]
    return {"keys": keys, "counts": counts, "seqs": seqs, "wants": wants, "index": index, "causes": causes}


def test_rank_targets_have_63_to_129_paths():
    """The oracle's number of paths of the pinned targets, asserted here and not taken from a run: 63, 64 and 65 (one
    trip of the ranking loop, its last lane, two trips), 127, 128, 129 (two trips, the last lane of the second, three);
    every target is accepted and adds at most 160 nodes; paths of one target differ in length and share prefixes, and
    some are cut into a dozen runs."""
    seen, most_runs = [], 0
    for (k, seed), pinned in RANK_WORLDS.items():
        w = _rank_world(k, seed)
        for paths, cand in pinned.items():
            x = w["wants"][w["index"][cand]]
            assert x["status"] == 0 and len(x["kmers"]) - x["n_ref"] <= FAST_EXTRA and len(x["paths"]) == paths, (k, seed, cand)
            assert x["paths"] == sorted(x["paths"]) and len({len(p) for p in x["paths"]}) > 3
            seen.append(paths)
        most_runs = max([most_runs] + [_runs(p) for x in w["wants"] for p in x["paths"]])
        assert len(w["seqs"]) > len(pinned)                    # (other targets around the pinned ones)
        assert all(w["causes"][w["index"][cand]] is None for cand in pinned.values())
    assert sorted(seen) == [63, 64, 65, 127, 128, 129]
    assert 8 <= most_runs <= 64                                # (no path here reaches the loops for more than 64 runs)


@gpu
@pytest.mark.parametrize("world", sorted(RANK_WORLDS), ids=lambda x: "k%d_seed%d" % x)
def test_ranks_at_63_64_65_127_128_129_paths(world):
    """Every target of a world in one batch, in two orders, delivered in all four forms: the paths, their order,
    path_len, path_min_cov and run_off are the oracle's."""
    k, seed = world
    w = _rank_world(k, seed)
    db = kmlib.Database.from_records(w["keys"], w["counts"], k).upload(0)
    st = kmlib.stream_create(0)
    n = len(w["seqs"])
    bt = kmlib.Batch(db, max_targets=n, max_total_bases=_bases(w["seqs"]))
    for order in (list(range(n)), list(range(n))[::-1]):
        seqs, wants = [w["seqs"][i] for i in order], [w["wants"][i] for i in order]
        bt.set_targets(seqs)
        want_off = np.concatenate([[0], np.cumsum([_runs(p) for x in wants for p in x["paths"]])])
        for lean in (0, LEAN):
            for c16 in (0, C16):
                bt.run(DELIVER | lean | c16, st)
                v = _copy(bt.result())
                tag = (world, order[0], bool(lean), bool(c16))
                assert int(bt.wait_result().n_big_tier) == sum(c is not None for c in w["causes"]), tag
                _check_against_oracle(v, wants, tag, lean=bool(lean))
                assert np.array_equal(v["run_off"].astype(np.int64), want_off), tag
                assert set(RANK_WORLDS[world]) <= set(np.diff(v["path_off"].astype(np.int64)).tolist()), tag
    bt.close()
    kmlib.stream_destroy(st)
    db.close()
