"""The two ends of a step's launch chain: k_pack zeroes the path-pool counters (no fill command per step), k_out_scan
requests every word of a target at once, k_out_pack requests a single path's record ahead of the count copies and
copies the counts in 16-byte groups.  Results are what they were: every delivery here is checked, target by target,
against the plain-C oracle, at the sizes where those kernels take another path (a wave edge and a block edge of
k_out_scan, more than one scan block, every alignment of a target's counts in the node pool and in the delivery,
counts on the escape list at the first, a middle and the last k-mer)."""
import ctypes as C

import numpy as np
import pytest

from km_amd import kmer as km
from km_amd import lib as kmlib
from km_amd import synth
from oracle import c_oracle

pytestmark = pytest.mark.gpu

K = 31
NOT_BARE = 0xFFFFFFFF
BOTH = kmlib.KM_STAGE_WALK | kmlib.KM_STAGE_GRAPH
DELIVER = BOTH | kmlib.KM_RUN_DELIVER
LEAN = kmlib.KM_DELIVER_LEAN
C16 = kmlib.KM_DELIVER_COUNT16
_ARRAYS = ("status", "n_ref", "probes", "node_off", "extra_off", "path_off", "run_off", "run_start", "run_len",
           "path_len", "path_min_cov", "node_count", "extra_kmer", "ref_max_cov")


def _copy(view):
    return {key: (np.array(val) if isinstance(val, np.ndarray) else val) for key, val in view.items()}


def _oracle(co, seqs):
    """The C oracle's answer per target; a target with a base outside ACGT is rejected before the walk."""
    out = []
    for s in seqs:
        if "N" in s:
            out.append({"status": kmlib.T_BAD_BASE, "kmers": np.zeros(0, np.uint64), "counts": np.zeros(0, np.uint32),
                        "paths": [], "min_cov": [], "probes": None, "n_ref": max(0, len(s) - K + 1)})
        else:
            out.append(co.analyse(km.encode(s)))
    return out


def _check_against_oracle(v, want, tag, lean=False):
    """Every array of a delivery from the oracle's per-target answers: the three CSR offset arrays are the exclusive
    prefix sums of the per-target sizes, the totals (the lengths of the tail arrays) agree with them, and every
    target's counts, walk-discovered k-mers, paths and min coverages are the oracle's."""
    n = len(want)
    ok = np.array([w["status"] == 0 for w in want], dtype=bool)
    assert np.array_equal(np.asarray(v["status"]), np.array([w["status"] for w in want], np.uint32)), tag
    n_ref = np.asarray(v["n_ref"]).astype(np.int64)
    nodes = np.array([len(w["kmers"]) if w["status"] == 0 else 0 for w in want], np.int64)
    paths = np.array([len(w["paths"]) if w["status"] == 0 else 0 for w in want], np.int64)
    extra = np.where(ok, nodes - np.minimum(n_ref, nodes), 0)
    refmax = np.asarray(v["ref_max_cov"])
    bare = refmax != NOT_BARE
    for t in np.nonzero(bare)[0]:
        w = want[t]
        assert ok[t] and extra[t] == 0 and w["paths"] == [list(range(int(n_ref[t])))], (tag, t)
        assert int(refmax[t]) == int(w["counts"].max()), (tag, t)
    sent = np.where(bare, 0, nodes) if lean else nodes
    for key, sizes in (("node_off", sent), ("extra_off", extra), ("path_off", paths)):
        got = np.asarray(v[key]).astype(np.int64)
        assert got.size == n + 1 and np.array_equal(got, np.concatenate([[0], np.cumsum(sizes)])), (tag, key)
    noff, eoff, poff = (np.asarray(v[key]).astype(np.int64) for key in ("node_off", "extra_off", "path_off"))
    roff = np.asarray(v["run_off"]).astype(np.int64)
    assert np.asarray(v["node_count"]).size == noff[-1] and np.asarray(v["extra_kmer"]).size == eoff[-1], tag
    assert np.asarray(v["path_len"]).size == poff[-1] == np.asarray(v["path_min_cov"]).size == roff.size - 1, tag
    assert roff[0] == 0 and roff[-1] == np.asarray(v["run_start"]).size == np.asarray(v["run_len"]).size, tag
    assert (np.diff(roff) >= 1).all(), tag
    for t in range(n):
        w = want[t]
        if w["status"] != 0:
            continue
        assert int(v["probes"][t]) == w["probes"], (tag, t)
        if sent[t]:
            assert np.array_equal(v["node_count"][noff[t]:noff[t + 1]], w["counts"]), (tag, t)
        assert np.array_equal(v["extra_kmer"][eoff[t]:eoff[t + 1]], w["kmers"][int(n_ref[t]):]), (tag, t)
        assert [kmlib.expand_path(v, p).tolist() for p in range(poff[t], poff[t + 1])] == w["paths"], (tag, t)
        assert np.asarray(v["path_min_cov"])[poff[t]:poff[t + 1]].tolist() == w["min_cov"], (tag, t)
        assert np.asarray(v["path_len"])[poff[t]:poff[t + 1]].tolist() == [len(p) for p in w["paths"]], (tag, t)
    if "node_count16" in v:
        assert np.array_equal(np.asarray(v["node_count16"]),
                              np.minimum(np.asarray(v["node_count"]), 0xFFFF).astype(np.uint16)), tag


def _same(a, b, tag):
    for key in _ARRAYS:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (tag, key)


# ---------------------------------------------------------------------------- 1. the counters start every step at zero
OT_NEEDS_HOST, OT_SERIAL = 5, 17          # words of totals[] (csrc/deliver_kernel.h)


def _totals(view):
    """totals[] of the delivery a result() view points into: region A of the delivery buffer starts with its 32 words,
    `status` follows them at byte 256 (csrc/batch_host.h: out_layout)."""
    addr = np.asarray(view["status"]).ctypes.data - 256
    return np.array((C.c_uint64 * 32).from_address(addr), dtype=np.uint64)


def test_pool_counters_are_zeroed_by_the_first_kernel_of_every_step(monkeypatch):
    """One workspace, the same targets, step after step with no set_targets in between: plain launches, a captured
    step and its replay, then a graph-only rerun (which has no k_pack in front and keeps a fill of its own).

    The graph kernels claim their paths through the pool counters.  Counters that are not reset only move every
    t_pathbase on, which no delivery shows, until a pool overflows — and then the host grows the pools, runs the graph
    stage again behind a fill of its own and delivers AGAIN, with the right results.  So the results alone cannot
    tell; the second delivery can: every delivery is stamped with a serial number (totals[OT_SERIAL]) that goes up
    by one per delivery, so a step that was delivered once moves it by exactly one.  The workspace is created with
    the test pools (2 paths and 4 runs per group): the first steps overflow them and the host grows them, fourfold
    each time, until the step fits.  A pool that had to grow to c per group holds a step that uses more than c / 4
    of it, so without a reset the counters pass c after four steps at the most; seven are run."""
    case = synth.make_case(n_targets=300, length=120, n_keys=30_000, seed=5101, variant_frac=0.8,
                           variants_per_target=(1, 2), exact_pad=False)
    seqs = [km.decode(r) for r in case["targets"]]
    db = kmlib.Database.from_records(case["keys"], case["counts"], K).upload(0)
    want = _oracle(c_oracle.COracle(case["keys"], case["counts"], K), seqs)
    assert sum(len(w["paths"]) >= 2 for w in want) >= 36
    st = kmlib.stream_create(0)
    monkeypatch.setenv("KM_TEST_SMALL_POOLS", "1")
    bt = kmlib.Batch(db, max_targets=300, max_total_bases=300 * 120)
    monkeypatch.delenv("KM_TEST_SMALL_POOLS")
    bt.set_targets(seqs)
    # until the pools hold a step: the deliveries of such a step are two or more
    serial, grew = 0, 0
    for settle in range(6):
        bt.run(DELIVER | LEAN, st)
        view = bt.result()
        now = int(_totals(view)[OT_SERIAL])
        first = _copy(view)
        step, serial = now - serial, now
        if step == 1:
            break
        grew += 1
    assert step == 1 and grew >= 1                            # (no growth: the pools were never near full, nothing is tested)
    _check_against_oracle(first, want, "first", lean=True)
    flags = [DELIVER | LEAN] * 3 + [DELIVER | LEAN | kmlib.KM_RUN_HIPGRAPH] * 2 \
        + [kmlib.KM_STAGE_GRAPH | kmlib.KM_RUN_DELIVER | LEAN, DELIVER | LEAN]      # (graph stage alone: no k_pack)
    for i, f in enumerate(flags):
        bt.run(f, st)
        got = bt.result()
        tot = _totals(got)
        assert int(tot[OT_NEEDS_HOST]) == 0, i
        assert int(tot[OT_SERIAL]) == serial + 1, (i, "delivered more than once: a pool overflowed")
        serial += 1
        _same(got, first, ("step", i))
    bt.close()
    kmlib.stream_destroy(st)
    db.close()


# ---------------------------------------------------------------------------- 2. the scan's edges
SCAN_SIZES = [1, 63, 64, 255, 256, 257, 513]


@pytest.fixture(scope="module")
def scan_world():
    """513 targets of 40-80 nt, a fifth of them with a variant; target 5 is shorter than k, target 9 has an N."""
    case = synth.make_case(n_targets=513, length=80, n_keys=20_000, seed=5102, variant_frac=0.4,
                           variants_per_target=(1, 2), exact_pad=False)
    seqs = [km.decode(r)[:40 + (7 * i) % 41] for i, r in enumerate(case["targets"])]
    seqs[0] = km.decode(case["targets"][0])
    seqs[5] = seqs[5][:20]
    seqs[9] = seqs[9][:25] + "N" + seqs[9][26:]
    db = kmlib.Database.from_records(case["keys"], case["counts"], K).upload(0)
    want = _oracle(c_oracle.COracle(case["keys"], case["counts"], K), seqs)
    assert want[5]["status"] == kmlib.T_EMPTY
    assert sum(len(w["paths"]) >= 2 for w in want) >= 20 and sum(len(w["kmers"]) > w["n_ref"] for w in want) >= 20
    yield {"db": db, "seqs": seqs, "want": want}
    db.close()


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_offsets_at_wave_and_block_edges(scan_world, n):
    seqs, want = scan_world["seqs"][:n], scan_world["want"][:n]
    st = kmlib.stream_create(0)
    bt = kmlib.Batch(scan_world["db"], max_targets=513, max_total_bases=513 * 80)
    bt.set_targets(seqs)
    n_bare = 0
    for lean in (0, LEAN):
        for c16 in (0, C16):
            bt.run(DELIVER | lean | c16, st)
            v = bt.result()
            assert ("node_count16" in v) == bool(c16), (n, lean, c16)
            _check_against_oracle(v, want, (n, bool(lean), bool(c16)), lean=bool(lean))
            n_bare = int((np.asarray(v["ref_max_cov"]) != NOT_BARE).sum())
    if n >= 63:
        assert 0 < n_bare < n                                  # lean delivery omits some targets' counts, not all
    bt.close()
    kmlib.stream_destroy(st)


# ---------------------------------------------------------------------------- 3. the wide copies
def test_counts_at_every_alignment_and_on_the_escape_list():
    """Consecutive targets of 2 .. 10 k-mers (k + 1 .. k + 9 bases), four rounds of them: a target's counts start at
    every residue mod 4 both in the node pool and in node_count, with 0 to 2 whole 16-byte groups between 0 to 3
    elements on either side; two long targets run the two-groups-in-flight loop more than once.  A short and a long
    target carry a count >= 65535 on their first, a middle and their last k-mer."""
    case = synth.make_case(n_targets=38, length=620, n_keys=30_000, seed=5103, variant_frac=0.5, exact_pad=False)
    rows = case["targets"]
    lengths = [K + 1 + i % 9 for i in range(36)] + [300, 620]
    seqs = [km.decode(r)[:L] for r, L in zip(rows, lengths)]
    keys, counts = case["keys"].copy(), case["counts"].copy()
    order = np.argsort(keys)
    hot = {}
    for t in (7, 36):                                          # 9 k-mers; 270 k-mers
        n_ref = lengths[t] - K + 1
        kms = km.canonical(km.sliding_kmers(km.encode(seqs[t]), K), K)
        for pos, value in ((0, 65_535), (n_ref // 2, 70_000), (n_ref - 1, 3_000_000)):
            at = order[np.searchsorted(keys[order], kms[pos])]
            assert keys[at] == kms[pos]
            counts[at] = value
            hot[(t, pos)] = value
    db = kmlib.Database.from_records(keys, counts, K).upload(0)
    want = _oracle(c_oracle.COracle(keys, counts, K), seqs)
    assert all(w["status"] == 0 for w in want)
    for (t, pos), value in hot.items():
        assert int(want[t]["counts"][pos]) == value
    st = kmlib.stream_create(0)
    bt = kmlib.Batch(db, max_targets=38, max_total_bases=sum(lengths))
    bt.set_targets(seqs)
    bt.run(DELIVER, st)
    v = _copy(bt.result())
    _check_against_oracle(v, want, "32-bit")
    noff = v["node_off"].astype(np.int64)
    n_ref = v["n_ref"].astype(np.int64)
    assert {int(x) % 4 for x in noff[:36]} == {0, 1, 2, 3}
    # where a target's counts start in the node pool: behind the storage of the targets before it, which is their
    # k-mers + the same allowance of walk-discovered nodes each — every residue mod 4, whatever that allowance is
    for slack in range(4):
        assert {int(slack * t + n_ref[:t].sum()) % 4 for t in range(36)} == {0, 1, 2, 3}, slack
    bt.run(DELIVER | C16, st)
    v16 = _copy(bt.result())
    assert "node_count16" in v16
    _check_against_oracle(v16, want, "16-bit")
    _same(v16, v, "16-bit against 32-bit")
    all_counts = np.concatenate([w["counts"] for w in want])
    big = np.nonzero(all_counts >= 0xFFFF)[0]
    assert set(int(noff[t] + pos) for (t, pos) in hot) <= set(big.tolist())
    esc = sorted(zip(v16["count_esc_node"].tolist(), v16["count_esc_value"].tolist()))
    assert esc == [(int(i), int(all_counts[i])) for i in big]
    assert (v16["node_count16"][big] == 0xFFFF).all()
    bt.run(DELIVER | LEAN | C16, st)
    _check_against_oracle(bt.result(), want, "lean 16-bit", lean=True)
    bt.close()
    kmlib.stream_destroy(st)
    db.close()


# ---------------------------------------------------------------------------- 4. the empty batch
def test_empty_batch_behind_a_full_one(scan_world):
    st = kmlib.stream_create(0)
    bt = kmlib.Batch(scan_world["db"], max_targets=513, max_total_bases=513 * 80)
    bt.set_targets(scan_world["seqs"][:100])
    bt.run(DELIVER | LEAN | C16, st)
    _check_against_oracle(bt.result(), scan_world["want"][:100], "before", lean=True)
    bt.set_targets([])
    for flags in (DELIVER, DELIVER | LEAN | C16):
        bt.run(flags, st)
        v = bt.result()
        assert np.asarray(v["status"]).size == 0 and np.asarray(v["node_count"]).size == 0
        assert np.asarray(v["node_off"]).tolist() == [0] and np.asarray(v["extra_off"]).tolist() == [0]
        assert np.asarray(v["path_off"]).tolist() == [0] and np.asarray(v["path_len"]).size == 0
    bt.set_targets(scan_world["seqs"][:100])
    bt.run(DELIVER, st)
    _check_against_oracle(bt.result(), scan_world["want"][:100], "after")
    bt.close()
    kmlib.stream_destroy(st)
