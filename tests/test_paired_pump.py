"""km_batch_pump pairs consecutive steps: k_seed of the next batch runs as single-wave blocks of the previous batch's
walk launch (graph_kernel.h: k_dfs_pure_seed, walk_kernel.h: seed_body).  Paired steps run on two streams the pump
takes for itself: k_pack and the paired launches on one, the back and the delivery of every step on the other, behind
an event.  KM_PUMP_UNPAIRED selects km_batch_run's own sequence, on the batch's stream, for every step.  By default
the pump pairs a step only where that pays (at most 4 batches, a lean delivery, seed blocks of the next batch for two
rounds of the device); the batches here are small, so the cases ask for every possible pair with KM_PUMP_PAIRED, and
the last case pins the default.

Every case pumps the same batches both ways in one process and compares every array of a full delivery (result(),
32-bit counts) and every field of sizes(), batch by batch; a sample of targets is checked against the plain-C oracle.
Batch.paired_steps() tells how many of a pump's steps really were paired."""
import numpy as np
import pytest

from km_amd import kmer as km
from km_amd import lib as kmlib
from km_amd import synth
from oracle import c_oracle

pytestmark = pytest.mark.gpu

BOTH = kmlib.KM_STAGE_WALK | kmlib.KM_STAGE_GRAPH
FULL = BOTH | kmlib.KM_RUN_DELIVER
_SIZE_FIELDS = ("n_targets", "n_paths", "n_nodes", "n_runs", "logical_probes", "table_fetches", "n_big_tier",
                "n_flagged", "seed_probes", "n_extra", "n_count_escapes")


def _merge(tables):
    """One table over several (keys, counts): the first one that has a key gives its count."""
    keys, first = np.unique(np.concatenate([t[0] for t in tables]), return_index=True)
    return keys, np.concatenate([t[1] for t in tables])[first]


def _seqs(case):
    return [km.decode(r) for r in case["targets"]]


def _batch(db, seqs, **prm):
    b = kmlib.Batch(db, max_targets=max(1, len(seqs)), max_total_bases=max(64, sum(len(s) for s in seqs)), **prm)
    b.set_targets(seqs)
    return b


def _snapshot(b):
    """Copies of every array of the delivery that is there (a full one), and every field of sizes()."""
    r = {key: np.array(val) for key, val in b.result().items()}
    s = b.sizes()
    r["_sizes"] = {f: int(getattr(s, f)) for f in _SIZE_FIELDS}
    return r


def _same(got, want, ctx):
    assert sorted(got) == sorted(want), ctx
    for key in want:
        if key == "_sizes":
            assert got[key] == want[key], (ctx, key, got[key], want[key])
        else:
            assert np.array_equal(got[key], want[key]), (ctx, key)


def _alone(b, flags=FULL):
    b.run(flags)
    return _snapshot(b)


def _pump_both_ways(batches, streams, steps, ctx, flags=FULL, paired_steps=None):
    """`steps` steps paired (KM_PUMP_PAIRED), then the same with KM_PUMP_UNPAIRED: the paired results of the batches that ran, after
    comparing the two.  `paired_steps`: how many steps of the first pump must have been paired (None: steps - 1)."""
    ran = min(len(batches), steps)
    before = sum(b.paired_steps() for b in batches)
    kmlib.pump(batches, streams, steps, flags | kmlib.KM_PUMP_PAIRED)
    paired = [_snapshot(b) for b in batches[:ran]]
    n_paired = sum(b.paired_steps() for b in batches) - before
    assert n_paired == (max(0, steps - 1) if paired_steps is None else paired_steps), (ctx, n_paired)
    kmlib.pump(batches, streams, steps, flags | kmlib.KM_PUMP_UNPAIRED)
    assert sum(b.paired_steps() for b in batches) == before + n_paired, ctx
    for q in range(ran):
        _same(paired[q], _snapshot(batches[q]), (ctx, "paired vs unpaired", q))
    return paired


def _against_oracle(b, r, co, seqs, which, ctx, **prm):
    """`r`: the snapshot of b's delivery; the node k-mers come from fetch() (the same delivery, copied)."""
    f = b.fetch()
    for key in ("status", "node_off", "node_count", "path_off", "path_min_cov", "probes"):
        assert np.array_equal(f[key], r[key]), (ctx, key)
    noff, poff = f["node_off"].astype(np.int64), f["path_off"].astype(np.int64)
    for t in which:
        if set(seqs[t]) - set("ACGTacgt"):
            assert int(f["status"][t]) == kmlib.T_BAD_BASE and poff[t + 1] == poff[t], (ctx, t)
            continue
        want = co.analyse(km.encode(seqs[t]), **prm)
        assert int(f["status"][t]) == want["status"], (ctx, t)
        if want["status"] != kmlib.T_OK:
            assert poff[t + 1] == poff[t], (ctx, t)
            continue
        assert np.array_equal(f["node_kmer"][noff[t]:noff[t + 1]], want["kmers"]), (ctx, t)
        assert np.array_equal(f["node_count"][noff[t]:noff[t + 1]], want["counts"]), (ctx, t)
        assert int(f["probes"][t]) == want["probes"], (ctx, t)
        assert [kmlib.expand_path(f, p).tolist() for p in range(poff[t], poff[t + 1])] == want["paths"], (ctx, t)
        assert f["path_min_cov"][poff[t]:poff[t + 1]].tolist() == want["min_cov"], (ctx, t)
        bare = int(r["ref_max_cov"][t]) != 0xFFFFFFFF
        assert not bare or (len(want["paths"]) == 1 and int(r["ref_max_cov"][t]) == int(want["counts"].max())), (ctx, t)


@pytest.fixture
def pool_streams():
    sts = [kmlib.stream_create(0) for _ in range(4)]
    yield sts
    for st in sts:
        kmlib.stream_destroy(st)


# ------------------------------------------------------------------ item and wave edges of the seed body
EDGE_NREF = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 470, 513)
EDGE_SEEDS = (0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 193, 254, 255, 256, 257, 300, 319, 320, 447, 448, 510, 511)


def _edge_case(k):
    """Per n_ref of EDGE_NREF a plain target and one whose reads carry a substitution behind the seeds of EDGE_SEEDS
    that it has (seed i is flagged by a substitution of base i + k): a variant inside the first and the last 64
    seeds of every item, at both ends of every wave.  One target shorter than k, one with an N, and a mixed case
    around them whose table is the padding."""
    rng = np.random.default_rng(7100 + k)
    base = synth.make_case(n_targets=40, length=300, k=k, n_keys=50_000, seed=7101 + k, variant_frac=0.4, exact_pad=False)
    seqs, tables, edge_ids = _seqs(base), [(base["keys"], base["counts"])], []
    for n_ref in EDGE_NREF:
        for with_variants in (False, True):
            T = synth.unique_kmer_seq(rng, n_ref + k - 1, k)
            reads = [(T, 60)]
            if with_variants:
                for i in EDGE_SEEDS:
                    p = i + k
                    if p < len(T):
                        reads.append((T[:p] + "ACGT"[("ACGT".index(T[p]) + 1 + i % 3) % 4] + T[p + 1:], 25))
            tables.append(synth.records_from_reads(reads, k))
            edge_ids.append(len(seqs))
            seqs.append(T)
    edge_ids += [len(seqs), len(seqs) + 1]
    seqs.append("ACGTTGCA" * 2 + "ACG")                     # 19 bases: no k-mer at k = 21 or 31
    seqs.append(seqs[3][:150] + "N" + seqs[3][151:])
    keys, counts = _merge(tables)
    return keys, counts, seqs, edge_ids


@pytest.mark.parametrize("k", [31, 21])
def test_item_and_wave_edges_of_the_seed_body(k, pool_streams):
    keys, counts, seqs, edge_ids = _edge_case(k)
    db = kmlib.Database.from_records(keys, counts, k).upload(0)
    other = synth.make_case(n_targets=64, length=200, k=k, n_keys=1_000, seed=7150 + k, variant_frac=0.0, exact_pad=False)
    a, b = _batch(db, _seqs(other)), _batch(db, seqs)
    want = _alone(b)
    got = _pump_both_ways([a, b], pool_streams[:2], 4, ("edges", k))
    _same(got[1], want, ("edges", k, "pumped vs alone"))
    flagged = int(np.count_nonzero(got[1]["ref_max_cov"][edge_ids] == 0xFFFFFFFF))
    assert flagged >= len(EDGE_NREF) - 2, flagged            # (n_ref = 1 has no seed with a successor)
    st = got[1]["status"]
    assert int(st[edge_ids[-2]]) == kmlib.T_EMPTY and int(st[edge_ids[-1]]) == kmlib.T_BAD_BASE
    co = c_oracle.COracle(keys, counts, k)
    _against_oracle(b, got[1], co, seqs, edge_ids[:-2] + edge_ids[-1:] + list(range(0, 40, 5)), ("edges", k))
    a.close()
    b.close()
    db.close()


# ------------------------------------------------------------------ ends of the pump
@pytest.fixture(scope="module")
def mixed_db():
    """One table, four target sets of 1, 64, 300 and 150 targets of it, and what each gives when run alone."""
    case = synth.make_case(n_targets=515, length=300, k=31, n_keys=50_000, seed=7200, variant_frac=0.4, exact_pad=False)
    db = kmlib.Database.from_records(case["keys"], case["counts"], 31).upload(0)
    seqs = _seqs(case)
    sets = [seqs[0:1], seqs[1:65], seqs[65:365], seqs[365:515]]
    want = []
    for s in sets:
        b = _batch(db, s)
        want.append(_alone(b))
        b.close()
    yield db, case, sets, want
    db.close()


@pytest.mark.parametrize("n", [2, 3, 4])
def test_ends_of_the_pump(n, mixed_db, pool_streams):
    db, case, sets, want = mixed_db
    batches = [_batch(db, s) for s in sets[:n]]
    co = c_oracle.COracle(case["keys"], case["counts"], 31)
    for steps in (1, 2, n, n + 1, 2 * n + 1):
        got = _pump_both_ways(batches, pool_streams[:n], steps, ("ends", n, steps))
        for q, r in enumerate(got):
            _same(r, want[q], ("ends", n, steps, "pumped vs alone", q))
    _against_oracle(batches[1], got[1], co, sets[1], range(0, 64, 4), ("ends", n))
    for b in batches:
        b.close()


def test_pump_on_the_null_stream_and_on_one_stream(mixed_db, pool_streams):
    """Every batch on the same stream (no event wait is needed: one queue orders everything), the null stream included."""
    db, _case, sets, want = mixed_db
    batches = [_batch(db, s) for s in sets[1:4]]
    for streams in ([None] * 3, [pool_streams[0]] * 3):
        got = _pump_both_ways(batches, streams, 7, ("one stream", streams[0] is None))
        for q, r in enumerate(got):
            _same(r, want[1 + q], ("one stream", q))
    for b in batches:
        b.close()


# ------------------------------------------------------------------ fallbacks give the same arrays
def test_two_k_in_one_pump(pool_streams):
    """Batches of k = 31, 31, 21, 21: the steps 31 -> 31 and 21 -> 21 are paired, 31 -> 21 and 21 -> 31 are not."""
    c31 = synth.make_case(n_targets=120, length=300, k=31, n_keys=50_000, seed=7301, variant_frac=0.4, exact_pad=False)
    c21 = synth.make_case(n_targets=120, length=300, k=21, n_keys=50_000, seed=7302, variant_frac=0.4, exact_pad=False)
    db31 = kmlib.Database.from_records(c31["keys"], c31["counts"], 31).upload(0)
    db21 = kmlib.Database.from_records(c21["keys"], c21["counts"], 21).upload(0)
    s31, s21 = _seqs(c31), _seqs(c21)
    batches = [_batch(db31, s31[:60]), _batch(db31, s31[60:]), _batch(db21, s21[:60]), _batch(db21, s21[60:])]
    want = [_alone(b) for b in batches]
    got = _pump_both_ways(batches, pool_streams, 9, "two k", paired_steps=4)
    for q, r in enumerate(got):
        _same(r, want[q], ("two k", q))
    _against_oracle(batches[3], got[3], c_oracle.COracle(c21["keys"], c21["counts"], 21), s21[60:], range(0, 60, 6), "two k")
    for b in batches:
        b.close()
    db31.close()
    db21.close()


def test_two_tables_of_one_k(pool_streams):
    """Each role of the launch reads its own batch's table."""
    cases = [synth.make_case(n_targets=100, length=260, k=21, n_keys=50_000, seed=7310 + i, variant_frac=0.4,
                             exact_pad=False) for i in range(2)]
    dbs = [kmlib.Database.from_records(c["keys"], c["counts"], 21).upload(0) for c in cases]
    batches = [_batch(db, _seqs(c)) for db, c in zip(dbs, cases)]
    want = [_alone(b) for b in batches]
    got = _pump_both_ways(batches, pool_streams[:2], 5, "two tables")
    for q, r in enumerate(got):
        _same(r, want[q], ("two tables", q))
        _against_oracle(batches[q], r, c_oracle.COracle(cases[q]["keys"], cases[q]["counts"], 21), _seqs(cases[q]),
                        range(0, 100, 10), ("two tables", q))
    for x in batches + dbs:
        x.close()


def test_batch_whose_walk_keeps_two_launches(pool_streams):
    """A longest target of 512 k-mers: k_dfs and k_graph_pure of that batch are two launches (batch_host.h:
    fuses_pure), so it takes no other batch's seeds into its walk launch — but its own seeds still run in the
    launch of the batch before it."""
    k = 31
    long_ = synth.make_case(n_targets=60, length=512 + k - 1, k=k, n_keys=40_000, seed=7320, variant_frac=0.5, exact_pad=False)
    short = synth.make_case(n_targets=120, length=300, k=k, n_keys=10_000, seed=7321, variant_frac=0.4, exact_pad=False)
    keys, counts = _merge([(long_["keys"], long_["counts"]), (short["keys"], short["counts"])])
    db = kmlib.Database.from_records(keys, counts, k).upload(0)
    ss = _seqs(short)
    batches = [_batch(db, _seqs(long_)), _batch(db, ss[:60]), _batch(db, ss[60:])]
    want = [_alone(b) for b in batches]
    # steps L S1 S2 L S1 S2 L: paired are S1 -> S2 and S2 -> L, twice
    got = _pump_both_ways(batches, pool_streams[:3], 7, "two launches", paired_steps=4)
    for q, r in enumerate(got):
        _same(r, want[q], ("two launches", q))
    _against_oracle(batches[0], got[0], c_oracle.COracle(keys, counts, k), _seqs(long_), range(0, 60, 6), "two launches")
    for b in batches:
        b.close()
    db.close()


def test_batches_without_items_and_without_targets(mixed_db, pool_streams):
    """A batch none of whose targets has a k-mer (no k_seed work item) and a batch of zero targets among ordinary ones:
    neither takes part in a paired launch as the seeded one, the empty one not at all."""
    db, _case, sets, want = mixed_db
    none_valid = ["ACGTAC" * 4, "TTGCA" * 5, "ACG"]
    batches = [_batch(db, sets[1]), _batch(db, none_valid), _batch(db, sets[3]), _batch(db, []), _batch(db, sets[2])]
    alone = [_alone(b) for b in batches]
    _same(alone[0], want[1], "alone")
    # steps A N C E B | A N C E B | A: A -> N no (nothing to seed), N -> C paired, C -> E no, E -> B no, B -> A paired
    got = _pump_both_ways(batches, pool_streams + [pool_streams[0]], 11, "no items", paired_steps=4)
    for q, r in enumerate(got):
        _same(r, alone[q], ("no items", q))
    assert (got[1]["status"] == kmlib.T_EMPTY).all() and got[3]["_sizes"]["n_targets"] == 0
    for b in batches:
        b.close()


def test_count_fetches_is_not_paired(mixed_db, pool_streams):
    db, _case, sets, want = mixed_db
    batches = [_batch(db, sets[1]), _batch(db, sets[3])]
    flags = FULL | kmlib.KM_RUN_COUNT_FETCHES
    alone = [_alone(b, flags) for b in batches]
    got = _pump_both_ways(batches, pool_streams[:2], 5, "fetches", flags=flags, paired_steps=0)
    for q, r in enumerate(got):
        _same(r, alone[q], ("fetches", q))
        assert r["_sizes"]["table_fetches"] > 0
    plain = dict(got[0], table_fetches=np.array(0), _sizes=dict(got[0]["_sizes"], table_fetches=0))
    _same(plain, want[1], "fetches vs plain")
    for b in batches:
        b.close()


# ------------------------------------------------------------------ extremes of the split
def test_every_target_flagged_and_none(pool_streams):
    cases = [synth.make_case(n_targets=150, length=300, k=31, n_keys=50_000, seed=7400 + i, variant_frac=vf, vaf=(0.3, 0.6),
                             exact_pad=False) for i, vf in enumerate((1.0, 0.0, 1.0))]
    keys, counts = _merge([(c["keys"], c["counts"]) for c in cases])
    db = kmlib.Database.from_records(keys, counts, 31).upload(0)
    batches = [_batch(db, _seqs(c)) for c in cases]
    want = [_alone(b) for b in batches]
    got = _pump_both_ways(batches, pool_streams[:3], 7, "extremes")
    for q, r in enumerate(got):
        _same(r, want[q], ("extremes", q))
    assert got[0]["_sizes"]["n_flagged"] > 140 and got[1]["_sizes"]["n_flagged"] == 0 and got[2]["_sizes"]["n_flagged"] > 140
    co = c_oracle.COracle(keys, counts, 31)
    for q in range(3):
        _against_oracle(batches[q], got[q], co, _seqs(cases[q]), range(0, 150, 15), ("extremes", q))
    for b in batches:
        b.close()
    db.close()


# ------------------------------------------------------------------ large tier
def test_large_tier_batch_paired_with_a_plain_one(pool_streams, monkeypatch):
    """Targets with three to five tandem duplications, and four with an insertion of 170 bases (200 new nodes: more
    than the LDS tier keeps); the device's own large tier (armed from the first run) finishes what outgrows the LDS
    tier in two more launches of the step's back, behind the paired launch."""
    k = 31
    rng = np.random.default_rng(7502)
    heavy = synth.make_case(n_targets=80, length=300, k=k, n_keys=50_000, seed=7500, variant_frac=0.5, heavy_frac=0.3,
                            exact_pad=False)
    plain = synth.make_case(n_targets=120, length=300, k=k, n_keys=10_000, seed=7501, variant_frac=0.4, exact_pad=False)
    tables = [(heavy["keys"], heavy["counts"]), (plain["keys"], plain["counts"])]
    heavy_seqs = _seqs(heavy)
    for j in range(4):
        T = synth.unique_kmer_seq(rng, 300, k)
        tables.append(synth.records_from_reads([(T, 60), (T[:80] + synth.random_seq(rng, 170) + T[80:], 30)], k))
        heavy_seqs.insert(20 * j + 3, T)
    keys, counts = _merge(tables)
    db = kmlib.Database.from_records(keys, counts, k).upload(0)
    monkeypatch.setenv("KM_BIG_DEVICE", "1")                 # (read at every km_batch_create)
    batches = [_batch(db, heavy_seqs), _batch(db, _seqs(plain))]
    want = [_alone(b) for b in batches]
    assert want[0]["_sizes"]["n_big_tier"] >= 4 and want[1]["_sizes"]["n_big_tier"] == 0
    got = _pump_both_ways(batches, pool_streams[:2], 5, "large tier")
    for q, r in enumerate(got):
        _same(r, want[q], ("large tier", q))
    _against_oracle(batches[0], got[0], c_oracle.COracle(keys, counts, k), heavy_seqs, range(3, 84, 4), "large tier")
    for b in batches:
        b.close()
    db.close()


# ------------------------------------------------------------------ reuse
def test_batches_are_reusable_after_a_paired_pump(mixed_db, pool_streams):
    """What a paired pump leaves in a batch — the stream of its last commands, a delivery awaited, an event recorded —
    does not show in a run of the batch alone, on its stream or another, nor in a second paired pump."""
    db, _case, sets, want = mixed_db
    batches = [_batch(db, s) for s in sets[1:4]]
    streams = pool_streams[:3]
    kmlib.pump(batches, streams, 7, FULL | kmlib.KM_PUMP_PAIRED)
    assert sum(b.paired_steps() for b in batches) == 6
    for q, b in enumerate(batches):
        b.run(FULL, streams[(q + 1) % 3])
        _same(_snapshot(b), want[1 + q], ("alone after", q))
        b.run(BOTH)
        _same(_snapshot(b), want[1 + q], ("alone after, delivered on demand", q))
    got = _pump_both_ways(batches, streams, 8, "second pump")
    for q, r in enumerate(got):
        _same(r, want[1 + q], ("second pump", q))
    lean = FULL | kmlib.KM_DELIVER_LEAN | kmlib.KM_DELIVER_COUNT16 | kmlib.KM_PUMP_PAIRED
    kmlib.pump(batches, streams, 6, lean)
    assert sum(b.paired_steps() for b in batches) == 6 + 7 + 5
    for q, b in enumerate(batches):
        assert np.array_equal(np.array(b.result()["ref_max_cov"]), want[1 + q]["ref_max_cov"])
        full = b.fetch()
        for key in ("status", "node_off", "node_count", "path_off", "path_len", "path_min_cov", "probes"):
            assert np.array_equal(full[key], got[q][key]), (q, key)
        b.close()


# ------------------------------------------------------------------ a walk grid larger than the device
def test_walk_grid_larger_than_the_device_is_not_paired(pool_streams):
    """A batch takes another's seeds into its walk launch only if its walk blocks are all resident at once (16 waves per
    compute unit).  The grid of a batch that has delivered nothing yet is its target count: 6 000 blocks, more than any
    device of today holds (375 compute units would), so no step of the first pump is paired.  The deliveries report
    no flagged target, the grid shrinks to 64 blocks, and the next pump pairs every step but its first."""
    case = synth.make_case(n_targets=12_000, length=80, k=31, n_keys=20_000, seed=7600, variant_frac=0.0, exact_pad=False)
    db = kmlib.Database.from_records(case["keys"], case["counts"], 31).upload(0)
    seqs = _seqs(case)
    batches = [_batch(db, seqs[:6_000]), _batch(db, seqs[6_000:])]
    first = _pump_both_ways(batches, pool_streams[:2], 3, "large grid", paired_steps=0)
    again = _pump_both_ways(batches, pool_streams[:2], 3, "small grid", paired_steps=2)
    for q in range(2):
        assert first[q]["_sizes"]["n_flagged"] == 0
        _same(again[q], first[q], ("large grid", q))
    _against_oracle(batches[0], again[0], c_oracle.COracle(case["keys"], case["counts"], 31), seqs[:6_000],
                    range(0, 6_000, 600), "large grid")
    for b in batches:
        b.close()
    db.close()


# ------------------------------------------------------------------ what the pump pairs by default
def test_default_pairs_only_where_it_pays(pool_streams):
    """Without KM_PUMP_PAIRED a step is paired only if the pump has at most 4 batches, the delivery is lean and the next
    batch has two seed blocks (one per target here: 30 k-mers each) for each of the device's 16 wave slots per compute
    unit: 20 000 blocks are enough for up to 625 compute units, 300 are not for any.  Both flags together: unpaired."""
    case = synth.make_case(n_targets=40_300, length=60, k=31, n_keys=20_000, seed=7700, variant_frac=0.0, exact_pad=False)
    db = kmlib.Database.from_records(case["keys"], case["counts"], 31).upload(0)
    seqs = _seqs(case)
    big = [_batch(db, seqs[:20_000]), _batch(db, seqs[20_000:40_000])]
    small = [_batch(db, seqs[40_000 + 100 * i:40_100 + 100 * i]) for i in range(3)]
    lean = FULL | kmlib.KM_DELIVER_LEAN | kmlib.KM_DELIVER_COUNT16

    def paired_by(batches, steps, flags):
        streams = [pool_streams[q % 4] for q in range(len(batches))]
        before = sum(b.paired_steps() for b in batches)
        kmlib.pump(batches, streams, steps, flags)
        return sum(b.paired_steps() for b in batches) - before, [_snapshot(b) for b in batches]

    # (the walk grid of a batch that has delivered nothing yet is its target count, more than the device holds at once)
    _n, want_big = paired_by(big, 2, lean | kmlib.KM_PUMP_UNPAIRED)
    _n, want_small = paired_by(small, 3, lean | kmlib.KM_PUMP_UNPAIRED)
    assert all(w["_sizes"]["n_flagged"] == 0 for w in want_big + want_small)
    n_paired, got = paired_by(big, 5, lean)
    assert n_paired == 4
    for q in range(2):
        _same(got[q], want_big[q], ("default", q))
    assert paired_by(big, 5, FULL)[0] == 0                                        # a full delivery
    assert paired_by(big, 5, lean | kmlib.KM_PUMP_PAIRED | kmlib.KM_PUMP_UNPAIRED)[0] == 0
    assert paired_by(small, 7, lean)[0] == 0                                      # too few seeds
    assert paired_by(small, 7, lean | kmlib.KM_PUMP_PAIRED)[0] == 6
    # big small big small big: only the steps small -> big are paired
    n_paired, got = paired_by([big[0], small[0]], 5, lean)
    assert n_paired == 2
    _same(got[0], want_big[0], "default, mixed: big")
    _same(got[1], want_small[0], "default, mixed: small")
    # five batches in flight: none, although big[0] -> big[1] could be
    assert paired_by(big + small, 11, lean)[0] == 0
    assert paired_by(big + small[:2], 9, lean)[0] == 4                            # four: big[0] -> big[1] and small[1] -> big[0], twice each
    for b in big + small:
        b.close()
    db.close()
