"""The paired pump's streams and block order (round 8): k_pack of the next batch runs on a third stream of the pump,
the front, beside the paired launch — the chain waits for an event behind it —, and the paired launch holds its seed
blocks in front of its pure-chain blocks (km_amd/csrc/pair_roles.h).  KM_PUMP_FRONT=0 and KM_PAIR_PURE_LAST=0 select
round 7's arrangement of either; the knobs are read once per process, so those arrangements run in child processes.

Every case pumps the same batches paired (KM_PUMP_PAIRED: the batches are far below the default's seed count) and with
KM_PUMP_UNPAIRED in one process, with the lean 16-bit delivery the pump pairs by default, and compares every array of
that delivery, every array of the full delivery fetched afterwards and every field of sizes(), batch by batch.  Batches
have 8-300 targets of 40-500 nt."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from km_amd import kmer as km  # noqa: E402
from km_amd import lib as kmlib  # noqa: E402
from km_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

K = 31
BOTH = kmlib.KM_STAGE_WALK | kmlib.KM_STAGE_GRAPH
FULL = BOTH | kmlib.KM_RUN_DELIVER
LEAN = FULL | kmlib.KM_DELIVER_LEAN | kmlib.KM_DELIVER_COUNT16
_SIZE_FIELDS = ("n_targets", "n_paths", "n_nodes", "n_runs", "logical_probes", "table_fetches", "n_big_tier",
                "n_flagged", "seed_probes", "n_extra", "n_count_escapes")


# ------------------------------------------------------------------ helpers
def _cut(case, lengths):
    """The case's targets as strings, target i cut to lengths[i % len(lengths)] bases."""
    return [km.decode(r)[:lengths[i % len(lengths)]] for i, r in enumerate(case["targets"])]


def _merge(cases):
    keys, first = np.unique(np.concatenate([c["keys"] for c in cases]), return_index=True)
    return keys, np.concatenate([c["counts"] for c in cases])[first]


def _batch(db, seqs, max_targets=None, max_bases=None):
    b = kmlib.Batch(db, max_targets=max_targets or max(1, len(seqs)),
                    max_total_bases=max_bases or max(64, sum(len(s) for s in seqs)))
    b.set_targets(seqs)
    return b


def _snapshot(b):
    """Copies of every array of the delivery that is there (lean after a lean pump), then of the full delivery that
    sizes() brings, and every field of sizes()."""
    first = {key: np.array(val) for key, val in b.result().items()}
    s = b.sizes()
    full = {key: np.array(val) for key, val in b.result().items()}
    return {"first": first, "full": full, "sizes": {f: int(getattr(s, f)) for f in _SIZE_FIELDS}}


def _same(got, want, ctx):
    assert got["sizes"] == want["sizes"], (ctx, got["sizes"], want["sizes"])
    for part in ("first", "full"):
        assert sorted(got[part]) == sorted(want[part]), (ctx, part)
        for key in want[part]:
            assert np.array_equal(got[part][key], want[part][key]), (ctx, part, key)


def _alone(b, flags=LEAN):
    b.run(flags)
    return _snapshot(b)


def _pump_both_ways(batches, streams, steps, ctx, flags=LEAN, paired_steps=None):
    """`steps` steps paired, then the same unpaired; returns the paired snapshots of the batches that ran after comparing
    the two.  `paired_steps`: how many steps of the first pump must have been paired (None: steps - 1)."""
    ran = min(len(batches), steps)
    before = sum(b.paired_steps() for b in batches)
    kmlib.pump(batches, streams, steps, flags | kmlib.KM_PUMP_PAIRED)
    n_paired = sum(b.paired_steps() for b in batches) - before
    assert n_paired == (max(0, steps - 1) if paired_steps is None else paired_steps), (ctx, n_paired)
    paired = [_snapshot(b) for b in batches[:ran]]
    kmlib.pump(batches, streams, steps, flags | kmlib.KM_PUMP_UNPAIRED)
    assert sum(b.paired_steps() for b in batches) == before + n_paired, ctx
    for q in range(ran):
        _same(paired[q], _snapshot(batches[q]), (ctx, "paired vs unpaired", q))
    return paired


@pytest.fixture
def pool_streams():
    sts = [kmlib.stream_create(0) for _ in range(4)]
    yield sts
    for st in sts:
        kmlib.stream_destroy(st)


def _mixed_sets():
    """One table and four target sets of it: 8 targets of 40-70 nt, 300 of 40-500, 64 of 300-500 and 150 of 500."""
    case = synth.make_case(n_targets=522, length=500, k=K, n_keys=5_000, seed=8100, variant_frac=0.4, exact_pad=False)
    short = _cut({"targets": case["targets"][0:8]}, [40, 44, 51, 70])
    wide = _cut({"targets": case["targets"][8:308]}, [40, 500, 61, 333, 120, 499, 256 + K - 1, 257 + K - 1, 75, 410])
    mid = _cut({"targets": case["targets"][308:372]}, [300, 500, 431])
    whole = _cut({"targets": case["targets"][372:522]}, [500])
    return case, [short, wide, mid, whole]


@pytest.fixture(scope="module")
def mixed_db():
    """The sets of _mixed_sets on the device, and what each gives when run alone (computed once, never changed)."""
    case, sets = _mixed_sets()
    db = kmlib.Database.from_records(case["keys"], case["counts"], K).upload(0)
    want = []
    for s in sets:
        b = _batch(db, s)
        want.append(_alone(b))
        b.close()
    yield db, sets, want
    db.close()


# ------------------------------------------------------------------ n batches, step counts that are no multiple of n
@pytest.mark.parametrize("n", [2, 3, 4])
def test_step_counts_that_are_no_multiple_of_n(n, mixed_db, pool_streams):
    db, sets, want = mixed_db
    order = [1, 0, 3, 2][:n]                                  # (300 targets, then 8: few seed blocks behind many)
    batches = [_batch(db, sets[i]) for i in order]
    for steps in (n + 1, 2 * n + 1, 3 * n - 1):
        got = _pump_both_ways(batches, pool_streams[:n], steps, ("steps", n, steps))
        for q, r in enumerate(got):
            _same(r, want[order[q]], ("steps", n, steps, "pumped vs alone", q))
    for b in batches:
        b.close()


def test_null_stream_and_one_caller_stream_for_two_batches(mixed_db, pool_streams):
    db, sets, want = mixed_db
    batches = [_batch(db, sets[i]) for i in (2, 3, 0)]
    for streams in ([None] * 3, [pool_streams[0], pool_streams[0], pool_streams[1]]):
        got = _pump_both_ways(batches, streams, 7, ("shared", streams[0] is None))
        for q, r in enumerate(got):
            _same(r, want[(2, 3, 0)[q]], ("shared", streams[0] is None, q))
    for b in batches:
        b.close()


# ------------------------------------------------------------------ seed blocks: far fewer than walk blocks, far more
def test_few_and_many_seed_blocks_behind_the_walk_blocks(mixed_db, pool_streams):
    """The walk grid of a batch that has delivered nothing is its target count, afterwards 1.25 x its flagged targets
    + 64: the 8-target batch (8 seed blocks) is seeded behind 300 and then about 200 walk blocks, the 300-target batch
    (over 400 seed blocks) behind 8 and then 64."""
    db, sets, want = mixed_db
    batches = [_batch(db, sets[1]), _batch(db, sets[0])]
    for round_ in range(2):
        got = _pump_both_ways(batches, pool_streams[:2], 5, ("few and many", round_))
        _same(got[0], want[1], ("few and many", round_, 0))
        _same(got[1], want[0], ("few and many", round_, 1))
    for b in batches:
        b.close()


# ------------------------------------------------------------------ a new target set on the stream, right before the pump
def test_new_targets_on_the_batch_stream_right_before_the_pump(pool_streams):
    """After a pump over a light set (nothing flagged: walk grid 64 blocks, a small delivery), a heavy set goes to each
    batch through its own stream (km_batch_set_targets_dev) and the pump follows at once, with a FULL delivery: the
    k_pack on the front must see the new bases, more targets are flagged than the walk grid has blocks (the rest goes
    through the large tier, inside the pump), and the delivery's tail is longer than the first copy's guess.  The
    reference workspaces go through the same history unpaired, with the sets given from the host."""
    import torch
    light = synth.make_case(n_targets=240, length=400, k=K, n_keys=5_000, seed=8200, variant_frac=0.0, exact_pad=False)
    heavy = synth.make_case(n_targets=240, length=400, k=K, n_keys=5_000, seed=8201, variant_frac=1.0,
                            variants_per_target=(3, 4), kinds=("snv", "ins"), vaf=(0.3, 0.6), exact_pad=False)
    keys, counts = _merge([light, heavy])
    db = kmlib.Database.from_records(keys, counts, K).upload(0)
    ls, hs = _cut(light, [400]), _cut(heavy, [400])
    halves = [slice(0, 120), slice(120, 240)]
    test = [_batch(db, ls[h]) for h in halves]
    ref = [_batch(db, ls[h]) for h in halves]
    streams = pool_streams[:2]
    kmlib.pump(test, streams, 5, LEAN | kmlib.KM_PUMP_PAIRED)
    kmlib.pump(ref, streams, 5, LEAN | kmlib.KM_PUMP_UNPAIRED)
    assert all(int(b.wait_result().n_flagged) == 0 for b in test + ref)
    blobs = []
    for q, h in enumerate(halves):
        blob, offs = kmlib.pack_sequences(hs[h])
        blobs.append(torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), blob])).to("cuda"))
    torch.cuda.synchronize()
    for q, h in enumerate(halves):
        _blob, offs = kmlib.pack_sequences(hs[h])
        test[q].set_targets_dev(blobs[q].data_ptr(), offs + np.uint64(3), streams[q])
    before = sum(b.paired_steps() for b in test)
    kmlib.pump(test, streams, 5, FULL | kmlib.KM_PUMP_PAIRED)
    assert sum(b.paired_steps() for b in test) - before == 4
    for q, h in enumerate(halves):
        ref[q].set_targets(hs[h])
    kmlib.pump(ref, streams, 5, FULL | kmlib.KM_PUMP_UNPAIRED)
    total_ref = 120 * (400 - K + 1)
    for q in range(2):
        got, want = _snapshot(test[q]), _snapshot(ref[q])
        _same(got, want, ("new set", q))
        assert got["sizes"]["n_flagged"] > 64 + 32                       # more than the grid's blocks
        # (batch_host.h: the first copy takes 4.5 bytes per reference k-mer + 64 KiB of the tail)
        assert 4 * got["sizes"]["n_nodes"] + 8 * got["sizes"]["n_extra"] > 4 * total_ref + total_ref // 2 + (64 << 10), got["sizes"]
    del blobs
    for x in test + ref:
        x.close()
    db.close()


# ------------------------------------------------------------------ a batch that keeps two launches
def test_front_is_taken_up_and_dropped_around_a_batch_of_two_launches(pool_streams):
    """A longest target of 512 k-mers: k_dfs and k_graph_pure of that batch are two launches, so it takes no other
    batch's seeds and a run of paired steps ends at it (its own seeds still run in the launch before it): steps
    L S1 S2 L S1 S2 L pair S1 -> S2 and S2 -> L, twice, and the pump's streams are taken up again in between."""
    long_ = synth.make_case(n_targets=40, length=512 + K - 1, k=K, n_keys=5_000, seed=8300, variant_frac=0.5, exact_pad=False)
    short = synth.make_case(n_targets=160, length=300, k=K, n_keys=5_000, seed=8301, variant_frac=0.4, exact_pad=False)
    keys, counts = _merge([long_, short])
    db = kmlib.Database.from_records(keys, counts, K).upload(0)
    ss = _cut(short, [300, 120, 44, 299])
    batches = [_batch(db, _cut(long_, [512 + K - 1, 511 + K - 1, 200])), _batch(db, ss[:60]), _batch(db, ss[60:])]
    want = [_alone(b) for b in batches]
    got = _pump_both_ways(batches, pool_streams[:3], 7, "two launches", paired_steps=4)
    for q, r in enumerate(got):
        _same(r, want[q], ("two launches", q))
    for b in batches:
        b.close()
    db.close()


# ------------------------------------------------------------------ no target flagged, every target flagged
def test_no_target_flagged_and_every_target_flagged(pool_streams):
    cases = [synth.make_case(n_targets=150, length=300, k=K, n_keys=5_000, seed=8400 + i, variant_frac=vf, vaf=(0.3, 0.6),
                             exact_pad=False) for i, vf in enumerate((0.0, 1.0, 0.0))]
    keys, counts = _merge(cases)
    db = kmlib.Database.from_records(keys, counts, K).upload(0)
    batches = [_batch(db, _cut(c, [300])) for c in cases]         # (whole: the table knows what lies behind a cut target)
    want = [_alone(b) for b in batches]                       # (from here on the walk grids follow what was flagged: 64 blocks at the floor)
    for round_ in range(2):
        got = _pump_both_ways(batches, pool_streams[:3], 7, ("extremes", round_))
        for q, r in enumerate(got):
            _same(r, want[q], ("extremes", round_, q))
    assert [g["sizes"]["n_flagged"] for g in got] == [0, got[1]["sizes"]["n_flagged"], 0] and got[1]["sizes"]["n_flagged"] > 140
    for b in batches:
        b.close()
    db.close()


# ------------------------------------------------------------------ pump after pump, then every batch alone
def test_three_pumps_in_a_row_then_each_batch_alone(mixed_db, pool_streams):
    db, sets, want = mixed_db
    batches = [_batch(db, sets[i]) for i in (3, 1, 2)]
    streams = pool_streams[:3]
    for steps, flags, n_paired in ((7, LEAN, 6), (4, FULL, 3), (8, LEAN, 7)):
        before = sum(b.paired_steps() for b in batches)
        kmlib.pump(batches, streams, steps, flags | kmlib.KM_PUMP_PAIRED)
        assert sum(b.paired_steps() for b in batches) - before == n_paired
    for q, b in enumerate(batches):
        _same(_snapshot(b), want[(3, 1, 2)[q]], ("after three pumps", q))
    for q, b in enumerate(batches):
        b.run(LEAN, streams[q])
        _same(_snapshot(b), want[(3, 1, 2)[q]], ("alone on its own stream", q))
    for b in batches:
        b.close()


# ------------------------------------------------------------------ the other arrangements, each in a process of its own
KNOBS = ("KM_PUMP_FRONT", "KM_PAIR_PURE_LAST")


def _digest():
    """What a child process prints: per batch of a paired pump over the sets of _mixed_sets, the SHA-256 of every array of
    the lean delivery and of the full one, and the sizes."""
    case, sets = _mixed_sets()
    db = kmlib.Database.from_records(case["keys"], case["counts"], K).upload(0)
    batches = [_batch(db, sets[i]) for i in (1, 0, 3, 2)]
    streams = [kmlib.stream_create(0) for _ in range(4)]
    kmlib.pump(batches, streams, 11, LEAN | kmlib.KM_PUMP_PAIRED)
    out = {"paired_steps": sum(b.paired_steps() for b in batches), "batches": []}
    for b in batches:
        snap = _snapshot(b)
        h = {part + "." + key: hashlib.sha256(np.ascontiguousarray(val).tobytes()).hexdigest()
             for part in ("first", "full") for key, val in sorted(snap[part].items())}
        out["batches"].append({"arrays": h, "sizes": snap["sizes"]})
    print(json.dumps(out))


def _child(env_knobs):
    env = {k_: v for k_, v in os.environ.items() if k_ not in KNOBS}
    env.update(env_knobs)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--digest"]
    proc = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert proc.returncode == 0, (env_knobs, proc.stderr[-3000:])
    return json.loads(proc.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def default_digest():
    return _child({})


@pytest.mark.parametrize("knobs", [{"KM_PUMP_FRONT": "0"}, {"KM_PAIR_PURE_LAST": "0"},
                                   {"KM_PUMP_FRONT": "0", "KM_PAIR_PURE_LAST": "0"}],
                         ids=["k_pack on the chain", "pure-chain blocks first", "round 7"])
def test_other_arrangements_deliver_the_same(knobs, default_digest):
    assert default_digest["paired_steps"] == 10
    assert _child(knobs) == default_digest


if __name__ == "__main__" and "--digest" in sys.argv:
    _digest()
