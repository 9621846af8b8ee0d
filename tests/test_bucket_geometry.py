"""Lookups and walks through every bucket geometry of the table (km_amd/csrc/device_common.h): empty buckets, one
pair, small, class mode, crowded, buckets the walk holds in its lanes and buckets too large for them.

A case builds a tiny table under an environment that forces one geometry (KM_DIR_LOG2, KM_TABLE_LOAD,
KM_TABLE_LEAN_CROWDED), reads it back (Database.debug_table) and first proves — from the directory and a plain numpy
model of "which bucket, which tag", restated from the layout text of device_common.h — what the case is meant to
show.  Only then are the kernels compared, all exact: query, children and cov_seqs against a dict, walk and graph
against oracle/km_oracle.py, the same batch through the lean 16-bit delivery and through the paired pump.  The model
itself is checked on the CPU against make_key (tests/host/key_probe.hip)."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from km_amd import kmer as km
from km_amd import lib as kmlib
from km_amd import synth
from km_amd.finder import BatchFinder
from km_amd.jellyfish import Jellyfish
from oracle import c_oracle
from oracle import km_oracle as ko
from test_structured_kmers import _against_c, _all_t_case, _c_want, _check_lookups, _lookup, _run, _sweep_case

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U32 = 0xFFFFFFFF
M32 = np.uint64(U32)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
LANE_SETS = 7                          # BUCKET_LANES_SETS of km_amd/csrc/device_common.h
HELD = 64 * LANE_SETS                  # the largest bucket k_dfs keeps in the lanes of its wave
EDGE = (65534, 65535, 65536, U32, 0)   # counts around the 16-bit escape, and a stored zero


# ------------------------------------------------------------------ the model: which bucket, which tag
def minimizer_len(k):
    m = min(k - 1, 15)
    if m % 2 == 0:
        m -= 1
    return max(m, 1)


def n_classes(k):
    """NC: the power of two >= 2w, at least 2."""
    w = k - minimizer_len(k)
    nc = 2
    while nc < 2 * w:
        nc *= 2
    return nc


def key_model(P, k, canonical, log2_buckets):
    """(bucket, tag, flip, cls) of the (k-1)-mers P: the window of P whose canonical m-mer c has the smallest
    (c * 0x9E3779B1 mod 2^32) & ~511, leftmost on ties; bucket = mm_bucket(c) >> (32 - log2 n_buckets); tag = P << 1,
    or (revcomp(P) << 1) | 1 in a canonical table when revcomp(P) < P; cls = strand * w + offset from the right."""
    P = np.asarray(P, dtype=np.uint64)
    m = minimizer_len(k)
    w = k - m
    mmask = np.uint64((1 << (2 * m)) - 1)
    R = km.revcomp(P, k - 1)
    best = np.full(P.shape, 1 << 40, dtype=np.uint64)
    bc = np.zeros(P.shape, dtype=np.uint64)
    bs = np.zeros(P.shape, dtype=np.uint64)
    bu = np.zeros(P.shape, dtype=np.uint64)
    for j in range(w):
        f = (P >> np.uint64(2 * (w - 1 - j))) & mmask
        r = (R >> np.uint64(2 * j)) & mmask
        c = np.minimum(f, r)
        order = ((c * np.uint64(0x9E3779B1)) & M32) & ~np.uint64(511)
        better = order < best                               # strictly: the leftmost window wins a tie
        best = np.where(better, order, best)
        bc = np.where(better, c, bc)
        bs = np.where(better, (f >= r).astype(np.uint64), bs)
        bu = np.where(better, np.uint64(j), bu)
    h = bc ^ np.uint64(0x5bd1e995)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    bucket = (h >> np.uint64(32 - log2_buckets)).astype(np.int64)
    flip = (R < P) if canonical else np.zeros(P.shape, dtype=bool)
    tag = np.where(flip, (R << np.uint64(1)) | np.uint64(1), P << np.uint64(1))
    cls = (bs * np.uint64(w) + (np.uint64(w - 1) - bu)).astype(np.int64)
    return bucket, tag, flip.astype(np.int64), cls


def record_orientations(keys, counts, k, canonical):
    """The orientations under which the records are entered, with their counts: none for a count of zero and for a
    non-canonical key of a canonical table, one for a palindrome or a non-canonical table, else two."""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.uint32)
    live = counts != 0
    keys, counts = keys[live], counts[live]
    if not canonical:
        return keys, counts
    rc = km.revcomp(keys, k)
    ok = rc >= keys
    two = rc > keys
    return np.concatenate([keys[ok], rc[two]]), np.concatenate([counts[ok], counts[two]])


def shape_capacity(cap, nc):
    """table_kernels.h: slots of a bucket that `cap` slots were asked for."""
    cap = np.asarray(cap, dtype=np.int64)
    cap = cap + (cap & 1)
    return np.where(cap >= nc, (cap + 2 * nc - 1) // (2 * nc) * (2 * nc), cap)


def table_model(keys, counts, k, canonical, log2_buckets):
    """The groups of a table: sorted tags, each one's bucket and four 16-bit counts; entries per bucket."""
    O, cnt = record_orientations(keys, counts, k, canonical)
    bucket, tag, flip, _ = key_model(O >> np.uint64(2), k, canonical, log2_buckets)
    base = (O & np.uint64(3)).astype(np.int64)
    slot = np.where(flip == 1, 3 - base, base)
    tags, first, inv = np.unique(tag, return_index=True, return_inverse=True)
    c4 = np.zeros((tags.size, 4), dtype=np.uint16)
    c4[inv, slot] = np.minimum(cnt, 65535).astype(np.uint16)
    return {"tags": tags, "bucket": bucket[first], "c4": c4,
            "entries": np.bincount(bucket, minlength=1 << log2_buckets).astype(np.int64)}


def classify(S, nc):
    """0 empty, 1 small (S < NC), 2 class mode (S = q NC, q even), 3 crowded (q odd) — as home_slot tells them apart."""
    S = np.asarray(S, dtype=np.int64)
    q = S // nc
    return np.where(S == 0, 0, np.where(q == 0, 1, np.where(q % 2 == 1, 3, 2)))


EMPTY_B, SMALL, CLASS, CROWDED = 0, 1, 2, 3


def home_slot_model(tag, cls, S, k):
    """home_slot of device_common.h for groups (tag, class) in buckets of S slots: floor(frac S / 2^32) in a small
    bucket, class * q + floor(h q / 2^32) in class mode, 2 floor(h (S / 2) / 2^32) in a crowded one; even throughout."""
    w = k - minimizer_len(k)
    nc = np.uint64(n_classes(k))
    inv32 = np.uint64((1 << 32) // (2 * w * 256))
    tag = np.asarray(tag, dtype=np.uint64)
    cls = np.asarray(cls).astype(np.uint64)
    S = np.asarray(S).astype(np.uint64)
    h = (((tag & M32) * np.uint64(0x9E3779B1)) & M32) ^ (((tag >> np.uint64(32)) * np.uint64(0x85EBCA6B)) & M32)
    frac = (((cls << np.uint64(8)) | (h >> np.uint64(24))) * inv32) & M32
    q = S // nc
    small, crowded = q == 0, (q & np.uint64(1)) == 1
    m = (np.where(small, frac, h) * np.where(small, S, np.where(crowded, S >> np.uint64(1), q))) >> np.uint64(32)
    even = m & ~np.uint64(1)
    return np.where(small, even, np.where(crowded, m << np.uint64(1), cls * q + even)).astype(np.int64)


# ------------------------------------------------------------------ the model against make_key, on the CPU
MODEL_KS = (2, 3, 4, 12, 16, 17, 21, 31, 32)


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    return hipcc


@functools.lru_cache(maxsize=None)
def _key_probe(sanitize=False):
    """tests/host/key_probe.hip, compiled once per session (host code only; hipcc is what builds the library)."""
    tmp = tempfile.mkdtemp(prefix="km_key_probe_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "key_probe_san" if sanitize else "key_probe")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O1" if sanitize else "-O2", "-std=c++17"] + extra +
                          ["-o", exe, os.path.join(HERE, "host", "key_probe.hip")])
    return exe


def _probe(exe, k, canonical, log2_buckets, P):
    text = "".join("%d\n" % x for x in P.tolist())
    out = subprocess.run([exe, str(k), str(int(canonical)), str(log2_buckets)], input=text, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = np.array(out.stdout.split(), dtype=np.uint64).reshape(-1, 4)
    assert got.shape[0] == P.size
    return got


def _model_probes(k, seed):
    """About 2 000 seeded (k-1)-mers (the whole space below that), the homopolymers, (AT)n, (TA)n and — k odd — one
    that is its own reverse complement."""
    n = k - 1
    rng = np.random.default_rng(seed)
    top = (1 << (2 * n)) - 1
    if top < 2000:
        P = np.arange(top + 1, dtype=np.uint64)
    else:
        P = rng.integers(0, top, size=2000, dtype=np.uint64, endpoint=True)
    special = [km.pack_str(b * n) for b in "ACGT"] + [km.pack_str(("AT" * n)[:n]), km.pack_str(("TA" * n)[:n])]
    if n % 2 == 0:
        half = synth.random_seq(rng, n // 2)
        pal = half + synth.revcomp_str(half)
        assert synth.revcomp_str(pal) == pal
        special.append(km.pack_str(pal))
    return np.concatenate([P, np.array(special, dtype=np.uint64)])


def test_key_model_equals_make_key():
    """bucket, tag, flip and class of the model against make_key itself, compiled for the host: every k where the
    geometry changes (w = 1, 2, 6, 16, 17; m = 1, 3, 11, 15), both canonical settings, 2^4 and 2^10 buckets; once
    more under AddressSanitizer and UBSan, where the shifts of k = 2 and k = 32 would show."""
    exe = _key_probe()
    n_flip = n_pal = 0
    for k in MODEL_KS:
        P = _model_probes(k, 9700 + k)
        for canonical in (True, False):
            for log2_buckets in (4, 10):
                bucket, tag, flip, cls = key_model(P, k, canonical, log2_buckets)
                got = _probe(exe, k, canonical, log2_buckets, P)
                ctx = (k, canonical, log2_buckets)
                assert np.array_equal(got[:, 0], bucket.astype(np.uint64)), ctx
                assert np.array_equal(got[:, 1], tag), ctx
                assert np.array_equal(got[:, 2], flip.astype(np.uint64)), ctx
                assert np.array_equal(got[:, 3], cls.astype(np.uint64)), ctx
                assert int(bucket.max()) < (1 << log2_buckets) and int(cls.max()) < 2 * (k - minimizer_len(k))
                assert canonical or not flip.any()
                n_flip += int(flip.sum())
        n_pal += int((km.revcomp(P, k - 1) == P).sum())
    assert n_flip > 2000 and n_pal >= 4                              # both tag forms, and (k-1)-mers equal to their own
    san = _key_probe(sanitize=True)                                  # reverse complement, were compared
    for k in MODEL_KS:
        P = _model_probes(k, 9700 + k)
        for canonical in (True, False):
            bucket, tag, flip, cls = key_model(P, k, canonical, 4)
            got = _probe(san, k, canonical, 4, P)
            assert np.array_equal(got[:, 0], bucket.astype(np.uint64)) and np.array_equal(got[:, 1], tag), (k, canonical)


def test_model_helpers():
    assert [minimizer_len(k) for k in MODEL_KS] == [1, 1, 3, 11, 15, 15, 15, 15, 15]
    assert [n_classes(k) for k in MODEL_KS] == [2, 4, 2, 2, 2, 4, 16, 32, 64]
    assert shape_capacity([0, 1, 2, 29, 31, 32, 64, 65, 240], 32).tolist() == [0, 2, 2, 30, 64, 64, 64, 128, 256]
    assert classify([0, 2, 30, 64, 96, 416, 448], 32).tolist() == [0, 1, 1, 2, 3, 3, 2]
    # a palindrome is entered once, a key above its reverse complement not at all, a zero count not at all
    keys = np.array([km.pack_str(s) for s in ("ACGT", "AAAA", "TTTT", "ACCA")], dtype=np.uint64)
    O, c = record_orientations(keys, np.array([3, 4, 5, 0], np.uint32), 4, True)
    assert sorted(km.unpack(x, 4) for x in O.tolist()) == ["AAAA", "ACGT", "TTTT"] and sorted(c.tolist()) == [3, 4, 4]
    O, c = record_orientations(keys, np.array([3, 4, 5, 0], np.uint32), 4, False)
    assert sorted(km.unpack(x, 4) for x in O.tolist()) == ["AAAA", "ACGT", "TTTT"] and sorted(c.tolist()) == [3, 4, 5]


# ------------------------------------------------------------------ records, oracle side
def _py_oracle(keys, counts, k, canonical):
    return ko.KmerDB(None, 0.05, 5, records={"k": k, "canonical": canonical, "keys": keys, "counts": counts})


def _analyse_all(keys, counts, k, canonical, names, seqs):
    py = _py_oracle(keys, counts, k, canonical)
    return [ko.analyse_target(s, n, py) for n, s in zip(names, seqs)]


def _place_edge_counts(keys, counts, k, canonical, names, seqs):
    """EDGE on k-mers in the middle of variant paths (nodes the walk discovered): the escaped counts and 65534 on the
    first variant targets, the zero on the last one, where it cuts that path alone."""
    wants = _analyse_all(keys, counts, k, canonical, names, seqs)
    pools = []
    for w in wants:
        runs = [[i for i in p if i >= w["n_ref"]] for p in w["paths"]]
        runs = [r for r in runs if len(r) >= 6]
        if runs:
            pools.append([km.pack_str(w["kmers"][i]) for i in max(runs, key=len)])
    assert len(pools) >= 2, "two targets with a variant path of six discovered nodes are needed"
    at = {int(x): i for i, x in enumerate(keys.tolist())}
    share = [[] for _ in pools[:-1]]
    for j, value in enumerate(EDGE[:-1]):
        share[j % len(share)].append(value)
    share.append([EDGE[-1]])
    counts = counts.copy()
    placed = []
    for pool, values in zip(pools, share):
        for r, value in enumerate(values):
            x = pool[(r + 1) * len(pool) // (len(values) + 1)]
            if canonical:
                x = int(km.canonical(np.array([x], np.uint64), k)[0])
            assert x in at and x not in placed
            counts[at[x]] = value
            placed.append(x)
    assert len(placed) == len(EDGE)
    return counts


def _finish(keys, counts, k, canonical, names, seqs, edge=True):
    """Everything the comparisons share, computed once: the dict, the oracle's results, the k-mers the walks visit."""
    if edge:
        counts = _place_edge_counts(keys, counts, k, canonical, names, seqs)
        assert set(EDGE) <= set(counts.tolist())
    wants = _analyse_all(keys, counts, k, canonical, names, seqs)
    walked = np.unique(np.array([km.pack_str(x) for w in wants for x in w["kmers"]], dtype=np.uint64))
    if edge:
        found = [c for w in wants for c in w["counts"][w["n_ref"]:]]
        assert any(c >= 65535 for c in found) and 65534 in found     # the walk itself passes escaped counts
        assert sum(len(w["paths"]) > 1 for w in wants) >= 2
    return {"k": k, "canonical": canonical, "keys": keys, "counts": counts, "names": names, "seqs": seqs,
            "table": dict(zip(keys.tolist(), counts.tolist())), "wants": wants, "walked": walked}


def _background(rng, n, k, canonical, taken):
    top = (1 << (2 * k)) - 1
    pad = rng.integers(0, top, size=n + 64, dtype=np.uint64, endpoint=True)
    if canonical:
        pad = km.canonical(pad, k)
    pad = np.unique(pad)
    pad = pad[~np.isin(pad, taken)]
    pad = pad[rng.permutation(pad.size)[:n]]
    return pad, rng.integers(2, 51, size=pad.size).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _synthetic(k, canonical, n_targets, length, n_background, seed, all_t=False):
    """n_targets targets with one variant each (all four kinds) and their own k-mers, a few hundred background keys;
    all_t: also the target and the reads around T^32 of test_all_t_key_of_a_non_canonical_k32_table."""
    case = synth.make_case(n_targets=n_targets, length=length, k=k, n_keys=0, seed=seed, variant_frac=1.0,
                           kinds=("snv", "ins", "del", "dup"), canonical=canonical)
    keys, counts = case["keys"], case["counts"]
    names, seqs = list(case["names"]), [km.decode(r) for r in case["targets"]]
    rng = np.random.default_rng(seed + 1)
    if all_t:
        assert k == 32 and not canonical
        T, reads = _all_t_case()
        tk, tc = synth.reads_to_records(reads, k, canonical=False)
        new = ~np.isin(tk, keys)
        keys, counts = np.concatenate([keys, tk[new]]), np.concatenate([counts, tc[new]])
        names.insert(0, "allT")
        seqs.insert(0, T)
    pad, padc = _background(rng, n_background, k, canonical, keys)
    keys, counts = np.concatenate([keys, pad]), np.concatenate([counts, padc])
    order = rng.permutation(keys.size)
    rec = _finish(keys[order], counts[order], k, canonical, names, seqs)
    if all_t:
        all_t_key = 0xFFFFFFFFFFFFFFFF
        assert rec["table"][all_t_key] == 330 and all_t_key in rec["walked"].tolist()
    return rec


# ------------------------------------------------------------------ proofs: directory and slots against the model
def _env_unit(env):
    return int(1.0 / float(env["KM_TABLE_LOAD"]) + 0.5) if "KM_TABLE_LOAD" in env else 2


def _upload(monkeypatch, rec, env, keys=None, counts=None):
    for name in ("KM_DIR_LOG2", "KM_TABLE_LOAD", "KM_TABLE_LEAN_CROWDED", "KM_TABLE_NO_SETTLE"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, str(value))
    keys = rec["keys"] if keys is None else keys
    counts = rec["counts"] if counts is None else counts
    return kmlib.Database.from_records(keys, counts, rec["k"], rec["canonical"]).upload(0)


def _read_table(db, rec, env):
    """The table as built against the model.  Directory: bucket b is empty iff the model enters nothing there, and
    holds at least shape_capacity(unit * entries) slots.  Slots: as many occupied ones as info.n_groups; their tags
    are the model's tags, each once, each in the bucket the model names, with the counts the model gives."""
    k, canonical = rec["k"], rec["canonical"]
    dir_, tag, c4 = db.debug_table()
    n_buckets = dir_.size - 1
    log2_buckets = n_buckets.bit_length() - 1
    assert n_buckets == 1 << log2_buckets
    if "KM_DIR_LOG2" in env:
        assert log2_buckets == int(env["KM_DIR_LOG2"])
    model = table_model(rec["keys"], rec["counts"], k, canonical, log2_buckets)
    nc = n_classes(k)
    start = 2 * dir_.astype(np.int64)
    S = np.diff(start)
    assert dir_[0] == 0 and (S >= 0).all() and tag.size == db.info.n_slots == max(64, int(start[-1]))
    assert np.array_equal(S == 0, model["entries"] == 0)
    assert (S >= shape_capacity(_env_unit(env) * model["entries"], nc)).all()
    assert (S % 2 == 0).all() and ((S < nc) | (S % nc == 0)).all()
    at = np.nonzero(tag != EMPTY)[0]
    assert at.size == db.info.n_groups == model["tags"].size
    order = np.argsort(tag[at])
    at = at[order]                                                   # the occupied slots, in tag order like the model
    assert np.array_equal(tag[at], model["tags"])
    bucket = np.searchsorted(start, at, side="right") - 1
    assert np.array_equal(bucket, model["bucket"])
    assert np.array_equal(c4[at], model["c4"])
    assert not c4[tag == EMPTY].any()
    # class mode: class c of a bucket of q NC slots owns the slots [c q, (c + 1) q), and a bucket that is still in
    # class mode has kept every key inside its home pair, so inside its class
    kind, slot = classify(S, nc), at - start[bucket]
    G = model["tags"] >> np.uint64(1)
    flipped = (model["tags"] & np.uint64(1)) == 1
    assert canonical or not flipped.any()
    P = np.where(flipped, km.revcomp(G, k - 1), G)                   # the (k-1)-mer as it was entered
    again, tags, _, cls = key_model(P, k, canonical, log2_buckets)
    assert np.array_equal(tags, model["tags"]) and np.array_equal(again, bucket)
    in_class = kind[bucket] == CLASS
    assert np.array_equal(slot[in_class] // (S[bucket][in_class] // nc), cls[in_class])
    home = home_slot_model(model["tags"], cls, S[bucket], k)
    assert (home % 2 == 0).all() and (home + 1 < S[bucket]).all()
    assert (((slot - home) >= 0) & ((slot - home) <= 1))[in_class].all()
    return {"S": S, "nc": nc, "log2": log2_buckets, "kind": kind, "tags": model["tags"], "bucket": bucket,
            "slot": slot, "home": home, "entries": model["entries"], "dir": dir_, "tag": tag, "c4": c4}


def _walked_groups(rec, tab):
    """The groups the walks look up behind the k-mers they visit (targets and variant paths): P = x[1:].  Per walked
    k-mer its bucket; per walked group that exists its bucket and its slot in the bucket."""
    k = rec["k"]
    P = rec["walked"] & np.uint64((1 << (2 * (k - 1))) - 1)
    bucket, tag, _, _ = key_model(P, k, rec["canonical"], tab["log2"])
    tags, first = np.unique(tag, return_index=True)
    bucket = bucket[first]
    pos = np.searchsorted(tab["tags"], tags)
    pos[pos >= tab["tags"].size] = 0
    there = tab["tags"][pos] == tags if tab["tags"].size else np.zeros(tags.size, dtype=bool)
    assert there.sum() * 2 >= tags.size                              # (most of them exist: the walk follows stored k-mers)
    return bucket, bucket[there], tab["slot"][pos[there]]


def _prove_layout(db, rec, tab, kinds, held=None, sets=(), probing=None, share=0.5):
    """At least `share` of the walked groups lie in buckets of the kinds named (and held in the lanes, or not); some
    walked group sits in every lane set of `sets`; the table probes beyond the home pair (or does not)."""
    bucket, there_bucket, there_slot = _walked_groups(rec, tab)
    ok = np.isin(tab["kind"][bucket], kinds)
    if held is not None:
        ok &= (tab["S"][bucket] <= HELD) == held
    assert ok.sum() >= share * bucket.size, (int(ok.sum()), bucket.size, np.bincount(tab["kind"][bucket], minlength=4).tolist(),
                                            sorted(set(tab["S"][bucket].tolist())))
    in_kind = np.isin(tab["kind"][there_bucket], kinds)
    if held is not None:
        in_kind &= (tab["S"][there_bucket] <= HELD) == held
    seen = set((there_slot[in_kind] // 64).tolist())
    assert set(sets) <= seen, (sorted(seen), sorted(set(tab["S"].tolist())))
    if probing is not None:
        assert (db.info.max_probe > 2) == probing, db.info.max_probe


# ------------------------------------------------------------------ comparisons, all exact
def _neighbours(keys, k):
    """The 3 k one-base neighbours of every key."""
    out = []
    for pos in range(k):
        sh = np.uint64(2 * pos)
        for d in (1, 2, 3):
            out.append(keys ^ (np.uint64(d) << sh))
    return np.concatenate(out)


def _compare_lookups(db, rec):
    k, canonical, table = rec["k"], rec["canonical"], rec["table"]
    keys = rec["keys"]
    probes = np.concatenate([keys, km.revcomp(keys, k), _neighbours(keys, k)])
    assert np.array_equal(db.query(probes), _lookup(table, probes, k, canonical))
    rng = np.random.default_rng(97)
    ask = np.concatenate([keys, km.revcomp(keys, k), rec["walked"], probes[rng.integers(0, probes.size, size=2000)]])

    def query(x):
        return _lookup(table, x, k, canonical)
    _check_lookups(db, query, ask, k)                                # query, then children at (0.05, 5) and (0, 0), both ways
    cov = db.cov_seqs(rec["seqs"])
    for t, seq in enumerate(rec["seqs"]):
        c = query(km.sliding_kmers(km.encode(seq), k)).astype(np.int64)
        want = (int(c.sum()), c.size, int((c == 0).sum()), 0, 0, int(c.min()), int(c.max()))
        assert tuple(int(cov[t][f]) for f in ("total", "n_kmers", "n_zero", "n_skipped", "n_nonbase", "min", "max")) == want, t


_RUN_FIELDS = ("status", "n_ref", "probes", "path_off", "run_off", "run_start", "run_len", "path_len", "path_min_cov")


def _compare_walks(db, rec):
    """Walk and graph against the oracle, field by field; the lean 16-bit delivery and the paired pump against that."""
    k, seqs = rec["k"], rec["seqs"]
    jf = Jellyfish("mem.jf", cutoff=0.05, n_cutoff=5, db=db)
    got = BatchFinder(jf).analyse(list(zip(rec["names"], seqs)))
    for g, want in zip(got, rec["wants"]):
        name = want["name"]
        assert not isinstance(g, Exception), (name, g)
        assert g.n_ref == want["n_ref"], name
        assert [km.unpack(x, k) for x in g.kmers] == want["kmers"], name
        assert g.counts.tolist() == want["counts"], name
        assert g.probes == want["probes"], name
        assert [p.tolist() for p in g.paths] == [list(p) for p in want["paths"]], name
        assert list(g.min_cov) == want["min_cov"], name
    full = _run(db, seqs)
    st = [kmlib.stream_create(0) for _ in range(2)]
    lean = kmlib.KM_RUN_DELIVER | kmlib.KM_DELIVER_LEAN | kmlib.KM_DELIVER_COUNT16
    v16 = _run(db, seqs, flags=lean, stream=st[0])
    assert "node_count16" in v16
    for field in _RUN_FIELDS:
        assert np.array_equal(v16[field], full[field]), ("lean16", field)
    for t in range(len(seqs)):
        a, e = int(v16["node_off"][t]), int(v16["node_off"][t + 1])
        if e > a:                                                    # (a lean delivery skips the nodes of a one-path target)
            fa, fe = int(full["node_off"][t]), int(full["node_off"][t + 1])
            assert np.array_equal(v16["node_count"][a:e], full["node_count"][fa:fe]), ("lean16", t)
    batches = []
    for _ in range(2):
        b = kmlib.Batch(db, max_targets=max(64, len(seqs)), max_total_bases=max(1 << 14, sum(len(s) for s in seqs)))
        b.set_targets(seqs)
        batches.append(b)
    kmlib.pump(batches, st, 4, kmlib.KM_STAGE_WALK | kmlib.KM_STAGE_GRAPH | kmlib.KM_RUN_DELIVER | kmlib.KM_PUMP_PAIRED)
    assert sum(b.paired_steps() for b in batches) == 3               # k_seed ran as blocks of the k_dfs_pure launch
    for b in batches:
        f = b.fetch()
        for field in _RUN_FIELDS + ("node_off", "node_kmer", "node_count"):
            assert np.array_equal(f[field], full[field]), ("pump", field)
        b.close()
    for s in st:
        kmlib.stream_destroy(s)


def _case(monkeypatch, rec, env, **proof):
    db = _upload(monkeypatch, rec, env)
    tab = _read_table(db, rec, env)
    _prove_layout(db, rec, tab, **proof)
    _compare_lookups(db, rec)
    _compare_walks(db, rec)
    db.close()
    return tab


# ------------------------------------------------------------------ case 4: targets that contain a heavy minimizer
@functools.lru_cache(maxsize=None)
def _heavy_mmer():
    """A canonical 15-mer whose order hash is tiny: the minimizer of every 30-mer that contains it (as in
    test_heavy_minimizer_bucket_falls_back_to_probing)."""
    cand = np.arange(1, 1 << 22, dtype=np.uint64)
    cand = cand[cand <= km.revcomp(cand, 15)]
    order = (cand * np.uint64(0x9E3779B1)) & M32
    return int(cand[int(np.argmin(order >> np.uint64(9)))])


@functools.lru_cache(maxsize=None)
def _heavy_crossing(n_heavy_targets, n_fill, seed):
    """k = 31.  One or two targets carry the heavy 15-mer in their middle (as it is; reverse-complemented) with a
    substitution six bases before it resp. behind it: reference and variant chains enter the heavy bucket, stay
    for up to w steps and leave.  n_fill random k-mers around the same 15-mer size that bucket; plain targets and
    some background lie in the small buckets of the default directory, and four targets of k + 1 bases whose second
    k-mer alone is stored, its two (k-1)-mers under different minimizers: groups that have a bucket of one pair to
    themselves."""
    k, m = 31, 15
    rng = np.random.default_rng(seed)
    mm = km.unpack(_heavy_mmer(), m)
    reads, names, seqs = [], [], []
    for t, (word, side) in enumerate(((mm, -1), (synth.revcomp_str(mm), +1))[:n_heavy_targets]):
        while True:
            T = synth.random_seq(rng, 55) + word + synth.random_seq(rng, 55)
            p = 55 - 6 if side < 0 else 55 + m + 5
            var = T[:p] + "ACGT"[("ACGT".index(T[p]) + 1 + t) % 4] + T[p + 1:]
            if not synth.has_repeated_kmer(T, k) and not synth.has_repeated_kmer(var, k):
                break
        cov = int(rng.integers(200, 900))
        reads += [(T, cov), (var, cov // 2)]
        names.append("heavy%d" % t)
        seqs.append(T)
    while len(names) < n_heavy_targets + 4:
        x = rng.integers(0, 1 << 62, size=1, dtype=np.uint64)
        b, _, _, _ = key_model(np.concatenate([x >> np.uint64(2), x & np.uint64((1 << 60) - 1)]), k, True, 10)
        if b[0] != b[1]:
            reads.append((km.unpack(int(x[0]), k), 40))                 # the stored k-mer: alone in the bucket of its prefix,
            names.append("lone%d" % len(names))                         # which the walk looks up from a target k-mer that
            seqs.append("ACGT"[len(names) % 4] + reads[-1][0])          # is not stored
    keys, counts = synth.records_from_reads(reads, k)
    plain = synth.make_case(n_targets=4 - n_heavy_targets, length=130, k=k, n_keys=0, seed=seed + 1, variant_frac=1.0,
                            kinds=("snv", "ins", "del", "dup"))
    new = ~np.isin(plain["keys"], keys)
    keys = np.concatenate([keys, plain["keys"][new]])
    counts = np.concatenate([counts, plain["counts"][new]])
    names += list(plain["names"])
    seqs += [km.decode(r) for r in plain["targets"]]
    # the filling of the heavy bucket: random k-mers with the 15-mer inside both of their (k-1)-mers
    base = rng.integers(0, 1 << 62, size=n_fill, dtype=np.uint64)
    off = rng.integers(1, k - m - 1, size=n_fill).astype(np.uint64)
    shift = np.uint64(2) * (np.uint64(k - m) - off)
    mask = np.uint64((1 << (2 * m)) - 1) << shift
    fill = np.unique(km.canonical((base & ~mask) | (np.uint64(_heavy_mmer()) << shift), k))
    fill = fill[~np.isin(fill, keys)]
    keys = np.concatenate([keys, fill])
    counts = np.concatenate([counts, rng.integers(2, 51, size=fill.size).astype(np.uint32)])
    pad, padc = _background(rng, 300, k, True, keys)
    keys, counts = np.concatenate([keys, pad]), np.concatenate([counts, padc])
    order = rng.permutation(keys.size)
    return _finish(keys[order], counts[order], k, True, names, seqs)


# ------------------------------------------------------------------ the cases
# The environments come from the build's arithmetic (k_dir_capacity, k_dir_grow in table_kernels.h); the directory
# proofs of every case decide whether they do what they are chosen for.
CLASS_MODE = {
    # k: (environment, _synthetic arguments, lane sets that must hold a walked group)
    # (k = 31: a super-k-mer brings up to 2 (w + 1) entries of its own, and a variant beside it as many again; at 20
    # slots per entry that alone is more than the lanes hold, so the load is 1/7 here)
    31: ({"KM_DIR_LOG2": 7, "KM_TABLE_LOAD": 0.14}, (31, True, 3, 150, 100, 9832), range(7)),
    21: ({"KM_DIR_LOG2": 7, "KM_TABLE_LOAD": 0.05}, (21, True, 3, 150, 100, 9822), range(4)),     # w = 6, NC = 16
    12: ({"KM_DIR_LOG2": 6, "KM_TABLE_LOAD": 0.05}, (12, True, 3, 150, 100, 9813), range(4)),     # w = 1, NC = 2
}
CROWDED_HELD = (31, True, 3, 140, 400, 9832)             # about 840 stored k-mers over 32 buckets


@gpu
@pytest.mark.parametrize("k", sorted(CLASS_MODE))
def test_class_mode_buckets_held_in_several_lane_sets(k, monkeypatch):
    """Case 1.  Sparse buckets (KM_TABLE_LOAD) of a small directory: S = q NC with q even, at most 448 slots, nothing
    crowds a pair twice.  At k = 12 every (k-1)-mer is its own minimizer and NC = 2: no bucket is small."""
    env, spec, sets = CLASS_MODE[k]
    rec = _synthetic(*spec)
    tab = _case(monkeypatch, rec, env, kinds=[CLASS], held=True, sets=sets)
    assert _env_unit(env) in (7, 20)
    if k == 12:
        assert not (tab["kind"] == SMALL).any()


@gpu
def test_crowded_buckets_held_in_every_lane_set(monkeypatch):
    """Case 2.  Buckets that doubled once and then became plain two-choice tables (S an odd multiple of NC) at a size
    the lanes still hold: keys outside their home pair, max_probe > 2, a walked group in each of the seven lane sets.
    KM_TABLE_LEAN_CROWDED=0 lets such a bucket double a second time first: other sizes, the same results."""
    rec = _synthetic(*CROWDED_HELD)
    lean = _case(monkeypatch, rec, {"KM_DIR_LOG2": 5, "KM_TABLE_LEAN_CROWDED": 1}, kinds=[CROWDED], held=True,
                 sets=range(LANE_SETS), probing=True)
    fat = _case(monkeypatch, rec, {"KM_DIR_LOG2": 5, "KM_TABLE_LEAN_CROWDED": 0}, kinds=[CROWDED], probing=True)
    assert np.array_equal(lean["entries"], fat["entries"]) and (fat["S"] >= lean["S"]).all()
    assert (fat["S"] > lean["S"]).sum() >= 4
    default = _upload(monkeypatch, rec, {"KM_DIR_LOG2": 5})          # lean is what a build does when nothing is set
    assert np.array_equal(default.debug_table()[0], lean["dir"])
    default.close()


@gpu
@pytest.mark.parametrize("k,canonical", [(31, True), (31, False), (32, False)])
def test_buckets_too_large_for_the_lanes(k, canonical, monkeypatch):
    """Case 3.  Sixteen buckets for about 4 000 stored k-mers: every bucket starts above 448 slots — the model alone
    says so — and every chain step goes through children_issue_wave / children_finish_wave.  At k = 32 the key
    2^64 - 1 (T^32) is stored and lies on a target's walk."""
    rec = _synthetic(k, canonical, 3, 160, 3400 if canonical else 4400, 9860 + k + canonical, k == 32)
    entries = table_model(rec["keys"], rec["counts"], k, canonical, 4)["entries"]
    assert (shape_capacity(2 * entries, n_classes(k)) > HELD).all() and 3800 <= rec["keys"].size <= 5000
    tab = _case(monkeypatch, rec, {"KM_DIR_LOG2": 4}, kinds=[CLASS, CROWDED], held=False, share=1.0)
    assert (tab["S"] > HELD).all()


def _bucket_runs(rec, tab, want, path):
    """The buckets behind the k-mers of one path, in path order, with the runs of equal buckets collapsed:
    [(bucket, nodes of the run that the walk discovered)]."""
    k = rec["k"]
    x = np.array([km.pack_str(want["kmers"][i]) for i in path], dtype=np.uint64)
    bucket, _, _, _ = key_model(x & np.uint64((1 << (2 * (k - 1))) - 1), k, rec["canonical"], tab["log2"])
    runs = []
    for b, i in zip(bucket.tolist(), path):
        if not runs or runs[-1][0] != b:
            runs.append([b, 0])
        runs[-1][1] += i >= want["n_ref"]
    return runs


@gpu
@pytest.mark.parametrize("side", ["held", "too_large"])
def test_chains_cross_from_small_buckets_into_a_heavy_one_and_back(side, monkeypatch):
    """Case 4.  The default directory (small and one-pair buckets) and one heavy minimizer that the targets and their
    variants contain: reference and variant chains enter the heavy bucket, stay for up to w steps and leave again.
    The heavy bucket is crowded and once small enough for the lanes (the bucket in the lanes changes), once too large
    (held, not held, held: DirCache and BucketLanes must both follow)."""
    rec = _heavy_crossing(1, 16, 9902) if side == "held" else _heavy_crossing(2, 300, 9901)
    db = _upload(monkeypatch, rec, {})
    tab = _read_table(db, rec, {})
    S, kind = tab["S"], tab["kind"]
    inside = np.array([km.pack_str(rec["seqs"][0][47:77])], np.uint64)          # a 30-mer around the heavy 15-mer
    heavy_bucket = int(key_model(inside, 31, True, tab["log2"])[0][0])
    assert kind[heavy_bucket] == CROWDED and (S[heavy_bucket] <= HELD) == (side == "held"), int(S[heavy_bucket])
    assert S[heavy_bucket] == S.max() and tab["log2"] >= 10 and db.info.max_probe > 2
    _prove_layout(db, rec, tab, kinds=[SMALL, CLASS], held=True, probing=True)      # beside it: ordinary small buckets
    n_crossing = 0
    for want in rec["wants"]:
        if not want["name"].startswith("heavy"):
            continue
        assert len(want["paths"]) >= 2
        for path in want["paths"][1:]:
            runs = _bucket_runs(rec, tab, want, path)
            at = [i for i, (b, _) in enumerate(runs) if b == heavy_bucket]
            assert len(at) == 1 and 0 < at[0] < len(runs) - 1            # entered once, from another bucket, and left
            before, after = runs[at[0] - 1][0], runs[at[0] + 1][0]
            assert S[before] <= HELD and S[after] <= HELD and before != heavy_bucket != after
            assert runs[at[0]][1] >= 5                                   # discovered nodes inside the heavy bucket ...
            assert sum(n for b, n in runs if b != heavy_bucket) >= 5     # ... and outside it
            n_crossing += 1
    assert n_crossing >= (1 if side == "held" else 2)
    _, there_bucket, _ = _walked_groups(rec, tab)
    assert (S[there_bucket] == 2).sum() >= 1                             # a walked group with a bucket of one pair to itself
    assert (tab["entries"][S == 2] == 1).all() and (S == 0).any()
    _compare_lookups(db, rec)
    _compare_walks(db, rec)
    db.close()


def _settle_builds(monkeypatch, rec, settle):
    """The records of case 2 as given, reversed and permuted: per order the table read back and max_probe; every
    build passes the proofs and the lookups, the last one the walks."""
    n = rec["keys"].size
    orders = [np.arange(n), np.arange(n)[::-1], np.random.default_rng(5).permutation(n)]
    env = {"KM_DIR_LOG2": 5} if settle else {"KM_DIR_LOG2": 5, "KM_TABLE_NO_SETTLE": 1}
    seen = []
    for i, order in enumerate(orders):
        db = _upload(monkeypatch, rec, env, rec["keys"][order], rec["counts"][order])
        tab = _read_table(db, rec, env)
        _prove_layout(db, rec, tab, kinds=[CROWDED], held=True, probing=True)
        _compare_lookups(db, rec)
        if i == 2:
            _compare_walks(db, rec)
        seen.append((tab, int(db.info.max_probe)))
        db.close()
    return seen


def _pairs_in_order(tab):
    """The table with the two slots of every aligned pair in tag order (an empty slot last, as a lookup needs it)."""
    tag, c4 = tab["tag"].reshape(-1, 2), tab["c4"].reshape(-1, 2, 4)
    swap = tag[:, 0] > tag[:, 1]
    tag, c4 = tag.copy(), c4.copy()
    tag[swap] = tag[swap][:, ::-1]
    c4[swap] = c4[swap][:, ::-1]
    return tag, c4


@gpu
def test_settled_table_is_a_function_of_the_records(monkeypatch):
    """Case 5.  The records of case 2 in three orders.  With the settle pass: the same directory and max_probe; every
    bucket that holds a key outside its home pair — the buckets k_table_settle lays out again by their keys alone —
    reads back as the same bytes, tags and counts; in the other buckets every pair holds the same groups (their order is
    the business of test_settled_table_reads_back_byte_identical_in_every_record_order).  Without it (KM_TABLE_NO_SETTLE) every comparison against the
    models still holds."""
    rec = _synthetic(*CROWDED_HELD)
    seen = _settle_builds(monkeypatch, rec, True)
    first = seen[0][0]
    start = 2 * first["dir"].astype(np.int64)
    off = first["slot"] - first["home"]
    settled = np.zeros(first["S"].size, dtype=bool)
    settled[first["bucket"][(off < 0) | (off > 1)]] = True
    assert settled.sum() >= 8 and (first["kind"][settled] != CLASS).all()
    in_settled = np.repeat(settled, first["S"])
    assert in_settled.size == start[-1]
    tags0, counts0 = _pairs_in_order(first)
    for tab, max_probe in seen[1:]:
        assert max_probe == seen[0][1]
        assert tab["dir"].tobytes() == first["dir"].tobytes()
        assert np.array_equal(tab["tag"][:start[-1]][in_settled], first["tag"][:start[-1]][in_settled])
        assert np.array_equal(tab["c4"][:start[-1]][in_settled], first["c4"][:start[-1]][in_settled])
        tags, counts = _pairs_in_order(tab)
        assert np.array_equal(tags, tags0) and np.array_equal(counts, counts0)
    _settle_builds(monkeypatch, rec, False)


@gpu
def test_settled_table_reads_back_byte_identical_in_every_record_order(monkeypatch):
    """Case 5, the bytes: with the settle pass on, directory, tags and counts read back are byte-identical across the
    three orders, and when the same order is built twice.  k_table_settle lays out the buckets that hold a key outside
    its home pair by their keys alone; in every other bucket k_table_order_pairs puts the two groups that share a home
    pair in tag order.  (Before that pass the race of k_table_insert showed here: against the first build the reversed
    order differed in 48 of 9 104 slots, the permuted one in 60, the same order built again in 32 — each a swap inside
    an aligned pair of a bucket that was not settled.)"""
    rec = _synthetic(*CROWDED_HELD)
    n = rec["keys"].size
    tabs = []
    for order in (np.arange(n), np.arange(n)[::-1], np.random.default_rng(5).permutation(n), np.arange(n)):
        db = _upload(monkeypatch, rec, {"KM_DIR_LOG2": 5}, rec["keys"][order], rec["counts"][order])
        tabs.append(db.debug_table())
        db.close()
    for dir_, tag, c4 in tabs[1:]:
        assert dir_.tobytes() == tabs[0][0].tobytes()
        print("slots whose tag differs from the first order's:", int((tag != tabs[0][1]).sum()))
        assert tag.tobytes() == tabs[0][1].tobytes()
        assert c4.tobytes() == tabs[0][2].tobytes()


# ------------------------------------------------------------------ case 6: degenerate directories
def _small_k_records(k, canonical):
    """The whole key space of synth.small_k_case with EDGE on k-mers the walks discover (on any, where they
    discover too few), and the C oracle's results for those counts."""
    keys, counts, seqs = _sweep_case(k, canonical)
    co = c_oracle.COracle(keys, counts, k, canonical)
    found = set()
    for s in seqs:
        w = _c_want(co, s)
        if w["status"] == 0:
            found |= set(km.canonical(np.array(w["kmers"][len(s) - k + 1:], np.uint64), k).tolist() if canonical
                         else w["kmers"][len(s) - k + 1:])
    found = sorted(found & set(keys.tolist()))
    rest = [x for x in keys.tolist() if x not in found]
    pick = (found[::max(1, len(found) // len(EDGE))] + rest)[:len(EDGE)]
    at = {int(x): i for i, x in enumerate(keys.tolist())}
    counts = counts.copy()
    for x, value in zip(pick, EDGE):
        counts[at[x]] = value
    co = c_oracle.COracle(keys, counts, k, canonical)
    return keys, counts, seqs, co, [_c_want(co, s) for s in seqs]


@gpu
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_degenerate_directories(k, canonical, monkeypatch):
    """Case 6.  The whole key space at k = 2, 3, 4 in sixteen buckets: one to thirteen buckets are used at all, each
    with far more entries than the 2 w classes (NC = 2 or 4); an empty table and a one-record table under the same
    environment.  Lookups over the whole space and the walks of synth.small_k_case."""
    env = {"KM_DIR_LOG2": 4}
    keys, counts, seqs, co, wants = _small_k_records(k, canonical)
    assert set(EDGE) <= set(counts.tolist())
    rec = {"k": k, "canonical": canonical, "keys": keys, "counts": counts}
    db = _upload(monkeypatch, rec, env)
    tab = _read_table(db, rec, env)
    used = tab["entries"] > 0
    w = k - minimizer_len(k)
    assert 1 <= used.sum() <= 13 and (tab["entries"][used] > 2 * w).all() and tab["nc"] == (4 if k == 3 else 2)
    assert np.isin(tab["kind"][used], [CLASS, CROWDED]).all()
    table = dict(zip(keys.tolist(), counts.tolist()))
    space = np.arange(1 << (2 * k), dtype=np.uint64)

    def query(x):
        return _lookup(table, x, k, canonical)
    _check_lookups(db, query, space, k)
    assert sum(x["status"] == 0 for x in wants) >= 6
    _against_c(db, co, k, seqs, ("geometry", k, canonical), wants=wants)
    db.close()
    # nothing stored: every bucket is empty (children_issue_wave then asks for the table's first slots instead)
    none = {"k": k, "canonical": canonical, "keys": keys[:0], "counts": counts[:0]}
    db = _upload(monkeypatch, none, env)
    tab = _read_table(db, none, env)
    assert not tab["S"].any() and db.info.n_groups == 0 and tab["tag"].size == 64
    _check_lookups(db, lambda x: _lookup({}, x, k, canonical), space, k)
    empty_co = c_oracle.COracle(keys[:0], counts[:0], k, canonical)
    _against_c(db, empty_co, k, seqs, ("geometry", k, canonical, "empty"))
    db.close()
    # one record: one or two groups, in buckets that nothing can have doubled
    for x, value in ((int(keys[keys.size // 2]), 65535), (0, 7)):
        one = {"k": k, "canonical": canonical, "keys": np.array([x], np.uint64), "counts": np.array([value], np.uint32)}
        db = _upload(monkeypatch, one, env)
        tab = _read_table(db, one, env)
        assert np.array_equal(tab["S"], shape_capacity(2 * tab["entries"], tab["nc"])) and tab["entries"].sum() <= 2
        assert 1 <= db.info.n_groups <= 2
        _check_lookups(db, lambda p: _lookup({x: value}, p, k, canonical), space, k)
        one_co = c_oracle.COracle(one["keys"], one["counts"], k, canonical)
        _against_c(db, one_co, k, seqs, ("geometry", k, canonical, "one"))
        db.close()
