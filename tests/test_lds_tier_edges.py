"""k_dfs and k_graph at the capacity edges of their LDS tier.

The LDS tier of k_dfs keeps four fixed-size structures per target (km_amd/csrc/tier_geometry.h sizes them for the
batch's longest target): a node set of hs_cap slots filled to 3/4 (set_limit), a position table of pcap slots,
FAST_EXTRA = 160 new nodes, and bcap branch / fcap stack frames.  A target that outgrows one of them is flagged
T_NEEDS_BIG and finished by the large tier.  Both tiers give the same answer, so the oracle cannot tell a target that
took the wrong one: only n_big_tier can, and it is asserted exactly here, from a model.

The model (plain Python, below): the geometry as arithmetic (checked against the library's own code through
tests/host/walk_geometry.hip), the position table's home slots and so the number of target k-mers that lose theirs
(n_losers: they are entered into the node set), and the oracle's depth-first walk with the kernel's book-keeping
beside it — set_count grows with every k-mer the walk meets for the first time, dead ends stay behind as ST_POPPED
tombstones, a full set is rebuilt from nodes + live stack and handed over only if that does not help.

Which guards a target can reach (walk_kernel.h, graph_kernel.h; the CPU tests show each side):
  reachable:   the crowded set at set-up (n_losers + 8 > set_limit), the extra nodes (n_nodes + add > n_ref + 160), the
               full set after a rebuild (live entries + 1 > set_limit), and with max_break >= 513 the 513th branch
               frame (bsp >= bcap) where n_losers + 513 <= set_limit (from 1 028 k-mers on, for a target that loses
               next to no slot); k_graph's n_cand > ccap (step 6: one candidate edge per path, and a dense graph at
               k = 4 has several hundred for fewer than 200 nodes — the large tier's host pass then needs workspaces
               sized by the edges, which it once did not take: test_candidate_edges_* is the regression case)
  unreachable in the LDS tier, for every n_ref it accepts (test_guards_that_geometry_makes_unreachable):
               depth >= fcap, bsp >= bcap while max_break <= 511, k_graph's n > ncap after a walk that stayed,
               3 n > 2 hcap, m > MAXOWN * NT
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from km_amd import kmer as km
from km_amd import lib as kmlib
from km_amd import synth
from test_graph_crossover import _host_program, _lds_tier_limit

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAST_EXTRA = 160
RATIO, COUNT = 0.05, 5
FIELDS = ("status", "n_ref", "probes", "node_off", "node_kmer", "node_count", "path_off", "run_off", "run_start",
          "run_len", "path_len", "path_min_cov")
M64 = (1 << 64) - 1


# ------------------------------------------------------------------ the library's own numbers
GEOMETRY_FIELDS = ("hs_cap", "pcap", "words_cap", "fcap", "bcap", "ncap", "hcap")


@functools.lru_cache(maxsize=None)
def _library_geometry(k, first_len, last_len, max_stack=500, max_break=10):
    """uint32[last_len - first_len + 1, 7]: the geometry of batches whose longest target has first_len .. last_len bases."""
    out = subprocess.run([_host_program("walk_geometry"), str(k), str(first_len), str(max_stack), str(max_break),
                          str(last_len)], capture_output=True, text=True, check=True, timeout=60).stdout
    rows = np.array([[int(x) for x in line.split()] for line in out.splitlines()], dtype=np.int64)
    assert rows.shape == (last_len - first_len + 1, len(GEOMETRY_FIELDS))
    return rows


_tier_limit = _lds_tier_limit             # the most k-mers a target of the LDS tier has (tests/host/lds_tier_limit.hip)


# ------------------------------------------------------------------ the model: geometry
def _round_up(v, m):
    return (v + m - 1) // m * m


def model_geometry(n_ref, max_stack=500, max_break=10):
    """What tier_geometry.h gives a batch whose longest target has n_ref k-mers (n_ref within the tier's limit)."""
    hs_cap = _round_up(((n_ref // 4 + FAST_EXTRA + 64) * 4 + 2) // 3, 64)
    pcap = 64
    while pcap < 4 * n_ref:
        pcap <<= 1
    ncap = n_ref + FAST_EXTRA + 2
    return {"hs_cap": hs_cap, "pcap": pcap, "fcap": _round_up(min(max_stack, 4094) + 2, 2),
            "bcap": min(max_break, 511) + 1, "ncap": ncap, "hcap": _round_up(ncap + ncap // 2 + 1, 64)}


def model_set_limit(k, hs_cap):
    cap = hs_cap - (64 if k == 32 else 0)                       # (k = 32 keeps 64 slots out of the hashed range: ALL_T)
    return 3 * cap // 4


def _prefix32(codes, k):
    """Low 32 bits of the (k-1)-mer prefix of every k-mer of a target (uint8 base codes): its last 16 bases from
    k = 17 on, all of it below."""
    n_ref = len(codes) - k + 1
    w = min(16, k - 1)
    first = k - 1 - w
    v = np.zeros(n_ref, dtype=np.uint64)
    for t in range(w):
        v = (v << np.uint64(2)) | codes[first + t:first + t + n_ref].astype(np.uint64)
    return v


def _pos_home(p32, pcap):
    pshift = 33 - (pcap & -pcap).bit_length()                   # 33 - ffs(pcap)
    return ((p32 * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(pshift)


def model_losers(seq, k, pcap):
    """Target k-mers that do not own their slot of the position table: every occupied slot has exactly one winner."""
    codes = km.encode(seq)
    n_ref = len(codes) - k + 1
    return n_ref - len(np.unique(_pos_home(_prefix32(codes, k), pcap)))


# ------------------------------------------------------------------ the model: the walk and its book-keeping
def _rc(x, k):
    x = ~x & M64
    x = ((x >> 2) & 0x3333333333333333) | ((x & 0x3333333333333333) << 2)
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0F) | ((x & 0x0F0F0F0F0F0F0F0F) << 4)
    return int.from_bytes(x.to_bytes(8, "little"), "big") >> (64 - 2 * k)


class HandOver(Exception):
    pass


def model_walk(seq, k, table, geo, max_stack=500, max_break=10):
    """The oracle's walk (oracle/km_oracle.py: walk) over `table` {canonical k-mer: count}, with what k_dfs books in
    its LDS tier.  -> dict: cause (None: the target stays in the tier; else the guard that hands it over), rebuilds,
    n_new (nodes the walk added), n_losers, set_limit, max_live (most live set entries a push needed)."""
    codes = km.encode(seq).tolist()
    n_ref = len(codes) - k + 1
    kmask = (1 << (2 * k)) - 1
    ref = []
    x = 0
    for i, c in enumerate(codes):
        x = ((x << 2) | c) & kmask
        if i >= k - 1:
            ref.append(x)
    assert len(set(ref)) == n_ref, "repeated k-mer"
    set_limit = model_set_limit(k, geo["hs_cap"])
    n_losers = model_losers(seq, k, geo["pcap"])
    out = {"cause": None, "rebuilds": 0, "n_new": 0, "n_losers": n_losers, "set_limit": set_limit, "max_live": n_losers,
           "n_ref": n_ref}
    if n_losers + 8 > set_limit:
        out["cause"] = "set-up"
        return out
    nodes = set(ref)
    new_nodes = set()
    seen = set()                                                # walk k-mers in the hashed set: live or tombstones
    st = {"reg": 1, "set_count": n_losers}
    stack, onstack = [], set()

    def kids_of(x):
        ys = [((x << 2) | b) & kmask for b in range(4)]
        cs = [table.get(min(y, _rc(y, k)), 0) for y in ys]
        floor = max(sum(cs) * RATIO, COUNT)
        return [y for y, c in zip(ys, cs) if c >= floor]

    def extend(breaks, bsp):
        kids = kids_of(stack[-1])
        if len(kids) > 1:
            breaks += 1
            if breaks > max_break:
                return
        for j, kid in enumerate(kids):
            if kid in nodes or kid in onstack:
                add = len(stack) - st["reg"]
                if add:
                    if out["n_new"] + add > FAST_EXTRA:
                        raise HandOver("extra nodes")
                    for m in stack[st["reg"]:]:
                        nodes.add(m)
                        new_nodes.add(m)
                    out["n_new"] += add
                    st["reg"] = len(stack)
            elif len(stack) + 1 <= max_stack:
                if kid not in seen and st["set_count"] + 1 > set_limit:
                    out["rebuilds"] += 1                        # the tombstones go: nodes + live stack stay
                    seen.clear()
                    seen.update(new_nodes)
                    seen.update(stack[1:])
                    st["set_count"] = n_losers + out["n_new"] + (len(stack) - st["reg"])
                    if st["set_count"] + 1 > set_limit:
                        raise HandOver("set full after a rebuild")
                if len(stack) >= geo["fcap"]:
                    raise HandOver("fcap")
                more = j + 1 < len(kids)
                if more and bsp >= geo["bcap"]:
                    raise HandOver("bcap")
                if kid not in seen:
                    seen.add(kid)
                    st["set_count"] += 1
                stack.append(kid)
                onstack.add(kid)
                out["max_live"] = max(out["max_live"], n_losers + out["n_new"] + (len(stack) - st["reg"]))
                extend(breaks, bsp + 1 if more else bsp)
                stack.pop()
                onstack.discard(kid)
                st["reg"] = min(st["reg"], len(stack))

    deep = sys.getrecursionlimit()
    sys.setrecursionlimit(max(deep, 2 * max_stack + 1000))      # (one Python frame per stack entry)
    try:
        for x in ref:
            stack[:] = [x]
            st["reg"] = 1
            extend(0, 0)
    except HandOver as e:
        out["cause"] = str(e)
    finally:
        sys.setrecursionlimit(deep)
    out["set_count"] = st["set_count"]
    return out


def _table(keys, counts):
    return dict(zip(keys.tolist(), counts.tolist()))


# ------------------------------------------------------------------ cases
def _k1mers(seq, k):
    return [seq[i:i + k - 1] for i in range(len(seq) - k + 2)]


def _grow_off_target(pool, own, n, k):
    """n new bases whose (k-1)-mers the pool has not handed out (a longer sequence's tail: n may be below k - 1)."""
    g = pool.grow(n + k - 1)
    own.update(_k1mers(g, k))
    return g[-n:]


def _feature_case(pool, name, n_ref, feats, cov=(60, 30)):
    """A target of n_ref k-mers and, in target order, one read per feature:
      ("dead", d)          leaves the target for d bases and ends: d k-mers that pass the keep rule and lead nowhere
      ("tail", x, TAIL)    a dead end of x bases that runs into the sequence TAIL (shared between several of them)
      ("ins", n)           an insertion of n bases: n + k - 1 k-mers that become nodes
      ("t32", x, y)        k = 32: a dead end of x bases, then T^32, then y more
    -> dict(name, target, reads, feats: what was planted where)."""
    k = pool.k
    T = pool.grow(n_ref + k - 1)
    own = set(_k1mers(T, k))
    reads = [(T, cov[0])]
    if callable(feats):
        feats = feats(T)
    step = (n_ref - k - 10) // len(feats)                       # (the last one at least k + 10 bases before the end)
    planted = []
    def body_of(f):
        if f[0] in ("ins", "dead"):
            return _grow_off_target(pool, own, f[1], k)
        if f[0] == "tail":
            own.update(_k1mers(f[2], k))
            return _grow_off_target(pool, own, f[1], k) + f[2]
        while True:
            head, rest = _grow_off_target(pool, own, f[1], k), _grow_off_target(pool, own, f[2], k)
            if head[-1] != "T" and rest[0] != "T":
                break
        own.add("T" * (k - 1))                                  # (the one (k-1)-mer the cases of a batch share)
        return head + "T" * 32 + rest

    for j, f in enumerate(feats):
        p = k + 1 + j * step
        body = body_of(f)
        tries = 0
        while True:
            if p >= k + 1 + (j + 1) * step:                     # (no place admits this body: another one)
                tries += 1
                assert tries < 20, "no room for the feature"
                p, body = k + 1 + j * step, body_of(f)
            hap = T[:p] + body + (T[p:] if f[0] == "ins" else "")
            if body[0] != T[p] and (f[0] != "ins" or body[-1] != T[p - 1]) and pool.admit(own, hap):
                break
            p += 1
        reads.append((hap, cov[1]))
        again = f[0] == "tail" and any(g[0] == "tail" for g in planted)      # (a shared tail counts once)
        planted.append((f[0], p, len(body) - (len(f[2]) if again else 0)))
    return {"name": name, "target": T, "reads": reads, "feats": planted, "k": k}


def _batch(cases, k, max_stack=500, max_break=10):
    """One table for the cases of a batch, the geometry their longest target fixes, and the model's verdicts."""
    keys, counts = synth.records_from_reads([r for c in cases for r in c["reads"]], k)
    n_max = max(len(c["target"]) for c in cases) - k + 1
    assert n_max <= _tier_limit(k, max_break)
    geo = model_geometry(n_max, max_stack, max_break)
    table = _table(keys, counts)
    models = [model_walk(c["target"], k, table, geo, max_stack, max_break) for c in cases]
    return {"k": k, "cases": cases, "keys": keys, "counts": counts, "geo": geo, "models": models,
            "max_stack": max_stack, "max_break": max_break}


# ---- a. extra nodes
@functools.lru_cache(maxsize=None)
def _extra_node_batch(k):
    pool = synth.DistinctPool(k, 7100 + k)
    long_, short = 240, 200                                     # k-mers: the 160 case is the batch's longest target
    one = lambda name, n_ref, new: _feature_case(pool, name, n_ref, [("ins", new - (k - 1))])
    two = lambda name, a, b: _feature_case(pool, name, long_ - 5, [("ins", a - (k - 1)), ("ins", b - (k - 1))])
    cases = [one("new159", long_ - 5, 159), one("new160_longest", long_, 160), one("new161", long_ - 5, 161),
             one("short_new160", short, 160), one("short_new161", short, 161),
             two("two_80_80", 80, 80), two("two_80_81", 80, 81)]
    return _batch(cases, k)


# ---- b. a crowded position table
def _steered_target(k, n_ref, pcap, want_losers, taken, rng, depth=4):
    """A target of n_ref k-mers, built base by base: while fewer than want_losers k-mers have lost their slot of the
    position table, the next base is the first of the `depth`-base extension whose prefixes land in the most slots
    already taken; from then on a base whose prefix lands in a free slot.  No (k-1)-mer repeats on either strand (in
    `taken` either, which is extended), so no k-mer does."""
    w = min(16, k - 1)
    mask = (1 << (2 * w)) - 1
    pshift = 33 - (pcap & -pcap).bit_length()
    home = lambda v: ((v * 0x9E3779B1) & 0xFFFFFFFF) >> pshift
    occupied = np.zeros(pcap, dtype=bool)
    while True:
        seq = "".join("ACGT"[i] for i in rng.integers(0, 4, k - 2))
        if "AAAA" not in seq and "TTTT" not in seq:
            break
    mine = set()
    losers = 0
    v = 0
    for ch in seq:
        v = ((v << 2) | "ACGT".index(ch)) & mask
    for _ in range(n_ref):                                      # each base completes the prefix of one more k-mer
        if losers < want_losers:
            vs = np.array([v], dtype=np.uint64)
            score = np.zeros(1, dtype=np.int64)
            for d in range(depth):
                vs = ((vs[:, None] << np.uint64(2)) | np.arange(4, dtype=np.uint64)[None, :]).reshape(-1) & np.uint64(mask)
                hit = occupied[((vs * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(pshift)]
                score = np.repeat(score, 4) + hit
            best = score.reshape(4, -1).max(axis=1) * 2 + occupied[[home(((v << 2) | b) & mask) for b in range(4)]]
            order = np.argsort(-best, kind="stable").tolist()
        else:                                                   # (a taken slot only if all four are)
            order = sorted(rng.permutation(4).tolist(), key=lambda b: bool(occupied[home(((v << 2) | b) & mask)]))
        for b in order:
            mer = (seq + "ACGT"[b])[-(k - 1):]
            r = synth.revcomp_str(mer)
            if mer != r and mer not in taken and r not in taken and mer not in mine and r not in mine:
                break
        else:
            raise AssertionError("dead end while steering")
        mine.update((mer, r))
        seq += "ACGT"[b]
        v = ((v << 2) | b) & mask
        slot = home(v)
        losers += int(occupied[slot])
        occupied[slot] = True
    taken |= mine
    for b in rng.permutation(4).tolist():                       # the last base: it completes no prefix
        mer = (seq + "ACGT"[b])[-(k - 1):]
        r = synth.revcomp_str(mer)
        if mer != r and mer not in taken and r not in taken:
            taken.update((mer, r))
            return seq + "ACGT"[b], losers
    raise AssertionError("dead end at the last base")


CROWDED_N_REF = 1000


@functools.lru_cache(maxsize=None)
def _crowded_batch(k):
    """Three targets of 1 000 k-mers: n_losers == set_limit - 8 with a dead end of 8 k-mers (fits: the set ends exactly
    full), the same with a dead end of 9 (the ninth finds the set full, the rebuild frees nothing: everything in it is
    a loser or on the live stack), and n_losers == set_limit - 7 (handed over at set-up).  (A room of 8 holds no
    variant that becomes nodes — the shortest has k - 1 k-mers; new nodes plus stack at the exact edge are the
    ins_room_* cases of the rebuild shapes.)"""
    rng = np.random.default_rng(9100 + k)
    geo = model_geometry(CROWDED_N_REF)
    limit = model_set_limit(k, geo["hs_cap"])
    taken = set()
    cases = []
    for name, losers, dead in (("room8_dead8", limit - 8, 8), ("room8_dead9", limit - 8, 9), ("room7", limit - 7, 8)):
        T, got = _steered_target(k, CROWDED_N_REF, geo["pcap"], losers, taken, rng)
        assert got == losers, (name, got, losers)
        p = len(T) // 2
        while True:                                             # the dead end: `dead` bases that leave the target at p
            tail = "".join("ACGT"[i] for i in rng.integers(0, 4, dead))
            mers = _k1mers(T[p - (k - 2):p] + tail, k)
            both = set(mers) | {synth.revcomp_str(m) for m in mers}
            if tail[0] != T[p] and len(both) == 2 * len(mers) and not both & taken:
                break
        taken |= both
        cases.append({"name": name, "target": T, "reads": [(T, 60), (T[:p] + tail, 30)], "k": k,
                      "feats": [("dead", p, dead)], "want_losers": losers})
    return _batch(cases, k)


# ---- c. the tombstone rebuild
REBUILD_N_REF = 130


def _dead_end_target(pool, name, first_room, d2=100, d3=100):
    """Three dead ends; the first one's length leaves the third `first_room` free set entries when its walk begins."""
    k = pool.k
    geo = model_geometry(REBUILD_N_REF)
    limit = model_set_limit(k, geo["hs_cap"])

    def feats(T):                                               # (the target's losers fix the first dead end's length)
        return [("dead", limit - model_losers(T, k, geo["pcap"]) - d2 - first_room), ("dead", d2), ("dead", d3)]
    return _feature_case(pool, name, REBUILD_N_REF, feats)


def _ins_then_room(T, over):
    geo = model_geometry(REBUILD_N_REF)
    room = model_set_limit(31, geo["hs_cap"]) - model_losers(T, 31, geo["pcap"])
    return [("ins", 30), ("dead", 50), ("dead", room - (30 + 31 - 1) + over)]


@functools.lru_cache(maxsize=None)
def _rebuild_batch(kind):
    if kind == "phases":                                        # room64 of the third dead end's runs: 0, 1, .. 64 and beyond
        pool = synth.DistinctPool(31, 5531)
        return _batch([_dead_end_target(pool, "room%d" % r, r) for r in range(68)], 31)
    if kind == "shapes":
        pool = synth.DistinctPool(31, 5532)
        tail = pool.grow(90)
        cases = [
            _feature_case(pool, "three_dead_ends", REBUILD_N_REF, [("dead", 100), ("dead", 100), ("dead", 100)]),
            # two rebuilds: the second finds the set as the first left it (had that one entered the owners of a
            # position-table slot as well, 122 entries nobody counted would fill the set's 384 slots here)
            _feature_case(pool, "five_dead_ends", REBUILD_N_REF, [("dead", 100)] * 5),
            _feature_case(pool, "one_too_long", REBUILD_N_REF, [("dead", 300)]),
            # the tail is walked, found again as a tombstone, dropped by the rebuild inside the long dead end, walked anew
            _feature_case(pool, "shared_tail", REBUILD_N_REF, [("tail", 40, tail), ("tail", 50, tail), ("dead", 150), ("tail", 30, tail)]),
            _feature_case(pool, "ins_before", REBUILD_N_REF, [("ins", 30), ("dead", 110), ("dead", 110), ("dead", 60)]),
            _feature_case(pool, "ins_after", REBUILD_N_REF, [("dead", 110), ("dead", 110), ("dead", 60), ("ins", 30)]),
            # new nodes plus stack at the exact edge of the recount after a rebuild: the insertion's 60 nodes, 50
            # tombstones that the rebuild drops, and a last dead end that ends with the set exactly full / one past it
            _feature_case(pool, "ins_room_exact", REBUILD_N_REF, lambda T: _ins_then_room(T, 0)),
            _feature_case(pool, "ins_room_plus1", REBUILD_N_REF, lambda T: _ins_then_room(T, 1)),
        ]
        return _batch(cases, 31)
    pool = synth.DistinctPool(32, 5533)                         # "k32": the same at k = 32, one dead end through T^32
    cases = [
        _feature_case(pool, "t32_then_rebuild", REBUILD_N_REF, [("t32", 20, 70), ("dead", 100), ("dead", 100), ("dead", 60)]),
        _feature_case(pool, "rebuild_then_t32", REBUILD_N_REF, [("dead", 100), ("dead", 100), ("dead", 60), ("t32", 20, 70)]),
    ]
    return _batch(cases, 32)


# ---- d. branch frames
COMB_N_REF = 1416                                               # the tier's longest target: set_limit 624
COMB_TEETH = (511, 512, 513)
COMB_MAX_STACK = 530


@functools.lru_cache(maxsize=None)
def _comb_cases():
    """Three targets of 1 416 k-mers (k = 31) steered AWAY from taken slots of the position table (hardly a loser: the
    set has room for a live stack of more than 512), each with a dead-end comb: a chain of T k-mers that leaves the
    target on a base below the target's own (so the seed keeps a branch frame), every chain k-mer with a second
    child, a leaf of a higher base that has no child.  The walk goes down the chain first: one more branch frame a
    step."""
    k = 31
    rng = np.random.default_rng(4400)
    pcap = model_geometry(COMB_N_REF)["pcap"]
    taken = set()
    cases = []

    def free(mer, also=()):
        r = synth.revcomp_str(mer)
        return mer != r and not {mer, r} & taken and mer not in also and r not in also
    for teeth in COMB_TEETH:
        T, _ = _steered_target(k, COMB_N_REF, pcap, 0, taken, rng)
        p = 100
        while T[p] == "A":
            p += 1
        while True:
            hap, leaves, mine, ok = T[:p], [], set(), True
            for j in range(teeth):
                for _ in range(20):
                    c = "A" if j == 0 else "ACG"[rng.integers(0, 3)]
                    leaf = "ACGT"[rng.integers("ACGT".index(c) + 1, 4)]
                    mc, ml = hap[-(k - 2):] + c, hap[-(k - 2):] + leaf
                    if free(mc, mine) and (j == 0 or free(ml, mine)):
                        break
                else:
                    ok = False
                    break
                mine.update((mc, synth.revcomp_str(mc)))
                if j:                                           # (the chain's first k-mer shares its parent with the target)
                    mine.update((ml, synth.revcomp_str(ml)))
                    leaves.append(hap[-(k - 1):] + leaf)
                hap += c
            if ok:
                break
            p += 1                                              # (this place does not admit a comb: the next one)
            while T[p] == "A":
                p += 1
        taken |= mine
        cases.append({"name": "comb%d" % teeth, "target": T, "k": k, "feats": [("comb", p, teeth)],
                      "reads": [(T, 60), (hap, 30)] + [(x, 30) for x in leaves]})
    return cases


@functools.lru_cache(maxsize=None)
def _comb_batch(max_break):
    return _batch(_comb_cases(), 31, max_stack=COMB_MAX_STACK, max_break=max_break)


# ---- f. candidate edges of k_graph
DENSE_K, DENSE_SEED = 4, 40


def _de_bruijn(k):
    """A sequence over ACGT in which every k-mer occurs exactly once (4^k + k - 1 bases): any piece of it is a target
    without a repeated k-mer."""
    a, out = [0] * (4 * k), []

    def db(t, p):
        if t > k:
            if k % p == 0:
                out.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    s = "".join("ACGT"[i] for i in out)
    return s + s[:k - 1]


@functools.lru_cache(maxsize=None)
def _dense_case():
    """k = 4: a target of 29 k-mers in a table that holds two thirds of all 4-mers.  The walk adds no more than 160
    nodes, but among some 180 of the 256 k-mers there are nearly every node has several successors: far more
    candidate edges (one path each) than nodes.  -> (case, the oracle's number of paths)."""
    from oracle import c_oracle
    k = DENSE_K
    rng = np.random.default_rng(DENSE_SEED)
    space = np.arange(1 << (2 * k), dtype=np.uint64)
    space = space[space <= km.revcomp(space, k)]
    n_ref = int(rng.integers(15, 40))
    T = synth.unique_kmer_seq(rng, n_ref + k - 1, k)
    frac = rng.uniform(0.3, 0.95)
    extra = space[rng.random(space.size) < frac]
    acc = {int(x): 60 for x in km.canonical(km.sliding_kmers(km.encode(T), k), k).tolist()}
    for x in extra.tolist():
        acc.setdefault(int(x), 30)
    keys = np.array(sorted(acc), dtype=np.uint64)
    counts = np.array([acc[x] for x in keys.tolist()], dtype=np.uint32)
    w = c_oracle.COracle(keys, counts, k).analyse(km.encode(T), ratio=RATIO, count=COUNT)
    assert w["status"] == 0 and w["kmers"].size - w["n_ref"] <= FAST_EXTRA
    return {"name": "dense", "target": T, "k": k, "keys": keys, "counts": counts, "feats": []}, len(w["paths"])


@functools.lru_cache(maxsize=None)
def _dense_batch(over):
    """The dense target and a longer one beside it (a piece of a de Bruijn sequence) that sets the batch's ncap — and
    with it ccap, the candidate edges step 6 of k_graph has room for — to the dense target's number of paths (`over`
    0: n_cand == ccap) or to one less (`over` 1)."""
    case, n_paths = _dense_case()
    n_long = n_paths - over - (FAST_EXTRA + 2)
    filler = {"name": "long", "target": _de_bruijn(DENSE_K)[:n_long + DENSE_K - 1], "k": DENSE_K, "feats": []}
    cases = [case, filler]
    geo = model_geometry(n_long)
    table = _table(case["keys"], case["counts"])
    models = [model_walk(c["target"], DENSE_K, table, geo) for c in cases]
    return {"k": DENSE_K, "cases": cases, "keys": case["keys"], "counts": case["counts"], "geo": geo, "models": models,
            "max_stack": 500, "max_break": 10}


# ------------------------------------------------------------------ CPU: the model against the library
@pytest.mark.parametrize("k", [11, 16, 17, 21, 31, 32])
def test_geometry_model_equals_the_librarys_numbers(k):
    limit = _tier_limit(k)
    assert limit == 1416
    for max_stack, max_break in ((500, 10), (40, 3), (5000, 600)):
        rows = _library_geometry(k, k, limit + k - 1, max_stack, max_break)
        assert limit == _tier_limit(k, max_break)
        for n_ref in (1, 2, 63, 64, 65, 130, 240, 255, 256, 257, 700, 1000, 1023, 1024, 1025, limit - 1, limit):
            want = model_geometry(n_ref, max_stack, max_break)
            got = dict(zip(GEOMETRY_FIELDS, rows[n_ref - 1].tolist()))
            assert {f: got[f] for f in want} == want, (k, n_ref, max_stack, max_break)
        # a longer target leaves the batch with the geometry of the limit
        beyond = _library_geometry(k, limit + k + 50, limit + k + 50, max_stack, max_break)[0]
        assert beyond.tolist() == rows[limit - 1].tolist()


def test_model_helpers():
    rng = np.random.default_rng(3)
    for k in (11, 16, 17, 21, 31, 32):
        xs = rng.integers(0, 1 << 63, 50, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        xs = np.append(xs, np.uint64(M64)) & np.uint64((1 << (2 * k)) - 1)
        assert [_rc(int(x), k) for x in xs] == km.revcomp(xs, k).tolist()
        seq = synth.random_seq(rng, 200)
        codes = km.encode(seq)
        w = min(16, k - 1)
        for i in (0, 1, 57, 200 - k):
            assert int(_prefix32(codes, k)[i]) == int(km.pack_str(seq[i + k - 1 - w:i + k - 1]))


def test_guards_that_geometry_makes_unreachable():
    """For every n_ref the LDS tier accepts, at every k the batch could have:
      depth >= fcap: the walk pushes at depth + 1 <= max_stack only and fcap >= max_stack + 2 while max_stack <= 4094;
        beyond that the node set would have to hold 4 096 live entries, and set_limit never reaches 1 000;
      bsp >= bcap: bsp <= max_break < bcap while max_break <= 511 (beyond that it CAN fire: test_comb_* below);
      k_graph after a walk that stayed (m <= n_ref + 160): n = m + 2 <= ncap, 3 n <= 2 hcap, m <= MAXOWN * NT."""
    for k in (11, 16, 21, 31, 32):
        limit = _tier_limit(k, 600)
        assert limit == _tier_limit(k, 10) == 1416
        for max_stack, max_break in ((500, 10), (4094, 511), (100000, 100000)):
            rows = _library_geometry(k, k, limit + k - 1, max_stack, max_break)
            g = dict(zip(GEOMETRY_FIELDS, rows.T))
            set_limit = 3 * (g["hs_cap"] - (64 if k == 32 else 0)) // 4
            assert (g["fcap"] >= min(max_stack, 4094) + 2).all()
            assert set_limit.max() < 1000 < 4096
            assert (g["bcap"] == min(max_break, 511) + 1).all()
            n_ref = np.arange(1, limit + 1)
            n = n_ref + FAST_EXTRA + 2                          # the most nodes + source + sink k_graph sees
            assert (n <= g["ncap"]).all() and (3 * n <= 2 * g["hcap"]).all()
            assert (2 * g["hcap"] >= 3 * g["ncap"] + 1).all()   # hcap >= ncap + floor(ncap / 2) + 1
            assert (n - 2 <= 8 * 256).all()                     # MAXOWN * NT (graph_kernel.h; NT read below)
    with open(os.path.join(ROOT, "km_amd", "csrc", "graph_kernel.h")) as fh:
        text = fh.read()
    assert re.search(r"constexpr uint32_t MAXOWN = 8;", text)
    assert re.findall(r"constexpr uint32_t GRAPH_THREADS = (\d+);", text) == ["256"]
    assert "NT = GRAPH_THREADS" in text


def _assert_oracle_accepts(batch):
    from oracle import c_oracle
    co = c_oracle.COracle(batch["keys"], batch["counts"], batch["k"])
    wants = []
    for c in batch["cases"]:
        w = co.analyse(km.encode(c["target"]), ratio=RATIO, count=COUNT, max_stack=batch["max_stack"],
                       max_break=batch["max_break"])
        assert w["status"] == 0, c["name"]                      # (no repeated k-mer)
        wants.append(w)
    return wants


@functools.lru_cache(maxsize=None)
def _wants(maker, arg):
    return _assert_oracle_accepts(maker(arg))


@pytest.mark.parametrize("k", [21, 31])
def test_extra_node_cases_sit_on_their_side_of_160(k):
    b = _extra_node_batch(k)
    wants = _wants(_extra_node_batch, k)
    new = [w["kmers"].size - w["n_ref"] for w in wants]
    assert new == [159, 160, 161, 160, 161, 160, 161]
    assert [m["cause"] for m in b["models"]] == [None, None, "extra nodes", None, "extra nodes", None, "extra nodes"]
    n_refs = [w["n_ref"] for w in wants]
    assert n_refs[1] == max(n_refs) and n_refs[1] + 160 + 2 == b["geo"]["ncap"]          # k_graph at n == ncap
    assert n_refs[3] == n_refs[4] == n_refs[1] - 40
    for c in b["cases"][5:]:                                    # two bookings: the second with n_nodes > n_ref already
        assert [f[0] for f in c["feats"]] == ["ins", "ins"]
    assert all(m["max_live"] + 1 <= m["set_limit"] for m in b["models"])                  # (the set is not what hands them over)


@pytest.mark.parametrize("k", [16, 21, 32])
def test_crowded_cases_sit_on_their_side_of_the_set_limit(k):
    b = _crowded_batch(k)
    _wants(_crowded_batch, k)
    limit = model_set_limit(k, b["geo"]["hs_cap"])
    assert b["geo"] == model_geometry(CROWDED_N_REF) and (k != 32 or limit == 3 * (b["geo"]["hs_cap"] - 64) // 4)
    got = [(m["n_losers"], m["cause"], m["rebuilds"]) for m in b["models"]]
    assert got == [(limit - 8, None, 0), (limit - 8, "set full after a rebuild", 1), (limit - 7, "set-up", 0)]
    assert b["models"][0]["set_count"] == limit and b["models"][0]["max_live"] == limit


@pytest.mark.parametrize("kind", ["phases", "shapes", "k32"])
def test_rebuild_cases_need_the_rebuild(kind):
    b = _rebuild_batch(kind)
    wants = _wants(_rebuild_batch, kind)
    by = {c["name"]: (c, m, w) for c, m, w in zip(b["cases"], b["models"], wants)}
    for name, (c, m, w) in by.items():
        planted = sum(n + (b["k"] - 1 if f == "ins" else 0) for f, _, n in c["feats"])
        if name == "one_too_long":
            assert m["cause"] == "set full after a rebuild" and m["rebuilds"] == 1
            continue
        if name.startswith("ins_room"):
            # (one rebuild drops the 50 tombstones; one past the edge a second one finds nothing to drop)
            assert m["n_new"] == 60 and m["rebuilds"] == (1 if name == "ins_room_exact" else 2), (name, m)
            assert (m["cause"], m["max_live"]) == ((None, m["set_limit"]) if name == "ins_room_exact" else
                                                   ("set full after a rebuild", m["set_limit"])), (name, m)
            continue
        # all the planted k-mers do not fit the set, what is alive at any one time does: only a rebuild gets it through
        assert m["cause"] is None and m["rebuilds"] >= 1, (name, m)
        assert m["n_losers"] + planted > m["set_limit"], (name, m, planted)
        assert m["max_live"] + 1 <= m["set_limit"], (name, m)
    if kind == "phases":
        for r, (c, m) in enumerate(zip(b["cases"], b["models"])):
            d1, d2 = c["feats"][0][2], c["feats"][1][2]
            assert m["set_limit"] - m["n_losers"] - d1 - d2 == r and m["rebuilds"] == 1 and m["n_new"] == 0
    elif kind == "shapes":
        assert by["ins_before"][1]["n_new"] == by["ins_after"][1]["n_new"] == 30 + 31 - 1
        assert by["shared_tail"][1]["rebuilds"] == 1
        c, m, w = by["five_dead_ends"]
        owners = m["n_ref"] - m["n_losers"]
        assert m["rebuilds"] == 2 and m["set_limit"] + owners > b["geo"]["hs_cap"]
    else:
        t32 = (1 << 64) - 1
        for name in by:
            assert t32 in by[name][2]["kmers"].tolist(), name   # T^32 became a node (its own child: a loop)


def test_comb_reaches_the_branch_frame_guard_only_past_max_break_511():
    """bsp >= bcap (walk_kernel.h): bsp <= max_break < bcap while max_break <= 511, and with max_break = 512 the break
    budget still ends the chain one step before frame 513.  Past that the guard fires — if the set does not hand the
    target over first: the 513th chain k-mer is pushed with 512 live entries on the stack and passes the set's own
    check only while n_losers + 513 <= set_limit.  set_limit reaches 528 at n_ref = 1 028 (room for 15 losers), 576 at
    1 220 and 624 from 1 412 on; a random target of 1 416 k-mers loses some 115 slots and fits none of them, so the
    targets here are steered to lose next to none."""
    rows = _library_geometry(31, 31, COMB_N_REF + 30, COMB_MAX_STACK, 600)
    limits = 3 * rows[:, 0] // 4
    assert (limits[:1027] < 513).all() and (limits[1027:1219] == 528).all() and (limits[1219:1411] == 576).all()
    assert (limits[1411:] == 624).all()
    for m in _comb_batch(600)["models"]:
        assert m["n_losers"] + 513 <= m["set_limit"] == 624
    seen = {}
    for max_break in (511, 512, 600):
        b = _comb_batch(max_break)
        _wants(_comb_batch, max_break)
        assert b["geo"]["bcap"] == 512 and b["geo"]["fcap"] == COMB_MAX_STACK + 2
        for teeth, m in zip(COMB_TEETH, b["models"]):
            assert m["n_losers"] <= 8 and m["n_new"] == 0
            seen[(teeth, max_break)] = m["cause"]
    assert {key for key, cause in seen.items() if cause is not None} == {(513, 600)}
    assert seen[(513, 600)] == "bcap"
    # the ones that stay walk the whole comb: the set fills with popped leaves and is rebuilt on the way back up
    assert all(m["rebuilds"] >= 1 for m in _comb_batch(512)["models"])


def test_dense_case_sits_on_both_sides_of_the_candidate_capacity():
    """n_cand > ccap (graph_kernel.h, step 6; ccap = ncap): k_graph emits one path per candidate edge (t_npaths =
    n_cand), so a target's n_cand is the oracle's number of paths.  Nothing bounds it by ncap: at k = 4 a walk of no
    more than 160 new nodes gives several hundred paths.  The batch's longest target sets ncap, so the same dense
    target sits at n_cand == ccap beside one long target and at ccap + 1 beside a target one k-mer shorter; its walk
    stays in the LDS tier both times, so it is k_graph of that tier that meets it."""
    case, n_paths = _dense_case()
    n_ref = len(case["target"]) - DENSE_K + 1
    assert n_paths > n_ref + FAST_EXTRA + 2 + 100               # (far beyond what its own length would allow)
    for over in (0, 1):
        b = _dense_batch(over)
        wants = _wants(_dense_batch, over)
        assert len(wants[0]["paths"]) == n_paths == b["geo"]["ncap"] + over
        assert wants[0]["kmers"].size - n_ref == b["models"][0]["n_new"] <= FAST_EXTRA
        assert b["models"][0]["cause"] is None, b["models"][0]
        assert len(b["cases"][1]["target"]) - DENSE_K + 1 + FAST_EXTRA + 2 == b["geo"]["ncap"]
        # (the long target runs through the same dense table: far past the edge itself, whichever tier walks it)
        assert len(wants[1]["paths"]) > b["geo"]["ncap"] + 100


# ------------------------------------------------------------------ GPU
def _run(batch, n_runs):
    seqs = [c["target"] for c in batch["cases"]]
    k = batch["k"]
    db = kmlib.Database.from_records(batch["keys"], batch["counts"], k).upload(0)
    b = kmlib.Batch(db, ratio=RATIO, count=COUNT, max_stack=batch["max_stack"], max_break=batch["max_break"],
                    max_targets=len(seqs), max_total_bases=sum(len(s) for s in seqs))
    b.set_targets(seqs)
    out = []
    for _ in range(n_runs):
        b.run()
        out.append(b.fetch())
    b.close()
    db.close()
    return out


def _check(r, wants, tag):
    noff, poff = r["node_off"].astype(np.int64), r["path_off"].astype(np.int64)
    assert len(r["status"]) == len(wants)
    for t, want in enumerate(wants):
        assert int(r["status"][t]) == 0, (tag, t)
        assert int(r["n_ref"][t]) == want["n_ref"], (tag, t)
        assert np.array_equal(r["node_kmer"][noff[t]:noff[t + 1]], want["kmers"]), (tag, t)
        assert np.array_equal(r["node_count"][noff[t]:noff[t + 1]], want["counts"]), (tag, t)
        assert int(r["probes"][t]) == want["probes"], (tag, t)
        got = [kmlib.expand_path(r, p).tolist() for p in range(poff[t], poff[t + 1])]
        assert got == [list(p) for p in want["paths"]], (tag, t)
        assert r["path_min_cov"][poff[t]:poff[t + 1]].tolist() == list(want["min_cov"]), (tag, t)


def _both_tiers(batch, wants, monkeypatch):
    """The batch on a fresh workspace, twice (the host finishes the large tier's targets of a workspace's first run,
    the device's own large tier those of the second), and on one made with KM_BIG_DEVICE_OFF=1 (read at every
    km_batch_create): the oracle's answer and the model's n_big_tier every time, identical arrays."""
    n_big = sum(m["cause"] is not None for m in batch["models"])
    monkeypatch.delenv("KM_BIG_DEVICE_OFF", raising=False)
    monkeypatch.delenv("KM_BIG_DEVICE", raising=False)
    first, second = _run(batch, 2)
    monkeypatch.setenv("KM_BIG_DEVICE_OFF", "1")
    host, = _run(batch, 1)
    for tag, r in (("first run", first), ("device tier", second), ("KM_BIG_DEVICE_OFF=1", host)):
        _check(r, wants, tag)
    for tag, r in (("first run", first), ("device tier", second), ("KM_BIG_DEVICE_OFF=1", host)):
        assert int(r["n_big_tier"]) == n_big, (tag, [m["cause"] for m in batch["models"]])
        for name in FIELDS:
            assert np.array_equal(first[name], r[name]), (tag, name)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 31])
def test_extra_nodes_at_159_160_161(k, monkeypatch):
    """n_nodes + add > n_ref + 160 (k_dfs) with one insertion and with two, in the batch's longest target (k_graph then
    runs at n == ncap) and in one 40 k-mers shorter."""
    _both_tiers(_extra_node_batch(k), _wants(_extra_node_batch, k), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 21, 32])
def test_crowded_position_table_at_the_set_limit(k, monkeypatch):
    """n_losers + 8 > set_limit at set-up, and a set that ends exactly full / one short: the whole-prefix hash
    (k = 16), the 16-base suffix (k = 21), cap = hs_cap - 64 (k = 32)."""
    _both_tiers(_crowded_batch(k), _wants(_crowded_batch, k), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("over", [0, 1])
def test_candidate_edges_at_ccap_and_one_past_it(over, monkeypatch):
    """The dense k = 4 target with exactly ccap candidate edges (k_graph of the LDS tier emits them all) and with
    ccap + 1 (it hands the target to the large tier's graph pass).  n_big_tier counts the large tier's walks only, so
    it says that the walk stayed; which graph pass answered shows in no figure the library hands out — the paths,
    all several hundred of them, must be the oracle's either way."""
    _both_tiers(_dense_batch(over), _wants(_dense_batch, over), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("max_break", [511, 512, 600])
def test_comb_of_511_512_513_branch_frames(max_break, monkeypatch):
    """A dead-end comb of 511, 512 and 513 teeth under a stack budget of 530: 512 branch frames fit the LDS tier, the
    513th (max_break = 600 only) hands the target over."""
    _both_tiers(_comb_batch(max_break), _wants(_comb_batch, max_break), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["phases", "shapes", "k32"])
def test_tombstone_rebuild(kind, monkeypatch):
    """The rebuild of the node set that drops ST_POPPED tombstones: at every offset of a chain run (phases), when it
    succeeds, when it cannot help, around a dead-end tail two branches share and around a variant that becomes nodes
    (shapes), and with T^32 in its slot outside the hashed range (k32)."""
    _both_tiers(_rebuild_batch(kind), _wants(_rebuild_batch, kind), monkeypatch)
