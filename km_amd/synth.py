"""Seeded synthetic workloads: random targets, a
canonical k-mer count table with injected variants / noise / padding.

The generator is the build's own; nothing here comes from the reference.  It is
used by bench.py (full size), by the GPU parity tests and by
tests/golden/make_golden.py (small slices that are also run through the
reference to produce committed golden TSVs).
"""

import hashlib
import json
import os

import numpy as np

from . import kmer as km

HEADLINE_SEED = 20260101


def _unique_kmer_rows(rng, n, length, k):
    """n random ACGT rows of `length` with no repeated k-mer inside a row
    (the reference raises ValueError on those: km/utils/common.py:55-59)."""
    rows = rng.integers(0, 4, size=(n, length), dtype=np.uint8)
    while True:
        kms = np.sort(km.sliding_kmers(rows, k), axis=1)
        bad = np.nonzero((kms[:, 1:] == kms[:, :-1]).any(axis=1))[0]
        if bad.size == 0:
            return rows
        rows[bad] = rng.integers(0, 4, size=(bad.size, length), dtype=np.uint8)


def _mutate(rng, row, kind, k):
    """Return (mutated_row, site_lo, site_hi): ref bases [site_lo, site_hi) are
    replaced.  Sites keep k-1 flanking bases on both sides so the variant path
    rejoins the target."""
    L = row.size
    lo_ok, hi_ok = k, L - k
    if kind == "snv":
        p = int(rng.integers(lo_ok, hi_ok))
        b = (int(row[p]) + int(rng.integers(1, 4))) % 4
        return np.concatenate([row[:p], [b], row[p + 1:]]).astype(np.uint8), p, p + 1
    if kind == "ins":
        n = int(rng.integers(1, 31))
        p = int(rng.integers(lo_ok, hi_ok))
        ins = rng.integers(0, 4, size=n, dtype=np.uint8)
        return np.concatenate([row[:p], ins, row[p:]]).astype(np.uint8), p, p
    if kind == "del":
        n = int(rng.integers(1, 31))
        p = int(rng.integers(lo_ok, max(lo_ok + 1, hi_ok - n)))
        return np.concatenate([row[:p], row[p + n:]]).astype(np.uint8), p, p + n
    if kind == "dup":  # tandem duplication of row[p:p+n] inserted right after itself
        n = int(rng.integers(20, 101))
        n = min(n, L - 2 * k - 1)
        p = int(rng.integers(lo_ok, max(lo_ok + 1, hi_ok - n)))
        return np.concatenate([row[:p + n], row[p:p + n], row[p + n:]]).astype(np.uint8), p + n, p + n
    raise ValueError(kind)


def make_case(n_targets=100, length=500, k=31, n_keys=200_000, seed=HEADLINE_SEED,
              variant_frac=0.30, variants_per_target=(1, 1), vaf=(0.1, 0.6),
              kinds=("snv", "ins", "del", "dup"), noise_frac=0.01, noise_counts=(2, 5),
              cov=(50, 2000), hom_frac=0.0, branch_noise_frac=0.0, name=None,
              exact_pad=True, canonical=True, heavy_frac=0.0, **_):
    """Build targets + (keys, counts).  Returns dict(targets=uint8[n,L] codes,
    names, keys uint64 (canonical, distinct), counts uint32, k)."""
    rng = np.random.default_rng(seed)
    rows = _unique_kmer_rows(rng, n_targets, length, k)
    base_cov = rng.integers(cov[0], cov[1], size=n_targets)
    ref_km = km.sliding_kmers(rows, k)                      # (T, n_ref)
    n_ref = ref_km.shape[1]
    jitter = rng.uniform(0.9, 1.1, size=ref_km.shape)
    ref_cnt = np.maximum(1, np.rint(base_cov[:, None] * jitter)).astype(np.int64)

    add_keys, add_cnts, add_tids = [], [], []
    has_var = rng.random(n_targets) < variant_frac
    for t in np.nonzero(has_var)[0]:
        nv = int(rng.integers(variants_per_target[0], variants_per_target[1] + 1))
        # heavy_frac: that share of the variant targets carries 3-5 tandem duplications instead (long
        # walks: the large tier of k_dfs / k_graph).  Nothing is drawn for it when it is 0, so that the
        # cases the goldens were made from stay what they are.
        heavy = bool(heavy_frac) and rng.random() < heavy_frac
        if heavy:
            nv = int(rng.integers(3, 6))
        for _v in range(nv):
            kind = "dup" if heavy else kinds[int(rng.integers(0, len(kinds)))]
            mut, lo, hi = _mutate(rng, rows[t], kind, k)
            f = float(rng.uniform(vaf[0], vaf[1]))
            if hom_frac and rng.random() < hom_frac:
                f = 1.0
            mk = km.sliding_kmers(mut, k)
            alt = mk[~np.isin(mk, ref_km[t])]
            if alt.size == 0:
                continue
            c = np.maximum(0, np.rint(base_cov[t] * f * rng.uniform(0.9, 1.1, size=alt.size)))
            add_keys.append(alt)
            add_cnts.append(c.astype(np.int64))
            add_tids.append(np.full(alt.size, t, dtype=np.int32))
            # ref k-mers spanning the replaced site lose the variant's share
            s0, s1 = max(0, lo - k + 1), min(n_ref, max(hi, lo + 1))
            span = np.arange(s0, s1)
            span = span[~np.isin(ref_km[t, span], mk)]
            ref_cnt[t, span] = np.rint(ref_cnt[t, span] * (1.0 - f)).astype(np.int64)

    # sibling noise: same k-1 prefix, different last base
    def siblings(frac, lo_c, hi_c, scale_by_cov):
        sel = rng.random(ref_km.shape) < frac
        tt, pp = np.nonzero(sel)
        if tt.size == 0:
            return
        sib = (ref_km[tt, pp] & ~np.uint64(3)) | (
            (ref_km[tt, pp] + rng.integers(1, 4, size=tt.size).astype(np.uint64)) & np.uint64(3))
        if scale_by_cov:
            c = np.maximum(1, np.rint(base_cov[tt] * rng.uniform(lo_c, hi_c, size=tt.size)))
        else:
            c = rng.integers(lo_c, hi_c, size=tt.size)
        add_keys.append(sib)
        add_cnts.append(c.astype(np.int64))
        add_tids.append(tt.astype(np.int32))

    siblings(noise_frac, noise_counts[0], noise_counts[1], False)
    if branch_noise_frac:
        siblings(branch_noise_frac, 0.06, 0.5, True)   # above the 5 % ratio: real dead-end branches

    keys = np.concatenate([ref_km.ravel()] + add_keys) if add_keys else ref_km.ravel()
    cnts = np.concatenate([ref_cnt.ravel()] + add_cnts) if add_cnts else ref_cnt.ravel()
    ref_tid = np.repeat(np.arange(n_targets, dtype=np.int32), n_ref)
    tids = np.concatenate([ref_tid] + add_tids) if add_tids else ref_tid
    if canonical:
        keys = km.canonical(keys, k)
    keep = cnts > 0
    keys, cnts, tids = keys[keep], cnts[keep], tids[keep]
    uk, first = np.unique(keys, return_index=True)          # first occurrence wins
    keys, cnts, tids = uk, cnts[first], tids[first]

    n_real = int(keys.size)
    n_pad = max(0, n_keys - keys.size)
    if n_pad and not exact_pad:
        # headline-size tables: skip the 100M-key sort; random 62-bit pads are distinct
        # with overwhelming probability, the rare one equal to a real key is dropped
        chunks_k, chunks_c = [keys], [cnts]
        left = n_pad
        while left > 0:
            m = min(left, 1 << 24)
            hi = (1 << (2 * k)) if 2 * k < 64 else int(np.iinfo(np.uint64).max)
            pad = rng.integers(0, hi, size=m, dtype=np.uint64)
            if canonical:
                pad = km.canonical(pad, k)
            # searched in sorted order: random probes into the 150 MB of real keys miss the cache on
            # every step and took five times as long; `ok` is the same either way
            order = np.argsort(pad)
            pad_s = pad[order]
            pos = np.searchsorted(keys, pad_s)
            pos[pos >= keys.size] = keys.size - 1
            ok = np.empty(m, dtype=bool)
            ok[order] = keys[pos] != pad_s
            chunks_k.append(pad[ok])
            chunks_c.append(rng.integers(2, 51, size=m)[ok])
            left -= m
        keys = np.concatenate(chunks_k)
        cnts = np.concatenate(chunks_c)
    elif n_pad:
        pad = (rng.integers(0, 1 << (2 * k), size=n_pad, dtype=np.uint64)
               if 2 * k < 64 else rng.integers(0, np.iinfo(np.uint64).max, size=n_pad, dtype=np.uint64))
        if canonical:
            pad = km.canonical(pad, k)
        padc = rng.integers(2, 51, size=n_pad)
        keys = np.concatenate([keys, pad])
        cnts = np.concatenate([cnts, padc])
        uk, first = np.unique(keys, return_index=True)
        keys, cnts = uk, cnts[first]
    names = ["%s%05d" % ((name or "syn") + "_t", i) for i in range(n_targets)]
    return {"targets": rows, "names": names, "keys": keys.astype(np.uint64),
            "counts": np.minimum(cnts, 0xFFFFFFFF).astype(np.uint32), "k": k, "n_real": n_real,
            # target each of the first n_real (non-pad) keys was generated for
            "key_target": tids}


def fast_canonical_keys(n, seed=0, k=31):
    """`n` DISTINCT canonical k-mers without a sort (real-size samples: example/run_leucegene.sh:24 counts with
    -s 799063683): the numbers seed_offset .. seed_offset + n - 1 pushed through a bijection of the 2k - 4 middle
    bits, between a first base A and a last base in {A, C, G} — the reverse complement of such a k-mer starts with
    T, G or C, so the k-mer itself is the canonical one.  Unsorted."""
    bits = 2 * k - 4
    assert 8 <= bits <= 58 and 0 < n < (1 << bits) - (1 << 20)
    M = np.uint64((1 << bits) - 1)
    idx = np.arange(n, dtype=np.uint64)
    x = (idx + np.uint64((int(seed) * 0x9E3779B1) % (1 << 20))) & M
    for mul, sh in ((0xFF51AFD7ED558CCD, 29), (0xC4CEB9FE1A85EC53, 31), (0x9E3779B97F4A7C15, 27)):
        x ^= x >> np.uint64(sh)                       # (each step is a bijection on `bits` bits)
        x *= np.uint64(mul)
        x &= M
    x ^= x >> np.uint64(bits // 2)
    x <<= np.uint64(2)
    x |= idx % np.uint64(3)
    return x


def make_sample(target_seqs, seed, k=31, n_keys=2_000_000, cov=(50, 2000), variant_frac=0.5,
                vaf=(0.1, 0.6), kinds=("snv", "ins", "del", "dup")):
    """One synthetic SAMPLE for BASELINE config 5: a k-mer count table for a GIVEN
    catalog of target sequences (strings, any lengths), seed = sample index.  Every target gets a
    coverage, half of them one variant at a random VAF, and the table is padded with random
    canonical k-mers to `n_keys`.  Returns (keys uint64, counts uint32), distinct canonical keys."""
    rng = np.random.default_rng(1000003 * (int(seed) + 1))
    all_k, all_c = [], []
    for seq in target_seqs:
        row = km.encode(seq).astype(np.uint8)
        if row.size < k or (row > 3).any():
            continue
        ref = km.sliding_kmers(row, k)
        base = int(rng.integers(cov[0], cov[1]))
        cnt = np.maximum(1, np.rint(base * rng.uniform(0.9, 1.1, size=ref.size))).astype(np.int64)
        if rng.random() < variant_frac and row.size >= 2 * k + 4:     # room for a variant with k-1 flanks
            kind = kinds[int(rng.integers(0, len(kinds)))]
            mut, lo, hi = _mutate(rng, row, kind, k)
            f = float(rng.uniform(vaf[0], vaf[1]))
            mk = km.sliding_kmers(mut, k)
            alt = mk[~np.isin(mk, ref)]
            if alt.size:
                all_k.append(alt)
                all_c.append(np.maximum(1, np.rint(base * f * rng.uniform(0.9, 1.1, size=alt.size))).astype(np.int64))
                s0, s1 = max(0, lo - k + 1), min(ref.size, max(hi, lo + 1))
                span = np.arange(s0, s1)
                span = span[~np.isin(ref[span], mk)]
                cnt[span] = np.maximum(1, np.rint(cnt[span] * (1.0 - f))).astype(np.int64)
        all_k.append(ref)
        all_c.append(cnt)
    keys = km.canonical(np.concatenate(all_k), k) if all_k else np.zeros(0, np.uint64)
    cnts = np.concatenate(all_c) if all_c else np.zeros(0, np.int64)
    n_pad = max(0, n_keys - keys.size)
    if n_pad > 20_000_000 and 12 <= k <= 31:
        # a real-size sample: distinct pads by construction (no sort of 10^8 keys), minus the few that are a real key
        uk, first = np.unique(keys, return_index=True)
        uc = np.minimum(cnts[first], 0xFFFFFFFF).astype(np.uint32)
        pads = fast_canonical_keys(n_pad, seed, k)
        at = np.searchsorted(uk, pads)
        at[at >= uk.size] = max(0, uk.size - 1)
        pads = pads[uk[at] != pads] if uk.size else pads
        pc = (np.arange(pads.size, dtype=np.uint32) * np.uint32(2654435761) >> np.uint32(16)) % np.uint32(49) + np.uint32(2)
        return np.concatenate([uk.astype(np.uint64), pads]), np.concatenate([uc, pc.astype(np.uint32)])
    if n_pad:
        hi = (1 << (2 * k)) if 2 * k < 64 else int(np.iinfo(np.uint64).max)
        keys = np.concatenate([keys, km.canonical(rng.integers(0, hi, size=n_pad, dtype=np.uint64), k)])
        cnts = np.concatenate([cnts, rng.integers(2, 51, size=n_pad)])
    uk, first = np.unique(keys, return_index=True)          # first occurrence wins
    return uk.astype(np.uint64), np.minimum(cnts[first], 0xFFFFFFFF).astype(np.uint32)


def write_jf(path, keys, counts, k, canonical=True):
    """Write keys/counts in the `binary/sorted` record layout our loaders read
    (9-digit length, JSON header, fixed key+count records)."""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.uint32)
    header = {"alignment": 8, "canonical": bool(canonical), "counter_len": 4,
              "format": "binary/sorted", "key_len": 2 * k, "val_len": 12,
              "size": int(1 << int(np.ceil(np.log2(max(16, 2 * keys.size))))),
              "cmdline": ["km_amd-synthetic"]}
    text = json.dumps(header, separators=(",", ":")).encode("ascii")
    text += b"\0" * ((-(9 + len(text))) % 8)
    kb = (2 * k + 7) // 8
    rec = np.zeros((keys.size, kb + 4), dtype=np.uint8)
    for b in range(kb):
        rec[:, b] = ((keys >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8)
    for b in range(4):
        rec[:, kb + b] = ((counts >> np.uint32(8 * b)) & np.uint32(0xFF)).astype(np.uint8)
    with open(path, "wb") as fh:
        fh.write(b"%09d" % len(text))
        fh.write(text)
        fh.write(rec.tobytes())


def write_case(outdir, **spec):
    """Materialise a case as FASTA files + one .jf.  Returns (fasta_paths, jf_path, meta)."""
    case = make_case(**spec)
    fas = []
    tdir = os.path.join(outdir, "targets")
    os.makedirs(tdir, exist_ok=True)
    h = hashlib.md5()
    for name, row in zip(case["names"], case["targets"]):
        p = os.path.join(tdir, name + ".fa")
        s = km.decode(row)
        with open(p, "w") as fh:
            fh.write(">synthetic:1-%d | name=%s\n%s\n" % (len(s), name, s))
        fas.append(p)
        h.update(s.encode())
    dbp = os.path.join(outdir, (spec.get("name") or "syn") + ".jf")
    write_jf(dbp, case["keys"], case["counts"], case["k"])
    h.update(case["keys"].tobytes())
    h.update(case["counts"].tobytes())
    return fas, dbp, {"md5": h.hexdigest(), "n_keys": int(case["keys"].size)}


# Small slices that tests/golden/make_golden.py runs through the reference.
GOLDEN_SPECS = [
    # config-4 shaped slice
    dict(name="cfg4_small", n_targets=100, length=500, n_keys=150_000, seed=HEADLINE_SEED),
    # every target mutated, 1-3 variants each, some homozygous, real dead-end branches
    dict(name="stress", n_targets=60, length=300, n_keys=60_000, seed=11, variant_frac=1.0,
         variants_per_target=(1, 3), hom_frac=0.25, branch_noise_frac=0.03, noise_frac=0.03),
    # low coverage around the -c 5 threshold
    dict(name="lowcov", n_targets=40, length=200, n_keys=20_000, seed=12, variant_frac=0.6,
         cov=(2, 30), vaf=(0.2, 0.8)),
    # tight walk budgets
    dict(name="tight", n_targets=40, length=300, n_keys=30_000, seed=13, variant_frac=1.0,
         variants_per_target=(1, 2), branch_noise_frac=0.05,
         params=dict(steps=40, branchs=2)),
    # node limit -> sys.exit after some targets were printed
    dict(name="nodelimit", n_targets=12, length=300, n_keys=10_000, seed=14, variant_frac=1.0,
         kinds=("dup",), params=dict(nodes=300)),
    # short k
    dict(name="k21", n_targets=30, length=150, k=21, n_keys=20_000, seed=15, variant_frac=0.8),
]


# ---------------------------------------------------------------------------- crossover cases
# Targets whose graph is known by construction (tests/test_graph_crossover.py, tests/golden/make_golden.py): every
# (k-1)-mer a pool hands out is distinct from every other ON BOTH STRANDS and none is its own reverse complement, so
# two nodes overlap only where a case says so and the canonical table never leads a walk onto the opposite strand.
_RC = str.maketrans("ACGT", "TGCA")


def revcomp_str(s):
    return s[::-1].translate(_RC)


class DistinctPool:
    """Deterministic source of sequences and haplotypes over one set of (k-1)-mers (see above)."""

    def __init__(self, k, seed):
        self.k = int(k)
        self.rng = np.random.default_rng(seed)
        self.seen = set()                      # every (k-1)-mer handed out, and its reverse complement

    def _free(self, mer, also=()):
        r = revcomp_str(mer)
        return mer != r and mer not in self.seen and r not in self.seen and mer not in also and r not in also

    def _add(self, mer):
        self.seen.add(mer)
        self.seen.add(revcomp_str(mer))

    def grow(self, n):
        """A new sequence of n >= k - 1 bases, grown base by base (a dead end starts it over)."""
        k1 = self.k - 1
        while True:
            s = "".join("ACGT"[i] for i in self.rng.integers(0, 4, k1))
            if not self._free(s):
                continue
            mine = {s, revcomp_str(s)}
            while len(s) < n:
                for b in self.rng.permutation(4):
                    mer = s[len(s) - k1 + 1:] + "ACGT"[b]
                    if self._free(mer, mine):
                        mine.add(mer)
                        mine.add(revcomp_str(mer))
                        s += "ACGT"[b]
                        break
                else:
                    break
            if len(s) == n:
                self.seen |= mine
                return s

    def admit(self, own, hap):
        """Take haplotype `hap` into a case whose forward (k-1)-mers are `own` (a set, extended here): every
        (k-1)-mer of it that the case does not have yet must be free.  False (and nothing changed) otherwise."""
        k1 = self.k - 1
        new, both = [], set()
        for i in range(len(hap) - k1 + 1):
            mer = hap[i:i + k1]
            if mer in own or mer in both:
                continue
            if not self._free(mer, both):
                return False
            new.append(mer)
            both.add(mer)
            both.add(revcomp_str(mer))
        for mer in new:
            self._add(mer)
            own.add(mer)
        return True


def _kmers_of(seq, k):
    return [seq[i:i + k] for i in range(len(seq) - k + 1)]


def _admit_snv(pool, own, seq, pos, step=1, alts=1):
    """`alts` substitutions of seq at the first position from `pos` on (in steps of `step`) at which they can be
    admitted.  -> (position, [haplotype, ...])."""
    while 0 <= pos < len(seq):
        haps = []
        trial = set(own)
        for b in "ACGT":
            if b != seq[pos] and len(haps) < alts:
                hap = seq[:pos] + b + seq[pos + 1:]
                if pool.admit(trial, hap):
                    haps.append(hap)
        if len(haps) == alts:
            own |= trial
            return pos, haps
        pos += step                                   # (what a failed position admitted stays taken: harmless)
    raise AssertionError("no position admits the substitution")


def crossover_case(pool, name, length, del_len, extra_ins=0, cov=(60, 35, 30), snvs=True):
    """One target of `length` bases with a deletion of `del_len` bases whose junction bases differ on both sides (the
    bubble has k - 1 new nodes, c = k edges, and bypasses b - a = del_len + k reference edges) and three SNVs on the
    reference background: upstream of the bubble, inside the deleted stretch, downstream of it.  `extra_ins` > 0 adds
    an insertion of that many bases near the end of the target (more walk nodes than the LDS tier keeps); `snvs`
    False leaves the deletion alone in its target (the one-bubble shape of k_graph's step 2c).
    -> dict(name, target, reads [(sequence, coverage)], expect {haplotype name: its new k-mers, in path order})."""
    k = pool.k
    T = pool.grow(length)
    own = set(_kmers_of(T, k - 1))
    p = 4 * k
    while True:
        assert p + del_len + 4 * k < length, "target too short for this deletion"
        dele = T[:p] + T[p + del_len:]
        if T[p] != T[p + del_len] and T[p - 1] != T[p + del_len - 1] and pool.admit(own, dele):
            break
        p += 1
    expect = {"del": _kmers_of(dele[p - k + 1:p + k - 1], k)}
    reads = [(T, cov[0]), (dele, cov[1])]
    for tag, pos, step in (("up", p - 2 * k, -1), ("in", p + del_len // 2, 1), ("down", p + del_len + 2 * k, 1)) if snvs else ():
        q, haps = _admit_snv(pool, own, T, pos, step)
        assert (q + k <= p - k) if tag == "up" else (p + k <= q < p + del_len - k) if tag == "in" else (q >= p + del_len + k and q + k < length)
        expect[tag] = _kmers_of(haps[0][q - k + 1:q + k], k)
        reads.append((haps[0], cov[2]))
    if extra_ins:
        ins = pool.grow(extra_ins)
        own |= set(_kmers_of(ins, k - 1))
        q = length - 2 * k
        # (junction bases differ on both sides, as for the deletion: every k-mer across a junction is new)
        while ins[0] == T[q] or ins[-1] == T[q - 1] or not pool.admit(own, T[:q] + ins + T[q:]):
            q -= 1
            assert q > p + del_len + 4 * k
        hap = T[:q] + ins + T[q:]
        expect["ins"] = _kmers_of(hap[q - k + 1:q + extra_ins + k - 1], k)
        reads.append((hap, cov[2]))
    return {"name": name, "target": T, "reads": reads, "expect": expect, "k": k, "kind": "sweep" if snvs else "solo"}


def nested_case(pool, name, cov=(60, 35, 35, 30)):
    """A deletion whose bubble (c1 = k edges) is cheaper than its reference route by 5 hops (b1 - a1 = 100 k + 5),
    enclosed by a second bubble of c2 = k + 1 edges (a deletion with one base inserted at its junction) that leaves
    the reference 48 k-mers before a1 and rejoins it 49 k-mers after b1; one SNV upstream of a2, one downstream of b2.
    In real numbers the route a1 -> inner bubble -> b1 -> b2 beats the outer bubble by 1 - 0.97 = 0.03 at b2, while
    the reference route a2 -> b2 LOSES to the outer bubble by 0.02: who wins at b2 (and, from the sink, at a2) depends
    on the true distances of the reference nodes past b1 (before a1), which are not the reference-chain sums.
    -> like crossover_case; expect has "del" (inner), "outer", "up", "down"."""
    k = pool.k
    d1 = 99 * k + 5
    length = 4 * k + 48 + d1 + 49 + 4 * k + 40
    T = pool.grow(length)
    own = set(_kmers_of(T, k - 1))
    p2 = 4 * k
    while True:
        p1, q2 = p2 + 48, p2 + 48 + d1 + 49
        assert q2 + 4 * k <= length, "target too short"
        inner = T[:p1] + T[p1 + d1:]
        ok = T[p1] != T[p1 + d1] and T[p1 - 1] != T[p1 + d1 - 1]
        outer = None
        for x in "ACGT" if ok else "":
            if x != T[p2] and x != T[q2 - 1]:
                trial = set(own)
                if pool.admit(trial, inner) and pool.admit(trial, T[:p2] + x + T[q2:]):
                    own, outer = trial, T[:p2] + x + T[q2:]
                    break
        if outer:
            break
        p2 += 1
    expect = {"del": _kmers_of(inner[p1 - k + 1:p1 + k - 1], k), "outer": _kmers_of(outer[p2 - k + 1:p2 + k], k)}
    reads = [(T, cov[0]), (inner, cov[1]), (outer, cov[2])]
    for tag, pos, step in (("up", p2 - 2 * k, -1), ("down", q2 + 2 * k, 1)):
        q, haps = _admit_snv(pool, own, T, pos, step)
        assert (q + k <= p2 - k) if tag == "up" else (q >= q2 + k and q + k < length)
        expect[tag] = _kmers_of(haps[0][q - k + 1:q + k], k)
        reads.append((haps[0], cov[3]))
    return {"name": name, "target": T, "reads": reads, "expect": expect, "k": k, "kind": "nested"}


def tie_case(pool, name, kind, length=None, cov=(60, 35, 30)):
    """kind "ins3": a 40-base insertion haplotype and two more that carry it with two different substitutions at one
    inserted position — inside the bubble the walk splits three ways and rejoins, the rejoin node has three
    in-neighbours at exactly the same distance.  kind "snv2": two substitutions at one reference position."""
    k = pool.k
    T = pool.grow(length or 6 * k + 40)
    own = set(_kmers_of(T, k - 1))
    p = 3 * k
    expect = {}
    if kind == "ins3":
        while True:
            ins = pool.grow(40)
            hap = T[:p] + ins + T[p:]
            if ins[0] != T[p] and ins[-1] != T[p - 1] and pool.admit(own | set(_kmers_of(ins, k - 1)), hap):
                break
        own |= set(_kmers_of(hap, k - 1))
        q, alts = _admit_snv(pool, own, hap, p + 20, 1, alts=2)
        assert p + 1 <= q <= p + 38
        reads = [(T, cov[0]), (hap, cov[1])] + [(h, cov[2]) for h in alts]
        expect["ins"] = _kmers_of(hap[p - k + 1:p + 40 + k - 1], k)
        for i, h in enumerate(alts):
            expect["alt%d" % i] = _kmers_of(h[q - k + 1:q + k], k)
    else:
        q, alts = _admit_snv(pool, own, T, p, 1, alts=2)
        reads = [(T, cov[0])] + [(h, cov[2]) for h in alts]
        for i, h in enumerate(alts):
            expect["alt%d" % i] = _kmers_of(h[q - k + 1:q + k], k)
    return {"name": name, "target": T, "reads": reads, "expect": expect, "k": k, "kind": kind}


def records_from_reads(reads, k):
    """Canonical k-mer records of (sequence, coverage) reads; coverages add up."""
    acc = {}
    for seq, c in reads:
        for key in km.canonical(km.sliding_kmers(km.encode(seq), k), k).tolist():
            acc[key] = acc.get(key, 0) + c
    keys = np.array(sorted(acc), dtype=np.uint64)
    return keys, np.array([acc[x] for x in keys.tolist()], dtype=np.uint32)


# 100 c - (b - a) of the crossover sweep: both sides of the closed forms' + 10 margin, the tie, both sides of the
# crossover of the float32 sums
CROSSOVER_MARGINS = (12, 11, 10, 9, 8, 3, 1, 0, -1, -2, -5)
CROSSOVER_GOLDEN = (10, 0, -5)                  # the k = 11 cases make_golden.py runs through the reference


def crossover_sweep(k, margins=CROSSOVER_MARGINS, extra_ins=0, seed=0, solo=(), nested=False, length=None):
    """The cases of the sweep at one k, over one pool (so they can share a table without meeting each other):
    case i has 100 k - (del_len + k) = margins[i]; after them one deletion-only case per margin of `solo`, then
    (`nested`) one nested_case.  `length`: of the sweep's targets (default 100 k + 8 k + 100)."""
    pool = DistinctPool(k, 977 * k + seed)
    length = (length or 100 * k + 8 * k + 100) + (extra_ins and 4 * k)
    cases = [crossover_case(pool, "x%d_%+d" % (k, v), length, 99 * k - v, extra_ins) for v in margins]
    cases += [crossover_case(pool, "solo%d_%+d" % (k, v), length, 99 * k - v, snvs=False) for v in solo]
    return cases + ([nested_case(pool, "nested%d" % k)] if nested else [])


# ---------------------------------------------------------------------------- structured cases
# Low-complexity and small-k inputs (tests/test_structured_kmers.py, tests/test_oracle_c.py): homopolymers,
# microsatellites, palindromes, a k-mer next to its own reverse complement, tables that hold the whole key space.
# Unlike the crossover cases above these WANT the coincidences that random 31-mers never show.
def random_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def has_repeated_kmer(seq, k):
    mers = _kmers_of(seq, k)
    return len(set(mers)) != len(mers)


def unique_kmer_seq(rng, n, k):
    """A random sequence of n bases with no k-mer twice."""
    while True:
        s = random_seq(rng, n)
        if not has_repeated_kmer(s, k):
            return s


def reads_to_records(reads, k, canonical=True):
    """records_from_reads, also for a table that stores k-mers as they are read."""
    if canonical:
        return records_from_reads(reads, k)
    acc = {}
    for seq, c in reads:
        for key in km.sliding_kmers(km.encode(seq), k).tolist():
            acc[key] = acc.get(key, 0) + c
    keys = np.array(sorted(acc), dtype=np.uint64)
    return keys, np.array([acc[x] for x in keys.tolist()], dtype=np.uint32)


def end_duplication_case(k, seed=0):
    """A tandem duplication that reaches the target's end: the variant path is the whole reference path plus a
    junction and a second copy of the tail, so the reference path is a proper prefix of it."""
    rng = np.random.default_rng(8100 + 37 * k + seed)
    T = unique_kmer_seq(rng, 3 * k + 10, k)
    return {"name": "enddup%d" % k, "target": T, "reads": [(T, 60), (T + T[-(k + 5):], 30)], "k": k}


def homopolymer_insertion_case(k, base, seed=0):
    """One more `base` in a run of k - 1 of them: the variant's only new k-mer is the homopolymer base^k, a one-node
    bubble between x base^(k-1) and base^(k-1) y whose node is behind its own suffix (the reference's graph has no
    edge from a node to itself: km/utils/MutationFinder.py:530)."""
    rng = np.random.default_rng(8600 + 43 * k + 5 * "ACGT".index(base) + seed)
    while True:
        left, right = random_seq(rng, k + 3), random_seq(rng, k + 3)
        T = left + base * (k - 1) + right
        V = left + base * k + right
        if left[-1] != base and right[0] != base and not has_repeated_kmer(T, k) and not has_repeated_kmer(V, k):
            return {"name": "homo_%s%d" % (base, k), "target": T, "reads": [(T, 60), (V, 30)], "k": k}


def dense_counts(rng, n):
    """30 % in 100 .. 70 000 (both sides of the 16-bit escape), the rest in 1 .. 5 (around `count`)."""
    c = rng.integers(1, 6, size=n)
    big = rng.random(n) < 0.3
    c[big] = rng.integers(100, 70_001, size=int(big.sum()))
    return c.astype(np.uint32)


def small_k_case(k, canonical, seed=0, n_targets=12):
    """k <= 10.  k <= 7: a table over the whole key space (k <= 4) or a seeded 80 % of it; random targets with no
    repeated k-mer.  k = 8 .. 10 (a half-full table of that size hardly branches): the targets' own reads plus a
    substitution or an insertion each, and a quarter of the key space around them at counts of 1 .. 5."""
    rng = np.random.default_rng(500 + k + 1000 * seed + (0 if canonical else 7919))
    space = np.arange(1 << (2 * k), dtype=np.uint64)
    if canonical:
        space = space[space <= km.revcomp(space, k)]
    max_len = min((1 << (2 * k)) // 2 + k, 60)
    targets = [unique_kmer_seq(rng, int(rng.integers(k + 1, max_len)), k) for _ in range(n_targets)]
    if k <= 7:
        keys = space if k <= 4 else space[rng.random(space.size) < 0.8]
        counts = dense_counts(rng, keys.size)
    else:
        reads = []
        for i, T in enumerate(targets):
            reads.append((T, int(rng.integers(40, 70_000 if i % 4 == 0 else 200))))
            p = int(rng.integers(1, len(T) - 1))
            if i % 2:
                var = T[:p] + "ACGT"[("ACGT".index(T[p]) + 1 + i % 3) % 4] + T[p + 1:]
            else:
                var = T[:p] + random_seq(rng, 1 + i % 5) + T[p:]
            reads.append((var, max(1, reads[-1][1] // 2)))
        rk, rc = reads_to_records(reads, k, canonical)
        pad = space[rng.random(space.size) < 0.25]
        pad = pad[~np.isin(pad, rk)]
        keys = np.concatenate([rk, pad])
        counts = np.concatenate([rc, rng.integers(1, 6, size=pad.size).astype(np.uint32)])
        order = np.argsort(keys)
        keys, counts = keys[order], counts[order]
    return {"k": k, "canonical": canonical, "keys": keys, "counts": counts, "targets": targets,
            "names": ["k%d_%d" % (k, i) for i in range(n_targets)]}


REPEAT_UNITS = ("A", "T", "AT", "TA", "AC", "CG")


def repeat_case(k, unit, seed=0):
    """Reads that enter a repeat of `unit` from the target and never leave it (the walk circles the repeat)."""
    rng = np.random.default_rng(8200 + 41 * k + 7 * REPEAT_UNITS.index(unit) + seed)
    while True:
        T = random_seq(rng, k + 5) + unit * (6 // len(unit)) + random_seq(rng, k + 7)
        if not has_repeated_kmer(T, k):
            break
    cut = k + 5 + 6
    return {"name": "rep_%s_%d" % (unit, k), "target": T, "k": k,
            "reads": [(T, 50), (T[:cut] + unit * (k + 4), 30)]}


def inversion_case(k, seed=0):
    """Target A + B + C, reads with B inverted: the walk follows the reverse strand of B, and where the table is
    canonical it meets every k-mer of B again as its own reverse complement."""
    rng = np.random.default_rng(8300 + 43 * k + seed)
    T = unique_kmer_seq(rng, (k + 10) + (2 * k + 3) + (k + 10), k)
    a, b = k + 10, k + 10 + 2 * k + 3
    return {"name": "inv%d" % k, "target": T, "k": k,
            "reads": [(T, 60), (T[:a] + revcomp_str(T[a:b]) + T[b:], 30)]}


def hairpin_case(k, seed=0):
    """Target S + rc(S): every k-mer stands next to its reverse complement; for even k the centre one is both."""
    rng = np.random.default_rng(8400 + 47 * k + seed)
    while True:
        S = random_seq(rng, k + 9)
        T = S + revcomp_str(S)
        if not has_repeated_kmer(T, k):
            return {"name": "hairpin%d" % k, "target": T, "k": k, "reads": [(T, 50)]}


def structured_cases(k, seed=0):
    """Every structured walk case at one k, each with a table of its own."""
    return ([repeat_case(k, u, seed) for u in REPEAT_UNITS]
            + [inversion_case(k, seed), hairpin_case(k, seed), end_duplication_case(k, seed)])
