"""Solid k-mers in two passes (km_counter_set_sketch, Counter.set_sketch, count_files(solid=), `count --solid`): what is
decided without a GPU, and the model and the inputs the GPU tests (test_count_solid.py) compare with.

The model is written from the rule (DESIGN.md §10 "Solid k-mers, two passes"; include/kmgpu.h) in plain Python with its
own mix64, and shares no code with km_amd/csrc/sketch_rule.h.  Which keys seen ONCE the sketch admits depends on the
order in which the device's lanes arrive, so the model does not predict the admitted set: it bounds it.  S, the keys
seen at least twice, is always admitted; `upper` is a superset of whatever any order can admit."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import test_count as tc
from km_amd import cli
from km_amd import count as kc
from km_amd import lib as kmlib

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG = 4
ALLT = (1 << 64) - 1
M64 = (1 << 64) - 1
ACGT = np.frombuffer(b"ACGT", np.uint8)
CASES = [(2, False), (5, True), (5, False), (31, True), (32, True), (32, False)]


# ------------------------------------------------------------------ the rule, restated
def mix64(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def model_slot(key, words):
    """(word, mask) of `key` in a sketch of `words` words."""
    h = mix64(key ^ 0x9E3779B97F4A7C15)
    return h >> (64 - (words.bit_length() - 1)), (1 << (h & 31)) | (1 << ((h >> 5) & 31)) | (1 << ((h >> 10) & 31))


def model_words(expected_distinct):
    w = 64
    while w < (expected_distinct + 1) // 2:
        w <<= 1
    return w


def solid_model(data, k, canonical, words):
    """-> (brute, S, upper, bounds) for the byte stream `data` (bases, any other byte a break) noted once, whole, in a
    sketch of `words` words.  brute: {key: count} of every window.  S: the keys with count >= 2.  upper: a superset of
    the keys any arrival order can admit.  It comes from a superset of plane 2: a key's mask enters plane 2 only from a
    fetch_or of that key which found the mask in plane 1, that is, from a second occurrence of the key (the key is in
    S), or from an occurrence that found all its bits set by OTHER keys of its word.  So plane 2 of a word is covered by
    the OR of the masks of its keys that are in S or whose mask the OR of the other keys' masks covers, and a key can be
    admitted only if that covers its mask.  The key ~0 has no sketch entry and is always counted: it is in `upper`
    whenever it occurs.  bounds: dict(bits_1 = the exact set bits of plane 1 (the OR of all masks: plane 2 is a subset
    of plane 1 bit for bit, so a note skipped on plane 2 leaves no bit of plane 1 unset), bits_2 = (lo, hi),
    kmers_admitted = (lo, hi))."""
    keys, counts = tc.model(data, k, canonical)
    brute = dict(zip(keys.tolist(), counts.tolist()))
    S = {key for key, n in brute.items() if n >= 2}
    by_word = {}
    for key in brute:
        if key == ALLT:
            continue
        word, mask = model_slot(key, words)
        by_word.setdefault(word, []).append((key, mask))
    upper = {ALLT} & set(brute)
    bits_1 = bits_2_lo = bits_2_hi = 0
    for members in by_word.values():
        n = len(members)
        before, after = [0] * (n + 1), [0] * (n + 1)             # OR of the masks in front of / behind each member
        for i, (_, mask) in enumerate(members):
            before[i + 1] = before[i] | mask
        for i in range(n - 1, -1, -1):
            after[i] = after[i + 1] | members[i][1]
        plane_2 = sure = 0
        for i, (key, mask) in enumerate(members):
            others = before[i] | after[i + 1]
            if key in S:
                sure |= mask
            if key in S or others & mask == mask:
                plane_2 |= mask
        upper |= {key for key, mask in members if plane_2 & mask == mask}
        bits_1 += bin(before[n]).count("1")
        bits_2_lo += bin(sure).count("1")
        bits_2_hi += bin(plane_2).count("1")
    in_table = lambda keys: sum(brute[key] for key in keys if key != ALLT)
    bounds = {"bits_1": bits_1, "bits_2": (bits_2_lo, bits_2_hi), "kmers_admitted": (in_table(S), in_table(upper))}
    return brute, S, upper, bounds


# ------------------------------------------------------------------ the inputs of the GPU tests
def solid_reads(seed, n_bytes=6000, genome=400):
    """Reads of 90-150 nt from both strands of a random genome of `genome` bases, 2 % substitutions, 0.5 % N, a fifth
    in lower case, about n_bytes in all."""
    rng = np.random.default_rng(seed)
    g = ACGT[rng.integers(0, 4, genome)].tobytes()
    reads, total = [], 0
    while total < n_bytes:
        ln = int(rng.integers(90, 151))
        a = int(rng.integers(0, genome - ln + 1))
        r = g[a:a + ln]
        if rng.integers(2):
            r = r.translate(tc._COMP)[::-1]
        r = np.frombuffer(r, np.uint8).copy()
        sub = rng.random(ln) < 0.02
        r[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
        r[rng.random(ln) < 0.005] = ord("N")
        r[rng.random(ln) < 0.2] |= 0x20
        reads.append(r.tobytes())
        total += ln + 1
    return reads


def as_stream(reads):
    """What add_bases takes: the reads with a break between them."""
    return b"\n".join(reads)


def as_fasta(reads):
    """What add_text takes: a record per read, every third read on two lines (the stripper joins them)."""
    out = []
    for i, r in enumerate(reads):
        body = r[:len(r) // 2] + b"\n" + r[len(r) // 2:] if i % 3 == 0 else r
        out.append(b">read%d\n" % i + body + b"\n")
    return b"".join(out)


def mers_of(keys, k=31):
    """The letters of each key, a row per key."""
    keys = np.asarray(keys, np.uint64)
    shifts = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    return ACGT[((keys[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)]


def distinct_canonical_mers(rng, n, k=31):
    """n distinct canonical k-mers (k odd: none is its own reverse complement) -> sorted uint64 keys."""
    from oracle import jf_reader as jr
    keys = np.unique(jr.canonical_np(rng.integers(0, 1 << (2 * k), 2 * n + 64, dtype=np.uint64), k))
    keys = keys[rng.permutation(keys.size)][:n]
    assert keys.size == n
    return np.sort(keys)


TABLE_SEED, TABLE_SOLID, TABLE_SINGLE, TABLE_EXPECTED = 21, 2000, 20000, 22000


def table_text():
    """About 2 000 k-mers planted twice or three times and about 20 000 planted once, an N behind each, shuffled."""
    rng = np.random.default_rng(TABLE_SEED)
    keys = distinct_canonical_mers(rng, TABLE_SOLID + TABLE_SINGLE)
    keys = keys[rng.permutation(keys.size)]
    times = np.ones(keys.size, np.int64)
    times[:TABLE_SOLID] = rng.integers(2, 4, TABLE_SOLID)
    planted = np.repeat(keys, times)
    planted = planted[rng.permutation(planted.size)]
    rows = np.full((planted.size, 32), ord("N"), np.uint8)
    rows[:, :31] = mers_of(planted)
    return rows.tobytes()


# ------------------------------------------------------------------ tests
def test_sketch_slot_and_words_equal_the_model():
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 1 << 64, 10_000, dtype=np.uint64).tolist() + [0, (1 << 62) - 1, ALLT - 1]
    for words in (64, 1 << 20, 1 << 40):
        for key in keys:
            word, mask = kmlib.sketch_slot(key, words)
            assert (word, mask) == model_slot(key, words), (key, words)
            assert 1 <= bin(mask).count("1") <= 3 and mask < 1 << 32 and 0 <= word < words
    for n in (0, 1, 127, 128, 129, 256, 257, 22_000, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1 << 41):
        assert kmlib.sketch_words(n) == model_words(n), n
    assert kmlib.sketch_words(22_000) == 16_384 and kmlib.sketch_words(0) == 64 and kmlib.sketch_words(1 << 41) == 1 << 40


def test_argument_errors_before_any_hip_call():
    lib = kmlib.load()
    for words in (0, 32, 96, (1 << 40) + 1, 1 << 41):
        with pytest.raises(kmlib.KmError) as e:
            kmlib.sketch_slot(5, words)
        assert e.value.code == E_ARG
    with pytest.raises(kmlib.KmError) as e:
        kmlib.sketch_words((1 << 41) + 1)
    assert e.value.code == E_ARG
    assert lib.km_sketch_words(5, None) == E_ARG and lib.km_sketch_slot(5, 64, None, None) == E_ARG
    assert lib.km_counter_set_sketch(None, 64) == E_ARG
    assert lib.km_counter_sketch_done(None) == E_ARG
    assert lib.km_counter_sketch_stats(None, None, None, None, None, None, None) == E_ARG


def test_rule_program_under_sanitizers(tmp_path):
    """csrc/sketch_rule.h built for the CPU with AddressSanitizer + UBSan (tests/host/sketch_rule.cpp): note and admit
    played sequentially on a host array."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "sketch_rule")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "host", "sketch_rule.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe], capture_output=True, env=env, timeout=600)
    assert proc.returncode == 0 and proc.stdout.endswith(b"SKETCH RULE OK\n"), (proc.stdout[-2000:], proc.stderr[-3000:])
    assert b"ERROR: AddressSanitizer" not in proc.stderr and b"runtime error" not in proc.stderr, proc.stderr[-3000:]


def sequential_sketch(occurrences, words):
    """The rule played in Python, one occurrence after the other -> {word: value}."""
    sketch = {}
    for key in occurrences:
        if key == ALLT:
            continue
        word, mask = model_slot(key, words)
        cur = sketch.get(word, 0)
        if (cur >> 32) & mask == mask:
            continue
        sketch[word] = cur | mask
        if cur & mask == mask:
            sketch[word] |= mask << 32
    return sketch


@pytest.mark.parametrize("k,canonical", CASES)
def test_model_bounds_hold_for_sequential_orders(k, canonical):
    """S is admitted and nothing outside `upper` is, for the input of the exactness test played forwards, backwards and
    shuffled at a saturated and at a roomy sketch; the statistics lie within the model's bounds."""
    data = as_stream(solid_reads(100 + 2 * k + canonical))
    occurrences = [key for key, n in zip(*(a.tolist() for a in tc.model(data, k, canonical))) for _ in range(n)]
    rng = np.random.default_rng(3)
    for words in (64, kmlib.sketch_words(2000)):
        brute, S, upper, bounds = solid_model(data, k, canonical, words)
        assert S <= upper <= set(brute) and S
        for order in (occurrences, occurrences[::-1], [occurrences[i] for i in rng.permutation(len(occurrences))]):
            sketch = sequential_sketch(order, words)
            admitted = {key for key in brute
                        if key == ALLT or (sketch.get(model_slot(key, words)[0], 0) >> 32) & model_slot(key, words)[1]
                        == model_slot(key, words)[1]}
            assert S <= admitted <= upper
            assert sum(bin(v & 0xFFFFFFFF).count("1") for v in sketch.values()) == bounds["bits_1"]
            bits_2 = sum(bin(v >> 32).count("1") for v in sketch.values())
            assert bounds["bits_2"][0] <= bits_2 <= bounds["bits_2"][1]


def test_the_table_input_meets_its_precondition():
    """The text of the GPU test "the table really is smaller": about 2 000 solid keys, about 20 000 singletons, and at
    W = sketch_words(22 000) at most a quarter of the singletons can ever be admitted."""
    data = table_text()
    words = kmlib.sketch_words(TABLE_EXPECTED)
    assert words == 16_384
    brute, S, upper, bounds = solid_model(data, 31, True, words)
    singletons = [key for key, n in brute.items() if n == 1]
    assert 1900 <= len(S) <= 2100 and 19_000 <= len(singletons) <= 21_000
    assert S <= upper
    assert len(upper) - len(S) <= len(singletons) / 4
    assert bounds["bits_2"][0] <= bounds["bits_2"][1] <= bounds["bits_1"]


def test_parse_args_solid():
    args = cli.parse_args(["count", "--solid", "1000", "-m", "21", "reads.fq"], cli.build_parser())
    assert args.solid == 1000 and args.only is None and args.lower_count == 1
    assert cli.parse_args(["count", "reads.fq"], cli.build_parser()).solid is None
    assert "--solid" in cli.build_parser()._subparsers._group_actions[0].choices["count"].format_help()
    for argv in (["count", "--solid", "1000", "--if", "t.fa", "reads.fq"], ["count", "--solid", "-3", "reads.fq"],
                 ["count", "--solid", "many", "reads.fq"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv, cli.build_parser())
        assert e.value.code == 2


def test_cli_refuses_solid_with_if_and_with_stdin(tmp_path):
    env = dict(os.environ, PYTHONPATH=tc.ROOT, KM_HIP_RUNTIME="system")
    reads = tmp_path / "r.fa"
    reads.write_text(">r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    run = lambda argv: subprocess.run([sys.executable, "-m", "km_amd", "count"] + argv, cwd=tmp_path, capture_output=True,
                                      text=True, timeout=300, env=env, stdin=subprocess.DEVNULL)
    res = run(["--solid", "1000", "-m", "21", "-o", "a.jf", "-"])
    assert res.returncode == 1 and res.stderr.splitlines()[-1].startswith("ERROR: count:"), res.stderr
    assert "standard input" in res.stderr
    res = run(["--solid", "1000", "-m", "21", "-o", "a.jf", "r.fa", "-"])
    assert res.returncode == 1 and res.stderr.splitlines()[-1].startswith("ERROR: count:"), res.stderr
    res = run(["--solid", "1000", "--if", "r.fa", "-m", "21", "-o", "a.jf", "r.fa"])
    assert res.returncode == 2 and "--solid" in res.stderr, res.stderr
    assert not os.path.exists(tmp_path / "a.jf")


def test_count_files_refuses_before_a_counter_exists(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError("a counter was created")
    monkeypatch.setattr(kmlib, "Counter", refuse)
    with pytest.raises(ValueError, match="only"):
        kc.count_files(["reads.fq"], k=31, solid=1000, only=np.array([1, 2], np.uint64))
    with pytest.raises(ValueError, match="standard input"):
        kc.count_files(["reads.fq", "-"], k=31, solid=1000)
    with pytest.raises(ValueError, match="standard input"):
        kc.count_files("-", k=31, solid=1000)
    with pytest.raises(ValueError, match="solid"):
        kc.count_files(["reads.fq"], k=31, solid=-1)
