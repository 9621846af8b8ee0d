"""`k_linear_kmin` (km_amd/csrc/kmin_kernel.h) on every short string and at every seam of a lane.

The kernel compares four bytes per step and reads runs off a bit mask; the runs of length 1 or 2 that lie strictly
inside a word are seen only by a side loop that is switched off once the lane's best key reaches 5; bytes past a
diagonal's end are masked by arithmetic on `rem`; the run that reaches the end closes in a later step or, for lane 0,
after the loop; and three exemptions decide the flag.  Four corpora put a run at each of those places:

  A  one planted copy of 1, 2 or 3 letters in text whose letters are all distinct, at every (a, d) of targets of
     2 .. 9 and 63 .. 68 letters: every lane of a wave, every byte of a word, the side loop and both sides of its switch;
  B  copies of 3 .. 33 letters planted in an order-2 de Bruijn text at the seams of a step (4 bytes), an iteration
     (16 bytes) and a work unit (64 diagonals), with 0, 1 or 5 letters behind the copy;
  C  periodic targets of 15 .. 257 letters, each followed in the call by a target that continues its period in phase:
     staged 16-byte aligned, a target of 16 m letters has bytes behind it that would lengthen its run without the end mask;
  D  all 23 493 strings over AC up to 12 letters, ACG up to 8 and ACGT up to 6.

Expected values come from two models that share nothing: `model` of tests/test_linear_kmin.py (k-mer sets and the
reference's neighbour counts; gives k and R) and `runs_model` below (the kernel's own definition: maximal runs on
every diagonal and the three exemptions; gives R and the flag), joined by `closed_form`, a restatement of
km_amd/csrc/kmin_rule.h.  The CPU tests prove the two equal on the corpora and that each corpus shows
what it is meant to show; the GPU tests compare k, R and the flag of every target, exactly."""
import functools
import itertools
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from km_amd import lib as kmlib

from test_linear_kmin import model

HERE = os.path.dirname(os.path.abspath(__file__))

# the 68 printable ASCII characters that are not lower-case letters: upper-casing leaves them alone
ALPHA = "".join(chr(c) for c in range(0x21, 0x7F) if not chr(c).islower())
assert len(ALPHA) == 68

FIXED_STARTS = (0, 1, 2, 3, 10)        # A and D
SEAM_STARTS = (1, 10)                  # B and C
RELATIVE = (-1, 0, 1, 2)               # A and D once more at start = n + each: the edges of start - 1 >= n and min(R + 2, n)
FLAG_MAX_N = 400                       # runs_model is quadratic: the flag is compared up to this length


# ------------------------------------------------------------------ the second model
def runs_plain(s):
    """(R, flag) from the definition, letter by letter: every maximal run of s[a] == s[a+d] on every diagonal d >= 1,
    exempt iff (d == 1 and x == 0) or (d == 1 and p + d == n) or (x == 0 and p + d == n)."""
    n = len(s)
    runs = []
    for d in range(1, n):
        x = None
        for a in range(n - d + 1):                      # a == n - d closes the run that reaches the end
            if a < n - d and s[a] == s[a + d]:
                if x is None:
                    x = a
            elif x is not None:
                runs.append((a - x, d, x, a))
                x = None
    R = max((r[0] for r in runs), default=0)
    flag = 0
    for length, d, x, p in runs:
        exempt = (d == 1 and x == 0) or (d == 1 and p + d == n) or (x == 0 and p + d == n)
        if length == R and not exempt:
            flag = 1
    return R, flag


def runs_model(s):
    """runs_plain with every diagonal at once: row d - 1 of `eq` is diagonal d, padded with unequal bytes."""
    n = len(s)
    if n < 2:
        return 0, 0
    b = np.frombuffer(s.encode("ascii"), np.uint8).astype(np.int16)
    behind = np.concatenate([b, np.full(n, -1, np.int16)])
    a = np.arange(n)
    d = np.arange(1, n)
    eq = b[None, :] == behind[a[None, :] + d[:, None]]          # eq[d - 1, a]; column n - 1 is never equal
    seen = np.cumsum(eq, axis=1)
    length = seen - np.maximum.accumulate(np.where(eq, 0, seen), axis=1)    # of the run that ends at a, inclusive
    ends = eq & ~np.concatenate([eq[:, 1:], np.zeros((n - 1, 1), bool)], axis=1)
    row, col = np.nonzero(ends)
    if row.size == 0:
        return 0, 0
    ln, dd, p = length[row, col], d[row], col + 1
    x = p - ln
    exempt = ((dd == 1) & (x == 0)) | ((dd == 1) & (p + dd == n)) | ((x == 0) & (p + dd == n))
    R = int(ln.max())
    return R, int(((ln == R) & ~exempt).any())


def closed_form(n, start, R, flag):
    """k from (n, start, R, flag): km_amd/csrc/kmin_rule.h restated."""
    if n == 0:
        return 0 if start <= 0 else start - 1
    if R == 0:
        flag = int(n >= 3)
    if start - 1 >= n:
        return start - 1
    lo = max(start, R + 1)
    if lo > R + 1:
        return lo
    return min(R + 2, n) if flag else R + 1


def reported_flag(n, R, flag):
    """The flag `detail=True` returns: the runs' flag after the closed form has had it."""
    if n == 0:
        return 0
    return int(n >= 3) if R == 0 else flag


_MODEL, _RUNS = {}, {}


def cached_model(s, start):
    """`model` is the reference of every test here and is never changed: one evaluation per (s, start) per session."""
    key = (s, start)
    if key not in _MODEL:
        _MODEL[key] = model(s, start)
    return _MODEL[key]


def cached_runs(s):
    if s not in _RUNS:
        _RUNS[s] = runs_model(s)
    return _RUNS[s]


# ------------------------------------------------------------------ the corpora
A_LENGTHS = tuple(range(2, 10)) + (63, 64, 65, 66, 67, 68)


@functools.lru_cache(maxsize=None)
def family_a(length):
    """[(s, n, a, d)]: ALPHA[:n] with s[a+d : a+d+length] = s[a : a+length], every a and d that fit."""
    out = []
    for n in A_LENGTHS:
        base = ALPHA[:n]
        for d in range(1, n):
            for a in range(0, n - d - length + 1):
                s = list(base)
                s[a + d:a + d + length] = base[a:a + length]
                out.append(("".join(s), n, a, d))
    return out


@functools.lru_cache(maxsize=None)
def debruijn2():
    """The order-2 de Bruijn sequence over ALPHA, closed with its first letter: every 2-mer once, R = 1."""
    m = len(ALPHA)
    db = []
    a = [0] * (2 * m)

    def gen(t, p):
        if t > 2:
            if 2 % p == 0:
                db.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            gen(t + 1, p)
            for j in range(a[t - p] + 1, m):
                a[t] = j
                gen(t + 1, t)
    gen(1, 1)
    return "".join(ALPHA[i] for i in db) + ALPHA[db[0]]


B_D = (1, 2, 3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 1023, 1024, 1025)
B_X = (0, 1, 2, 3, 13, 15, 16, 17)
B_LEN = (3, 4, 5, 15, 16, 17, 31, 32, 33)
B_TAIL = (0, 1, 5)


@functools.lru_cache(maxsize=None)
def family_b():
    """[(s, d, x, length, tail)]: a copy of `length` letters planted d behind x in the de Bruijn text, `tail` letters
    behind the copy.  The three longest d only at the corners of x, length and tail."""
    bg = debruijn2()
    out = []
    for d in B_D:
        far = d >= 1023
        for x, length, tail in itertools.product((0, 17) if far else B_X, (5, 33) if far else B_LEN,
                                                 (0, 5) if far else B_TAIL):
            n = x + d + length + tail
            s = list(bg[:n])
            s[x + d:x + d + length] = s[x:x + length]
            out.append(("".join(s), d, x, length, tail))
    return out


C_UNITS = ("A", "AC", "ACG", "ACGT", "ACGTA")
C_N = (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def family_c():
    """[(s, period)] in the order of the call: the first n letters of a periodic text, then the n letters behind them."""
    out = []
    for u in C_UNITS:
        for n in C_N:
            text = u * (2 * n // len(u) + 1)
            out.append((text[:n], len(u)))
            out.append((text[n:2 * n], len(u)))
    return out


@functools.lru_cache(maxsize=None)
def family_d():
    out = []
    for letters, longest in (("AC", 12), ("ACG", 8), ("ACGT", 6)):
        for n in range(longest + 1):
            out.extend("".join(t) for t in itertools.product(letters, repeat=n))
    return out


@functools.lru_cache(maxsize=None)
def corpus(name):
    """The targets of a corpus as the GPU tests send them, one call's list."""
    if name in ("A1", "A2", "A3"):
        return [row[0] for row in family_a(int(name[1]))]
    if name == "A":
        return corpus("A1") + corpus("A2") + corpus("A3")
    if name == "B":
        return [row[0] for row in family_b()]
    if name == "C":
        return [row[0] for row in family_c()]
    assert name == "D"
    return family_d()


def relative_calls(seqs):
    """{start: targets}: every target once at each start = n - 1, n, n + 1, n + 2, one call per value of start."""
    calls = {}
    for s in seqs:
        for delta in RELATIVE:
            calls.setdefault(len(s) + delta, []).append(s)
    return calls


# ------------------------------------------------------------------ CPU: the corpora and the two models
def test_corpora_have_the_stated_sizes():
    assert len(family_a(1)) == 12_803 and sum(1 for r in family_a(1) if r[1] == 68) == 2_278
    assert len(debruijn2()) == 4_625 and len(set(zip(debruijn2(), debruijn2()[1:]))) == 4_624
    assert len(family_b()) == 15 * 8 * 9 * 3 + 3 * 2 * 2 * 2
    assert len(family_c()) == 2 * 5 * 20
    assert len(family_d()) == 23_493 == (2 ** 13 - 1) + (3 ** 9 - 1) // 2 + (4 ** 7 - 1) // 3


def test_runs_model_is_the_letter_by_letter_definition():
    """The vectorised runs_model against runs_plain: on every short string, on A at 2 .. 9 and 63 letters, and on
    every 20th target of B up to 260 letters and of C."""
    for s in set(family_d()):
        assert runs_model(s) == runs_plain(s), s
    for length in (1, 2, 3):
        for s, n, a, d in family_a(length):
            if n <= 9 or (n == 63 and (a + d) % 7 == 0):
                assert runs_model(s) == runs_plain(s), (n, a, d, length)
    for s in [r[0] for r in family_b() if len(r[0]) <= 260][::20] + corpus("C")[::20]:
        assert runs_model(s) == runs_plain(s), s


def _models_agree(seqs, starts):
    for s in seqs:
        R, flag = cached_runs(s)
        for start in starts(s) if callable(starts) else starts:
            k, rep = cached_model(s, start)
            assert rep == R, (s, start)
            assert closed_form(len(s), start, R, flag) == k, (s, start, R, flag)


def _with_relative(fixed):
    return lambda s: fixed + tuple(len(s) + delta for delta in RELATIVE)


def test_closed_form_on_every_short_string():
    """DESIGN.md §9 on corpus D: k from the runs and the closed form is k from k-mer sets and neighbour counts, and
    both models find the same R, at every start of the GPU tests."""
    _models_agree(set(family_d()), _with_relative(FIXED_STARTS + (-1,)))


@pytest.mark.parametrize("length", (1, 2, 3))
def test_closed_form_on_family_a(length):
    _models_agree(corpus("A%d" % length), _with_relative(FIXED_STARTS))


def test_closed_form_on_family_b_and_c():
    """The members of B up to 260 letters, and C (not asked of C, but cheap)."""
    _models_agree([s for s in corpus("B") if len(s) <= 260], SEAM_STARTS)
    _models_agree(corpus("C"), SEAM_STARTS)


def test_family_a_is_one_run_and_three_exemptions():
    """A planted single letter is the only repeat: R = 1 everywhere, and the flag is 0 exactly at the three exempt
    placements of each n: the first two letters equal, the last two equal, the first equal to the last.  A run of one
    letter strictly inside a word (byte 1 or 2 of its step) is in the set for every lane, and so are the runs of 2
    and 3 on both sides of the side loop's switch."""
    inner = set()
    for s, n, a, d in family_a(1):
        R, flag = cached_runs(s)
        exempt = (a, d) in {(0, 1), (n - 2, 1), (0, n - 1)}
        assert (R, flag) == (1, 0 if exempt else 1), (n, a, d)
        if a % 4 in (1, 2) and n >= 63:
            inner.add((d - 1) % 64)
    assert inner == set(range(64))
    for length in (2, 3):                   # a copy that overlaps its source (d < length) repeats d letters of it
        assert all(cached_runs(s)[0] == min(length, d) for s, _n, _a, d in family_a(length))
    assert {n for _s, n, _a, d in family_a(1) if d > 64} == {66, 67, 68}          # a second work unit


def test_family_b_puts_runs_on_the_seams():
    """At least half of B has R == the planted length exactly (where it has not, the copy's neighbours lengthened the
    run, and the models say by how much), the runs end on every byte of a step, on 16-byte iterations and either side
    of the 64-diagonal seam, and the copies that reach the target's end and that cover a whole diagonal are there."""
    rows = [r for r in family_b() if r[1] < 1023]
    exact = [r for r in rows if cached_runs(r[0])[0] == r[3]]
    assert 2 * len(exact) >= len(rows), len(exact)
    assert {(x + length) % 4 for _s, _d, x, length, _t in exact} == {0, 1, 2, 3}
    assert {(x + length) % 16 for _s, _d, x, length, _t in exact} >= {0, 1, 15}
    assert {d for _s, d, _x, _l, _t in exact} >= {63, 64, 65, 66, 127, 128, 129, 191, 192, 193}
    whole = [r for r in exact if r[2] == 0 and r[4] == 0]
    at_end = [r for r in exact if r[2] != 0 and r[4] == 0]
    assert whole and all(cached_runs(r[0])[1] == 0 for r in whole)
    assert at_end and all(cached_runs(r[0])[1] == 1 for r in at_end if r[1] > 1)
    far = [r for r in family_b() if r[1] >= 1023]
    assert all(cached_model(r[0], 1)[1] >= r[3] for r in far)


def test_family_c_is_one_exempt_run_that_the_neighbour_would_lengthen():
    seqs = family_c()
    for i, (s, p) in enumerate(seqs):
        assert len(s) > p and cached_runs(s) == (len(s) - p, 0), (s, p)
        if i % 2 == 0:
            nxt = seqs[i + 1][0]
            assert len(nxt) == len(s) and cached_runs(s + nxt) == (2 * len(s) - p, 0)      # in phase
    assert sum(len(s) % 16 == 0 for s, _p in seqs) == 2 * 5 * 6          # 16, 32, 48, 64, 128, 256


# ------------------------------------------------------------------ CPU: the closed form standing alone
def _rule_grid():
    grid = [(n, start, R, flag) for n in range(13) for start in range(-3, 16) for R in range(max(n - 1, 0) + 1)
            for flag in (0, 1)]
    top = 2 ** 31 - 1
    for n in (top - 2, top - 1, top):
        for start in (-top - 1, -top, -top + 1, -1, 0, 1, 2, 10, top - 2, top - 1, top):
            for R in (0, 1, 2, 9, 10, n - 3, n - 2, n - 1):
                grid.extend((n, start, R, flag) for flag in (0, 1))
    for n in range(13):
        for start in (-top - 1, -top, top - 1, top):
            grid.extend((n, start, R, flag) for R in range(max(n - 1, 0) + 1) for flag in (0, 1))
    return grid


def test_rule_program_under_sanitizers(tmp_path):
    """csrc/kmin_rule.h built for the CPU with AddressSanitizer + UBSan (tests/host/kmin_rule.cpp): k and the reported
    flag of every (n, start, R, flag) with n up to 12, and around n = 2^31 - 1 and start = +-(2^31 - 1), against
    closed_form and reported_flag."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "kmin_rule")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "host", "kmin_rule.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    grid = _rule_grid()
    assert len(grid) > 3000
    text = "".join("%d %d %d %d\n" % row for row in grid)
    proc = subprocess.run([exe], input=text.encode(), capture_output=True, env=env, timeout=120)
    assert proc.returncode == 0 and proc.stdout.endswith(b"KMIN RULE OK\n"), (proc.stdout[-500:], proc.stderr[-3000:])
    assert b"ERROR: AddressSanitizer" not in proc.stderr and b"runtime error" not in proc.stderr, proc.stderr[-3000:]
    got = [tuple(map(int, line.split())) for line in proc.stdout.decode().split("\n")[:-2]]
    want = [(closed_form(n, start, R, flag), reported_flag(n, R, flag)) for n, start, R, flag in grid]
    assert len(got) == len(want)
    for row, g, w in zip(grid, got, want):
        assert g == w, row


# ------------------------------------------------------------------ GPU
def _expected(seqs, start):
    """(k, R, flag, has_flag) arrays from the models; has_flag marks the targets short enough for runs_model."""
    k = np.zeros(len(seqs), np.int32)
    rep = np.zeros(len(seqs), np.int32)
    flag = np.zeros(len(seqs), np.uint8)
    has = np.zeros(len(seqs), bool)
    for i, s in enumerate(seqs):
        k[i], rep[i] = cached_model(s, start)
        if len(s) <= FLAG_MAX_N:
            R, f = cached_runs(s)
            assert R == rep[i], (s, start)
            flag[i], has[i] = reported_flag(len(s), R, f), True
    return k, rep, flag, has


def _check_call(seqs, start, what):
    """One call: k, R and the flag of every target against the models.  Returns the call's three arrays."""
    got = kmlib.linear_kmin(seqs, start, detail=True)
    k, rep, flag, has = _expected(seqs, start)
    for name, g, w, mask in (("R", got[1], rep, None), ("flag", got[2], flag, has), ("k", got[0], k, None)):
        bad = np.nonzero((g != w) if mask is None else ((g != w) & mask))[0]
        assert bad.size == 0, "%s, start %d: %d of %d targets differ in %s; first: target %d %r (n = %d) got %d, model %d" % (
            what, start, bad.size, len(seqs), name, bad[0], seqs[bad[0]][:80], len(seqs[bad[0]]), g[bad[0]], w[bad[0]])
    return got


def _check_permuted(seqs, start, what, seed):
    """The same targets under a seeded permutation: the units of unlike targets share a block."""
    order = list(range(len(seqs)))
    random.Random(seed).shuffle(order)
    _check_call([seqs[i] for i in order], start, what + ", permuted")


@pytest.mark.gpu
@pytest.mark.parametrize("start", FIXED_STARTS)
@pytest.mark.parametrize("name", ("A1", "A2", "A3", "D"))
def test_gpu_every_lane_and_every_short_string(name, start):
    """A (one case per planted length) and D, one call per start; at start 1 a second call in permuted order."""
    _check_call(corpus(name), start, name)
    if start == 1:
        _check_permuted(corpus(name), start, name, 21)


@pytest.mark.gpu
@pytest.mark.parametrize("start", SEAM_STARTS)
@pytest.mark.parametrize("name", ("B", "C"))
def test_gpu_seams_and_end_mask(name, start):
    """B and C, one call per start, C in the order that puts each target's continuation directly behind it."""
    got = _check_call(corpus(name), start, name)
    if name == "C":
        assert got[1].tolist() == [len(s) - p for s, p in family_c()] and not got[2].any()
    if start == 1:
        _check_permuted(corpus(name), start, name, 22)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("A1", "A2", "A3", "D"))
def test_gpu_start_at_the_length_of_each_target(name):
    """start = n - 1, n, n + 1, n + 2 for every target of A and D: one call per value of start."""
    calls = relative_calls(corpus(name))
    assert sum(map(len, calls.values())) == 4 * len(corpus(name)) and len(calls) <= 20
    for start in sorted(calls):
        _check_call(calls[start], start, name + " at its own length")


def _staging_sample():
    rng = random.Random(23)
    pool = corpus("D") + corpus("A")
    ones = ["A", "C", "G", "T"]
    return ["", "A", ""] + rng.sample(pool, 2000 - 10) + ["", "", "G"] + [rng.choice(ones), "", "T", ""]


@pytest.mark.gpu
def test_gpu_staging_one_target_per_launch(monkeypatch):
    """2 000 targets of D and A with empty and one-letter targets among them, leading and trailing: staged 16 bytes
    at a time every non-empty target is alone in its launch and a group of empty ones launches nothing; at 4 096
    bytes a launch holds a few dozen.  The arrays are those of one launch."""
    seqs = _staging_sample()
    assert len(seqs) == 2000 and seqs[0] == "" and seqs[-1] == "" and max(map(len, seqs)) == 68
    one = _check_call(seqs, 1, "staging sample")
    for stage in ("16", "4096"):
        monkeypatch.setenv("KM_KMIN_STAGE_BYTES", stage)
        chunked = kmlib.linear_kmin(seqs, 1, detail=True)
        for x, y in zip(one, chunked):
            assert np.array_equal(x, y), stage


@pytest.mark.gpu
def test_gpu_c_abi_with_offsets_that_do_not_start_at_zero():
    """km_linear_kmin called directly: the text starts 7 bytes into the array (an unaligned source, base_off[0] == 7)
    and ends without a byte to spare; about a hundred targets of B, the same rows as through the binding."""
    seqs = corpus("B")[5::31]
    assert 100 <= len(seqs) <= 110 and max(map(len, seqs)) > 1000
    want = _check_call(seqs, 1, "B sample")
    lib = kmlib.load()
    blob = np.frombuffer(b"ACGTACG" + "".join(seqs).encode("ascii"), np.uint8)
    offs = np.zeros(len(seqs) + 1, np.uint64)
    offs[0] = 7
    offs[1:] = 7 + np.cumsum([len(s) for s in seqs])
    assert int(offs[-1]) == blob.size
    k = np.full(len(seqs), -7, np.int32)
    rep = np.full(len(seqs), -7, np.int32)
    flag = np.full(len(seqs), 7, np.uint8)
    P = kmlib.ptr
    assert lib.km_linear_kmin(0, P(blob), P(offs), len(seqs), 1, P(k), P(rep), P(flag), None) == 0
    for x, y in zip(want, (k, rep, flag)):
        assert np.array_equal(x, y)
