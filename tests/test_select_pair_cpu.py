"""The paired selection of FASTQ reads (km_select_pair_*, `bait -1 .. -2 ..`) where no GPU is needed: the model every
paired test compares with, that model pinned on cases computed by hand from the rule of include/kmgpu.h,
csrc/select_pair_rule.h driven on the CPU under AddressSanitizer + UBSan, and the command's argument rules.

``model_pair_select`` is written from the rule text alone on top of ``fastq_records`` and ``read_hits`` of
tests/test_select_cpu.py; it shares nothing with csrc/select_pair_rule.h."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from km_amd import cli
import test_select_cpu as sm

HERE = os.path.dirname(os.path.abspath(__file__))
RULES = ("any", "both", "sum")
RULE_CODE = {"any": 0, "both": 1, "sum": 2}
fastq, random_bases, kmers_of = sm.fastq, sm.random_bases, sm.kmers_of


# ------------------------------------------------------------------ the model
class PairError(Exception):
    """kind: "malformed" (mate, and the Malformed of that mate as .cause), "names" (index: the first pair whose names
    differ) or "count" (mate: the one with more records, index: the first pair without a partner)."""

    def __init__(self, kind, index=None, mate=None, cause=None):
        Exception.__init__(self, "%s pair %r mate %r %r" % (kind, index, mate, cause))
        self.kind, self.index, self.mate, self.cause = kind, index, mate, cause


def pair_name(header):
    """The name of a record from its raw header line."""
    name = header[1:]
    for i, ch in enumerate(name):
        if ch in b" \t\r\n":
            name = name[:i]
            break
    if len(name) >= 2 and name[-2:] in (b"/1", b"/2"):
        name = name[:-2]
    return name


def pair_score(h1, h2, rule):
    if rule == "any":
        return max(h1, h2)
    if rule == "both":
        return min(h1, h2)
    assert rule == "sum"
    return min(h1 + h2, 2 ** 32 - 1)


def pair_keep(h1, h2, rule, min_hits, invert):
    return (pair_score(h1, h2, rule) >= min_hits) != bool(invert)


def _closed(out):
    return out + b"\n" if out and not out.endswith(b"\n") else out


def model_pair_select(text1, text2, table, k, canonical, min_hits=1, invert=False, min_qual=0, rule="any", check_names=True):
    """The bytes two final streams leave on the two descriptors -> (out1, out2), or PairError."""
    mates = []
    for mate, text in ((1, text1), (2, text2)):
        try:
            mates.append(sm.fastq_records(text) if text else [])
        except sm.Malformed as e:
            raise PairError("malformed", mate=mate, cause=e) from e
    n = min(len(mates[0]), len(mates[1]))
    if check_names:
        for r in range(n):
            if pair_name(mates[0][r][0]) != pair_name(mates[1][r][0]):
                raise PairError("names", index=r)
    if len(mates[0]) != len(mates[1]):
        raise PairError("count", index=n, mate=1 if len(mates[0]) > n else 2)
    out = [[], []]
    for rec1, rec2 in zip(*mates):
        h1 = sm.read_hits(sm._content(rec1[1]), sm._content(rec1[3]), table, k, canonical, min_qual)
        h2 = sm.read_hits(sm._content(rec2[1]), sm._content(rec2[3]), table, k, canonical, min_qual)
        if pair_keep(h1, h2, rule, min_hits, invert):
            out[0].append(b"".join(rec1))
            out[1].append(b"".join(rec2))
    return _closed(b"".join(out[0])), _closed(b"".join(out[1]))


def kept_pairs(text1, text2, table, k, canonical, min_hits=1, invert=False, min_qual=0, rule="any"):
    """The indices of the kept pairs of two well-formed streams of equal record count."""
    h1 = sm.model_hits(text1, table, k, canonical, min_qual)
    h2 = sm.model_hits(text2, table, k, canonical, min_qual)
    return [r for r, (a, b) in enumerate(zip(h1, h2)) if pair_keep(a, b, rule, min_hits, invert)]


# ------------------------------------------------------------------ the model on cases computed by hand
# keep for min_hits = 2, not inverted: rows h1 = 0..3, columns h2 = 0..3
KEEP_AT_2 = {
    "any": [[0, 0, 1, 1],       # max(h1, h2) >= 2
            [0, 0, 1, 1],
            [1, 1, 1, 1],
            [1, 1, 1, 1]],
    "both": [[0, 0, 0, 0],      # min(h1, h2) >= 2
             [0, 0, 0, 0],
             [0, 0, 1, 1],
             [0, 0, 1, 1]],
    "sum": [[0, 0, 1, 1],       # h1 + h2 >= 2
            [0, 1, 1, 1],
            [1, 1, 1, 1],
            [1, 1, 1, 1]],
}


def test_the_truth_table_of_the_three_rules():
    for rule in RULES:
        for h1, h2 in itertools.product(range(4), repeat=2):
            want = bool(KEEP_AT_2[rule][h1][h2])
            assert pair_keep(h1, h2, rule, 2, False) is want, (rule, h1, h2)
            assert pair_keep(h1, h2, rule, 2, True) is (not want), (rule, h1, h2)
    # the other two thresholds from the definitions, written out per rule
    for h1, h2 in itertools.product(range(4), repeat=2):
        assert pair_keep(h1, h2, "any", 1, False) is (h1 >= 1 or h2 >= 1)
        assert pair_keep(h1, h2, "both", 1, False) is (h1 >= 1 and h2 >= 1)
        assert pair_keep(h1, h2, "sum", 1, False) is (h1 + h2 >= 1)
        assert pair_keep(h1, h2, "any", 3, False) is (h1 == 3 or h2 == 3)
        assert pair_keep(h1, h2, "both", 3, False) is (h1 == 3 and h2 == 3)
        assert pair_keep(h1, h2, "sum", 3, False) is ((h1, h2) not in ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)))
        for rule in RULES:
            for min_hits in (1, 2, 3):
                assert pair_keep(h1, h2, rule, min_hits, True) is not pair_keep(h1, h2, rule, min_hits, False)
    assert pair_score(2 ** 32 - 1, 1, "sum") == 2 ** 32 - 1 and pair_score(2 ** 31, 2 ** 31, "sum") == 2 ** 32 - 1


def test_the_truth_table_through_the_model():
    """Reads with 0, 1, 2 and 3 windows of the table (k = 3), every combination as a pair."""
    table = {sm._pack(b"ACG"): 1}
    reads = [b"TTT", b"ACG", b"ACGTACG", b"ACGACGACG"]
    assert [sm.read_hits(r, b"I" * len(r), table, 3, False) for r in reads] == [0, 1, 2, 3]
    pairs = list(itertools.product(range(4), repeat=2))
    names = [b"p%d" % i for i in range(len(pairs))]
    text1 = fastq([reads[a] for a, _ in pairs], names=names)
    text2 = fastq([reads[b] for _, b in pairs], names=names)
    recs1 = [b"".join(r) for r in sm.fastq_records(text1)]
    recs2 = [b"".join(r) for r in sm.fastq_records(text2)]
    for rule in RULES:
        for invert in (False, True):
            want = [i for i, (a, b) in enumerate(pairs) if bool(KEEP_AT_2[rule][a][b]) != invert]
            out1, out2 = model_pair_select(text1, text2, table, 3, False, min_hits=2, invert=invert, rule=rule)
            assert out1 == b"".join(recs1[i] for i in want) and out2 == b"".join(recs2[i] for i in want), (rule, invert)
            assert kept_pairs(text1, text2, table, 3, False, min_hits=2, invert=invert, rule=rule) == want


def test_names():
    agree = [(b"a/1", b"a/2"), (b"a/1", b"a/1"), (b"a", b"a/2"), (b"r x=1", b"r y=2"), (b"r\tx", b"r z"), (b"", b""),
             (b"/1", b""), (b" c1", b"\tc2"), (b"a/1 c", b"a/2\td"), (b"ab/2", b"ab")]
    differ = [(b"a/3", b"a"), (b"read1", b"read10"), (b"a", b"b"), (b"a/1/1", b"a/1"), (b"a /1", b"a/1x"), (b"1", b""),
              (b"a/", b"a")]
    for x, y in agree:
        assert pair_name(b"@" + x + b"\n") == pair_name(b"@" + y + b"\r\n"), (x, y)
    for x, y in differ:
        assert pair_name(b"@" + x + b"\n") != pair_name(b"@" + y + b"\n"), (x, y)
    assert pair_name(b"@a/1\n") == b"a" and pair_name(b"@/1\n") == b"" and pair_name(b"@/\n") == b"/"
    assert pair_name(b"@x/2 /1\n") == b"x" and pair_name(b"@abc") == b"abc" and pair_name(b"@a/1\r\n") == b"a"
    table = {sm._pack(b"ACG"): 1}
    read = b"ACGT"
    for x, y in agree:
        out = model_pair_select(fastq([read], names=[x]), fastq([read], names=[y]), table, 3, True)
        assert out == (fastq([read], names=[x]), fastq([read], names=[y]))
    for x, y in differ:
        t1, t2 = fastq([read, read], names=[b"q", x]), fastq([read, read], names=[b"q/2", y])
        with pytest.raises(PairError) as e:
            model_pair_select(t1, t2, table, 3, True)
        assert (e.value.kind, e.value.index) == ("names", 1)
        assert model_pair_select(t1, t2, table, 3, True, check_names=False) == (t1, t2)


def test_count_mismatch_and_malformed_mates():
    table = {sm._pack(b"ACG"): 1}
    three, two = fastq([b"ACGT"] * 3), fastq([b"ACGT"] * 2)
    with pytest.raises(PairError) as e:
        model_pair_select(three, two, table, 3, True)
    assert (e.value.kind, e.value.mate, e.value.index) == ("count", 1, 2)
    with pytest.raises(PairError) as e:
        model_pair_select(two, three, table, 3, True, check_names=False)
    assert (e.value.kind, e.value.mate, e.value.index) == ("count", 2, 2)
    with pytest.raises(PairError) as e:
        model_pair_select(b"", two, table, 3, True)
    assert (e.value.kind, e.value.mate, e.value.index) == ("count", 2, 0)
    assert model_pair_select(b"", b"", table, 3, True) == (b"", b"")
    # the streams before the final call hold what they hold: a shorter mate is no error while more may come, which is
    # why the model takes whole streams only
    bad = two[:9] + b"-" + two[10:]
    assert two[9:10] == b"+"
    with pytest.raises(PairError) as e:
        model_pair_select(two, bad, table, 3, True)
    assert (e.value.kind, e.value.mate, e.value.cause.kind, e.value.cause.offset) == ("malformed", 2, sm.NO_PLUS, 9)
    # the last newline is decided per output
    out = model_pair_select(two[:-1], two, table, 3, True)
    assert out == (two, two)
    out = model_pair_select(fastq([b"ACGT", b"TTTT"], last_newline=False), fastq([b"TTTT", b"TTTT"], last_newline=False), table, 3, True)
    assert out == (fastq([b"ACGT"]), fastq([b"TTTT"]))


def test_identical_mates_select_what_the_single_end_rule_selects():
    rng = np.random.default_rng(31)
    genome = random_bases(rng, 400)
    reads = [genome[a:a + 50] if i % 3 else random_bases(rng, 50) for i, a in enumerate(rng.integers(0, 350, 120).tolist())]
    table = kmers_of([genome[:200]], 31, True)
    text = fastq(reads, last_newline=False)
    for rule in ("any", "both"):
        for min_hits in (1, 2, 5):
            for invert in (False, True):
                want = sm.model_select(text, table, 31, True, min_hits, invert)
                assert 0 < len(want) < len(text)
                assert model_pair_select(text, text, table, 31, True, min_hits, invert, rule=rule) == (want, want)
    # (sum doubles every score)
    assert model_pair_select(text, text, table, 31, True, 2, rule="sum")[0] == sm.model_select(text, table, 31, True, 1)


# ------------------------------------------------------------------ csrc/select_pair_rule.h on the CPU
def pair_texts(seed, n, every=(3, 5, 7), lengths=(40, 40), name_lengths=None, eol=b"\n", last_newline=(True, True), quals=False):
    """Two mate texts of n pairs and the table they are baited with: every every[0]-th pair hits through mate 1 only,
    every every[1]-th through mate 2 only, every every[2]-th through both (a later one wins), the rest not at all.  A
    read that hits is at least 33 bases of the genome, so all its windows hit; every other pair that hits through both
    does so with 36 bases of the genome and random ones behind them in either mate: 6 windows each.  With 40-nt reads
    and min_hits = 10 the three rules therefore keep three different sets: any (10, 0), (0, 10), (10, 10); both
    (10, 10) alone; sum those of any and (6, 6).
    lengths: per mate a read length or a (low, high) range to draw from."""
    rng = np.random.default_rng(seed)
    genome = random_bases(rng, 600)

    def length(m):
        return lengths[m] if isinstance(lengths[m], int) else int(rng.integers(lengths[m][0], lengths[m][1] + 1))

    def hit(ln):
        a = int(rng.integers(0, len(genome) - ln))
        return genome[a:a + ln]

    reads, names = ([], []), ([], [])
    for i in range(n):
        which = (False, False)
        if i % every[0] == 0:
            which = (True, False)
        if i % every[1] == 0:
            which = (False, True)
        if i % every[2] == 0:
            which = (True, True)
        partial = which == (True, True) and (i // every[2]) % 2 == 1
        for m in (0, 1):
            ln = length(m)
            if partial:
                reads[m].append(hit(36) + random_bases(rng, max(ln, 36) - 36))
            else:
                reads[m].append(hit(max(ln, 33)) if which[m] else random_bases(rng, ln))
        name = b"read%d" % i if name_lengths is None else (b"%d" % i + b"n" * 40)[:name_lengths[i % len(name_lengths)]]
        names[0].append(name + (b"/1" if i % 2 else b"") + (b" first" if i % 4 == 1 else b""))
        names[1].append(name + (b"/2" if i % 3 else b"") + (b"\tsecond mate" if i % 4 == 2 else b""))
    q = [None, None]
    if quals:
        for m in (0, 1):
            q[m] = []
            for r in reads[m]:
                line = bytearray(b"I" * len(r))
                for at in rng.integers(0, len(r), 2):
                    line[at] = 33 + int(rng.integers(0, 20))
                q[m].append(bytes(line))
    texts = tuple(fastq(reads[m], names=names[m], quals=q[m], eol=eol, last_newline=last_newline[m]) for m in (0, 1))
    return texts[0], texts[1], kmers_of([genome], 31, True)


def pair_rule_input(path, k, canonical, min_hits, invert, min_qual, rule, check_names, table, stages, text1, text2):
    with open(path, "wb") as fh:
        fh.write(b"%d %d %d %d %d %d %d %d %d %d %d\n" % (k, canonical, min_hits, invert, min_qual, RULE_CODE[rule], check_names,
                                                         len(table), len(stages), len(text1), len(text2)))
        fh.write(b" ".join(b"%d" % v for v in stages) + b"\n")
        fh.write(b"".join(b"%d %d\n" % kv for kv in table.items()))
        fh.write(b"TEXT\n" + text1 + text2)


def parse_program_output(got, stages):
    """-> per stage {"pieces", "pairs", "kept", "resent", "failure", "out"}"""
    runs = []
    for stage in stages:
        head, _, got = got.partition(b"\n")
        w = head.split()
        assert w[0::2][:5] == [b"STAGE", b"PIECES", b"PAIRS", b"KEPT", b"RESENT"] and int(w[1]) == stage, head
        run = {"pieces": int(w[3]), "pairs": int(w[5]), "kept": int(w[7]), "resent": (int(w[9]), int(w[10])), "failure": None, "out": []}
        if got.startswith((b"NAMES ", b"COUNT ")):
            line, _, got = got.partition(b"\n")
            run["failure"] = tuple(line.decode().split())
        for m in (1, 2):
            head, _, got = got.partition(b"\n")
            w = head.split()
            assert w[0] == b"OUT%d" % m, head
            run["out"].append(got[:int(w[1])])
            got = got[int(w[1]):]
        runs.append(run)
    assert got == b"SELECT PAIR RULE OK\n"
    return runs


def pair_rule_cases():
    out = []
    for i, rule in enumerate(RULES):
        t1, t2, table = pair_texts(40 + i, 700, lengths=((20, 90), (20, 90)), last_newline=(i != 1, i != 2))
        out.append(("unequal " + rule, 1 + (rule == "sum"), i == 1, 0, rule, 1, t1, t2, table))
    t1, t2, table = pair_texts(44, 300, lengths=(60, (35, 70)), eol=b"\r\n", quals=True, name_lengths=list(range(0, 41)))
    out.append(("quality, names", 2, 0, 53, "any", 1, t1, t2, table))
    t1, t2, table = pair_texts(45, 300, lengths=(40, 75))
    recs = [b"".join(r) for r in sm.fastq_records(t2)]
    out.append(("names differ", 1, 0, 0, "any", 1, t1, b"".join(recs[:211]) + b"@other\n" + recs[211].split(b"\n", 1)[1] + b"".join(recs[212:]), table))
    out.append(("mate 2 short", 1, 0, 0, "both", 1, t1, b"".join(recs[:-1]), table))
    out.append(("mate 1 short", 1, 1, 0, "any", 0, b"".join(recs[:-1]), t1, table))
    # the structured corpus of tests/test_text_kernels_every_k.py, a few KB of it, as mate 1, and its reverse complement
    # or random bases as mate 2; these cases carry their own k and canonical behind the table
    import test_text_kernels_every_k as every_k
    for k in every_k.RULE_KS:
        t1, t2 = every_k.pair_case(k, small=True)
        baits = [sm._content(s) for _, s, _, _ in sm.fastq_records(t1)][::3]
        for canonical in (True, False):
            rule = "sum" if canonical else "both"
            out.append(("structured " + rule, 3 if rule == "sum" else 2, 0, 0, rule, 1, t1, t2, kmers_of(baits, k, canonical), k, canonical))
    return out


def test_pair_rule_program_under_sanitizers(tmp_path):
    """csrc/select_pair_rule.h built for the CPU with AddressSanitizer + UBSan (tests/host/select_pair_rule.cpp): score,
    keep and the two lengths of every pair, the name comparison, the consumed offsets and the re-send loop, and every
    word of both gathers with R below a piece's own record count, into buffers of exactly the device buffers' sizes, at
    staging sizes 256 and 4 096, against the model."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "select_pair_rule")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "host", "select_pair_rule.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    stages = [256, 4096]
    for case in pair_rule_cases():
        name, min_hits, invert, min_qual, rule, check_names, text1, text2, table = case[:9]
        k, canonical = case[9:] or (31, True)
        path = str(tmp_path / "in.bin")
        pair_rule_input(path, k, int(canonical), min_hits, invert, min_qual, rule, check_names, table, stages, text1, text2)
        proc = subprocess.run([exe, path], capture_output=True, env=env, timeout=600)
        assert proc.returncode == 0 and proc.stdout.endswith(b"SELECT PAIR RULE OK\n"), (name, proc.stdout[-300:], proc.stderr[-3000:])
        assert b"ERROR: AddressSanitizer" not in proc.stderr and b"runtime error" not in proc.stderr, proc.stderr[-3000:]
        runs = parse_program_output(proc.stdout, stages)
        full = None                                               # what a run without the name check writes
        if "short" not in name:
            full = model_pair_select(text1, text2, table, k, canonical, min_hits, invert, min_qual, rule, False)
        try:
            want = model_pair_select(text1, text2, table, k, canonical, min_hits, invert, min_qual, rule, bool(check_names))
            error = None
        except PairError as e:
            want, error = None, e
        for stage, run in zip(stages, runs):
            ctx = (name, stage)
            if error is None:
                assert run["failure"] is None and run["out"] == list(want), ctx
                n_pairs = len(sm.fastq_records(text1))
                assert run["pairs"] == n_pairs and 0 < run["kept"] < n_pairs, ctx
                assert len(want[0]) > 0 and run["pieces"] >= len(text1) // stage, ctx
                if "unequal" in name:
                    assert run["resent"][0] > 0 and run["resent"][1] > 0 and run["pieces"] > 10, ctx
            elif error.kind == "names":
                assert run["failure"] == ("NAMES", str(error.index)), ctx
                recs1 = [b"".join(r) for r in sm.fastq_records(text1)]
                kept = kept_pairs(text1, text2, table, k, canonical, min_hits, invert, min_qual, rule)
                done = run["pairs"]                               # the pairs of the pieces before the failing one
                assert 0 < done <= error.index, ctx
                assert run["out"][0] == b"".join(recs1[r] for r in kept if r < done) and run["out"] == [
                    o[:len(g)] for o, g in zip(full, run["out"])], ctx
            else:
                assert error.kind == "count" and run["failure"] == ("COUNT", str(error.mate), str(error.index)), ctx
                assert run["pairs"] == error.index, ctx
                short = min(len(sm.fastq_records(text1)), len(sm.fastq_records(text2)))
                cut1 = b"".join(b"".join(r) for r in sm.fastq_records(text1)[:short])
                cut2 = b"".join(b"".join(r) for r in sm.fastq_records(text2)[:short])
                assert run["out"] == list(model_pair_select(cut1, cut2, table, k, canonical, min_hits, invert, min_qual, rule,
                                                            bool(check_names))), ctx


# ------------------------------------------------------------------ the bait command without a GPU
def test_paired_bait_arguments(tmp_path):
    p = cli.parse_args(["bait", "-d", "db.jf", "-1", "a_1.fq", "-2", "a_2.fq.gz", "-o", "o_1.fq", "-O", "o_2.fq"])
    assert (p.mate1, p.mate2, p.output, p.output2, p.pair_rule, p.no_name_check, p.reads) == (
        ["a_1.fq"], ["a_2.fq.gz"], "o_1.fq", "o_2.fq", None, False, [])
    p = cli.parse_args(["bait", "-d", "db.jf", "-n", "2", "-v", "-Q", "5", "-1", "a_1.fq", "-1", "b_1.fq", "-2", "a_2.fq", "-2", "-",
                        "-o", "o_1.fq", "-O", "o_2.fq", "--pair-rule", "both", "--no-name-check"])
    assert (p.mate1, p.mate2, p.output, p.output2, p.pair_rule, p.no_name_check, p.reads, p.min_hits, p.invert, p.min_qual_char) == (
        ["a_1.fq", "b_1.fq"], ["a_2.fq", "-"], "o_1.fq", "o_2.fq", "both", True, [], 2, True, "5")
    for rule in RULES:
        assert cli.parse_args(["bait", "-d", "db.jf", "-1", "a", "-2", "b", "-o", "x", "-O", "y", "--pair-rule", rule]).pair_rule == rule
    # single-end keeps its fields
    p = cli.parse_args(["bait", "-d", "db.jf", "-o", "o.fq", "a.fq"])
    assert (p.mate1, p.mate2, p.output, p.output2, p.pair_rule, p.no_name_check, p.reads) == ([], [], "o.fq", None, None, False, ["a.fq"])
    pair = ["-1", "a_1.fq", "-2", "a_2.fq"]
    for bad in (["bait", "-d", "db.jf", "-1", "a_1.fq", "-o", "x", "-O", "y"],                          # -1 without -2
                ["bait", "-d", "db.jf", "-2", "a_2.fq", "-o", "x", "-O", "y"],
                ["bait", "-d", "db.jf", "-1", "a", "-1", "b", "-2", "c", "-o", "x", "-O", "y"],         # unequal counts
                ["bait", "-d", "db.jf"] + pair + ["-o", "x", "-O", "y", "more.fq"],                     # positional reads beside them
                ["bait", "-d", "db.jf", "-O", "y", "a.fq"],                                             # paired options, no pair
                ["bait", "-d", "db.jf", "--pair-rule", "any", "a.fq"],
                ["bait", "-d", "db.jf", "--no-name-check", "a.fq"],
                ["bait", "-d", "db.jf"] + pair,                                                         # no outputs
                ["bait", "-d", "db.jf"] + pair + ["-o", "x"],
                ["bait", "-d", "db.jf"] + pair + ["-O", "y"],
                ["bait", "-d", "db.jf"] + pair + ["-o", "x", "-O", "x"],                                # one path
                ["bait", "-d", "db.jf"] + pair + ["-o", "x", "-O", "./x"],
                ["bait", "-d", "db.jf"] + pair + ["-o", "x", "-O", "y", "--pair-rule", "either"],
                ["bait", "-d", "db.jf"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(bad)
        assert e.value.code == 2, bad
