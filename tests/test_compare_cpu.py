"""`compare` where no GPU is needed: the model every GPU test of tests/test_compare.py compares with, the parser, the
text of km_amd.count.format_compare byte for byte, the refusals of km_amd.count.compare_files that come before a
counter exists, and csrc/cooc_rule.h driven on the CPU under AddressSanitizer + UBSan as a stand-alone program
(tests/host/cooc_rule.cpp says what it covers).

The model is written from the rule of include/kmgpu.h alone, with Python sets, and shares no code with the kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from km_amd import cli
from km_amd import count as kc
from km_amd import lib as kmlib

HERE = os.path.dirname(os.path.abspath(__file__))
TOP = 0xFFFFFFFF


# ------------------------------------------------------------------ the model
def compare_model(inputs, lower=1, upper=TOP):
    """inputs: (keys, counts) per input, in order -> dict(n_inputs, union, shared[n][n], in_exactly[n + 1], private[n])
    of plain ints.  Input i is the set of the keys of its records with max(lower, 1) <= count <= upper."""
    sets = []
    for keys, counts in inputs:
        keys = np.asarray(keys, np.uint64).tolist()
        counts = np.asarray(counts, np.uint32).tolist()
        sets.append({key for key, c in zip(keys, counts) if c != 0 and lower <= c <= upper})
    n = len(sets)
    everything = set().union(*sets) if sets else set()
    held = {key: sum(key in s for s in sets) for key in everything}
    in_exactly = [0] * (n + 1)
    for m in held.values():
        in_exactly[m] += 1
    return {"n_inputs": n, "union": len(everything),
            "shared": [[len(sets[i] & sets[j]) for j in range(n)] for i in range(n)],
            "in_exactly": in_exactly,
            "private": [sum(1 for key in s if held[key] == 1) for s in sets]}


def same_result(got, want):
    """A result of Counter.cooccurrence / compare_files against the model's: every number."""
    n = want["n_inputs"]
    return got["n_inputs"] == n and got["union"] == want["union"] and \
        np.asarray(got["shared"]).shape == (n, n) and np.asarray(got["shared"]).tolist() == want["shared"] and \
        np.asarray(got["in_exactly"]).tolist() == want["in_exactly"] and \
        np.asarray(got["private"]).tolist() == want["private"]


def test_model_on_hand_written_cases():
    a = ([1, 2, 3, 4], [1, 1, 5, 9])
    b = ([3, 4, 5], [2, 1, 1])
    c = ([], [])
    m = compare_model([a, b, c])
    assert m == {"n_inputs": 3, "union": 5, "shared": [[4, 2, 0], [2, 3, 0], [0, 0, 0]], "in_exactly": [0, 3, 2, 0],
                 "private": [2, 1, 0]}
    # the cut is per record, on both sides; count 0 is absent whatever lower is
    m = compare_model([a, b], lower=2)
    assert (m["shared"], m["union"], m["in_exactly"], m["private"]) == ([[2, 1], [1, 1]], 2, [0, 1, 1], [1, 0])
    m = compare_model([a, b], lower=1, upper=1)
    assert (m["shared"], m["union"], m["in_exactly"], m["private"]) == ([[2, 0], [0, 2]], 4, [0, 4, 0], [2, 2])
    m = compare_model([([7, 8], [0, 3]), ([7, 8], [1, 0])], lower=0)
    assert (m["shared"], m["union"]) == ([[1, 0], [0, 1]], 2)
    # a key with two records, one passing the cut: present; twice the same records: nothing changes
    m = compare_model([([9, 9, 6], [1, 50, 1]), ([9], [60])], lower=40)
    assert (m["shared"], m["private"], m["in_exactly"]) == ([[1, 1], [1, 1]], [0, 0], [0, 0, 1])
    assert compare_model([(a[0] * 2, a[1] * 2), b]) == compare_model([a, b])
    # one input, no input, the same input twice
    assert compare_model([a]) == {"n_inputs": 1, "union": 4, "shared": [[4]], "in_exactly": [0, 4], "private": [4]}
    assert compare_model([]) == {"n_inputs": 0, "union": 0, "shared": [], "in_exactly": [0], "private": []}
    m = compare_model([a, a])
    assert (m["shared"], m["in_exactly"], m["private"]) == ([[4, 4], [4, 4]], [0, 0, 4], [0, 0])
    # shared is symmetric and its diagonal the sets' sizes, the spectrum sums to the union
    rng = np.random.default_rng(5)
    inputs = [(rng.integers(0, 40, 30), rng.integers(0, 4, 30)) for _ in range(5)]
    m = compare_model(inputs, lower=2)
    assert all(m["shared"][i][j] == m["shared"][j][i] for i in range(5) for j in range(5))
    assert sum(m["in_exactly"]) == m["union"] and sum(m["private"]) == m["in_exactly"][1]


# ------------------------------------------------------------------ the parser
def test_parser_rules(capsys):
    p = cli.build_parser()
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["compare"], p)
    assert e.value.code == 2
    args = cli.parse_args(["compare", "a.jf"], p)
    assert (args.lower_count, args.upper_count, args.matrix, args.summary, args.spectrum, args.output, args.inputs) == (
        1, TOP, None, None, None, None, ["a.jf"])
    args = cli.parse_args(["compare", "-L", "3", "-U", "70", "--matrix", "jaccard", "--summary", "s.tsv", "--spectrum", "m.tsv",
                           "-o", "out.tsv", "a.jf", "b.jf", "c.jf"], p)
    assert (args.lower_count, args.upper_count, args.matrix, args.summary, args.spectrum, args.output, args.inputs) == (
        3, 70, "jaccard", "s.tsv", "m.tsv", "out.tsv", ["a.jf", "b.jf", "c.jf"])
    assert cli.parse_args(["compare", "--matrix", "shared", "a.jf"], p).matrix == "shared"
    for bad in (["-L", "-1"], ["-L", "x"], ["-U", "4294967296"], ["-U", "1.5"], ["--matrix", "cosine"], ["--matrix"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["compare"] + bad + ["a.jf"], p)
        assert e.value.code == 2, bad
    capsys.readouterr()


# ------------------------------------------------------------------ the text
HAND = {"n_inputs": 3, "union": 9, "records": [7, 5, 0],
        "shared": np.array([[6, 2, 0], [2, 5, 0], [0, 0, 0]], np.uint64),
        "in_exactly": np.array([0, 7, 2, 0], np.uint64), "private": np.array([4, 3, 0], np.uint64)}
NAMES = ["a.jf", "dir/b.jf", "c.jf"]


def test_format_pairs_byte_for_byte():
    assert kc.format_compare(NAMES, HAND) == kc.format_compare(NAMES, HAND, "pairs") == (
        "a\tb\tdistinct_a\tdistinct_b\tshared\tjaccard\tcontain_a\tcontain_b\n"
        "a.jf\tdir/b.jf\t6\t5\t2\t0.222222\t0.333333\t0.400000\n"
        "a.jf\tc.jf\t6\t0\t0\t0.000000\t0.000000\tNA\n"
        "dir/b.jf\tc.jf\t5\t0\t0\t0.000000\t0.000000\tNA\n")


def test_format_both_matrices_byte_for_byte():
    assert kc.format_compare(NAMES, HAND, "shared") == (
        "\ta.jf\tdir/b.jf\tc.jf\n"
        "a.jf\t6\t2\t0\n"
        "dir/b.jf\t2\t5\t0\n"
        "c.jf\t0\t0\t0\n")
    assert kc.format_compare(NAMES, HAND, "jaccard") == (
        "\ta.jf\tdir/b.jf\tc.jf\n"
        "a.jf\t1.000000\t0.222222\t0.000000\n"
        "dir/b.jf\t0.222222\t1.000000\t0.000000\n"
        "c.jf\t0.000000\t0.000000\tNA\n")


def test_format_summary_and_spectrum_byte_for_byte():
    assert kc.format_compare(NAMES, HAND, "summary") == (
        "input\trecords\tdistinct\tprivate\n"
        "a.jf\t7\t6\t4\n"
        "dir/b.jf\t5\t5\t3\n"
        "c.jf\t0\t0\t0\n")
    assert kc.format_compare(NAMES, HAND, "spectrum") == "1\t7\n2\t2\n3\t0\n"


def test_format_two_empty_inputs_and_one_input_alone():
    empty = {"n_inputs": 2, "union": 0, "records": [0, 3], "shared": np.zeros((2, 2), np.uint64),
             "in_exactly": np.zeros(3, np.uint64), "private": np.zeros(2, np.uint64)}
    assert kc.format_compare(["x", "y"], empty) == (
        "a\tb\tdistinct_a\tdistinct_b\tshared\tjaccard\tcontain_a\tcontain_b\n"
        "x\ty\t0\t0\t0\tNA\tNA\tNA\n")
    assert kc.format_compare(["x", "y"], empty, "jaccard") == "\tx\ty\nx\tNA\tNA\ny\tNA\tNA\n"
    assert kc.format_compare(["x", "y"], empty, "spectrum") == "1\t0\n2\t0\n"
    one = {"n_inputs": 1, "union": 4, "records": [4], "shared": np.array([[4]], np.uint64),
           "in_exactly": np.array([0, 4], np.uint64), "private": np.array([4], np.uint64)}
    assert kc.format_compare(["only.jf"], one) == "a\tb\tdistinct_a\tdistinct_b\tshared\tjaccard\tcontain_a\tcontain_b\n"
    assert kc.format_compare(["only.jf"], one, "shared") == "\tonly.jf\nonly.jf\t4\n"
    assert kc.format_compare(["only.jf"], one, "jaccard") == "\tonly.jf\nonly.jf\t1.000000\n"
    assert kc.format_compare(["only.jf"], one, "summary") == "input\trecords\tdistinct\tprivate\nonly.jf\t4\t4\t4\n"
    assert kc.format_compare(["only.jf"], one, "spectrum") == "1\t4\n"
    with pytest.raises(ValueError):
        kc.format_compare(["only.jf"], one, "cosine")
    with pytest.raises(ValueError):
        kc.format_compare(["x", "y"], one)
    # the text of the model's own result: lists of ints format as arrays do
    m = dict(compare_model([([1, 2, 3], [1, 1, 1]), ([3], [1])]), records=[3, 1])
    assert kc.format_compare(["p", "q"], m).splitlines()[1] == "p\tq\t3\t1\t1\t0.333333\t0.333333\t1.000000"


# ------------------------------------------------------------------ refusals before the GPU
def test_compare_files_refuses_before_any_counter(tmp_path, monkeypatch):
    made = []
    monkeypatch.setattr(kmlib, "Counter", lambda *a, **kw: made.append((a, kw)) or pytest.fail("a counter was created"))
    keys, counts = np.array([1, 2, 3], np.uint64), np.array([3, 4, 5], np.uint32)
    a = str(tmp_path / "a.jf")
    b = str(tmp_path / "b.jf")
    c = str(tmp_path / "c.jf")
    kc.write_records(a, keys, counts, 31, True)
    kc.write_records(b, keys, counts, 21, True)
    kc.write_records(c, keys, counts, 31, False)
    for other, said in ((b, "k=21"), (c, "canonical=False")):
        with pytest.raises(ValueError) as e:
            kc.compare_files([a, a, other])
        assert other in str(e.value) and a in str(e.value) and said in str(e.value) and "3 inputs" in str(e.value)
    missing = str(tmp_path / "no_such.jf")
    with pytest.raises(ValueError) as e:
        kc.compare_files([a, missing])
    assert missing in str(e.value) and "2" in str(e.value)
    with pytest.raises(ValueError) as e:
        kc.compare_files([a] * 33)
    assert "33 inputs" in str(e.value) and "32" in str(e.value)
    with pytest.raises(ValueError) as e:
        kc.compare_files([])
    assert "0 inputs" in str(e.value)
    assert made == []


def test_command_reports_a_refusal_with_status_1_and_opens_no_output(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(kmlib, "Counter", lambda *a, **kw: pytest.fail("a counter was created"))
    a = str(tmp_path / "a.jf")
    b = str(tmp_path / "b.jf")
    kc.write_records(a, np.array([1], np.uint64), np.array([1], np.uint32), 31, True)
    kc.write_records(b, np.array([1], np.uint64), np.array([1], np.uint32), 25, True)
    out = tmp_path / "out.tsv"
    with pytest.raises(SystemExit) as e:
        cli.main(["compare", "-o", str(out), "--summary", str(tmp_path / "s.tsv"), a, b])
    assert str(e.value.code).startswith("ERROR: compare: ") and "k=25" in str(e.value.code)
    assert not out.exists() and not (tmp_path / "s.tsv").exists()
    capsys.readouterr()
    # as a process: the message on standard error, status 1
    import sys
    proc = subprocess.run([sys.executable, "-m", "km_amd", "compare", a, str(tmp_path / "no_such.jf")], capture_output=True,
                          cwd=os.path.dirname(HERE), timeout=120)
    assert proc.returncode == 1 and proc.stdout == b"" and proc.stderr.startswith(b"ERROR: compare: "), proc.stderr[-500:]
    proc = subprocess.run([sys.executable, "-m", "km_amd", "compare"], capture_output=True, cwd=os.path.dirname(HERE), timeout=120)
    assert proc.returncode == 2 and proc.stdout == b""


# ------------------------------------------------------------------ the rule header on the CPU
def test_rule_program_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "cooc_rule")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "host", "cooc_rule.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe], capture_output=True, env=env, timeout=600)
    assert proc.returncode == 0, (proc.stdout[-2000:], proc.stderr[-3000:])
    assert b"ERROR: AddressSanitizer" not in proc.stderr and b"runtime error" not in proc.stderr, proc.stderr[-3000:]
    done = re.fullmatch(rb"COOC RULE OK (\d+) cases\n", proc.stdout)
    assert done, proc.stdout[-2000:]
    # per n: the mapping, all zero, all one, 5 single slots, 3 single inputs, 8 rounds of 3 random kinds
    assert int(done.group(1)) >= 32 * (1 + 1 + 1 + 5 + 3 + 8 * 3)
