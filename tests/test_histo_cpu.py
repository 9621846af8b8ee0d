"""The count histogram and the table statistics, the parts that need no GPU: the bin layout (km_histo_layout), the two
text writers (km_amd.count.format_histo / format_stats), what km_counter_histo / km_jf_histo refuse before any device
work, the sanitizer build of csrc/histo_layout.h and the argument parser.  The GPU side is tests/test_histo.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from km_amd import cli
from km_amd import count as kc
from km_amd import lib as kmlib

HERE = os.path.dirname(os.path.abspath(__file__))
JF_DIR = os.path.join(HERE, "data", "jf")
CATALOG = os.path.join(HERE, "data", "catalog", "GRCh38")
ITD = os.path.join(JF_DIR, "03H116_ITD.jf")
TOP = 0xFFFFFFFF
KM_E_IO, KM_E_FORMAT, KM_E_ARG, KM_E_CAPACITY = 1, 2, 4, 8


def test_layout_of_the_quoted_cases():
    assert kmlib.histo_layout() == (1, 10001)
    assert kmlib.histo_layout(1, 10000, 1) == (1, 10001)
    assert kmlib.histo_layout(5, 20, 5) == (1, 5)
    assert kmlib.histo_layout(100, 200, 10) == (90, 13)
    assert kmlib.histo_layout(1, 1, 1) == (1, 2)
    lib = kmlib.load()
    assert lib.km_histo_layout(1, 10000, 1, None, None) == 0             # either output may be NULL


@pytest.mark.parametrize("args, named", [
    ((1, 10, 0), "increment 0"),
    ((11, 10, 1), "11"),
    ((1, 2 ** 64 - 2, 1), "18446744073709551614"),
    ((1, 2 ** 26, 1), "67108865"),
])
def test_layout_refuses_with_a_message_naming_the_value(args, named):
    with pytest.raises(kmlib.KmError) as e:
        kmlib.histo_layout(*args)
    assert e.value.code == KM_E_ARG and named in str(e.value)


def test_format_histo_against_literal_strings():
    bins = np.array([3, 0, 7, 0, 2 ** 40], np.uint64)
    assert kc.format_histo(90, 10, bins) == "90 3\n110 7\n130 1099511627776\n"
    assert kc.format_histo(90, 10, bins, full=True) == "90 3\n100 0\n110 7\n120 0\n130 1099511627776\n"
    assert kc.format_histo(1, 1, np.zeros(4, np.uint64)) == ""
    assert kc.format_histo(1, 1, np.zeros(3, np.uint64), full=True) == "1 0\n2 0\n3 0\n"
    assert kc.format_histo(1, 1, np.zeros(0, np.uint64), full=True) == ""
    assert kc.format_histo(1, 1, [5, 6]) == "1 5\n2 6\n"


def test_format_stats_against_literal_strings():
    assert kc.format_stats({"unique": 7, "distinct": 12, "total": 2 ** 33 + 1, "max_count": TOP}) == \
        "Unique:    7\nDistinct:  12\nTotal:     8589934593\nMax_count: 4294967295\n"
    assert kc.format_stats({"unique": 0, "distinct": 0, "total": 0, "max_count": 0}) == \
        "Unique:    0\nDistinct:  0\nTotal:     0\nMax_count: 0\n"


def test_refusals_come_before_any_device_work(tmp_path):
    """No GPU is needed for any of these: each fails with its code on a machine without one."""
    lib = kmlib.load()
    dflt = (1, 10000, 1, 1, TOP)
    assert lib.km_counter_histo(None, *dflt, None, 0, None) == KM_E_ARG
    assert lib.km_jf_histo(0, None, *dflt, None, 0, None, None, None, None) == KM_E_ARG
    assert lib.km_histo_kernel_ms(None) == KM_E_ARG
    with pytest.raises(kmlib.KmError) as e:
        kc.histo_file(str(tmp_path / "no_such.jf"))
    assert e.value.code == KM_E_IO
    with pytest.raises(kmlib.KmError) as e:
        kc.histo_file(os.path.join(CATALOG, "IDH1_R132.fa"))
    assert e.value.code == KM_E_FORMAT
    with pytest.raises(kmlib.KmError) as e:
        kc.histo_file(ITD, increment=0)
    assert e.value.code == KM_E_ARG
    with pytest.raises(kmlib.KmError) as e:
        kc.histo_file(ITD, low=9, high=8)
    assert e.value.code == KM_E_ARG
    bins = np.zeros(10000, np.uint64)
    assert lib.km_jf_histo(0, os.fsencode(ITD), *dflt, kmlib.ptr(bins), bins.size, None, None, None, None) == KM_E_CAPACITY
    assert b"10001" in lib.km_last_error() and not bins.any()
    assert lib.km_jf_histo(-1, os.fsencode(ITD), *dflt, None, 0, None, None, None, None) == KM_E_ARG


def test_layout_rule_and_writers_under_the_sanitizers(tmp_path):
    """csrc/histo_layout.h built for the CPU with AddressSanitizer + UBSan (tests/host/histo_layout.cpp): the bin rule
    against a brute-force loop over a grid of small (low, high, inc), the refusals, the two writers."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "histo_layout")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "host", "histo_layout.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert proc.returncode == 0 and "LAYOUT OK" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in proc.stderr and "runtime error" not in proc.stderr, proc.stderr[-3000:]


def test_parser_accepts_histo_and_stats():
    p = cli.build_parser()
    a = p.parse_args(["histo", "-h", "100", "-l", "2", "-i", "2", "-f", "x.jf"])
    assert (a.low, a.high, a.increment, a.full, a.lower_count, a.upper_count, a.output, a.db) == (
        2, 100, 2, True, 1, TOP, None, "x.jf")
    a = p.parse_args(["histo", "x.jf"])
    assert (a.low, a.high, a.increment, a.full) == (1, 10000, 1, False)
    a = p.parse_args(["histo", "-L", "3", "-U", "9", "-o", "h.txt", "x.jf"])
    assert (a.lower_count, a.upper_count, a.output) == (3, 9, "h.txt")
    a = p.parse_args(["stats", "-L", "2", "-U", "50", "x.jf"])
    assert (a.lower_count, a.upper_count, a.output, a.db) == (2, 50, None, "x.jf")
    for bad in (["histo", "-l", "-1", "x.jf"], ["histo", "-h", "-5", "x.jf"], ["histo", "-i", "-2", "x.jf"],
                ["histo", "-L", "-1", "x.jf"], ["stats", "-U", "-1", "x.jf"], ["stats", "-U", "4294967296", "x.jf"],
                ["histo", "-L", "4294967296", "x.jf"]):
        with pytest.raises(SystemExit) as e:                             # negative, or no 32-bit count: refused here
            p.parse_args(bad)
        assert e.value.code == 2
    with pytest.raises(SystemExit) as e:                                 # help is --help only on this sub-parser
        p.parse_args(["histo", "--help"])
    assert e.value.code == 0
    assert p.parse_args(["count", "--histo", "h.txt", "-o", "o.jf", "r.fq"]).histo == "h.txt"
    assert p.parse_args(["merge", "--histo", "h.txt", "a.jf", "b.jf"]).histo == "h.txt"
    assert p.parse_args(["count", "r.fq"]).histo is None and p.parse_args(["merge", "a.jf"]).histo is None
