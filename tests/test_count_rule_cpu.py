"""The lane walk of the counting kernels (csrc/count_rule.h: k_count_insert, k_count_filtered, k_sketch_note,
k_count_solid) where no GPU is needed: the header driven on the CPU under AddressSanitizer + UBSan as a stand-alone
program, against a naive enumeration of the windows (tests/host/count_rule.cpp says what it covers)."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_rule_program_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "count_rule")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "host", "count_rule.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe], capture_output=True, env=env, timeout=600)
    assert proc.returncode == 0, (proc.stdout[-2000:], proc.stderr[-3000:])
    assert b"ERROR: AddressSanitizer" not in proc.stderr and b"runtime error" not in proc.stderr, proc.stderr[-3000:]
    done = re.fullmatch(rb"COUNT RULE OK (\d+) cases\n", proc.stdout)
    assert done, proc.stdout[-2000:]
    # 31 k, both strands' rules, four own_from: 13 lengths in three cases of letters, 7 places of a non-base and 3 more texts
    assert int(done.group(1)) >= 31 * 2 * 4 * (13 * 3 + 7 + 3)
