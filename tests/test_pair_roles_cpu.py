"""The block -> role map of the paired launch (km_amd/csrc/pair_roles.h, used by k_dfs_pure_seed) driven on the CPU under
AddressSanitizer + UBSan: a bijection onto the walk, pure-chain and seed index ranges for every small grid and for large
ones up to 2^31 - 1 and 2^32 - 1 blocks, in both orders of the seed and the pure-chain blocks (tests/host/pair_roles.cpp)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_role_map_program_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "pair_roles")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "host", "pair_roles.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe], capture_output=True, env=env, timeout=300)
    assert proc.returncode == 0 and proc.stdout.startswith(b"PAIR ROLES OK 3000 small grids, 32 large"), \
        (proc.stdout[-2000:], proc.stderr[-3000:])
    assert b"ERROR: AddressSanitizer" not in proc.stderr and b"runtime error" not in proc.stderr, proc.stderr[-3000:]


def test_the_kernel_uses_the_shared_map():
    """The kernel picks its role through pair_block and nothing else: no second copy of the arithmetic to drift."""
    src = open(os.path.join(HERE, "..", "km_amd", "csrc", "graph_kernel.h")).read()
    body = src[src.index("void k_dfs_pure_seed("):src.index("// Direct mode (large tier")]
    assert '#include "pair_roles.h"' in src and body.count("pair_block(blockIdx.x,") == 1
    assert body.count("blockIdx") == 1 and "gridDim" not in body
