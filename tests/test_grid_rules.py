"""Two rules that csrc/ states once, checked on the host without a GPU: the anchor-count dispatch (anchor_dispatch.hpp:
one call of f per K in 1..8, a refusal outside) and the voxel grid's hash-table sizing (hash_table_size.hpp, which
HashTable::size_for is). tests/native/grid_rules_check.cpp compiles the two product headers alone, with the host address
and undefined-behaviour sanitizers, and runs as a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamicfuion_python_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "grid_rules_check.cpp")
BUILD = os.path.join(ROOT, "tests", "native", "build")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def checker():
    if HIPCC is None:
        pytest.skip("hipcc not available")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "grid_rules_check")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("anchor_dispatch.hpp", "hash_table_size.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        tmp = f"{exe}.{os.getpid()}.tmp"   # concurrent workers (pytest -n) each build their own copy, then swap it in
        subprocess.check_call([HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
                               "-fno-sanitize-recover=all",   # the sanitizers on the host code only
                               "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-x", "c++", SRC, "-o", tmp])
        os.replace(tmp, exe)
    return exe


def test_anchor_dispatch_and_table_sizing(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "grid_rules_check OK" in r.stdout
