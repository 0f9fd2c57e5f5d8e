"""The coupled data term's per-frame host bookkeeping (csrc/coupled_host.hpp: keys -> pairs, CSR by row, the ARAP edges on
each pair, the pair incidences by node) checked without a GPU: tests/native/pair_tables_check.cpp compiles the product
header alone, with the host address and undefined-behaviour sanitizers, and runs as a stand-alone program. The same
program checks incidence_csr, the one statement of the incidences-by-node CSR that the arrowhead solve's structure uses for
the ARAP edges too, on degenerate sizes and on the two-layer hierarchy of the 8 x 8 node grid (the CPU oracle's edges,
which the GPU suite holds bit-identical to the library's)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamicfuion_python_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "pair_tables_check.cpp")
BUILD = os.path.join(ROOT, "tests", "native", "build")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def checker():
    if HIPCC is None:
        pytest.skip("hipcc not available")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "pair_tables_check")
    deps = [SRC, os.path.join(CSRC, "coupled_host.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        tmp = f"{exe}.{os.getpid()}.tmp"   # concurrent workers (pytest -n) each build their own copy, then swap it in
        subprocess.check_call([HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
                               "-fno-sanitize-recover=all",   # the sanitizers on the host code only
                               "-I", CSRC, "-x", "c++", SRC, "-o", tmp])
        os.replace(tmp, exe)
    return exe


def test_pair_tables(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout


def test_incidence_csr_on_the_grid_hierarchy(checker, oracle_mod, tmp_path):
    from dynamicfuion_python_amd import synthetic as S
    nodes, _ = S.node_grid(8, 8)
    _, counts, edges, _ = oracle_mod.build_hierarchy(nodes, 0.18, 2)
    assert len(counts) == 2 and counts.sum() == 64 and len(edges) > 0 and edges.min() >= 0 and edges.max() < 64
    f = tmp_path / "edges.bin"
    with open(f, "wb") as fh:
        np.array([len(edges), 64], np.int32).tofile(fh)
        np.ascontiguousarray(edges, np.int32).tofile(fh)
    r = subprocess.run([checker, str(f)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(edges)} edges over 64 nodes ok" in r.stdout
