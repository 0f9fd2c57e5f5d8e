"""The Schur-corner plan (csrc/corner.hip plan_corner: nested dissection, tile symbolic factorisation, launch levels,
back-substitution chains) checked on the host, without a GPU: tests/native/corner_plan_check.hip compiles the product
plan code for the host and emulates every factor launch task by task in double precision -- fill completeness,
race freedom within each launch (no task writes what another task of the launch reads or writes), back-substitution
order, and the residual of a random SPD system with the structure (< 1e-9). Structures: 2-D grid hierarchies as the
fitter builds them (stem nodes attached to their 4 nearest corner nodes), with and without corner-corner edges (>= 3
layers), with positions (coordinate bisection, the fitter path) and without (BFS separators, the C-ABI path), random
point clouds, disconnected corners and the degenerate sizes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from _arrowhead_util import PLAN_CASES as CASES
from _arrowhead_util import structure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamicfuion_python_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "corner_plan_check.hip")
BUILD = os.path.join(ROOT, "tests", "native", "build")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def checker():
    if HIPCC is None:
        pytest.skip("hipcc not available")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "corner_plan_check")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("corner.hip", "fitter_kernels.hpp", "arrow_device.hpp", "kernels.hpp", "common.hpp", "device_memory.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        tmp = f"{exe}.{os.getpid()}.tmp"   # concurrent workers (pytest -n) each build their own copy, then swap it in
        subprocess.check_call([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                               "-x", "hip", SRC, "-o", tmp], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        os.replace(tmp, exe)
    return exe


def run(checker, tmp_path, edges, n0, N, pos):
    f = tmp_path / "structure.bin"
    with open(f, "wb") as fh:
        np.array([len(edges), n0, N], np.int32).tofile(fh)
        edges.astype(np.int32).tofile(fh)
        if pos is not None:
            pos.astype(np.float32).tofile(fh)
    r = subprocess.run([checker, str(f)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("with_positions", [True, False], ids=["coordinate_bisection", "bfs_separators"])
@pytest.mark.parametrize("name", list(CASES))
def test_corner_plan_emulated(checker, tmp_path, name, with_positions):
    make_pos, spc, knn, seed = CASES[name]
    pos = make_pos()
    edges, n0, N = structure(pos, spc, knn, seed)
    out = run(checker, tmp_path, edges, n0, N, pos if with_positions else None)
    assert "residual" in out
