"""The fitter's per-frame launch choices (csrc/launch_plan.hpp choose_launches: order tables, pixel-launch build, anchor
format, warp and raster kernels) checked on the host, without a GPU: tests/native/launch_plan_check.cpp compiles the
product header alone and walks a table of cases whose expected choices are written out by hand from the rules."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamicfuion_python_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "launch_plan_check.cpp")
BUILD = os.path.join(ROOT, "tests", "native", "build")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def checker():
    if HIPCC is None:
        pytest.skip("hipcc not available")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "launch_plan_check")
    deps = [SRC, os.path.join(CSRC, "launch_plan.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        tmp = f"{exe}.{os.getpid()}.tmp"   # concurrent workers (pytest -n) each build their own copy, then swap it in
        subprocess.check_call([HIPCC, "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-x", "c++", SRC, "-o", tmp])
        os.replace(tmp, exe)
    return exe


def test_launch_choices_table(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout
