"""DeviceBuffer (csrc/device_memory.hpp) checked by a stand-alone host program, tests/native/device_memory_check.hip,
built and run like the corner plan checker: move construction and assignment leave the source empty, release() is
idempotent, and on a machine without a device ensure() fails with NNRT_ERROR_HIP, an error text, a null pointer and a
zero count. On a machine with a device the same program checks that ensure() succeeds, keeps its pointer while the
request fits, and that the bytes-in-use counter follows every allocation and release back to its start."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamicfuion_python_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "device_memory_check.hip")
BUILD = os.path.join(ROOT, "tests", "native", "build")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def checker():
    if HIPCC is None:
        pytest.skip("hipcc not available")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "device_memory_check")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("device_memory.hpp", "common.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        tmp = f"{exe}.{os.getpid()}.tmp"   # concurrent workers (pytest -n) each build their own copy, then swap it in
        subprocess.check_call([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                               "-x", "hip", SRC, "-o", tmp], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        os.replace(tmp, exe)
    return exe


def test_device_buffer_host_contract(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device_memory_check OK" in r.stdout
