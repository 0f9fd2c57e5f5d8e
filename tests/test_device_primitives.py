"""The device scan, sort and select calls (csrc/device_primitives.hpp) checked by a stand-alone program,
tests/native/device_primitives_check.hip, built and run like the device memory checker and linked with
csrc/device_primitives.hip directly. Without a device: n == 0 returns NNRT_OK and leaves the scratch alone, n = 2^31 is
refused with an error text. With a device: every function against the host's std::exclusive_scan, std::stable_sort,
std::copy_if and std::unique at n = 1, 63, 64, 65, 1023, 1024, 1025 and 100003, and the reserve rule of the scratch
(large -> small -> larger: the pointer stays on the second call; the bytes in use return to their start)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamicfuion_python_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "device_primitives_check.hip")
LIB_SRC = os.path.join(CSRC, "device_primitives.hip")
BUILD = os.path.join(ROOT, "tests", "native", "build")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def checker():
    if HIPCC is None:
        pytest.skip("hipcc not available")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "device_primitives_check")
    deps = [SRC, LIB_SRC] + [os.path.join(CSRC, f) for f in ("device_primitives.hpp", "device_memory.hpp", "common.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        tmp = f"{exe}.{os.getpid()}.tmp"   # concurrent workers (pytest -n) each build their own copy, then swap it in
        subprocess.check_call([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                               "-x", "hip", SRC, LIB_SRC, "-o", tmp], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        os.replace(tmp, exe)
    return exe


def _run(checker, mode):
    r = subprocess.run([checker, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"device_primitives_check OK ({mode})" in r.stdout


def test_device_primitives_refuse_and_skip_without_a_device(checker):
    _run(checker, "host")


@pytest.mark.gpu
def test_device_primitives_match_the_host(checker):
    _run(checker, "device")
