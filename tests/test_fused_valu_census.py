"""tools/fused_valu_census.py (compile-only): the fused pixel launch keeps the registers its 5 waves per SIMD need, and the
report names every region and class."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_census_budgets_and_report():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.fail("hipcc is needed (the library build needs it too)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fused_valu_census.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert "== k_fit_pixels_fused<0,4,5>" in out and "== k_fit_pixels_fused<0,4,4>" in out
    for region in ("prologue", "pass 1", "grouping", "gather", "jacobians", "sums fast path", "sums slot-serial", "total"):
        assert any(l.startswith(region) for l in out.splitlines()), region
    total = [l for l in out.splitlines() if l.startswith("total")][0].split()
    assert int(total[9]) > 1000 and int(total[3]) == 0, "VALU total / packed instructions of <0,4,5>"
