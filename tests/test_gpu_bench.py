"""A plain bench.py run on the GPU: --steps N times exactly N steps, the result line carries the headline fields only,
and --dump-outputs writes the last timed step's outputs, the same from run to run (small S1 scene, in-process)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bench  # noqa: E402

OUTPUTS = ("node_rotations", "node_translations", "updates", "gradient", "hessian", "residuals", "residual_mask", "pixel_faces")
FULL_ONLY = ("ms_per_solve", "setup_ms", "kernel_ms", "stage_ms", "roofline", "kernels", "cpu_baseline")


def _run(capsys, *argv):
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    capsys.readouterr()
    bench.main(list(argv))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_the_requested_steps_and_dumps_its_outputs(capsys, tmp_path):
    # 13 steps at 10 per graph launch: one whole launch and a shorter one of 3
    args = ("--gpus", "1", "--config", "S1", "--steps", "13", "--warmup", "3")
    a = _run(capsys, *args, "--dump-outputs", str(tmp_path / "a"))
    b = _run(capsys, *args, "--dump-outputs", str(tmp_path / "b"))
    for out in (a, b):
        assert out["steps"] == 13 and out["warmup"] == 3 and out["full"] is False
        assert out["unit"] == "GN iters/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
        assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(1000.0 / out["ms_per_step"])
        assert not set(FULL_ONLY) & set(out)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in OUTPUTS)
    got = {n: (np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")) for n in OUTPUTS}
    assert sum(x.nbytes for x, _ in got.values()) <= bench.DUMP_BYTES
    for n, (x, y) in got.items():
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and np.isfinite(x).all(), n
    # the same inputs in both runs: the raster and the residuals are the same bit for bit (no atomics on their way); the
    # JtJ / Jt r sums are double sums of float products in an order that varies, so the Hessian and gradient agree to
    # float rounding (1e-6, the parity tests' bound for them) and the solved update and node motion to 1e-4 (theirs)
    for n in ("pixel_faces", "residual_mask", "residuals"):
        assert np.array_equal(*got[n]), n
    for n, tol in (("gradient", 1e-6), ("hessian", 1e-6), ("updates", 1e-4), ("node_rotations", 1e-4), ("node_translations", 1e-4)):
        x, y = got[n]
        assert np.abs(x - y).max() <= tol * np.abs(x).max(), n
    assert np.abs(got["updates"][0]).max() > 0 and got["residual_mask"][0].sum() > 0
    assert got["node_rotations"][0].shape[1:] == (3, 3) and got["node_translations"][0].shape[1:] == (3,)
