"""CPU checks of the coupled data term (nnrt_fitter_set_data_coupling): the float64 assembly in
tests/_coupled_util.py against the oracle's own data term and against the convergence measured when the mode was
proposed, so the GPU tests compare against something checked; and the switch through the C ABI and the Python layers."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _coupled_util import (block_diagonal_step, coupled_step, coupled_system, data_system, face_pairs, gt_translations_virtual,   # noqa: E402
                           identity_motion, solve_dense)
from _util import rel_err, scene_target   # noqa: E402

LM = 0.001


@pytest.fixture(scope="module")
def s1(oracle_mod):
    from dynamicfuion_python_amd import synthetic as S
    sc = S.make_scene("S1")
    return sc, scene_target(oracle_mod, sc)


@pytest.fixture(scope="module")
def trajectories(oracle_mod, s1):
    """Five coupled and four block-diagonal steps of the restatement on S1 from the identity, computed once."""
    sc, depth = s1
    N = len(sc.nodes)
    gt = gt_translations_virtual(sc)
    R, t = identity_motion(N)
    coupled = []
    for _ in range(5):   # entry k: the cost and the error of the state BEFORE step k + 1
        err = float(np.linalg.norm(t - gt, axis=1).mean())
        R, t, sysm, _ = coupled_step(oracle_mod, sc, depth, R, t, lm=LM)
        coupled.append((sysm["data"]["cost"], err))
    coupled.append((data_system(oracle_mod, sc, depth, R, t)["cost"], float(np.linalg.norm(t - gt, axis=1).mean())))
    R, t = identity_motion(N)
    block = []
    for _ in range(4):
        R, t, d, _ = block_diagonal_step(oracle_mod, sc, depth, R, t, lm=LM)
        block.append(d["cost"])
    block.append(data_system(oracle_mod, sc, depth, R, t)["cost"])
    return coupled, block


def test_assembly_equals_the_oracle_data_term(oracle_mod, s1):
    """The diagonal blocks and the right-hand side of the float64 assembly are oracle.data_hessian_gradient's (its float32
    sums of the same float32 rows) to 1e-6 relative; 5e-8 was measured."""
    sc, depth = s1
    N = len(sc.nodes)
    d = data_system(oracle_mod, sc, depth)
    diag = d["Hfull"][np.arange(N), np.arange(N)]
    e_h, e_g = rel_err(diag, d["hessian_diag"].reshape(N, 6, 6)), rel_err(d["g"], d["gradient"])
    print(f"S1 assembly vs oracle.data_hessian_gradient: H {e_h:.2g}, g {e_g:.2g}")
    assert e_h < 1e-6 and e_g < 1e-6
    # the assembly is symmetric as a whole: block (j, i) is block (i, j) transposed (to the fp64 summation order)
    assert np.abs(d["Hfull"] - np.transpose(d["Hfull"], (1, 0, 3, 2))).max() <= 1e-12 * np.abs(d["Hfull"]).max()


def test_s1_pair_count(oracle_mod, s1):
    sc, depth = s1
    pairs = face_pairs(oracle_mod, sc)
    assert len(pairs) == 140
    assert (pairs[:, 0] < pairs[:, 1]).all()
    sysm = coupled_system(oracle_mod, sc, depth, lm=LM)
    assert np.array_equal(sysm["pairs"], pairs)
    _, cond = solve_dense(sysm["diag"], sysm["pairs"], sysm["blocks"], sysm["rhs"])
    print(f"S1 coupled system from the identity: 140 pairs of 276, fp64 condition number {cond:.3g}")
    assert cond < 1e6   # a float32 Cholesky is adequate (4.2e4 was measured)


def test_restatement_converges_and_block_diagonal_does_not(trajectories):
    coupled, block = trajectories
    print("coupled   (cost, mean |t - gt|) per iteration:", [(f"{c:.4g}", f"{e:.4g}") for c, e in coupled])
    print("block-diagonal cost per iteration:", [f"{c:.4g}" for c in block])
    assert coupled[5][0] < coupled[0][0] / 50
    for k in range(4):
        assert block[k + 1] > block[k], f"block-diagonal cost fell at iteration {k + 1}"


# ---- the switch through the layers ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from dynamicfuion_python_amd import _native
    return _native


NEW_SYMBOLS = ("nnrt_fitter_set_data_coupling", "nnrt_fitter_get_data_coupling", "nnrt_fitter_coupled_pair_count", "nnrt_fitter_get_coupled_system")


def test_symbols_signatures_and_header(native):
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW_SYMBOLS) <= exported
    lib = native.lib()
    c_int32, c_int64, c_void_p = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert list(lib.nnrt_fitter_set_data_coupling.argtypes) == [c_void_p, c_int32]
    assert list(lib.nnrt_fitter_get_data_coupling.argtypes) == [c_void_p, ctypes.POINTER(c_int32)]
    assert lib.nnrt_fitter_coupled_pair_count.restype is c_int64
    assert list(lib.nnrt_fitter_get_coupled_system.argtypes) == [c_void_p] * 5 + [c_int64, c_int64, c_void_p]
    header = open(os.path.join(os.path.dirname(native.LIB_PATH), "..", "include", "nnrt_mi355x.h")).read()
    assert "#define NNRT_DATA_BLOCK_DIAGONAL 0" in header and "#define NNRT_DATA_COUPLED 1" in header
    for name in NEW_SYMBOLS:
        assert name in header
    assert "invalidates the prepared frame" in header


def test_null_fitter_is_refused(native):
    lib = native.lib()
    v = ctypes.c_int32(7)
    assert lib.nnrt_fitter_set_data_coupling(None, 1) == 1   # NNRT_ERROR_ARGUMENT
    assert lib.nnrt_fitter_get_data_coupling(None, ctypes.byref(v)) == 1 and v.value == 7
    assert lib.nnrt_fitter_coupled_pair_count(None) == -1
    buf = np.zeros(36, np.float32)
    assert lib.nnrt_fitter_get_coupled_system(None, native.ptr(buf), native.ptr(buf), native.ptr(buf), native.ptr(buf), 1, 1, None) == 1


class _FakeFitter:
    """Stands in for the native fitter: records what the Python layers hand down, and refuses what the C ABI refuses."""
    made = []

    def __init__(self, *a, **kw):
        self.kw, self.coupling, self.modes = kw, None, list(kw.get("iteration_mode_sequence", ()))
        _FakeFitter.made.append(self)

    def set_data_coupling(self, v):
        self.coupling = v


def test_parameters_reach_the_fitter(monkeypatch):
    from dynamicfuion_python_amd.alignment.render_based import rendering_alignment_optimizer as rao
    from dynamicfuion_python_amd.fusion import pipeline as P
    from dynamicfuion_python_amd.nnrt import alignment as A
    assert issubclass(A.DataCoupling, int) and (A.DataCoupling.BLOCK_DIAGONAL, A.DataCoupling.COUPLED) == (0, 1)
    assert rao.RenderingAlignmentParameters().data_coupling is A.DataCoupling.BLOCK_DIAGONAL
    assert P.FusionParameters().coupled_data_term is False
    monkeypatch.setattr(A, "DeformableMeshToImageFitter", _FakeFitter)
    K = np.array([[100.0, 0, 32], [0, 100.0, 24], [0, 0, 1]])
    _FakeFitter.made.clear()
    rao.RenderingAlignmentOptimizer((48, 64), 0, K, rao.RenderingAlignmentParameters(data_coupling=A.DataCoupling.COUPLED))
    rao.RenderingAlignmentOptimizer((48, 64), 0, K, P.alignment_parameters(P.FusionParameters(coupled_data_term=True)))
    rao.RenderingAlignmentOptimizer((48, 64), 0, K, P.alignment_parameters(P.FusionParameters()))
    assert [f.coupling for f in _FakeFitter.made] == [A.DataCoupling.COUPLED, A.DataCoupling.COUPLED, A.DataCoupling.BLOCK_DIAGONAL]
    with pytest.raises(ValueError):   # a bad enum value never reaches the C ABI
        rao.RenderingAlignmentOptimizer((48, 64), 0, K, rao.RenderingAlignmentParameters(data_coupling=2))


def test_python_methods_exist():
    from dynamicfuion_python_amd.nnrt import alignment as A
    F = A.DeformableMeshToImageFitter
    assert callable(F.set_data_coupling) and callable(F.coupled_system)
    assert isinstance(F.data_coupling, property) and isinstance(F.coupled_pair_count, property)
