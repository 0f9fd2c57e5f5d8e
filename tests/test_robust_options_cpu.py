"""CPU checks of the fitter's robust options: the expected-value helper (tests/_robust_util.py) reproduces oracle.fit when
nothing is re-weighted, and the options exist through the C ABI and the Python constructor."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _robust_util import arap_term, data_term, huber_scale, identity_motion, patch_targets, virtual_nodes   # noqa: E402
from _util import oracle_fit_scene, scene_target   # noqa: E402


@pytest.fixture(scope="module")
def S():
    from dynamicfuion_python_amd import synthetic
    return synthetic


def _scene(S, O, name):
    return S.make_scene(name, hierarchy_builder=lambda n, c, l: O.build_hierarchy(n, c, l))


# ---- 1. helper validation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ALL", "TRANSLATION_ONLY", "ROTATION_ONLY"])
def test_helper_equals_oracle_fit_without_reweighting(S, oracle_mod, mode):
    """s = 1: the helper's assembly of the oracle's stage functions is oracle.fit's one-iteration data term, bit for bit."""
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    _, _, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1, modes=(mode,))
    dg_h = data_term(oracle_mod, sc, depth, mode=mode)
    assert np.array_equal(dg_h["pixel_faces"], dg_o["pixel_faces"])
    assert np.array_equal(dg_h["residual_mask"], dg_o["residual_mask"])
    for key in ("residuals", "hessian_diag", "gradient", "updates"):
        assert np.array_equal(dg_h[key], dg_o[key], equal_nan=True), key
    assert dg_h["status"] == dg_o["status"] == 0


def test_helper_equals_oracle_fit_eight_anchors(S, oracle_mod):
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    _, _, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1, anchor_count=8)
    dg_h = data_term(oracle_mod, sc, depth, anchor_count=8)
    for key in ("pixel_faces", "residual_mask", "residuals", "hessian_diag", "gradient", "updates"):
        assert np.array_equal(dg_h[key], dg_o[key], equal_nan=True), key


def test_helper_arap_equals_oracle_fit_without_reweighting(S, oracle_mod):
    """Square penalty on S1_ARAP from a state off the identity: the helper's data blocks + ARAP blocks + LM, solved by the
    oracle's arrowhead solve, give oracle.fit's gradient and updates bit for bit."""
    sc = _scene(S, oracle_mod, "S1_ARAP")
    depth = scene_target(oracle_mod, sc)
    N = len(sc.nodes)
    R1, t1, _ = oracle_fit_scene(oracle_mod, sc, depth, 1)
    _, _, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1, R0=R1, t0=t1)
    dg_h = data_term(oracle_mod, sc, depth, R1, t1)
    ar = arap_term(oracle_mod, sc, R1, t1)
    assert np.all(ar["s"] == 1.0)
    h = sc.hierarchy
    edges = np.asarray(h["edges"], np.int32)
    ej = oracle_mod.arap_edge_jacobians(edges, h["edge_layers"], h["radii"], None, virtual_nodes(sc), R1, 200.0)
    g = oracle_mod.arap_gradient(edges, ej, ar["residuals"].reshape(-1), dg_h["gradient"])
    assert np.array_equal(dg_h["hessian_diag"], dg_o["hessian_diag"])
    assert np.array_equal(g, dg_o["gradient"])
    diag = ar["diag"].reshape(-1) + dg_h["hessian_diag"]
    diag = diag.reshape(N, 6, 6).copy()
    diag[:, np.arange(6), np.arange(6)] += np.float32(0.001)
    x = oracle_mod.solve_arrowhead(diag, ar["wing"], edges, int(h["layer_counts"][0]), g)
    assert np.array_equal(x, dg_o["updates"])


def test_huber_scale_restatement():
    r = np.array([[3e-3, 4e-3, 0.0], [3e-5, 0.0, 4e-5], [0.0, 0.0, 0.0]], np.float32)
    s, n = huber_scale(r, 1e-3)
    assert s[1] == 1.0 and s[2] == 1.0
    assert s[0] == np.sqrt(np.float32(1e-3) / n[0], dtype=np.float32)
    assert abs(float(s[0]) ** 2 * float(n[0]) - 1e-3) < 1e-9   # weight delta / |r|: the scaled norm^2 is delta |r|


def test_median_cutoffs_split_the_scenes(S, oracle_mod):
    """The cutoffs the GPU tests take from the helper cut about half: at least a quarter on each side."""
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    dg = data_term(oracle_mod, sc, depth)
    m = dg["residual_mask"]
    c = float(np.median(np.abs(dg["r"][m])))
    dg_t = data_term(oracle_mod, sc, depth, tukey_c=c)
    inside = int(dg_t["contributes"].sum())
    assert inside >= m.sum() / 4 and m.sum() - inside >= m.sum() / 4
    assert np.array_equal(dg_t["residual_mask"], m)
    sc = _scene(S, oracle_mod, "S1_ARAP")
    depth = scene_target(oracle_mod, sc)
    R1, t1, _ = oracle_fit_scene(oracle_mod, sc, depth, 1)
    norms = arap_term(oracle_mod, sc, R1, t1)["norms"]
    delta = float(np.median(norms))
    s = arap_term(oracle_mod, sc, R1, t1, huber_delta=delta)["s"]
    assert (s == 1.0).sum() >= len(s) / 4 and (s < 1.0).sum() >= len(s) / 4


def test_outlier_patch_is_cut_by_its_cutoff(S, oracle_mod):
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    A, B, patch = patch_targets(depth)
    dg = data_term(oracle_mod, sc, A)
    m = dg["residual_mask"]
    inl = m & ~patch.reshape(-1)
    c = 1.5 * float(np.abs(dg["r"][inl]).max())
    assert patch.sum() == 144 and (m & patch.reshape(-1)).sum() > 100
    assert np.abs(dg["r"][m & patch.reshape(-1)]).min() > c   # every patch pixel lies beyond the cutoff
    dg_a = data_term(oracle_mod, sc, A, tukey_c=c)
    dg_b = data_term(oracle_mod, sc, B, tukey_c=c)
    assert np.array_equal(dg_a["contributes"], dg_b["contributes"])
    for key in ("hessian_diag", "gradient", "updates"):
        assert np.array_equal(dg_a[key], dg_b[key]), key


# ---- 2. the options through the C ABI ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from dynamicfuion_python_amd import _native
    return _native


def test_robust_option_symbols_and_signatures(native):
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"nnrt_fitter_set_robust_options", "nnrt_fitter_get_robust_options"} <= exported
    lib = native.lib()
    c_int32, c_void_p = ctypes.c_int32, ctypes.c_void_p
    assert lib.nnrt_fitter_set_robust_options.restype is c_int32
    assert list(lib.nnrt_fitter_set_robust_options.argtypes) == [c_void_p, c_int32, c_int32]
    assert lib.nnrt_fitter_get_robust_options.restype is c_int32
    assert list(lib.nnrt_fitter_get_robust_options.argtypes) == [c_void_p, ctypes.POINTER(c_int32), ctypes.POINTER(c_int32)]
    header = open(os.path.join(os.path.dirname(native.LIB_PATH), "..", "include", "nnrt_mi355x.h")).read()
    assert "#define NNRT_PENALTY_REFERENCE 0" in header and "#define NNRT_PENALTY_IRLS 1" in header


def test_robust_options_reject_a_null_fitter(native):
    lib = native.lib()
    a, b = ctypes.c_int32(7), ctypes.c_int32(7)
    assert lib.nnrt_fitter_set_robust_options(None, 0, 0) == 1   # NNRT_ERROR_ARGUMENT, nothing launched
    assert lib.nnrt_fitter_get_robust_options(None, ctypes.byref(a), ctypes.byref(b)) == 1
    assert (a.value, b.value) == (7, 7)


def test_fitter_params_did_not_grow(native):
    assert ctypes.sizeof(native.FitterParams) == 4 * (13 + 16)


def test_python_defaults():
    from dynamicfuion_python_amd.alignment.render_based import rendering_alignment_optimizer as rao
    from dynamicfuion_python_amd.nnrt import alignment as A
    assert issubclass(A.PenaltyForm, int) and (A.PenaltyForm.REFERENCE, A.PenaltyForm.IRLS) == (0, 1)
    sig = inspect.signature(A.DeformableMeshToImageFitter.__init__)
    names = list(sig.parameters)
    assert names[-2:] == ["penalty_form", "guard_zero_rotation"]
    assert sig.parameters["penalty_form"].default is A.PenaltyForm.REFERENCE
    assert sig.parameters["guard_zero_rotation"].default is False
    assert hasattr(A.DeformableMeshToImageFitter, "set_robust_options")
    assert isinstance(A.DeformableMeshToImageFitter.robust_options, property)
    p = rao.RenderingAlignmentParameters()
    assert p.penalty_form is A.PenaltyForm.REFERENCE and p.guard_zero_rotation is False
