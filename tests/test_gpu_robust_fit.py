"""GPU tests of the fitter's robust options (nnrt_fitter_set_robust_options): the IRLS Tukey data term and the IRLS Huber
ARAP term against the expected values tests/_robust_util.py assembles from the CPU oracle's stage functions (validated in
tests/test_robust_options_cpu.py), and the zero-rotation guard. Scenes: S1 (96 x 128, 24 nodes) and S1_ARAP (96 x 128,
48 nodes, 2 layers)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _robust_util import arap_term, data_term, patch_targets   # noqa: E402
from _util import exact_system_solution, oracle_fit_scene, rel_err, scene_target   # noqa: E402
from test_gpu_parity import REFINE_PIVOT_RATIO, _compare_iteration, nan_rel_err   # noqa: E402

pytestmark = pytest.mark.gpu

LM = 0.001


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import _native
    _native.lib()
    from dynamicfuion_python_amd import nnrt
    return nnrt


@pytest.fixture(scope="module")
def scenes(oracle_mod):
    """The two scenes, their target depths and the outlier targets, computed once (the tests only read them)."""
    from dynamicfuion_python_amd import synthetic as S
    out = {}
    for name in ("S1", "S1_ARAP"):
        sc = S.make_scene(name, hierarchy_builder=lambda n, c, l: oracle_mod.build_hierarchy(n, c, l))
        depth = scene_target(oracle_mod, sc)
        A, B, patch = patch_targets(depth)
        out[name] = (sc, depth, A, B, patch)
    return out


def _fitter(nn, sc, iterations=1, modes=None, anchor_count=4, graph=0, **kw):
    G, A = nn.geometry, nn.alignment
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, anchor_count, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                      sc.layer_count)
    ft = A.DeformableMeshToImageFitter(iterations, modes or [A.IterationMode.ALL], preconditioning_dampening_factor=LM, use_hip_graph=graph, **kw)
    return wf, ft


def _mesh(nn, sc):
    return nn.geometry.TriangleMesh(sc.points, sc.normals, sc.faces)


def _fit(nn, sc, depth, iterations=1, **kw):
    wf, ft = _fitter(nn, sc, iterations, **kw)
    ft.fit_to_image(wf, _mesh(nn, sc), None, depth, None, sc.K, None, 1.0)
    return wf, ft, ft.diagnostics()


def _motion(wf):
    return wf.get_node_rotations(True), wf.get_node_translations(True)


def _inlier_cutoff(oracle_mod, sc, target, patch):
    dg = data_term(oracle_mod, sc, target)
    inl = dg["residual_mask"] & ~patch.reshape(-1)
    return 1.5 * float(np.abs(dg["r"][inl]).max())


# ---- 3. Tukey IRLS parity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,anchor_count", [("ALL", 4), ("TRANSLATION_ONLY", 4), ("ROTATION_ONLY", 4), ("ALL", 8)])
def test_tukey_irls_parity(nn, oracle_mod, scenes, mode, anchor_count):
    """One iteration on S1 from the identity; anchor_count 8 runs the MAX_ANCHORS build of the fused launch. The cutoff is
    the median |r| of the square-penalty run, so about half the masked pixels are cut."""
    A = nn.alignment
    sc, depth = scenes["S1"][:2]
    N = len(sc.nodes)
    sq = data_term(oracle_mod, sc, depth, mode=mode, anchor_count=anchor_count)
    m = sq["residual_mask"]
    c = float(np.median(np.abs(sq["r"][m])))
    dg_h = data_term(oracle_mod, sc, depth, mode=mode, anchor_count=anchor_count, tukey_c=c, lm=LM)
    inside = int(dg_h["contributes"].sum())
    assert inside >= m.sum() / 4 and m.sum() - inside >= m.sum() / 4
    wf, ft, dg_g = _fit(nn, sc, depth, modes=[A.IterationMode[mode]], anchor_count=anchor_count, use_tukey_penalty_for_data_term=True,
                        tukey_penalty_cutoff_cm=c, penalty_form=A.PenaltyForm.IRLS)
    assert ft.robust_options == (A.PenaltyForm.IRLS, False)
    s = 6 if mode == "ALL" else 3
    print(f"{mode} K={anchor_count}: c {c:.4g}, {inside} of {int(m.sum())} contribute; residuals "
          f"{np.abs(dg_h['residuals'] - dg_g['residuals']).max():.2g} abs, H {nan_rel_err(dg_g['hessian'][: N * s * s], dg_h['hessian_diag']):.2g}, "
          f"g {nan_rel_err(dg_g['gradient'][: N * s], dg_h['gradient']):.2g}, updates {nan_rel_err(dg_g['updates'][: N * s], dg_h['updates']):.2g}")
    _compare_iteration(dg_h, dg_g, s, N)


# ---- 4. outliers carry no weight ------------------------------------------------------------------------------------
def _two_iterations(nn, sc, target, **kw):
    wf, ft = _fitter(nn, sc, 2, **kw)
    ft.prepare(wf, _mesh(nn, sc), target, None, sc.K, None, 1.0)
    per = []
    for k in range(2):
        ft.iterate(wf, k, 1)
        dg = ft.diagnostics()
        per.append((dg["hessian"].copy(), dg["gradient"].copy(), dg["updates"].copy()))
    ft.check()
    return per, _motion(wf)


def test_outliers_carry_no_weight(nn, oracle_mod, scenes):
    """Target A: a 12 x 12 patch pushed 0.5 m back; target B: the same patch without depth. Under IRLS with a cutoff of
    1.5 x the largest inlier |r| both give the same two iterations bit for bit; under the square penalty they do
    not. (The reference form also drops a pixel beyond the cutoff from H and g, so it cannot serve as the contrast.)"""
    A = nn.alignment
    sc, _, tA, tB, patch = scenes["S1"]
    c = _inlier_cutoff(oracle_mod, sc, tA, patch)
    irls = dict(use_tukey_penalty_for_data_term=True, tukey_penalty_cutoff_cm=c, penalty_form=A.PenaltyForm.IRLS)
    per_a, mot_a = _two_iterations(nn, sc, tA, **irls)
    per_b, mot_b = _two_iterations(nn, sc, tB, **irls)
    for k in range(2):
        for a, b, what in zip(per_a[k], per_b[k], ("H", "g", "updates")):
            assert np.array_equal(a, b), f"iteration {k + 1}: {what} differs between the two targets"
        assert np.abs(per_a[k][2]).max() > 0
    assert np.array_equal(mot_a[0], mot_b[0]) and np.array_equal(mot_a[1], mot_b[1])
    assert np.isfinite(mot_a[0]).all() and np.isfinite(mot_a[1]).all()
    # the same pair under the square penalty is not identical: the patch pulls at full weight there
    per_a, mot_a = _two_iterations(nn, sc, tA)
    per_b, mot_b = _two_iterations(nn, sc, tB)
    assert not np.array_equal(per_a[0][1], per_b[0][1], equal_nan=True)
    assert not np.array_equal(mot_a[1], mot_b[1], equal_nan=True)


# ---- 5. Huber IRLS parity -------------------------------------------------------------------------------------------
def test_huber_irls_parity(nn, oracle_mod, scenes):
    A = nn.alignment
    sc, depth = scenes["S1_ARAP"][:2]
    N = len(sc.nodes)
    wf, ft0 = _fitter(nn, sc, 1)
    mesh = _mesh(nn, sc)
    ft0.fit_to_image(wf, mesh, None, depth, None, sc.K, None, 1.0)   # one SQUARE iteration leaves the identity
    R1, t1 = _motion(wf)
    assert np.isfinite(R1).all() and np.abs(t1).max() > 0
    norms = arap_term(oracle_mod, sc, R1, t1)["norms"]
    delta = float(np.median(norms))
    ar = arap_term(oracle_mod, sc, R1, t1, huber_delta=delta)
    E = len(ar["s"])
    assert (ar["s"] == 1.0).sum() >= E / 4 and (ar["s"] < 1.0).sum() >= E / 4
    ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=LM, use_hip_graph=0,
                                       use_huber_penalty_for_arap_term=True, huber_penalty_constant=delta)
    ft.set_robust_options(A.PenaltyForm.IRLS, False)
    ft.prepare(wf, mesh, depth, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, 1)
    ft.check()
    dg_g = ft.diagnostics()
    diag, wing, rhs = ft.arrowhead_system(N, E)
    dg_h = data_term(oracle_mod, sc, depth, R1, t1)
    hd = dg_g["hessian"][: N * 36].reshape(N, 6, 6)
    want_diag = (ar["diag"] + hd).astype(np.float32)
    want_diag[:, np.arange(6), np.arange(6)] += np.float32(LM)
    want_rhs = (dg_h["gradient"] + ar["gradient"]).astype(np.float32)
    errs = rel_err(diag, want_diag), rel_err(wing, ar["wing"]), rel_err(rhs, want_rhs)
    x64, ratio = exact_system_solution(ft, wf, N)
    u_err = nan_rel_err(dg_g["updates"][: 6 * N], x64)
    print(f"S1_ARAP Huber IRLS: delta {delta:.4g}, {int((ar['s'] < 1).sum())} of {E} edges scaled; diag {errs[0]:.2g}, wing {errs[1]:.2g}, "
          f"rhs {errs[2]:.2g}; updates {u_err:.2g} from the fp64 solution (fp64 pivot ratio {ratio:.2g})")
    assert max(errs) < 1e-6, errs
    # ... and the scaling did change the system: the square-penalty blocks are further away than that
    sq = arap_term(oracle_mod, sc, R1, t1)
    assert rel_err(wing, sq["wing"]) > 1e-3
    if ratio > REFINE_PIVOT_RATIO:
        assert u_err <= 1e-4


# ---- 6. the zero-rotation guard -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S1", "S1_ARAP"])
def test_guard_on_an_empty_frame(nn, scenes, name):
    sc = scenes[name][0]
    N = len(sc.nodes)
    empty = np.zeros((sc.H, sc.W), np.float32)
    wf, ft, dg = _fit(nn, sc, empty)
    assert np.isnan(wf.get_node_rotations(True)).all()   # Rodrigues' 0 / 0, as in the reference (A7)
    wf, ft, dg = _fit(nn, sc, empty, guard_zero_rotation=True)   # fit_to_image checks the device error flag
    assert ft.robust_options[1] is True
    R, t = _motion(wf)
    assert np.array_equal(R, np.tile(np.eye(3, dtype=np.float32), (N, 1, 1)))
    assert np.array_equal(t, np.zeros((N, 3), np.float32))
    assert np.array_equal(dg["updates"][: 6 * N], np.zeros(6 * N, np.float32))


def test_guard_touches_only_zero_update_nodes(nn, oracle_mod, scenes):
    """S1 with depth only in the strip u < W / 4: the nodes no strip pixel reaches have a zero update."""
    sc, depth = scenes["S1"][:2]
    N = len(sc.nodes)
    strip = depth.copy()
    strip[:, sc.W // 4:] = 0
    _, _, dg_o = oracle_fit_scene(oracle_mod, sc, strip, 1, raise_on_failure=False)
    zero = (dg_o["updates"].reshape(N, 6) == 0).all(axis=1)
    assert zero.any() and (~zero).any()
    wf0, _, dg0 = _fit(nn, sc, strip)
    wf1, _, dg1 = _fit(nn, sc, strip, guard_zero_rotation=True)
    R0, t0 = _motion(wf0)
    R1, t1 = _motion(wf1)
    assert np.array_equal((dg1["updates"][: 6 * N].reshape(N, 6) == 0).all(axis=1), zero)
    assert np.isnan(R0[zero]).all() and np.isfinite(R0[~zero]).all()
    assert np.isfinite(R1).all() and np.isfinite(t1).all() and np.isfinite(dg1["updates"][: 6 * N]).all()
    assert np.array_equal(R1[zero], np.tile(np.eye(3, dtype=np.float32), (int(zero.sum()), 1, 1)))
    assert np.array_equal(R1[~zero], R0[~zero]) and np.array_equal(t1, t0)
    assert np.array_equal(dg1["updates"], dg0["updates"])


# ---- 7. graphs ------------------------------------------------------------------------------------------------------
def test_setter_drops_graphs_and_matches_a_fresh_fitter(nn, oracle_mod, scenes):
    from dynamicfuion_python_amd._native import NnrtError
    A = nn.alignment
    sc, _, tA, _, patch = scenes["S1"]
    c = _inlier_cutoff(oracle_mod, sc, tA, patch)
    kw = dict(use_tukey_penalty_for_data_term=True, tukey_penalty_cutoff_cm=c, graph=2)
    mesh = _mesh(nn, sc)
    wf, ft = _fitter(nn, sc, 2, **kw)
    ft.prepare(wf, mesh, tA, None, sc.K, None, 1.0)
    wf.reset_motion()
    ft.iterate(wf, 0, 2)      # REFERENCE form: captured on first use ...
    wf.reset_motion()
    ft.iterate(wf, 0, 2)      # ... and replayed
    assert ft.graph_count == 1
    ref_motion = _motion(wf)
    ft.set_robust_options(A.PenaltyForm.IRLS, 1)
    assert ft.graph_count == 0
    assert ft.robust_options == (A.PenaltyForm.IRLS, True)
    wf.reset_motion()
    ft.iterate(wf, 0, 2)      # the prepared frame is kept
    ft.check()
    wf2, ft2 = _fitter(nn, sc, 2, penalty_form=A.PenaltyForm.IRLS, guard_zero_rotation=True, **kw)
    ft2.prepare(wf2, mesh, tA, None, sc.K, None, 1.0)
    ft2.iterate(wf2, 0, 2)
    for a, b in zip(_motion(wf), _motion(wf2)):
        assert np.isfinite(a).all() and np.array_equal(a, b)
    d1, d2 = ft.diagnostics(), ft2.diagnostics()
    for key in ("residuals", "hessian", "gradient", "updates"):
        assert np.array_equal(d1[key], d2[key]), key
    assert not np.array_equal(_motion(wf)[1], ref_motion[1], equal_nan=True)   # the options changed the fit
    for bad, word in (((2, 0), "penalty_form"), ((-1, 0), "penalty_form"), ((0, 2), "guard_zero_rotation"), ((1, -1), "guard_zero_rotation")):
        with pytest.raises(NnrtError, match=word):
            ft.set_robust_options(*bad)
    assert ft.robust_options == (A.PenaltyForm.IRLS, True)


# ---- 8. optimizer ---------------------------------------------------------------------------------------------------
def test_optimizer_passes_the_options_through(nn, oracle_mod, scenes):
    from dynamicfuion_python_amd.alignment.render_based.rendering_alignment_optimizer import (PenaltyFunction, RenderingAlignmentOptimizer,
                                                                                             RenderingAlignmentParameters)
    A, G = nn.alignment, nn.geometry
    sc, _, tA, _, patch = scenes["S1_ARAP"]
    c = _inlier_cutoff(oracle_mod, sc, tA, patch)
    pts, valid = oracle_mod.unproject(tA, sc.K, 1.0, 10.0)
    pts = np.where(valid[:, None], pts, 0).astype(np.float32)
    prm = RenderingAlignmentParameters(data_term_penalty_function=PenaltyFunction.TUKEY, data_term_penalty_constant=c,
                                       regularization_term_penalty_function=PenaltyFunction.HUBER, max_iteration_count=sc.iterations,
                                       penalty_form=A.PenaltyForm.IRLS, guard_zero_rotation=True)
    mesh = _mesh(nn, sc)

    def graph():
        return G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, sc.layer_count)

    opt = RenderingAlignmentOptimizer((sc.H, sc.W), None, sc.K, prm)
    assert opt.fitter.robust_options == (A.PenaltyForm.IRLS, True)
    wf = opt.optimize_graph(graph(), mesh, pts.reshape(sc.H, sc.W, 3))
    R, t = _motion(wf)
    assert np.isfinite(R).all() and np.isfinite(t).all() and np.abs(t).max() > 0
    ft = A.DeformableMeshToImageFitter(prm.max_iteration_count, list(prm.iteration_mode_sequence), use_tukey_penalty_for_data_term=True,
                                       tukey_penalty_cutoff_cm=c, preconditioning_dampening_factor=prm.preconditioning_dampening_factor,
                                       arap_term_weight=prm.arap_term_weight, use_huber_penalty_for_arap_term=True,
                                       huber_penalty_constant=prm.regularization_term_penalty_constant, penalty_form=A.PenaltyForm.IRLS,
                                       guard_zero_rotation=True)
    wf2 = graph()
    ft.fit_to_image(wf2, mesh, None, pts, valid.astype(np.uint8), sc.K, None, (sc.H, sc.W))
    R2, t2 = _motion(wf2)
    assert np.array_equal(R, R2) and np.array_equal(t, t2)
