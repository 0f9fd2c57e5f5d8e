"""GPU parity tests: every HIP stage and the fused GN iteration against the CPU oracle on the same seeded inputs.

Tolerances: integer/index outputs (anchors, rasterized faces, masks) must be identical; the raster and warp stages are
bit-identical by construction (same float expression order, -ffp-contract=off, transcendentals rounded once from
double on both sides). The data-term JtJ / Jt r sums are exact on both sides (float products summed in double: GPU
wave/atomic order vs the oracle's serial order differ only in double rounding), so Hessian and gradient blocks are
compared at <= 1e-6 relative and the solved updates / node motion at <= 1e-4 relative (north_star tolerance).
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from _util import (FIXTURES, arrowhead_fp64_solution, arrowhead_fp64_system, exact_system_solution, fp64_pivot_ratio, oracle_fit_scene, read_ply,  # noqa: E402
                   rel_err, scene_target, transform_mesh, xy_plane)
from golden import kat_literals as L  # noqa: E402


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import _native
    _native.lib()
    from dynamicfuion_python_amd import nnrt
    return nnrt


@pytest.fixture(scope="module")
def S():
    from dynamicfuion_python_amd import synthetic
    return synthetic


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _scene(S, O, name, seed=0):
    return S.make_scene(name, seed=seed, hierarchy_builder=lambda n, c, l: O.build_hierarchy(n, c, l))


# ---------------------------------------------------------------------------------------------------------------------
# stages
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("S1", 4), ("C1", 4), ("C2", 4), ("C1", 1), ("C1", 3), ("C1", 8)])
def test_anchors_bit_exact(nn, S, oracle_mod, name, k):
    sc = _scene(S, oracle_mod, name)
    a_o, w_o = oracle_mod.compute_anchors(sc.points, sc.nodes, k, sc.coverage)
    a_g, w_g = nn.geometry.functional.compute_anchors_and_weights_euclidean_fixed_node_weight(sc.points, sc.nodes, k, 0, sc.coverage)
    assert np.array_equal(a_o, _np(a_g))
    assert np.array_equal(w_o, _np(w_g))


def test_anchors_variable_coverage_and_threshold(nn, S, oracle_mod):
    sc = _scene(S, oracle_mod, "S1")
    cw = oracle_mod.node_coverage_weights(sc.nodes, sc.coverage)
    a_o, w_o = oracle_mod.compute_anchors(sc.points, sc.nodes, 4, 0.0, node_weights=cw)
    a_g, w_g = nn.geometry.functional.compute_anchors_and_weights_euclidean_variable_node_weight(sc.points, sc.nodes, cw, 4, 0)
    assert np.array_equal(a_o, _np(a_g)) and np.array_equal(w_o, _np(w_g))
    a_o, w_o = oracle_mod.compute_anchors(sc.points, sc.nodes, 4, 0.1, minimum_valid_anchor_count=2)
    a_g, w_g = nn.geometry.functional.compute_anchors_and_weights_euclidean_fixed_node_weight(sc.points, sc.nodes, 4, 2, 0.1)
    assert np.array_equal(a_o, _np(a_g)) and np.array_equal(w_o, _np(w_g))


@pytest.mark.parametrize("extrinsic", [False, True])
def test_warp_bit_exact(nn, S, oracle_mod, extrinsic):
    sc = _scene(S, oracle_mod, "C1")
    a, w = oracle_mod.compute_anchors(sc.points, sc.nodes, 4, sc.coverage)
    E = None
    if extrinsic:
        E = np.eye(4)
        E[:3, :3] = S.rodrigues_np(np.array([[0.01, -0.02, 0.03]], np.float32))[0]
        E[:3, 3] = [0.01, -0.005, 0.02]
    wp_o, wn_o = oracle_mod.warp_mesh(sc.points, sc.normals, sc.nodes, sc.gt_rotations, sc.gt_translations, a, w, E)
    m = nn.geometry.functional.warp_triangle_mesh(nn.geometry.TriangleMesh(sc.points, sc.normals, sc.faces), sc.nodes, sc.gt_rotations,
                                                  sc.gt_translations, a, w, extrinsics=np.eye(4) if E is None else E)
    assert np.array_equal(wp_o, _np(m.vertex_positions))
    assert np.array_equal(wn_o, _np(m.vertex_normals))


@pytest.mark.parametrize("name,from_identity,vertex_path", [("C1", False, "0"), ("C1", True, "0"), ("C2", False, "0"), ("C1", False, "1"),
                                                             ("C1", True, "1"), ("C2", False, "1"), ("C2", False, "1-int32"),
                                                             ("C1", True, "1-int32")])
def test_fitter_warp_bit_exact(nn, S, oracle_mod, name, from_identity, vertex_path, monkeypatch):
    """The fitter's own warp -- the mesh an iteration rasterizes -- equals the oracle's warp of the motion the iteration
    started from, bit for bit: from the ground-truth motion (general kernel) and from the identity (iterate_from_identity's
    IDENTITY kernel); with the lane-per-(vertex, slot) quad kernel (NNRT_WARP_VERTEX=0) and the lane-per-vertex kernel
    meshes of 64 k vertices and more take (=1), the latter reading the per-frame 16-bit anchor copy or, with
    NNRT_ANCHORS16=0 ("1-int32"), the int32 anchors."""
    monkeypatch.setenv("NNRT_WARP_VERTEX", vertex_path[0])
    monkeypatch.setenv("NNRT_ANCHORS16", "0" if vertex_path.endswith("int32") else "1")
    sc = _scene(S, oracle_mod, name)
    depth = scene_target(oracle_mod, sc)
    wf, ft = _new_fit(nn, sc, depth, 1)
    plan = ft.launch_plan()   # the forced paths are the ones the frame runs (4 anchors, fewer than 65535 nodes)
    assert plan["warp_vertex"] == int(vertex_path[0]) and plan["anchors16"] == (0 if vertex_path.endswith("int32") else 1)
    V, Nn = len(sc.points), len(sc.nodes)
    if from_identity:
        ft.iterate_from_identity(wf, 0, 1)
        R0, t0 = np.tile(np.eye(3, dtype=np.float32), (Nn, 1, 1)), np.zeros((Nn, 3), np.float32)
    else:
        wf.set_node_rotations(sc.gt_rotations)   # original node order
        wf.set_node_translations(sc.gt_translations)
        R0, t0 = wf.get_node_rotations(True), wf.get_node_translations(True)
        ft.iterate(wf, 0, 1)
    p_g, n_g = ft.warped_mesh(V)
    a, w = ft.anchors(V, 4)
    p_o, n_o = oracle_mod.warp_mesh(sc.points, sc.normals, wf.get_node_positions(True), R0, t0, a, w)
    assert np.array_equal(p_g, p_o) and np.array_equal(n_g, n_o)


def test_ndc_extraction_bit_exact_and_fixture(nn, S, oracle_mod):
    V, N, F = xy_plane(1.2615, (0, 0, 1), 4)
    K = np.array([[580., 0., 320.], [0., 580., 240.], [0., 0., 1.]])
    ndc_g, m_g = nn.rendering.functional.get_mesh_ndc_face_vertices_and_clip_mask(nn.geometry.TriangleMesh(V, N, F), K, (480, 640), 0.0, 2.0)
    gt = np.load(os.path.join(FIXTURES, "extracted_face_vertices.npy"))
    gm = np.load(os.path.join(FIXTURES, "extracted_face_mask.npy"))
    assert np.array_equal(_np(m_g), gm)
    assert np.allclose(_np(ndc_g)[gm], gt[gm], atol=1e-5)
    sc = _scene(S, oracle_mod, "C1")
    ndc_o, m_o = oracle_mod.extract_face_ndc(sc.points, sc.faces, sc.K, sc.H, sc.W, 0.0, 10.0)
    ndc_g, m_g = nn.rendering.functional.get_mesh_ndc_face_vertices_and_clip_mask(nn.geometry.TriangleMesh(sc.points, sc.normals, sc.faces),
                                                                                   sc.K, (sc.H, sc.W), 0.0, 10.0)
    assert np.array_equal(m_o, _np(m_g)) and np.array_equal(ndc_o, _np(ndc_g))


def _warped_face_ndc(oracle_mod, sc):
    a, w = oracle_mod.compute_anchors(sc.points, sc.nodes, 4, sc.coverage)
    wp, wn = oracle_mod.warp_mesh(sc.points, sc.normals, sc.nodes, sc.gt_rotations, sc.gt_translations, a, w)
    fndc, fm = oracle_mod.extract_face_ndc(wp, sc.faces, sc.K, sc.H, sc.W, 0.0, 10.0)
    return wp, wn, fndc, fm


@pytest.mark.parametrize("name,blur,persp,clip", [("S1", 0.5, True, False), ("S1", 0.0, False, False), ("S1", 0.5, True, True),
                                                  ("C1", 0.5, True, False)])
def test_rasterize_k1_bit_exact(nn, S, oracle_mod, name, blur, persp, clip):
    sc = _scene(S, oracle_mod, name)
    _, _, fndc, fm = _warped_face_ndc(oracle_mod, sc)
    ref = oracle_mod.rasterize(fndc, fm, sc.H, sc.W, blur, 1, -1, -1, persp, clip, True)
    got = nn.rendering.rasterize_ndc_triangles(fndc, fm, (sc.H, sc.W), blur, 1, -1, -1, persp, clip, True)
    for r, g in zip(ref, got):
        assert np.array_equal(r, _np(g))


@pytest.mark.parametrize("k", [2, 4, 8])
def test_rasterize_multi_face_bit_exact(nn, S, oracle_mod, k):
    sc = _scene(S, oracle_mod, "S1")
    _, _, fndc, fm = _warped_face_ndc(oracle_mod, sc)
    ref = oracle_mod.rasterize(fndc, fm, sc.H, sc.W, 0.5, k, -1, -1, True, False, True)
    got = nn.rendering.rasterize_ndc_triangles(fndc, fm, (sc.H, sc.W), 0.5, k, -1, -1, True, False, True)
    for r, g in zip(ref, got):
        assert np.array_equal(r, _np(g))


def test_rasterize_edge_cases(nn, oracle_mod):
    H = W = 32
    # empty face set, all faces clipped, degenerate (zero-area) and back-facing triangles
    empty = np.zeros((0, 3, 3), np.float32)
    fi, dep, _, _ = nn.rendering.rasterize_ndc_triangles(empty, None, (H, W), 0.5, 1, -1, -1, True, False, True)
    assert (_np(fi) == -1).all() and (_np(dep) == -1).all()
    tri = np.array([[[-0.5, -0.5, 1.0], [-0.5, 0.5, 1.0], [0.5, -0.5, 1.0]],     # front
                    [[0.5, -0.5, 1.0], [-0.5, 0.5, 1.0], [-0.5, -0.5, 1.0]],     # back-facing
                    [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.1, 0.1, 1.0]]], np.float32)  # degenerate
    mask = np.array([1, 1, 1], np.uint8)
    for cull in (True, False):
        ref = oracle_mod.rasterize(tri, mask, H, W, 0.5, 1, -1, -1, True, False, cull)
        got = nn.rendering.rasterize_ndc_triangles(tri, mask, (H, W), 0.5, 1, -1, -1, True, False, cull)
        for r, g in zip(ref, got):
            assert np.array_equal(r, _np(g))
    ref = oracle_mod.rasterize(tri, np.zeros(3, np.uint8), H, W, 0.5, 1, -1, -1, True, False, True)
    assert (ref[0] == -1).all()
    got = nn.rendering.rasterize_ndc_triangles(tri, np.zeros(3, np.uint8), (H, W), 0.5, 1, -1, -1, True, False, True)
    assert (_np(got[0]) == -1).all()
    with pytest.raises(RuntimeError):
        nn.rendering.rasterize_ndc_triangles(tri, mask, (H, W), 0.5, 9, -1, -1, True, False, True)


@pytest.mark.parametrize("k", [1, 4])
def test_rasterize_non_finite_faces(nn, S, oracle_mod, k):
    """Faces with NaN / inf vertex coordinates (what an A7 NaN node rotation produces) are never rasterized, on every
    path: the oracle and the GPU agree bit for bit, and each pixel's winner is the winner without those faces."""
    sc = _scene(S, oracle_mod, "S1")
    _, _, fndc, fm = _warped_face_ndc(oracle_mod, sc)
    bad = fndc.copy()
    rng = np.random.default_rng(5)
    sel = rng.choice(len(bad), len(bad) // 7, replace=False)
    bad[sel[0::3], rng.integers(0, 3), rng.integers(0, 3)] = np.nan
    bad[sel[1::3], rng.integers(0, 3), 2] = np.inf
    bad[sel[2::3], rng.integers(0, 3), 0] = -np.inf
    ref = oracle_mod.rasterize(bad, fm, sc.H, sc.W, 0.5, k, -1, -1, True, False, True)
    got = nn.rendering.rasterize_ndc_triangles(bad, fm, (sc.H, sc.W), 0.5, k, -1, -1, True, False, True)
    for r, g in zip(ref, got):
        assert np.array_equal(r, _np(g))
    keep = fm.copy()
    keep[sel] = 0
    clean = oracle_mod.rasterize(fndc, keep, sc.H, sc.W, 0.5, k, -1, -1, True, False, True)
    assert np.array_equal(clean[0], ref[0])
    if k == 1:
        f1 = oracle_mod.rasterize_k1_fast(bad, fm, sc.H, sc.W, 0.5, True, True)
        assert np.array_equal(f1[0], ref[0])


def test_interpolate_and_unproject(nn, S, oracle_mod):
    sc = _scene(S, oracle_mod, "S1")
    wp, wn, fndc, fm = _warped_face_ndc(oracle_mod, sc)
    fi, dep, bary, _ = oracle_mod.rasterize(fndc, fm, sc.H, sc.W, 0.5, 1, -1, -1, True, False, True)
    attrs = wn[sc.faces]
    r = oracle_mod.interpolate_face_attributes(fi, bary, attrs)
    g = nn.rendering.functional.interpolate_vertex_attributes(fi, bary, attrs)
    assert np.array_equal(r, _np(g))
    depth = np.where(dep[..., 0] > 0, dep[..., 0], 0).astype(np.float32) * 1000.0
    p_o, m_o = oracle_mod.unproject(depth, sc.K, 1000.0, 10.0)
    p_g, m_g = nn.geometry.functional.unproject_raster_depth_without_filtering(depth, sc.K, depth_scale=1000.0, depth_max=10.0)
    assert np.array_equal(p_o, _np(p_g)) and np.array_equal(m_o, _np(m_g))


def test_rodrigues_and_block_cholesky_kats(nn, oracle_mod):
    R = nn.core.linalg.AxisAngleVectorsToMatricesRodrigues(L.RODRIGUES_AXIS_ANGLE)
    assert np.allclose(_np(R), L.RODRIGUES_EXPECTED, rtol=1e-3, atol=1e-7)
    assert np.array_equal(_np(R), oracle_mod.rodrigues(L.RODRIGUES_AXIS_ANGLE))
    for col in range(2):
        x = nn.core.linalg.SolveBlockDiagonalCholesky(L.CHOLESKY_A, L.CHOLESKY_B[:, col])
        assert np.allclose(_np(x), L.CHOLESKY_X[:, col], atol=2e-5, rtol=1e-4)
    with pytest.raises(RuntimeError):
        nn.core.linalg.SolveBlockDiagonalCholesky(-L.CHOLESKY_A, L.CHOLESKY_B[:, 0])


def test_arrowhead_long_back_substitution_chain(nn):
    """A corner no separator splits (every corner node shares a stem node with every other: a 700-node clique, 4200
    unknowns) is one nested-dissection group, i.e. one elimination-tree chain of 66 tile columns -- longer than the 64
    column descriptors k_corner_back stages in LDS at a time, so the chain crosses a staging block. The solve is held to
    the fp64 dense solution of the same system."""
    rng = np.random.default_rng(11)
    n0, n1 = 2, 700
    N = n0 + n1
    edges = np.array([(i, n0 + j) for i in range(n0) for j in range(n1)], np.int32)
    wing = rng.normal(0, 0.3, (len(edges), 6, 6)).astype(np.float32)
    diag = np.empty((N, 6, 6), np.float32)
    for i in range(N):
        A = rng.normal(size=(6, 6))
        diag[i] = (A @ A.T + 6 * np.eye(6) * (1 + (n1 if i < n0 else n0))).astype(np.float32)
    b = rng.normal(size=6 * N).astype(np.float32)
    x_g = _np(nn.core.linalg.SolveBlockSparseArrowheadCholesky(diag, wing, edges, n0, b)).astype(np.float64)
    Hd = np.zeros((6 * N, 6 * N))
    for i in range(N):
        Hd[6 * i:6 * i + 6, 6 * i:6 * i + 6] = diag[i]
    for e, (i, j) in enumerate(edges):
        Hd[6 * i:6 * i + 6, 6 * j:6 * j + 6] = wing[e]
        Hd[6 * j:6 * j + 6, 6 * i:6 * i + 6] = wing[e].T
    x64 = np.linalg.solve(Hd, b.astype(np.float64))
    assert rel_err(x_g, x64) < 1e-4
    assert np.abs(Hd @ x_g - b).max() < 1e-3 * np.abs(b).max()


@pytest.mark.parametrize("n0,n1,degree", [(40, 6, 4), (300, 30, 4), (1, 1, 1), (2000, 200, 4)])
def test_arrowhead_solver_vs_oracle(nn, oracle_mod, n0, n1, degree):
    rng = np.random.default_rng(n0)
    N = n0 + n1
    edges = []
    for i in range(n0):
        for j in rng.choice(n1, size=min(degree, n1), replace=False):
            edges.append((i, n0 + int(j)))
    edges = np.array(edges, np.int32)
    wing = rng.normal(0, 0.3, (len(edges), 6, 6)).astype(np.float32)
    diag = np.empty((N, 6, 6), np.float32)
    for i in range(N):
        A = rng.normal(size=(6, 6))
        diag[i] = (A @ A.T + 6 * np.eye(6) * (1 + degree)).astype(np.float32)
    for e, (i, j) in enumerate(edges):   # keep the full matrix diagonally dominant (SPD)
        diag[j] += np.eye(6, dtype=np.float32) * 6 * degree
    b = rng.normal(size=6 * N).astype(np.float32)
    x_o = oracle_mod.solve_arrowhead(diag, wing, edges, n0, b)
    x_g = _np(nn.core.linalg.SolveBlockSparseArrowheadCholesky(diag, wing, edges, n0, b))
    assert rel_err(x_g, x_o) < 1e-4
    # residual check against the assembled dense matrix (float64)
    Hd = np.zeros((6 * N, 6 * N))
    for i in range(N):
        Hd[6 * i:6 * i + 6, 6 * i:6 * i + 6] = diag[i]
    for e, (i, j) in enumerate(edges):
        Hd[6 * i:6 * i + 6, 6 * j:6 * j + 6] = wing[e]
        Hd[6 * j:6 * j + 6, 6 * i:6 * i + 6] = wing[e].T
    assert np.abs(Hd @ x_g - b).max() < 1e-3 * np.abs(b).max()


# ---------------------------------------------------------------------------------------------------------------------
# fused GN iteration
# ---------------------------------------------------------------------------------------------------------------------
def _gpu_fit(nn, sc, depth, iterations=1, lm=0.001, modes=None, tukey=False, coverage_method=0, graph=True, extrinsics=None,
             anchor_count=4, **fkw):
    G, A = nn.geometry, nn.alignment
    modes = modes or [A.IterationMode.ALL]
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, anchor_count, 0, G.WarpNodeCoverageComputationMethod(coverage_method),
                                      sc.layer_count)
    ft = A.DeformableMeshToImageFitter(iterations, modes, preconditioning_dampening_factor=lm, use_tukey_penalty_for_data_term=tukey,
                                       use_hip_graph=2 if graph else 0, **fkw)
    ft.fit_to_image(wf, G.TriangleMesh(sc.points, sc.normals, sc.faces), None, depth, None, sc.K, extrinsics, 1.0)
    return wf, ft, ft.diagnostics()


def nan_rel_err(a, b):
    """rel_err over the finite entries after asserting that both hold NaN at the same places (reference quirk A7: a
    node whose update has |omega| = 0 gets a NaN rotation, on both implementations)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN patterns differ"
    ok = np.isfinite(b)
    return rel_err(a[ok], b[ok]) if ok.any() else 0.0


def _compare_iteration(dg_o, dg_g, s, N):
    pf_o, pf_g = dg_o["pixel_faces"].astype(np.int64), dg_g["pixel_faces"].astype(np.int64)
    diff = np.nonzero(pf_o != pf_g)[0]
    assert len(diff) == 0, f"{len(diff)} rasterized faces differ, e.g. pixels {diff[:5]}: oracle {pf_o[diff[:5]]}, GPU {pf_g[diff[:5]]}"
    assert np.array_equal(dg_o["residual_mask"], dg_g["residual_mask"])
    assert np.allclose(dg_o["residuals"], dg_g["residuals"], rtol=0, atol=1e-6, equal_nan=True)
    assert nan_rel_err(dg_g["hessian"][: N * s * s], dg_o["hessian_diag"]) < 1e-6
    assert nan_rel_err(dg_g["gradient"][: N * s], dg_o["gradient"]) < 1e-6
    assert nan_rel_err(dg_g["updates"][: N * s], dg_o["updates"]) < 1e-4


@pytest.mark.parametrize("name", ["S1", "C1", "C2"])
def test_fit_one_iteration_parity(nn, S, oracle_mod, name):
    sc = _scene(S, oracle_mod, name)
    depth = scene_target(oracle_mod, sc)
    R_o, t_o, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1)
    wf, ft, dg_g = _gpu_fit(nn, sc, depth, 1)
    _compare_iteration(dg_o, dg_g, 6, len(sc.nodes))
    assert rel_err(wf.get_node_translations(True), t_o) < 1e-4
    assert rel_err(wf.get_node_rotations(True) - np.eye(3), R_o - np.eye(3)) < 1e-4


@pytest.mark.parametrize("name", ["S1", "C1", "C2", "C1_ARAP", "C2_ARAP", "C5"])
def test_reference_arithmetic_margins(nn, S, oracle_mod, name):
    """north_star's bar against the reference CPU path's own arithmetic (the oracle's default mode, restored here whatever
    the library build): one GN iteration per config, block-diagonal and ARAP. The product forms the pixel-node Jacobians
    as the reference's unfused products (csrc NNRT_JAC_FMA=0), so H and g agree to the fp64 summation order (1e-6); a
    development build with FMA-formed Jacobians (NNRT_JAC_FMA=1) is held to 1e-5 there. Faces and mask exact, residuals
    1e-6 absolute, updates, node translations and max |R - I| 1e-4 relative; every margin is printed."""
    from dynamicfuion_python_amd import _native
    oracle_mod.set_fused_jacobians(False)
    sc = _scene(S, oracle_mod, name)
    depth = scene_target(oracle_mod, sc)
    R_o, t_o, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1)
    wf, ft, dg_g = _gpu_fit(nn, sc, depth, 1)
    N = len(sc.nodes)
    assert np.array_equal(dg_o["pixel_faces"].astype(np.int64), dg_g["pixel_faces"].astype(np.int64))
    assert np.array_equal(dg_o["residual_mask"], dg_g["residual_mask"])
    r_abs = float(np.nanmax(np.abs(dg_o["residuals"] - dg_g["residuals"]))) if len(dg_o["residuals"]) else 0.0
    h_err = nan_rel_err(dg_g["hessian"][: N * 36], dg_o["hessian_diag"])
    g_err = nan_rel_err(dg_g["gradient"][: N * 6], dg_o["gradient"])
    u_err = nan_rel_err(dg_g["updates"][: N * 6], dg_o["updates"])
    t_err = rel_err(wf.get_node_translations(True), t_o)
    r_err = rel_err(wf.get_node_rotations(True) - np.eye(3), R_o - np.eye(3))
    fma = _native.jacobian_fma()
    print(f"{name} ({'FMA' if fma else 'unfused'} Jacobians) vs the reference arithmetic: residuals {r_abs:.2g} abs, H {h_err:.2g}, "
          f"g {g_err:.2g}, updates {u_err:.2g}, t {t_err:.2g}, R - I {r_err:.2g}")
    hg_bar = 1e-5 if fma else 1e-6
    assert r_abs <= 1e-6
    assert h_err < hg_bar and g_err < hg_bar
    assert u_err < 1e-4 and t_err < 1e-4 and r_err < 1e-4


@pytest.mark.parametrize("name,mode", [("C2", "ALL"), ("C1", "TRANSLATION_ONLY"), ("C1", "ROTATION_ONLY")])
def test_block_diagonal_update_bit_exact(nn, S, oracle_mod, name, mode):
    """The block-diagonal solve + update (k_solve_update_lanes: 8 lanes per node, lane r forming row r of the factor)
    performs the one-lane potrf + potrs float operations in the same order: on the GPU's own H and g, its updates equal
    the oracle's float block solve (orc_solve_block_diagonal; SolveBlockDiagonalCholeskyCUDA.cpp:59-100) bit for bit,
    and the node motion from identity equals t = 0 + dt, R = I . Rodrigues(w) (RodriguesImpl.h:66-88, A10) exactly."""
    sc = _scene(S, oracle_mod, name)
    depth = scene_target(oracle_mod, sc)
    wf, ft, dg = _gpu_fit(nn, sc, depth, 1, modes=[getattr(nn.alignment.IterationMode, mode)])
    s, N = (6 if mode == "ALL" else 3), len(sc.nodes)
    H = np.asarray(dg["hessian"][: N * s * s], np.float32).reshape(N, s, s)
    g = np.asarray(dg["gradient"][: N * s], np.float32)
    x_o, _ = oracle_mod.solve_block_diagonal(H, g, lm=0.001)
    x_g = np.asarray(dg["updates"][: N * s], np.float32)
    assert np.array_equal(x_g, x_o, equal_nan=True)
    x = x_g.reshape(N, s)
    t_g, R_g = wf.get_node_translations(True), wf.get_node_rotations(True)
    if mode == "ALL":
        assert np.array_equal(t_g, np.float32(0) + x[:, 3:], equal_nan=True)
    elif mode == "TRANSLATION_ONLY":
        assert np.array_equal(t_g, np.float32(0) + x, equal_nan=True)
    if mode != "TRANSLATION_ONLY":
        dR = oracle_mod.rodrigues(np.ascontiguousarray(x[:, :3])).reshape(N, 3, 3)
        I3 = np.eye(3, dtype=np.float32)
        R_e = np.empty_like(dR)
        for r in range(3):
            for c in range(3):
                R_e[:, r, c] = (I3[r, 0] * dR[:, 0, c] + I3[r, 1] * dR[:, 1, c]) + I3[r, 2] * dR[:, 2, c]
        assert np.array_equal(R_g.reshape(N, 3, 3), R_e, equal_nan=True)


@pytest.mark.parametrize("name,k", [("S1", 1), ("S1", 3), ("C1", 6), ("C1", 8)])
def test_fit_anchor_count_parity(nn, S, oracle_mod, name, k):
    """FitToImage with anchor counts other than the common 4 (the warp field's anchor_count,
    HierarchicalGraphWarpField.h:44): K < 4 runs the 4-slot pixel-kernel instantiation with empty slots, K > 4 the
    MAX_ANCHORS one and the lane-per-vertex warp; every stage against the oracle iteration with the same K."""
    sc = _scene(S, oracle_mod, name)
    depth = scene_target(oracle_mod, sc)
    R_o, t_o, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1, anchor_count=k)
    wf, ft, dg_g = _gpu_fit(nn, sc, depth, 1, anchor_count=k)
    _compare_iteration(dg_o, dg_g, 6, len(sc.nodes))
    assert rel_err(wf.get_node_translations(True), t_o) < 1e-4
    assert rel_err(wf.get_node_rotations(True) - np.eye(3), R_o - np.eye(3)) < 1e-4


def test_fit_without_valid_depth_parity(nn, S, oracle_mod):
    """A depth frame with no valid pixel (DeformableMeshToImageFitter.cpp:111-275 with an empty residual mask): no data
    term, H = LM damping only, a zero update and the reference's |omega| = 0 Rodrigues NaN (A7) -- on both
    implementations, NaN for NaN."""
    sc = _scene(S, oracle_mod, "S1")
    depth = np.zeros_like(scene_target(oracle_mod, sc))
    _, _, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1)
    wf, ft, dg_g = _gpu_fit(nn, sc, depth, 1)
    assert not dg_g["residual_mask"].any() and not dg_o["residual_mask"].any()
    _compare_iteration(dg_o, dg_g, 6, len(sc.nodes))


@pytest.mark.parametrize("mode", ["TRANSLATION_ONLY", "ROTATION_ONLY"])
def test_fit_single_mode_parity(nn, S, oracle_mod, mode):
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    _, _, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1, modes=(mode,))
    _, _, dg_g = _gpu_fit(nn, sc, depth, 1, modes=[nn.alignment.IterationMode[mode]])
    _compare_iteration(dg_o, dg_g, 3, len(sc.nodes))


def test_fit_mode_cycle_state_synchronised(nn, S, oracle_mod):
    """An iteration-mode list cycles over the iterations (DeformableMeshToImageFitter.cpp:111-120, mode = modes[i %
    count]): TRANSLATION_ONLY, ROTATION_ONLY, ALL, TRANSLATION_ONLY from one prepared frame, each iteration checked
    against the oracle's single-mode iteration started from exactly the GPU's node motion before it."""
    G, A = nn.geometry, nn.alignment
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    N = len(sc.nodes)
    modes = ["TRANSLATION_ONLY", "ROTATION_ONLY", "ALL"]
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                      sc.layer_count)
    ft = A.DeformableMeshToImageFitter(4, [A.IterationMode[m] for m in modes], preconditioning_dampening_factor=0.001)
    ft.prepare(wf, G.TriangleMesh(sc.points, sc.normals, sc.faces), depth, None, sc.K)
    for k in range(4):
        R0, t0 = wf.get_node_rotations(True), wf.get_node_translations(True)
        ft.iterate(wf, k, 1)
        m = modes[k % len(modes)]
        _, _, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1, R0=R0, t0=t0, modes=(m,))
        _compare_iteration(dg_o, ft.diagnostics(), 6 if m == "ALL" else 3, N)
        R1, t1 = wf.get_node_rotations(True), wf.get_node_translations(True)
        if m == "TRANSLATION_ONLY":
            assert np.array_equal(R1, R0)
        if m == "ROTATION_ONLY":
            assert np.array_equal(t1, t0)


def test_fit_tukey_and_variable_coverage_parity(nn, S, oracle_mod):
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    _, _, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1, use_tukey=True, tukey_cutoff=0.01)
    _, _, dg_g = _gpu_fit(nn, sc, depth, 1, tukey=True, tukey_penalty_cutoff_cm=0.01)
    _compare_iteration(dg_o, dg_g, 6, len(sc.nodes))
    cw = oracle_mod.node_coverage_weights(sc.nodes, sc.coverage)
    _, _, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1, coverage_method=1, node_weights=cw)
    _, _, dg_g = _gpu_fit(nn, sc, depth, 1, coverage_method=1)
    _compare_iteration(dg_o, dg_g, 6, len(sc.nodes))


NOT_POSITIVE_DEFINITE = 3   # include/nnrt_mi355x.h NNRT_ERROR_NOT_POSITIVE_DEFINITE


REFINE_PIVOT_RATIO = 1e-7   # fp64 min / max Cholesky pivot above which the arrowhead solve is held to 1e-4
REFINED_PIVOT_RATIO = 1e-12  # ... and above which an accepted refinement step is (measured converging down to 6e-12)
REFINE_FLOOR = 1e-5         # csrc/fitter_kernels.hpp NNRT_REFINE_PIVOT_FLOOR: no refinement below this corner pivot / diag(S)


def _synchronised_iteration(nn, oracle_mod, sc, depth, wf, ft, k):
    """One GN iteration on the GPU from the warp field's current motion, checked against the oracle started from exactly
    that motion (read back bit for bit). Returns (status, update rel err): status "ok", or "potrf" when both
    implementations hit the reference's potrf failure (NNRT_LAPACK_CHECK) in this iteration."""
    from dynamicfuion_python_amd._native import NnrtError
    N = len(sc.nodes)
    R0, t0 = wf.get_node_rotations(True), wf.get_node_translations(True)
    ft.iterate(wf, k, 1)
    dg_g = ft.diagnostics()
    gpu_failed = False
    try:
        ft.check()
    except NnrtError as e:
        assert e.status == NOT_POSITIVE_DEFINITE, str(e)
        gpu_failed = True
    try:
        R_o, t_o, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1, R0=R0, t0=t0, raise_on_failure=False)
        oracle_failed = dg_o["status"] != 0
    except RuntimeError as e:   # the arrowhead solve aborts without diagnostics
        oracle_failed, dg_o, oracle_msg = True, None, str(e)
    else:
        oracle_msg = ""
    if gpu_failed != oracle_failed:
        # Only one float32 factorization broke down. Allowed only on an arrowhead system that is positive definite but so
        # ill-conditioned in fp64 that a float32 Cholesky's success depends on its elimination order (the GPU's
        # nested-dissection corner vs the oracle's natural order); the trajectory ends there (the reference raises on
        # one side only, so later states have no counterpart).
        msg = (f"iteration {k + 1}: GPU potrf failure {gpu_failed}, oracle {oracle_failed} ({oracle_msg}); GPU H / g / updates "
               f"non-finite: {int((~np.isfinite(dg_g['hessian'])).sum())} / {int((~np.isfinite(dg_g['gradient'])).sum())} / "
               f"{int((~np.isfinite(dg_g['updates'])).sum())}")
        assert sc.layer_count > 1, msg
        A, _ = arrowhead_fp64_system(oracle_mod, sc, R0, t0, hessian_diag=dg_g["hessian"][: N * 36], gradient=dg_g["gradient"][: 6 * N])
        ratio = fp64_pivot_ratio(A)
        assert 0.0 < ratio < 1e-6, f"{msg}; fp64 min / max Cholesky pivot {ratio:.3g}"
        if not gpu_failed:
            assert np.isfinite(dg_g["updates"][: 6 * N]).all(), msg
        return f"potrf ({'oracle' if oracle_failed else 'GPU'} only: fp64 pivot ratio {ratio:.2g})", None, {}
    if gpu_failed:
        if dg_o is not None:   # block-diagonal: the same blocks fail (NaN updates), every other node's update agrees
            u_g, u_o = dg_g["updates"][: 6 * N], dg_o["updates"]
            assert nan_rel_err(u_g, u_o) < 1e-4
            assert np.array_equal(dg_o["pixel_faces"].astype(np.int64), dg_g["pixel_faces"].astype(np.int64))
            assert nan_rel_err(dg_g["hessian"][: N * 36], dg_o["hessian_diag"]) < 1e-6
        return "potrf", None, {}
    solve_note = ""
    e_own = None
    info = {"own": None, "exact": None, "oracle_float": None, "gate": None}
    u_err = nan_rel_err(dg_g["updates"][: 6 * N], dg_o["updates"])
    if sc.layer_count > 1:
        # the solve against the fp64 solution of EXACTLY the float system the GPU factored and refined (its diagonal
        # blocks with LM, wing blocks and right-hand side, exported by nnrt_fitter_get_arrowhead_system): the solver's own
        # error, free of any assembly difference. A refined solve, and any solve of a system whose
        # fp64 pivot ratio exceeds REFINE_PIVOT_RATIO, must be within 1e-4 of it.
        x_exact, ratio_exact = exact_system_solution(ft, wf, N)
        gate = ft.refine_info()
        info["gate"] = gate
        if x_exact is not None:
            e_exact = nan_rel_err(dg_g["updates"][: 6 * N], x_exact)
            info["exact"] = e_exact
            solve_note += (f", exact-system err {e_exact:.2g} (its fp64 pivot ratio {ratio_exact:.2g}; corner pivot / diag(S) "
                           f"{gate['pivot_ratio']:.2g}, refined {gate['refined']})")
            solve_note += f", correction {gate['correction']:.2g} accepted {gate['accepted']}" if gate["refined"] else ""
            if (gate["refined"] and gate["accepted"] and ratio_exact > REFINED_PIVOT_RATIO) or ratio_exact > REFINE_PIVOT_RATIO:
                assert e_exact <= 1e-4, (f"iteration {k + 1}: solve {e_exact:.3g} from the fp64 solution of its own float system "
                                         f"(refined {gate['refined']}, accepted {gate['accepted']}, corner pivot / diag(S) "
                                         f"{gate['pivot_ratio']:.3g}, fp64 pivot ratio {ratio_exact:.3g})")
        # The GPU's arrowhead solve (f32 factor + one step of iterative refinement with an fp64 residual) against the fp64
        # solution of the GPU's own normal equations (its data blocks and right-hand side): wherever the system's fp64
        # Cholesky pivot ratio exceeds REFINE_PIVOT_RATIO the solve must reach 1e-4 (the 2x-oracle rule below
        # is kept only for the degenerate iterations under it)
        A_own, b_own = arrowhead_fp64_system(oracle_mod, sc, R0, t0, hessian_diag=dg_g["hessian"][: N * 36], gradient=dg_g["gradient"][: 6 * N])
        import scipy.sparse.linalg as spl
        e_own = nan_rel_err(dg_g["updates"][: 6 * N], spl.spsolve(A_own.tocsc(), b_own))
        ratio_own = fp64_pivot_ratio(A_own)
        info["own"] = e_own
        solve_note += f", assembled-system err vs fp64 {e_own:.2g} (fp64 pivot ratio {ratio_own:.2g})"
        if ratio_own > REFINE_PIVOT_RATIO:
            assert e_own <= 1e-4, f"iteration {k + 1}: refined solve error {e_own:.3g} vs fp64 at pivot ratio {ratio_own:.3g}"
        # ... and against the fp64 solution of the ORACLE's normal equations: the two float systems
        # differ by assembly rounding (delta, measured on H and g; <= 1e-6 by _compare_iteration), which the system's
        # conditioning amplifies by about 1 / (fp64 pivot ratio). Both the fp64 solutions' own distance and the GPU
        # update's distance from the oracle system's solution must stay inside that predicted amplification.
        A_o, b_o = arrowhead_fp64_system(oracle_mod, sc, R0, t0, dg_o)
        x64_o = spl.spsolve(A_o.tocsc(), b_o)
        delta = max(nan_rel_err(dg_g["hessian"][: N * 36], dg_o["hessian_diag"]), nan_rel_err(dg_g["gradient"][: 6 * N], dg_o["gradient"]))
        predicted = 4.0 * delta / max(ratio_own, 1e-300)
        d64 = nan_rel_err(spl.spsolve(A_own.tocsc(), b_own), x64_o)
        e_oracle_sys = nan_rel_err(dg_g["updates"][: 6 * N], x64_o)
        info["oracle_float"] = nan_rel_err(dg_o["updates"], x64_o)   # the reference-order float solve's own error
        solve_note += f", vs the oracle system's fp64 solution {e_oracle_sys:.2g} (fp64 solutions {d64:.2g} apart, predicted <= {predicted:.2g})"
        assert d64 <= max(1e-4, predicted), f"iteration {k + 1}: fp64 solutions {d64:.3g} apart, assembly {delta:.3g} predicts {predicted:.3g}"
        assert e_oracle_sys <= max(1e-4, e_own + predicted), \
            f"iteration {k + 1}: update {e_oracle_sys:.3g} from the oracle system's fp64 solution (own {e_own:.3g}, predicted {predicted:.3g})"
    if sc.layer_count > 1 and u_err >= 1e-4:
        # Ill-conditioned arrowhead system: two float32 solves with different blockings cannot agree to 1e-4 (the GPU
        # factors the dense Schur corner with MFMA tiles, the oracle serially). Both are held against the fp64 solution
        # of the same system instead: the GPU's solve must be as accurate as the reference-order float solve.
        # each solver against the fp64 solution of its OWN normal equations (the GPU's and the oracle's float systems differ by
        # assembly rounding, ~1e-7 relative, which an ill-conditioned system amplifies beyond any solver's doing)
        x64 = arrowhead_fp64_solution(oracle_mod, sc, R0, t0, dg_o)
        e_g = e_own
        e_o = nan_rel_err(dg_o["updates"], x64)
        assert e_g <= max(2.0 * e_o, 1e-4), f"iteration {k + 1}: GPU solve error {e_g:.3g} vs fp64, oracle float solve {e_o:.3g}"
        solve_note += (f", ill-conditioned solve: GPU err vs fp64 {e_g:.2g}, oracle f32 err vs fp64 {e_o:.2g} (GPU vs the oracle's fp64 "
                       f"system {nan_rel_err(dg_g['updates'][: 6 * N], x64):.2g})")
        dg_g = dict(dg_g, updates=dg_o["updates"])   # the remaining checks are the data term's and the raster's
    _compare_iteration(dg_o, dg_g, 6, N)
    R_g, t_g = wf.get_node_rotations(True), wf.get_node_translations(True)
    # node motion: the translation increments against the oracle (they are the updates' translation rows), and the
    # rotations as R0 . Rodrigues(omega) of the GPU's own update (fp64 restatement, A7 NaN at |omega| = 0, A10 right
    # multiplication): the update itself is held to 1e-4 above
    # node motion = the GPU's own update applied to the state it started from: t += dt (float32, exact) and
    # R <- R . Rodrigues(omega) (checked against an fp64 restatement below); the update itself is held to the oracle's
    xg = ft.diagnostics()["updates"][: 6 * N].reshape(N, 6)
    assert np.array_equal(t_g, (t0 + xg[:, 3:]).astype(np.float32), equal_nan=True)
    x = xg.astype(np.float64)
    th = np.linalg.norm(x[:, :3], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = x[:, :3] / th[:, None]
    Kx = np.zeros((N, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
    dR = np.eye(3) + np.sin(th)[:, None, None] * Kx + (1 - np.cos(th))[:, None, None] * (Kx @ Kx)
    R_expect = R0.astype(np.float64) @ dR
    assert np.array_equal(np.isnan(R_g), np.isnan(R_expect))
    ok = np.isfinite(R_expect)
    assert np.abs(R_g[ok] - R_expect[ok]).max(initial=0.0) < 1e-5
    nan_nodes = int(np.isnan(R_g).reshape(N, -1).any(1).sum())
    return ("ok" if nan_nodes == 0 else f"ok, {nan_nodes} NaN rotations (A7)") + solve_note, u_err, info


def _new_fit(nn, sc, depth, iterations):
    G, A = nn.geometry, nn.alignment
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                      sc.layer_count)
    ft = A.DeformableMeshToImageFitter(iterations, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001)
    ft.prepare(wf, G.TriangleMesh(sc.points, sc.normals, sc.faces), depth, None, sc.K)
    return wf, ft


# (config, iterations run, iterations that must succeed, the iteration at which the reference algorithm itself must
# raise potrf or None). The reference's GN step is block-diagonal in the data term (A17) and overshoots: on C2 its
# iteration-2 Hessian blocks lose positive definiteness in float (condition > 1e10), i.e. FitToImage throws there -- on
# the GPU and in the oracle alike. The ARAP configs run until the arrowhead system degenerates (A7 NaN rotations,
# condition > 1e9); wherever a potrf failure occurs, both implementations must hit it in the same iteration. C5: the
# GPU's iteration-3 solve lies closer to the fp64 solution than the oracle's float solve (5.4e-4 vs 8.3e-4), and from
# the state it reaches both implementations raise potrf at iteration 4 (7 A7 NaN rotations by then). C2_ARAP: after
# iteration 4 (condition ~1e9, both float solves 0.14 from fp64, one A7 NaN rotation) the iteration-5 system is positive
# definite in fp64 with a pivot ratio below 1e-6: the oracle's natural-order float Cholesky breaks down, the GPU's
# nested-dissection order does not (round 2's order broke down too) -- accepted as a one-sided breakdown, trajectory ends.
# The C5 trajectory's solve errors vs the fp64 solution of its own system at iterations 1-3, measured 1.6e-6 / 1.8e-5 /
# 1.7e-4 (round 5, multi-wave panel elimination; iteration 3 at an fp64 pivot ratio 2.1e-8, below REFINE_PIVOT_RATIO, where
# no 1e-4 rule applies; its corner pivot / diag(S) 7.7e-5 lies just under the refinement floor, so it is not refined --
# the one-wave elimination's rounding put it above and refined it to 1.0e-4, a floor of 5e-5 refines it to 1.3e-4; the
# oracle's own float solve is 6.8e-4 from fp64): pinned at 1.5x as regression bounds. Iteration 4 is degenerate (35 A7 NaN rotations, corner pivot /
# diag(S) 3.8e-7 below the refinement floor, fp64 pivot ratio 7e-12): 0.011, the oracle's float solve 0.016.
# The FMA-formed Jacobians (csrc NNRT_JAC_FMA, the product build) assemble a system a few float ulps away per term, and
# from iteration 2 on the trajectory visits different states (iteration 2: 1 A7 NaN rotation; iteration 3: fp64 pivot
# ratio 7.4e-9, corner pivot / diag(S) 7.5e-5, unrefined): measured 1.6e-6 / 2.5e-5 / 1.04e-3, the oracle's own float
# solve of that iteration-3 system 6.0e-4 from fp64. Each build's trajectory is pinned at its own measurement.
# Round 6: these errors are measured against a system re-assembled from the ORACLE's ARAP blocks, whose own 2^-24 entry
# rounding moves the fp64 solution by 8.7e-6 (iteration 2) .. 4e-6 (iteration 3) here -- the floor any solver meets them
# at (the GPU's refined solves are 2e-8 / 3e-7 from the fp64 solution of their OWN system: PINNED_EXACT_ERRORS); a
# development build that re-associated the substitution sums moved iteration 2's from 2.0e-5 to 3.0e-5, its exact error unchanged
PINNED_SOLVE_ERRORS = {("C5", 1): 3e-6, ("C5", 2): 5e-5, ("C5", 3): 2.6e-4}
PINNED_SOLVE_ERRORS_FMA = {("C5", 1): 3e-6, ("C5", 2): 3e-5, ("C5", 3): 1.6e-3}
# the same iterations against the fp64 solution of exactly the float system the GPU solved (nnrt_fitter_get_arrowhead_system;
# round 6, floor 1e-5, window to 1e-2, safeguarded step): measured 1.4e-6 (unrefined, gate 0.27) / 2.2e-8 / 3.0e-7 (refined,
# gates 0.0018 and 7.4e-5, corrections 8.3e-6 and 5.4e-4 accepted) -- VERDICT r5 item 2's C5 iteration 3, refined to well
# under 1e-4 of its exact solution
PINNED_EXACT_ERRORS = {("C5", 1): 3e-6, ("C5", 2): 1e-6, ("C5", 3): 1e-6}
TRAJECTORIES = [("S1", 6, 6, None), ("C2", 2, 1, 2), ("C2_ARAP", 10, 4, None), ("C5", 6, 3, None)]


@pytest.mark.parametrize("name,iterations,min_ok,fails_at", TRAJECTORIES)
def test_fit_state_synchronised_trajectory(nn, S, oracle_mod, name, iterations, min_ok, fails_at):
    """GN iterations 1..n of one frame (DeformableMeshToImageFitter.cpp:111-275), each checked against the oracle
    started from exactly the GPU's node motion before it. Iterations k >= 2 run the general kernels (non-identity R/t in
    the warp and update, deformed meshes, changed associations) without the compounding of the reference's divergent
    GN between two implementations; the iteration at which the reference raises potrf must raise on both."""
    sc = _scene(S, oracle_mod, name)
    depth = scene_target(oracle_mod, sc)
    wf, ft = _new_fit(nn, sc, depth, iterations)
    report = []
    for k in range(iterations):
        nan_before = int(np.isnan(wf.get_node_rotations(True)).reshape(len(sc.nodes), -1).any(1).sum())
        status, err, info = _synchronised_iteration(nn, oracle_mod, sc, depth, wf, ft, k)
        print(f"{name} iteration {k + 1}: {status}, update rel err {err}, NaN rotations before {nan_before}", flush=True)
        report.append((k + 1, status, err))
        from dynamicfuion_python_amd import _native
        pin = (PINNED_SOLVE_ERRORS_FMA if _native.jacobian_fma() else PINNED_SOLVE_ERRORS).get((name, k + 1))
        if pin is not None:   # the measured errors vs fp64 as regression bounds
            e_own, e_exact, e_of = info.get("own"), info.get("exact"), info.get("oracle_float")
            assert e_own is not None and e_own <= pin, f"{name} iteration {k + 1}: solve error vs fp64 {e_own} above its pinned {pin:.3g}"
            # ... and never less accurate than the reference-order float solve: each solver against the
            # fp64 solution of its own float system (the GPU's exported exactly, the oracle's assembled from its blocks)
            assert e_exact <= max(e_of, 1e-5), f"{name} iteration {k + 1}: GPU {e_exact:.3g} vs fp64, the oracle's float solve {e_of:.3g}"
            pin_x = PINNED_EXACT_ERRORS.get((name, k + 1))
            if pin_x is not None:
                assert e_exact is not None and e_exact <= pin_x, f"{name} iteration {k + 1}: exact-system error {e_exact} above {pin_x:.3g}"
        if status.startswith("potrf"):
            break
    print(f"{name}: {report}")
    assert sum(r[1].startswith("ok") for r in report) >= min_ok
    if fails_at is not None:
        assert report[-1][1] == "potrf" and report[-1][0] == fails_at


@pytest.mark.parametrize("name,iterations", [("C1_ARAP", 4), ("C2_ARAP", 5), ("C5", 4)])
def test_refinement_gate(nn, S, oracle_mod, name, iterations):
    """The arrowhead solve's refinement gate (one step of iterative refinement when the corner factorization's smallest
    pivot / diag(S) lies in [REFINE_FLOOR, threshold)) against what refinement buys. Along the GPU's
    own trajectory every iteration is solved twice from the same motion, the gate forced shut (threshold 0) and forced
    open (threshold inf; still nothing below the floor, where one step does not converge), and both are compared with the
    fp64 solution of that iteration's normal equations (the GPU's data blocks and right-hand side, identical in both
    runs). Where the product gate stays shut above the floor the plain f32 solve must already meet 1e-4; wherever the
    fp64 pivot ratio exceeds REFINE_PIVOT_RATIO the product's solve must."""
    import scipy.sparse.linalg as spl
    from dynamicfuion_python_amd._native import NnrtError
    sc = _scene(S, oracle_mod, name)
    depth = scene_target(oracle_mod, sc)
    N = len(sc.nodes)
    wf, ft = _new_fit(nn, sc, depth, iterations)
    threshold = ft.refine_info()["threshold"]
    from dynamicfuion_python_amd import _native
    floor = _native.refine_floor()   # REFINE_FLOOR in the product build; development builds may lower it

    def solve(R0, t0, k, ratio):
        wf.set_node_rotations(R0, True)
        wf.set_node_translations(t0, True)
        ft.set_refine_ratio(ratio)
        ft.iterate(wf, k, 1)
        try:
            ft.check()
        except NnrtError:
            return None
        dg = ft.diagnostics()
        info = ft.refine_info()
        return dg["updates"][: 6 * N].copy(), dg["hessian"][: 36 * N].copy(), dg["gradient"][: 6 * N].copy(), info["pivot_ratio"], info

    rows = []
    for k in range(iterations):
        R0, t0 = wf.get_node_rotations(True), wf.get_node_translations(True)
        if not np.isfinite(R0).all():
            break   # A7 NaN rotations: the systems from here on are degenerate
        plain = solve(R0, t0, k, 0.0)
        refined = solve(R0, t0, k, np.inf)
        if plain is None or refined is None:
            break
        assert np.array_equal(plain[1], refined[1]) and np.array_equal(plain[2], refined[2])
        assert plain[3] == refined[3]   # the same factorization
        # judged against the fp64 solution of exactly the float system both solves factored (the fitter's export; VERDICT
        # r5 item 2) -- until round 5 against a system re-assembled from the oracle's ARAP blocks, whose 2^-24 entry
        # differences alone moved the fp64 solution by up to 2.6e-4 at these pivot ratios
        x64, ratio64 = exact_system_solution(ft, wf, N)
        if x64 is None:
            break
        e_plain, e_ref = nan_rel_err(plain[0], x64), nan_rel_err(refined[0], x64)
        gate = plain[3]
        rows.append((k + 1, gate, ratio64, e_plain, e_ref))
        refines = gate >= floor                 # the forced-open solve ran the refinement step
        opens = refines and gate < threshold    # ... and the product's gate does
        print(f"{name} iteration {k + 1}: corner pivot / diag(S) {gate:.3g} (gate {'open' if opens else 'shut'}: window "
              f"[{floor:g}, {threshold:g})), exact-system fp64 pivot ratio {ratio64:.3g}, err vs fp64: plain f32 {e_plain:.3g}, "
              f"forced refinement {e_ref:.3g}", flush=True)
        accepted = refined[4]["accepted"]
        print(f"    forced step: max |d| / max |x| {refined[4]['correction']:.3g}, accepted {accepted}", flush=True)
        if gate >= threshold:
            assert e_plain <= 1e-4, f"iteration {k + 1}: gate shut at {gate:.3g} but the plain solve is {e_plain:.3g} from fp64"
        if refines:
            # the safeguard: a step never leaves the solve further from the exact solution than the plain solve (a rejected
            # step keeps the plain solve bit for bit) ...
            assert e_ref <= max(e_plain, 1e-4), f"iteration {k + 1}: refined {e_ref:.3g} vs plain {e_plain:.3g}"
            if not accepted:
                assert np.array_equal(refined[0], plain[0])
            # ... and an accepted one converges wherever the system is not degenerate
            if accepted and ratio64 > REFINED_PIVOT_RATIO:
                assert e_ref <= 1e-4, f"iteration {k + 1}: refined solve {e_ref:.3g} from fp64 at corner pivot / diag(S) {gate:.3g}"
        elif ratio64 > REFINE_PIVOT_RATIO:
            assert e_plain <= 1e-4, f"iteration {k + 1}: unrefined solve {e_plain:.3g} from fp64 at fp64 pivot ratio {ratio64:.3g}"
        if not opens:   # continue along the product's trajectory
            solve(R0, t0, k, 0.0)
    ft.set_refine_ratio(threshold)
    print(f"{name}: {rows}")
    assert len(rows) >= 2


@pytest.mark.parametrize("name,walk", [("C5", "1"), ("C2_ARAP", "0"), ("C1_ARAP", "0")])
def test_flow_substitution_matches_chain_launches(nn, S, oracle_mod, name, walk):
    """The dataflow substitution launches (k_corner_flow: the back chains and the stem pass in one launch, the whole
    gated refinement step in a second) perform the same float operations as the per-depth chain launches they replace:
    along three GN iterations with the refinement forced open wherever the gate's floor allows (and once shut), updates,
    node motion and gate words are bit-identical between fitters planned with NNRT_CORNER_FLOW=1 and =0 (with
    NNRT_CORNER_TRIM=1 / 0: eliminations stopped at a tile's real columns against full 64-column ones;
    NNRT_CORNER_FOLD_INV=1 / 0: the diagonal inverses formed in the last factor launch against a k_corner_invert launch;
    NNRT_CORNER_WALK=0 makes the small C1 / C2 corners use chains instead of the single-workgroup walk)."""
    import os
    sc = _scene(S, oracle_mod, name)
    depth = scene_target(oracle_mod, sc)
    N = len(sc.nodes)
    runs = {}
    old = {k: os.environ.get(k) for k in ("NNRT_CORNER_FLOW", "NNRT_CORNER_WALK", "NNRT_CORNER_TRIM", "NNRT_CORNER_FOLD_INV")}
    try:
        os.environ["NNRT_CORNER_WALK"] = walk
        for flow in ("1", "0"):
            os.environ["NNRT_CORNER_FLOW"] = flow
            os.environ["NNRT_CORNER_TRIM"] = flow   # the padding-trimmed eliminations change no bit either
            os.environ["NNRT_CORNER_FOLD_INV"] = flow   # nor the inverses' launch
            wf, ft = _new_fit(nn, sc, depth, 3)
            rows = []
            for k, ratio in enumerate((np.inf, 0.0, np.inf)):
                ft.set_refine_ratio(ratio)
                ft.iterate(wf, k, 1)
                ft.check()
                dg = ft.diagnostics()
                rows.append((dg["updates"][: 6 * N].copy(), wf.get_node_rotations(True), wf.get_node_translations(True), ft.refine_info()))
            runs[flow] = rows
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for k, (a, b) in enumerate(zip(runs["1"], runs["0"])):
        assert np.array_equal(a[0], b[0], equal_nan=True), f"iteration {k + 1}: updates differ"
        assert np.array_equal(a[1], b[1], equal_nan=True) and np.array_equal(a[2], b[2], equal_nan=True), f"iteration {k + 1}: motion differs"
        assert a[3] == b[3]
        print(f"{name} iteration {k + 1}: gate {a[3]}", flush=True)


def test_fit_c2_from_stored_states(nn, S, oracle_mod):
    """C2 GN iterations from ten non-identity node states (fractions of the ground-truth motion plus noise: the
    states a frame passes through between the identity and the solution) -- the general warp / update kernels on a
    deformed C2 mesh, where the reference's own trajectory stops at iteration 2 (see TRAJECTORIES)."""
    sc = _scene(S, oracle_mod, "C2")
    depth = scene_target(oracle_mod, sc)
    wf, ft = _new_fit(nn, sc, depth, 1)
    vidx = np.arange(len(sc.nodes))
    states = [(0.5, 0), (0.25, 1e-3), (0.5, 1e-3), (0.75, 1e-3), (1.0, 1e-3), (1.25, 1e-3), (1.5, 2e-3), (-0.5, 1e-3), (0.9, 3e-3), (2.0, 0)]
    for j, (fraction, noise) in enumerate(states):
        R, t = sc.partial_motion(fraction, seed=j, noise=noise)
        wf.set_node_rotations(R[vidx])
        wf.set_node_translations(t[vidx])
        status, err, _ = _synchronised_iteration(nn, oracle_mod, sc, depth, wf, ft, j + 1)
        assert status.startswith("ok"), f"state {j}: {status}"


@pytest.mark.parametrize("name", ["S1_ARAP", "C1_ARAP", "C2_ARAP", "C5"])
def test_fit_arap_parity(nn, S, oracle_mod, name):
    """layer_count 2 + ARAP: arrowhead (stem blocks + dense Schur corner) solve."""
    sc = _scene(S, oracle_mod, name)
    wf = nn.geometry.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, nn.geometry.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                                sc.layer_count)
    assert np.array_equal(wf.get_virtual_node_indices(), sc.hierarchy["virtual_indices"])
    assert np.array_equal(wf.get_edges(), sc.hierarchy["edges"])
    depth = scene_target(oracle_mod, sc)
    R_o, t_o, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1)
    wf, _, dg_g = _gpu_fit(nn, sc, depth, 1)
    _compare_iteration(dg_o, dg_g, 6, len(sc.nodes))
    assert rel_err(wf.get_node_translations(True), t_o) < 1e-4


@pytest.mark.parametrize("name", ["S1_ARAP4", "C2_ARAP3", "C2_ARAP4"])
def test_fit_multilayer_arap_parity(nn, S, oracle_mod, name):
    """>= 3 layers (the binding's default is 4, HierarchicalGraphWarpField.h:44): edges whose source lies outside layer 0
    give corner off-diagonal blocks, which the reference computes into locals and drops (A3, ArapHessianImpl.h:81-84,
    :147-154); both implementations follow the uncapped math of sparse_block_cholesky_scripts.py:106-160 instead. The
    first iteration's update is held to the fp64 solution of the same normal equations (corner-corner blocks included)
    as tightly as the oracle's float solve; then two GN iterations, each state-synchronised against the oracle (H, g
    <= 1e-6; updates <= 1e-4 or, ill-conditioned, the fp64 rule)."""
    sc = _scene(S, oracle_mod, name)
    h = sc.hierarchy
    N = len(sc.nodes)
    assert len(h["layer_counts"]) == sc.layer_count >= 3
    assert (h["edges"][:, 0] >= h["layer_counts"][0]).any(), "no corner off-diagonal blocks"
    depth = scene_target(oracle_mod, sc)
    _, _, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1)
    wf, _, dg_g = _gpu_fit(nn, sc, depth, 1)
    assert np.array_equal(wf.get_edges(), h["edges"])
    I3 = np.tile(np.eye(3, dtype=np.float32), (N, 1, 1))
    x64 = arrowhead_fp64_solution(oracle_mod, sc, I3, np.zeros((N, 3), np.float32), dg_o)
    x64_g = arrowhead_fp64_solution(oracle_mod, sc, I3, np.zeros((N, 3), np.float32), None, hessian_diag=dg_g["hessian"][: 36 * N],
                                    gradient=dg_g["gradient"][: 6 * N])
    e_g = nan_rel_err(dg_g["updates"][: 6 * N], x64_g)   # each solver vs the fp64 solution of its own normal equations
    e_o = nan_rel_err(dg_o["updates"], x64)
    print(f"{name}: layers {list(h['layer_counts'])}, GPU update err vs fp64 {e_g:.3g}, oracle float {e_o:.3g}")
    assert e_g <= max(2.0 * e_o, 1e-4)
    wf, ft = _new_fit(nn, sc, depth, 2)
    for k in range(2):
        status, err, _ = _synchronised_iteration(nn, oracle_mod, sc, depth, wf, ft, k)
        print(f"{name} iteration {k + 1}: {status}, update rel err {err}")
        assert status.startswith("ok"), status


def test_c5_four_layer_solve_vs_fp64(nn, S, oracle_mod):
    """C5's graph (5000 nodes) at the binding's default of 4 layers: the GPU's own normal equations (its data blocks and
    right-hand side, checked against the oracle at smaller sizes above) solved in fp64 -- the tile-sparse corner with its
    corner-corner blocks must reproduce that solution within 1e-4 relative."""
    sc = _scene(S, oracle_mod, "C5_L4")
    N = len(sc.nodes)
    depth = scene_target(oracle_mod, sc)
    wf, ft, dg_g = _gpu_fit(nn, sc, depth, 1)
    I3 = np.tile(np.eye(3, dtype=np.float32), (N, 1, 1))
    x64 = arrowhead_fp64_solution(oracle_mod, sc, I3, np.zeros((N, 3), np.float32), None, hessian_diag=dg_g["hessian"][: 36 * N],
                                   gradient=dg_g["gradient"][: 6 * N])
    e_g = nan_rel_err(dg_g["updates"][: 6 * N], x64)
    print(f"C5_L4: layers {list(sc.hierarchy['layer_counts'])}, GPU update err vs fp64 {e_g:.3g}")
    assert e_g < 1e-4


def test_hip_graph_matches_eager(nn, S, oracle_mod):
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    # one iteration: identical work, only the fp64 atomic order may differ -> identical float results
    wf1, _, d1 = _gpu_fit(nn, sc, depth, 1, graph=True)
    wf2, _, d2 = _gpu_fit(nn, sc, depth, 1, graph=False)
    assert np.array_equal(d1["pixel_faces"], d2["pixel_faces"])
    assert np.array_equal(d1["residuals"], d2["residuals"])
    assert rel_err(d1["updates"], d2["updates"]) < 1e-6
    # two iterations (replayed graph vs eager launches)
    wf1, _, d1 = _gpu_fit(nn, sc, depth, 2, graph=True)
    wf2, _, d2 = _gpu_fit(nn, sc, depth, 2, graph=False)
    assert (d1["pixel_faces"] == d2["pixel_faces"]).mean() > 0.999
    assert rel_err(wf1.get_node_translations(), wf2.get_node_translations()) < 1e-4


def test_sequence_graph_and_iterate_from_identity(nn, S, oracle_mod):
    """A mixed-mode run of iterations captured as one graph matches eager launches, and iterate_from_identity(count)
    leaves the state of ONE iteration from the identity warp (every iteration restarts from it)."""
    A, G = nn.alignment, nn.geometry
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    modes = [A.IterationMode.TRANSLATION_ONLY, A.IterationMode.ROTATION_ONLY, A.IterationMode.ALL]
    wf1, _, d1 = _gpu_fit(nn, sc, depth, 3, modes=modes, graph=True)
    wf2, _, d2 = _gpu_fit(nn, sc, depth, 3, modes=modes, graph=False)
    assert (d1["pixel_faces"] == d2["pixel_faces"]).mean() > 0.999
    assert rel_err(wf1.get_node_translations(), wf2.get_node_translations()) < 1e-4
    assert rel_err(wf1.get_node_rotations(), wf2.get_node_rotations()) < 1e-4
    _, _, d_one = _gpu_fit(nn, sc, depth, 1, graph=False)
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                      sc.layer_count)
    ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001, use_hip_graph=2)
    ft.prepare(wf, G.TriangleMesh(sc.points, sc.normals, sc.faces), depth, None, sc.K)
    for count in (3, 5, 3):   # replays of cached graphs of different lengths
        ft.iterate_from_identity(wf, 0, count)
    ft.check()
    dg = ft.diagnostics()
    assert np.array_equal(dg["pixel_faces"], d_one["pixel_faces"])
    assert rel_err(dg["updates"], d_one["updates"]) < 1e-6
    # the identity start is folded into the warp / update kernels on this path (no reset launch): the final state is
    # one iteration's, for every mode, graph-captured or eager
    for mode in (A.IterationMode.ALL, A.IterationMode.TRANSLATION_ONLY, A.IterationMode.ROTATION_ONLY):
        wf_one, _, _ = _gpu_fit(nn, sc, depth, 1, modes=[mode], graph=False)
        for graph in (True, False):
            wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                              sc.layer_count)
            wf.set_node_translations(np.full((len(sc.nodes), 3), 0.5, np.float32))   # overwritten by the identity start
            ft = A.DeformableMeshToImageFitter(1, [mode], preconditioning_dampening_factor=0.001, use_hip_graph=2 if graph else 0)
            ft.prepare(wf, G.TriangleMesh(sc.points, sc.normals, sc.faces), depth, None, sc.K)
            ft.iterate_from_identity(wf, 0, 2)
            ft.check()
            assert rel_err(wf.get_node_translations(), wf_one.get_node_translations()) < 1e-6
            assert rel_err(wf.get_node_rotations() - np.eye(3), wf_one.get_node_rotations() - np.eye(3)) < 1e-6


def test_graph_policy_and_cache_invalidation(nn, S, oracle_mod):
    """use_hip_graph = 1 (auto): a sequence runs eagerly on its first request and is captured from its second; a new
    camera (intrinsics) at the same sizes, or a new warp field (even one reusing the old handle's memory), drops the
    cached graphs, so a reused fitter equals a fresh one (stale camera / warp-field address reuse)."""
    A, G = nn.alignment, nn.geometry
    from dynamicfuion_python_amd import _native as NV
    lib = NV.lib()
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    mesh = G.TriangleMesh(sc.points, sc.normals, sc.faces)

    def new_wf():
        return G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                            sc.layer_count)

    def fresh(K):
        wf = new_wf()
        ft = A.DeformableMeshToImageFitter(2, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001, use_hip_graph=0)
        ft.fit_to_image(wf, mesh, None, depth, None, K, None, 1.0)
        return wf.get_node_translations(), ft.diagnostics()

    ft = A.DeformableMeshToImageFitter(2, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001, use_hip_graph=1)
    wf = new_wf()
    ft.fit_to_image(wf, mesh, None, depth, None, sc.K, None, 1.0)
    assert lib.nnrt_fitter_graph_count(ft._h) == 0          # first request: eager
    t_ref, _ = fresh(sc.K)
    assert np.array_equal(wf.get_node_translations(), t_ref)
    wf.reset_motion()
    ft.fit_to_image(wf, mesh, None, depth, None, sc.K, None, 1.0)
    assert lib.nnrt_fitter_graph_count(ft._h) == 1          # second request: captured + replayed
    assert rel_err(wf.get_node_translations(), t_ref) < 1e-6
    # same sizes, different intrinsics
    K2 = sc.K.copy()
    K2[0, 0] *= 1.05
    K2[1, 2] += 3.0
    wf.reset_motion()
    ft.fit_to_image(wf, mesh, None, depth, None, K2, None, 1.0)
    assert lib.nnrt_fitter_graph_count(ft._h) == 0
    wf.reset_motion()
    ft.fit_to_image(wf, mesh, None, depth, None, K2, None, 1.0)   # captured with the new camera
    t2, d2 = fresh(K2)
    assert rel_err(wf.get_node_translations(), t2) < 1e-6
    assert np.array_equal(ft.diagnostics()["pixel_faces"], d2["pixel_faces"])
    # a new warp field of the same size (the old one destroyed first, so its memory may be reused)
    del wf
    wf = new_wf()
    ft.fit_to_image(wf, mesh, None, depth, None, K2, None, 1.0)
    assert lib.nnrt_fitter_graph_count(ft._h) == 0
    assert rel_err(wf.get_node_translations(), t2) < 1e-6
    # the two launcher switches are part of what a graph bakes in: changing one between frames drops the graphs, the
    # next frame runs the newly chosen kernel and the one after it captures again (same inputs throughout)
    import os
    switches = ("NNRT_RASTER_DENSE", "NNRT_WARP_VERTEX")
    old = {k: os.environ.get(k) for k in switches}
    try:
        for k in switches:
            os.environ.pop(k, None)
        wf.reset_motion()
        ft.fit_to_image(wf, mesh, None, depth, None, K2, None, 1.0)
        assert lib.nnrt_fitter_graph_count(ft._h) == 1
        assert ft.launch_plan()["raster_dense"] == 0 and ft.launch_plan()["warp_vertex"] == 0   # S1's defaults
        for k, choice in zip(switches, ("raster_dense", "warp_vertex")):
            os.environ[k] = "1"
            wf.reset_motion()
            ft.fit_to_image(wf, mesh, None, depth, None, K2, None, 1.0)
            assert lib.nnrt_fitter_graph_count(ft._h) == 0, k
            assert ft.launch_plan()[choice] == 1, k
            wf.reset_motion()
            ft.fit_to_image(wf, mesh, None, depth, None, K2, None, 1.0)
            assert lib.nnrt_fitter_graph_count(ft._h) == 1, k
            assert np.array_equal(ft.diagnostics()["pixel_faces"], d2["pixel_faces"]), k
            assert rel_err(wf.get_node_translations(), t2) < 1e-6, k
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_buffer_move_alone_drops_graphs(nn, S, oracle_mod):
    """A captured graph bakes every buffer's address in. A mesh with a few more (unused) vertices at the same image,
    node and anchor counts makes the per-vertex buffers grow and move: the graphs are dropped, and the reused fitter
    equals a fresh one. This does not isolate the moved-buffer check from the frame key: the vertex count is in the key
    too, and since the fitter's buffers only grow, and every size follows from what the key holds, no sequence of
    prepare() calls moves a buffer without also changing the key. The check per allocation guards the sizes a later
    change might add outside the key; what this test holds is the outcome, that no graph survives a frame whose
    buffers moved."""
    A, G = nn.alignment, nn.geometry
    from dynamicfuion_python_amd import _native as NV
    lib = NV.lib()
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    mesh = G.TriangleMesh(sc.points, sc.normals, sc.faces)
    pad = 5   # vertices no face uses
    points = np.concatenate([sc.points, np.repeat(sc.points[:1], pad, 0)])
    normals = np.concatenate([sc.normals, np.repeat(sc.normals[:1], pad, 0)])
    padded = G.TriangleMesh(points, normals, sc.faces)

    def new_wf():
        return G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                            sc.layer_count)

    ft = A.DeformableMeshToImageFitter(2, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001, use_hip_graph=1)
    wf = new_wf()
    for _ in range(2):   # the second request captures
        wf.reset_motion()
        ft.fit_to_image(wf, mesh, None, depth, None, sc.K, None, 1.0)
    assert lib.nnrt_fitter_graph_count(ft._h) == 1
    wf.reset_motion()
    ft.fit_to_image(wf, padded, None, depth, None, sc.K, None, 1.0)
    assert lib.nnrt_fitter_graph_count(ft._h) == 0
    wf_new = new_wf()
    ft_new = A.DeformableMeshToImageFitter(2, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001, use_hip_graph=0)
    ft_new.fit_to_image(wf_new, padded, None, depth, None, sc.K, None, 1.0)
    dg, dg_new = ft.diagnostics(), ft_new.diagnostics()
    for k in ("pixel_faces", "residual_mask"):
        assert np.array_equal(dg[k], dg_new[k]), k
    # (the second iteration starts from the first one's update, whose fp64 atomics' order differs run to run)
    assert rel_err(wf.get_node_translations(), wf_new.get_node_translations()) < 1e-6


@pytest.mark.parametrize("name", ["S1", "S1_ARAP"])
def test_iterate_from_snapshot(nn, S, oracle_mod, name):
    """iterate_from_snapshot(count): every iteration restarts from the stored (non-identity) node motion, so after any
    count the state equals one iteration from the snapshot -- the benchmark step (general kernels; both the block-diagonal
    and the ARAP path read the snapshot as the iteration's starting state instead of copying it back first)."""
    A, G = nn.alignment, nn.geometry
    sc = _scene(S, oracle_mod, name)
    depth = scene_target(oracle_mod, sc)
    mesh = G.TriangleMesh(sc.points, sc.normals, sc.faces)
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                      sc.layer_count)
    ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001, use_hip_graph=2)
    ft.prepare(wf, mesh, depth, None, sc.K)
    ft.iterate(wf, 0, 1)
    ft.snapshot_motion(wf)
    R1, t1 = wf.get_node_rotations(True), wf.get_node_translations(True)
    ft.iterate(wf, 1, 1)
    R2, t2 = wf.get_node_rotations(True), wf.get_node_translations(True)
    for count in (4, 1, 4):
        ft.iterate_from_snapshot(wf, 1, count)
    ft.check()
    assert rel_err(wf.get_node_translations(True), t2) < 1e-6
    assert rel_err(wf.get_node_rotations(True) - R1, R2 - R1) < 1e-6
    # against the oracle started from the snapshot
    R_o, t_o, _ = oracle_fit_scene(oracle_mod, sc, depth, 1, R0=R1, t0=t1)
    assert rel_err(wf.get_node_translations(True) - t1, t_o - t1) < 1e-4


def test_two_replicas_interleaved_on_two_streams(nn, S, oracle_mod):
    """C4 precondition on one GPU (replicas): two fitters with their own warp fields (seeds 0 and 1) replay
    their graphs interleaved on two streams; each matches its own oracle fit, i.e. buffers, graphs and streams are
    isolated per handle."""
    A, G = nn.alignment, nn.geometry
    reps = []
    for seed in (0, 1):
        sc = _scene(S, oracle_mod, "S1", seed)
        depth = scene_target(oracle_mod, sc)
        st = torch.cuda.Stream()
        wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                          sc.layer_count)
        ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001, use_hip_graph=2)
        ft.prepare(wf, G.TriangleMesh(sc.points, sc.normals, sc.faces), depth, None, sc.K, stream=st)
        ft.snapshot_motion(wf, stream=st)
        reps.append((sc, depth, st, wf, ft))
    assert not np.array_equal(reps[0][0].nodes, reps[1][0].nodes)
    for _ in range(4):
        for sc, depth, st, wf, ft in reps:
            ft.iterate_from_identity(wf, 0, 3, stream=st)   # each iteration restarts at the identity warp
    torch.cuda.synchronize()
    for sc, depth, st, wf, ft in reps:
        ft.check(stream=st)
        _, t_o, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1)
        _compare_iteration(dg_o, ft.diagnostics(stream=st), 6, len(sc.nodes))
        assert rel_err(wf.get_node_translations(True), t_o) < 1e-4
    # whole frame fits (iterations 1..3 from the snapshot = identity) interleaved, each state-synchronised at the end
    for _ in range(2):
        for sc, depth, st, wf, ft in reps:
            ft.fit_from_snapshot(wf, 3, stream=st)
    torch.cuda.synchronize()
    for sc, depth, st, wf, ft in reps:
        ft.check(stream=st)
        R2, t2 = wf.get_node_rotations(True), wf.get_node_translations(True)
        assert np.isfinite(t2).all()
        # the last iteration again from the state before it, alone on the default stream
        ft.restore_motion(wf, stream=st)
        ft.iterate(wf, 0, 2, stream=st)
        torch.cuda.synchronize()
        R1, t1 = wf.get_node_rotations(True), wf.get_node_translations(True)
        _, t_o, _ = oracle_fit_scene(oracle_mod, sc, depth, 1, R0=R1, t0=t1)
        ft.iterate(wf, 2, 1, stream=st)
        torch.cuda.synchronize()
        assert rel_err(wf.get_node_translations(True) - t1, t_o - t1) < 1e-4
        assert rel_err(wf.get_node_translations(True), t2) < 1e-4


def _replica(nn, S, oracle_mod, name, seed, stream, fraction=0.5):
    """A fitter + warp field for scene (name, seed) prepared on `stream`; the block-diagonal path starts from a stored
    mid-motion state (the snapshot, bench.py's step), the ARAP path from the identity."""
    A, G = nn.alignment, nn.geometry
    sc = _scene(S, oracle_mod, name, seed)
    depth = scene_target(oracle_mod, sc)
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                      sc.layer_count)
    R0 = t0 = None
    if sc.layer_count == 1:
        R0, t0 = sc.partial_motion(fraction, seed=seed, noise=1e-3)
        wf.set_node_rotations(R0)
        wf.set_node_translations(t0)
        torch.cuda.synchronize()
    ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001, use_hip_graph=2)
    ft.prepare(wf, G.TriangleMesh(sc.points, sc.normals, sc.faces), depth, None, sc.K, stream=stream)
    ft.snapshot_motion(wf, stream=stream)
    return dict(sc=sc, depth=depth, st=stream, wf=wf, ft=ft, R0=R0, t0=t0)


def _replay(rep, count):
    if rep["R0"] is not None:
        rep["ft"].iterate_from_snapshot(rep["wf"], 1, count, stream=rep["st"])
    else:
        rep["ft"].iterate_from_identity(rep["wf"], 0, count, stream=rep["st"])


def test_c4_eight_c2_replicas_on_eight_streams(nn, S, oracle_mod):
    """C4 (BASELINE.json configs[3]: 8 independent 640x480 sequences, 1500 nodes each; SURVEY 8(e) replicas) -- the
    replicas' workload run on ONE GPU: eight C2 fitters and warp fields (seeds 0-7), each on its own stream, replay their
    hipGraphs interleaved (one GN iteration from a stored mid-motion state, restored before every iteration: bench.py's
    step); each then matches its own oracle iteration from that state: pixel faces exact, H and g <= 1e-6, updates
    <= 1e-4 (DeformableMeshToImageFitter.cpp:111-275)."""
    reps = [_replica(nn, S, oracle_mod, "C2", seed, torch.cuda.Stream()) for seed in range(8)]
    assert len({r["sc"].nodes.tobytes() for r in reps}) == 8
    for _ in range(3):
        for r in reps:
            _replay(r, 4)
    torch.cuda.synchronize()
    for seed, r in enumerate(reps):
        r["ft"].check(stream=r["st"])
        dg = r["ft"].diagnostics(stream=r["st"])
        _, t_o, dg_o = oracle_fit_scene(oracle_mod, r["sc"], r["depth"], 1, R0=r["R0"], t0=r["t0"])
        _compare_iteration(dg_o, dg, 6, len(r["sc"].nodes))
        assert rel_err(r["wf"].get_node_translations(True) - r["t0"], t_o - r["t0"]) < 1e-4, f"replica {seed}"


def test_concurrent_fits_match_solo_runs(nn, S, oracle_mod):
    """No kernel depends on the timing of another workgroup (the Schur-corner factorization in particular: the diagonal
    factor is written to its own array, never over the tile the column's panel workgroups stage): a C5 ARAP fit replayed
    concurrently with a C2 fit, and with a second C5 fit, on separate streams (their workgroups share the CUs) gives the
    result it gives alone -- updates within 1e-6 relative (only the fp64 atomic order of the data term may differ)."""
    c5a = _replica(nn, S, oracle_mod, "C5", 0, torch.cuda.Stream())
    c5b = _replica(nn, S, oracle_mod, "C5", 1, torch.cuda.Stream())
    c2 = _replica(nn, S, oracle_mod, "C2", 0, torch.cuda.Stream())
    solo = {}
    for key, r in (("c5a", c5a), ("c5b", c5b), ("c2", c2)):
        _replay(r, 1)
        torch.cuda.synchronize()
        r["ft"].check(stream=r["st"])
        solo[key] = r["ft"].diagnostics(stream=r["st"])["updates"].copy()
    for pair in ((c5a, c2), (c5a, c5b)):
        for _ in range(6):
            for r in pair:
                _replay(r, 2)
        torch.cuda.synchronize()
        for r in pair:
            r["ft"].check(stream=r["st"])
    for key, r in (("c5a", c5a), ("c5b", c5b), ("c2", c2)):
        u = r["ft"].diagnostics(stream=r["st"])["updates"]
        assert np.isfinite(solo[key]).all()
        assert rel_err(u, solo[key]) < 1e-6, key


def test_iterate_from_identity_with_arap(nn, S, oracle_mod):
    """ARAP path (the reset stays a separate launch there): iterate_from_identity(3) == one iteration."""
    A, G = nn.alignment, nn.geometry
    sc = _scene(S, oracle_mod, "C1_ARAP")
    depth = scene_target(oracle_mod, sc)
    wf_one, _, _ = _gpu_fit(nn, sc, depth, 1)
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                      sc.layer_count)
    ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001)
    ft.prepare(wf, G.TriangleMesh(sc.points, sc.normals, sc.faces), depth, None, sc.K)
    ft.iterate_from_identity(wf, 0, 3)
    ft.check()
    assert rel_err(wf.get_node_translations(), wf_one.get_node_translations()) < 1e-4


def test_fit_with_extrinsics_parity(nn, S, oracle_mod):
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    E = np.eye(4)
    E[:3, 3] = [0.002, -0.001, 0.003]
    _, _, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1, extrinsics=E)
    _, _, dg_g = _gpu_fit(nn, sc, depth, 1, extrinsics=E)
    _compare_iteration(dg_o, dg_g, 6, len(sc.nodes))


def _plane25_scene(oracle_mod):
    """cpp/tests/test_deformable_mesh_fitter_advanced.cpp:55-128: the 25-node plane meshes and nodes flipped about y and
    moved 1.2 away from the camera, the target rendered at 100 x 100, its depth unprojected; plus the shipped ground-truth
    node motion (:116-120, node_{translations,rotations}_25-node_plane.npy) carried into that frame (t' = F t,
    R' = F R F with F = diag(-1, 1, -1)): it warps the source mesh onto the target to 2.4e-7."""
    T = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 1.2], [0, 0, 0, 1.]])
    Ps, Ns, Fs = read_ply(os.path.join(FIXTURES, "plane_skin_25_nodes_source.ply"))
    Pt, Nt, Ft = read_ply(os.path.join(FIXTURES, "plane_skin_25_nodes_target.ply"))
    Ps, Ns = transform_mesh(Ps, Ns, T)
    Pt, Nt = transform_mesh(Pt, Nt, T)
    nodes = np.load(os.path.join(FIXTURES, "nodes_25-node_plane.npy")).astype(np.float32)
    nodes = (nodes.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    F = np.diag([-1.0, 1.0, -1.0])
    t_gt = np.load(os.path.join(FIXTURES, "node_translations_25-node_plane.npy")).astype(np.float64) @ F.T
    R_gt = F @ np.load(os.path.join(FIXTURES, "node_rotations_25-node_plane.npy")).astype(np.float64) @ F
    K = np.array([[100.0, 0, 50], [0, 100.0, 50], [0, 0, 1]])
    fndc, fm = oracle_mod.extract_face_ndc(Pt, Ft, K, 100, 100, 0.0, 10.0)
    fi, dep, _, _ = oracle_mod.rasterize(fndc, fm, 100, 100, 0.0, 1, -1, -1, True, False, True)
    depth = np.where(dep[..., 0] > 0, dep[..., 0], 0).astype(np.float32)
    refp, refm = oracle_mod.unproject(depth, K, 1.0, 10.0)
    weights = oracle_mod.node_coverage_weights(nodes, 0.1)
    return SimpleNamespace(Ps=Ps, Ns=Ns, Fs=Fs, Pt=Pt, Ft=Ft, nodes=nodes, K=K, fndc=fndc, fm=fm, fi=fi, dep=dep, depth=depth,
                           refp=refp, refm=refm, weights=weights, t_gt=t_gt, R_gt=R_gt)


def _plane25_fitter(nn, p, iterations):
    G, A = nn.geometry, nn.alignment
    wf = G.HierarchicalGraphWarpField(p.nodes, 0.1, False, 4, 0, G.WarpNodeCoverageComputationMethod.MINIMAL_K_NEIGHBOR_NODE_DISTANCE, 1)
    assert np.array_equal(wf.get_node_coverage_weights(), p.weights)
    ft = A.DeformableMeshToImageFitter(iterations, [A.IterationMode.ALL], 1e-6, True, 10.0, False, 0.01, 0.001)
    return wf, ft


def _plane25_oracle_iteration(oracle_mod, p, R0, t0):
    return oracle_mod.fit(nodes=p.nodes, rotations=R0, translations=t0, mesh_points=p.Ps, mesh_normals=p.Ns, faces=p.Fs,
                          ref_points=p.refp, ref_mask=p.refm, H=100, W=100, K=p.K, max_iterations=1, lm_factor=0.001, coverage=0.1,
                          coverage_method=1, node_weights=p.weights)


def test_25_node_plane_fixture_parity(nn, oracle_mod):
    # cpp/tests/test_deformable_mesh_fitter_advanced.cpp:55-143 scene (parity of the first iteration GPU vs oracle)
    p = _plane25_scene(oracle_mod)
    fi_g, dep_g, _, _ = nn.rendering.rasterize_ndc_triangles(p.fndc, p.fm, (100, 100), 0.0, 1, -1, -1, True, False, True)
    assert np.array_equal(p.fi, _np(fi_g)) and np.array_equal(p.dep, _np(dep_g))
    I = np.tile(np.eye(3, dtype=np.float32), (25, 1, 1))
    R_o, t_o, dg_o = _plane25_oracle_iteration(oracle_mod, p, I, np.zeros((25, 3), np.float32))
    wf, ft = _plane25_fitter(nn, p, 1)
    ft.fit_to_image(wf, nn.geometry.TriangleMesh(p.Ps, p.Ns, p.Fs), None, p.depth, p.depth > 0, p.K, np.eye(4), 1.0)
    _compare_iteration(dg_o, ft.diagnostics(), 6, 25)


def test_25_node_plane_distance_to_ground_truth(nn, oracle_mod):
    """the fit against the reference's own ground-truth motion for its 25-node plane scene
    (test_deformable_mesh_fitter_advanced.cpp:116-120; the reference test asserts nothing, :140-142). Three GN iterations
    on the GPU from the identity; each is checked against the oracle iteration started from the GPU's motion, and the
    distance of the node motion from the ground truth (mean |t - t_gt|, max |R - R_gt|, mean warped-vertex distance from
    the target mesh) is recorded for both. The reference algorithm (block-diagonal data term, A17) does not approach its
    own ground truth on this scene: from 0.092 (mean translation distance at the identity) it moves to 0.25 and 0.78 (the
    reference notes its fit misbehaving at iteration 2, :135). So what is pinned is what the oracle achieves: per
    iteration the GPU's distances equal the oracle's (1e-3 relative), and they grow or shrink where the oracle's do."""
    p = _plane25_scene(oracle_mod)
    wf, ft = _plane25_fitter(nn, p, 3)
    ft.prepare(wf, nn.geometry.TriangleMesh(p.Ps, p.Ns, p.Fs), p.depth, p.depth > 0, p.K, np.eye(4), 1.0)
    a, w = oracle_mod.compute_anchors(p.Ps, p.nodes, 4, 0.1, node_weights=p.weights)

    def dist(R, t):
        R, t = np.asarray(R, np.float32).reshape(25, 3, 3), np.asarray(t, np.float32).reshape(25, 3)
        Pw, _ = oracle_mod.warp_mesh(p.Ps, p.Ns, p.nodes, R, t, a, w)
        return (float(np.linalg.norm(t - p.t_gt, axis=1).mean()), float(np.abs(R - p.R_gt).max()),
                float(np.linalg.norm(Pw - p.Pt, axis=1).mean()))

    d0 = dist(np.tile(np.eye(3, dtype=np.float32), (25, 1, 1)), np.zeros((25, 3), np.float32))
    rows_g, rows_o = [d0], [d0]
    for k in range(3):
        R0, t0 = wf.get_node_rotations(True), wf.get_node_translations(True)
        ft.iterate(wf, k, 1)
        ft.check()
        R_o, t_o, dg_o = _plane25_oracle_iteration(oracle_mod, p, R0, t0)
        _compare_iteration(dg_o, ft.diagnostics(), 6, 25)
        dg_, do_ = dist(wf.get_node_rotations(True), wf.get_node_translations(True)), dist(R_o, t_o)
        print(f"25-node plane iteration {k + 1}: distance to GT (mean |t - t_gt|, max |R - R_gt|, mean vertex) GPU {dg_}, "
              f"oracle {do_}", flush=True)
        for x, y in zip(dg_, do_):   # the updates agree to 1e-4 (_compare_iteration); distances derived from them to 1e-3
            assert abs(x - y) <= 1e-3 * max(abs(y), 1e-3)
        rows_g.append(dg_)
        rows_o.append(do_)
    for k in range(1, len(rows_g)):
        for c in range(3):
            assert (rows_g[k][c] > rows_g[k - 1][c]) == (rows_o[k][c] > rows_o[k - 1][c]), (k, c, rows_g, rows_o)
    assert abs(rows_o[0][0] - 0.0917) < 1e-3 and rows_o[1][0] > rows_o[0][0]   # the reference's fit moves away from its GT


# ---------------------------------------------------------------------------------------------------------------------
# full-size properties and error behaviour
# ---------------------------------------------------------------------------------------------------------------------
def test_c3_raster_parity_and_iteration_properties(nn, S, oracle_mod):
    sc = _scene(S, oracle_mod, "C3")
    _, _, fndc, fm = _warped_face_ndc(oracle_mod, sc)
    ref = oracle_mod.rasterize_k1_fast(fndc, fm, sc.H, sc.W, 0.5, True, True)
    got = nn.rendering.rasterize_ndc_triangles(fndc, fm, (sc.H, sc.W), 0.5, 1, -1, -1, True, False, True)
    for r, g in zip(ref, got):
        assert np.array_equal(r, _np(g))
    depth = np.where(ref[1][..., 0] > 0, ref[1][..., 0], 0).astype(np.float32)
    wf, ft, dg = _gpu_fit(nn, sc, depth, 1)
    N = len(sc.nodes)
    Hb = dg["hessian"].reshape(N, 6, 6)
    assert np.allclose(Hb, Hb.transpose(0, 2, 1))
    assert (np.linalg.eigvalsh(Hb.astype(np.float64)) > -1e-3 * np.abs(Hb).max()).all()
    assert np.array_equal(dg["residual_mask"], (dg["pixel_faces"] >= 0) & (depth.reshape(-1) > 0))
    assert np.isfinite(dg["updates"]).all()
    # the full GN iteration against the oracle at 1280x960 / 4.5 M triangles / 3000 nodes (DeformableMeshToImageFitter.cpp:
    # 111-275): pixel faces exact, residuals, H and g <= 1e-6, updates <= 1e-4
    R_o, t_o, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1)
    _compare_iteration(dg_o, dg, 6, N)
    assert rel_err(wf.get_node_translations(True), t_o) < 1e-4
    assert rel_err(wf.get_node_rotations(True) - np.eye(3), R_o - np.eye(3)) < 1e-4
    # SURVEY 8(d) C3's parity condition (A4, PixelVertexAnchorJacobiansImpl.h:33, :348-358): no node's pixel list reaches
    # the reference's 4000-entry cap, so its capped lists hold the same associations as the uncapped math here
    a, _ = ft.anchors(len(sc.points), 4)
    sel = dg["residual_mask"] & (dg["pixel_faces"] >= 0)
    fn = np.sort(a[sc.faces[dg["pixel_faces"][sel].astype(np.int64)]].reshape(int(sel.sum()), -1), axis=1)
    uniq = (fn >= 0) & np.concatenate([np.ones((len(fn), 1), bool), fn[:, 1:] != fn[:, :-1]], axis=1)
    per_node = np.bincount(fn[uniq], minlength=N)
    print(f"C3: {int(sel.sum())} residual pixels, {int(uniq.sum())} associations, max pixels per node {per_node.max()}")
    assert per_node.max() <= 3999


@pytest.mark.parametrize("name", ["C2", "S1"])
def test_pixel_tile_order_same_iteration(nn, S, oracle_mod, name):
    """The pixel launch's per-frame tile order (tiles without reference pixels dealt to each XCD band's end; on by default
    beyond one residency round, forced here with NNRT_TILE_ORDER=2) changes which workgroup runs which tile, not the
    iteration: pixel faces, masks and residuals identical, H and g within the fp64 summation order (1e-6), updates 1e-5,
    against the arithmetic XCD bands (NNRT_TILE_ORDER=0)."""
    import os
    sc = _scene(S, oracle_mod, name)
    depth = scene_target(oracle_mod, sc)
    N = len(sc.nodes)
    old = os.environ.get("NNRT_TILE_ORDER")
    out = {}
    try:
        for v in ("2", "0"):
            os.environ["NNRT_TILE_ORDER"] = v
            _, ft, dg = _gpu_fit(nn, sc, depth, 1)
            assert ft.launch_plan()["tile_order"] == (1 if v == "2" else 0), "the forced path is not the one that ran"
            out[v] = dg
    finally:
        if old is None:
            os.environ.pop("NNRT_TILE_ORDER", None)
        else:
            os.environ["NNRT_TILE_ORDER"] = old
    a, b = out["2"], out["0"]
    assert np.array_equal(a["pixel_faces"], b["pixel_faces"]) and np.array_equal(a["residual_mask"], b["residual_mask"])
    assert np.array_equal(a["residuals"], b["residuals"])
    assert rel_err(a["hessian"][: 36 * N], b["hessian"][: 36 * N]) < 1e-6
    assert rel_err(a["gradient"][: 6 * N], b["gradient"][: 6 * N]) < 1e-6
    assert nan_rel_err(a["updates"][: 6 * N], b["updates"][: 6 * N]) < 1e-5


@pytest.mark.parametrize("name", ["S1", "C2"])
def test_raster_dense_path_same_iteration(nn, S, oracle_mod, name):
    """The dense-mesh scatter (one face per lane, 64 per wave; the default when a mesh has at least as many faces as the
    image has pixels, e.g. C3) and the lane-pair scatter (C1 / C2) perform the same per-face operations into the same
    keyed minimum: forced on (NNRT_RASTER_DENSE=1) and off (=0) on sparser scenes, the rasterization is bit-identical (faces,
    masks, residuals) and the data term equal to its fp64 summation order."""
    import os
    sc = _scene(S, oracle_mod, name)
    depth = scene_target(oracle_mod, sc)
    N = len(sc.nodes)
    old = os.environ.get("NNRT_RASTER_DENSE")
    out = {}
    try:
        for v in ("1", "0"):
            os.environ["NNRT_RASTER_DENSE"] = v
            _, ft, dg = _gpu_fit(nn, sc, depth, 1)
            assert ft.launch_plan()["raster_dense"] == (int(v)), "the forced path is not the one that ran"
            out[v] = dg
    finally:
        if old is None:
            os.environ.pop("NNRT_RASTER_DENSE", None)
        else:
            os.environ["NNRT_RASTER_DENSE"] = old
    a, b = out["1"], out["0"]
    assert (a["pixel_faces"] >= 0).sum() > 1000
    for k in ("pixel_faces", "residual_mask", "residuals"):
        assert np.array_equal(a[k], b[k]), k
    # (H and g: the fp64 atomics' order differs run to run, as in test_pixel_tile_order_same_iteration)
    assert rel_err(a["hessian"][: 36 * N], b["hessian"][: 36 * N]) < 1e-6
    assert rel_err(a["gradient"][: 6 * N], b["gradient"][: 6 * N]) < 1e-6
    assert nan_rel_err(a["updates"][: 6 * N], b["updates"][: 6 * N]) < 1e-5


@pytest.mark.parametrize("name", ["S1", "C2"])
def test_pixel_launch_builds_same_iteration(nn, S, oracle_mod, name):
    """The pixel launch's two builds -- 5 waves per SIMD with the per-pixel records in memory (one-round launches, C2) and
    4 waves per SIMD with each record kept in its pixel lane's registers and read by cross-lane shuffles (launches of
    several residency rounds, C3) -- transport the same record floats: forced (NNRT_PIX_WPE4=1 / 0) on the same scene,
    the residuals are bit-identical and the data term equal up to its fp64 atomics' order."""
    import os
    sc = _scene(S, oracle_mod, name)
    depth = scene_target(oracle_mod, sc)
    N = len(sc.nodes)
    old = os.environ.get("NNRT_PIX_WPE4")
    out = {}
    try:
        for v in ("1", "0"):
            os.environ["NNRT_PIX_WPE4"] = v
            _, ft, dg = _gpu_fit(nn, sc, depth, 1)
            assert ft.launch_plan()["pix_low_occupancy"] == (int(v)), "the forced path is not the one that ran"
            out[v] = dg
    finally:
        if old is None:
            os.environ.pop("NNRT_PIX_WPE4", None)
        else:
            os.environ["NNRT_PIX_WPE4"] = old
    a, b = out["1"], out["0"]
    assert (a["pixel_faces"] >= 0).sum() > 500
    for k in ("pixel_faces", "residual_mask", "residuals"):
        assert np.array_equal(a[k], b[k]), k
    assert rel_err(a["hessian"][: 36 * N], b["hessian"][: 36 * N]) < 1e-6
    assert rel_err(a["gradient"][: 6 * N], b["gradient"][: 6 * N]) < 1e-6
    assert nan_rel_err(a["updates"][: 6 * N], b["updates"][: 6 * N]) < 1e-5


def test_errors_fail_loudly(nn, S, oracle_mod):
    A, G = nn.alignment, nn.geometry
    with pytest.raises(RuntimeError):
        A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=2.0)
    with pytest.raises(RuntimeError):
        G.HierarchicalGraphWarpField(np.zeros((2, 3), np.float32), 0.1, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, 1)
    # a node far from the mesh gets no pixels: with LM = 0 its 6x6 block is zero -> potrf failure (reference raises)
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    sc.nodes = np.concatenate([sc.nodes, np.array([[5.0, 5.0, 5.0]], np.float32)])
    with pytest.raises(RuntimeError, match="positive-definite"):
        _gpu_fit(nn, sc, depth, 1, lm=0.0)
    # a triangle index outside the vertex array is rejected (validated on the device, nothing gathered out of bounds)
    sc = _scene(S, oracle_mod, "S1")
    sc.faces = np.concatenate([sc.faces, np.array([[0, 1, len(sc.points)]], sc.faces.dtype)])
    with pytest.raises(RuntimeError, match="index out of range"):
        _gpu_fit(nn, sc, depth, 1, lm=0.001)


def test_fit_point_cloud_overload_parity(nn, S, oracle_mod):
    """FitToImage(warp_field, mesh, color, reference_point_cloud, mask, K, E, rendering_image_size)
    (DeformableMeshToImageFitter.cpp:85-276) with a reference cloud that is NOT an unprojected depth image."""
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    refp, refm = oracle_mod.unproject(depth, sc.K, 1.0, 10.0)
    rng = np.random.default_rng(3)
    pts = (refp + rng.normal(scale=1e-3, size=refp.shape)).astype(np.float32)
    mask = (refm.astype(bool) & (rng.random(len(refm)) > 0.1)).astype(np.uint8)
    N = len(sc.nodes)
    R_o, t_o, dg_o = oracle_mod.fit(nodes=sc.nodes, rotations=np.tile(np.eye(3, dtype=np.float32), (N, 1, 1)),
                                    translations=np.zeros((N, 3), np.float32), mesh_points=sc.points, mesh_normals=sc.normals,
                                    faces=sc.faces, ref_points=pts, ref_mask=mask, H=sc.H, W=sc.W, K=sc.K, max_iterations=1,
                                    lm_factor=0.001, coverage=sc.coverage)
    G, A = nn.geometry, nn.alignment
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, 1)
    ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001)
    ft.fit_to_image(wf, G.TriangleMesh(sc.points, sc.normals, sc.faces), None, pts, mask, sc.K, None, (sc.H, sc.W))
    _compare_iteration(dg_o, ft.diagnostics(), 6, N)
    assert rel_err(wf.get_node_translations(True), t_o) < 1e-4


def test_fit_rgbd_overload_matches_depth_overload(nn, S, oracle_mod):
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    G, A = nn.geometry, nn.alignment
    mesh = G.TriangleMesh(sc.points, sc.normals, sc.faces)
    out = []
    for use_rgbd in (False, True):
        wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, 1)
        ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001)
        if use_rgbd:
            ft.fit_to_image(wf, mesh, G.RGBDImage(None, depth * 1000.0), None, sc.K, None, 1000.0)
        else:
            ft.fit_to_image(wf, mesh, None, depth, None, sc.K, None, 1.0)
        out.append(ft.diagnostics())
    assert np.array_equal(out[0]["pixel_faces"], out[1]["pixel_faces"])
    assert rel_err(out[1]["updates"], out[0]["updates"]) < 1e-4


def test_rendering_alignment_optimizer_slot(nn, S, oracle_mod):
    """alignment.render_based.RenderingAlignmentOptimizer.optimize_graph over the fitter (point-cloud overload)."""
    from dynamicfuion_python_amd.alignment.render_based import (PenaltyFunction, RenderingAlignmentOptimizer,
                                                                 RenderingAlignmentParameters)
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    refp, refm = oracle_mod.unproject(depth, sc.K, 1.0, 10.0)
    N = len(sc.nodes)
    _, t_o, dg_o = oracle_mod.fit(nodes=sc.nodes, rotations=np.tile(np.eye(3, dtype=np.float32), (N, 1, 1)),
                                  translations=np.zeros((N, 3), np.float32), mesh_points=sc.points, mesh_normals=sc.normals,
                                  faces=sc.faces, ref_points=refp, ref_mask=refm, H=sc.H, W=sc.W, K=sc.K, max_iterations=1,
                                  lm_factor=0.001, coverage=sc.coverage)
    G = nn.geometry
    graph = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, 1)
    params = RenderingAlignmentParameters(data_term_penalty_function=PenaltyFunction.SQUARE, max_iteration_count=1)
    opt = RenderingAlignmentOptimizer((sc.H, sc.W), None, sc.K, params)
    pts = np.where(refm[:, None].astype(bool), refp, 0).reshape(sc.H, sc.W, 3)
    opt.optimize_graph(graph, G.TriangleMesh(sc.points, sc.normals, sc.faces), pts, None)
    assert rel_err(graph.get_node_translations(True), t_o) < 1e-4


def test_graph_warp_field_warp_mesh(nn, S, oracle_mod):
    """GraphWarpField.warp_mesh (cpp/pybind/geometry/geometry.cpp:293-302): anchors over the field's nodes + blend warp."""
    sc = _scene(S, oracle_mod, "S1")
    G = nn.geometry
    wf = G.GraphWarpField(sc.nodes, sc.coverage, False, 4, 0)
    wf.set_node_rotations(sc.gt_rotations)
    wf.set_node_translations(sc.gt_translations)
    out = wf.warp_mesh(G.TriangleMesh(sc.points, sc.normals, sc.faces))
    a, w = oracle_mod.compute_anchors(sc.points, sc.nodes, 4, sc.coverage)
    wp, wn = oracle_mod.warp_mesh(sc.points, sc.normals, sc.nodes, sc.gt_rotations, sc.gt_translations, a, w)
    assert np.array_equal(_np(out.vertex_positions), wp)
    assert np.array_equal(_np(out.vertex_normals), wn)
    assert np.allclose(wf.get_warped_nodes(), sc.nodes + sc.gt_translations)
    wf.reset_rotations()
    assert np.array_equal(wf.get_node_rotations(), np.tile(np.eye(3, dtype=np.float32), (len(sc.nodes), 1, 1)))
    assert np.array_equal(wf.get_node_translations(), sc.gt_translations)


@pytest.mark.parametrize("name", ["S1", "C1"])
def test_normals_bit_exact(nn, S, oracle_mod, name):
    """compute_triangle_normals / compute_vertex_normals / compute_ordered_point_cloud_normals (NormalsOperationsImpl.h)
    against the oracle restatement: identical bits (vertex sums in ascending face order on both sides)."""
    sc = _scene(S, oracle_mod, name)
    G = nn.geometry
    mesh = G.TriangleMesh(sc.points, None, sc.faces)
    for normalized in (False, True):
        tn = _np(G.functional.compute_triangle_normals(mesh, normalized))
        assert np.array_equal(tn, oracle_mod.triangle_normals(sc.points, sc.faces, normalized))
        vn = _np(G.functional.compute_vertex_normals(mesh, normalized))
        assert np.array_equal(vn, oracle_mod.vertex_normals(sc.points, sc.faces, normalized))
    assert np.array_equal(_np(mesh.vertex_normals), vn)
    depth = scene_target(oracle_mod, sc)
    pts, _ = nn.geometry.functional.unproject_raster_depth_without_filtering(depth, sc.K, depth_scale=1.0, depth_max=10.0)
    on = _np(G.functional.compute_ordered_point_cloud_normals(pts, (sc.H, sc.W)))
    assert np.array_equal(on, oracle_mod.ordered_point_cloud_normals(_np(pts), sc.H, sc.W))
    with pytest.raises(RuntimeError):
        G.functional.compute_ordered_point_cloud_normals(pts[:-1], (sc.H, sc.W))
    bad = G.TriangleMesh(sc.points, None, np.array([[0, 1, len(sc.points)]], np.int64))
    with pytest.raises(RuntimeError):
        G.functional.compute_vertex_normals(bad)
    with pytest.raises(RuntimeError):
        G.functional.compute_triangle_normals(bad)
    # the library stays usable after a rejected call (nothing gathered outside the vertex array)
    assert np.array_equal(_np(G.functional.compute_triangle_normals(mesh, True)), oracle_mod.triangle_normals(sc.points, sc.faces, True))


# ---- warp-field construction on the GPU (hierarchy.hip): medoid subsampling, K-NN edges, coverage weights ------------

def test_hierarchy_kat_gpu(nn):
    """cpp/tests/test_graph_warp_field.cpp:30-340 through the device construction (3 layers, radii 0.25/0.5/1.0)."""
    G = nn.geometry
    wf = G.HierarchicalGraphWarpField(L.HIERARCHY_NODES, 0.25, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, 3, 4,
                                      [0.25, 0.5, 1.0])
    vidx, edges = wf.get_virtual_node_indices(), wf.get_edges()
    assert list(wf.get_layer_node_counts()) == [19, 10, 4]
    assert sorted(vidx[:19].tolist()) == L.HIERARCHY_LAYER0
    assert sorted(vidx[19:29].tolist()) == L.HIERARCHY_LAYER1
    assert sorted(vidx[29:].tolist()) == L.HIERARCHY_LAYER2
    assert edges[:, 0].tolist() == L.HIERARCHY_EDGE_SOURCES
    assert sorted((int(vidx[i]), int(vidx[j])) for i, j in edges) == sorted(L.HIERARCHY_EDGES_ORIGINAL)


def _grid_nodes(n, seed, jitter=1e-3):
    rng = np.random.default_rng(seed)
    side = int(np.sqrt(n))
    i = np.arange(n)
    nodes = np.stack([(i % side) * 0.025 + rng.uniform(-jitter, jitter, n), (i // side) * 0.025, 1.5 + 0.01 * rng.uniform(-1, 1, n)], 1)
    return nodes.astype(np.float32)


@pytest.mark.parametrize("n,layers,degree,kind", [(1500, 2, 4, "grid"), (5000, 2, 4, "grid"), (3000, 4, 4, "random"),
                                                   (2000, 3, 6, "random"), (700, 2, 1, "duplicates")])
def test_hierarchy_and_coverage_bit_exact(nn, oracle_mod, n, layers, degree, kind):
    """Device construction == the sequential restatement: layer membership, virtual order, edges, edge layers, coverage
    weights (exact float equality: same per-cell summation order, correctly rounded sqrt)."""
    if kind == "grid":
        nodes = _grid_nodes(n, 1)
    elif kind == "random":
        nodes = np.random.default_rng(n).uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    else:   # exact duplicates and equal distances: medoid ties and K-NN ties resolved by index
        base = np.random.default_rng(3).integers(0, 6, (n // 2, 3)).astype(np.float32) * 0.04
        nodes = np.concatenate([base, base])
    coverage = 0.03 if kind == "grid" else 0.05
    G = nn.geometry
    vidx_o, counts_o, edges_o, el_o = oracle_mod.build_hierarchy(nodes, coverage, layers, degree)
    wf = G.HierarchicalGraphWarpField(nodes, coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.MINIMAL_K_NEIGHBOR_NODE_DISTANCE, layers,
                                      degree)
    assert np.array_equal(wf.get_layer_node_counts(), counts_o)
    assert np.array_equal(wf.get_virtual_node_indices(), vidx_o)
    assert np.array_equal(wf.get_edges(), edges_o)
    assert np.array_equal(wf.get_edge_layer_indices(), el_o)
    w_o = oracle_mod.node_coverage_weights(nodes, coverage)
    assert np.array_equal(wf.get_node_coverage_weights(), w_o[vidx_o])


def test_dlpack_fit_matches_pointer_fit(nn, S, oracle_mod):
    """include/nnrt_dlpack.h: torch-ROCm tensors lent through DLPack run the same fit as the pointer entry point (same
    kernels, same inputs -> identical node motion); device / dtype mismatches are argument errors."""
    import ctypes
    from dynamicfuion_python_amd import _native
    sc = _scene(S, oracle_mod, "S1")
    depth = scene_target(oracle_mod, sc)
    wf_p, _, _ = _gpu_fit(nn, sc, depth, 2, graph=False)
    G, A = nn.geometry, nn.alignment
    lib = _native.lib()
    h = ctypes.c_void_p()
    caps = []

    def dl(x):
        cap, ptr = _native.dlpack(x)
        caps.append(cap)
        return ptr

    nodes_dev = torch.as_tensor(sc.nodes, device="cuda")
    assert lib.nnrt_warp_field_create_dlpack(dl(nodes_dev), sc.coverage, 0, 4, 0, 0, sc.layer_count, 4, None, 0, ctypes.byref(h)) == 0
    wf_d = G.HierarchicalGraphWarpField.__new__(G.HierarchicalGraphWarpField)
    wf_d._h, wf_d.device, wf_d.node_count, wf_d.anchor_count = h, 0, len(sc.nodes), 4
    ft = A.DeformableMeshToImageFitter(2, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001, use_hip_graph=False)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    verts, nrms, faces = dev(sc.points.astype(np.float32)), dev(sc.normals.astype(np.float32)), dev(sc.faces.astype(np.int64))
    dep = dev(depth.astype(np.float32))
    K, E = np.ascontiguousarray(sc.K, np.float64), np.eye(4)
    st = lib.nnrt_fitter_fit_to_image_dlpack(ft._h, h, dl(verts), dl(nrms), dl(faces), dl(dep), None, dl(K), dl(E), 1.0, None)
    assert st == 0, lib.nnrt_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(wf_d.get_node_translations(True), wf_p.get_node_translations(True))
    assert np.array_equal(wf_d.get_node_rotations(True), wf_p.get_node_rotations(True))
    # mismatches: int32 faces, host-resident vertices
    st = lib.nnrt_fitter_fit_to_image_dlpack(ft._h, h, dl(verts), dl(nrms), dl(faces.to(torch.int32)), dl(dep), None, dl(K), dl(E), 1.0, None)
    assert st == 1 and b"faces: unsupported dtype" in lib.nnrt_last_error()
    st = lib.nnrt_fitter_fit_to_image_dlpack(ft._h, h, dl(verts.cpu()), dl(nrms), dl(faces), dl(dep), None, dl(K), dl(E), 1.0, None)
    assert st == 1 and b"vertices: must be a ROCm device tensor" in lib.nnrt_last_error()


@pytest.mark.parametrize("kf", [1, 4])
def test_dlpack_rasterize_matches_binding(nn, oracle_mod, kf):
    """nnrt_rasterize_ndc_triangles_dlpack writes the same fragments as nnrt.rendering.rasterize_ndc_triangles."""
    from dynamicfuion_python_amd import _native
    T = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 1.2], [0, 0, 0, 1.]])
    Pt, _, Ft = read_ply(os.path.join(FIXTURES, "plane_skin_25_nodes_target.ply"))
    Pt = (Pt.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    K = np.array([[100.0, 0, 50], [0, 100.0, 50], [0, 0, 1]])
    fndc, fm = oracle_mod.extract_face_ndc(Pt, Ft, K, 100, 100, 0.0, 10.0)
    ref = nn.rendering.rasterize_ndc_triangles(fndc, fm, (100, 100), 0.5, kf, -1, -1, True, False, True)
    nd, md = torch.as_tensor(fndc, device="cuda"), torch.as_tensor(fm.astype(np.bool_), device="cuda")
    out = [torch.empty((100, 100, kf), dtype=torch.int64, device="cuda"), torch.empty((100, 100, kf), device="cuda"),
           torch.empty((100, 100, kf, 3), device="cuda"), torch.empty((100, 100, kf), device="cuda")]
    caps = [_native.dlpack(x) for x in [nd, md] + out]
    lib = _native.lib()
    st = lib.nnrt_rasterize_ndc_triangles_dlpack(caps[0][1], caps[1][1], 0.5, 1, 0, 1, *[c[1] for c in caps[2:]], None)
    assert st == 0, lib.nnrt_last_error()
    torch.cuda.synchronize()
    for a, b in zip(out, ref):
        assert np.array_equal(_np(a), _np(b))
    bad = _native.dlpack(torch.empty((100, 100, kf, 2), device="cuda"))   # barycentrics with 2 components
    st = lib.nnrt_rasterize_ndc_triangles_dlpack(caps[0][1], caps[1][1], 0.5, 1, 0, 1, caps[2][1], caps[3][1], bad[1], caps[5][1], None)
    assert st == 1 and b"barycentrics: dimension 3 is 2, expected 3" in lib.nnrt_last_error()
