"""The rasterizer and the fused GN iteration at portrait, odd and thin image sizes, against the CPU oracle.

The rest of the suite reaches csrc/raster.hip and the fused pixel launch at square or 4:3 landscape sizes only, all but
one a multiple of 16 on both axes. Here: H > W (min(H, W) is W, both ndc_range branches swap), a partial last tile
column and row at once, images thinner than a 16 x 16 tile or with a one-pixel last tile row, and the K > 1 hit lists
at all of these. Inputs: _raster_shape_util.shape_soup / shape_scene; tests/test_raster_shapes_cpu.py shows on the CPU
that every (size, options) set below reaches the scatter's three row modes, staged and unstaged waves, a row deal of
several rounds and every rejection cause. Tolerances: the rasterizer bit-exact; the iteration exactly as
test_gpu_parity._compare_iteration (faces and masks identical, residuals 1e-6 absolute, H and g 1e-6, updates 1e-4).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from _raster_shape_util import FIT_SHAPES, RASTER_OPTIONS, RASTER_SIZES, shape_scene, shape_soup  # noqa: E402
from _util import oracle_fit_scene, rel_err, scene_target  # noqa: E402
from test_gpu_parity import _compare_iteration, _gpu_fit, _new_fit, _np, nan_rel_err  # noqa: E402


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import _native
    _native.lib()
    from dynamicfuion_python_amd import nnrt
    return nnrt


_SOUPS = {}


def _soup(H, W):
    if (H, W) not in _SOUPS:
        _SOUPS[(H, W)] = shape_soup(H, W)   # shared, never written
    return _SOUPS[(H, W)]


def _same(ref, got, what):
    for name, r, g in zip(("faces", "depths", "barycentrics", "distances"), ref, got):
        g = _np(g)
        assert r.shape == g.shape, f"{what}: {name} shape {g.shape}, oracle {r.shape}"
        if not np.array_equal(r, g):
            bad = np.argwhere(~((r == g) | (np.isnan(r) & np.isnan(g))))
            raise AssertionError(f"{what}: {len(bad)} {name} differ, e.g. at {bad[:4].tolist()}: oracle {r[tuple(bad[0])]}, GPU {g[tuple(bad[0])]}")


# ---------------------------------------------------------------------------------------------------------------------
# standalone rasterizer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blur,persp,clip", RASTER_OPTIONS)
@pytest.mark.parametrize("H,W", RASTER_SIZES)
def test_rasterize_k1_shapes_bit_exact(nn, oracle_mod, H, W, blur, persp, clip):
    f, m = _soup(H, W)
    ref = oracle_mod.rasterize(f, m, H, W, blur, 1, -1, -1, persp, clip, True)
    got = nn.rendering.rasterize_ndc_triangles(f, m, (H, W), blur, 1, -1, -1, persp, clip, True)
    _same(ref, got, f"{H}x{W} K=1 blur {blur}")
    assert (ref[0] >= 0).mean() >= 0.25


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("H,W", RASTER_SIZES)
def test_rasterize_multi_face_shapes_bit_exact(nn, oracle_mod, H, W, k):
    f, m = _soup(H, W)
    ref = oracle_mod.rasterize(f, m, H, W, 0.5, k, -1, -1, True, False, True)
    got = nn.rendering.rasterize_ndc_triangles(f, m, (H, W), 0.5, k, -1, -1, True, False, True)
    _same(ref, got, f"{H}x{W} K={k}")
    assert (ref[0][..., k - 1] >= 0).any() or H * W < 4   # some pixel fills all K slots


@pytest.mark.parametrize("H,W", [(53, 37), (17, 129)])
@pytest.mark.parametrize("k", [1, 4])
def test_rasterize_shapes_without_culling(nn, oracle_mod, H, W, k):
    """cull_back_faces=False: the soup's clockwise half is drawn too (negative area, negative reciprocal)."""
    f, m = _soup(H, W)
    ref = oracle_mod.rasterize(f, m, H, W, 0.5, k, -1, -1, True, False, False)
    culled = oracle_mod.rasterize(f, m, H, W, 0.5, k, -1, -1, True, False, True)
    assert not np.array_equal(ref[0], culled[0])
    got = nn.rendering.rasterize_ndc_triangles(f, m, (H, W), 0.5, k, -1, -1, True, False, False)
    _same(ref, got, f"{H}x{W} K={k} unculled")


@pytest.mark.parametrize("first,second", [((65, 63), (37, 53)), ((37, 53), (129, 17)), ((200, 3), (3, 200))])
def test_rasterize_repeated_call_at_another_size(nn, oracle_mod, first, second):
    """Two calls on the same stream straight after one another at different sizes: the second result does not depend
    on the first (the key image is reset per call, the scratch is reused in stream order)."""
    out = []
    for H, W in (first, second):
        f, m = _soup(H, W)
        out.append(nn.rendering.rasterize_ndc_triangles(f, m, (H, W), 0.5, 1, -1, -1, True, False, True))
    for (H, W), got in zip((first, second), out):
        f, m = _soup(H, W)
        _same(oracle_mod.rasterize(f, m, H, W, 0.5, 1, -1, -1, True, False, True), got, f"{H}x{W} after/before another size")


@pytest.mark.parametrize("H,W", [(200, 3), (3, 200)])
@pytest.mark.parametrize("k", [1, 4])
def test_rasterize_faces_larger_than_the_image(nn, oracle_mod, H, W, k):
    """Faces whose boxes overhang the image on both axes and on every side: pixel_first / pixel_last clamp to [0, dim)."""
    rx, ry = max(W / H, 1.0), max(H / W, 1.0)
    tri = []
    for i, s in enumerate((1.5, 3.0, 20.0, 1000.0)):
        z = 1.0 + 0.25 * i
        tri.append([(-s * rx, -s * ry, z), (s * rx, -s * ry, z + 0.1), (0.0, s * ry, z + 0.2)])
        tri.append([(s * rx, s * ry, z + 0.05), (-s * rx, s * ry, z + 0.15), (0.0, -s * ry, z)])
    # overhanging one corner each
    for cx, cy in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
        tri.append([(cx * rx - 2 * rx, cy * ry - 2 * ry, 0.8), (cx * rx + 2 * rx, cy * ry - 2 * ry, 0.8), (cx * rx, cy * ry + 2 * ry, 0.9)])
    tri = np.array(tri, np.float32)
    area = (tri[:, 0, 0] - tri[:, 1, 0]) * (tri[:, 1, 1] - tri[:, 2, 1]) - (tri[:, 0, 1] - tri[:, 1, 1]) * (tri[:, 1, 0] - tri[:, 2, 0])
    tri[area < 0] = tri[area < 0][:, [0, 2, 1]]
    for blur in (0.5, 0.0):
        ref = oracle_mod.rasterize(tri, None, H, W, blur, k, -1, -1, True, False, True)
        assert (ref[0][..., 0] >= 0).all()
        got = nn.rendering.rasterize_ndc_triangles(tri, None, (H, W), blur, k, -1, -1, True, False, True)
        _same(ref, got, f"{H}x{W} K={k} blur {blur} overhanging faces")


@pytest.mark.parametrize("H,W,fx", [(53, 37, 45.0), (37, 53, 45.0)])
def test_mesh_extraction_and_rasterize_meshes_shapes(nn, oracle_mod, H, W, fx):
    sc = shape_scene(H, W, fx)
    mesh = nn.geometry.TriangleMesh(sc.points, sc.normals, sc.faces)
    ndc_o, m_o = oracle_mod.extract_face_ndc(sc.points, sc.faces, sc.K, H, W, 0.0, 10.0)
    ndc_g, m_g = nn.rendering.functional.get_mesh_ndc_face_vertices_and_clip_mask(mesh, sc.K, (H, W), 0.0, 10.0)
    assert np.array_equal(m_o, _np(m_g).astype(bool)) and np.array_equal(ndc_o, _np(ndc_g))
    assert m_o.any() and m_o.all() == (W > H)   # the mesh overhangs the portrait image: some of its faces are clipped
    for k in (1, 4):
        ref = oracle_mod.rasterize(ndc_o, m_o, H, W, 0.5, k, -1, -1, False, False, True)
        got, _ = nn.rendering.rasterize_meshes(mesh, sc.K, (H, W), blur_radius_pixels=0.5, faces_per_pixel=k, near_clipping_distance=0.0,
                                               far_clipping_distance=10.0)
        _same(ref, got, f"rasterize_meshes {H}x{W} K={k}")
        assert (ref[0] >= 0).sum() > 500


def test_wrong_call_fails_loudly_at_a_portrait_size(nn, oracle_mod):
    H, W = 53, 37
    f, m = _soup(H, W)
    with pytest.raises(RuntimeError):
        nn.rendering.rasterize_ndc_triangles(f, m, (H, W), 0.5, 9, -1, -1, True, False, True)
    got = nn.rendering.rasterize_ndc_triangles(f, m, (H, W), 0.5, 1, -1, -1, True, False, True)
    _same(oracle_mod.rasterize(f, m, H, W, 0.5, 1, -1, -1, True, False, True), got, "the valid call after the refused one")


# ---------------------------------------------------------------------------------------------------------------------
# fused iteration
# ---------------------------------------------------------------------------------------------------------------------
_SCENES = {}


def _scene_and_target(oracle_mod, H, W, fx):
    if (H, W) not in _SCENES:
        sc = shape_scene(H, W, fx)
        depth = scene_target(oracle_mod, sc)   # shared, never written
        _SCENES[(H, W)] = (sc, depth)
    return _SCENES[(H, W)]


@pytest.mark.parametrize("H,W,fx", FIT_SHAPES)
def test_fit_one_iteration_shapes_from_identity(nn, oracle_mod, H, W, fx):
    sc, depth = _scene_and_target(oracle_mod, H, W, fx)
    R_o, t_o, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1)
    wf, ft, dg_g = _gpu_fit(nn, sc, depth, 1)
    assert (dg_o["pixel_faces"] >= 0).sum() > 400 and dg_o["residual_mask"].sum() > 350
    _compare_iteration(dg_o, dg_g, 6, len(sc.nodes))
    assert rel_err(wf.get_node_translations(True), t_o) < 1e-4
    assert rel_err(wf.get_node_rotations(True) - np.eye(3), R_o - np.eye(3)) < 1e-4


@pytest.mark.parametrize("H,W,fx", FIT_SHAPES)
def test_fit_one_iteration_shapes_from_partial_motion(nn, oracle_mod, H, W, fx):
    """From half the ground-truth motion: the general warp kernel and a deformed mesh under the odd-size raster."""
    sc, depth = _scene_and_target(oracle_mod, H, W, fx)
    wf, ft = _new_fit(nn, sc, depth, 1)
    R, t = sc.partial_motion(0.5)
    wf.set_node_rotations(R)
    wf.set_node_translations(t)
    R0, t0 = wf.get_node_rotations(True), wf.get_node_translations(True)
    ft.iterate(wf, 0, 1)
    dg_g = ft.diagnostics()
    ft.check()
    R_o, t_o, dg_o = oracle_fit_scene(oracle_mod, sc, depth, 1, R0=R0, t0=t0)
    assert (dg_o["pixel_faces"] >= 0).sum() > 400 and dg_o["residual_mask"].sum() > 350
    _compare_iteration(dg_o, dg_g, 6, len(sc.nodes))
    assert rel_err(wf.get_node_translations(True), t_o) < 1e-4
    assert rel_err(wf.get_node_rotations(True) - np.eye(3), R_o - np.eye(3)) < 1e-4


SWITCHES = [("NNRT_RASTER_DENSE", ("1", "0"), "raster_dense", {"1": 1, "0": 0}),
            ("NNRT_TILE_ORDER", ("2", "0"), "tile_order", {"2": 1, "0": 0}),
            ("NNRT_PIX_WPE4", ("1", "0"), "pix_low_occupancy", {"1": 1, "0": 0})]


@pytest.mark.parametrize("switch,values,plan_key,plan_value", SWITCHES, ids=[s[0] for s in SWITCHES])
@pytest.mark.parametrize("H,W,fx", [(53, 37, 45.0), (107, 75, 90.0)])
def test_launch_switches_same_iteration_shapes(nn, oracle_mod, monkeypatch, H, W, fx, switch, values, plan_key, plan_value):
    """Each launch switch forced both ways at a portrait size with partial tiles on both axes: the same iteration (faces,
    masks and residuals identical; H, g 1e-6 and updates 1e-5 -- the fp64 atomics' order -- as the same-iteration tests of
    test_gpu_parity), and the forced path is the one the frame ran."""
    sc, depth = _scene_and_target(oracle_mod, H, W, fx)
    N = len(sc.nodes)
    out = {}
    for v in values:
        monkeypatch.setenv(switch, v)
        _, ft, dg = _gpu_fit(nn, sc, depth, 1)
        assert ft.launch_plan()[plan_key] == plan_value[v], "the forced path is not the one that ran"
        out[v] = dg
    a, b = out[values[0]], out[values[1]]
    assert (a["pixel_faces"] >= 0).sum() > 1000
    for k in ("pixel_faces", "residual_mask", "residuals"):
        assert np.array_equal(a[k], b[k]), k
    assert rel_err(a["hessian"][: 36 * N], b["hessian"][: 36 * N]) < 1e-6
    assert rel_err(a["gradient"][: 6 * N], b["gradient"][: 6 * N]) < 1e-6
    assert nan_rel_err(a["updates"][: 6 * N], b["updates"][: 6 * N]) < 1e-5


def test_default_raster_build_follows_faces_per_pixel(nn, oracle_mod):
    """Unforced, the dense scatter runs where the mesh has at least as many faces as the image has pixels (53 x 37) and
    the lane-pair scatter where it has fewer (107 x 75)."""
    assert os.environ.get("NNRT_RASTER_DENSE") is None
    for (H, W, fx), dense in (((53, 37, 45.0), 1), ((107, 75, 90.0), 0)):
        sc, depth = _scene_and_target(oracle_mod, H, W, fx)
        _, ft = _new_fit(nn, sc, depth, 1)
        assert ft.launch_plan()["raster_dense"] == dense


@pytest.mark.parametrize("from_identity", [True, False])
def test_fitter_warp_bit_exact_portrait(nn, oracle_mod, from_identity):
    H, W, fx = 53, 37, 45.0
    sc, depth = _scene_and_target(oracle_mod, H, W, fx)
    wf, ft = _new_fit(nn, sc, depth, 1)
    V, Nn = len(sc.points), len(sc.nodes)
    if from_identity:
        ft.iterate_from_identity(wf, 0, 1)
        R0, t0 = np.tile(np.eye(3, dtype=np.float32), (Nn, 1, 1)), np.zeros((Nn, 3), np.float32)
    else:
        wf.set_node_rotations(sc.gt_rotations)
        wf.set_node_translations(sc.gt_translations)
        R0, t0 = wf.get_node_rotations(True), wf.get_node_translations(True)
        ft.iterate(wf, 0, 1)
    p_g, n_g = ft.warped_mesh(V)
    a, w = ft.anchors(V, 4)
    p_o, n_o = oracle_mod.warp_mesh(sc.points, sc.normals, wf.get_node_positions(True), R0, t0, a, w)
    assert np.array_equal(p_g, p_o) and np.array_equal(n_g, n_o)
