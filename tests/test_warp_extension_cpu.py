"""CPU checks of the warp field extension: the numpy restatement's own sanity, the switch's defaults and
refusal, and the two entry points' host-side argument checks, which fail with NNRT_ERROR_ARGUMENT and a message before
anything is launched (pointers are never dereferenced, so made-up device addresses serve)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import _warp_extension_util as WU

BASE = 0x7f0000000000
ARGUMENT = 1


@pytest.fixture(scope="module")
def native():
    from dynamicfuion_python_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def _p(offset):
    return ctypes.c_void_p(BASE + offset)


POINTS, NODES, ROTATIONS, TRANSLATIONS, WEIGHTS, OUT_A, OUT_B, OUT_C = (0x100000 * k for k in range(1, 9))


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _field(seed=3, count=40):
    rng = np.random.default_rng(seed)
    nodes = rng.uniform(-0.2, 0.2, (count, 3)).astype(np.float32)
    points = rng.uniform(-0.25, 0.25, (17, 3)).astype(np.float32)
    return rng, nodes, points


def test_blend_of_one_rigid_motion_returns_it():
    """Every node carries the same map x -> Q x + T (t_k = Q g_k + T - g_k): the blend at p is that map expressed at p."""
    rng, nodes, points = _field()
    Q = WU.rotations_about([[1.0, -2.0, 0.5]], [37.0])[0]
    T = np.array([0.03, -0.01, 0.02])
    g = nodes.astype(np.float64)
    rotations = np.tile(Q, (len(nodes), 1, 1))
    translations = g @ Q.T + T - g
    R, t, fallbacks = WU.blend_node_transformations(points, nodes, rotations, translations, 4, 0.05)
    p = points.astype(np.float64)
    assert fallbacks == 0
    assert np.abs(R - Q.astype(np.float32).astype(np.float64)).max() < 1e-7     # the inputs pass through float32
    assert np.abs(t - (p @ Q.T + T - p)).max() < 1e-7


def test_blend_of_the_identity_is_exact():
    _, nodes, points = _field()
    for K in (1, 4, 8):
        R, t, fallbacks = WU.blend_node_transformations(points, nodes, np.tile(np.eye(3, dtype=np.float32), (len(nodes), 1, 1)),
                                                        np.zeros((len(nodes), 3), np.float32), K, 0.05)
        assert fallbacks == 0 and np.array_equal(R, np.tile(np.eye(3), (len(points), 1, 1))) and np.array_equal(t, np.zeros((len(points), 3)))


def test_blend_falls_back_on_opposite_rotations():
    nodes = np.float32([[-0.02, 0, 0], [0.02, 0, 0]])
    rotations = np.stack([WU.rotations_about([[0, 0, 1.0]], [30.0])[0], WU.rotations_about([[0, 0, 1.0]], [210.0])[0]]).astype(np.float32)
    R, _, fallbacks = WU.blend_node_transformations(np.zeros((1, 3), np.float32), nodes, rotations, np.zeros((2, 3), np.float32), 4, 0.05)
    assert fallbacks == 1 and np.array_equal(R[0], rotations[0].astype(np.float64))


def test_support_ratio_of_a_node_position_is_zero():
    _, nodes, _ = _field()
    for weights in (None, np.linspace(0.001, 0.004, len(nodes)).astype(np.float32)):
        ratio, nearest = WU.vertex_support(nodes, nodes, 0.05, weights)
        assert np.array_equal(ratio, np.zeros(len(nodes), np.float32)) and np.array_equal(nearest, np.arange(len(nodes)))
    ratio, nearest = WU.vertex_support(nodes[:3], nodes[:0], 0.05)
    assert np.isposinf(ratio).all() and (nearest == -1).all()
    ratio, nearest = WU.vertex_support(np.float32([[np.nan, 0, 0], [0.05, 0, 0]]), np.zeros((2, 3), np.float32), 0.05)
    assert list(ratio) == [0.0, 1.0] and list(nearest) == [-1, 0]   # a non-finite vertex; the lower of two equal nodes


# ---- the switch -----------------------------------------------------------------------------------------------------------
def test_extension_is_off_by_default():
    from dynamicfuion_python_amd import fusion as F
    p = F.FusionParameters()
    assert p.warp_field_extension is False
    assert p.warp_field_extension_support_ratio == 1.0 and p.warp_field_extension_minimum_new_node_count == 1
    r = F.FrameResult(0)
    assert r.node_count == 0 and r.new_node_count == 0


def test_pipeline_refuses_extension_with_shortest_path_anchors():
    from dynamicfuion_python_amd import fusion as F
    params = F.FusionParameters(warp_field_extension=True, anchor_computation_mode=F.AnchorComputationMode.SHORTEST_PATH)
    with pytest.raises(NotImplementedError, match="warp_field_extension"):
        F.FusionPipeline(None, params)   # refused before the sequence or a device is touched


def test_python_signatures():
    from dynamicfuion_python_amd import nnrt
    from dynamicfuion_python_amd.warp_field import extend_warp_field
    f = nnrt.geometry.functional
    assert [(p.name, p.default) for p in inspect.signature(f.compute_vertex_support).parameters.values()] == [
        ("points", inspect.Parameter.empty), ("nodes", inspect.Parameter.empty), ("node_coverage", 0.05), ("node_coverage_weights", None)]
    assert [(p.name, p.default) for p in inspect.signature(f.blend_node_transformations).parameters.values()] == [
        ("points", inspect.Parameter.empty), ("nodes", inspect.Parameter.empty), ("node_rotations", inspect.Parameter.empty),
        ("node_translations", inspect.Parameter.empty), ("anchor_count", 4), ("node_coverage", 0.05)]
    assert [(p.name, p.default) for p in inspect.signature(extend_warp_field).parameters.values()] == [
        ("warp_field", inspect.Parameter.empty), ("canonical_mesh", inspect.Parameter.empty), ("make_warp_field", inspect.Parameter.empty),
        ("support_ratio_threshold", 1.0), ("minimum_new_node_count", 1)]


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def _support(native, points=_p(POINTS), count=10, nodes=_p(NODES), node_count=5, coverage=0.05, weights=None, ratio=_p(OUT_A),
             nearest=_p(OUT_B)):
    lib = native.lib()
    st = lib.nnrt_compute_vertex_support(points, count, nodes, node_count, coverage, weights, ratio, nearest, None)
    return st, lib.nnrt_last_error()


def _blend(native, points=_p(POINTS), count=10, nodes=_p(NODES), rotations=_p(ROTATIONS), translations=_p(TRANSLATIONS), node_count=5, K=4,
           coverage=0.05, out_rotations=_p(OUT_A), out_translations=_p(OUT_B), fallback=_p(OUT_C)):
    lib = native.lib()
    n = np.full(1, -1, np.int64)
    st = lib.nnrt_blend_node_transforms(points, count, nodes, rotations, translations, node_count, K, coverage, out_rotations,
                                        out_translations, fallback, native.ptr(n), None)
    return st, lib.nnrt_last_error(), int(n[0])


@pytest.mark.parametrize("kwargs, message", [
    (dict(points=None), b"null"),
    (dict(nodes=None), b"null"),
    (dict(ratio=None), b"null"),
    (dict(nearest=None), b"null"),
    (dict(count=-1), b"point count"),
    (dict(node_count=-1), b"node count"),
    (dict(coverage=0.0), b"node_coverage"),
    (dict(coverage=-0.05), b"node_coverage"),
    (dict(coverage=float("nan")), b"node_coverage"),
    (dict(coverage=float("inf")), b"node_coverage"),
])
def test_vertex_support_refuses_bad_arguments(native, kwargs, message):
    st, msg = _support(native, **kwargs)
    assert st == ARGUMENT
    assert msg.startswith(b"invalid argument") and message in msg


@pytest.mark.parametrize("kwargs, message", [
    (dict(K=0), b"anchor_count"),
    (dict(K=9), b"anchor_count"),
    (dict(K=-1), b"anchor_count"),
    (dict(points=None), b"null"),
    (dict(nodes=None), b"null"),
    (dict(rotations=None), b"null"),
    (dict(translations=None), b"null"),
    (dict(out_rotations=None), b"null"),
    (dict(out_translations=None), b"null"),
    (dict(fallback=None), b"null"),
    (dict(count=-1), b"point count"),
    (dict(node_count=-1), b"node count"),
    (dict(node_count=0), b"no node"),
    (dict(coverage=0.0), b"node_coverage"),
    (dict(coverage=float("nan")), b"node_coverage"),
    (dict(coverage=1e-30), b"node_coverage"),   # its square is not a normal float
])
def test_blend_refuses_bad_arguments(native, kwargs, message):
    st, msg, _ = _blend(native, **kwargs)
    assert st == ARGUMENT
    assert msg.startswith(b"invalid argument") and message in msg


def test_surface_growth_switch_refuses_a_null_grid(native):
    lib = native.lib()
    assert lib.nnrt_voxel_grid_set_non_rigid_surface_growth(None, 1) == ARGUMENT
    assert b"null" in lib.nnrt_last_error()


def test_zero_size_calls_succeed(native):
    assert _support(native, points=None, count=0, ratio=None, nearest=None)[0] == 0
    assert _support(native, points=None, count=0, nodes=None, node_count=0, ratio=None, nearest=None)[0] == 0
    st, _, n = _blend(native, points=None, count=0, nodes=None, rotations=None, translations=None, node_count=0, out_rotations=None,
                      out_translations=None, fallback=None)
    assert (st, n) == (0, 0)
