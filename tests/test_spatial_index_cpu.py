"""The uniform-grid point index without a GPU: the numpy restatement (tests/_spatial_index_util.py) reproduces the reference's
known answers (tests/golden/spatial_index_kat.py), the mirror has the six bindings with the reference's signatures, and the
C-ABI refuses bad arguments on the host before any device work (made-up non-null addresses stand in for arrays the checks
never reach, as in tests/test_depth_filter_abi.py)."""
import ctypes
import inspect
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _spatial_index_util as U  # noqa: E402
from golden import spatial_index_kat as KAT  # noqa: E402
from test_mirror_signatures import _matches  # noqa: E402  (the rule stated in that file's docstring)

FAKE = 0x7f0000000000   # never dereferenced

SIX = [("nnrt.core", "kd_tree", "__init__"), ("nnrt.core", "kd_tree", "find_k_nearest_to_points"),
       ("nnrt.geometry.functional", "m", "mean_grid_downsample_3d_points"),
       ("nnrt.geometry.functional", "m", "closest_to_mean_grid_subsample_3d_points"),
       ("nnrt.geometry.functional", "m", "fast_mean_radius_downsample_3d_points"),
       ("nnrt.geometry.functional", "m", "fast_median_radius_subsample_3d_points")]


# ---------------------------------------------------------------- the oracle reproduces the reference's known answers ----
@pytest.mark.parametrize("case", ["KNN15", "KNN100"])
def test_oracle_knn_reproduces_the_reference(case):
    points, queries = getattr(KAT, case + "_POINTS"), getattr(KAT, case + "_QUERIES")
    want_i, want_d = getattr(KAT, case + "_INDICES"), getattr(KAT, case + "_DISTANCES")
    got_i, got_d = U.knn(points, queries, want_i.shape[1])
    assert np.array_equal(got_i, want_i)
    assert np.abs(got_d.astype(np.float64) - want_d.astype(np.float64)).max() <= KAT.KNN_DISTANCE_MARGIN


def sorted_rows(a):
    a = np.asarray(a)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def test_oracle_mean_grid_reproduces_the_reference():
    got = U.mean_grid(KAT.MEAN_GRID_POINTS, KAT.MEAN_GRID_CELL_SIZE)
    assert got.shape == KAT.MEAN_GRID_EXPECTED.shape
    assert np.abs(sorted_rows(got).astype(np.float64) - sorted_rows(KAT.MEAN_GRID_EXPECTED)).max() <= KAT.MEAN_GRID_MARGIN


def check_median_kat(sample):
    sample = set(int(i) for i in sample)
    assert len(sample) == 4
    for i in KAT.MEDIAN_GRID_MUST_HOLD:
        assert i in sample
    for pair in KAT.MEDIAN_GRID_ONE_OF:
        assert len(sample & set(pair)) == 1


def test_oracle_median_grid_reproduces_the_reference():
    check_median_kat(U.median_grid(KAT.MEDIAN_GRID_POINTS, KAT.MEDIAN_GRID_CELL_SIZE))


def test_oracle_closest_to_mean_reproduces_the_reference():
    assert np.array_equal(U.closest_to_mean_grid(KAT.CLOSEST_TO_MEAN_POINTS, KAT.CLOSEST_TO_MEAN_CELL_SIZE), KAT.CLOSEST_TO_MEAN_EXPECTED)


def test_oracle_orders_cells_by_first_member_and_floors_negative_coordinates():
    pts = np.array([[2.5, 0, 0], [-1.0, 0, 0], [2.25, 0, 0], [-0.5, 0, 0], [-1.5, 0, 0], [0.0, 0, 0]], np.float32)
    members = U.cells_of(pts, 1.0)
    assert [m.tolist() for m in members] == [[0, 2], [1, 3], [4], [5]]   # -1.0 and -0.5 share cell -1; truncation would merge -0.5 with 0.0
    assert [m.tolist() for m in U.cells_of(pts, 1.0, (0.5, 0.5, 0.5))] == [[0], [1, 4], [2], [3, 5]]
    idx, dist = U.knn(pts[:2], pts[:1], 4)
    assert idx.tolist() == [[0, 1, -1, -1]] and dist[0, 0] == 0 and dist[0, 1] == 3.5 and np.isinf(dist[0, 2:]).all()
    assert U.ulp_distance(np.float32([1.0, -0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0])).tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------- the mirror's names ----
def _target(nn, module, receiver, name):
    if receiver == "kd_tree":
        cls = getattr(nn.core, "KDTree")
        return cls if name == "__init__" else getattr(cls, name)
    return getattr(nn.geometry.functional, name)


@pytest.mark.parametrize("key", SIX, ids=lambda k: f"{k[1]}.{k[2]}")
def test_mirror_has_the_binding_with_the_reference_signature(key):
    import dynamicfuion_python_amd.nnrt as nn
    with open(os.path.join(HERE, "golden", "reference_signatures.json")) as f:
        rows = [r for r in json.load(f) if (r["module"], r["receiver"], r["name"]) == key]
    assert len(rows) == 1, key
    fn = _target(nn, *key)
    params = list(inspect.signature(fn).parameters.values())
    if params and params[0].name == "self":
        params = params[1:]
    assert _matches(params, rows[0]["args"]), (key, rows[0]["args"], [(p.name, p.default) for p in params])


def test_grid_functions_are_module_level_and_take_a_grid_offset():
    import dynamicfuion_python_amd.nnrt.geometry as G
    for name in ("mean_grid_downsample_3d_points", "closest_to_mean_grid_subsample_3d_points"):
        fn = getattr(G, name)
        assert getattr(G.functional, name) is fn
        assert tuple(inspect.signature(fn).parameters["grid_offset"].default) == (0., 0., 0.)
    for name in ("fast_mean_radius_downsample_3d_points", "fast_median_radius_subsample_3d_points"):
        assert getattr(G.functional, name) is getattr(G, name)


def test_kdtree_refuses_shapes_and_k_before_any_device_work():
    import dynamicfuion_python_amd.nnrt as nn
    for bad in (np.zeros((4, 2), np.float32), np.zeros((4, 3, 1), np.float32), np.zeros(6, np.float32), np.zeros((0, 3), np.float32)):
        with pytest.raises(RuntimeError, match="points|point"):
            nn.core.KDTree(bad)


# -------------------------------------------------------------------------------------------------------- the C-ABI ----
@pytest.fixture(scope="module")
def native():
    from dynamicfuion_python_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


GRID_ENTRIES = ("nnrt_mean_grid_downsample_3d_points", "nnrt_closest_to_mean_grid_subsample_3d_points",
                "nnrt_median_grid_subsample_3d_points_binned")


@pytest.mark.parametrize("entry", GRID_ENTRIES)
def test_grid_entry_points_refuse_bad_arguments_on_the_host(native, entry):
    lib = native.lib()
    assert entry in native.exported_symbols()
    count = np.full(1, -7, np.int64)

    def call(d_points=FAKE, n=100, cell=0.5, offset=(0., 0., 0.), d_out=FAKE + 0x100000, h_count=count):
        st = getattr(lib, entry)(ctypes.c_void_p(d_points), n, cell, offset[0], offset[1], offset[2], ctypes.c_void_p(d_out),
                                 None if h_count is None else native.ptr(h_count), None)
        return st, lib.nnrt_last_error()

    nan, inf = float("nan"), float("inf")
    for kw, text in ((dict(cell=0.0), b"grid_cell_size"), (dict(cell=-1.0), b"grid_cell_size"), (dict(cell=nan), b"grid_cell_size"),
                     (dict(cell=inf), b"grid_cell_size"), (dict(offset=(0., nan, 0.)), b"offset"), (dict(offset=(inf, 0., 0.)), b"offset"),
                     (dict(d_points=None), b"null d_points"), (dict(d_out=None), b"null output"), (dict(h_count=None), b"null h_cell_count"),
                     (dict(n=-1), b"point count"), (dict(n=2 ** 31), b"point count"), (dict(n=0, cell=0.0), b"grid_cell_size")):
        st, msg = call(**kw)
        assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (kw, st, msg)
    st, _ = call(n=0, d_points=None, d_out=None)   # no points: no cells, nothing launched
    assert st == 0 and count[0] == 0
    with pytest.raises(native.NnrtError):
        native.check(call(cell=0.0)[0])


def test_point_index_refuses_bad_arguments_on_the_host(native):
    lib = native.lib()
    for name in ("nnrt_point_index_create", "nnrt_point_index_destroy", "nnrt_point_index_get_info", "nnrt_point_index_find_k_nearest"):
        assert name in native.exported_symbols()
    handle = ctypes.c_void_p(0x1234)

    def create(d_points=FAKE, n=10, dims=3, out=True):
        st = lib.nnrt_point_index_create(ctypes.c_void_p(d_points), n, dims, None, ctypes.byref(handle) if out else None)
        return st, lib.nnrt_last_error()

    for kw, text in ((dict(n=0), b"point_count"), (dict(n=-3), b"point_count"), (dict(dims=2), b"[point_count, 3]"), (dict(dims=1), b"[point_count, 3]"),
                     (dict(dims=4), b"[point_count, 3]"), (dict(d_points=None), b"null d_points"), (dict(out=False), b"null output")):
        handle.value = 0x1234
        st, msg = create(**kw)
        assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (kw, st, msg)
        assert kw.get("out") is False or handle.value is None   # a refused creation leaves a null handle

    def find(index=FAKE, d_queries=FAKE, q=5, dims=3, k=4, d_idx=FAKE + 0x1000, d_dist=FAKE + 0x2000):
        st = lib.nnrt_point_index_find_k_nearest(ctypes.c_void_p(index), ctypes.c_void_p(d_queries), q, dims, k, ctypes.c_void_p(d_idx),
                                                 ctypes.c_void_p(d_dist), None)
        return st, lib.nnrt_last_error()

    for kw, text in ((dict(k=0), b"k must be in [1, 16]"), (dict(k=17), b"k must be in [1, 16]"), (dict(k=-1), b"k must be in [1, 16]"),
                     (dict(index=None), b"null index"), (dict(dims=2), b"[query_count, 3]"), (dict(q=-1), b"query count"),
                     (dict(d_queries=None), b"null d_query_points"), (dict(d_idx=None), b"null d_out_indices"),
                     (dict(d_dist=None), b"null d_out_distances"), (dict(q=0, k=17), b"k must be in [1, 16]")):
        st, msg = find(**kw)
        assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (kw, st, msg)
    assert find(q=0, d_queries=None, d_idx=None, d_dist=None)[0] == 0   # no queries: nothing launched, nothing read
    assert lib.nnrt_point_index_get_info(None, None, None, None, None) == 1
    lib.nnrt_point_index_destroy(None)   # a null handle is no error
