"""The uniform-grid point index on the GPU (csrc/spatial_grid.hip): nnrt.core.KDTree and the grid
down-samplers of nnrt.geometry.functional against the numpy restatement (tests/_spatial_index_util.py) and the reference's
known answers (tests/golden/spatial_index_kat.py), at the point counts where a wavefront, a workgroup or a cell's rounds
end, and the binned medoid against the all-pairs median_grid_subsample_3d_points it must equal bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _spatial_index_util as U  # noqa: E402
from golden import spatial_index_kat as KAT  # noqa: E402
from test_spatial_index_cpu import check_median_kat, sorted_rows  # noqa: E402

F32 = np.float32
FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_fixtures")
KS = (1, 4, 8, 16)
QS = (1, 65, 257)
HALF = (0.5, 0.5, 0.5)


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import nnrt
    return nnrt


def _np(t):
    return t.detach().cpu().numpy()


# --------------------------------------------------------------------------------------------------------- known answers ----
@pytest.mark.parametrize("case", ["KNN15", "KNN100"])
def test_knn_reproduces_the_reference(nn, case):
    points, queries = getattr(KAT, case + "_POINTS"), getattr(KAT, case + "_QUERIES")
    want_i, want_d = getattr(KAT, case + "_INDICES"), getattr(KAT, case + "_DISTANCES")
    tree = nn.core.KDTree(points)
    for sort_output in (False, True):
        got_i, got_d = tree.find_k_nearest_to_points(queries, want_i.shape[1], sort_output)
        assert got_i.dtype == torch.int32 and got_d.dtype == torch.float32 and got_i.is_cuda and got_d.is_cuda
        assert np.array_equal(_np(got_i), want_i)
        assert np.abs(_np(got_d).astype(np.float64) - want_d.astype(np.float64)).max() <= KAT.KNN_DISTANCE_MARGIN
    tree.close()


def test_grid_samplers_reproduce_the_reference(nn):
    fn = nn.geometry.functional
    got = _np(fn.mean_grid_downsample_3d_points(KAT.MEAN_GRID_POINTS, KAT.MEAN_GRID_CELL_SIZE))
    assert got.shape == KAT.MEAN_GRID_EXPECTED.shape
    assert np.abs(sorted_rows(got).astype(np.float64) - sorted_rows(KAT.MEAN_GRID_EXPECTED)).max() <= KAT.MEAN_GRID_MARGIN
    check_median_kat(_np(nn.geometry.functional.median_grid_subsample_3d_points(KAT.MEDIAN_GRID_POINTS, KAT.MEDIAN_GRID_CELL_SIZE)))
    check_median_kat(_np(fn.median_grid_subsample_3d_points_binned(KAT.MEDIAN_GRID_POINTS, KAT.MEDIAN_GRID_CELL_SIZE)))
    got = fn.closest_to_mean_grid_subsample_3d_points(KAT.CLOSEST_TO_MEAN_POINTS, KAT.CLOSEST_TO_MEAN_CELL_SIZE)
    assert got.dtype == torch.int64 and np.array_equal(_np(got), KAT.CLOSEST_TO_MEAN_EXPECTED)


# ------------------------------------------------------------------------------------------------------------------ K-NN ----
def check_knn(nn, points, queries_by_count):
    """indices equal and distances bit-equal to the brute force at every k, for each query set; one index, one brute force
    at k = 16 per query set (a row's first k entries are the k nearest)."""
    tree = nn.core.KDTree(points)
    assert tree.info()["point_count"] == len(points)
    for queries in queries_by_count:
        want_i, want_d = U.knn(points, queries, 16)
        for k in KS:
            got_i, got_d = tree.find_k_nearest_to_points(queries, k)
            got_i, got_d = _np(got_i), _np(got_d)
            assert got_i.shape == (len(queries), k) and got_d.shape == (len(queries), k)
            assert np.array_equal(got_i, want_i[:, :k]), (len(points), len(queries), k)
            assert np.array_equal(got_d.view(np.uint32), want_d[:, :k].view(np.uint32)), (len(points), len(queries), k)
            if k > len(points):
                assert (got_i[:, len(points):] == -1).all() and np.isposinf(got_d[:, len(points):]).all()
    tree.close()


def uniform(n, seed, lo=-3.0, hi=5.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(F32)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000])
def test_knn_equals_brute_force_on_uniform_points(nn, n):
    points = uniform(n, 100 + n)
    # queries inside the box and up to half a box outside it
    check_knn(nn, points, [uniform(q, 7 * n + q, -7.0, 9.0) for q in QS])


def lattice(n, seed):
    g = np.arange(-3, 4)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F32)
    return pts[np.random.default_rng(seed).permutation(len(pts))[:n]]


def layout(name):
    """(points, [query sets of 1, 65 and 257 queries])"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "identical":   # every point the same: one cell of zero extent, order by index alone
        points = np.tile(np.array([[0.7, -1.3, 2.1]], F32), (65, 1))
        return points, [np.concatenate([points[:1], uniform(q - 1, q, -2.0, 3.0)]) for q in QS]
    if name == "cluster":     # 130 points inside one cell and 5 far outliers
        points = np.concatenate([rng.uniform(0.251, 0.252, (130, 3)), rng.uniform(-40.0, 40.0, (5, 3))]).astype(F32)
        return points, [np.concatenate([uniform(q - q // 2, q, -45.0, 45.0), rng.uniform(0.2505, 0.2525, (q // 2, 3)).astype(F32)]) for q in QS]
    if name == "coplanar":    # z = 0: the grid is two-dimensional
        points = uniform(257, 5)
        points[:, 2] = 0.0
        return points, [uniform(q, q + 1, -4.0, 6.0) for q in QS]
    if name == "lattice":     # integer coordinates: many exactly equal distances, order decided by index
        points = lattice(257, 3)
        queries = np.concatenate([lattice(129, 4), lattice(128, 6) + F32(0.5)])
        return points, [queries[:q] for q in QS]
    if name == "far_queries":   # 100 box diagonals outside the cloud, in every direction
        points = uniform(257, 8)
        diagonal = float(np.linalg.norm(points.max(0) - points.min(0)))
        directions = rng.normal(size=(257, 3))
        directions /= np.linalg.norm(directions, axis=1, keepdims=True)
        directions[:6] = np.concatenate([np.eye(3), -np.eye(3)])   # along the axes too
        queries = (points.mean(0) + 100.0 * diagonal * directions).astype(F32)
        return points, [queries[:q] for q in QS]
    if name == "queries_are_points":
        points = uniform(1000, 9)
        return points, [points[rng.permutation(1000)[:q]] for q in QS]
    raise KeyError(name)


@pytest.mark.parametrize("name", ["identical", "cluster", "coplanar", "lattice", "far_queries", "queries_are_points"])
def test_knn_equals_brute_force_on_hard_layouts(nn, name):
    points, query_sets = layout(name)
    check_knn(nn, points, query_sets)


def test_knn_far_from_the_origin_and_empty_query_set(nn):
    """A small cloud at a large offset (the cell size is floored so that every cell fits the key) and no queries."""
    points = (uniform(257, 12, -0.01, 0.01) + np.array([5000.0, -7000.0, 3000.0], F32)).astype(F32)
    check_knn(nn, points, [points[:65] + F32(0.001)])
    tree = nn.core.KDTree(points)
    got_i, got_d = tree.find_k_nearest_to_points(np.zeros((0, 3), F32), 4)
    assert tuple(got_i.shape) == (0, 4) and tuple(got_d.shape) == (0, 4)
    for bad_k in (0, 17):
        with pytest.raises(RuntimeError):
            tree.find_k_nearest_to_points(points[:3], bad_k)
    with pytest.raises(RuntimeError):
        tree.find_k_nearest_to_points(np.zeros((3, 2), F32), 4)
    tree.close()
    with pytest.raises(RuntimeError, match="closed"):
        tree.find_k_nearest_to_points(points[:3], 4)


# --------------------------------------------------------------------------------------------------------- grid functions ----
CELL = 0.25   # a power of two: its multiples are exact float32 values


def grid_points(n, per_cell, seed, cluster=False):
    """n points in a box sized for about per_cell members per cell of size CELL; every third point sits exactly on a multiple
    of CELL (negative ones included), so flooring and truncating differ; cluster: the first 130 lie in one cell."""
    rng = np.random.default_rng(seed)
    side = CELL * max(np.cbrt(n / per_cell), 1.0)
    pts = rng.uniform(-side / 2, side / 2, (n, 3)).astype(F32)
    snapped = np.round(pts / F32(CELL)) * F32(CELL)
    pts[::3] = snapped[::3]
    if cluster:
        pts[:130] = rng.uniform(0.26, 0.37, (130, 3)).astype(F32)   # one cell at offset 0 and at offset 0.5
    return pts


def check_grid_functions(nn, pts, cell, offset):
    fn = nn.geometry.functional
    want = U.mean_grid(pts, cell, offset)
    got = _np(fn.mean_grid_downsample_3d_points(pts, cell, offset))
    assert got.shape == want.shape and got.dtype == F32   # the cell count, and row for row the same cells
    assert U.ulp_distance(got, want).max(initial=0) <= 1
    got = fn.closest_to_mean_grid_subsample_3d_points(pts, cell, offset)
    assert got.dtype == torch.int64 and np.array_equal(_np(got), U.closest_to_mean_grid(pts, cell, offset))
    got = fn.median_grid_subsample_3d_points_binned(pts, cell, offset)
    assert got.dtype == torch.int64 and np.array_equal(_np(got), U.median_grid(pts, cell, offset))
    return got


@pytest.mark.parametrize("offset", [(0., 0., 0.), HALF], ids=["offset0", "offset0.5"])
@pytest.mark.parametrize("per_cell", [1, 10])
@pytest.mark.parametrize("n", [1, 64, 65, 257, 2000])
def test_grid_functions_equal_the_restatement(nn, n, per_cell, offset):
    check_grid_functions(nn, grid_points(n, per_cell, 31 * n + per_cell), CELL, offset)


@pytest.mark.parametrize("offset", [(0., 0., 0.), HALF], ids=["offset0", "offset0.5"])
@pytest.mark.parametrize("n", [257, 2000])
def test_grid_functions_with_a_cell_of_130_members(nn, n, offset):
    pts = grid_points(n, 1, n + 5, cluster=True)
    sizes = [len(m) for m in U.cells_of(pts, CELL, offset)]
    assert max(sizes) >= 130   # more than two rounds of a wavefront
    check_grid_functions(nn, pts, CELL, offset)


def test_grid_functions_with_a_cell_size_that_is_no_power_of_two(nn):
    check_grid_functions(nn, uniform(257, 77, -1.0, 1.0), 0.3, (0., 0., 0.))
    check_grid_functions(nn, uniform(65, 78, -1.0, 1.0), 10.0, HALF)   # one cell holds every point


@pytest.mark.parametrize("cell", [0.05, CELL, 0.6])
def test_binned_medoid_equals_the_all_pairs_medoid(nn, cell):
    """At offset 0 the binned path returns what median_grid_subsample_3d_points (the all-pairs kernels, unchanged) returns."""
    fn = nn.geometry.functional
    nodes = np.load(os.path.join(FIXTURES, "nodes_25-node_plane.npy")).astype(F32).reshape(-1, 3)
    for pts in (grid_points(2000, 1, 31 * 2000 + 1), grid_points(2000, 10, 31 * 2000 + 10), grid_points(2000, 1, 2005, cluster=True), nodes):
        size = cell if pts is not nodes else cell * float(np.ptp(nodes, axis=0).max())
        want = _np(fn.median_grid_subsample_3d_points(pts, size))
        got = _np(fn.median_grid_subsample_3d_points_binned(pts, size))
        assert len(want) >= 1 and np.array_equal(got, want)


@pytest.mark.parametrize("n,radius", [(65, 0.05), (257, 0.08), (2000, 0.04)])
def test_two_stage_radius_samplers_equal_the_composition_of_their_stages(nn, n, radius):
    fn = nn.geometry.functional
    pts = uniform(n, 50 + n, -0.5, 0.5)
    want = U.fast_mean_radius(pts, radius)
    got = _np(fn.fast_mean_radius_downsample_3d_points(pts, radius))
    assert got.shape == want.shape and U.ulp_distance(got, want).max(initial=0) <= 1
    want = U.fast_median_radius(pts, radius)
    got = fn.fast_median_radius_subsample_3d_points(pts, radius)
    assert got.dtype == torch.int64
    got = _np(got)
    assert np.array_equal(got, want)
    assert 1 <= len(got) < n and got.min() >= 0 and got.max() < n and len(set(got.tolist())) == len(got)   # indices into the input


# -------------------------------------------------------------------------------------------------- refusals and lifetime ----
def test_non_finite_and_out_of_range_points_are_refused_and_the_next_call_succeeds(nn):
    fn = nn.geometry.functional
    good = uniform(65, 1)
    with_nan = good.copy()
    with_nan[40, 1] = np.nan
    with_inf = good.copy()
    with_inf[64, 2] = -np.inf
    too_far = good.copy()
    too_far[3, 0] = 3.0e6   # cell 3e6 / 1.0 is outside [-2^20, 2^20)
    for call in (fn.mean_grid_downsample_3d_points, fn.closest_to_mean_grid_subsample_3d_points, fn.median_grid_subsample_3d_points_binned):
        for bad, text in ((with_nan, "non-finite"), (with_inf, "non-finite"), (too_far, "outside")):
            with pytest.raises(RuntimeError, match=text):
                call(bad, 1.0)
        assert len(call(good, 1.0)) == len(U.cells_of(good, 1.0))
    for bad in (with_nan, with_inf):
        with pytest.raises(RuntimeError, match="non-finite"):
            nn.core.KDTree(bad)
    check_knn(nn, too_far, [good[:65]])   # the index picks its own cell size: a far point is no error
    for call in (fn.mean_grid_downsample_3d_points, fn.closest_to_mean_grid_subsample_3d_points):
        with pytest.raises(RuntimeError):
            call(good, 0.0)
        with pytest.raises(RuntimeError):
            call(np.zeros((4, 2), F32), 1.0)


def test_kdtree_lifetime_and_streams(nn):
    """Built, queried on a stream of its own, closed, built again; closing returns the device memory the index held."""
    from dynamicfuion_python_amd import _native as N
    points, queries = uniform(1000, 21), uniform(257, 22)
    want_i, want_d = U.knn(points, queries, 4)
    torch.cuda.synchronize()
    before = N.lib().nnrt_device_bytes_in_use()
    tree = nn.core.KDTree(torch.as_tensor(points, device="cuda"))
    assert N.lib().nnrt_device_bytes_in_use() > before
    stream = torch.cuda.Stream()
    q = torch.as_tensor(queries, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got_i, got_d = tree.find_k_nearest_to_points(q, 4)
    stream.synchronize()
    assert np.array_equal(_np(got_i), want_i) and np.array_equal(_np(got_d), want_d)
    tree.close()
    tree.close()   # closing twice is harmless
    assert N.lib().nnrt_device_bytes_in_use() == before
    again = nn.core.KDTree(points)
    got_i, _ = again.find_k_nearest_to_points(queries, 4)
    assert np.array_equal(_np(got_i), want_i)
    del again
    import gc
    gc.collect()
    assert N.lib().nnrt_device_bytes_in_use() == before
