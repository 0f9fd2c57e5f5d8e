"""csrc/graph_sampling.hip against the sequential restatement (tests/_graph_util.py): the vertex erosion mask and the greedy
node sampling are compared with array_equal -- both are exact, deterministic algorithms, so there is no tolerance. Every
sampling case runs twice (bit-identical) and is also held to the two defining properties of the node set, independently
of the restatement: nodes are pairwise farther apart than coverage, and every candidate is within coverage of a node."""
import numpy as np
import pytest

import _graph_util as GU

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import nnrt
    return nnrt


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------- erosion ----
def _grid_mesh():
    """8 x 8 vertices, two triangles per quad, the 2 x 2 quads in the middle left out; vertex 64 belongs to no face."""
    faces = []
    for r in range(7):
        for c in range(7):
            if r in (3, 4) and c in (3, 4):
                continue
            a, b, d, e = 8 * r + c, 8 * r + c + 1, 8 * (r + 1) + c, 8 * (r + 1) + c + 1
            faces += [(a, b, d), (b, e, d)]
    return np.zeros((65, 3), np.float32), np.asarray(faces, np.int64)


@pytest.mark.parametrize("iterations", [0, 1, 2, 10])
def test_erosion_mask_matches_restatement(nn, iterations):
    vertices, faces = _grid_mesh()
    want = GU.erosion_mask(65, faces, iterations, 4)
    got = nn.get_vertex_erosion_mask(vertices, faces, iterations, 4)
    assert got.dtype == torch.bool and tuple(got.shape) == (65, 1) and got.is_cuda
    assert np.array_equal(_np(got)[:, 0], want)
    assert not want[64]                       # the lone vertex is eroded whatever the iteration count
    if iterations == 0:
        assert np.array_equal(np.flatnonzero(~want[:64]), [36])   # the hole's centre vertex has no face either
    if iterations == 1:
        assert 0 < want.sum() < 64
    if iterations == 10:
        assert not want.any()                 # the mesh erodes to nothing
    again = nn.get_vertex_erosion_mask(torch.from_numpy(vertices).cuda(), torch.from_numpy(faces).cuda(), iterations, 4)
    assert torch.equal(got, again)


def test_erosion_mask_without_faces_is_all_false(nn):
    got = nn.get_vertex_erosion_mask(np.zeros((5, 3), np.float32), np.zeros((0, 3), np.int64), 3, 4)
    assert tuple(got.shape) == (5, 1) and not _np(got).any()


def test_erosion_mask_refuses_an_out_of_range_face_index(nn):
    from dynamicfuion_python_amd._native import NnrtError
    vertices, faces = _grid_mesh()
    for bad in (65, -1):
        broken = faces.copy()
        broken[17, 1] = bad
        with pytest.raises(NnrtError, match="face index") as e:
            nn.get_vertex_erosion_mask(vertices, broken, 2, 4)
        assert e.value.status == 1
    assert np.array_equal(_np(nn.get_vertex_erosion_mask(vertices, faces, 2, 4))[:, 0], GU.erosion_mask(65, faces, 2, 4))


# --------------------------------------------------------------------------------------------------- sampling ----
def _check(nn, points, coverage, mask=None, order=None):
    """Runs the sampling twice; returns (indices, rounds) after every check the module docstring names."""
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    got_t, rounds = nn.graph_proc.sample_node_indices(points, mask, order, coverage)
    again_t, _ = nn.graph_proc.sample_node_indices(points, mask, order, coverage)
    # the nodes are bit-identical from run to run; the round count is not part of the result (a lane may or may not see a
    # decision taken earlier in the same round, which moves work between rounds and nothing else)
    assert got_t.dtype == torch.int64 and torch.equal(got_t, again_t)
    got = _np(got_t)
    want = GU.sample_nodes(points, coverage, mask, order)
    assert np.array_equal(got, want), f"{len(got)} nodes, restatement {len(want)}"
    cand = GU.candidates(points, mask, order)
    assert rounds <= len(cand) and (rounds >= 1) == (len(cand) > 0)
    nodes = points[got]
    close = GU.within(nodes[:, None, :], nodes[None, :, :], coverage)
    assert not (close & ~np.eye(len(nodes), dtype=bool)).any(), "two nodes within coverage of each other"
    if len(cand):
        assert GU.within(points[cand][:, None, :], nodes[None, :, :], coverage).any(axis=1).all(), "a candidate no node covers"
    return got, rounds


def test_collinear_chain_takes_several_rounds(nn):
    points = np.zeros((200, 3), np.float32)
    points[:, 0] = np.arange(200, dtype=np.float32) * np.float32(0.01)
    up, rounds_up = _check(nn, points, 0.05)
    assert up[0] == 0 and 2 <= rounds_up <= 200
    down, rounds_down = _check(nn, points, 0.05, order=np.arange(199, -1, -1))
    assert down[0] == 199 and 2 <= rounds_down <= 200
    assert (np.diff(up) > 0).all() and (np.diff(down) < 0).all()   # acceptance order is priority order


@pytest.fixture(scope="module")
def cloud():
    rng = np.random.default_rng(7)
    return rng.uniform(-1.0, 1.0, (3000, 3)).astype(np.float32), rng.random(3000) < 0.6


def test_uniform_cloud(nn, cloud):
    points, _ = cloud
    got, _ = _check(nn, points, 0.1)
    assert 100 < len(got) < 3000


def test_uniform_cloud_with_mask(nn, cloud):
    points, mask = cloud
    got, _ = _check(nn, points, 0.1, mask=mask)
    assert mask[got].all()
    _check(nn, points, 0.1, mask=mask.reshape(-1, 1))


@pytest.mark.parametrize("count", [1, 63, 65, 257])
def test_candidate_counts_around_wave_and_block_sizes(nn, count):
    points = np.random.default_rng(count).uniform(0.0, 0.5, (count, 3)).astype(np.float32)
    got, rounds = _check(nn, points, 0.1)
    assert got[0] == 0 and (rounds == 1) == (count == 1)


def test_duplicated_points_keep_the_first(nn):
    base = np.random.default_rng(3).uniform(-1.0, 1.0, (40, 3)).astype(np.float32) * 4.0
    points = np.concatenate([base, base[::-1], base])
    got, _ = _check(nn, points, 1e-3)
    assert np.array_equal(got, np.arange(40))


def test_exact_tie_counts_as_covered(nn):
    points = np.array([[0, 0, 0], [0.25, 0, 0], [0.25 + 2.0 ** -20, 0, 0]], np.float32)
    got, _ = _check(nn, points, 0.25)
    assert np.array_equal(got, [0, 2])


def test_pairs_across_cell_faces_edges_and_corners(nn):
    """The grid origin is the bounding-box minimum (the point at 0) and the cell edge coverage * (1 + 2^-20): each pair
    straddles the first cell boundary along one, two or three axes, shifted by whole cells so the pairs do not interact."""
    c = 0.1
    edge = c * (1.0 + 2.0 ** -20)
    pairs = [  # (a, b, b is covered by a)
        ((0.099, 0.05, 0.05), (0.101, 0.05, 0.05), True),      # face, inside
        ((0.05, 0.05, 0.05), (0.1501, 0.05, 0.05), False),     # face, outside
        ((0.099, 0.099, 0.05), (0.101, 0.101, 0.05), True),    # edge, inside
        ((0.03, 0.03, 0.05), (0.101, 0.101, 0.05), False),     # edge, outside: sqrt(2) * 0.071 > 0.1
        ((0.099, 0.099, 0.099), (0.101, 0.101, 0.101), True),  # corner, inside
        ((0.043, 0.043, 0.043), (0.101, 0.101, 0.101), False),  # corner, outside: sqrt(3) * 0.058 > 0.1
    ]
    points, expect = [(0.0, 0.0, 0.0)], [0]
    for k, (a, b, covered) in enumerate(pairs, start=1):
        shift = np.array([10 * k * edge, 0.0, 10 * (k % 2) * edge])
        expect.append(len(points))
        points.append(tuple(np.array(a) + shift))
        if not covered:
            expect.append(len(points))
        points.append(tuple(np.array(b) + shift))
    points = np.asarray(points, np.float32)
    got, _ = _check(nn, points, c)
    assert np.array_equal(got, expect)
    cells = np.floor(points.astype(np.float64) / edge).astype(np.int64)
    for k in range(6):   # every pair does straddle a boundary on the intended number of axes
        assert (cells[2 + 2 * k] - cells[1 + 2 * k] != 0).sum() == k // 2 + 1
    _check(nn, points, c, order=np.arange(len(points) - 1, -1, -1))


def test_far_outlier_keeps_the_grid_sparse(nn, cloud):
    """One point 10^5 cells away: the grid is kept as sorted cell keys, O(candidates), and the result stays exact."""
    points = np.concatenate([cloud[0][:1000], np.array([[1e4, 0, 0]], np.float32)])
    free_before = torch.cuda.mem_get_info()[0]
    got, _ = _check(nn, points, 0.1)
    assert got[-1] == 1000
    assert torch.cuda.mem_get_info()[0] >= free_before - (64 << 20)   # scratch is returned


def test_extent_beyond_the_key_range_is_refused(nn):
    from dynamicfuion_python_amd._native import NnrtError
    with pytest.raises(NnrtError, match="cells") as e:
        nn.graph_proc.sample_node_indices(np.array([[0, 0, 0], [0, 1e6, 0]], np.float32), None, None, 0.1)
    assert e.value.status == 1


def test_order_entry_out_of_range_is_refused(nn):
    from dynamicfuion_python_amd._native import NnrtError
    with pytest.raises(NnrtError, match="d_order") as e:
        nn.graph_proc.sample_node_indices(np.zeros((3, 3), np.float32), None, np.array([0, 3, 1]), 0.1)
    assert e.value.status == 1


def test_non_finite_vertex_is_skipped(nn, cloud):
    points = cloud[0][:300].copy()
    points[0, 1] = np.nan
    points[7, 2] = np.inf
    got, _ = _check(nn, points, 0.1)
    assert got[0] == 1 and 7 not in got


def test_everything_masked_out_gives_no_node(nn, cloud):
    got, rounds = _check(nn, cloud[0][:100], 0.1, mask=np.zeros(100, bool))
    assert len(got) == 0 and rounds == 0
    positions, indices = nn.sample_nodes(cloud[0][:100], np.zeros((100, 1), bool), 0.1, True, False)
    assert tuple(positions.shape) == (0, 3) and tuple(indices.shape) == (0, 1)


def test_mirror_sample_nodes(nn, cloud):
    """nnrt.sample_nodes: shapes and dtypes of the reference binding, the mask honoured only when asked for, and the
    seeded shuffle -- equal to the restatement under the same permutation and reproducible."""
    points, mask = cloud
    points, mask = points[:800], mask[:800]
    positions, indices = nn.sample_nodes(points, mask.reshape(-1, 1), 0.1, True, False)
    assert positions.dtype == torch.float32 and indices.dtype == torch.int32 and positions.is_cuda and indices.is_cuda
    assert tuple(indices.shape) == (positions.shape[0], 1) and positions.shape[1] == 3
    want = GU.sample_nodes(points, 0.1, mask)
    assert np.array_equal(_np(indices)[:, 0], want) and np.array_equal(_np(positions), points[want])
    _, unmasked = nn.sample_nodes(torch.from_numpy(points).cuda(), torch.from_numpy(mask).cuda(), 0.1, False, False)
    assert np.array_equal(_np(unmasked)[:, 0], GU.sample_nodes(points, 0.1))
    permutation = nn.graph_proc.shuffle_permutation(800, 123).numpy()
    assert np.array_equal(np.sort(permutation), np.arange(800)) and not np.array_equal(permutation, np.arange(800))
    _, shuffled = nn.sample_nodes(points, mask, 0.1, True, True, seed=123)
    _, shuffled_again = nn.sample_nodes(points, mask, 0.1, True, True, seed=123)
    assert torch.equal(shuffled, shuffled_again)
    assert np.array_equal(_np(shuffled)[:, 0], GU.sample_nodes(points, 0.1, mask, permutation))
    _check(nn, points, 0.1, mask=mask, order=permutation)
    _, fresh = nn.sample_nodes(points, mask, 0.1, True, True)   # seed=None: a fresh permutation, still a valid node set
    fresh = _np(fresh)[:, 0]
    assert mask[fresh].all() and not (GU.within(points[fresh][:, None], points[fresh][None], 0.1) & ~np.eye(len(fresh), dtype=bool)).any()


def test_graph_builder(nn):
    """build_deformation_graph_from_mesh: erosion -> sampling -> hierarchical warp field over the sampled nodes; a mesh that
    erodes to nothing raises."""
    from dynamicfuion_python_amd.nnrt import geometry as G
    from dynamicfuion_python_amd.warp_field import build_deformation_graph_from_mesh
    n = 24
    ys, xs = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    vertices = np.stack([xs * 0.02, ys * 0.02, 1.0 + 0.05 * np.sin(xs * 0.3)], axis=-1).reshape(-1, 3).astype(np.float32)
    quads = (ys[:-1, :-1] * n + xs[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([quads, quads + 1, quads + n], 1), np.stack([quads + 1, quads + n + 1, quads + n], 1)]).astype(np.int64)
    mesh = G.TriangleMesh(vertices, None, faces)
    wf = build_deformation_graph_from_mesh(mesh, 0.05, 2, 4, 8, 3)
    want = GU.sample_nodes(vertices, 0.05, GU.erosion_mask(len(vertices), faces, 2, 4))
    assert wf.node_count == len(want) > 8
    assert np.array_equal(wf.get_node_positions(), vertices[want])   # original (sampling) order
    with pytest.raises(ValueError, match="no graph node"):
        build_deformation_graph_from_mesh(mesh, 0.05, 100, 4, 8, 3)
