"""Shortest-path anchors on the GPU (csrc/anchors_shortest_path.hip): bit-exact against the CPU restatement
(tests/_anchor_sp_util.py) through the mirror, the refusal of out-of-range edges, the behaviour the mode exists for (two
sheets), the fitter's set_anchor_graph and the fusion loop's AnchorComputationMode.SHORTEST_PATH.

Every bit-exact case first asserts on the CPU that no point's pops met a tie between two different nodes and that its
popped keys are distinct: the result then does not depend on the queue's internals ("Shortest-path anchors")."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _anchor_sp_util as U  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DD = os.path.join(GOLDEN, "deepdeform")
C = 0.1   # node coverage of the synthetic cases (= their node spacing)


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import _native
    _native.lib()
    from dynamicfuion_python_amd import nnrt
    return nnrt


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _points_near(nodes, count, seed):
    rng = np.random.default_rng(seed)
    lo, hi = nodes.min(0) - 0.5 * C, nodes.max(0) + 0.5 * C
    return rng.uniform(lo, hi, (count, 3)).astype(np.float32)


def _grid_case(K, D, V=257, seed=3):
    nodes = U.jittered_grid(15, 10, C, seed)
    return dict(points=_points_near(nodes, V, seed + 100), nodes=nodes, edges=U.knn_edge_rows(nodes, D), K=K)


def _components_case():
    # three disconnected components, the last with 3 nodes (< K = 6): a walk that starts there runs dry and seeds again
    parts = [U.jittered_grid(8, 8, C, 11), U.jittered_grid(6, 6, C, 12) + np.float32([1.2, 0, 0.3]),
             U.jittered_grid(3, 1, C, 13) + np.float32([0.3, 1.1, 0.0])]
    nodes = np.concatenate(parts).astype(np.float32)
    edges = np.full((len(nodes), 4), -1, np.int32)
    at = 0
    for p in parts:
        rows = U.knn_edge_rows(p, 4)
        edges[at:at + len(p)] = np.where(rows >= 0, rows + at, -1)
        at += len(p)
    points = np.concatenate([_points_near(p, 70, 20 + i) for i, p in enumerate(parts)])
    return dict(points=points, nodes=nodes, edges=edges, K=6)


def _dense_case():
    # K = 8, D = 8 on a dense cluster: up to 1 + 7 * 8 inserts per walk against a capacity of 40
    rng = np.random.default_rng(5)
    nodes = rng.uniform(0, 0.5, (200, 3)).astype(np.float32)
    return dict(points=rng.uniform(0, 0.5, (200, 3)).astype(np.float32), nodes=nodes, edges=U.knn_edge_rows(nodes, 8), K=8)


def _node_count_case(N):
    rng = np.random.default_rng(1000 + N)
    nodes = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    return dict(points=rng.uniform(0, 1, (100, 3)).astype(np.float32), nodes=nodes, edges=U.knn_edge_rows(nodes, 4), K=4)


def _variable_case():
    c = _grid_case(4, 4, V=200, seed=7)
    rng = np.random.default_rng(8)
    c["node_weights"] = (np.float32(C * C) * np.float32(10.0) ** rng.uniform(0, 1, len(c["nodes"]))).astype(np.float32)   # c^2 over a decade
    return c


def _few_nodes_case():
    nodes = np.array([[0, 0, 0], [0.1, 0.02, 0], [0.03, 0.12, 0.01]], np.float32)
    return dict(points=_points_near(nodes, 70, 31), nodes=nodes, edges=U.knn_edge_rows(nodes, 2), K=4)


def _empty_rows_case():
    nodes = U.jittered_grid(5, 4, C, 41)
    return dict(points=_points_near(nodes, 70, 42), nodes=nodes, edges=np.full((20, 3), -1, np.int32), K=4)


CASES = {f"grid-K{K}-D{D}": functools.partial(_grid_case, K, D) for K in (1, 4, 8) for D in (1, 4, 8)}
CASES.update({f"V{V}": functools.partial(_grid_case, 4, 4, V) for V in (1, 63, 64, 65, 130)})
CASES.update({f"N{N}": functools.partial(_node_count_case, N) for N in (63, 64, 65, 130)})
CASES.update(components=_components_case, dense=_dense_case, variable=_variable_case, few_nodes=_few_nodes_case, empty_rows=_empty_rows_case)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The case and its CPU restatement, computed once."""
    c = CASES[name]()
    a, w, popped, dropped, ties = U.shortest_path_anchors(c["points"], c["nodes"], c["edges"], c["K"], coverage=C, node_weights=c.get("node_weights"))
    assert U.keys_distinct(popped) and not ties.any(), f"{name}: a tie between two nodes' keys; pick another seed"
    for arr in (a, w):
        arr.setflags(write=False)
    return c, a, w, dropped


def _gpu(nn, c, points=None):
    f = nn.geometry.functional
    p = c["points"] if points is None else points
    if c.get("node_weights") is not None:
        a, w = f.compute_anchors_and_weights_shortest_path_variable_node_weight(p, c["nodes"], c["node_weights"], c["edges"], c["K"])
    else:
        a, w = f.compute_anchors_and_weights_shortest_path_fixed_node_weight(p, c["nodes"], c["edges"], c["K"], C)
    return _np(a), _np(w)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_exact_against_restatement(nn, name):
    c, a, w, dropped = _reference(name)
    a_g, w_g = _gpu(nn, c)
    assert a_g.dtype == np.int32 and w_g.dtype == np.float32 and a_g.shape == (len(c["points"]), c["K"])
    assert np.array_equal(a_g, a)
    assert np.array_equal(w_g, w)
    if name == "dense":
        assert dropped.any(), "the dense case is meant to fill the 40-entry queue"
    if name == "components":
        small = len(c["nodes"]) - 3
        started_small = a[:, 0] >= small
        assert started_small.any() and (a[started_small, 3:] < small).all() and (a[started_small, :3] >= small).all()
    if name == "few_nodes":
        assert (a[:, 3] == -1).all() and (a[:, :3] >= 0).all() and (w[:, 3] == 0).all()
    if name == "empty_rows":
        assert (a >= 0).all()   # one seed per anchor: the Euclidean order


def test_known_answer_case(nn):
    k = np.load(os.path.join(GOLDEN, "anchor_shortest_path_kat.npz"))
    a_r, w_r, popped, _, ties = U.shortest_path_anchors(k["points"], k["nodes"], k["edges"], 8, coverage=1.0)
    assert U.keys_distinct(popped) and not ties.any()
    a, w = nn.geometry.functional.compute_anchors_and_weights_shortest_path_fixed_node_weight(k["points"], k["nodes"], k["edges"], 8, 1.0)
    assert np.array_equal(_np(a), k["anchors"])
    assert np.allclose(_np(w), k["weights"])
    assert np.array_equal(_np(a), a_r) and np.array_equal(_np(w), w_r)


def test_no_nodes_and_no_points(nn):
    f = nn.geometry.functional
    a, w = f.compute_anchors_and_weights_shortest_path_fixed_node_weight(np.zeros((70, 3), np.float32), np.zeros((0, 3), np.float32),
                                                                         np.zeros((0, 4), np.int32), 4, C)
    assert (_np(a) == -1).all() and (_np(w) == 0.25).all() and a.shape == (70, 4)
    c = _reference("grid-K4-D4")[0]
    a, w = f.compute_anchors_and_weights_shortest_path_fixed_node_weight(np.zeros((0, 3), np.float32), c["nodes"], c["edges"], 4, C)
    assert a.shape == (0, 4) and w.shape == (0, 4)


def test_point_image(nn):
    c, a, w, _ = _reference("grid-K4-D4")
    img = np.ascontiguousarray(c["points"][:63].reshape(7, 9, 3))
    a_g, w_g = _gpu(nn, c, img)
    assert a_g.shape == (7, 9, 4) and w_g.shape == (7, 9, 4)
    assert np.array_equal(a_g.reshape(63, 4), a[:63]) and np.array_equal(w_g.reshape(63, 4), w[:63])


def test_argument_checks(nn):
    f = nn.geometry.functional
    c = _reference("grid-K4-D4")[0]
    with pytest.raises(RuntimeError):
        f.compute_anchors_and_weights_shortest_path_fixed_node_weight(c["points"], c["nodes"], c["edges"], 0, C)
    with pytest.raises(RuntimeError):
        f.compute_anchors_and_weights_shortest_path_fixed_node_weight(c["points"], c["nodes"], c["edges"].astype(np.int64), 4, C)
    with pytest.raises(RuntimeError):
        f.compute_anchors_and_weights_shortest_path_fixed_node_weight(c["points"], c["nodes"], c["edges"][:-1], 4, C)
    with pytest.raises(RuntimeError):
        f.compute_anchors_and_weights_shortest_path_fixed_node_weight(c["points"][:, :2], c["nodes"], c["edges"], 4, C)
    with pytest.raises(RuntimeError):
        f.compute_anchors_and_weights_shortest_path_fixed_node_weight(c["points"], c["nodes"], c["edges"], 9, C)   # MAX_ANCHORS


def test_out_of_range_edge_is_refused_and_writes_nothing(nn):
    from dynamicfuion_python_amd import _native as N
    c = _reference("grid-K4-D4")[0]
    edges = c["edges"].copy()
    edges[17, 2] = len(c["nodes"])   # one past the last node
    dev = torch.device("cuda")
    p, n, e = (torch.as_tensor(x, device=dev) for x in (c["points"], c["nodes"], edges))
    a = torch.full((len(c["points"]), 4), -7, dtype=torch.int32, device=dev)
    w = torch.full((len(c["points"]), 4), 0.5, dtype=torch.float32, device=dev)
    st = N.lib().nnrt_compute_anchors_and_weights_shortest_path(N.ptr(p), p.shape[0], N.ptr(n), n.shape[0], N.ptr(e), 4, 4, C, None, N.ptr(a),
                                                                 N.ptr(w), N.stream_ptr())
    torch.cuda.synchronize()
    assert st == 1 and b"edge" in N.lib().nnrt_last_error()
    assert (_np(a) == -7).all() and (_np(w) == 0.5).all()
    with pytest.raises(N.NnrtError):
        nn.geometry.functional.compute_anchors_and_weights_shortest_path_fixed_node_weight(c["points"], c["nodes"], edges, 4, C)


def _two_sheets():
    """Two parallel 6 x 6 sheets 1.5 c apart, nodes on a c-spaced grid with 4-neighbour edges inside a sheet only; the
    points are the sheets themselves on a c / 2 grid that reaches c / 2 past the outermost nodes. A point past a corner has
    its own sheet's corner node at 0.71 c, two more at 1.58 c, and then the other sheet's corner node at 1.66 c, closer
    than its own sheet's fourth (2.12 c): Euclidean anchoring crosses the gap there."""
    n = 6
    gx, gy = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    flat = np.stack([gx.ravel() * C, gy.ravel() * C], axis=1)
    nodes = np.concatenate([np.c_[flat, np.zeros(n * n)], np.c_[flat, np.full(n * n, 1.5 * C)]]).astype(np.float32)
    edges = np.full((2 * n * n, 4), -1, np.int32)
    for s in range(2):
        for i in range(n):
            for j in range(n):
                nb = [(i + di, j + dj) for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)) if 0 <= i + di < n and 0 <= j + dj < n]
                edges[s * n * n + i * n + j, :len(nb)] = [s * n * n + a * n + b for a, b in nb]
    m = 2 * n + 1
    px, py = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    pflat = np.stack([(px.ravel() - 1) * C / 2, (py.ravel() - 1) * C / 2], axis=1)
    points = np.concatenate([np.c_[pflat, np.zeros(m * m)], np.c_[pflat, np.full(m * m, 1.5 * C)]]).astype(np.float32)
    return points, nodes, edges, m * m, n * n


def test_anchors_stay_on_their_sheet(nn, oracle_mod):
    points, nodes, edges, per_sheet, nodes_per_sheet = _two_sheets()
    sheet_of_point = (np.arange(len(points)) >= per_sheet).astype(np.int64)
    a_r, w_r, _, _, _ = U.shortest_path_anchors(points, nodes, edges, 4, coverage=C)
    assert ((a_r >= nodes_per_sheet) == sheet_of_point[:, None]).all()            # the restatement: own sheet only
    a_e, w_e = oracle_mod.compute_anchors(points, nodes, 4, C)
    crossing = ((a_e >= nodes_per_sheet) != sheet_of_point[:, None]).any(axis=1)
    assert crossing.any()                                                          # Euclidean: some point reaches across
    f = nn.geometry.functional
    a, w = f.compute_anchors_and_weights_shortest_path_fixed_node_weight(points, nodes, edges, 4, C)
    assert np.array_equal(_np(a), a_r) and np.array_equal(_np(w), w_r)             # the regular grid has ties: the index rule on both sides
    # move the upper sheet's nodes: the lower sheet's points stay where they are under the shortest-path anchors
    R = np.tile(np.eye(3, dtype=np.float32), (len(nodes), 1, 1))
    t = np.zeros((len(nodes), 3), np.float32)
    t[nodes_per_sheet:] = [0.0, 0.0, 0.5 * C]
    mesh = nn.geometry.TriangleMesh(points, None, np.zeros((0, 3), np.int64))
    moved = _np(f.warp_triangle_mesh(mesh, nodes, R, t, a, w).vertex_positions)
    lower = sheet_of_point == 0
    # sum_k w_k (g_k + (p - g_k)) with |p|, |g| < 1: a few float32 roundings of values below 1, far under 1e-6
    assert np.abs(moved[lower] - points[lower]).max() < 1e-6
    assert np.allclose(moved[~lower] - points[~lower], [0, 0, 0.5 * C], rtol=0, atol=1e-6)
    moved_e = _np(f.warp_triangle_mesh(mesh, nodes, R, t, torch.as_tensor(a_e), torch.as_tensor(w_e)).vertex_positions)
    assert np.abs(moved_e[lower] - points[lower]).max() > 1e-3                     # the Euclidean anchors drag the lower sheet along


# ---------------------------------------------------------------------------------------------------------------------
# fitter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def s1(oracle_mod):
    from dynamicfuion_python_amd import synthetic as S
    from _util import scene_target
    sc = S.make_scene("S1", seed=0, hierarchy_builder=lambda n, c, l: oracle_mod.build_hierarchy(n, c, l))
    return sc, scene_target(oracle_mod, sc)


def _fitter(nn, sc):
    G, A = nn.geometry, nn.alignment
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, sc.layer_count)
    ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001)
    return wf, ft, G.TriangleMesh(sc.points, sc.normals, sc.faces)


def _iterate_from_ground_truth(sc, wf, ft):
    wf.set_node_rotations(sc.gt_rotations)
    wf.set_node_translations(sc.gt_translations)
    R0, t0 = wf.get_node_rotations(True), wf.get_node_translations(True)
    ft.iterate(wf, 0, 1)
    ft.check()
    return R0, t0


def test_fitter_anchor_graph(nn, oracle_mod, s1):
    sc, depth = s1
    V = len(sc.points)
    wf, ft, mesh = _fitter(nn, sc)
    nodes_v = wf.get_node_positions(True)
    edges = U.knn_edge_rows(nodes_v, 4)
    ft.set_anchor_graph(edges)
    ft.prepare(wf, mesh, depth, None, sc.K)
    a, w = ft.anchors(V, 4)
    a_s, w_s = nn.geometry.functional.compute_anchors_and_weights_shortest_path_fixed_node_weight(sc.points, nodes_v, edges, 4, sc.coverage)
    assert np.array_equal(a, _np(a_s)) and np.array_equal(w, _np(w_s))
    a_e, _ = nn.geometry.functional.compute_anchors_and_weights_euclidean_fixed_node_weight(sc.points, nodes_v, 4, 0, sc.coverage)
    assert not np.array_equal(np.sort(a, axis=1), np.sort(_np(a_e), axis=1))       # the graph changes some vertex's anchor set
    R0, t0 = _iterate_from_ground_truth(sc, wf, ft)
    p_g, n_g = ft.warped_mesh(V)
    p_o, n_o = oracle_mod.warp_mesh(sc.points, sc.normals, nodes_v, R0, t0, a, w)
    assert np.array_equal(p_g, p_o) and np.array_equal(n_g, n_o)
    assert np.isfinite(ft.diagnostics()["updates"]).all()
    # a graph over another node count is refused at prepare(); an out-of-range entry when it is set
    ft.set_anchor_graph(U.knn_edge_rows(nodes_v[:-1], 4))
    with pytest.raises(RuntimeError, match="node_count"):
        ft.prepare(wf, mesh, depth, None, sc.K)
    bad = edges.copy()
    bad[0, 0] = len(nodes_v)
    with pytest.raises(RuntimeError, match="edge"):
        ft.set_anchor_graph(bad)
    # back to Euclidean: the same anchors and the same iteration as a fitter that never had a graph
    ft.set_anchor_graph(None)
    wf.reset_rotations()
    wf.set_node_translations(np.zeros((len(nodes_v), 3), np.float32))
    ft.prepare(wf, mesh, depth, None, sc.K)
    wf2, ft2, _ = _fitter(nn, sc)
    ft2.prepare(wf2, mesh, depth, None, sc.K)
    a1, w1 = ft.anchors(V, 4)
    a2, w2 = ft2.anchors(V, 4)
    assert np.array_equal(a1, a2) and np.array_equal(w1, w2) and np.array_equal(a1, _np(a_e))
    _iterate_from_ground_truth(sc, wf, ft)
    _iterate_from_ground_truth(sc, wf2, ft2)
    assert np.array_equal(ft.diagnostics()["updates"], ft2.diagnostics()["updates"])
    assert np.array_equal(wf.get_node_translations(True), wf2.get_node_translations(True))


# ---------------------------------------------------------------------------------------------------------------------
# fusion loop
# ---------------------------------------------------------------------------------------------------------------------
def test_fusion_pipeline_shortest_path(nn):
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.data import frame as dfr
    seq = dfr.FrameSequenceDataset(17, dfr.DataSplit.TEST, base_dataset_type=dfr.DatasetType.LOCAL, base_directory=DD, frame_indices=[300, 600])
    params = F.FusionParameters(anchor_computation_mode=F.AnchorComputationMode.SHORTEST_PATH)
    params.alignment.max_iteration_count = 1
    pipe = F.FusionPipeline(seq, params)
    pipe.process_frame(seq.get_next_frame())
    wf = pipe.active_graph
    canonical = pipe.canonical_mesh
    nodes_v, weights_v = wf.get_node_positions(True), wf.get_node_coverage_weights()
    edges_v = pipe.anchor_graph_edges
    # the re-indexed rows describe the file's graph: the same node positions at both ends of every edge
    file_nodes, file_edges = seq.load_graph_data(seq.get_current_graph_name())[:2]
    assert edges_v.shape == file_edges.shape and (edges_v >= 0).sum() == (file_edges >= 0).sum() > 0

    def position_pairs(nodes, rows):
        return sorted((tuple(nodes[i]), tuple(nodes[t])) for i in range(len(rows)) for t in rows[i] if t >= 0)
    assert position_pairs(nodes_v, edges_v) == position_pairs(file_nodes, file_edges)
    res = pipe.process_frame(seq.get_next_frame())
    assert res.tracked
    V = canonical.vertex_positions.shape[0]
    a, w = pipe.optimizer.fitter.anchors(V, 4)
    f = nn.geometry.functional
    a_s, w_s = f.compute_anchors_and_weights_shortest_path_variable_node_weight(canonical.vertex_positions, nodes_v, weights_v, edges_v, 4)
    assert np.array_equal(a, _np(a_s)) and np.array_equal(w, _np(w_s))
    a_e, _ = f.compute_anchors_and_weights_euclidean_variable_node_weight(canonical.vertex_positions, nodes_v, weights_v, 4, 0)
    assert (np.sort(a, axis=1) != np.sort(_np(a_e), axis=1)).any(axis=1).sum() >= 1
    t = wf.get_node_translations(True)
    assert np.isfinite(t).all() and np.abs(t).max() > 1e-3
