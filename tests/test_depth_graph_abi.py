"""CPU checks of the depth-image graph entry points (nnrt_compute_mesh_from_depth, nnrt_compute_edges_shortest_path,
nnrt_node_and_edge_clean_up, nnrt_compute_clusters): the host-side argument checks fail with NNRT_ERROR_ARGUMENT and a
message before anything is launched (device pointers are never dereferenced, so made-up addresses serve), the two host-code
passes equal the sequential restatement (tests/_depth_graph_util.py), and the nnrt mirror binds the names with the
reference's parameter names and order (cpp/pybind/nnrt_pybind.cpp:79-80, :143-153, :219-225). The checks that need the
device's data (face and node indices out of range, duplicate node vertices, a capacity the mesh exceeds) are in
tests/test_gpu_depth_graph.py."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import _depth_graph_util as DU

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


IMAGE, VERTICES, PIXELS, FACES, MASK, NODES, EDGES, WEIGHTS, DISTANCES = (0x100000 * i for i in range(1, 10))


def _mesh(native, image=_p(IMAGE), height=4, width=5, limit=0.05, vertices=_p(VERTICES), pixels=_p(PIXELS), vertex_capacity=20, faces=_p(FACES),
          face_capacity=24, counts=(True, True)):
    lib = native.lib()
    nv, nf = np.full(1, -1, np.int64), np.full(1, -1, np.int64)
    st = lib.nnrt_compute_mesh_from_depth(image, height, width, limit, vertices, pixels, vertex_capacity, faces, face_capacity,
                                          native.ptr(nv) if counts[0] else None, native.ptr(nf) if counts[1] else None, None)
    return st, lib.nnrt_last_error(), int(nv[0]), int(nf[0])


def _edges(native, vertices=_p(VERTICES), vertex_count=20, mask=_p(MASK), faces=_p(FACES), face_count=24, nodes=_p(NODES), node_count=3,
           neighbors=8, coverage=0.05, enforce=0, edges=_p(EDGES), weights=_p(WEIGHTS), distances=_p(DISTANCES)):
    lib = native.lib()
    passes = np.full(1, -1, np.int32)
    st = lib.nnrt_compute_edges_shortest_path(vertices, vertex_count, mask, faces, face_count, nodes, node_count, neighbors, coverage, enforce,
                                              edges, weights, distances, native.ptr(passes), None)
    return st, lib.nnrt_last_error(), int(passes[0])


@pytest.mark.parametrize("kwargs, message", [
    (dict(image=None), b"null"),
    (dict(vertices=None), b"null"),
    (dict(pixels=None), b"null"),
    (dict(faces=None), b"null"),
    (dict(counts=(False, True)), b"null"),
    (dict(counts=(True, False)), b"null"),
    (dict(height=-1), b"negative image size"),
    (dict(width=-1), b"negative image size"),
    (dict(height=1 << 15, width=1 << 15), b"image size"),
    (dict(vertex_capacity=-1), b"capacity"),
    (dict(face_capacity=-1), b"capacity"),
    (dict(vertices=_p(IMAGE + 16)), b"overlap"),
    (dict(pixels=_p(IMAGE - 8)), b"overlap"),
    (dict(faces=_p(IMAGE + 4 * 3 * 19)), b"overlap"),
])
def test_mesh_from_depth_refuses_bad_arguments(native, kwargs, message):
    st, msg, _, _ = _mesh(native, **kwargs)
    assert st == ARGUMENT
    assert msg.startswith(b"invalid argument") and message in msg


@pytest.mark.parametrize("height, width", [(0, 0), (1, 7), (7, 1), (0, 5)])
def test_mesh_from_depth_of_an_image_without_cells_is_empty_and_launches_nothing(native, height, width):
    """No device is needed: H < 2 or W < 2 returns two zero counts before any HIP call, whatever the capacities."""
    st, _, nv, nf = _mesh(native, height=height, width=width)
    assert (st, nv, nf) == (0, 0, 0)
    st, _, nv, nf = _mesh(native, height=height, width=width, vertices=None, pixels=None, faces=None, vertex_capacity=0, face_capacity=0)
    assert (st, nv, nf) == (0, 0, 0)


@pytest.mark.parametrize("kwargs, message", [
    (dict(vertices=None), b"null"),
    (dict(faces=None), b"null"),
    (dict(nodes=None), b"null"),
    (dict(edges=None), b"null"),
    (dict(weights=None), b"null"),
    (dict(distances=None), b"null"),
    (dict(vertex_count=-1), b"vertex count"),
    (dict(face_count=-1), b"face count"),
    (dict(face_count=(1 << 31) // 6), b"face count"),
    (dict(node_count=-1), b"node count"),
    (dict(neighbors=0), b"max_neighbor_count"),
    (dict(neighbors=-8), b"max_neighbor_count"),
    (dict(neighbors=1025), b"max_neighbor_count"),
    (dict(node_count=1 << 22, neighbors=1024), b"out of range"),
    (dict(coverage=0.0), b"node_coverage"),
    (dict(coverage=-0.05), b"node_coverage"),
    (dict(coverage=float("inf")), b"node_coverage"),
    (dict(coverage=float("nan")), b"node_coverage"),
])
def test_edges_shortest_path_refuses_bad_arguments(native, kwargs, message):
    st, msg, _ = _edges(native, **kwargs)
    assert st == ARGUMENT
    assert msg.startswith(b"invalid argument") and message in msg


def test_edges_shortest_path_without_nodes_succeeds(native):
    st, _, passes = _edges(native, nodes=None, node_count=0, edges=None, weights=None, distances=None)
    assert (st, passes) == (0, 0)


# ------------------------------------------------------------------------------------- the two host-code passes ----
def _clean_up(native, edges, valid, node_count=None, neighbors=None, null_edges=False, null_mask=False):
    lib = native.lib()
    e = np.ascontiguousarray(edges, np.int32)
    m = np.ascontiguousarray(valid, np.uint8).reshape(-1).copy()
    st = lib.nnrt_node_and_edge_clean_up(None if null_edges else native.ptr(e), e.shape[0] if node_count is None else node_count,
                                         e.shape[1] if neighbors is None else neighbors, None if null_mask else native.ptr(m))
    return st, lib.nnrt_last_error(), m.astype(bool)


def _clusters(native, edges, node_count=None, neighbors=None, null=()):
    lib = native.lib()
    e = np.ascontiguousarray(edges, np.int32)
    ids = np.full(max(e.shape[0], 1), -7, np.int32)
    sizes = np.full(max(e.shape[0], 1), -7, np.int32)
    count = np.full(1, -7, np.int64)
    args = dict(edges=native.ptr(e), ids=native.ptr(ids), sizes=native.ptr(sizes), count=native.ptr(count))
    args.update({k: None for k in null})
    st = lib.nnrt_compute_clusters(args["edges"], e.shape[0] if node_count is None else node_count, e.shape[1] if neighbors is None else neighbors,
                                   args["ids"], args["sizes"], args["count"])
    n = int(count[0])
    return st, lib.nnrt_last_error(), [int(s) for s in sizes[:max(n, 0)]], ids[: e.shape[0]].reshape(-1, 1)


def _row(*entries, K=4):
    return list(entries) + [-1] * (K - len(entries))


# a chain 0 - 1 - 2 - 3 - 4 hanging off a 4-clique 4 5 6 7 unravels one node per pass from its free end when the rows are
# visited in descending order of the chain, and in one pass when visited in ascending order: the result must be the same
CHAIN_ON_CLIQUE = np.array([_row(1), _row(0, 2), _row(1, 3), _row(2, 4), _row(3, 5, 6, 7), _row(4, 6, 7), _row(4, 5, 7), _row(4, 5, 6)], np.int32)
REVERSED_CHAIN = CHAIN_ON_CLIQUE[::-1].copy()
REVERSED_CHAIN[REVERSED_CHAIN >= 0] = 7 - REVERSED_CHAIN[REVERSED_CHAIN >= 0]
# entries after a row's first -1 are not neighbours: node 0 has one neighbour, node 3 two
MID_ROW_STOP = np.array([[1, -1, 2, 3], [0, 2, 3, -1], [0, 1, 3, -1], [1, 2, -1, 0]], np.int32)
TWO_COMPONENTS = np.array([_row(1, 2), _row(0, 2), _row(0, 1), _row(4, 5), _row(3, 5), _row(3, 4), _row()], np.int32)
ISOLATED = np.array([_row()], np.int32)
ONE_WAY = np.array([_row(3), _row(), _row(1), _row(), _row(5, 6), _row(4, 6), _row(4, 5)], np.int32)   # edges named by one side only
GRAPHS = {"chain_on_clique": CHAIN_ON_CLIQUE, "reversed_chain": REVERSED_CHAIN, "mid_row_stop": MID_ROW_STOP, "two_components": TWO_COMPONENTS,
          "isolated": ISOLATED, "one_way": ONE_WAY}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_node_and_edge_clean_up_matches_the_restatement(native, name):
    edges = GRAPHS[name]
    valid = np.ones(len(edges), bool)
    st, _, got = _clean_up(native, edges, valid)
    assert st == 0
    assert np.array_equal(got, DU.node_and_edge_clean_up(edges, valid))
    if name == "chain_on_clique":
        assert got.tolist() == [False] * 4 + [True] * 4
    if name == "reversed_chain":   # several passes in this visiting order, the same set
        assert got.tolist() == [True] * 4 + [False] * 4
    if name == "mid_row_stop":
        assert got.tolist() == [False, True, True, True]
    # a node that enters invalid stays invalid and still counts as a neighbour (the reference tests against the nodes this
    # call removed)
    valid[len(edges) // 2] = False
    st, _, got = _clean_up(native, edges, valid)
    assert st == 0 and np.array_equal(got, DU.node_and_edge_clean_up(edges, valid))


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_compute_clusters_matches_the_restatement(native, name):
    edges = GRAPHS[name]
    st, _, sizes, ids = _clusters(native, edges)
    want_sizes, want_ids = DU.compute_clusters(edges)
    assert st == 0
    assert sizes == want_sizes and np.array_equal(ids, want_ids)
    if name == "two_components":
        assert sizes == [3, 3, 1] and ids[:, 0].tolist() == [0, 0, 0, 1, 1, 1, 2]
    if name == "one_way":
        assert sizes == [2, 2, 3] and ids[:, 0].tolist() == [0, 1, 1, 0, 2, 2, 2]
    if name == "isolated":
        assert sizes == [1] and ids.tolist() == [[0]]


def test_host_passes_refuse_bad_arguments(native):
    edges = TWO_COMPONENTS
    ones = np.ones(len(edges), bool)
    for kwargs, message in [(dict(node_count=-1), b"node count"), (dict(neighbors=-1), b"max_neighbor_count"), (dict(null_edges=True), b"null"),
                            (dict(null_mask=True), b"null")]:
        st, msg, _ = _clean_up(native, edges, ones, **kwargs)
        assert st == ARGUMENT and msg.startswith(b"invalid argument") and message in msg
    for kwargs, message in [(dict(node_count=-1), b"node count"), (dict(neighbors=-1), b"max_neighbor_count"), (dict(null=("edges",)), b"null"),
                            (dict(null=("ids",)), b"null"), (dict(null=("sizes",)), b"null"), (dict(null=("count",)), b"null")]:
        st, msg, _, _ = _clusters(native, edges, **kwargs)
        assert st == ARGUMENT and msg.startswith(b"invalid argument") and message in msg
    for bad in (7, -2):
        broken = edges.copy()
        broken[1, 1] = bad
        st, msg, got = _clean_up(native, broken, ones)
        assert st == ARGUMENT and b"outside [-1, node_count)" in msg and got.all()   # refused before anything is cleared
        st, msg, _, _ = _clusters(native, broken)
        assert st == ARGUMENT and b"outside [-1, node_count)" in msg
    # no nodes: nothing to do
    assert _clean_up(native, np.zeros((0, 4), np.int32), np.zeros(0, bool), null_edges=True, null_mask=True)[0] == 0
    st, _, sizes, _ = _clusters(native, np.zeros((0, 4), np.int32), null=("edges", "ids", "sizes"))
    assert st == 0 and sizes == []


def test_mirror_host_passes_work_on_host_arrays_in_place():
    """nnrt.node_and_edge_clean_up updates a numpy mask or a torch tensor in place and returns it; nnrt.compute_clusters
    returns (list, (N, 1) int32). Neither needs a device for host inputs."""
    import torch
    from dynamicfuion_python_amd import nnrt
    mask = np.ones((8, 1), bool)
    assert nnrt.node_and_edge_clean_up(CHAIN_ON_CLIQUE, mask) is mask
    assert mask[:, 0].tolist() == [False] * 4 + [True] * 4
    tensor = torch.ones((8, 1), dtype=torch.bool)
    assert nnrt.node_and_edge_clean_up(torch.from_numpy(CHAIN_ON_CLIQUE), tensor) is tensor
    assert tensor[:, 0].tolist() == [False] * 4 + [True] * 4
    sizes, clusters = nnrt.compute_clusters(TWO_COMPONENTS)
    assert sizes == [3, 3, 1] and isinstance(sizes, list)
    assert clusters.dtype == np.int32 and clusters.shape == (7, 1) and clusters[:, 0].tolist() == [0, 0, 0, 1, 1, 1, 2]
    sizes, clusters = nnrt.compute_clusters(torch.from_numpy(TWO_COMPONENTS))
    assert sizes == [3, 3, 1] and clusters.dtype == torch.int32 and tuple(clusters.shape) == (7, 1)
    with pytest.raises(ValueError, match="entries for"):
        nnrt.node_and_edge_clean_up(CHAIN_ON_CLIQUE, np.ones(5, bool))


def test_mirror_binds_the_reference_names():
    from dynamicfuion_python_amd import nnrt
    mesh = list(inspect.signature(nnrt.compute_mesh_from_depth).parameters.values())
    assert [p.name for p in mesh] == ["point_image", "max_triangle_edge_distance"]
    assert all(p.default is inspect.Parameter.empty for p in mesh)
    masked, unmasked = (list(s.parameters.values()) for s in nnrt.compute_edges_shortest_path.signatures())
    assert [p.name for p in masked] == ["vertex_positions_in", "vertex_mask_in", "face_indices_in", "node_indices_in", "max_neighbor_count",
                                        "node_coverage", "enforce_total_num_neighbors"]
    assert [p.name for p in unmasked] == ["vertex_positions_in", "face_indices_in", "node_indices_in", "max_neighbor_count", "node_coverage",
                                          "enforce_total_num_neighbors"]
    assert all(p.default is inspect.Parameter.empty for p in masked + unmasked)
    assert [p.name for p in inspect.signature(nnrt.node_and_edge_clean_up).parameters.values()] == ["graph_edges", "valid_nodes_mask"]
    assert [p.name for p in inspect.signature(nnrt.compute_clusters).parameters.values()] == ["graph_edges_in"]
    with pytest.raises(TypeError, match="incompatible function arguments"):
        nnrt.compute_edges_shortest_path(np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32), np.zeros((1, 1), np.int32), 8, 0.05)


def test_graph_builder_signature_and_pipeline_parameters():
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.warp_field.graph_warp_field import build_graph_nodes_from_depth_image
    params = list(inspect.signature(build_graph_nodes_from_depth_image).parameters.values())
    assert [p.name for p in params[:3]] == ["depth", "mask", "intrinsic_matrix"]
    # create_graph_data.py:27-38, without device, scene_flow_path, enable_visual_debugging and minimum_valid_anchor_count
    assert [(p.name, p.default) for p in params[3:-1]] == [
        ("max_triangle_distance", 0.05), ("depth_scale_reciprocal", 1000.0), ("erosion_num_iterations", 10), ("erosion_min_neighbors", 4),
        ("remove_nodes_with_too_few_neighbors", True), ("use_only_valid_vertices", True), ("sample_random_shuffle", False), ("neighbor_count", 8),
        ("enforce_neighbor_count", True), ("node_coverage", 0.05)]
    assert params[-1].kind == inspect.Parameter.VAR_KEYWORD
    with pytest.raises(ValueError, match="scene_flow_path"):
        build_graph_nodes_from_depth_image(np.zeros((4, 4), np.uint16), None, np.eye(3), scene_flow_path="flow.sflow")
    with pytest.raises(TypeError, match="unexpected keyword"):
        build_graph_nodes_from_depth_image(np.zeros((4, 4), np.uint16), None, np.eye(3), enable_visual_debugging=True)
    p = F.FusionParameters()
    assert p.graph_generation_mode == F.GraphGenerationMode.FIRST_FRAME_LOADED_GRAPH   # the default stays
    assert p.graph_from_depth_image is False   # the depth-image mode is opt-in
    assert (p.graph_max_triangle_distance, p.graph_neighbor_count, p.graph_enforce_neighbor_count, p.graph_remove_nodes_with_too_few_neighbors,
            p.graph_use_only_valid_vertices, p.graph_sample_random_shuffle) == (0.05, 8, False, True, True, False)
    assert (p.graph_depth_image_erosion_iteration_count, p.graph_depth_image_erosion_min_neighbor_count) == (4, 4)
    assert (p.graph_erosion_iteration_count, p.graph_erosion_min_neighbor_count) == (10, 4)   # the mesh mode keeps its values
