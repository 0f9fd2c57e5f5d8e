"""csrc/depth_graph.hip against the sequential restatement (tests/_depth_graph_util.py): the pixel-connected depth mesh
(bit-exact: vertices, pixels, faces, numbering and order), the geodesic node edges (ids and distances bit-exact, weights
against the float64 formula on those distances), the builder and FusionPipeline with FIRST_FRAME_DEPTH_IMAGE on the
committed seq017 frames 300 -> 600 (tests/golden/deepdeform).

Every edge test asserts that the distances of the first K + 1 nodes reached from each source are pairwise distinct, so the
rule that orders equal distances (node index here, heap state in the reference) decides nothing. Weight tolerance: one
float32 exp (<= 2 ulp), at most seven additions and one division give about 12 * 2^-24 = 7e-7 relative; the tests allow
2e-6."""
import os

import numpy as np
import pytest

import _depth_graph_util as DU
import _graph_util as GU

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deepdeform")
COVERAGE = 0.05
WEIGHT_RTOL = 2e-6


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import nnrt
    return nnrt


def point_image(H, W, seed, spacing=0.006, holes=None):
    """Smoothly varying random depth around 1 m (no planes: no equal geodesic distances), back-projected with a pinhole
    whose pixels lie `spacing` apart at 1 m; z = 0 and a zero point where `holes` is set."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z = np.ones((H, W))
    for _ in range(4):
        a, b, ph = rng.uniform(0.05, 0.25, 2).tolist() + [rng.uniform(0, 6.28)]
        z += rng.uniform(0.01, 0.03) * np.sin(a * u + b * v + ph)
    z += rng.uniform(-2e-4, 2e-4, (H, W))
    if holes is not None:
        z[holes] = 0
    p = np.stack([(u - W / 2) * spacing * z, (v - H / 2) * spacing * z, z], -1).astype(np.float32)
    p[z == 0] = 0
    return p


def _island_holes(H=45, W=70):
    holes = np.zeros((H, W), bool)   # an L of invalid pixels cuts the bottom-left corner off: a component of 7 nodes
    holes[28, :16] = True
    holes[28:, 16] = True
    return holes


def _mesh_cases():
    cases = {"9x17": (point_image(9, 17, 1), 0.05), "45x70": (point_image(45, 70, 7, holes=_island_holes()), 0.05),
             "2x2": (point_image(2, 2, 2), 0.05), "h1": (point_image(1, 9, 3), 0.05), "w1": (point_image(9, 1, 4), 0.05),
             "all_invalid": (np.zeros((6, 11, 3), np.float32), 0.05)}
    single = np.zeros((5, 7, 3), np.float32)
    single[2:4, 3:5] = point_image(2, 2, 5)
    single[3, 4] = 0   # only triangle (00, 01, 10) of cell (3, 2) is left
    cases["single_triangle"] = (single, 0.05)
    yy, xx = np.meshgrid(np.arange(12), np.arange(19), indexing="ij")
    cases["checkerboard"] = (point_image(12, 19, 6, holes=(yy % 3 == 1) & (xx % 3 == 1)), 0.05)
    step = point_image(10, 13, 8)
    far = (xx[:10, :13] + yy[:10, :13]) > 11   # a depth step along an anti-diagonal: on one side of it a cell keeps only its
    step[far] *= np.float32(1.5)               # first triangle, on the other only its second
    cases["diagonal_step"] = (step, 0.05)
    nan = point_image(9, 17, 9)
    nan[4, 8, 2] = np.nan
    cases["nan_pixel"] = (nan, 0.05)
    tight = point_image(9, 17, 10)
    cases["tight_threshold"] = (tight, float(np.quantile(DU.edge_length(tight[1:, :-1], tight[:-1, 1:]), 0.8)))   # a fifth of the diagonals fail
    return cases


MESH_CASES = _mesh_cases()


def _assert_mesh_equal(got, want):
    vertices, pixels, faces = (_np(t) for t in got)
    assert vertices.dtype == np.float32 and pixels.dtype == np.int32 and faces.dtype == np.int32
    assert vertices.shape == want[0].shape and pixels.shape == want[1].shape and faces.shape == want[2].shape
    assert np.array_equal(vertices.view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(pixels, want[1])
    assert np.array_equal(faces, want[2])


@pytest.mark.parametrize("name", sorted(MESH_CASES))
def test_mesh_from_depth_is_bit_exact(nn, name):
    image, limit = MESH_CASES[name]
    want = DU.mesh_from_depth(image, limit)
    expected_faces = {"2x2": 2, "h1": 0, "w1": 0, "all_invalid": 0, "single_triangle": 1}
    if name in expected_faces:
        assert len(want[2]) == expected_faces[name]
    elif name == "9x17":
        assert len(want[2]) == 2 * 8 * 16   # every triangle passes
    else:
        assert 0 < len(want[2]) < 2 * (image.shape[0] - 1) * (image.shape[1] - 1)   # some triangles fail, some pass
    if name == "diagonal_step":   # cells with only the first and cells with only the second triangle exist
        per_cell = np.bincount(want[1][want[2][:, 0], 1] * 13 + want[1][want[2][:, 0], 0], minlength=130)
        assert (per_cell == 1).any()
    got = nn.compute_mesh_from_depth(image, limit)
    _assert_mesh_equal(got, want)
    assert all(t.is_cuda for t in got)
    _assert_mesh_equal(nn.compute_mesh_from_depth(torch.from_numpy(image).cuda(), limit), want)


def test_mesh_from_depth_refuses_other_inputs_and_small_capacities(nn):
    from dynamicfuion_python_amd import _native as N
    image, limit = MESH_CASES["9x17"]
    for bad in (image.astype(np.float64), image[..., :2], image.reshape(-1, 3), torch.from_numpy(image).to(torch.float16)):
        with pytest.raises(ValueError, match="point image"):
            nn.compute_mesh_from_depth(bad, limit)
    want = DU.mesh_from_depth(image, limit)
    nv, nf = len(want[0]), len(want[2])
    p = torch.from_numpy(image).cuda()
    guard = 0x7F
    for vcap, fcap in ((nv - 1, nf), (nv, nf - 1), (0, 0)):
        vertices = torch.full((nv + 4, 3), guard, dtype=torch.float32, device="cuda")
        pixels = torch.full((nv + 4, 2), guard, dtype=torch.int32, device="cuda")
        faces = torch.full((nf + 4, 3), guard, dtype=torch.int32, device="cuda")
        counts = np.full(2, -1, np.int64)
        st = N.lib().nnrt_compute_mesh_from_depth(N.ptr(p), 9, 17, limit, N.ptr(vertices), N.ptr(pixels), vcap, N.ptr(faces), fcap,
                                                  N.ptr(counts[0:1]), N.ptr(counts[1:2]), N.stream_ptr())
        assert st == 1 and b"capacity" in N.lib().nnrt_last_error()
        assert counts.tolist() == [0, 0]
        assert bool((vertices == guard).all()) and bool((pixels == guard).all()) and bool((faces == guard).all())   # nothing written
    # the exact capacity is enough
    vertices = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    pixels = torch.empty((nv, 2), dtype=torch.int32, device="cuda")
    faces = torch.empty((nf, 3), dtype=torch.int32, device="cuda")
    counts = np.full(2, -1, np.int64)
    N.check(N.lib().nnrt_compute_mesh_from_depth(N.ptr(p), 9, 17, limit, N.ptr(vertices), N.ptr(pixels), nv, N.ptr(faces), nf, N.ptr(counts[0:1]),
                                                 N.ptr(counts[1:2]), N.stream_ptr()))
    assert counts.tolist() == [nv, nf]
    _assert_mesh_equal((vertices, pixels, faces), want)


# ------------------------------------------------------------------------------------------ committed frame ----
@pytest.fixture(scope="module")
def frame300(nn):
    """The committed depth frame back-projected on the GPU with the committed intrinsics, and the restatement's mesh of it."""
    from dynamicfuion_python_amd.data import camera as dcam
    from dynamicfuion_python_amd.data import io as dio
    depth = dio.load_depth_image(os.path.join(DD, "test", "seq017", "depth", "000300.png"))
    fx, fy, cx, cy = dcam.load_intrinsic_matrix_entries_from_text_4x4_matrix(os.path.join(DD, "test", "seq017", "intrinsics.txt"))
    points = _np(nn.backproject_depth_ushort(depth, fx, fy, cx, cy, 1000.0))
    return depth, (fx, fy, cx, cy), points, DU.mesh_from_depth(points, 0.05)


def test_mesh_from_depth_on_the_committed_frame(nn, frame300):
    _, _, points, want = frame300
    assert len(want[0]) > 200000 and len(want[2]) > 400000
    _assert_mesh_equal(nn.compute_mesh_from_depth(points, 0.05), want)


# ---------------------------------------------------------------------------------------------------- edges ----
def _check_edges(nn, vertices, faces, node_indices, K, enforce, vertex_mask=None):
    """Runs both the mirror and the restatement; returns (edges, counts) after asserting ids, distances and weights."""
    want_e, _, want_d, first = DU.edges_shortest_path(vertices, faces, node_indices, K, COVERAGE, enforce, vertex_mask)
    for i, reached in first.items():
        assert len(set(reached)) == len(reached), f"node {i}: equal distances among its first K + 1 nodes; the input is unfit"
    if vertex_mask is None:
        got = nn.compute_edges_shortest_path(vertices, faces, node_indices, K, COVERAGE, enforce)
    else:
        got = nn.compute_edges_shortest_path(vertices, vertex_mask, faces, node_indices, K, COVERAGE, enforce)
    assert len(got) == 4 and got[3] is None
    edges, weights, distances = (_np(t) for t in got[:3])
    assert edges.dtype == np.int32 and weights.dtype == np.float32 and distances.dtype == np.float32
    assert edges.shape == weights.shape == distances.shape == (len(node_indices), K)
    assert np.array_equal(edges, want_e)
    assert np.array_equal(distances.view(np.uint32), want_d.view(np.uint32))
    counts = (want_e >= 0).sum(axis=1)
    want_w = DU.weights_from_distances(want_d, counts, COVERAGE)
    assert np.all(np.abs(weights - want_w) <= WEIGHT_RTOL * want_w)
    assert np.all(weights[want_e < 0] == 0)
    return edges, counts


@pytest.fixture(scope="module")
def synthetic(nn):
    image, limit = MESH_CASES["45x70"]
    vertices, pixels, faces = DU.mesh_from_depth(image, limit)
    eroded = GU.erosion_mask(len(vertices), faces, 1, 4)
    cut = ~((pixels[:, 0] >= 40) & (pixels[:, 0] <= 41))   # two masked-out pixel columns split the surface
    return vertices, pixels, faces, eroded, cut


@pytest.mark.parametrize("K", [8, 2])
@pytest.mark.parametrize("enforce", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_edges_shortest_path_on_the_synthetic_mesh(nn, synthetic, K, enforce, masked):
    vertices, pixels, faces, eroded, cut = synthetic
    sample_mask = eroded & cut if masked else eroded
    _, node_indices = nn.sample_nodes(vertices, sample_mask.reshape(-1, 1), COVERAGE, True, False)
    node_indices = _np(node_indices)
    assert np.array_equal(node_indices[:, 0], GU.sample_nodes(vertices, COVERAGE, sample_mask))
    assert len(node_indices) == 63
    edges, counts = _check_edges(nn, vertices, faces, node_indices, K, enforce, cut if masked else None)
    node_pixels = pixels[node_indices[:, 0]]
    island = (node_pixels[:, 0] < 16) & (node_pixels[:, 1] > 28)
    assert island.sum() == 7   # fewer than K + 1 = 9 nodes: with K = 8 the enforced mode ends there by exhaustion
    if K == 8:
        assert counts[~island].max() == 8
        if enforce:
            assert np.all(counts[island] == 6) and np.all(counts[~island] == 8)
        else:
            assert counts.min() < 6   # the radius leaves some rows short
    else:
        assert np.all(counts == 2)
    assert np.all(island[edges[island][edges[island] >= 0]])   # no edge leaves the island
    if masked:
        left = node_pixels[:, 0] < 40
        for i in range(len(edges)):
            named = edges[i][edges[i] >= 0]
            assert np.all(left[named] == left[i])   # no edge crosses the masked columns


def test_edges_shortest_path_refuses_bad_indices_and_skips_negative_nodes(nn, synthetic):
    from dynamicfuion_python_amd._native import NnrtError
    vertices, _, faces, eroded, _ = synthetic
    nodes = GU.sample_nodes(vertices, COVERAGE, eroded).astype(np.int32)
    for bad in (-1, len(vertices)):
        broken = faces.copy()
        broken[100, 1] = bad
        with pytest.raises(NnrtError, match="face index outside"):
            nn.compute_edges_shortest_path(vertices, broken, nodes, 8, COVERAGE, False)
    beyond = nodes.copy()
    beyond[5] = len(vertices)
    with pytest.raises(NnrtError, match="outside \\[0, vertex_count\\)"):
        nn.compute_edges_shortest_path(vertices, faces, beyond, 8, COVERAGE, False)
    twice = nodes.copy()
    twice[9] = twice[3]
    with pytest.raises(NnrtError, match="duplicate node vertex"):
        nn.compute_edges_shortest_path(vertices, faces, twice, 8, COVERAGE, False)
    # a negative node index: an all-default row, and no other node sees it (graph_proc.cpp:232-237, :253)
    skipped = nodes.copy()
    skipped[4] = -1
    edges, counts = _check_edges(nn, vertices, faces, skipped.reshape(-1, 1), 8, False)
    assert counts[4] == 0 and not (edges == 4).any()
    # no faces: every row default
    got = nn.compute_edges_shortest_path(vertices, np.zeros((0, 3), np.int32), nodes, 8, COVERAGE, True)
    assert bool((got[0] == -1).all()) and bool((got[1] == 0).all()) and bool((got[2] == 0).all())


def test_edges_shortest_path_on_a_crop_of_the_committed_frame(nn, frame300):
    _, _, points, _ = frame300
    crop = np.ascontiguousarray(points[180:300, 240:400])   # 160 x 120
    got = nn.compute_mesh_from_depth(crop, 0.05)
    want = DU.mesh_from_depth(crop, 0.05)
    _assert_mesh_equal(got, want)
    vertices, _, faces = want
    mask = nn.get_vertex_erosion_mask(vertices, faces, 4, 4)
    assert np.array_equal(_np(mask)[:, 0], GU.erosion_mask(len(vertices), faces, 4, 4))
    _, node_indices = nn.sample_nodes(vertices, mask, COVERAGE, True, False)
    node_indices = _np(node_indices)
    assert len(node_indices) == 78
    _check_edges(nn, vertices, faces, node_indices, 8, False)


# ------------------------------------------------------------------------------------- builder and pipeline ----
def test_fusion_pipeline_builds_its_graph_from_the_first_depth_image(nn, frame300):
    from dynamicfuion_python_amd.data import frame as dfr
    from dynamicfuion_python_amd import fusion as F
    _, _, _, (vertices, pixels, faces) = frame300   # seq017 has no masks and no far clipping: the loaded frame is the frame
    seq = dfr.FrameSequenceDataset(17, dfr.DataSplit.TEST, base_dataset_type=dfr.DatasetType.LOCAL, base_directory=DD,
                                   frame_indices=[300, 600])
    with pytest.raises(NotImplementedError, match="graph_from_depth_image=True"):   # the mode is opt-in
        F.FusionPipeline(seq, F.FusionParameters(graph_generation_mode=F.GraphGenerationMode.FIRST_FRAME_DEPTH_IMAGE))
    params = F.FusionParameters(graph_generation_mode=F.GraphGenerationMode.FIRST_FRAME_DEPTH_IMAGE, graph_from_depth_image=True)
    params.alignment.max_iteration_count = 1
    pipe = F.FusionPipeline(seq, params)
    assert not seq.has_masks() and seq.far_clipping_distance_mm == 0
    pipe.process_frame(seq.get_next_frame())

    g = pipe.depth_image_graph
    _assert_mesh_equal((g.vertices, g.vertex_pixels, g.faces), (vertices, pixels, faces))
    assert np.array_equal(_np(pipe.graph_source_mesh.vertex_positions), vertices)
    assert np.array_equal(_np(pipe.graph_source_mesh.triangle_indices), faces)
    eroded = GU.erosion_mask(len(vertices), faces, 4, 4)
    assert np.array_equal(_np(g.non_eroded_vertices)[:, 0], eroded)
    sampled = GU.sample_nodes(vertices, params.node_coverage, eroded)
    # the nodes the builder kept: the sampled ones minus those the clean-up removed, in sampling order
    got_edges, got_weights, got_distances, _ = nn.compute_edges_shortest_path(vertices, faces, sampled.astype(np.int32), 8, params.node_coverage,
                                                                             False)
    rows = np.linspace(0, len(sampled) - 1, 8).astype(int).tolist()
    want_e, _, want_d, first = DU.edges_shortest_path(vertices, faces, sampled, 8, params.node_coverage, False, rows=rows)
    for i in rows:
        assert len(set(first[i])) == len(first[i])
        assert np.array_equal(_np(got_edges)[i], want_e[i])
        assert np.array_equal(_np(got_distances)[i].view(np.uint32), want_d[i].view(np.uint32))
    counts = (want_e[rows] >= 0).sum(axis=1)
    want_w = DU.weights_from_distances(want_d[rows], counts, params.node_coverage)
    assert np.all(np.abs(_np(got_weights)[rows] - want_w) <= WEIGHT_RTOL * want_w)
    # the rest of the builder on those edges: clean-up, compaction, clusters (restatement: create_graph_data.py:162-285)
    all_edges = _np(got_edges)
    valid = DU.node_and_edge_clean_up(all_edges, np.ones(len(sampled), bool))
    assert 0 < valid.sum() <= len(sampled)
    kept = sampled[valid]
    assert np.array_equal(_np(pipe.sampled_node_vertex_indices)[:, 0], kept)
    assert np.array_equal(_np(pipe.sampled_node_positions), vertices[kept])
    e, w, d = DU.compact_graph(all_edges, _np(got_weights), _np(got_distances), valid)
    assert np.array_equal(_np(pipe.geodesic_edges), e)
    assert np.array_equal(_np(g.edge_distances).view(np.uint32), d.view(np.uint32))
    assert np.all(np.abs(_np(g.edge_weights) - w) <= WEIGHT_RTOL * w)   # a row sum in another order and one division
    sizes, clusters = DU.compute_clusters(e)
    assert g.cluster_sizes == sizes and np.array_equal(_np(pipe.graph_clusters), clusters)
    assert min(sizes) > 2

    wf = pipe.active_graph
    assert wf.node_count == len(kept)
    held = wf.get_node_positions()   # make_warp_field only re-orders: the warp field holds the cleaned node set
    assert np.array_equal(held[np.lexsort(held.T)], vertices[kept][np.lexsort(vertices[kept].T)])

    res = pipe.process_frame(seq.get_next_frame())
    assert res.tracked
    t = wf.get_node_translations(True)
    assert np.isfinite(t).all() and np.abs(t).max() > 0
    assert not seq.has_more_frames()


def test_builder_masks_the_depth_and_refuses_degenerate_graphs(nn, frame300):
    from dynamicfuion_python_amd.warp_field.graph_warp_field import build_graph_nodes_from_depth_image
    depth, (fx, fy, cx, cy), points, _ = frame300
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    mask = np.zeros(depth.shape, np.uint8)
    mask[180:300, 240:400] = 255
    g = build_graph_nodes_from_depth_image(depth, mask, K, erosion_num_iterations=4, enforce_neighbor_count=False)
    masked_points = np.where(mask[..., None] > 0, points, np.float32(0))
    _assert_mesh_equal((g.vertices, g.vertex_pixels, g.faces), DU.mesh_from_depth(masked_points, 0.05))
    assert g.node_positions.shape[0] == g.edges.shape[0] == g.clusters.shape[0] > 20 and g.edges.shape[1] == 8
    assert np.array_equal(_np(g.node_positions), _np(g.vertices)[_np(g.node_vertex_indices)[:, 0]])
    assert int(g.edges.max()) < g.edges.shape[0] and sum(g.cluster_sizes) == g.edges.shape[0]
    assert np.allclose(_np(g.edge_weights).sum(axis=1), 1.0, atol=1e-6)
    with pytest.raises(ValueError, match="no mesh"):
        build_graph_nodes_from_depth_image(depth, np.zeros_like(mask), K)
    tiny = np.zeros_like(mask)
    tiny[200:206, 300:306] = 1   # a 6 x 6 patch erodes to nothing
    with pytest.raises(ValueError, match="no graph node"):
        build_graph_nodes_from_depth_image(depth, tiny, K)
