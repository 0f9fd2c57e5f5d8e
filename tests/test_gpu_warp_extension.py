"""Extending the warp field over newly fused surface on the GPU (csrc/warp_extension.hip): the support kernel
bit for bit against the numpy restatement (tests/_warp_extension_util.py), the blend kernel against its float64
restatement within the measured bounds below, extend_warp_field on a small plane, and the fusion loop on a static
synthetic scene whose first frame shows only part of the surface."""
import functools

import numpy as np
import pytest

import _graph_util as GU
import _rigid_align_util as RU
import _warp_extension_util as WU

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C = 0.05

# 4 x the largest errors of k_blend_node_transforms against the float64 restatement over test_blend_accuracy's cases, as
# measured on an MI355X and recorded in DESIGN §18 ("Measured"); the margin covers float32 summation and exp rounding
# differences between compiler versions.
ROTATION_ERROR_BOUND = 4 * 2.195e-7        # max |R_new - R64|
TRANSLATION_ERROR_BOUND = 4 * 3.04e-8       # max |t_new - t64|, metres
ORTHOGONALITY_ERROR_BOUND = 4 * 1.916e-7    # max |R_new^T R_new - I|


@pytest.fixture(scope="module")
def f():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import nnrt
    return nnrt.geometry.functional


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# ---- support ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def support_points():
    """1,000 points in a 0.3 m box, one of them with a NaN coordinate; never modified."""
    p = np.random.default_rng(11).uniform(0.0, 0.3, (1000, 3)).astype(np.float32)
    p[123, 1] = np.nan
    return p


def support_nodes(count):
    """`count` nodes in the same box, node 0 two millimetres from point 7; from two nodes on, the last one repeats node 0
    (a tie at every point nearest to it, point 7 among them)."""
    rng = np.random.default_rng(100 + count)
    nodes = rng.uniform(0.0, 0.3, (count, 3)).astype(np.float32)
    if count >= 1:
        nodes[0] = support_points()[7] + np.float32([0.002, 0, 0])
        nodes[-1] = nodes[0]
    weights = rng.uniform(0.03 ** 2, 0.08 ** 2, count).astype(np.float32)
    weights[-1:] = weights[:1]
    return nodes, weights


@pytest.mark.parametrize("variable", [False, True], ids=["fixed", "variable"])
@pytest.mark.parametrize("node_count", [0, 1, 63, 64, 65, 257])
def test_vertex_support_is_bit_identical(f, node_count, variable):
    points = support_points()
    nodes, weights = support_nodes(node_count)
    ratio, nearest = f.compute_vertex_support(points, nodes, C, weights if variable else None)
    want_ratio, want_nearest = WU.vertex_support(points, nodes, C, weights if variable else None)
    ratio, nearest = _np(ratio), _np(nearest)
    assert ratio.dtype == np.float32 and nearest.dtype == np.int32 and ratio.shape == nearest.shape == (1000,)
    assert np.array_equal(ratio.view(np.uint32), want_ratio.view(np.uint32))
    assert np.array_equal(nearest, want_nearest)
    assert ratio[123] == 0 and nearest[123] == -1
    if node_count == 0:
        assert np.isposinf(np.delete(ratio, 123)).all() and (nearest == -1).all()
    if node_count >= 2:
        assert nearest[7] == 0 and not (nearest == node_count - 1).any()   # the lowest index wins the tie
    if node_count >= 1 and not variable:
        anchors, _ = f.compute_anchors_and_weights_euclidean_fixed_node_weight(points, nodes, 1, 0, C)
        supported = ratio <= 2
        assert supported.sum() > (100 if node_count > 1 else 1)
        assert np.array_equal(nearest[supported], _np(anchors)[supported, 0])


# ---- blend ------------------------------------------------------------------------------------------------------------------
def blend_case(M, N):
    rng = np.random.default_rng(1000 * M + N)
    nodes = rng.uniform(0.0, 0.3, (N, 3)).astype(np.float32)
    points = rng.uniform(0.0, 0.3, (M, 3)).astype(np.float32)
    rotations, translations = WU.random_motion(rng, N)
    return points, nodes, rotations, translations


@functools.lru_cache(maxsize=None)
def blend_reference(M, N, K):
    return WU.blend_node_transformations(*blend_case(M, N), K, C)


def test_blend_accuracy(f):
    """R_new, t_new and max |R^T R - I| against the float64 restatement, over M in {1, 65} x N in {1, 3, 200} x K in
    {1, 4, 8} (K > N included), rotations up to 60 degrees about random axes, translations up to 5 cm."""
    worst = dict(R=0.0, t=0.0, ortho=0.0)
    for M in (1, 65):
        for N in (1, 3, 200):
            for K in (1, 4, 8):
                R, t, fallbacks = f.blend_node_transformations(*blend_case(M, N), K, C)
                want_R, want_t, want_fallbacks = blend_reference(M, N, K)
                R, t = _np(R).astype(np.float64), _np(t).astype(np.float64)
                assert R.shape == (M, 3, 3) and t.shape == (M, 3) and fallbacks == want_fallbacks == 0
                e_R, e_t = np.abs(R - want_R).max(), np.abs(t - want_t).max()
                e_o = np.abs(np.einsum("mba,mbc->mac", R, R) - np.eye(3)).max()
                print(f"blend M {M} N {N} K {K}: max |R - R64| {e_R:.3g}, max |t - t64| {e_t:.3g}, max |R^T R - I| {e_o:.3g}")
                assert (np.linalg.det(R) > 0).all()
                worst = dict(R=max(worst["R"], e_R), t=max(worst["t"], e_t), ortho=max(worst["ortho"], e_o))
    print(f"blend worst: rotation {worst['R']:.4g}, translation {worst['t']:.4g}, orthogonality {worst['ortho']:.4g}")
    assert worst["R"] <= ROTATION_ERROR_BOUND and worst["t"] <= TRANSLATION_ERROR_BOUND and worst["ortho"] <= ORTHOGONALITY_ERROR_BOUND


def test_blend_is_deterministic_and_exact_on_the_identity(f):
    points, nodes, rotations, translations = blend_case(65, 200)
    first = f.blend_node_transformations(points, nodes, rotations, translations, 4, C)
    again = f.blend_node_transformations(points, nodes, rotations, translations, 4, C)
    assert np.array_equal(_np(first[0]), _np(again[0])) and np.array_equal(_np(first[1]), _np(again[1]))
    eye = np.tile(np.eye(3, dtype=np.float32), (len(nodes), 1, 1))
    for K in (1, 4, 8):
        R, t, fallbacks = f.blend_node_transformations(points, nodes, eye, np.zeros_like(nodes), K, C)
        assert fallbacks == 0 and np.array_equal(_np(R), eye[:65]) and np.array_equal(_np(t), np.zeros((65, 3), np.float32))


def test_blend_falls_back_on_opposite_rotations(f):
    """Two equidistant nodes whose rotations differ by 180 degrees: their average is singular; the lower-indexed node's
    rotation is returned and counted. A second query point next to node 1 alone blends normally."""
    nodes = np.float32([[-0.02, 0, 0], [0.02, 0, 0]])
    rotations = np.stack([WU.rotations_about([[0, 0, 1.0]], [30.0])[0], WU.rotations_about([[0, 0, 1.0]], [210.0])[0]]).astype(np.float32)
    translations = np.float32([[0.01, 0, 0], [0, 0.01, 0]])
    points = np.float32([[0, 0, 0], [0.3, 0, 0]])
    R, t, fallbacks = f.blend_node_transformations(points, nodes, rotations, translations, 4, C)
    want_R, want_t, want_fallbacks = WU.blend_node_transformations(points, nodes, rotations, translations, 4, C)
    assert fallbacks == want_fallbacks == 1
    assert np.array_equal(_np(R)[0], rotations[0])
    assert np.abs(_np(R)[1] - want_R[1]).max() <= ROTATION_ERROR_BOUND and np.abs(_np(t) - want_t).max() <= TRANSLATION_ERROR_BOUND


# ---- extend_warp_field --------------------------------------------------------------------------------------------------------
def ordering_factory(G):
    """FusionPipeline.make_warp_field's re-ordering toward the hierarchy's virtual order (quirk A5), returning the order."""
    def make(nodes):
        def build(n):
            return G.HierarchicalGraphWarpField(n, node_coverage=C, anchor_count=4, minimum_valid_anchor_count=0, layer_count=2)
        nodes = np.ascontiguousarray(nodes, np.float32)
        order = np.arange(len(nodes))
        wf = build(nodes)
        for _ in range(3):
            vidx = wf.get_virtual_node_indices()
            if np.array_equal(vidx, np.arange(len(nodes))):
                break
            nodes, order = nodes[vidx], order[vidx]
            wf = build(nodes)
        return wf, order
    return make


def test_extend_warp_field_on_a_plane(f):
    """A 12 x 12 vertex grid at spacing c / 2 with nodes over its left third."""
    from dynamicfuion_python_amd.nnrt import geometry as G
    from dynamicfuion_python_amd.warp_field import extend_warp_field
    xs = np.arange(12, dtype=np.float32) * np.float32(C / 2)
    vertices = np.stack([np.repeat(xs, 12), np.tile(xs, 12), np.full(144, 1.0, np.float32)], 1)   # x-major
    old_nodes = vertices[(np.repeat(np.arange(12), 12) % 2 == 0) & (np.tile(np.arange(12), 12) % 2 == 0) & (vertices[:, 0] < 0.09)]
    assert len(old_nodes) == 12
    make = ordering_factory(G)
    field, _ = make(old_nodes)
    N = field.node_count
    R_old, t_old = WU.random_motion(np.random.default_rng(5), N, 25.0, 0.02)
    field.set_node_rotations(R_old)
    field.set_node_translations(t_old)
    held = field.get_node_positions()

    extended, order, added = extend_warp_field(field, G.TriangleMesh(vertices, None, None), make)
    added = _np(added)
    M = len(added)
    assert extended is not field and M > 0 and extended.node_count == N + M and sorted(order) == list(range(N + M))
    everything = np.concatenate([held, added])
    assert np.array_equal(extended.get_node_positions(), everything[order])
    # old nodes keep their motion exactly
    is_old = order < N
    assert np.array_equal(extended.get_node_rotations()[is_old], R_old[order[is_old]])
    assert np.array_equal(extended.get_node_translations()[is_old], t_old[order[is_old]])
    # the new nodes are vertices beyond the old nodes' support and apart from each other
    assert all((vertices == a).all(axis=1).any() for a in added)
    assert (WU.vertex_support(added, held, C)[0] > 1.0).all()
    for i in range(M):
        others = np.delete(added, i, axis=0)
        assert not GU.within(others, added[i], C).any()
        assert (np.linalg.norm(others.astype(np.float64) - added[i], axis=1) >= C * (1 - 1e-6)).all()
    # their motion is the old field's at their positions
    R_new, t_new, _ = f.blend_node_transformations(added, held, R_old, t_old, 4, C)
    assert np.array_equal(extended.get_node_rotations()[~is_old], _np(R_new)[order[~is_old] - N])
    assert np.array_equal(extended.get_node_translations()[~is_old], _np(t_new)[order[~is_old] - N])
    assert (WU.vertex_support(vertices, everything, C)[0] <= 1.0).all()   # the whole grid is supported now
    again, order2, added2 = extend_warp_field(extended, vertices, make)
    assert again is extended and np.array_equal(order2, np.arange(N + M)) and tuple(added2.shape) == (0, 3)
    # a minimum the sampling does not reach leaves the field alone
    same, _, none = extend_warp_field(field, vertices, make, minimum_new_node_count=M + 1)
    assert same is field and tuple(none.shape) == (0, 3)


# ---- the fusion loop ----------------------------------------------------------------------------------------------------------
H, W, FRAMES = 192, 256, 5   # a pixel covers about one 5 mm voxel at the surface's 1.2 m
VISIBLE_X = -0.1   # the first frame shows the surface left of this; it reaches x = 0.6, 14 node coverages further


def write_sequence(directory):
    """A static scene: the analytic height field of the rigid-alignment tests seen from a fixed camera, FRAMES times; the
    first frame's depth is masked out right of VISIBLE_X."""
    from PIL import Image
    K = RU.intrinsics(H, W)
    points = RU.live_point_image(H, W, K)
    depth = np.round(points[..., 2].astype(np.float64) * 1000.0).astype(np.uint16)
    for i in range(FRAMES):
        d = np.where(points[..., 0] < VISIBLE_X, depth, 0).astype(np.uint16) if i == 0 else depth
        Image.fromarray(d).save(str(directory / f"depth_{i:04d}.png"))
        Image.fromarray(np.full((H, W, 3), 128, np.uint8)).save(str(directory / f"rgb_{i:04d}.png"))
    rows = [[K[0, 0], 0, K[0, 2], 0], [0, K[1, 1], K[1, 2], 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    (directory / "camera_intrinsics.txt").write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in rows) + "\n")


def run_pipeline(directory, extension):
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.data import frame as dfr
    seq = dfr.FrameSequenceDataset(base_dataset_type=dfr.DatasetType.CUSTOM, custom_frame_directory=str(directory)).load()
    params = F.FusionParameters(graph_generation_mode=F.GraphGenerationMode.FIRST_FRAME_EXTRACTED_MESH,
                                mesh_extraction_weight_thresholding_mode=F.MeshExtractionWeightThresholdingMode.CONSTANT,
                                mesh_extraction_weight_threshold=0, warp_field_extension=extension)
    params.alignment.max_iteration_count = 1
    params.alignment.guard_zero_rotation = True
    params.alignment.arap_term_weight = 20000.0   # nothing moves: a stiff graph keeps the fit at the sub-millimetre residuals' level
    pipe = F.FusionPipeline(seq, params)
    extents = []
    while seq.has_more_frames():
        pipe.process_frame(seq.get_next_frame())
        extents.append(float(_np(pipe.canonical_mesh.vertex_positions)[:, 0].max()))
    return pipe, extents


def test_fusion_pipeline_extends_its_graph(f, tmp_path):
    """Extension off and on over the same five frames. Off, the canonical mesh ends at x = -0.1, the edge of what the
    first frame showed, in every frame: the reference's non-rigid integration takes in no surface it first sees while
    tracking. On, the pipeline also switches the volume to set_non_rigid_surface_growth, the graph
    follows the fused surface and the surface the graph: measured on an MI355X, 156 -> 189 -> 210 -> 231 -> 259 nodes
    and a canonical mesh reaching x = -0.06, -0.01, 0.06, 0.125 after the four tracked frames."""
    write_sequence(tmp_path)
    off, off_extents = run_pipeline(tmp_path, False)
    on, on_extents = run_pipeline(tmp_path, True)
    print(f"canonical mesh max x per frame: off {off_extents}, on {on_extents}")
    print(f"node counts: off {[r.node_count for r in off.results]}, on {[r.node_count for r in on.results]}, "
          f"added {[r.new_node_count for r in on.results]}")
    assert len(off.results) == len(on.results) == FRAMES and all(r.tracked for r in on.results[1:])
    # off: the graph is the first frame's and the model stops growing a support radius beyond it
    assert len({r.node_count for r in off.results}) == 1 and off.results[0].node_count == off.active_graph.node_count > 0
    assert all(r.new_node_count == 0 for r in off.results)
    assert off_extents[-1] == off_extents[-2]
    assert 0.6 - off_extents[-1] > 4 * C   # the hidden part reaches well beyond what the first frame's nodes support
    # on: the same first frame, then nodes follow the fused surface and the surface follows the nodes
    assert on.results[0].node_count == off.results[0].node_count and on.results[0].new_node_count == 0
    assert on.results[-1].node_count > off.results[-1].node_count
    assert on.results[-1].node_count == on.active_graph.node_count == on.results[0].node_count + sum(r.new_node_count for r in on.results)
    assert np.isfinite(on.active_graph.get_node_rotations()).all() and np.isfinite(on.active_graph.get_node_translations()).all()
    # node_order indexes [the first frame's nodes; the added ones]
    assert sorted(on.node_order) == list(range(on.active_graph.node_count))
    first_frame_nodes = _np(on.sampled_node_positions)
    kept = on.node_order < len(first_frame_nodes)
    assert np.array_equal(on.active_graph.get_node_positions()[kept], first_frame_nodes[on.node_order[kept]])
    # the volume's switch: off, only the canonical frame's rigid integration ever counted an observation (T2); on, every
    # frame's does, and voxels right of the first frame's edge carry weight. The edge is taken 3 cm further right: a
    # free-space voxel in front of the surface (z down to 1.04 m against a surface at up to 1.25 m) projects onto surface
    # up to 1.2 times as far from the optical axis, so up to x = -0.083 voxels saw the first frame's surface
    off_voxels, on_voxels = _np(off.volume.extract_voxel_values_and_coordinates()), _np(on.volume.extract_voxel_values_and_coordinates())
    assert off_voxels[:, 4].max() == 1 and on_voxels[:, 4].max() == FRAMES
    assert not (off_voxels[off_voxels[:, 0] > VISIBLE_X + 0.03, 4] > 0).any()
    assert (on_voxels[on_voxels[:, 0] > VISIBLE_X + 0.03, 4] > 0).sum() > 1000
    # the model follows the graph along the revealed direction, frame after frame
    assert on_extents[-1] - off_extents[-1] >= C
    assert all(b > a for a, b in zip(on_extents, on_extents[1:]))
