"""GPU parity of the TSDF voxel block grid (csrc/tsdf_grid.hpp and the tsdf_*.hip sources) beyond the two scenes of test_gpu_tsdf.py: every storage
pair, block resolution 16, a real camera pose, a separate colour camera, anchor counts 1 ... 8 with every minimum, variable
node coverage, the candidate-list limits, several frames, growth mode, the hash table under growth and after a refused
call -- all bit for bit against the oracle restatement (oracle/tsdf_oracle.cpp) -- and marching cubes against plain numpy.
Inputs are 64 x 48 frames from _tsdf_util.small_tsdf_scene. Every scene pins exact counts (COUNTS and the literals next to
the cases): they were taken from the oracle alone, run on the CPU (it is deterministic), so that no comparison can pass
on an empty volume."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _tsdf_util as TU  # noqa: E402

EYE = np.eye(4)


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import nnrt
    return nnrt


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


class Field:
    """Warp-field inputs of one case: camera-space nodes with their motion and the anchor rule."""

    def __init__(self, nodes, R, t, coverage, K=4, min_valid=1, variable=False):
        self.nodes, self.R, self.t = np.ascontiguousarray(nodes, np.float32), np.ascontiguousarray(R, np.float32), np.ascontiguousarray(t, np.float32)
        self.coverage, self.K, self.min_valid, self.variable = coverage, K, min_valid, variable
        self.c2 = None   # squared per-node coverage (variable coverage): the HIP field's own on the GPU, the oracle's on the CPU


def scene_field(sc, K=4, min_valid=1, variable=False):
    nodes, R, t = sc.nodes, sc.rotations, sc.translations
    if variable:   # a 21st node 0.3 m behind the surface: its coverage (distance to the nearest other node) is ~4x the others'
        nodes = np.vstack([nodes, [[-0.05, 0.04, 0.82]]]).astype(np.float32)
        R = np.concatenate([R, R[:1]])
        t = np.vstack([t, t[:1]])
    return Field(nodes, R, t, sc.coverage, K, min_valid, variable)


class OracleSide:
    def __init__(self, O, voxel, res, wdt, cdt, field, growth=False, capacity=None):
        self.O, self.f, self.growth = O, field, growth
        self.g = O.OracleGrid(voxel, res, wdt, cdt)
        if field is not None and field.variable and field.c2 is None:
            field.c2 = O.node_coverage_weights(field.nodes, field.coverage)

    def touch(self, depth, K, E, sc):
        return self.g.touch(depth, K, E, sc.depth_scale, sc.depth_max, sc.trunc_mult)

    def activate(self, coords):
        self.g.activate(coords)

    def integrate(self, blocks, depth, color, Kd, Kc, E, sc):
        self.g.integrate(blocks, depth, color, Kd, Kc, E, sc.depth_scale, sc.depth_max, sc.trunc_mult)

    def find(self, depth, Kd, E, sc):
        f = self.f
        return self.g.find_blocks_intersecting_truncation_region(depth, f.nodes, f.R, f.t, f.coverage, f.K, f.min_valid, Kd, E, sc.depth_scale,
                                                                 sc.depth_max, sc.trunc_mult)

    def nonrigid(self, blocks, depth, color, normals, Kd, Kc, E, sc):
        f = self.f
        return self.g.integrate_non_rigid(blocks, f.nodes, f.R, f.t, f.coverage, f.K, f.min_valid, depth, color, normals, Kd, Kc, E,
                                          sc.depth_scale, sc.depth_max, sc.trunc_mult, node_coverage_sq=f.c2, grow_surface=self.growth)

    def boxes(self, keys, E):
        f = self.f
        return self.O.warped_block_boxes(keys, self.g.res * self.g.voxel, f.nodes, f.R, f.t, f.coverage, f.K, f.min_valid, E)

    def values(self):
        return self.g.values_all()

    def values_at(self, q):
        return self.g.values_at(q)

    def coords(self):
        return self.g.block_coords()

    def mesh(self, threshold):
        V, Nn, C, T = self.g.mesh(threshold)
        return [V, Nn, C if self.g.color else None, T]

    def sleeve(self):
        nb = self.g.inactive_neighbors()
        self.g.activate(nb)
        return len(nb)


class GpuSide:
    def __init__(self, nn, voxel, res, wdt, cdt, field, growth=False, capacity=16):
        G = nn.geometry
        self.f = field
        names, dts, ch = ["tsdf", "weight"], ["float32", wdt], [1, 1]
        if cdt != "none":
            names, dts, ch = names + ["color"], dts + [cdt], ch + [3]
        self.g = G.NonRigidSurfaceVoxelBlockGrid(names, dts, ch, voxel, res, capacity)
        self.has_color = cdt != "none"
        if growth:
            self.g.set_non_rigid_surface_growth(True)
        self.wf = None
        if field is not None:
            method = G.WarpNodeCoverageComputationMethod.MINIMAL_K_NEIGHBOR_NODE_DISTANCE if field.variable else \
                G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE
            self.wf = G.HierarchicalGraphWarpField(field.nodes, field.coverage, True, field.K, field.min_valid, method, 1)
            self.wf.set_node_rotations(field.R)
            self.wf.set_node_translations(field.t)
            # one layer: the field's own (virtual) node order is the input order, so both sides search the same node list
            assert np.array_equal(self.wf.get_node_positions(True), field.nodes)
            assert np.array_equal(self.wf.get_node_rotations(True), field.R) and np.array_equal(self.wf.get_node_translations(True), field.t)
            if field.variable:
                field.c2 = self.wf.get_node_coverage_weights().copy()   # the oracle then reads the HIP field's own weights

    def touch(self, depth, K, E, sc):
        return _np(self.g.compute_unique_block_coordinates(depth, K, E, sc.depth_scale, sc.depth_max, sc.trunc_mult))

    def activate(self, coords):
        self.g.activate(coords)

    def integrate(self, blocks, depth, color, Kd, Kc, E, sc):
        if color is None:
            self.g.integrate(blocks, depth, Kd, E, sc.depth_scale, sc.depth_max, sc.trunc_mult)
        else:
            self.g.integrate(blocks, depth, color, Kd, Kc, E, sc.depth_scale, sc.depth_max, sc.trunc_mult)

    def find(self, depth, Kd, E, sc):
        return _np(self.g.find_blocks_intersecting_truncation_region(depth, self.wf, Kd, E, sc.depth_scale, sc.depth_max, sc.trunc_mult))

    def nonrigid(self, blocks, depth, color, normals, Kd, Kc, E, sc):
        return _np(self.g.integrate_non_rigid(blocks, self.wf, depth, color, normals, Kd, Kc, E, sc.depth_scale, sc.depth_max, sc.trunc_mult))

    def boxes(self, keys, E):
        return _np(self.g.get_bounding_boxes_of_warped_blocks(keys, self.wf, E))

    def values(self):
        return _np(self.g.extract_voxel_values_and_coordinates())

    def values_at(self, q):
        return _np(self.g.extract_voxel_values_at(q))

    def coords(self):
        return _np(self.g.get_block_coordinates())

    def mesh(self, threshold=None):
        m = self.g.extract_triangle_mesh() if threshold is None else self.g.extract_triangle_mesh(threshold, -1)
        return [_np(m.vertex_positions), _np(m.vertex_normals), _np(m.vertex_colors) if self.has_color else None, _np(m.triangle_indices)]

    def sleeve(self):
        return self.g.activate_sleeve_blocks()


def pipeline(side, sc, sc2, E=EYE, Kc=None, color_hw=None, with_color=True, thresholds=(0.0,), extra_frames=()):
    """touch, rigid integrate (of sc and of every extra frame), truncation-region search, non-rigid integrate of the second
    frame sc2, values, block coordinates, meshes, sleeve activation: every stage's result by name."""
    out = {}

    def color_of(s):
        if not with_color:
            return None
        if color_hw is None:
            return s.color
        return np.ascontiguousarray(s.color[:color_hw[0], :color_hw[1]])
    Kc = sc.K if Kc is None else Kc
    out["touch"] = b = side.touch(sc.depth, sc.K, E, sc)
    side.integrate(b, sc.depth, color_of(sc), sc.K, Kc, E, sc)
    for i, fr in enumerate(extra_frames):
        out[f"touch_frame{i + 1}"] = bf = side.touch(fr.depth, fr.K, E, fr)
        side.integrate(bf, fr.depth, color_of(fr), fr.K, Kc, E, fr)
    out["rigid"] = side.values()
    out["found"] = nb = side.find(sc2.depth, sc.K, E, sc2)
    out["cos"] = side.nonrigid(nb, sc2.depth, color_of(sc2), sc2.normals, sc.K, Kc, E, sc2)
    out["nonrigid"] = side.values()
    out["coords"] = side.coords()
    for th in thresholds:
        out[f"mesh{th:g}"] = side.mesh(th)
    out["sleeve_n"] = side.sleeve()
    out["sleeve_coords"] = side.coords()
    return out


def changed_voxels(before, after):
    """voxels whose tsdf or weight the non-rigid pass changed (blocks it activated start at zero)"""
    pad = np.zeros((len(after), 2), np.float32)
    pad[:len(before)] = before[:, 3:5]
    return int((pad != after[:, 3:5]).any(1).sum())


def counts(out):
    """(blocks touched, voxels with weight > 0 after the rigid pass, non-zero cosine pixels, voxels changed by the
    non-rigid pass, sleeve blocks, triangles per threshold ...)"""
    tri = tuple(len(v[3]) for k, v in out.items() if k.startswith("mesh"))
    return (len(out["touch"]), int((out["rigid"][:, 4] > 0).sum()), int((out["cos"] != 0).sum()), changed_voxels(out["rigid"], out["nonrigid"]),
            int(out["sleeve_n"])) + tri


def assert_same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        if k.startswith("mesh"):
            for name, a, b in zip(("vertices", "normals", "colors", "triangles"), got[k], want[k]):
                assert (a is None) == (b is None), (k, name)
                if b is not None:
                    assert a.shape == b.shape and np.array_equal(a, b), (k, name)
        else:
            assert np.array_equal(got[k], want[k]), k


def scenes(O, u16=False, rough=False, seed=0):
    """the frame that is integrated rigidly and the (1 cm farther) frame of the non-rigid pass"""
    return TU.small_tsdf_scene(O, seed, u16=u16, rough=rough), TU.small_tsdf_scene(O, seed, u16=u16, rough=rough, depth_shift=0.01)


def both(nn, O, sc, field_args, grid_args, growth=False, **kw):
    """the pipeline on the GPU and in the oracle; returns (gpu results, oracle results)"""
    res, wdt, cdt = grid_args
    fg, fo = scene_field(sc[0], **field_args), scene_field(sc[0], **field_args)
    gpu = GpuSide(nn, sc[0].voxel_size, res, wdt, cdt, fg, growth)
    fo.c2 = fg.c2
    orc = OracleSide(O, sc[0].voxel_size, res, wdt, cdt, fo, growth)
    return pipeline(gpu, sc[0], sc[1], **kw), pipeline(orc, sc[0], sc[1], **kw)


# ---- storage and resolution ------------------------------------------------------------------------------------------
STORAGE = [(w, c) for w in ("float32", "uint16") for c in ("none", "float32", "uint16", "uint8")]
# counts(): from the oracle on the CPU, one row per (depth type, block resolution); the storage types do not change them
STORAGE_COUNTS = {
    (False, 8): (43, 10171, 2434, 851, 632, 2595), (True, 8): (43, 10165, 2434, 846, 632, 2588),
    (False, 16): (14, 15325, 2528, 937, 246, 2606), (True, 16): (14, 15318, 2528, 932, 246, 2599),
}


@pytest.mark.parametrize("res", [8, 16])
@pytest.mark.parametrize("u16", [False, True], ids=["depth_f32", "depth_u16"])
@pytest.mark.parametrize("wdt,cdt", STORAGE)
def test_storage_pairs_and_resolutions(nn, oracle_mod, wdt, cdt, u16, res):
    """Every (weight, color) storage pair with float32 and uint16 depth at block resolutions 8 and 16 (a grid without
    color is integrated without a color image), every stage against the oracle."""
    sc = scenes(oracle_mod, u16=u16)
    got, want = both(nn, oracle_mod, sc, {}, (res, wdt, cdt), with_color=cdt != "none")
    assert counts(want) == STORAGE_COUNTS[(u16, res)]
    assert_same(got, want)


# ---- pose and cameras ------------------------------------------------------------------------------------------------
POSE_COUNTS = {8: (46, 10357, 2469, 777, 630, 2693), 16: (12, 12090, 2515, 805, 218, 2693)}   # counts(): from the oracle on the CPU
# counts() + (voxels observed with / without a color pixel): from the oracle on the CPU
COLOR_CAMERA_COUNTS = {False: (43, 10171, 2434, 851, 632, 2595, 7669, 2502), True: (43, 10165, 2434, 846, 632, 2588, 7665, 2500)}
COLOR_K = np.array([[60.0, 0.0, 20.0], [0.0, 60.0, 15.0], [0.0, 0.0, 1.0]])


@pytest.mark.parametrize("res", [8, 16])
def test_camera_pose(nn, oracle_mod, res):
    """A real extrinsic (10 degrees about y and a translation) through touch, both integrations, the truncation-region
    search and the warped block boxes."""
    O = oracle_mod
    E = TU.extrinsic_about_y()
    sc = scenes(O)
    got, want = both(nn, O, sc, {}, (res, "float32", "float32"), E=E)
    assert counts(want) == POSE_COUNTS[res]
    assert_same(got, want)
    # the pose matters: the same frames under the identity pose touch other blocks
    assert not np.array_equal(want["touch"], OracleSide(O, sc[0].voxel_size, res, "float32", "none", None).touch(sc[0].depth, sc[0].K, EYE, sc[0]))
    f = scene_field(sc[0])
    keys = np.array([[0, 0, 0], [-1, 0, 0], [0, -1, 1], [1, 1, 0], [0, 0, 1]], np.int32)
    assert np.array_equal(GpuSide(nn, sc[0].voxel_size, res, "float32", "none", f).boxes(keys, E),
                          OracleSide(O, sc[0].voxel_size, res, "float32", "none", f).boxes(keys, E))


@pytest.mark.parametrize("u16", [False, True], ids=["depth_f32", "depth_u16"])
def test_color_camera_of_its_own(nn, oracle_mod, u16):
    """Color intrinsics that differ from the depth camera's and a 40 x 30 color image: some observed voxels' color pixel
    falls outside it and keeps color 0."""
    sc = scenes(oracle_mod, u16=u16)
    got, want = both(nn, oracle_mod, sc, {}, (8, "float32", "float32"), Kc=COLOR_K, color_hw=(30, 40))
    seen = want["rigid"][:, 4] > 0
    colored = (want["rigid"][:, 5:] != 0).any(1)
    assert counts(want) + (int((seen & colored).sum()), int((seen & ~colored).sum())) == COLOR_CAMERA_COUNTS[u16]
    assert (seen & colored).any() and (seen & ~colored).any()
    assert_same(got, want)


# ---- anchors ---------------------------------------------------------------------------------------------------------
ANCHOR_CASES = sorted({(K, m) for K in (1, 2, 3, 5, 8) for m in (0, 2, K)} - {(1, 2)})
# counts(): from the oracle on the CPU
ANCHOR_COUNTS = {
    (1, 0): (43, 10171, 2459, 10009, 632, 2661), (1, 1): (43, 10171, 2459, 10009, 632, 2661),
    (2, 0): (43, 10171, 2437, 9987, 632, 2602), (2, 2): (43, 10171, 2437, 9987, 632, 2602),
    (3, 0): (43, 10171, 2420, 9928, 632, 2595), (3, 2): (43, 10171, 2420, 9928, 632, 2595), (3, 3): (43, 10171, 2420, 9928, 632, 2595),
    (5, 0): (43, 10171, 2421, 9958, 632, 2567), (5, 2): (43, 10171, 2421, 9958, 632, 2567), (5, 5): (43, 10171, 2412, 9809, 632, 2574),
    (8, 0): (43, 10171, 2421, 9973, 632, 2570), (8, 2): (43, 10171, 2421, 9973, 632, 2570), (8, 8): (43, 10171, 1979, 7230, 632, 2633),
}


@pytest.mark.parametrize("K,min_valid", ANCHOR_CASES)
def test_anchor_counts_and_minimums(nn, oracle_mod, K, min_valid):
    """k_integrate_non_rigid<K> and k_warped_block_boxes<K> (through the truncation-region search) at K = 1, 2, 3, 5, 8
    with minimum_valid_anchor_count 0, 2 and K, in growth mode so that the blended position decides most voxels."""
    sc = scenes(oracle_mod)
    got, want = both(nn, oracle_mod, sc, dict(K=K, min_valid=min_valid), (8, "float32", "float32"), growth=True)
    assert counts(want) == ANCHOR_COUNTS[(K, min_valid)]
    assert counts(want)[3] > 0   # the non-rigid pass changed voxels
    assert_same(got, want)


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8])
def test_minimum_above_anchor_count(nn, oracle_mod, K):
    """minimum_valid_anchor_count = K + 1: no voxel can qualify. The warp field refuses such a minimum at construction
    (as the reference's anchor computation does), so the kernels never see it; the oracle, given it, changes no voxel."""
    O, G = oracle_mod, nn.geometry
    sc = scenes(O)
    with pytest.raises(RuntimeError):
        G.HierarchicalGraphWarpField(sc[0].nodes, sc[0].coverage, True, K, K + 1, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, 1)
    want = pipeline(OracleSide(O, sc[0].voxel_size, 8, "float32", "float32", scene_field(sc[0], K=K, min_valid=K + 1), True), sc[0], sc[1])
    assert changed_voxels(want["rigid"], want["nonrigid"]) == 0 and not want["cos"].any()


# counts(): from the oracle on the CPU
VARIABLE_COUNTS = {(4, False): (43, 10171, 2435, 847, 632, 2593), (4, True): (43, 10171, 2435, 9940, 632, 2591),
                   (8, True): (43, 10171, 2425, 9959, 632, 2584)}


@pytest.mark.parametrize("K,growth", [(4, False), (4, True), (8, True)])
def test_variable_node_coverage(nn, oracle_mod, K, growth):
    """Per-node coverage (the node_weights branch of anchors_finish and the search range from the largest weight) with one
    node whose coverage is about four times the others'."""
    sc = scenes(oracle_mod)
    fg = scene_field(sc[0], K=K, min_valid=2, variable=True)
    got, want = both(nn, oracle_mod, sc, dict(K=K, min_valid=2, variable=True), (8, "float32", "float32"), growth=growth)
    c2 = oracle_mod.node_coverage_weights(fg.nodes, fg.coverage)
    assert c2[20] > 9 * np.median(c2[:20])   # squared coverage: more than 3x the others'
    assert counts(want) == VARIABLE_COUNTS[(K, growth)]
    assert counts(want)[3] > 0
    assert_same(got, want)


BOX_KEYS = np.array([[x, y, z] for x in (-1, 0) for y in (-1, 0, 1) for z in (0, 1)], np.int32)


def box_field(n, K, coverage, seed):
    """nodes spread over the metric range of BOX_KEYS' corners (the reference takes the integer key as the corner)"""
    rng = np.random.default_rng(seed)
    return Field(rng.uniform(-1.3, 2.3, (n, 3)), TU.rotation_vectors_to_matrices(rng.normal(0, 0.05, (n, 3))),
                 rng.uniform(-0.02, 0.02, (n, 3)), coverage, K, 0)


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8])
def test_warped_block_boxes_anchor_counts(nn, oracle_mod, K):
    f = box_field(400, K, 0.3, K)
    # from the inputs: corners with more than K nodes in range (the K-NN has to choose) and with fewer than K
    corners = (BOX_KEYS[:, None, :] + np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])[None] * np.float32(0.08)).reshape(-1, 3)
    near = (np.linalg.norm(corners[:, None, :] - f.nodes[None], axis=2) <= 2 * f.coverage).sum(1)
    assert (near > K).any() and (near.min() < 8)
    got = GpuSide(nn, 0.01, 8, "float32", "none", f).boxes(BOX_KEYS, TU.extrinsic_about_y(4.0, (0.01, 0.02, -0.01)))
    want = OracleSide(oracle_mod, 0.01, 8, "float32", "none", f).boxes(BOX_KEYS, TU.extrinsic_about_y(4.0, (0.01, 0.02, -0.01)))
    assert np.array_equal(got, want)
    assert (want[:, 3:] > want[:, :3]).all(1).any()   # boxes with an extent: corners moved by their anchors


# ---- candidate limits ------------------------------------------------------------------------------------------------
CANDIDATE_COUNTS = {2048: (292, 579), 2049: (283, 576), 2100: (297, 573)}   # (non-zero cosine pixels, voxels changed): from the oracle on the CPU


@pytest.mark.parametrize("n_nodes", [2048, 2049, 2100])
def test_candidate_list_limit(nn, oracle_mod, n_nodes):
    """Two blocks with 2048, 2049 and 2100 nodes all in anchor range of every voxel: the LDS candidate list holds 2048, so
    the last two take the overflow path (every node searched from global memory)."""
    O = oracle_mod
    sc, sc2 = scenes(O)
    blocks = np.array([[0, 0, 6], [-1, 0, 6]], np.int32)
    rng = np.random.default_rng(n_nodes)
    nodes = (np.array([0.0, 0.035, 0.515]) + rng.uniform(-0.015, 0.015, (n_nodes, 3))).astype(np.float32)
    f = Field(nodes, TU.rotation_vectors_to_matrices(rng.normal(0, 0.03, (n_nodes, 3))), rng.uniform(-0.004, 0.004, (n_nodes, 3)), 0.15, 4, 1)
    # from the inputs: every node is within 2 c of every voxel of both blocks, so the in-range count of a block is n_nodes
    vox = (blocks[:, None, :] * 8 + np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3)[None]).reshape(-1, 3) * np.float32(0.01)
    far = max(np.linalg.norm(vox[i::64, None, :] - nodes[None], axis=2).max() for i in range(64))
    assert far < 2 * f.coverage * 0.99
    assert (n_nodes > 2048) == (n_nodes != 2048)
    res = []
    for side in (GpuSide(nn, sc.voxel_size, 8, "float32", "float32", f, True), OracleSide(O, sc.voxel_size, 8, "float32", "float32", f, True)):
        side.integrate(blocks, sc.depth, sc.color, sc.K, sc.K, EYE, sc)
        before = side.values()
        cos = side.nonrigid(np.zeros((0, 3), np.int32), sc2.depth, sc2.color, sc2.normals, sc.K, sc.K, EYE, sc2)
        res.append((before, cos, side.values(), side.coords()))
    (b0, c0, v0, k0), (b1, c1, v1, k1) = res
    assert (int((c1 != 0).sum()), changed_voxels(b1, v1)) == CANDIDATE_COUNTS[n_nodes]
    assert np.array_equal(b0, b1) and np.array_equal(c0, c1) and np.array_equal(v0, v1) and np.array_equal(k0, k1)


@pytest.mark.parametrize("n_nodes", [4096, 4097])
def test_warped_block_boxes_node_staging_limit(nn, oracle_mod, n_nodes):
    """4096 nodes are staged in LDS, 4097 are read from global memory."""
    f = box_field(n_nodes, 4, 0.12, n_nodes)
    got = GpuSide(nn, 0.01, 8, "float32", "none", f).boxes(BOX_KEYS[:5], EYE)
    want = OracleSide(oracle_mod, 0.01, 8, "float32", "none", f).boxes(BOX_KEYS[:5], EYE)
    assert np.array_equal(got, want) and (want[:, 3:] > want[:, :3]).all(1).any()


# ---- several frames --------------------------------------------------------------------------------------------------
FRAMES_COUNTS = (43, 10944, 2447, 895, 650, 2577, 2554, 2450, 0, 3.0)   # counts() with triangles at thresholds 0, 1, 2, 3 + (largest weight,): from the oracle on the CPU


def test_several_frames_then_thresholds(nn, oracle_mod):
    """Three rigid integrations of three depths into uint16 weights and uint16 color (running averages with w > 0, the
    truncation of averaged color), a non-rigid one, then meshes at thresholds 0, 1, 2 and the default 3.0 (empty: no
    weight exceeds 3)."""
    O = oracle_mod
    sc = scenes(O, u16=True)
    frames = [TU.small_tsdf_scene(O, 5 + i, u16=True, depth_shift=s) for i, s in enumerate((0.004, -0.006))]
    got, want = both(nn, O, sc, {}, (8, "uint16", "uint16"), thresholds=(0.0, 1.0, 2.0, 3.0), extra_frames=frames)
    assert counts(want) + (float(want["rigid"][:, 4].max()),) == FRAMES_COUNTS
    assert len(want["mesh3"][3]) == 0 and len(got["mesh3"][3]) == 0
    assert_same(got, want)
    # the default threshold is 3.0
    g = GpuSide(nn, sc[0].voxel_size, 8, "uint16", "uint16", None)
    for fr in [sc[0]] + frames:
        g.integrate(g.touch(fr.depth, fr.K, EYE, fr), fr.depth, fr.color, fr.K, fr.K, EYE, fr)
    assert len(g.mesh(None)[3]) == 0


# ---- growth mode -----------------------------------------------------------------------------------------------------
GROWTH_COUNTS = {True: (8979, 14498, 2434, 2537, 632, 1917, 1912), False: (0, 0, 2434, 2537, 632, 0, 0)}   # per growth flag, from the oracle on the CPU: (voxels with weight > 0 after pass 1, after pass 2, non-zero
#                      cosine pixels of pass 1, of pass 2, sleeve blocks, triangles at threshold 0, at threshold 1)


def growth_sequence(side, O):
    """an empty grid: first blocks from a touch, then search, non-rigid pass, sleeve, a second non-rigid pass 1 cm farther"""
    sc, sc2 = scenes(O)
    out = {}
    side.activate(side.touch(sc.depth, sc.K, EYE, sc))
    out["found"] = nb = side.find(sc.depth, sc.K, EYE, sc)
    out["cos1"] = side.nonrigid(nb, sc.depth, sc.color, sc.normals, sc.K, sc.K, EYE, sc)
    out["values1"] = side.values()
    out["sleeve_n"] = side.sleeve()
    out["cos2"] = side.nonrigid(np.zeros((0, 3), np.int32), sc2.depth, sc2.color, sc2.normals, sc.K, sc.K, EYE, sc2)
    out["values2"] = side.values()
    out["coords"] = side.coords()
    out["mesh0"], out["mesh1"] = side.mesh(0.0), side.mesh(1.0)
    return out


def growth_counts(o):
    return (int((o["values1"][:, 4] > 0).sum()), int((o["values2"][:, 4] > 0).sum()), int((o["cos1"] != 0).sum()), int((o["cos2"] != 0).sum()),
            int(o["sleeve_n"]), len(o["mesh0"][3]), len(o["mesh1"][3]))


def test_growth_mode(nn, oracle_mod):
    """Surface first seen in a non-rigid pass: with growth on it gains weight and reaches the mesh, with growth off (the
    reference's behaviour) it never does; both against the oracle."""
    O = oracle_mod
    sc = scenes(O)[0]
    runs = {}
    for growth in (True, False):
        got = growth_sequence(GpuSide(nn, sc.voxel_size, 8, "float32", "float32", scene_field(sc), growth), O)
        want = growth_sequence(OracleSide(O, sc.voxel_size, 8, "float32", "float32", scene_field(sc), growth), O)
        assert growth_counts(want) == GROWTH_COUNTS[growth]
        assert_same(got, want)
        runs[growth] = got
    on, off = runs[True], runs[False]
    assert not np.array_equal(on["values1"], off["values1"]) and not np.array_equal(on["values2"], off["values2"])
    assert (on["values2"][:, 4] == 2).any() and not off["values2"][:, 4].any()
    assert len(on["mesh0"][3]) > 0 and len(on["mesh1"][3]) > 0 and len(off["mesh0"][3]) == 0


# ---- hash table ------------------------------------------------------------------------------------------------------
HASH_COUNTS = (309, 5309, 132692, 599)   # (scene blocks, distinct keys, sleeve blocks, triangles): numpy / the oracle on the CPU


def hash_calls():
    rng = np.random.default_rng(11)
    lo, hi = -(1 << 20), (1 << 20)
    keys = rng.integers(lo, hi, (5000, 3)).astype(np.int32)
    keys[17], keys[4100] = (lo, lo, lo), (hi - 1, hi - 1, hi - 1)
    calls = [keys[:1200], keys[1200:2500], keys[2500:3800], keys[3800:]]
    calls[0] = np.concatenate([calls[0], calls[0][100:300]])                  # duplicates within a call
    calls[2] = np.concatenate([keys[50:250], calls[2], calls[2][::7]])       # duplicates across calls and within
    calls[3] = np.concatenate([calls[3], keys[2400:2600]])
    return [np.ascontiguousarray(c) for c in calls]


def first_occurrence_unique(coords):
    _, idx = np.unique(coords, axis=0, return_index=True)
    return coords[np.sort(idx)]


def test_hash_table_growth_extremes_and_refused_call(nn, oracle_mod):
    """From capacity 16 through several growth steps: ~5,000 random keys over the whole domain in four calls (both extreme
    corners, duplicates within and across calls), a refused call in between, then a sleeve activation (about 140,000
    more blocks) and a mesh. Blocks of 2^3 voxels keep the volume small."""
    O = oracle_mod
    sc = TU.small_tsdf_scene(O, 0)
    gpu, orc = GpuSide(nn, 0.02, 2, "float32", "none", None, capacity=16), OracleSide(O, 0.02, 2, "float32", "none", None)
    blocks = orc.touch(sc.depth, sc.K, EYE, sc)
    assert np.array_equal(gpu.touch(sc.depth, sc.K, EYE, sc), blocks)
    for side in (gpu, orc):
        side.integrate(blocks, sc.depth, None, sc.K, sc.K, EYE, sc)
    calls = hash_calls()
    everything = [blocks]
    for i, c in enumerate(calls):
        if i == 2:   # a refused call: valid keys (new ones among them) and one coordinate out of range
            bad = np.concatenate([calls[2][:300], [[0, 1 << 20, 0]], calls[3][:300]]).astype(np.int32)
            with pytest.raises(RuntimeError):
                gpu.activate(bad)
            # the refused call changed nothing that a later call returns
            assert gpu.g.get_block_count() == len(first_occurrence_unique(np.concatenate(everything)))
            assert np.array_equal(gpu.coords(), first_occurrence_unique(np.concatenate(everything)))
            assert len(gpu.values_at(np.ascontiguousarray(calls[3][:300] * 2))) == 0
            valid = np.ascontiguousarray(np.concatenate([calls[2][:300], calls[3][:300]]))
            gpu.activate(valid)
            orc.activate(valid)
            everything.append(valid)
            assert np.array_equal(gpu.coords(), first_occurrence_unique(np.concatenate(everything)))
        gpu.activate(c)
        orc.activate(c)
        everything.append(c)
        assert np.array_equal(gpu.coords(), first_occurrence_unique(np.concatenate(everything))), i
    want_keys = first_occurrence_unique(np.concatenate(everything))
    assert np.array_equal(orc.coords(), want_keys)
    assert (want_keys == -(1 << 20)).all(1).any() and (want_keys == (1 << 20) - 1).all(1).any()
    # one voxel of every block is found (the block's first), none of 100 inactive blocks'
    rows = gpu.values_at(want_keys * 2)
    assert len(rows) == len(want_keys) and np.array_equal(rows, orc.values_at(want_keys * 2))
    rng = np.random.default_rng(12)
    inactive = rng.integers(-(1 << 19), 1 << 19, (100, 3)).astype(np.int32)
    assert not (inactive[:, None, :] == want_keys[None]).all(2).any()
    assert len(gpu.values_at(inactive * 2)) == 0
    n_gpu, n_orc = gpu.sleeve(), orc.sleeve()
    assert n_gpu == n_orc
    assert np.array_equal(gpu.coords(), orc.coords())
    mg, mo = gpu.mesh(0.0), orc.mesh(0.0)
    assert (len(blocks), len(want_keys), n_orc, len(mo[3])) == HASH_COUNTS
    assert_same({"mesh": mg}, {"mesh": mo})


# ---- marching cubes against plain numpy --------------------------------------------------------------------------------
CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)])
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
# per (res, threshold), from the oracle on the CPU: (distinct cube configurations, valid surface cubes by triangle count 1 .. 5)
MC_COUNTS = {(8, 0.0): (209, 922, 825, 645, 405, 124), (8, 1.0): (203, 672, 632, 530, 296, 77),
             (16, 0.0): (209, 923, 825, 645, 405, 124), (16, 1.0): (203, 679, 637, 531, 296, 77)}


@pytest.mark.parametrize("threshold", [0.0, 1.0])
@pytest.mark.parametrize("res", [8, 16])
def test_marching_cubes_against_numpy(nn, res, threshold, oracle_mod):
    """The extracted mesh of a rough volume (per-pixel depth noise of +-2 voxels, two integrations, so that threshold 1
    cuts into the surface) against numpy over the extracted voxel values: counts from the triangle table, every vertex
    at the float64 zero crossing of its grid edge, unit normals along the float64 gradient, manifold edges. The oracle
    only supplies the depth normals that the scene builder wants."""
    from dynamicfuion_python_amd.nnrt.voxel_grid import marching_cubes_table
    sc, sc2 = scenes(oracle_mod, rough=True, seed=3)
    gpu = GpuSide(nn, sc.voxel_size, res, "float32", "float32", None)
    gpu.integrate(gpu.touch(sc.depth, sc.K, EYE, sc), sc.depth, sc.color, sc.K, sc.K, EYE, sc)
    gpu.integrate(gpu.touch(sc2.depth, sc.K, EYE, sc2), sc2.depth, sc2.color, sc.K, sc.K, EYE, sc2)
    rows = gpu.values()
    V, Nn, _, T = gpu.mesh(threshold)
    voxel = float(np.float32(sc.voxel_size))
    ijk = np.rint(rows[:, :3].astype(np.float64) / voxel).astype(np.int64)
    lo = ijk.min(0) - 1
    shape = tuple(ijk.max(0) - lo + 2)
    p = ijk - lo
    tsdf, weight, exists, row_of = np.zeros(shape), np.zeros(shape), np.zeros(shape, bool), np.full(shape, -1, np.int64)
    tsdf[p[:, 0], p[:, 1], p[:, 2]] = rows[:, 3]
    weight[p[:, 0], p[:, 1], p[:, 2]] = rows[:, 4]
    exists[p[:, 0], p[:, 1], p[:, 2]] = True
    row_of[p[:, 0], p[:, 1], p[:, 2]] = np.arange(len(rows))
    assert weight.max() == 2 and (weight == 1).any()

    def at(a, q):
        return a[q[:, 0], q[:, 1], q[:, 2]]
    corner = p[:, None, :] + CORNERS[None]                                           # [n, 8, 3]
    cw = weight[corner[..., 0], corner[..., 1], corner[..., 2]]
    ce = exists[corner[..., 0], corner[..., 1], corner[..., 2]]
    ct = tsdf[corner[..., 0], corner[..., 1], corner[..., 2]]
    cfg = ((ct < 0) * (1 << np.arange(8))[None]).sum(1)
    valid = (ce & (cw > threshold)).all(1) & (cfg != 0) & (cfg != 255)
    tri, _ = marching_cubes_table()
    ntri = np.argmax(tri < 0, axis=1) // 3   # a row ends at its first -1
    assert len(T) == ntri[cfg[valid]].sum()
    by_count = tuple(int((ntri[cfg[valid]] == k).sum()) for k in (1, 2, 3, 4, 5))
    assert (len(np.unique(cfg[valid])),) + by_count == MC_COUNTS[(res, threshold)]
    assert all(by_count[:4])   # configurations with 1, 2, 3 and 4 triangles are reached
    # owned edges with a sign change among the valid cubes: (row of the owner voxel, axis), in the kernel's vertex order
    owned = set()
    for a, b in EDGES:
        crossing = valid & ((ct[:, a] < 0) != (ct[:, b] < 0))
        low = np.minimum(CORNERS[a], CORNERS[b])
        axis = int(np.argmax(CORNERS[a] != CORNERS[b]))
        owned.update(zip(at(row_of, p[crossing] + low).tolist(), [axis] * int(crossing.sum())))
    owned = np.array(sorted(owned), np.int64)
    assert len(V) == len(owned) and len(V) > 0
    o = p[owned[:, 0]]
    e = o + np.eye(3, dtype=np.int64)[owned[:, 1]]
    to, te = at(tsdf, o), at(tsdf, e)
    r = to / (to - te)
    want = ((o + lo).astype(np.float64) + r[:, None] * np.eye(3)[owned[:, 1]]) * voxel
    tol = 8 * 2.0 ** -24 * np.maximum(np.abs(want), voxel)
    assert (np.abs(V.astype(np.float64) - want) <= tol).all()
    # normals: unit length or exactly zero, along the float64 central-difference gradient (a missing neighbour gives the centre)

    def gradient(q):
        g = np.zeros((len(q), 3))
        c = at(tsdf, q)
        for k in range(3):
            d = np.eye(3, dtype=np.int64)[k]
            hi, lo_ = np.where(at(exists, q + d), at(tsdf, q + d), c), np.where(at(exists, q - d), at(tsdf, q - d), c)
            g[:, k] = hi - lo_
        return g
    grad = (1 - r)[:, None] * gradient(o) + r[:, None] * gradient(e)
    length = np.linalg.norm(Nn.astype(np.float64), axis=1)
    zero = (Nn == 0).all(1)
    assert (np.abs(length[~zero] - 1) <= 4 * 2.0 ** -24).all()
    strong = np.linalg.norm(grad, axis=1) > 1e-3
    assert strong.sum() > len(V) // 2 and ((Nn * grad).sum(1)[strong] > 0).all()
    # no undirected edge more than twice; an edge used twice is used once in each direction
    d = np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]])
    assert (d[:, 0] != d[:, 1]).all()
    directed, dc = np.unique(d, axis=0, return_counts=True)
    assert (dc == 1).all()
    _, uc = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    assert uc.max() == 2 and (uc == 2).sum() > len(uc) // 2


# ---- the grid's owners: reused scratch table and error word, the one compaction step, no per-call allocation ------------
def bytes_in_use():
    from dynamicfuion_python_amd import _native
    return int(_native.lib().nnrt_device_bytes_in_use())


def test_dedupe_table_is_reused_across_frames(nn, oracle_mod):
    """unique_block_coordinates on one grid for a frame that touches many blocks, one that touches few, then the first
    again: each result is a fresh grid's (and the oracle's) for that frame, in order, and the grid's own blocks and table
    are as they were (the dedupe table is scratch of its own)."""
    sc = TU.small_tsdf_scene(oracle_mod, 0)
    few = np.zeros_like(sc.depth)
    few[20:28, 28:36] = sc.depth[20:28, 28:36]
    gpu = GpuSide(nn, sc.voxel_size, 8, "float32", "float32", None, capacity=64)
    blocks = gpu.touch(sc.depth, sc.K, EYE, sc)
    gpu.integrate(blocks, sc.depth, sc.color, sc.K, sc.K, EYE, sc)
    coords0, values0 = gpu.coords(), gpu.values()
    want = {}
    for name, depth in (("many", sc.depth), ("few", few)):
        want[name] = GpuSide(nn, sc.voxel_size, 8, "float32", "float32", None, capacity=64).touch(depth, sc.K, EYE, sc)
        assert np.array_equal(want[name], OracleSide(oracle_mod, sc.voxel_size, 8, "float32", "float32", None).touch(depth, sc.K, EYE, sc))
    assert len(want["many"]) == 43 and 0 < len(want["few"]) <= 8
    for name, depth in (("many", sc.depth), ("few", few), ("many", sc.depth)):
        assert np.array_equal(gpu.touch(depth, sc.K, EYE, sc), want[name]), name
        assert np.array_equal(gpu.coords(), coords0) and np.array_equal(gpu.values(), values0), name
    # the table still finds every block: one voxel row per block's first voxel
    assert len(gpu.values_at(np.ascontiguousarray(coords0 * 8))) == len(coords0)


def test_error_word_is_reused_across_refused_calls(nn):
    """Two refused activations (a coordinate out of range, at either end) and then a valid one on the same grid: both
    refusals leave the grid as it was, the valid call creates exactly its blocks, and the grid holds as much device memory
    as a fresh one of equal capacity after the same valid calls (the error word is the handle's, allocated once)."""
    base = np.array([(0, 0, 0), (1, 0, 0), (-3, 2, 5), (7, 7, 7), (0, -1, 0)], np.int32)
    valid = np.array([(2, 0, 0), (1, 0, 0), (4, 4, 4), (-5, -5, -5), (2, 0, 0), (9, 1, 1), (0, 0, 1), (0, 1, 0), (3, 3, 3)], np.int32)
    bad1, bad2 = valid.copy(), valid.copy()
    bad1[3] = (0, 1 << 20, 0)
    bad2[0] = (-(1 << 20) - 1, 0, 0)
    expect = first_occurrence_unique(np.concatenate([base, valid]))
    start = bytes_in_use()
    gpu = GpuSide(nn, 0.01, 8, "float32", "none", None, capacity=64)
    gpu.activate(base)
    coords0, values0 = gpu.coords(), gpu.values()
    for bad in (bad1, bad2):
        with pytest.raises(RuntimeError):
            gpu.activate(bad)
        assert gpu.g.get_block_count() == len(base)
        assert np.array_equal(gpu.coords(), coords0) and np.array_equal(gpu.values(), values0)
        assert len(gpu.values_at(np.ascontiguousarray(valid * 8))) == 1   # (1, 0, 0) alone is active
    gpu.activate(valid)
    assert gpu.g.get_block_count() == len(expect) == 12 and np.array_equal(gpu.coords(), expect)
    held = bytes_in_use() - start
    # the same calls without the refusals on a second grid, so that its scratch and result buffers match too
    start = bytes_in_use()
    fresh = GpuSide(nn, 0.01, 8, "float32", "none", None, capacity=64)
    fresh.activate(base)
    fresh.values_at(np.ascontiguousarray(valid * 8))
    fresh.activate(valid)
    assert np.array_equal(fresh.coords(), expect)
    assert bytes_in_use() - start == held


@pytest.mark.parametrize("cdt", ["none", "float32"], ids=["width5", "width8"])
def test_values_at_compaction_counts_and_patterns(nn, oracle_mod, cdt):
    """extract_voxel_values_at against rows of extract_voxel_values_and_coordinates, for 1, 255, 256 and 257 queries
    (either side of one workgroup) with none, all and every other one found, at row widths 5 and 8. A found query's row
    is its coordinate and the stored values at the reference's index b res^3 + x + res (y + res z) (the global
    coordinate), -2 throughout when that index leaves the active blocks' storage."""
    sc = TU.small_tsdf_scene(oracle_mod, 0)
    gpu = GpuSide(nn, sc.voxel_size, 8, "float32", cdt, None, capacity=64)
    origin = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)], np.int32)
    gpu.activate(origin)
    blocks = gpu.touch(sc.depth, sc.K, EYE, sc)
    gpu.integrate(blocks, sc.depth, sc.color if cdt != "none" else None, sc.K, sc.K, EYE, sc)
    gpu.activate(np.array([(3, 3, 20)], np.int32))   # the last block, far out: the reference's index leaves the storage there
    rows_all, coords = gpu.values(), gpu.coords()
    C = 8 if cdt != "none" else 5
    assert rows_all.shape == (len(coords) * 512, C) and np.array_equal(coords[:4], origin) and (rows_all[:, 4] > 0).any()
    assert len(coords) == 4 + 43 + 1 and tuple(coords[-1]) == (3, 3, 20)
    rng = np.random.default_rng(21)
    vs = np.float32(sc.voxel_size)

    def expected(q):
        block_of = {tuple(c): b for b, c in enumerate(coords)}
        out = []
        for x, y, z in q:
            b = block_of.get((int(x) // 8, int(y) // 8, int(z) // 8))   # queries are non-negative: // is the C++ division
            if b is None:
                continue
            lin = b * 512 + int(x) + 8 * (int(y) + 8 * int(z))
            row = np.full(C, -2, np.float32)
            if lin < len(rows_all):   # never negative here
                row[:3] = np.array([x, y, z], np.float32) * vs
                row[3:] = rows_all[lin, 3:]
            out.append(row)
        return np.array(out, np.float32).reshape(-1, C)

    last = coords[-1] * 8   # a found query whose row is -2 throughout
    for n in (1, 255, 256, 257):
        hit = np.stack([rng.integers(0, 16, n), rng.integers(0, 16, n), rng.integers(0, 8, n)], 1).astype(np.int32)
        hit[n // 2] = last + (7, 7, 7)
        miss = hit + np.int32(8000)
        for name, q in (("none", miss), ("all", hit), ("alternating", np.where((np.arange(n) % 2 == 0)[:, None], hit, miss))):
            q = np.ascontiguousarray(q, np.int32)
            got, want = gpu.values_at(q), expected(q)
            assert len(want) == {"none": 0, "all": n, "alternating": (n + 1) // 2}[name]
            assert got.shape == want.shape and np.array_equal(got, want), (n, name)
    assert (expected(np.ascontiguousarray([last + (7, 7, 7)], np.int32)) == -2).all()


@pytest.mark.parametrize("active", [9, 10])
def test_sleeve_compaction_either_side_of_one_workgroup(nn, oracle_mod, active):
    """The inactive-neighbour compaction with 27 * active candidates either side of 256 (243 and 270): the sleeve count
    (duplicates kept) and the blocks it activates against the oracle's."""
    keys = np.array([(x, y, 0) for y in range(3) for x in range(3)] + [(5, 5, 5)], np.int32)[:active]
    gpu, orc = GpuSide(nn, 0.01, 8, "float32", "none", None, capacity=16), OracleSide(oracle_mod, 0.01, 8, "float32", "none", None)
    for side in (gpu, orc):
        side.activate(keys)
    n_gpu, n_orc = gpu.sleeve(), orc.sleeve()
    # of a block's 27 neighbours (itself included) the active ones are dropped: 4 at a corner of the 3 x 3 plane, 6 at an
    # edge, 9 at its centre; the tenth block stands alone
    assert n_gpu == n_orc and n_orc == {9: 243 - (4 * 4 + 4 * 6 + 9), 10: 243 - (4 * 4 + 4 * 6 + 9) + 26}[active]
    assert np.array_equal(gpu.coords(), orc.coords()) and len(gpu.coords()) == {9: 75, 10: 75 + 27}[active]


def test_no_device_allocation_per_frame(nn, oracle_mod):
    """After one warm-up frame the grid allocates nothing: nnrt_device_bytes_in_use is the same before and after
    unique_block_coordinates, integrate and integrate_non_rigid, for three further frames of the same sizes."""
    sc, sc2 = scenes(oracle_mod)
    gpu = GpuSide(nn, sc.voxel_size, 8, "float32", "float32", scene_field(sc), growth=True, capacity=256)

    def frame(check):
        steps = []
        before = bytes_in_use()
        b = gpu.touch(sc.depth, sc.K, EYE, sc)
        steps.append(bytes_in_use() - before)
        gpu.integrate(b, sc.depth, sc.color, sc.K, sc.K, EYE, sc)
        steps.append(bytes_in_use() - before)
        cos = gpu.nonrigid(b, sc2.depth, sc2.color, sc2.normals, sc.K, sc.K, EYE, sc2)
        steps.append(bytes_in_use() - before)
        assert len(b) == 43 and (cos != 0).any()
        if check:
            assert steps == [0, 0, 0]
    frame(False)
    for _ in range(3):
        frame(True)
    assert gpu.g.get_block_count() == 43
