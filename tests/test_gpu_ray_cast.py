"""VoxelBlockGrid.ray_cast on the GPU (csrc/tsdf_ray_cast.hip: k_range_blocks, k_ray_cast) against the float32 numpy restatement
of DESIGN §19 (tests/_ray_cast_util.py), bit for bit. Every case fills a GPU grid, pulls its voxel rows and block
coordinates back and runs the restatement on those, so the ray cast is compared apart from integration. Frames are the
64 x 48 ones of _tsdf_util.small_tsdf_scene; every case also asserts that rays hit, so nothing passes on an empty image."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _ray_cast_util as RC  # noqa: E402
import _tsdf_util as TU  # noqa: E402

EYE = np.eye(4)
DEPTH_MIN = 0.1
MAPS = RC.ATTRIBUTES


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import nnrt
    return nnrt


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def make_grid(nn, voxel, res, weight="float32", color="float32", cls=None):
    names, dts, ch = ["tsdf", "weight"], ["float32", weight], [1, 1]
    if color != "none":
        names, dts, ch = names + ["color"], dts + [color], ch + [3]
    return (cls or nn.geometry.NonRigidSurfaceVoxelBlockGrid)(names, dts, ch, voxel, res, 16)


def fill(g, sc, times=3, E=EYE, color=True):
    blocks = g.compute_unique_block_coordinates(sc.depth, sc.K, E, sc.depth_scale, sc.depth_max, sc.trunc_mult)
    for _ in range(times):
        if color:
            g.integrate(blocks, sc.depth, sc.color, sc.K, sc.K, E, sc.depth_scale, sc.depth_max, sc.trunc_mult)
        else:
            g.integrate(blocks, sc.depth, sc.K, E, sc.depth_scale, sc.depth_max, sc.trunc_mult)
    return blocks


def cast_both(g, K, E, W, H, attributes=MAPS, depth_scale=1.0, depth_min=DEPTH_MIN, depth_max=TU.SMALL_DEPTH_MAX, weight_threshold=3.0,
              trunc_mult=TU.SMALL_TRUNC_MULT, f=8, cast_blocks=None):
    """The GPU call and the restatement on the grid's own voxels; asserts that they agree exactly; returns both."""
    if g.get_block_count():
        rows, blocks = _np(g.extract_voxel_values_and_coordinates()), _np(g.get_block_coordinates())
    else:   # the exports of an empty grid have nothing to write to
        rows, blocks = np.zeros((0, 8), np.float32), np.zeros((0, 3), np.int32)
    cast = blocks if cast_blocks is None else np.asarray(cast_blocks, np.int32).reshape(-1, 3)
    got = g.ray_cast(cast, K, E, W, H, attributes, depth_scale, depth_min, depth_max, weight_threshold, trunc_mult, f)
    assert set(got) == {"range"} | set(attributes)
    got = {k: _np(v) for k, v in got.items()}
    want = RC.ray_cast(rows, blocks, g.get_block_resolution(), g.get_voxel_size(), cast, K, E, W, H, tuple(attributes), depth_scale, depth_min,
                       depth_max, weight_threshold, trunc_mult, f)
    assert got["range"].dtype == np.float32 and got["range"].shape == want["range"].shape == (-(-H // f), -(-W // f), 2)
    assert np.array_equal(got["range"], want["range"]), "range"
    for name in attributes:
        assert got[name].dtype == np.float32 and got[name].shape == (H, W, 1 if name == "depth" else 3), name
        if name == "depth":
            assert np.array_equal(got["depth"][..., 0] != 0, want["hit"]), "hit mask"
        differ = (got[name] != want[name]).any(-1)
        assert not differ.any(), f"{name}: {int(differ.sum())} pixels differ, first at {tuple(np.argwhere(differ)[0])}: " \
                                 f"{got[name][differ][0]} != {want[name][differ][0]}"
    return got, want


@pytest.fixture(scope="module")
def float_scene(oracle_mod):
    return TU.small_tsdf_scene(oracle_mod, 0, hole=False, far_strip=False)


@pytest.fixture(scope="module")
def float_grid(nn, float_scene):
    """res 8, float weight and colour, the float scene integrated three times (shared, never modified)"""
    g = make_grid(nn, float_scene.voxel_size, 8)
    fill(g, float_scene)
    return g


def test_float_scene_all_attributes(float_grid, float_scene):
    """Case 1: 48 x 64, res 8, the integration camera, f = 8, all four maps; and against the analytic surface."""
    sc = float_scene
    got, want = cast_both(float_grid, sc.K, EYE, sc.W, sc.H)
    assert want["hit"].sum() > 2500 and (got["normal"] != 0).any(-1).sum() > 2000 and got["color"].max() > 0.5
    err, missed, expected, hits, stray = RC.compare_with_surface(want | {"depth": got["depth"]}, RC.small_scene_surface(sc.K), sc.K, EYE, 1.0,
                                                                 DEPTH_MIN, sc.depth_max, sc.W, sc.H, (sc.H, sc.W))
    print(f"max depth error {err:.6f} m, missed {missed:.4f} of {expected}")
    assert err <= RC.DEPTH_TOLERANCE and missed <= RC.MISS_CAP and stray == 0


def test_loop_storage_types_res16(nn, oracle_mod):
    """Case 2: uint16 depth, uint16 weight, uint16 colour (the fusion loop's types), block resolution 16."""
    sc = TU.small_tsdf_scene(oracle_mod, 0, u16=True, hole=False, far_strip=False)
    g = make_grid(nn, sc.voxel_size, 16, "uint16", "uint16")
    fill(g, sc)
    got, want = cast_both(g, sc.K, EYE, sc.W, sc.H, depth_scale=1000.0)
    assert want["hit"].sum() > 2500 and got["color"].max() > 0.5
    assert got["depth"].max() > 400.0   # millimetres


@pytest.mark.parametrize("f", [8, 1, 64])
def test_ragged_tiles_moved_camera(float_grid, float_scene, f):
    """Case 3: a 45 x 61 image (ragged 8 x 8 wavefront tiles and ragged range tiles) from a rotated, shifted camera;
    f = 1 (a range entry per pixel) and f = 64 (one entry for the whole image)."""
    sc = float_scene
    got, want = cast_both(float_grid, sc.K, TU.extrinsic_about_y(), 61, 45, f=f)
    assert want["hit"].sum() > 1200
    if f == 64:
        assert got["range"].shape == (1, 1, 2)


def test_weight_threshold(nn, float_scene):
    """Case 4: weight_threshold = 3 after one integration misses everywhere; after three the rays hit."""
    sc = float_scene
    g = make_grid(nn, sc.voxel_size, 8)
    fill(g, sc, times=1)
    got, want = cast_both(g, sc.K, EYE, sc.W, sc.H)
    assert not want["hit"].any() and not any(got[k].any() for k in MAPS)
    assert (got["range"][..., 0] < got["range"][..., 1]).any()   # the blocks are there: the rays were marched
    fill(g, sc, times=2)
    got, want = cast_both(g, sc.K, EYE, sc.W, sc.H)
    assert want["hit"].sum() > 2500


def two_layer_frames(sc):
    """A far plane at 0.6 m with a hole, and a plate at 0.3 m over the left half of the image (nothing on the right)."""
    far, near = sc.depth.copy(), sc.depth.copy()
    far[:] = 0.6
    far[30:38, 40:50] = 0.0
    near[:] = 0.0
    near[:, :32] = 0.3
    return far, near


@pytest.mark.parametrize("pose", ["integration_camera", "about_y"])
def test_two_layers_cross_empty_blocks(nn, float_scene, pose):
    """Case 5: rays past the plate's edge leave its blocks, cross the absent blocks between 0.3 m and 0.6 m (the exit
    step) and hit the far plane, or miss in its hole; no ray hits in the gap."""
    sc = float_scene
    g = make_grid(nn, sc.voxel_size, 8)
    frame = TU.SmallScene()
    frame.__dict__.update(sc.__dict__)
    for depth in two_layer_frames(sc):
        frame.depth = depth
        fill(g, frame)
    E = EYE if pose == "integration_camera" else TU.extrinsic_about_y(4.0, (0.01, 0.0, 0.0))
    got, want = cast_both(g, sc.K, E, sc.W, sc.H)
    vz = got["vertex"][..., 2][want["hit"]]          # world z: the integration camera's depth
    band = sc.voxel_size * sc.trunc_mult
    on_plate, on_plane = np.abs(vz - 0.3) <= band, np.abs(vz - 0.6) <= band
    assert (on_plate | on_plane).all(), f"hits in the gap at z = {vz[~(on_plate | on_plane)]}"
    assert on_plate.sum() > 800 and on_plane.sum() > 800
    if pose == "integration_camera":
        d = got["depth"][..., 0]
        assert (np.abs(d[4:-4, 36:40] - 0.6) <= sc.voxel_size).all()    # just past the plate's edge: the far plane
        assert (np.abs(d[4:-4, 4:28] - 0.3) <= sc.voxel_size).all()
        assert not d[32:36, 42:48].any()                                 # the hole


def test_camera_inside_the_blocks(float_grid, float_scene):
    """Case 6: the camera at world z = 0.42, between the corners of the blocks at z in [0.40, 0.48): those blocks have
    corners with zc <= 0 and cover the whole range map from depth_min."""
    sc = float_scene
    E = np.eye(4)
    E[2, 3] = -0.42
    dmin = 0.01
    got, want = cast_both(float_grid, sc.K, E, sc.W, sc.H, depth_min=dmin)
    assert (got["range"][..., 0] == np.float32(dmin)).all()
    assert want["hit"].sum() > 500


def test_non_rigid_grid(nn, oracle_mod):
    """Case 7: NonRigidSurfaceVoxelBlockGrid after a rigid and one non-rigid integration of the small scene."""
    import test_gpu_tsdf_cases as TC
    sc, sc2 = TC.scenes(oracle_mod)
    side = TC.GpuSide(nn, sc.voxel_size, 8, "float32", "float32", TC.scene_field(sc))
    blocks = side.touch(sc.depth, sc.K, EYE, sc)
    side.integrate(blocks, sc.depth, sc.color, sc.K, sc.K, EYE, sc)
    found = side.find(sc2.depth, sc.K, EYE, sc2)
    side.nonrigid(found, sc2.depth, sc2.color, sc2.normals, sc.K, sc.K, EYE, sc2)
    cast_both(side.g, sc.K, EYE, sc.W, sc.H, weight_threshold=2.0)   # only voxels both passes observed
    got, want = cast_both(side.g, sc.K, EYE, sc.W, sc.H, weight_threshold=1.0)
    assert want["hit"].sum() > 1500


def test_empty_inputs_and_fewer_attributes(nn, float_grid, float_scene):
    """Case 8: an empty grid, and empty block_coords on a filled one, give all-zero maps; a second call with fewer
    attributes returns only those, fully written."""
    sc = float_scene
    empty = make_grid(nn, sc.voxel_size, 8)
    for g, cast in ((empty, np.zeros((0, 3), np.int32)), (empty, [[0, 0, 6]]), (float_grid, np.zeros((0, 3), np.int32))):
        got, want = cast_both(g, sc.K, EYE, sc.W, sc.H, cast_blocks=cast)
        assert not any(got[k].any() for k in MAPS)
        assert (got["range"][..., 0] == np.float32(sc.depth_max)).all() and (got["range"][..., 1] == np.float32(DEPTH_MIN)).all()
    cast_both(float_grid, sc.K, EYE, sc.W, sc.H)
    got, want = cast_both(float_grid, sc.K, TU.extrinsic_about_y(), sc.W, sc.H, attributes=["vertex"])   # a list is accepted
    assert want["hit"].sum() > 1200 and set(got) == {"range", "vertex"}
    got, _ = cast_both(float_grid, sc.K, EYE, sc.W, sc.H, attributes=("depth",), cast_blocks=np.zeros((0, 3), np.int32))
    assert not got["depth"].any()


def test_refusals_leave_the_grid_usable(nn, float_grid, float_scene):
    """Case 9: every documented refusal, by its exception type; the grid renders as before afterwards."""
    from dynamicfuion_python_amd import _native as N
    sc, g = float_scene, float_grid
    blocks = g.get_block_coordinates()

    def call(**kw):
        a = dict(width=sc.W, height=sc.H, render_attributes=("depth",), depth_scale=1.0, depth_min=DEPTH_MIN, depth_max=sc.depth_max,
                 weight_threshold=3.0, trunc_voxel_multiplier=sc.trunc_mult, range_map_down_factor=8, extrinsic=EYE)
        a.update(kw)
        return g.ray_cast(blocks, sc.K, **a)
    for kw in (dict(width=0), dict(height=0), dict(range_map_down_factor=0), dict(depth_min=-0.1), dict(depth_min=0.9, depth_max=0.9),
               dict(depth_min=1.0, depth_max=0.5), dict(depth_scale=0.0), dict(depth_scale=-1.0), dict(extrinsic=np.zeros((4, 4))),
               dict(depth_max=1.0e4)):      # 2 * 1e4 / 0.01 steps > 2^20
        with pytest.raises(N.NnrtError):
            call(**kw)
    assert b"2^20" in N.lib().nnrt_last_error()
    with pytest.raises(N.NnrtError, match="without color"):
        fill_free = make_grid(nn, sc.voxel_size, 8, color="none")
        fill_free.ray_cast(blocks, sc.K, EYE, sc.W, sc.H)          # the default attributes ask for colour
    for name in ("index", "mask", "interp_ratio", "interp_ratio_dx"):
        with pytest.raises(NotImplementedError, match=name):
            call(render_attributes=("depth", name))
    with pytest.raises(ValueError, match="albedo"):
        call(render_attributes=["albedo"])
    # the C entry point's pointer checks: null intrinsics, null range map, a requested map that is null
    lib = N.lib()
    K = np.ascontiguousarray(sc.K, np.float64)
    rng = torch.empty((6, 8, 2), dtype=torch.float32, device=g.get_device())
    depth = torch.empty((sc.H, sc.W, 1), dtype=torch.float32, device=g.get_device())

    def raw(grid=g._h, k=K, range_map=rng, mask=1, depth_map=depth):
        return lib.nnrt_voxel_grid_ray_cast(grid, N.ptr(blocks), blocks.shape[0], N.ptr(k), None, sc.W, sc.H, mask, 1.0, DEPTH_MIN, sc.depth_max, 3.0,
                                            sc.trunc_mult, 8, N.ptr(range_map), N.ptr(depth_map), None, None, None, N.stream_ptr())
    assert raw() == 0
    for bad in (dict(grid=None), dict(k=None), dict(range_map=None), dict(depth_map=None), dict(mask=2), dict(mask=4), dict(mask=8), dict(mask=16)):
        assert raw(**bad) == 1, bad
        assert b"invalid argument" in lib.nnrt_last_error()
    cast_both(g, sc.K, EYE, sc.W, sc.H)


def write_static_sequence(directory, sc, frames=2):
    from PIL import Image
    for i in range(frames):
        Image.fromarray(sc.depth).save(str(directory / f"depth_{i:04d}.png"))
        Image.fromarray(sc.color).save(str(directory / f"rgb_{i:04d}.png"))
    K = sc.K
    rows = [[K[0, 0], 0, K[0, 2], 0], [0, K[1, 1], K[1, 2], 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    (directory / "camera_intrinsics.txt").write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in rows) + "\n")


def test_fusion_pipeline_renders_its_canonical_model(nn, oracle_mod, tmp_path):
    """Case 10: FusionPipeline.render_canonical_model after two frames of a static sequence (the small scene's uint16
    frame, no hole, no far strip) from the identity pose at the pipeline's default threshold: the depth against the first
    frame's input depth within the CPU-measured tolerance under the 5 % cap (tests/test_ray_cast_cpu.py checks the
    restatement at this configuration first), and the whole call against the restatement, bit for bit."""
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.data import frame as dfr
    sc = TU.small_tsdf_scene(oracle_mod, 0, u16=True, hole=False, far_strip=False)
    write_static_sequence(tmp_path, sc)
    seq = dfr.FrameSequenceDataset(base_dataset_type=dfr.DatasetType.CUSTOM, custom_frame_directory=str(tmp_path)).load()
    params = F.FusionParameters(graph_generation_mode=F.GraphGenerationMode.FIRST_FRAME_EXTRACTED_MESH)
    params.alignment.max_iteration_count = 1
    params.alignment.guard_zero_rotation = True
    params.alignment.arap_term_weight = 20000.0   # nothing moves: a stiff graph keeps the fit at the residuals' level
    pipe = F.FusionPipeline(seq, params)
    pipe.run()
    assert len(pipe.results) == 2 and pipe.results[1].tracked and pipe.mesh_extraction_threshold() == 1
    out = pipe.render_canonical_model()
    assert set(out) == {"range", "depth", "normal"} and tuple(out["depth"].shape) == (sc.H, sc.W, 1)
    got = {k: _np(v) for k, v in out.items()}
    err, missed, expected = RC.compare_with_input_depth(got, sc.depth / 1000.0, DEPTH_MIN, 3.0, 1000.0)
    print(f"canonical model against the first frame: max depth error {err:.6f} m, missed {missed:.4f} of {expected}")
    assert err <= RC.DEPTH_TOLERANCE and missed <= RC.MISS_CAP
    g = pipe.volume
    _, want = cast_both(g, pipe.K, pipe.extrinsics, sc.W, sc.H, ("depth", "normal"), 1000.0, DEPTH_MIN, 3.0, 1.0, pipe.truncation_voxel_multiplier, 8)
    assert np.array_equal(got["depth"], want["depth"]) and np.array_equal(got["normal"], want["normal"])
    # other poses and thresholds go through
    moved = pipe.render_canonical_model(("vertex",), extrinsics=TU.extrinsic_about_y(), weight_threshold=0)
    assert set(moved) == {"range", "vertex"} and bool(moved["vertex"].any())
