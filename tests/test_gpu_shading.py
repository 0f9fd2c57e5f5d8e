"""The shaders and the depth comparison on the GPU (csrc/shading.hip: k_shade_pixels, k_depth_agreement,
k_depth_agreement_finish) against the reference's two known-answer images and the numpy restatements of DESIGN §22
(tests/_shading_util.py), at the image sizes where a lane-per-pixel launch and a blocked reduction can go wrong, and the
fusion loop's model-agreement switch on a small static sequence."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _depth_filter_util as DF  # noqa: E402
import _shading_util as SU  # noqa: E402

F32 = np.float32
# 1 x 1; one row; smaller than a wavefront; whole workgroups; ragged both ways (4095 = 16 workgroups less one pixel, two
# records of the comparison); a multiple of the workgroup that is no multiple of a comparison record
SIZES = [(1, 1), (1, 64), (7, 5), (64, 64), (63, 65), (48, 64)]


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import nnrt
    return nnrt


def _np(t):
    return t.detach().cpu().numpy()


def camera(H, W):
    f = 0.9 * max(H, W)
    return np.array([[f, 0.0, W / 2 - 0.3], [0.0, f, H / 2 + 0.2], [0.0, 0.0, 1.0]])


def scene_meshes(H, W, seed):
    """Camera-space meshes around z = 2 with colours beyond [0, 1] and normals turned toward the camera: a quad over the left
    and middle of the image, a nearer triangle across it, the quad moved off screen, and the quad's vertices without faces."""
    rng = np.random.default_rng(seed)
    f = 0.9 * max(H, W)
    sx, sy = 2 * (W / 2) / f, 2 * (H / 2) / f   # half extents of the image at z = 2

    def attributes(n):
        normals = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-1.0, -0.3, (n, 1))], 1).astype(F32)
        return normals, rng.uniform(-0.2, 1.2, (n, 3)).astype(F32)

    quad = np.array([[-0.8 * sx, -0.7 * sy, 2.0], [0.3 * sx, -0.6 * sy, 2.2], [0.2 * sx, 0.8 * sy, 1.9], [-0.7 * sx, 0.6 * sy, 2.1]], F32)
    tri = np.array([[-0.2 * sx, -0.9 * sy, 1.5], [0.9 * sx, 0.0, 1.6], [-0.1 * sx, 0.9 * sy, 1.4]], F32)
    qn, qc = attributes(4)
    tn, tc = attributes(3)
    a = dict(vertex_positions=quad, triangle_indices=np.array([[0, 1, 2], [0, 2, 3]], np.int64), vertex_normals=qn, vertex_colors=qc)
    b = dict(vertex_positions=tri, triangle_indices=np.array([[0, 2, 1]], np.int64), vertex_normals=tn, vertex_colors=tc)
    away = dict(a, vertex_positions=(quad + F32([100.0, 0, 0])).astype(F32))
    faceless = dict(a, triangle_indices=np.zeros((0, 3), np.int64))
    return {"two meshes": [a, b], "off screen": [away], "no faces": [faceless]}


def as_meshes(nn, parts):
    return [nn.geometry.TriangleMesh(d["vertex_positions"], d["vertex_normals"], d["triangle_indices"], vertex_colors=d["vertex_colors"])
            for d in parts]


# ---- the reference's known answers ---------------------------------------------------------------------------------------
def triangle_fragments(nn, blur):
    mesh = nn.geometry.TriangleMesh(SU.TRIANGLE_VERTICES, None, SU.TRIANGLE_FACES, vertex_colors=SU.TRIANGLE_COLORS)
    ndc, mask = nn.rendering.functional.get_mesh_ndc_face_vertices_and_clip_mask(mesh, SU.TRIANGLE_K, SU.TRIANGLE_SIZE)
    return mesh, nn.rendering.rasterize_ndc_triangles(ndc, mask, SU.TRIANGLE_SIZE, blur, 1)


def test_vertex_color_shader_reproduces_the_reference_image(nn):
    mesh, fragments = triangle_fragments(nn, 0.0)
    for meshes in ([mesh], mesh):
        image = nn.rendering.VertexColorShader().shade_meshes(*fragments, meshes)
        assert image.dtype == torch.uint8 and image.is_cuda and tuple(image.shape) == (480, 640, 3)
        assert int((_np(image) != SU.golden_image("triangle_vertex_colors.png")).sum()) == 0
    assert int((_np(fragments[0])[..., 0] >= 0).sum()) == SU.VERTEX_COLOR_COVERED
    # the same through render_meshes (identity extrinsics, the reference's NDC mapping)
    image, rendered = nn.rendering.render_meshes(mesh, SU.TRIANGLE_K, SU.TRIANGLE_SIZE, nn.rendering.VertexColorShader())
    assert int((_np(image) != SU.golden_image("triangle_vertex_colors.png")).sum()) == 0
    assert all(torch.equal(a, b) for a, b in zip(rendered, fragments))
    with pytest.raises(RuntimeError, match="meshes"):
        nn.rendering.VertexColorShader().shade_meshes(*fragments)
    with pytest.raises(RuntimeError, match="vertex_colors"):
        nn.rendering.VertexColorShader().shade_meshes(*fragments, [nn.geometry.TriangleMesh(SU.TRIANGLE_VERTICES, None, SU.TRIANGLE_FACES)])
    with pytest.raises(RuntimeError, match="vertex_normals"):
        nn.rendering.HeadlightShader().shade_meshes(*fragments, [mesh])


def test_flat_edge_shader_reproduces_the_reference_image(nn):
    _, fragments = triangle_fragments(nn, 1.0)
    shader = nn.rendering.FlatEdgeShader(2.0, (1.0, 1.0, 1.0))
    image = _np(shader.shade_meshes(*fragments))
    assert image.dtype == np.uint8 and image.shape == (480, 640, 3)
    assert int((image != SU.golden_image("triangle.png")).sum()) == 0
    assert int(image.any(-1).sum()) == SU.FLAT_EDGE_LIT
    assert shader.get_ndc_line_width(480, 640) == float(SU.ndc_line_width(2.0, 480, 640)) == float(F32(2.0) / F32(240.0))
    shader.set_line_color((0.0, 0.5, 1.0))
    shader.set_pixel_line_width(3.0)
    assert np.array_equal(_np(shader.shade_meshes(*fragments)), SU.shade_flat_edge(*[_np(fragments[i]) for i in (0, 3)], 3.0, (0.0, 0.5, 1.0)))
    from dynamicfuion_python_amd import _native
    shader.set_pixel_line_width(0.0)
    with pytest.raises(_native.NnrtError, match="pixel_line_width"):
        shader.shade_meshes(*fragments)


# ---- parity with the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("faces_per_pixel", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shaders_equal_the_restatement(nn, size, faces_per_pixel):
    R = nn.rendering
    H, W = size
    K = camera(H, W)
    drawn = 0
    for name, parts in scene_meshes(H, W, 7 * H + W).items():
        meshes = as_meshes(nn, parts)
        joined = SU.join(parts)
        for blur, convention in ((0.0, R.NDC_REFERENCE), (1.5, R.NDC_REFERENCE), (0.0, R.NDC_CONSISTENT)):
            fragments, camera_meshes = R.rasterize_meshes(meshes, K, size, blur_radius_pixels=blur, faces_per_pixel=faces_per_pixel,
                                                          cull_back_faces=False, ndc_convention=convention)
            fi, _, bary, dist = (_np(t) for t in fragments)
            assert fi.shape == (H, W, faces_per_pixel) and fi.max() < len(joined["triangle_indices"])
            covered = fi[..., 0] >= 0
            if name != "two meshes":
                assert not covered.any()
            elif blur == 0.0 and convention == R.NDC_REFERENCE:
                drawn = int(covered.sum())
            where = (name, blur, convention)
            got = _np(R.VertexColorShader().shade_meshes(*fragments, camera_meshes))
            assert got.dtype == np.uint8 and got.shape == (H, W, 3)
            assert np.array_equal(got, SU.shade_vertex_color(fi, bary, joined["triangle_indices"], joined["vertex_colors"])), where
            assert (got[~covered] == 0).all()
            for width, color in ((1.0, (1.0, 1.0, 1.0)), (2.5, (0.3, 1.7, -0.2))):
                got = _np(R.FlatEdgeShader(width, color).shade_meshes(*fragments))
                assert np.array_equal(got, SU.shade_flat_edge(fi, dist, width, color)), where + (width,)
            for color, ambient in (((0.8, 0.8, 0.8), 0.1), ((1.3, 0.5, 0.05), 0.35)):
                got = _np(R.HeadlightShader(color, ambient).shade_meshes(*fragments, camera_meshes))
                want = SU.shade_headlight(fi, bary, joined["triangle_indices"], joined["vertex_normals"], color, ambient)
                off = np.abs(got.astype(np.int32) - want.astype(np.int32))
                assert off.max(initial=0) <= 1, where + (color, int(off.max()))
                assert (got[~covered] == 0).all()
            # a zero normal gives the ambient level
            dark = [nn.geometry.TriangleMesh(m.vertex_positions, torch.zeros_like(m.vertex_normals), m.triangle_indices) for m in camera_meshes]
            got = _np(R.HeadlightShader((0.8, 0.6, 1.0), 0.25).shade_meshes(*fragments, dark))
            level = SU.to_byte(np.array([(F32(255) * F32(c)) * F32(0.25) for c in (0.8, 0.6, 1.0)], F32))
            assert (got[covered] == level).all() and (got[~covered] == 0).all(), where
    assert drawn > 0   # the pixel of the 1 x 1 image included


def test_render_meshes_moves_world_space_meshes_into_the_camera(nn):
    R = nn.rendering
    H, W = 48, 64
    parts = scene_meshes(H, W, 3)["two meshes"]
    K = camera(H, W)
    angle = 0.2
    E = np.eye(4)
    E[:3, :3] = [[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]]
    E[:3, 3] = [0.05, -0.02, 0.1]
    world = []
    for d in parts:   # world = E^-1 camera
        p = (d["vertex_positions"].astype(np.float64) - E[:3, 3]) @ E[:3, :3]
        world.append(dict(d, vertex_positions=p.astype(F32), vertex_normals=(d["vertex_normals"].astype(np.float64) @ E[:3, :3]).astype(F32)))
    shader = R.HeadlightShader()
    image, fragments = R.render_meshes(as_meshes(nn, world), K, (H, W), shader, extrinsics=E, cull_back_faces=False)
    direct, direct_fragments = R.render_meshes(as_meshes(nn, parts), K, (H, W), shader, cull_back_faces=False)
    assert len(fragments) == 4 and image.dtype == torch.uint8 and tuple(image.shape) == (H, W, 3)
    same = _np(fragments[0]) == _np(direct_fragments[0])
    assert same.mean() > 0.97   # the round trip through float32 may move a silhouette pixel
    assert np.abs(_np(fragments[1])[same] - _np(direct_fragments[1])[same]).max() < 1e-4
    assert np.abs(_np(image).astype(int) - _np(direct).astype(int))[same[..., 0]].max() <= 2


# ---- depth agreement -----------------------------------------------------------------------------------------------------
def plane_fragments(nn, H, W, faces_per_pixel, K=None, x=None, y=None):
    """A plane at z = 1 over the left part of the image (its right edge at about 70 % of the width), rasterized with raster
    pixel (u, v) = pixel (u, v) of K. The NDC extraction keeps a face only if one of its vertices is inside the image
    (ExtractClippedFaceVerticesImpl.h), so the rectangle, whose corners may lie outside, is a fan around a vertex a quarter
    pixel off the image's centre."""
    K = camera(H, W) if K is None else K
    f = K[0, 0]
    x = (-(W / f), 0.2 * W / f) if x is None else x
    y = (-(H / f), H / f) if y is None else y
    centre = [((W - 1) / 2 - 0.25 - K[0, 2]) / f, ((H - 1) / 2 + 0.25 - K[1, 2]) / K[1, 1], 1.0]
    p = np.array([[x[0], y[0], 1.0], [x[1], y[0], 1.0], [x[1], y[1], 1.0], [x[0], y[1], 1.0], centre], F32)
    mesh = nn.geometry.TriangleMesh(p, None, np.array([[4, 0, 1], [4, 1, 2], [4, 2, 3], [4, 3, 0]], np.int64))
    fragments, _ = nn.rendering.rasterize_meshes(mesh, K, (H, W), faces_per_pixel=faces_per_pixel, cull_back_faces=False,
                                                 ndc_convention=nn.rendering.NDC_CONSISTENT)
    return fragments


def frame_mm(H, W):
    """1010 mm everywhere, a block of zeros at the top left, values beyond a 3 m limit along the bottom."""
    frame = np.full((H, W), 1010, np.uint16)
    frame[: (H + 2) // 3, : (W + 3) // 4] = 0
    if H > 1:
        frame[H - (H + 3) // 4:, :] = 4000
    elif W > 1:
        frame[:, W // 2: W // 2 + W // 8] = 4000
    return frame


def check_agreement(nn, fragments, frame, scale, depth_max, threshold):
    fi, depths = _np(fragments[0]), _np(fragments[1])
    want, want_image = SU.compare_depth(fi, depths, frame, scale, depth_max, threshold)
    runs = [nn.rendering.compare_depth_to_raster(fragments[0], fragments[1], frame, scale, depth_max, threshold) for _ in range(2)]
    got, image = runs[0]
    assert image.dtype == torch.float32 and image.is_cuda and tuple(image.shape) == frame.shape
    image = _np(image)
    assert (got.both, got.model_only, got.frame_only, got.inliers) == (want["both"], want["model_only"], want["frame_only"], want["inliers"])
    assert got.both + got.model_only + got.frame_only <= frame.size
    assert np.array_equal(np.isnan(image), np.isnan(want_image))
    assert np.array_equal(image.view(np.uint32), want_image.view(np.uint32))   # NaN where stated, the same bits elsewhere
    for name in ("sum_abs", "sum_sq"):
        print(f"{frame.shape} {name}: kernel {getattr(got, name)!r}, fsum {want[name]!r}")
        assert abs(getattr(got, name) - want[name]) <= 1e-9 * abs(want[name])
    assert got.max_abs == want["max_abs"]
    assert got.rmse >= got.mean_abs * (1 - 1e-12) >= 0 and got.inliers <= got.both
    again, again_image = runs[1]
    assert again == got and np.array_equal(_np(again_image).view(np.uint32), image.view(np.uint32))   # the same bits, run to run
    return got, want


@pytest.mark.parametrize("faces_per_pixel", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_depth_agreement_equals_the_restatement(nn, size, faces_per_pixel):
    H, W = size
    fragments = plane_fragments(nn, H, W, faces_per_pixel)
    frame = frame_mm(H, W)
    got, _ = check_agreement(nn, fragments, frame, 1000.0, 3.0, 0.0101)
    covered = _np(fragments[0])[..., 0] >= 0
    assert covered[0, 0]
    if W >= 5:
        assert not covered[:, -1].any() and got.frame_only > 0   # the plane ends before the right edge
    if H * W > 1:
        assert got.model_only > 0   # zeros and values beyond the limit under the plane
    if min(H, W) >= 5:
        assert got.both > 0 and got.inliers == got.both and abs(got.mean_abs - 0.01) < 1e-4
    # a tighter threshold leaves no inlier, a nearer limit no overlap
    assert nn.rendering.compare_depth_to_raster(fragments[0], fragments[1], frame, 1000.0, 3.0, 0.005)[0].inliers == 0
    near = nn.rendering.compare_depth_to_raster(fragments[0], fragments[1], frame, 1000.0, 1.0, 0.01)[0]
    assert near.both == 0 and near.frame_only == 0 and (near.mean_abs, near.rmse, near.inlier_ratio) == (0.0, 0.0, 0.0)
    # float32 metres with a NaN, an infinity, a negative and a zero pixel
    metres = (frame.astype(F32) / F32(1000.0)).astype(F32) + np.random.default_rng(H + W).uniform(-0.02, 0.02, (H, W)).astype(F32)
    for value, (v, u) in zip((np.nan, np.inf, -1.0, 0.0), ((0, 0), (H // 2, W // 2), (H - 1, 0), (H // 2, 0))):
        metres[v, u] = value
    got, want = check_agreement(nn, fragments, metres, 1.0, 3.0, 0.01)
    assert np.isnan(_np(nn.rendering.compare_depth_to_raster(fragments[0], fragments[1], torch.from_numpy(metres), 1.0)[1])[0, 0])
    if min(H, W) >= 5:
        assert 0 < got.inliers < got.both


def test_consistent_ndc_puts_pixels_of_the_intrinsics_on_raster_pixels(nn):
    """A rectangle whose projection ends 0.4 and 0.2 pixels short of pixel centres covers exactly the pixels inside it."""
    K = np.array([[40.0, 0.0, 32.0], [0.0, 40.0, 24.0], [0.0, 0.0, 1.0]])
    fragments = plane_fragments(nn, 48, 64, 1, K, x=(-0.51, 0.26), y=(-0.41, 0.32))   # u in [11.6, 42.4], v in [7.6, 36.8]
    covered = _np(fragments[0])[..., 0] >= 0
    want = np.zeros((48, 64), bool)
    want[8:37, 12:43] = True
    assert np.array_equal(covered, want)
    assert np.abs(_np(fragments[1])[..., 0][covered] - 1.0).max() < 1e-6
    frame = np.where(want, 1010, 0).astype(np.uint16)
    frame[0, 0] = 900
    agreement, _ = nn.rendering.compare_depth_to_raster(fragments[0], fragments[1], frame)
    assert (agreement.both, agreement.model_only, agreement.frame_only) == (29 * 31, 0, 1)


def test_compare_depth_refuses_mismatched_inputs(nn):
    fragments = plane_fragments(nn, 7, 5, 1)
    with pytest.raises(ValueError):
        nn.rendering.compare_depth_to_raster(fragments[0], fragments[1], np.zeros((7, 6), np.uint16))
    with pytest.raises(ValueError):
        nn.rendering.compare_depth_to_raster(fragments[0], fragments[1], np.zeros((7, 5), np.float64))
    from dynamicfuion_python_amd import _native
    with pytest.raises(_native.NnrtError, match="depth_scale"):
        nn.rendering.compare_depth_to_raster(fragments[0], fragments[1], np.zeros((7, 5), np.uint16), depth_scale=0.0)
    empty = nn.rendering.compare_depth_to_raster(torch.zeros((0, 5, 1), dtype=torch.int64), torch.zeros((0, 5, 1)), np.zeros((0, 5), np.uint16))
    assert empty[0] == nn.rendering.DepthAgreement() and tuple(empty[1].shape) == (0, 5)


# ---- the loop -------------------------------------------------------------------------------------------------------
FRAMES = 3


def write_sequence(directory):
    """The static plane of tests/_depth_filter_util.py: a clean canonical frame, then frames with +-3 mm of seeded noise and
    holes. Colours stay above 63 so that no fused vertex colour is black."""
    from PIL import Image
    rng = np.random.default_rng(5)
    color = rng.integers(64, 256, (DF.PLANE_H, DF.PLANE_W, 3)).astype(np.uint8)
    depths = [DF.plane_depth_mm()] + [DF.noisy_plane_depth_mm(i) for i in range(1, FRAMES)]
    for i, d in enumerate(depths):
        Image.fromarray(d).save(str(directory / f"depth_{i:04d}.png"))
        Image.fromarray(color).save(str(directory / f"rgb_{i:04d}.png"))
    K = DF.PLANE_K
    rows = [[K[0, 0], 0, K[0, 2], 0], [0, K[1, 1], K[1, 2], 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    (directory / "camera_intrinsics.txt").write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in rows) + "\n")
    return depths


def make_pipeline(directory, **switches):
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.data import frame as dfr
    seq = dfr.FrameSequenceDataset(base_dataset_type=dfr.DatasetType.CUSTOM, custom_frame_directory=str(directory)).load()
    params = F.FusionParameters(graph_generation_mode=F.GraphGenerationMode.FIRST_FRAME_EXTRACTED_MESH,
                                mesh_extraction_weight_thresholding_mode=F.MeshExtractionWeightThresholdingMode.CONSTANT,
                                mesh_extraction_weight_threshold=0, **switches)
    params.alignment.max_iteration_count = 1
    params.alignment.guard_zero_rotation = True
    params.alignment.arap_term_weight = 20000.0   # nothing moves: a stiff graph keeps the fit at the residuals' level
    return F.FusionPipeline(seq, params)


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    directory = tmp_path_factory.mktemp("agreement_plane")
    return directory, write_sequence(directory)


@pytest.fixture(scope="module")
def default_run(nn, sequence):
    pipe = make_pipeline(sequence[0])
    pipe.run()
    return pipe


NEW_FIELDS = ("model_overlap_count", "model_only_count", "frame_only_count", "model_depth_mean_abs", "model_depth_rmse", "model_inlier_ratio")


def earlier_fields(result):
    d = dict(vars(result))
    d.pop("seconds")
    for name in NEW_FIELDS:
        d.pop(name)
    d["extrinsics"] = d["extrinsics"].tobytes()
    return d


def assert_same_model(a, b):
    for name in ("vertex_positions", "vertex_normals", "triangle_indices", "vertex_colors"):
        assert torch.equal(getattr(a.canonical_mesh, name), getattr(b.canonical_mesh, name)), name


def test_loop_with_the_switch_off_is_the_default_loop(nn, sequence, default_run):
    pipe = make_pipeline(sequence[0], model_agreement=False)
    pipe.run()
    assert len(pipe.results) == FRAMES == len(default_run.results)
    for a, b in zip(pipe.results, default_run.results):
        assert earlier_fields(a) == earlier_fields(b)
        assert all(getattr(a, name) == 0 and getattr(b, name) == 0 for name in NEW_FIELDS)
    assert default_run.results[-1].tracked and default_run.results[-1].canonical_triangle_count > 0
    assert_same_model(pipe, default_run)


def test_loop_scores_every_tracked_frame(nn, sequence, default_run):
    R = nn.rendering
    pipe = make_pipeline(sequence[0], model_agreement=True, model_agreement_inlier_threshold=0.004)
    taken = []
    measure = pipe.measure_model_agreement

    def measure_and_render(depth):
        # the same point of the frame: after the fit, before integration
        image, fragments = pipe.render_warped_model()
        alone, _ = R.compare_depth_to_raster(fragments[0], fragments[1], depth, 1000.0, pipe._depth_max(), 0.004)
        taken.append((alone, image, fragments, depth.clone()))
        return measure(depth)

    pipe.measure_model_agreement = measure_and_render
    pipe.run()
    assert len(pipe.results) == FRAMES and len(taken) == FRAMES - 1
    for a, b in zip(pipe.results, default_run.results):
        assert earlier_fields(a) == earlier_fields(b)
    assert_same_model(pipe, default_run)
    first = pipe.results[0]
    assert not first.tracked and all(getattr(first, name) == 0 for name in NEW_FIELDS)
    for result, (alone, image, fragments, depth), frame in zip(pipe.results[1:], taken, sequence[1][1:]):
        assert result.tracked and result.model_overlap_count > 0
        assert (result.model_overlap_count, result.model_only_count, result.frame_only_count) == (alone.both, alone.model_only, alone.frame_only)
        assert (result.model_depth_mean_abs, result.model_depth_rmse, result.model_inlier_ratio) == (alone.mean_abs, alone.rmse, alone.inlier_ratio)
        assert result.model_depth_rmse >= result.model_depth_mean_abs >= 0 and alone.inliers <= alone.both
        assert 0 <= result.model_inlier_ratio <= 1
        # the raw frame was measured, and the stand-alone call equals the restatement on it
        assert np.array_equal(_np(depth.view(torch.int16)).view(np.uint16), frame)
        want, _ = SU.compare_depth(_np(fragments[0]), _np(fragments[1]), frame, 1000.0, pipe._depth_max(), 0.004)
        assert (alone.both, alone.model_only, alone.frame_only, alone.inliers) == (want["both"], want["model_only"], want["frame_only"], want["inliers"])
        # the model is the plane the frames show, drawn where they show it
        assert alone.both > 0.8 * frame.size and result.model_depth_mean_abs < 0.01
        print(f"frame {result.frame_index}: overlap {alone.both}, model only {alone.model_only}, frame only {alone.frame_only}, "
              f"mean |d| {alone.mean_abs * 1e3:.3f} mm, rmse {alone.rmse * 1e3:.3f} mm, within 4 mm {alone.inlier_ratio:.3f}")
        assert image.dtype == torch.uint8 and image.is_cuda and tuple(image.shape) == (DF.PLANE_H, DF.PLANE_W, 3)
        assert np.array_equal(_np(image).any(-1), _np(fragments[0])[..., 0] >= 0)
    # after the run: the default shader by the mesh's attributes, a given shader, a given camera
    image, fragments = pipe.render_warped_model()
    covered = _np(fragments[0])[..., 0] >= 0
    assert covered.any() and np.array_equal(_np(image).any(-1), covered)
    grey, grey_fragments = pipe.render_warped_model(R.HeadlightShader())
    assert torch.equal(grey_fragments[0], fragments[0]) and np.array_equal(_np(grey).any(-1), covered)
    assert (_np(grey)[covered].std(-1) == 0).all() and not np.array_equal(_np(grey), _np(image))
    moved = np.eye(4)
    moved[0, 3] = 0.2
    shifted = _np(pipe.render_warped_model(extrinsics=moved)[1][0])[..., 0] >= 0
    assert shifted.any() and not np.array_equal(shifted, covered)
