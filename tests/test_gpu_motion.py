"""The motion images and the flow comparison on the GPU (csrc/motion.hip: k_motion_pixels, k_flow_error,
k_flow_error_finish) against the numpy restatements of DESIGN §32 (tests/_motion_util.py) and against a known rigid
motion, at the image sizes where a lane-per-pixel launch and a two-stage reduction can go wrong, and the fusion loop's
motion-image switch on the small static sequence of tests/test_gpu_shading.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _depth_filter_util as DF  # noqa: E402
import _motion_util as MU  # noqa: E402
import test_gpu_shading as TS  # noqa: E402  (write_sequence, make_pipeline, assert_same_model: the loop tests' helpers)

F32 = np.float32
EPS = 2.0 ** -24
# 1 x 1; under one wavefront; exactly one workgroup; 255 pixels; one pixel past a workgroup; several workgroups with K = 2
MOTION_CASES = [(1, 1, 1), (7, 9, 1), (16, 16, 1), (15, 17, 1), (1, 257, 1), (33, 31, 2)]


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import nnrt
    return nnrt


def _np(t):
    return t.detach().cpu().numpy()


def camera(H, W):
    """synthetic.grid_mesh spans 1.2 m x 0.9 m around z = 1.2: about 70 % of the image each way, so every vertex projects into
    the image (the NDC extraction keeps a face only if one of its vertices does) and the border stays background. The
    principal point is a fraction of a pixel off the image's centre."""
    return np.array([[0.7 * W, 0.0, (W - 1) / 2 + 0.13], [0.0, 0.7 * H / 0.75, (H - 1) / 2 + 0.21], [0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def mesh():
    from dynamicfuion_python_amd import synthetic
    points, _, faces = synthetic.grid_mesh(5, 4)   # 24 triangles
    rng = np.random.default_rng(32)
    moved = (points + rng.normal(0.0, 0.01, points.shape)).astype(F32)
    return points, faces, moved


def fragments_of(nn, points, faces, H, W, faces_per_pixel=1):
    fragments, _ = nn.rendering.rasterize_meshes(nn.geometry.TriangleMesh(points, None, faces), camera(H, W), (H, W),
                                                 faces_per_pixel=faces_per_pixel, cull_back_faces=False,
                                                 ndc_convention=nn.rendering.NDC_CONSISTENT)
    return fragments


def check_motion(nn, fragments, faces, source, target, K):
    """The kernel against the restatement: the blends bit for bit, the optical flow within its bound."""
    got = nn.rendering.motion_from_fragments(fragments[0], fragments[2], faces, source, target, K)
    H, W = fragments[0].shape[:2]
    for name, channels, dtype in (("source_points", 3, torch.float32), ("scene_flow", 3, torch.float32), ("optical_flow", 2, torch.float32)):
        image = getattr(got, name)
        assert image.is_cuda and image.dtype == dtype and tuple(image.shape) == (H, W, channels), name
    assert got.mask.dtype == torch.bool and tuple(got.mask.shape) == (H, W)
    want = MU.motion_images(_np(fragments[0]), _np(fragments[2]), faces, source, target, K)
    mask = _np(got.mask)
    assert np.array_equal(mask, want["mask"])
    for name in ("source_points", "scene_flow"):
        assert np.array_equal(_np(getattr(got, name)).view(np.uint32), want[name].view(np.uint32)), name
    flow = _np(got.optical_flow)
    excess = np.abs(flow.astype(np.float64) - want["optical_flow64"]) / MU.optical_flow_bound(want["optical_flow_scale"])[..., None]
    print(f"{H}x{W}: {int(mask.sum())} valid pixels, optical flow error at most {excess.max():.3f} of its bound")
    assert excess.max() <= 1.0
    assert not flow[~mask].any() and not _np(got.source_points)[~mask].any() and not _np(got.scene_flow)[~mask].any()
    return got, want


@pytest.mark.parametrize("H,W,faces_per_pixel", MOTION_CASES, ids=lambda v: str(v))
def test_motion_pixels_equal_the_restatement(nn, mesh, H, W, faces_per_pixel):
    points, faces, moved = mesh
    fragments = fragments_of(nn, points, faces, H, W, faces_per_pixel)
    assert tuple(fragments[0].shape) == (H, W, faces_per_pixel)
    covered = _np(fragments[0])[..., 0] >= 0
    got, want = check_motion(nn, fragments, faces, points, moved, camera(H, W))
    assert covered.any() and np.array_equal(_np(got.mask), covered)   # every covered pixel has both points in front of the camera
    if min(H, W) >= 7:
        assert not covered.all()   # the border is background
    # target vertices behind the camera: the pixels whose blended target point has z <= 0 are invalid and zero (the face drawn
    # on the most pixels is behind with all three vertices, its neighbours with one or two)
    behind = moved.copy()
    behind[faces[np.bincount(_np(fragments[0])[..., 0][covered]).argmax()], 2] = -50.0
    got, _ = check_motion(nn, fragments, faces, points, behind, camera(H, W))
    lost = covered & ~_np(got.mask)
    assert lost.any() and not _np(got.scene_flow)[lost].any() and not _np(got.optical_flow)[lost].any()
    # a source vertex behind the camera does the same
    got, _ = check_motion(nn, fragments, faces, behind, moved, camera(H, W))
    assert (covered & ~_np(got.mask)).any()


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    A = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * A + (1 - np.cos(angle)) * A @ A


def test_a_rigid_motion_gives_its_known_flow(nn, mesh):
    points, faces, _ = mesh
    H, W = 24, 32
    K = camera(H, W)
    source = nn.geometry.TriangleMesh(points, None, faces)
    R, t = rotation([0.3, 1.0, -0.2], 0.05), np.array([0.01, -0.02, 0.03])
    target = (points.astype(np.float64) @ R.T + t).astype(F32)
    images, fragments = nn.rendering.render_motion(source, target, K, (H, W))
    mask = _np(images.mask)
    covered = _np(fragments[0])[..., 0] >= 0
    assert tuple(fragments[0].shape) == (H, W, 1) and mask.any() and not mask.all() and np.array_equal(mask, covered)
    ps = _np(images.source_points).astype(np.float64)[mask]
    want = ps @ (R - np.eye(3)).T + t
    bound = 4 * EPS * (3 * np.abs(ps).sum(1) + np.abs(t).max() + 1)
    error = np.abs(_np(images.scene_flow).astype(np.float64)[mask] - want)
    print(f"scene flow error at most {(error / bound[:, None]).max():.3f} of its bound")
    assert (error <= bound[:, None]).all()
    # the optical flow is the projection difference of the source point and the source point moved by (R, t)
    pt = ps @ R.T + t
    f = [float(F32(v)) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2])]
    us, ut = MU._project(ps, *f), MU._project(pt, *f)
    scale = np.maximum.reduce([np.ones(len(ps)), np.abs(us).max(1), np.abs(ut).max(1), np.full(len(ps), abs(f[2])), np.full(len(ps), abs(f[3]))])
    error = np.abs(_np(images.optical_flow).astype(np.float64)[mask] - (ut - us))
    print(f"optical flow error at most {(error / MU.optical_flow_bound(scale)[:, None]).max():.3f} of its bound")
    assert (error <= MU.optical_flow_bound(scale)[:, None]).all()
    assert np.abs(ut - us).max() > 0.5   # the motion is visible
    # the identity: both flows are exactly zero everywhere
    still, _ = nn.rendering.render_motion(source, points, K, (H, W))
    assert np.array_equal(_np(still.mask), mask)
    assert not _np(still.scene_flow).any() and not _np(still.optical_flow).any()
    assert np.array_equal(_np(still.source_points), _np(images.source_points))
    # extrinsics: a world-space mesh moved into the cameras is the camera-space call
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = rotation([0, 0, 1], 0.02), [0.01, 0.0, 0.02]
    world = nn.geometry.TriangleMesh(((points.astype(np.float64) - E[:3, 3]) @ E[:3, :3]).astype(F32), None, faces)
    moved, _ = nn.rendering.render_motion(world, world.vertex_positions, K, (H, W), source_extrinsics=E, target_extrinsics=E)
    assert _np(moved.mask).sum() > 0.9 * mask.sum() and not _np(moved.scene_flow).any()
    with pytest.raises(ValueError, match="target_vertex_positions"):
        nn.rendering.render_motion(source, points[:-1], K, (H, W))
    with pytest.raises(ValueError):
        nn.rendering.motion_from_fragments(fragments[0], fragments[2][:-1], faces, points, points, K)


# ---- the flow comparison ---------------------------------------------------------------------------------------------------
# 1, 63, 64, 65, 256 and 257 pixels; 7 records; 67 records, more than the finish launch's wavefront has lanes
FLOW_SIZES = [(1, 1), (7, 9), (8, 8), (5, 13), (16, 16), (1, 257), (40, 40), (130, 130)]
THRESHOLD = 0.05


def flow_inputs(H, W, C):
    """Predicted flow with four pixels in five drawn; truth = predicted + noise of about the inlier threshold, with NaN and
    -inf in single channels of some pixels; a truth mask with five pixels in six valid."""
    rng = np.random.default_rng(1000 * C + H * W)
    predicted = rng.normal(0.0, 1.0, (H, W, C)).astype(F32)
    drawn = rng.random((H, W)) < 0.8
    truth = (predicted + rng.normal(0.0, 0.03, (H, W, C))).astype(F32)
    holes = rng.random((H, W))
    channel = rng.integers(0, C, (H, W))
    for value, (low, high) in ((np.nan, (0.0, 0.06)), (-np.inf, (0.06, 0.12))):
        v, u = np.nonzero((holes >= low) & (holes < high))
        truth[v, u, channel[v, u]] = value
    known = rng.random((H, W)) < 5 / 6
    return predicted, drawn, truth, known


def check_flow(nn, predicted, drawn, truth, known):
    H, W, _ = predicted.shape
    n = H * W
    want, want_image = MU.flow_error(predicted, drawn, truth, known, THRESHOLD)
    runs = [nn.rendering.compare_flow(predicted, drawn, truth, known, inlier_threshold=THRESHOLD) for _ in range(2)]
    got, image = runs[0]
    assert image.dtype == torch.float32 and image.is_cuda and tuple(image.shape) == (H, W)
    image = _np(image)
    assert (got.both, got.predicted_only, got.truth_only, got.inliers) == (want["both"], want["predicted_only"], want["truth_only"], want["inliers"])
    assert got.max_epe == want["max_epe"]
    for name in ("sum_epe", "sum_sq"):
        print(f"{H}x{W} {name}: kernel {getattr(got, name)!r}, numpy {want[name]!r}")
        assert abs(getattr(got, name) - want[name]) <= n * 2.0 ** -53 * abs(want[name])
    both = np.asarray(drawn, bool) & np.isfinite(truth).all(-1) & (True if known is None else np.asarray(known, bool))
    assert np.array_equal(np.isnan(image), ~both)
    assert np.array_equal(image.view(np.uint32)[both], want_image.view(np.uint32)[both])   # the double's nearest float32
    again, again_image = runs[1]
    assert again == got and np.array_equal(_np(again_image).view(np.uint32), image.view(np.uint32))   # the same bits, run to run
    assert got.rmse >= got.mean_epe * (1 - 1e-12) >= 0 and got.inliers <= got.both
    return got


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("size", FLOW_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_flow_error_equals_the_restatement(nn, size, C):
    H, W = size
    predicted, drawn, truth, known = flow_inputs(H, W, C)
    got = check_flow(nn, predicted, drawn, truth, known)
    if H * W >= 63:
        assert got.both > 0 and got.predicted_only > 0 and got.truth_only > 0 and 0 < got.inliers < got.both
    absent = check_flow(nn, predicted, drawn, truth, None)   # no truth mask: the non-finite pixels alone are invalid
    assert absent.both >= got.both and absent.both + absent.predicted_only == int(drawn.sum())
    # nothing drawn, nothing known, both: the record is all zeros bar the one-sided count
    nothing = check_flow(nn, predicted, np.zeros((H, W), bool), truth, known)
    assert (nothing.both, nothing.predicted_only, nothing.sum_epe, nothing.max_epe, nothing.mean_epe) == (0, 0, 0.0, 0.0, 0.0)
    unknown = check_flow(nn, predicted, drawn, truth, np.zeros((H, W), np.uint8))
    assert (unknown.both, unknown.truth_only, unknown.predicted_only) == (0, 0, int(drawn.sum()))
    # every pixel valid and predicted == truth: zero error everywhere, every pixel an inlier
    same = check_flow(nn, predicted, np.ones((H, W), bool), predicted, None)
    assert (same.both, same.inliers, same.sum_epe, same.sum_sq, same.max_epe) == (H * W, H * W, 0.0, 0.0, 0.0)


def test_compare_flow_refuses_mismatched_inputs(nn):
    flow, mask = np.zeros((7, 5, 3), F32), np.ones((7, 5), bool)
    with pytest.raises(ValueError):
        nn.rendering.compare_flow(flow, mask, np.zeros((7, 5, 2), F32), inlier_threshold=0.1)
    with pytest.raises(ValueError):
        nn.rendering.compare_flow(flow, mask[:-1], flow, inlier_threshold=0.1)
    with pytest.raises(ValueError):
        nn.rendering.compare_flow(flow, mask, flow, mask[:, :-1], inlier_threshold=0.1)
    with pytest.raises(ValueError):
        nn.rendering.compare_flow(np.zeros((7, 5, 4), F32), mask, np.zeros((7, 5, 4), F32), inlier_threshold=0.1)
    with pytest.raises(TypeError):
        nn.rendering.compare_flow(flow, mask, flow)   # the threshold has no default
    from dynamicfuion_python_amd import _native
    with pytest.raises(_native.NnrtError, match="inlier_threshold"):
        nn.rendering.compare_flow(flow, mask, flow, inlier_threshold=-1.0)
    empty = nn.rendering.compare_flow(np.zeros((0, 5, 2), F32), np.zeros((0, 5), bool), np.zeros((0, 5, 2), F32), inlier_threshold=0.1)
    assert empty[0] == nn.rendering.FlowAgreement() and tuple(empty[1].shape) == (0, 5)


# ---- the loop -------------------------------------------------------------------------------------------------------------
MOTION_FIELDS = ("motion_pixel_count", "scene_flow_count", "scene_flow_epe_mean", "scene_flow_rmse", "optical_flow_count",
                 "optical_flow_epe_mean", "optical_flow_rmse")


def fields_before(result):
    """A FrameResult without its clock and without the fields of the motion images."""
    d = dict(vars(result))
    d.pop("seconds")
    for name in MOTION_FIELDS:
        d.pop(name)
    d["extrinsics"] = d["extrinsics"].tobytes()
    return d


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    directory = tmp_path_factory.mktemp("motion_plane")
    TS.write_sequence(directory)
    return directory


@pytest.fixture(scope="module")
def plain_run(nn, sequence):
    pipe = TS.make_pipeline(sequence, motion_images=False)
    pipe.run()
    return pipe


@pytest.fixture(scope="module")
def motion_run(nn, sequence):
    """The loop with motion images and a provider that hands back the frame's own motion field as the truth."""
    seen = []

    def provider(pipeline, frame):
        motion = pipeline.last_motion
        seen.append((frame.frame_index, motion, int(motion.mask.sum())))
        return {"scene_flow": motion.scene_flow.clone(), "scene_flow_mask": motion.mask.clone(),
                "optical_flow": motion.optical_flow.clone(), "optical_flow_mask": None}

    from dynamicfuion_python_amd import fusion as F
    pipe = TS.make_pipeline(sequence, motion_images=True)
    pipe = F.FusionPipeline(pipe.sequence, pipe.parameters, flow_truth_provider=provider)
    pipe.run()
    return pipe, seen


def test_loop_renders_the_motion_of_every_tracked_frame(nn, motion_run):
    pipe, seen = motion_run
    assert len(pipe.results) == TS.FRAMES and len(seen) == TS.FRAMES - 1
    first = pipe.results[0]
    assert not first.tracked and all(getattr(first, name) == 0 for name in MOTION_FIELDS)
    for result, (frame_index, motion, count) in zip(pipe.results[1:], seen):
        assert result.tracked and result.frame_index == frame_index
        assert result.motion_pixel_count == count > 0
        assert tuple(motion.scene_flow.shape) == (DF.PLANE_H, DF.PLANE_W, 3) and tuple(motion.mask.shape) == (DF.PLANE_H, DF.PLANE_W)
    motion = pipe.last_motion
    assert motion is seen[-1][1]
    assert tuple(motion.source_points.shape) == (DF.PLANE_H, DF.PLANE_W, 3) and tuple(motion.optical_flow.shape) == (DF.PLANE_H, DF.PLANE_W, 2)
    # a static plane under a stiff graph: the model's motion between two frames is far below a millimetre and a pixel
    assert float(motion.scene_flow.abs().max()) < 1e-3 and float(motion.optical_flow.abs().max()) < 1.0
    # a state against itself does not move
    still, fragments = pipe.render_model_motion(pipe.active_graph, pipe.extrinsics)
    assert tuple(fragments[0].shape) == (DF.PLANE_H, DF.PLANE_W, 1)
    assert bool(still.mask.any()) and not bool(still.scene_flow.any()) and not bool(still.optical_flow.any())
    # and against another state it does, by that state's translation
    shifted = pipe.active_graph.clone()
    shifted.set_node_translations(shifted.get_node_translations() + F32([0.0, 0.0, 0.01]))
    moved, _ = pipe.render_model_motion(pipe.active_graph, pipe.extrinsics, shifted)
    both = moved.mask & still.mask
    assert bool(both.any()) and float((moved.scene_flow[both] - torch.tensor([0.0, 0.0, 0.01], device=both.device)).abs().max()) < 1e-5


def test_loop_scores_its_own_motion_field_as_exact(nn, motion_run):
    pipe, _ = motion_run
    for result in pipe.results[1:]:
        assert result.scene_flow_count == result.motion_pixel_count > 0
        assert result.optical_flow_count == result.motion_pixel_count
        assert (result.scene_flow_epe_mean, result.scene_flow_rmse, result.optical_flow_epe_mean, result.optical_flow_rmse) == (0.0, 0.0, 0.0, 0.0)


def test_loop_with_motion_images_tracks_and_fuses_as_without(nn, plain_run, motion_run):
    pipe, _ = motion_run
    assert plain_run.last_motion is None and plain_run.flow_truth_provider is None
    assert len(plain_run.results) == TS.FRAMES == len(pipe.results)
    for a, b in zip(plain_run.results, pipe.results):
        assert fields_before(a) == fields_before(b)
        assert all(getattr(a, name) == 0 for name in MOTION_FIELDS)
    assert plain_run.results[-1].tracked and plain_run.results[-1].canonical_triangle_count > 0
    for name in ("get_node_rotations", "get_node_translations", "get_node_positions"):
        assert np.array_equal(getattr(plain_run.active_graph, name)().view(np.uint32), getattr(pipe.active_graph, name)().view(np.uint32)), name
    TS.assert_same_model(plain_run, pipe)
