"""The depth filters on the GPU (csrc/depth_filter.hip: k_median_depth, k_bilateral_depth) against the numpy restatements of
DESIGN §20 (tests/_depth_filter_util.py), bit for bit, at the image sizes where tiling, halo and clipping can go wrong, and
the fusion loop's depth-filter switch on a small noisy static sequence."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _depth_filter_util as DF  # noqa: E402

U16 = np.uint16
# 1 x 1; smaller than any window; one tile; one pixel past a tile both ways; ragged; several whole tiles
SHAPES = [(1, 1), (3, 5), (16, 16), (17, 33), (37, 53), (64, 48)]
RADII = [0, 1, 3, 8]   # 8: the halo is as wide as the tile
SCALAR_LOOP_LIMIT = 15000  # window visits up to which the scalar restatement is run as well as its image form


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import nnrt
    return nnrt


def _np(t):
    return t.detach().cpu().numpy()


def random_depth(shape, seed):
    """uint16 over the full range (values >= 32768 included) with 30 % zeros."""
    rng = np.random.default_rng(seed)
    d = rng.integers(1, 65536, shape).astype(U16)
    d[rng.random(shape) < 0.3] = 0
    return d


def contents(shape, seed):
    single = np.zeros(shape, U16)
    single[shape[0] // 2, shape[1] - 1] = 40000
    return {"random": random_depth(shape, seed), "zero": np.zeros(shape, U16), "single": single, "constant": np.full(shape, 51234, U16)}


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_median_equals_the_restatement(nn, shape, radius):
    for name, image in contents(shape, 100 * radius + shape[1]).items():
        for preserve in (False, True):
            got = nn.filter_depth(image, radius, preserve_zero=preserve)
            assert got.dtype == torch.uint16 and got.is_cuda and tuple(got.shape) == shape
            want = DF.median_restatement(image, radius, preserve)
            assert np.array_equal(_np(got.view(torch.int16)).view(U16), want), (name, preserve)


def test_median_overloads_and_input_kinds(nn):
    image = random_depth((37, 53), 3)
    want = DF.median_restatement(image, 3)
    assert want.max() >= 32768   # values past the int16 range survive the int16 transport
    dev = torch.device("cuda", torch.cuda.current_device())
    as_torch = torch.from_numpy(image.view(np.int16)).to(dev).view(torch.uint16)
    for source in (image, as_torch, torch.from_numpy(image.view(np.int16)).view(torch.uint16), as_torch.view(torch.int16)):
        assert np.array_equal(_np(nn.filter_depth(source, 3).view(torch.int16)).view(U16), want)
        assert np.array_equal(_np(nn.filter_depth(depth_image_in=source, radius=3).view(torch.int16)).view(U16), want)
    out = torch.zeros((37, 53), dtype=torch.int16, device=dev).view(torch.uint16)
    assert nn.filter_depth(as_torch, out, 3) is None
    assert np.array_equal(_np(out.view(torch.int16)).view(U16), want)
    out.zero_()
    assert nn.filter_depth(image, depth_image_out=out, radius=3, preserve_zero=True) is None
    assert np.array_equal(_np(out.view(torch.int16)).view(U16), DF.median_restatement(image, 3, True))
    assert np.array_equal(_np(as_torch.view(torch.int16)).view(U16), image)   # the input is not modified
    from dynamicfuion_python_amd import _native
    with pytest.raises(ValueError):
        nn.filter_depth(as_torch, torch.zeros((37, 52), dtype=torch.int16, device=dev), 3)
    with pytest.raises(ValueError):
        nn.filter_depth(as_torch, torch.zeros((37, 53), dtype=torch.int16), 3)
    with pytest.raises(ValueError):
        nn.filter_depth(image.astype(np.float32), 3)
    with pytest.raises(_native.NnrtError, match="d_out must not be d_in"):
        nn.filter_depth(as_torch, as_torch, 3)
    with pytest.raises(_native.NnrtError, match="radius"):
        nn.filter_depth(as_torch, 9)
    assert tuple(nn.filter_depth(np.zeros((0, 5), U16), 2).shape) == (0, 5)


def bilateral_raw(image, radius, spatial, weights, index_scale, depth_scale):
    """The C entry point with caller-supplied tables."""
    from dynamicfuion_python_amd import _native as N
    dev = torch.device("cuda", torch.cuda.current_device())
    if image.dtype == U16:
        d, code = torch.from_numpy(image.view(np.int16)).to(dev), 1
    else:
        d, code = torch.from_numpy(image).to(dev), 0
    out = torch.full(image.shape, -1.0, dtype=torch.float32, device=dev)
    spatial, weights = np.ascontiguousarray(spatial, np.float32), np.ascontiguousarray(weights, np.float32)
    N.check(N.lib().nnrt_bilateral_filter_depth(N.ptr(d), code, image.shape[0], image.shape[1], radius, N.ptr(spatial), N.ptr(weights),
                                                len(weights), ctypes.c_float(index_scale), ctypes.c_float(depth_scale), N.ptr(out), N.stream_ptr()))
    return _np(out)


def bilateral_want(image, radius, spatial, weights, index_scale, depth_scale):
    want = DF.bilateral_restatement_images(image, radius, spatial, weights, index_scale, depth_scale)
    if image.size * (2 * radius + 1) ** 2 <= SCALAR_LOOP_LIMIT:
        assert np.array_equal(want, DF.bilateral_restatement(image, radius, spatial, weights, index_scale, depth_scale))
    return want


def smooth_depth(shape, seed, step=True):
    """A slanted surface around 1500 units with +-20 units of noise, 30 % zeros, a far side beyond any cutoff used here
    (values >= 32768) right of the middle column, and a few full-range outliers."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:shape[0], 0:shape[1]]
    d = 1500 + 3 * u + 2 * v + rng.integers(-20, 21, shape)
    if step:
        d[:, shape[1] // 2:] += 40000
    outliers = rng.random(shape) < 0.02
    d[outliers] = rng.integers(1, 65536, shape)[outliers]
    d[rng.random(shape) < 0.3] = 0
    return d.astype(U16)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bilateral_equals_the_restatement(nn, shape, radius):
    from dynamicfuion_python_amd.nnrt.image_proc import bilateral_weight_tables
    sigma_s = max(radius / 2.0, 0.5)
    images = contents(shape, 10 * radius + shape[0])
    images["smooth"] = smooth_depth(shape, radius + shape[1])
    for name, image in images.items():
        # uint16, the default cutoff ceil(3 * 30) = 90: the step's far side is excluded
        spatial, weights = bilateral_weight_tables(radius, sigma_s, 30.0)
        got = _np(nn.image_proc.bilateral_filter_depth(image, radius, sigma_s, 30.0))
        want = bilateral_want(image, radius, spatial, weights, 1.0, 1000.0)
        assert got.dtype == np.float32 and np.array_equal(got, want), name
        assert np.array_equal(got == 0, image == 0)   # the centre always contributes: valid pixels stay valid, holes stay holes
        # float32 metres: the table is indexed in millimetres, the output is not rescaled
        metres = (image.astype(np.float32) / np.float32(1000.0)).astype(np.float32)
        got = _np(nn.image_proc.bilateral_filter_depth(metres, radius, sigma_s, 30.0, depth_scale=1000.0))
        assert np.array_equal(got, bilateral_want(metres, radius, spatial, weights, 1000.0, 1.0)), name
    image = images["smooth"]
    # cutoff 0: one range weight, only equal values mix
    spatial, weights = bilateral_weight_tables(radius, sigma_s, 30.0, 0)
    assert weights.shape == (1,)
    got = _np(nn.image_proc.bilateral_filter_depth(image, radius, sigma_s, 30.0, range_cutoff=0, depth_scale=1.0))
    assert np.array_equal(got, bilateral_want(image, radius, spatial, weights, 1.0, 1.0))
    # the largest table, 4096 entries
    spatial, weights = bilateral_weight_tables(radius, sigma_s, 1365.0)
    assert weights.shape == (4096,)
    got = _np(nn.image_proc.bilateral_filter_depth(image, radius, sigma_s, 1365.0))
    assert np.array_equal(got, bilateral_want(image, radius, spatial, weights, 1.0, 1000.0))
    # caller-supplied tables that are no Gaussians (zeros included), a fractional index scale, straight to the C entry point
    rng = np.random.default_rng(radius)
    spatial = rng.random((2 * radius + 1) ** 2).astype(np.float32)
    spatial[rng.random(spatial.shape) < 0.2] = 0.0
    weights = rng.random(300).astype(np.float32)
    weights[::7] = 0.0
    got = bilateral_raw(image, radius, spatial, weights, 0.37, 5000.0)
    assert np.array_equal(got, bilateral_want(image, radius, spatial, weights, 0.37, 5000.0))
    assert (got[image == 0] == 0).all()


def test_bilateral_float_input_with_invalid_values(nn):
    rng = np.random.default_rng(4)
    metres = (0.8 + 0.4 * rng.random((37, 53))).astype(np.float32)
    metres[3, 3], metres[5, 40], metres[20, 20], metres[36, 52], metres[0, 0] = np.nan, np.inf, -1.0, 0.0, 3.0e38
    from dynamicfuion_python_amd.nnrt.image_proc import bilateral_weight_tables
    spatial, weights = bilateral_weight_tables(3, 1.5, 60.0)
    got = _np(nn.image_proc.bilateral_filter_depth(torch.from_numpy(metres), 3, 1.5, 60.0))
    assert np.array_equal(got, DF.bilateral_restatement_images(metres, 3, spatial, weights, 1000.0, 1.0))
    assert got[3, 3] == 0 and got[5, 40] == 0 and got[20, 20] == 0 and got[36, 52] == 0 and np.isfinite(got).all()


def test_bilateral_keeps_the_step_and_shrinks_noise(nn):
    """The two properties tests/test_depth_filter_cpu.py measures on the restatement, on the kernel, at the same bounds."""
    import test_depth_filter_cpu as C
    image = C.step_edge()
    got = _np(nn.image_proc.bilateral_filter_depth(image, 3, 1.5, 30.0, range_cutoff=90)).astype(np.float64)
    deviation = float(np.abs(got - image / 1000.0).max())
    print(f"step edge: largest deviation from the pixel's own side {deviation!r} m")
    assert deviation <= C.STEP_EDGE_BOUND
    plane, noisy = C.noisy_image_plane()
    got = _np(nn.image_proc.bilateral_filter_depth(noisy, 3, 1.5, 30.0, depth_scale=1.0)).astype(np.float64)
    before, after = float(np.sqrt(np.mean((noisy - plane) ** 2))), float(np.sqrt(np.mean((got - plane) ** 2)))
    print(f"noisy plane: RMS distance {before:.4f} units before, {after:.4f} after")
    assert after < before


# ---- the loop -------------------------------------------------------------------------------------------------------
FRAMES = 3


def write_noisy_sequence(directory):
    """Frame 0 is the clean plane (the canonical frame); the tracked frames carry +-3 mm of seeded noise and zeroed pixels."""
    from PIL import Image
    rng = np.random.default_rng(2)
    color = rng.integers(0, 256, (DF.PLANE_H, DF.PLANE_W, 3)).astype(np.uint8)
    depths = [DF.plane_depth_mm()] + [DF.noisy_plane_depth_mm(i) for i in range(1, FRAMES)]
    for i, d in enumerate(depths):
        Image.fromarray(d).save(str(directory / f"depth_{i:04d}.png"))
        Image.fromarray(color).save(str(directory / f"rgb_{i:04d}.png"))
    K = DF.PLANE_K
    rows = [[K[0, 0], 0, K[0, 2], 0], [0, K[1, 1], K[1, 2], 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    (directory / "camera_intrinsics.txt").write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in rows) + "\n")
    return depths


def run_loop(directory, **filters):
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.data import frame as dfr
    seq = dfr.FrameSequenceDataset(base_dataset_type=dfr.DatasetType.CUSTOM, custom_frame_directory=str(directory)).load()
    # a constant extraction threshold of 0: with raw noisy normals the cosine test of integrate_non_rigid lets so few voxels
    # gain weight that the default ramp (1 after the second frame) would leave the unfiltered run nothing to track
    params = F.FusionParameters(graph_generation_mode=F.GraphGenerationMode.FIRST_FRAME_EXTRACTED_MESH,
                                mesh_extraction_weight_thresholding_mode=F.MeshExtractionWeightThresholdingMode.CONSTANT,
                                mesh_extraction_weight_threshold=0, **filters)
    params.alignment.max_iteration_count = 1
    params.alignment.guard_zero_rotation = True
    params.alignment.arap_term_weight = 20000.0   # nothing moves: a stiff graph keeps the fit at the residuals' level
    pipe = F.FusionPipeline(seq, params)
    pipe.run()
    return pipe


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    directory = tmp_path_factory.mktemp("noisy_plane")
    return directory, write_noisy_sequence(directory)


@pytest.fixture(scope="module")
def default_run(nn, sequence):
    return run_loop(sequence[0])


def comparable(result):
    d = dict(vars(result))
    d.pop("seconds")
    d["extrinsics"] = d["extrinsics"].tobytes()
    return d


def test_loop_with_both_radii_zero_is_the_default_loop(nn, sequence, default_run):
    pipe = run_loop(sequence[0], depth_median_radius=0, depth_bilateral_radius=0)
    assert len(pipe.results) == FRAMES == len(default_run.results)
    for a, b in zip(pipe.results, default_run.results):
        assert comparable(a) == comparable(b) and a.depth_filtered is False
    assert default_run.results[-1].tracked and default_run.results[-1].canonical_triangle_count > 0
    for name in ("vertex_positions", "vertex_normals", "triangle_indices"):
        assert torch.equal(getattr(pipe.canonical_mesh, name), getattr(default_run.canonical_mesh, name)), name
    raw = nn.backproject_depth_ushort(sequence[1][-1], pipe.fx, pipe.fy, pipe.cx, pipe.cy, 1000.0)
    assert torch.equal(pipe.tracking_point_image, raw)


def test_loop_tracks_filtered_depth(nn, sequence, default_run):
    pipe = run_loop(sequence[0], depth_median_radius=1, depth_bilateral_radius=3)
    assert len(pipe.results) == FRAMES and not pipe.results[0].depth_filtered and not pipe.results[0].tracked
    for r in pipe.results[1:]:
        assert r.tracked and r.depth_filtered and r.canonical_triangle_count > 0
    last = sequence[1][-1]
    # the point image of the last tracked frame: the two filters and the back-projection, called directly
    median = nn.filter_depth(last, 1, preserve_zero=True)
    metres = nn.image_proc.bilateral_filter_depth(median, 3, 1.5, 30.0, depth_scale=1000.0)
    points = nn.backproject_depth_float(metres, pipe.fx, pipe.fy, pipe.cx, pipe.cy)
    assert torch.equal(pipe.tracking_point_image, points)
    # ... and those equal the restatements
    want_median = DF.median_restatement(last, 1, True)
    assert np.array_equal(_np(median.view(torch.int16)).view(U16), want_median)
    from dynamicfuion_python_amd.nnrt.image_proc import bilateral_weight_tables
    spatial, weights = bilateral_weight_tables(3, 1.5, 30.0)
    assert np.array_equal(_np(metres), DF.bilateral_restatement_images(want_median, 3, spatial, weights, 1.0, 1000.0))
    # the median alone goes through the uint16 back-projection
    only_median = run_loop(sequence[0], depth_median_radius=1)
    assert only_median.results[-1].tracked and only_median.results[-1].depth_filtered
    assert torch.equal(only_median.tracking_point_image, nn.backproject_depth_ushort(median, pipe.fx, pipe.fy, pipe.cx, pipe.cy, 1000.0))
    # normals of the filtered points are closer to the plane's than those of the raw points
    size = (DF.PLANE_H, DF.PLANE_W)
    raw_points = nn.backproject_depth_ushort(last, pipe.fx, pipe.fy, pipe.cx, pipe.cy, 1000.0)
    angle_raw, count_raw = DF.mean_angle_to_plane_normal(_np(nn.geometry.compute_ordered_point_cloud_normals(raw_points.reshape(-1, 3), size)))
    angle_filtered, count_filtered = DF.mean_angle_to_plane_normal(_np(nn.geometry.compute_ordered_point_cloud_normals(points.reshape(-1, 3), size)))
    print(f"mean angle to the plane's normal: raw {angle_raw:.3f} deg over {count_raw} pixels, filtered {angle_filtered:.3f} deg over {count_filtered}")
    assert count_raw > 40000 and count_filtered > 40000
    assert angle_filtered < angle_raw
    off = [r.seconds for r in default_run.results[1:]]
    on = [r.seconds for r in pipe.results[1:]]
    print(f"tracked frame time: filters off {min(off) * 1e3:.2f} ms, filters on {min(on) * 1e3:.2f} ms (256 x 192, best of {len(on)})")


def test_loop_refuses_radii_out_of_range(nn, sequence):
    with pytest.raises(ValueError, match="depth_median_radius"):
        run_loop(sequence[0], depth_median_radius=9)
    with pytest.raises(ValueError, match="depth_bilateral_radius"):
        run_loop(sequence[0], depth_bilateral_radius=-1)
