"""The depth filters' semantics without a GPU: the numpy restatements of tests/_depth_filter_util.py on
hand-made images whose answers are written out here, the weight tables against their formula, the mirror's signatures,
and the two properties the loop relies on (an edge wider than the cutoff is not blurred; noise on a plane shrinks),
measured on the restatement before the GPU tests assert them of the kernels."""
import inspect
import math

import numpy as np
import pytest

import _depth_filter_util as DF

U16 = np.uint16


def test_median_even_count_takes_the_upper_median():
    image = np.zeros((5, 5), U16)
    image[2, 1:5] = [10, 40, 20, 30]          # row 2: 0 10 40 20 30
    out = DF.median_restatement(image, 1)
    # window of (2, 2): 10 40 20 -> index 1 of (10, 20, 40); of (2, 3): 40 20 30 -> 30; of (2, 1): 10 40 -> index 1 = 40
    assert out[2, 2] == 20 and out[2, 3] == 30
    assert out[2, 1] == 40                    # two values: the upper one
    assert out[2, 4] == 30                    # 20 30 -> upper
    assert out[1, 0] == 10 and out[3, 0] == 10   # a single value in the window
    assert out[0, 0] == 0 and out[4, 4] == 0 and out[0, 4] == 0   # nothing in the window: 0, where the reference indexes an empty vector


def test_median_all_zero_and_hole_handling():
    assert not DF.median_restatement(np.zeros((5, 5), U16), 2).any()
    image = np.full((5, 5), 7, U16)
    image[2, 2] = 0
    filled = DF.median_restatement(image, 1, preserve_zero=False)
    kept = DF.median_restatement(image, 1, preserve_zero=True)
    assert filled[2, 2] == 7 and np.array_equal(filled, np.full((5, 5), 7, U16))   # the reference's behaviour: the hole is filled
    want = np.full((5, 5), 7, U16)
    want[2, 2] = 0
    assert np.array_equal(kept, want)
    # a valid pixel next to holes is filtered in both modes: the window skips the zeros
    image = np.array([[0, 0, 0, 0, 0], [0, 9, 0, 0, 0], [0, 0, 5, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], U16)
    assert DF.median_restatement(image, 1, preserve_zero=True)[1, 1] == 9     # (5, 9) -> index 1
    assert DF.median_restatement(image, 1, preserve_zero=True)[0, 0] == 0
    assert DF.median_restatement(image, 1, preserve_zero=False)[0, 0] == 9    # silhouettes dilate by the radius
    assert DF.median_restatement(image, 1, preserve_zero=False)[4, 4] == 0


def test_median_corner_windows_are_clipped_and_extreme_values_survive():
    image = np.arange(1, 26, dtype=U16).reshape(5, 5)      # 1 .. 25, row-major
    out = DF.median_restatement(image, 1)
    assert out[0, 0] == 6       # (1, 2, 6, 7) -> index 2
    assert out[0, 4] == 9       # (4, 5, 9, 10) -> index 2
    assert out[4, 0] == 21      # (16, 17, 21, 22) -> index 2
    assert out[4, 4] == 24      # (19, 20, 24, 25) -> index 2
    assert out[0, 2] == 7       # (2, 3, 4, 7, 8, 9) -> index 3
    assert out[2, 2] == 13      # the full 3 x 3 window: its middle
    assert np.array_equal(DF.median_restatement(image, 0), image)
    assert np.array_equal(DF.median_restatement(image, 8), np.full((5, 5), 13, U16))   # every window is the whole image
    image = np.full((5, 5), 65535, U16)
    image[0] = 1
    out = DF.median_restatement(image, 1)
    assert out[0, 0] == 65535 and out[0, 2] == 65535      # (1, 1, 65535, 65535) -> index 2; six values -> index 3
    assert out[2, 2] == 65535
    image = np.full((5, 5), 1, U16)
    image[4, 4] = 65535
    out = DF.median_restatement(image, 1)
    assert out[4, 4] == 1 and out[0, 0] == 1
    assert DF.median_restatement(np.array([[65535]], U16), 3)[0, 0] == 65535
    assert DF.median_restatement(np.array([[1]], U16), 3)[0, 0] == 1


def _tables(radius, spatial_sigma, range_sigma, range_cutoff=None):
    from dynamicfuion_python_amd.nnrt.image_proc import bilateral_weight_tables
    return bilateral_weight_tables(radius, spatial_sigma, range_sigma, range_cutoff)


def test_weight_tables_follow_the_formula():
    for radius, s_s, s_r, cutoff in ((3, 1.5, 30.0, None), (8, 4.0, 12.5, 40), (1, 0.5, 1365.0, None), (0, 1.0, 2.0, 0)):
        spatial, weights = _tables(radius, s_s, s_r, cutoff)
        n = (math.ceil(3 * s_r) if cutoff is None else cutoff) + 1
        assert spatial.dtype == np.float32 and weights.dtype == np.float32
        assert spatial.shape == (2 * radius + 1, 2 * radius + 1) and weights.shape == (n,)
        assert spatial[radius, radius] == 1.0 and weights[0] == 1.0
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                want = math.exp(-(dx * dx + dy * dy) / (2.0 * s_s * s_s))
                assert abs(float(spatial[dy + radius, dx + radius]) - want) <= float(np.spacing(np.float32(want)))
        steps = np.arange(n, dtype=np.float64)
        want = np.exp(-steps * steps / (2.0 * s_r * s_r))
        assert (np.abs(weights.astype(np.float64) - want) <= np.spacing(want.astype(np.float32)).astype(np.float64)).all()
    assert _tables(1, 0.5, 1365.0)[1].shape == (4096,)     # the largest table the library takes
    for bad in ((-1, 1.0, 1.0, None), (2, 0.0, 1.0, None), (2, 1.0, -3.0, None), (2, 1.0, 1.0, -1)):
        with pytest.raises(ValueError):
            _tables(*bad)


def test_filter_depth_signatures_are_the_reference_s():
    from dynamicfuion_python_amd import nnrt
    assert nnrt.filter_depth is nnrt.image_proc.filter_depth
    into, new = nnrt.filter_depth.signatures()
    positional = inspect.Parameter.POSITIONAL_OR_KEYWORD

    def leading(sig):
        return [p.name for p in sig.parameters.values() if p.kind == positional]
    assert leading(into) == ["depth_image_in", "depth_image_out", "radius"]     # nnrt_pybind.cpp:97-99
    assert leading(new) == ["depth_image_in", "radius"]                         # nnrt_pybind.cpp:100-102
    for sig in (into, new):
        assert all(p.default is inspect.Parameter.empty for p in sig.parameters.values() if p.kind == positional)
        extra = [p for p in sig.parameters.values() if p.kind != positional]
        assert [(p.name, p.kind, p.default) for p in extra] == [("preserve_zero", inspect.Parameter.KEYWORD_ONLY, False)]
    with pytest.raises(TypeError):
        nnrt.filter_depth(np.zeros((2, 2), U16))
    with pytest.raises(TypeError):
        nnrt.filter_depth(np.zeros((2, 2), U16), 1.5)


def test_image_form_of_the_bilateral_restatement_equals_the_scalar_loop():
    rng = np.random.default_rng(5)
    for (H, W), radius, cutoff in (((7, 9), 1, 50), ((6, 5), 3, 0), ((9, 11), 2, 20000)):
        d = rng.integers(0, 65536, (H, W)).astype(U16)
        d[rng.random((H, W)) < 0.3] = 0
        d[0, 0] = d[0, 1]   # an equal pair: difference 0
        spatial, _ = _tables(radius, 1.2, 30.0, 1)
        weights = rng.random(min(cutoff + 1, 4096)).astype(np.float32)
        a = DF.bilateral_restatement(d, radius, spatial, weights, 1.0, 1000.0)
        b = DF.bilateral_restatement_images(d, radius, spatial, weights, 1.0, 1000.0)
        assert np.array_equal(a, b) and a.any()
    f = (rng.random((8, 7)) * 2.0).astype(np.float32)
    f[1, 1], f[2, 2], f[3, 3], f[4, 4] = np.nan, np.inf, -1.0, 3.0e38
    spatial, weights = _tables(2, 1.0, 400.0)
    a = DF.bilateral_restatement(f, 2, spatial, weights, 1000.0, 1.0)
    b = DF.bilateral_restatement_images(f, 2, spatial, weights, 1000.0, 1.0)
    assert np.array_equal(a, b) and a[1, 1] == 0 and a[2, 2] == 0 and a[3, 3] == 0 and a[4, 4] == np.float32(3.0e38)


# the largest |out - side| of the step-edge case below in metres, as measured on the restatement; the bound
# is four times it, the margin DESIGN §18 uses for float32 rounding noise
STEP_EDGE_MEASURED = 2.622604369229009e-07
STEP_EDGE_BOUND = 4.0 * STEP_EDGE_MEASURED


def step_edge():
    image = np.full((12, 16), 1000, U16)
    image[:, 8:] = 1400
    return image


def test_bilateral_keeps_a_step_wider_than_the_cutoff():
    image = step_edge()
    spatial, weights = _tables(3, 1.5, 30.0, 90)
    out = DF.bilateral_restatement(image, 3, spatial, weights, 1.0, 1000.0)
    assert np.array_equal(out, DF.bilateral_restatement_images(image, 3, spatial, weights, 1.0, 1000.0))
    side = image.astype(np.float64) / 1000.0
    deviation = float(np.abs(out.astype(np.float64) - side).max())
    print(f"step edge 1000 | 1400, cutoff 90: largest deviation from the pixel's own side {deviation!r} m")
    assert deviation <= STEP_EDGE_BOUND
    # without the cutoff the far side would leak in: with a table wide enough to reach it the edge pixels move
    _, wide = _tables(3, 1.5, 300.0, 500)
    blurred = DF.bilateral_restatement_images(image, 3, spatial, wide, 1.0, 1000.0)
    assert float(np.abs(blurred.astype(np.float64) - side).max()) > 0.01


def noisy_image_plane():
    rng = np.random.default_rng(11)
    v, u = np.mgrid[0:48, 0:64].astype(np.float64)
    plane = 1000.0 + 0.5 * u + 0.25 * v
    return plane, np.round(plane + rng.uniform(-3.0, 3.0, plane.shape)).astype(U16)


def test_bilateral_shrinks_noise_on_a_plane():
    plane, noisy = noisy_image_plane()
    spatial, weights = _tables(3, 1.5, 30.0)
    out = DF.bilateral_restatement_images(noisy, 3, spatial, weights, 1.0, 1.0)
    before = float(np.sqrt(np.mean((noisy.astype(np.float64) - plane) ** 2)))
    after = float(np.sqrt(np.mean((out.astype(np.float64) - plane) ** 2)))
    print(f"noisy plane, +-3 units: RMS distance to the plane {before:.4f} units before, {after:.4f} after")
    assert after < before


def test_filters_bring_normals_of_the_noisy_plane_closer(oracle_mod):
    """The loop test's inequality (tests/test_gpu_depth_filter.py), first on the restatement: median radius 1 with holes
    kept, then bilateral radius 3, on the 256 x 192 plane with +-3 mm noise and zeroed pixels."""
    noisy = DF.noisy_plane_depth_mm(1)
    median = DF.median_restatement(noisy, 1, preserve_zero=True)
    assert np.array_equal(median == 0, noisy == 0)
    spatial, weights = _tables(3, 1.5, 30.0)
    metres = DF.bilateral_restatement_images(median, 3, spatial, weights, 1.0, 1000.0)
    raw = oracle_mod.ordered_point_cloud_normals(DF.backproject(noisy / 1000.0).reshape(-1, 3), DF.PLANE_H, DF.PLANE_W)
    filtered = oracle_mod.ordered_point_cloud_normals(DF.backproject(metres).reshape(-1, 3), DF.PLANE_H, DF.PLANE_W)
    angle_raw, count_raw = DF.mean_angle_to_plane_normal(raw)
    angle_filtered, count_filtered = DF.mean_angle_to_plane_normal(filtered)
    print(f"mean angle to the plane's normal: raw {angle_raw:.3f} deg over {count_raw} pixels, filtered {angle_filtered:.3f} deg over {count_filtered}")
    assert count_raw > 40000 and count_filtered > 40000
    assert angle_filtered < angle_raw
