"""The inputs of tests/test_gpu_raster_shapes.py, checked without a GPU: at every (size, options) set the GPU file runs,
the oracle's three rasterizers agree bit for bit (so the reference side is sound at portrait, odd and thin sizes), and
branch_census -- a numpy restatement of raster.hip's branch conditions -- shows that the set reaches the code it is
there for: all three scatter modes, staged and unstaged waves in the 32- and the 64-face grouping, a row deal of more
than one round, every rejection cause. Where a size cannot meet a condition the test asserts the exemption and why."""
import numpy as np
import pytest

from _raster_shape_util import (DEAL_ROUND, DENSE_FACES_PER_WAVE, DENSE_TILE_KEYS, FACES_PER_WAVE, FIT_SHAPES, RASTER_OPTIONS, RASTER_SIZES,
                                TILE_KEYS, blur_ndc, branch_census, near_all_side, ndc_range, pixel_centres, shape_scene, shape_soup)
from _util import oracle_fit_scene, scene_target

# pixels with a face after one oracle iteration from the identity (recorded)
FIT_COVERED = {(53, 37): 1305, (37, 53): 1659, (107, 75): 5169, (75, 107): 6279, (17, 129): 527, (129, 17): 405, (33, 47): 1293}
SETS = [(H, W, blur, persp, clip) for (H, W) in RASTER_SIZES for (blur, persp, clip) in RASTER_OPTIONS]


def _id(s):
    return f"{s[0]}x{s[1]}-blur{s[2]}-{'persp' if s[3] else 'flat'}-{'clip' if s[4] else 'noclip'}"


def test_pixel_centres_and_ranges():
    """The restated pixel formula: the short axis spans (-1, 1), the long one (-d1/d2, d1/d2), centres symmetric about
    0 and half a pixel inside the range -- for portrait and landscape alike."""
    for H, W in RASTER_SIZES:
        for d1, d2 in ((W, H), (H, W)):
            c = pixel_centres(d1, d2).astype(np.float64)
            r = max(d1 / d2, 1.0)
            assert abs(float(ndc_range(d1, d2)) - 2 * r) < 1e-6 * r
            assert np.allclose(c, -r + (2 * np.arange(d1) + 1) * r / d1, atol=4e-7 * r)
            assert (np.diff(c) > 0).all()


@pytest.mark.parametrize("H,W", RASTER_SIZES, ids=lambda v: str(v))
def test_soup_layout(H, W):
    f, m = shape_soup(H, W)
    assert f.dtype == np.float32 and f.shape[1:] == (3, 3) and m.dtype == np.uint8 and len(m) == len(f)
    assert len(f) % 128 != 0
    assert 0.05 < 1.0 - m.mean() < 0.15
    assert (~np.isfinite(f)).any(axis=(1, 2)).sum() == 4
    f2, m2 = shape_soup(H, W)
    assert np.array_equal(f, f2, equal_nan=True) and np.array_equal(m, m2)


@pytest.mark.parametrize("s", SETS, ids=_id)
def test_oracle_rasterizers_agree(oracle_mod, s):
    H, W, blur, persp, clip = s
    f, m = shape_soup(H, W)
    for k in (1, 4):
        binned = oracle_mod.rasterize(f, m, H, W, blur, k, -1, -1, persp, clip, True)
        brute = oracle_mod.rasterize(f, m, H, W, blur, k, 0, -1, persp, clip, True)
        for a, b in zip(binned, brute):
            assert np.array_equal(a, b)
        if k == 1 and not clip:   # (rasterize_k1_fast has no barycentric clipping)
            fast = oracle_mod.rasterize_k1_fast(f, m, H, W, blur, persp, True)
            for a, b in zip(binned, fast):
                assert np.array_equal(a, b)


@pytest.mark.parametrize("s", SETS, ids=_id)
def test_set_reaches_its_branches(oracle_mod, s):
    H, W, blur, persp, clip = s
    f, m = shape_soup(H, W)
    c = branch_census(f, m, H, W, blur, clip)
    print(f"census {_id(s)}: {c}")
    assert c["mode"][0] >= 20
    if near_all_side(H, W, blur) <= 0:
        # no face can be near_all: its blur-widened box has a squared diagonal of at least 8 b^2, which is below b / 2
        # only for b < 1 / 16, i.e. min(H, W) > 16 blur_px (and never at blur 0)
        b = float(blur_ndc(blur, H, W))
        assert blur == 0 or min(H, W) <= 16 * blur
        assert 8 * b * b >= 0.5 * b
        assert c["mode"][1] == 0 and c["mode"][2] == 0
    elif clip:
        assert c["mode"][1] >= 20
        assert c["mode"][2] == 0   # clip_barycentric keeps every near_all face on the guarded quotients
    else:
        assert c["mode"][1] >= 20  # near_all faces at depths of 1e10 and more: outside face_rows_fast's range
        assert c["mode"][2] >= 20
    for g, keys in ((FACES_PER_WAVE, TILE_KEYS), (DENSE_FACES_PER_WAVE, DENSE_TILE_KEYS)):
        assert c[f"staged{g}"] >= 1
        if H * W <= keys:
            assert c[f"unstaged{g}"] == 0   # the whole image fits the wave's tile
        else:
            assert c[f"unstaged{g}"] >= 1
        if H * g <= DEAL_ROUND:
            assert c[f"multi_round{g}"] == 0   # g faces of at most H rows each: one round of 64 holds them
        else:
            assert c[f"multi_round{g}"] >= 1
    for cause, n in c["rejected"].items():
        assert n >= 1, cause
    k8 = oracle_mod.rasterize(f, m, H, W, blur, 8, -1, -1, persp, clip, True)[0]
    hits = (k8 >= 0).sum(-1)
    assert (hits >= 1).mean() >= 0.25
    assert (hits >= 4).sum() >= 1   # K = 4's bounded queue fills: later hits run its replacement test
    assert (hits >= 5).sum() >= 1 or H * W < 4


def test_coincident_faces_tie_goes_to_the_lower_index(oracle_mod):
    """The two coincident specials have equal depth everywhere: with the nearer faces over them masked out, the oracle
    picks the lower index, and never the higher."""
    H, W = 37, 53
    f, m = shape_soup(H, W)
    eq = [i for i in range(len(f) - 1) if np.array_equal(f[i], f[i + 1])]
    assert len(eq) == 1
    lo = eq[0]
    only = np.zeros_like(m)
    only[[lo, lo + 1]] = 1
    fi = oracle_mod.rasterize(f, only, H, W, 0.5, 1, -1, -1, True, False, True)[0]
    assert (fi == lo).sum() > 20 and (fi == lo + 1).sum() == 0


@pytest.mark.parametrize("H,W,fx", FIT_SHAPES, ids=lambda v: str(v))
def test_fit_scenes_on_the_oracle(oracle_mod, H, W, fx):
    """The fused-iteration scenes: the oracle runs a finite iteration, a fair share of the pixels see a face, and the mesh
    has more faces than the image has pixels or not as the launch-switch tests assume."""
    sc = shape_scene(H, W, fx)
    depth = scene_target(oracle_mod, sc)
    assert depth.shape == (H, W)
    _, _, dg = oracle_fit_scene(oracle_mod, sc, depth, 1)
    covered = int((dg["pixel_faces"] >= 0).sum())
    print(f"{H}x{W}: {covered} pixels with a face, {int(dg['residual_mask'].sum())} residuals")
    assert covered == FIT_COVERED[(H, W)] and dg["residual_mask"].sum() >= 0.9 * covered
    assert np.isfinite(dg["updates"]).all() and np.isfinite(dg["hessian_diag"]).all()
    if (H, W) in ((53, 37), (107, 75)):
        assert len(sc.faces) == 2 * 48 * 36
        assert (len(sc.faces) >= H * W) == ((H, W) == (53, 37))   # the dense scatter is the default at 53 x 37 only
