"""CPU checks of VoxelBlockGrid.ray_cast: the mirror's signature against the golden row, and the float32 numpy
restatement (tests/_ray_cast_util.py, the GPU tests' yardstick) against the analytic surface of the small TSDF scene.
The volumes here are the oracle's (OracleGrid); nothing runs on a GPU."""
import inspect
import json
import os

import numpy as np
import pytest

import _ray_cast_util as RC
import _tsdf_util as TU

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_signatures.json")
EYE = np.eye(4)
DEPTH_MIN = 0.1


def test_signature_matches_the_reference_binding():
    """geometry.cpp:205: names, order and scalar defaults of ray_cast; render_attributes defaults to ("depth", "color")."""
    import dynamicfuion_python_amd.nnrt as nn
    with open(GOLDEN) as f:
        row = [r for r in json.load(f) if r["receiver"] == "voxel_block_grid" and r["name"] == "ray_cast"]
    assert len(row) == 1
    ref = row[0]["args"]
    fn = getattr(nn.geometry.VoxelBlockGrid, "ray_cast", None)
    assert fn is not None, "VoxelBlockGrid.ray_cast is missing from the mirror"
    params = list(inspect.signature(fn).parameters.values())[1:]
    assert [p.name for p in params] == [name for name, _ in ref]
    for p, (name, default) in zip(params, ref):
        if default is None:
            assert p.default is inspect.Parameter.empty, name
        elif name == "render_attributes":
            assert default == 'std::vector<std::string>{"depth", "color"}' and tuple(p.default) == ("depth", "color")
        else:
            assert p.default == float(default.rstrip("f")) and isinstance(p.default, (int, float)), name
    assert nn.geometry.NonRigidSurfaceVoxelBlockGrid.ray_cast is fn   # inherited: it renders the canonical volume


def test_analytic_surface_restates_the_scene(oracle_mod):
    sc = TU.small_tsdf_scene(oracle_mod, 0, hole=False, far_strip=False)
    v, u = np.mgrid[0:sc.H, 0:sc.W].astype(np.float64)
    assert np.array_equal(RC.small_scene_surface(sc.K)(u, v).astype(np.float32), sc.depth)


def oracle_volume(O, sc, res, weight="float32", color="float32", times=3, voxel=None):
    g = O.OracleGrid(sc.voxel_size if voxel is None else voxel, res, weight, color)
    blocks = g.touch(sc.depth, sc.K, EYE, sc.depth_scale, sc.depth_max, sc.trunc_mult)
    for _ in range(times):
        g.integrate(blocks, sc.depth, sc.color, sc.K, sc.K, EYE, sc.depth_scale, sc.depth_max, sc.trunc_mult)
    return g.values_all(), g.block_coords()


@pytest.fixture(scope="module")
def float_scene(oracle_mod):
    return TU.small_tsdf_scene(oracle_mod, 0, hole=False, far_strip=False)


@pytest.fixture(scope="module")
def volumes(oracle_mod, float_scene):
    return {res: oracle_volume(oracle_mod, float_scene, res) for res in (8, 16)}


@pytest.mark.parametrize("pose", ["integration_camera", "about_y"])
@pytest.mark.parametrize("res", [8, 16])
def test_restatement_against_the_analytic_surface(float_scene, volumes, res, pose):
    """Depth within DEPTH_TOLERANCE of the analytic surface along every hit pixel's ray, no hit where the surface is
    not, at most MISS_CAP of the expected pixels missing, unit normals that face the camera."""
    sc = float_scene
    rows, blocks = volumes[res]
    E = EYE if pose == "integration_camera" else TU.extrinsic_about_y()
    r = RC.ray_cast(rows, blocks, res, sc.voxel_size, blocks, sc.K, E, sc.W, sc.H, RC.ATTRIBUTES, sc.depth_scale, DEPTH_MIN, sc.depth_max, 3.0,
                    sc.trunc_mult, 8)
    surface = RC.small_scene_surface(sc.K)
    err, missed, expected, hits, stray = RC.compare_with_surface(r, surface, sc.K, E, sc.depth_scale, DEPTH_MIN, sc.depth_max, sc.W, sc.H,
                                                                 (sc.H, sc.W))
    print(f"res {res} {pose}: max depth error {err:.6f} m, missed {missed:.4f} of {expected}, {hits} hits, {r['steps']} steps")
    assert expected > 1000 and hits > 1000
    assert stray == 0
    assert err <= RC.MEASURED_MAX_DEPTH_ERROR     # the measurement the tolerance rests on still holds
    assert err <= RC.DEPTH_TOLERANCE
    assert missed <= RC.MISS_CAP
    assert r["steps"] < RC.step_bound(DEPTH_MIN, sc.depth_max, sc.voxel_size)   # no ray came near the trip bound
    # every map is 0 at a miss
    for name in RC.ATTRIBUTES:
        assert not r[name][~r["hit"]].any(), name
    # normals: unit length (float32: three squares, two sums, a root, a quotient -> a few ulp) or exactly 0
    hit = r["hit"]
    n = r["normal"].astype(np.float64)
    length = np.linalg.norm(n, axis=-1)
    has = length > 0
    assert has[hit].mean() > 0.9 and not has[~hit].any()
    assert np.abs(length[has] - 1.0).max() < 1e-6
    # ... and they face the camera wherever the analytic surface is seen at less than 75 degrees from its normal, there
    # and at every pixel up to 2 away (the interpolation cell of a hit next to the bump's silhouette reaches across the
    # 6 cm depth step, where the sign of n . ray is not determined by the surface)
    _, u, v = RC.analytic_depth_along_rays(surface, sc.K, E, sc.W, sc.H, DEPTH_MIN, sc.depth_max)
    cos = np.nan_to_num(RC.analytic_incidence(surface, sc.K, E, sc.W, sc.H, u, v), nan=1.0)
    padded = np.pad(cos, 2, mode="edge")
    cos = np.min([padded[dy:dy + sc.H, dx:dx + sc.W] for dy in range(5) for dx in range(5)], axis=0)
    view = r["vertex"].astype(np.float64) - np.linalg.inv(E)[:3, 3]
    facing = (n * view).sum(-1)
    steep = has & (cos > np.cos(np.deg2rad(75.0)))
    print(f"normals checked for facing: {steep.sum()} of {has.sum()}")
    assert steep.sum() > 0.8 * has.sum() and (facing[steep] < 0).all()
    # colour stays inside what was integrated
    c = r["color"][hit]
    assert c.min() >= 0.0 and c.max() <= 1.0 and c.max() > 0.5


def test_empty_inputs(float_scene, volumes):
    """Empty block_coords, and an empty grid: every range entry stays (depth_max, depth_min) and every ray misses."""
    sc = float_scene
    rows, blocks = volumes[8]
    none = np.zeros((0, 3), np.int32)
    for r in (RC.ray_cast(rows, blocks, 8, sc.voxel_size, none, sc.K, EYE, sc.W, sc.H, RC.ATTRIBUTES, 1.0, DEPTH_MIN, sc.depth_max, 3.0, 3.0, 8),
              RC.ray_cast(np.zeros((0, 8), np.float32), none, 8, sc.voxel_size, blocks, sc.K, EYE, sc.W, sc.H, RC.ATTRIBUTES, 1.0, DEPTH_MIN,
                          sc.depth_max, 3.0, 3.0, 8)):
        assert r["range"].shape == (6, 8, 2)
        assert (r["range"][..., 0] == np.float32(sc.depth_max)).all() and (r["range"][..., 1] == np.float32(DEPTH_MIN)).all()
        assert not r["hit"].any() and r["steps"] == 0
        for name in RC.ATTRIBUTES:
            assert not r[name].any()


def test_inactive_rows_and_threshold(float_scene, volumes):
    """Rows of block_coords that are not active change nothing; a weight threshold above the volume's weights misses."""
    sc = float_scene
    rows, blocks = volumes[8]
    args = (sc.K, EYE, sc.W, sc.H, RC.ATTRIBUTES, 1.0, DEPTH_MIN, sc.depth_max)
    want = RC.ray_cast(rows, blocks, 8, sc.voxel_size, blocks, *args, 3.0, 3.0, 8)
    extra = np.vstack([blocks, [[50, 50, 50], [-40, 0, 3]]]).astype(np.int32)
    got = RC.ray_cast(rows, blocks, 8, sc.voxel_size, extra, *args, 3.0, 3.0, 8)
    for k in ("range", "hit") + RC.ATTRIBUTES:
        assert np.array_equal(got[k], want[k]), k
    assert not RC.ray_cast(rows, blocks, 8, sc.voxel_size, blocks, *args, 4.0, 3.0, 8)["hit"].any()


def test_restatement_at_the_fusion_loop_configuration(oracle_mod):
    """FusionParameters' defaults (voxel 5 mm, 16^3 blocks, uint16 weight and colour, truncation 5 voxels, depth in
    millimetres, depth_max 3 m) after two integrations of the small scene's uint16 frame, cast at weight threshold 1:
    against the frame's own depth, what tests/test_gpu_ray_cast.py asks of FusionPipeline.render_canonical_model."""
    sc = TU.small_tsdf_scene(oracle_mod, 0, u16=True, hole=False, far_strip=False)
    sc.depth_max, sc.trunc_mult = 3.0, 0.025 / 0.005
    rows, blocks = oracle_volume(oracle_mod, sc, 16, "uint16", "uint16", times=2, voxel=0.005)
    r = RC.ray_cast(rows, blocks, 16, 0.005, blocks, sc.K, EYE, sc.W, sc.H, ("depth", "normal"), 1000.0, DEPTH_MIN, 3.0, 1.0, sc.trunc_mult, 8)
    err, missed, expected = RC.compare_with_input_depth(r, sc.depth / 1000.0, DEPTH_MIN, 3.0, 1000.0)
    print(f"fusion configuration: max depth error {err:.6f} m, missed {missed:.4f} of {expected}")
    assert expected == (sc.H - 2 * RC.BORDER_CUT) * (sc.W - 2 * RC.BORDER_CUT)
    assert err <= RC.DEPTH_TOLERANCE and missed <= RC.MISS_CAP
