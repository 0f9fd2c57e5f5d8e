"""CPU: the TSDF voxel-block-grid oracle restatement (oracle/tsdf_oracle.cpp) against the reference's own known-answer
tests (cpp/tests/test_non_rigid_surface_voxel_block_grid.cpp, transcribed in tests/golden/kat_literals.py) and
structural properties of the generated marching-cubes table."""
import numpy as np
import pytest

from golden import kat_literals as L
import _tsdf_util as TU


def test_warped_block_boxes_kat(oracle_mod):
    O = oracle_mod
    t = np.tile(L.VBG_BOX_TRANSLATION, (4, 1))
    R = np.tile(np.eye(3, dtype=np.float32), (4, 1, 1))
    boxes = O.warped_block_boxes(L.VBG_BOX_KEYS, L.VBG_BOX_VOXEL_SIZE * L.VBG_BOX_RESOLUTION, L.VBG_BOX_NODES, R, t,
                                 L.VBG_BOX_COVERAGE, 4, 0, np.eye(4))
    assert np.allclose(boxes, L.VBG_BOX_EXPECTED)


def test_boxes_intercepting_surface_mask_kat(oracle_mod):
    m = oracle_mod.boxes_mask(L.VBG_MASK_BOXES, L.VBG_MASK_DEPTH, L.VBG_MASK_K, 1.0, 100.0, 1, 0.5)
    assert np.array_equal(m.astype(bool), L.VBG_MASK_EXPECTED)


def _kat_volume(O, apply_oblique_test):
    plane, color, K, deformed, nodes, R, t = TU.reference_nonrigid_kat_inputs()
    g = O.OracleGrid(0.01, 8, "uint16", "uint16")
    blocks = g.touch(plane, K, np.eye(4), 1000.0, 3.0, 2.0)
    g.integrate(blocks, plane, color, K, K, np.eye(4), 1000.0, 3.0, 2.0)
    pts = TU.unproject_points(deformed, K)
    normals = O.ordered_point_cloud_normals(pts, 100, 100)
    cos = g.integrate_non_rigid(np.array([[0, 0, 1]], np.int32), nodes, R, t, 0.005, 4, 1, deformed, color, normals, K, K, np.eye(4),
                                1000.0, 3.0, 2.0, apply_oblique_test=apply_oblique_test)
    return g, blocks, cos


def test_integrate_non_rigid_kat(oracle_mod):
    """The reference KAT's expected rows follow from its code with the oblique-view test (`cosine > 0.5`,
    NonRigidSurfaceVoxelBlockGridImpl.h:192) left out: the camera-facing normals of ComputeOrderedPointCloudNormals
    (NormalsOperationsImpl.h:208-210) give cosine ~1 on the plane, which that test rejects. With the test, as the code
    reads, the non-rigid update never applies there; both facts are checked."""
    g, blocks, _ = _kat_volume(oracle_mod, apply_oblique_test=False)
    assert {tuple(b) for b in blocks} == {(x, y, 0) for x in (-1, 0) for y in (-1, 0)}
    rows = g.values_at(L.VBG_NR_QUERIES)
    assert np.allclose(rows, L.VBG_NR_EXPECTED, rtol=1e-5, atol=5e-6)
    g2, _, cos = _kat_volume(oracle_mod, apply_oblique_test=True)
    rows2 = g2.values_at(L.VBG_NR_QUERIES)
    assert (cos[20:80, 20:80] > 0.5).any()
    # as written: every row keeps its rigid-integration value (weight 1, the non-rigid pass never reached the update)
    assert np.allclose(rows2[:, 4], 1.0) and np.allclose(rows2[:, 5:], 100.0)
    assert np.allclose(rows2[[0, 3, 4], 3], 0.0, atol=1e-6)


def test_marching_cubes_table_properties(oracle_mod):
    """Each cube state's triangles use exactly its crossing edges; closed sphere -> watertight, consistently oriented,
    Euler characteristic 2, outward normals."""
    g = oracle_mod.OracleGrid(0.1, 8)
    coords = np.array([[x, y, z] for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)], np.int32)
    g.activate(coords)
    vals = g.values_all()
    # write a sphere SDF through an integration-free path: tsdf from positions (radius 0.37, truncated to [-1, 1])
    r = np.linalg.norm(vals[:, :3] + 0.05, axis=1)
    _sphere_fill(oracle_mod, g, np.clip((r - 0.37) / 0.3, -1, 1).astype(np.float32))
    V, Nn, _, T = g.mesh(0.0)
    assert len(T) > 100
    edges = {}
    for tri in T:
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            edges[(a, b)] = edges.get((a, b), 0) + 1
    assert all(c == 1 for c in edges.values()), "a directed edge repeats: inconsistent orientation"
    assert all((b, a) in edges for (a, b) in edges), "open boundary: not watertight"
    assert len(V) - len(edges) // 2 + len(T) == 2
    cen = V[T].mean(1)
    fn = np.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]])
    assert (np.einsum("ij,ij->i", fn, cen + 0.05) > 0).mean() > 0.99, "triangles must face away from negative tsdf"
    assert (np.einsum("ij,ij->i", Nn, V + 0.05) > 0).mean() > 0.99


def _sphere_fill(O, g, tsdf):
    # weights 1 (> threshold 0) and the given tsdf, written by integrating nothing and patching through a raw pointer
    import ctypes
    lib = O.lib()
    lib.orc_grid_set_values.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    w = np.ones_like(tsdf)
    lib.orc_grid_set_values(g.h, tsdf.ctypes.data, w.ctypes.data)


CUBE_CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
CUBE_EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]


def _mc_python(vol, tri):
    """Marching cubes in plain Python with a [256, >=16] emission-order table (bit c: corner c has value < 0)."""
    verts, tris, states = {}, [], set()
    nx, ny, nz = vol.shape

    def vid(x, y, z, e):
        a, b = CUBE_EDGES[e]
        p = (x + CUBE_CORNERS[a][0], y + CUBE_CORNERS[a][1], z + CUBE_CORNERS[a][2])
        q = (x + CUBE_CORNERS[b][0], y + CUBE_CORNERS[b][1], z + CUBE_CORNERS[b][2])
        key = (min(p, q), max(p, q))
        if key not in verts:
            r = (0.0 - vol[p]) / (vol[q] - vol[p])
            verts[key] = (len(verts), np.array(p, float) + r * (np.array(q, float) - np.array(p, float)))
        return verts[key][0]

    for x in range(nx - 1):
        for y in range(ny - 1):
            for z in range(nz - 1):
                idx = sum(1 << c for c in range(8) if vol[x + CUBE_CORNERS[c][0], y + CUBE_CORNERS[c][1], z + CUBE_CORNERS[c][2]] < 0)
                states.add(idx)
                row = tri[idx]
                for t in range(0, len(row), 3):
                    if row[t] < 0:
                        break
                    tris.append(tuple(vid(x, y, z, int(e)) for e in row[t:t + 3]))
    V = np.zeros((len(verts), 3))
    for i, p in verts.values():
        V[i] = p
    return V, np.array(tris, np.int64), states


def test_marching_cubes_table_is_the_published_one(oracle_mod):
    """The product's and the oracle's marching-cubes tables (csrc/mc_table.hpp, oracle/mc_table_oracle.hpp: the published
    Lorensen-Cline / Bourke table that Open3D's ExtractTriangleMesh indexes, VoxelBlockGrid.cpp:461-497) are equal in
    emission order; every cube state uses exactly its crossing edges; random volumes -- every one of the 256 states --
    give closed, consistently oriented surfaces whose triangles face away from negative values. Topology parity with
    Open3D's own meshes stays unpinned (no Open3D output exists here)."""
    from dynamicfuion_python_amd.nnrt.voxel_grid import marching_cubes_table
    tri_p, mask_p = marching_cubes_table()
    tri_o = oracle_mod.marching_cubes_table()
    for cfg in range(256):   # the product's rows end at their first -1
        end = int(np.argmax(tri_p[cfg] < 0))
        assert np.array_equal(tri_p[cfg, :end], tri_o[cfg, :end]) and (tri_o[cfg, end:] == -1).all(), cfg
    # Bourke's row 1 is (0, 8, 3); Open3D stores table vertex v at triangle slot 2 - v, so it emits (3, 8, 0)
    assert list(tri_o[1, :4]) == [3, 8, 0, -1] and list(tri_p[1, :4]) == [3, 8, 0, -1]
    ntri = [(tri_o[c] >= 0).sum() // 3 for c in range(256)]
    assert max(ntri) == 5 and ntri[0] == ntri[255] == 0
    for cfg in range(256):
        inside = [(cfg >> c) & 1 for c in range(8)]
        cross = {e for e, (a, b) in enumerate(CUBE_EDGES) if inside[a] != inside[b]}
        assert set(int(e) for e in tri_o[cfg] if e >= 0) == cross, cfg
        assert mask_p[cfg] == sum(1 << e for e in cross)
    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(4):
        vol = rng.uniform(-1, 1, (12, 12, 12))
        vol[[0, -1], :, :] = vol[:, [0, -1], :] = vol[:, :, [0, -1]] = 1.0   # outside on the border: closed surfaces
        V, T, states = _mc_python(vol, tri_o)
        seen |= states
        directed = {}
        for t in T:
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                directed[(a, b)] = directed.get((a, b), 0) + 1
        assert all(c == 1 for c in directed.values()), "inconsistent orientation"
        assert all((b, a) in directed for (a, b) in directed), "open boundary"
    n = 20
    g = np.mgrid[0:n, 0:n, 0:n].transpose(1, 2, 3, 0).astype(float)
    V, T, _ = _mc_python(np.linalg.norm(g - 9.5, axis=-1) - 6.3, tri_o)
    fn = np.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]])
    assert (np.einsum("ij,ij->i", fn, V[T].mean(1) - 9.5) > 0).all()
    assert len(seen) >= 250


def _growth_case(O, grow_surface):
    """One block (0, 0, 6) of 8^3 voxels (z = 0.48 ... 0.55), a flat depth of 0.515 m, one node at the origin with identity
    motion and a coverage that reaches every voxel (so a voxel warps onto itself, exactly), camera-facing normals except
    on the image rows below 8, which have none. Returns the voxel rows, the cosine map and the numpy expectation."""
    f32 = np.float32
    K = TU.simple_intrinsics(100.0, 4.0, 4.0)
    depth = np.full((24, 24), 0.515, f32)
    normals = np.tile(f32([0, 0, -1]), (24, 24, 1))
    normals[:8] = 0
    g = O.OracleGrid(0.01, 8)
    cos = g.integrate_non_rigid(np.array([[0, 0, 6]], np.int32), np.zeros((1, 3), f32), np.eye(3, dtype=f32)[None], np.zeros((1, 3), f32), 1.0,
                                1, 1, depth, None, normals.reshape(-1, 3), K, K, np.eye(4), 1.0, 3.0, 3.0, grow_surface=grow_surface)
    rows = g.values_all()
    x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
    assert z.min() == f32(48) * f32(0.01) and z.max() == f32(55) * f32(0.01)
    iz = f32(1) / z
    u, v = np.floor((f32(100) * x) * iz + f32(4) + f32(0.5)).astype(int), np.floor((f32(100) * y) * iz + f32(4) + f32(0.5)).astype(int)
    assert u.max() < 24 and v.max() < 24
    trunc = f32(0.01) * f32(3.0)
    psdf = f32(0.515) - z
    in_band = psdf > -trunc
    assert in_band.sum() == 7 * 64 and (psdf[in_band] < trunc).any() and (psdf[in_band] >= trunc).any()
    tsdf = np.where(psdf < trunc, psdf, trunc) / trunc
    return rows, cos, u, v, in_band, tsdf, v >= 8


def test_growth_mode_off_keeps_the_reference_rule(oracle_mod):
    """Growth off (the default): the weight is never counted and voxels seen head-on (cosine > 0.5) are skipped; only
    pixels without a normal (cosine 0) pass the reference's oblique test."""
    rows, cos, u, v, in_band, tsdf, has_normal = _growth_case(oracle_mod, False)
    assert (rows[:, 4] == 0).all()
    assert has_normal.any() and (~has_normal).any()
    assert (cos[v[has_normal], u[has_normal]] > 0.9).all()
    assert (rows[has_normal, 3] == 0).all()
    upd = in_band & ~has_normal
    assert np.array_equal(rows[upd, 3], tsdf[upd]) and (rows[~in_band, 3] == 0).all()


def test_growth_mode_on_counts_head_on_observations(oracle_mod):
    """Growth on: exactly the voxels within the truncation band that see a camera-facing normal get weight 1 and
    tsdf = min(psdf, trunc) / trunc; pixels with a zero normal (cosine 0) are skipped."""
    rows, cos, u, v, in_band, tsdf, has_normal = _growth_case(oracle_mod, True)
    upd = in_band & has_normal
    assert 0 < upd.sum() < in_band.sum()
    assert np.array_equal(rows[:, 4], upd.astype(np.float32))
    assert np.array_equal(rows[:, 3], np.where(upd, tsdf, np.float32(0)))
    assert (cos[v[~has_normal], u[~has_normal]] == 0).all() and (rows[~has_normal, 3:5] == 0).all()


def test_growth_mode_counts_weights_through_the_typed_store(oracle_mod):
    """uint16 weights and uint8 color: two growth-mode passes leave weight 2 and the truncated running color average."""
    O = oracle_mod
    K = TU.simple_intrinsics(100.0, 4.0, 4.0)
    depth = np.full((24, 24), 515, np.uint16)
    normals = np.tile(np.float32([0, 0, -1]), (24 * 24, 1))
    g = O.OracleGrid(0.01, 8, "uint16", "uint8")
    for value in (100, 201):
        g.integrate_non_rigid(np.array([[0, 0, 6]], np.int32), np.zeros((1, 3), np.float32), np.eye(3, dtype=np.float32)[None],
                              np.zeros((1, 3), np.float32), 1.0, 1, 1, depth, np.full((24, 24, 3), value, np.uint8), normals, K, K, np.eye(4),
                              1000.0, 3.0, 3.0, grow_surface=True)
    rows = g.values_all()
    seen = rows[:, 4] > 0
    assert seen.sum() == 7 * 64 and (rows[seen, 4] == 2).all()
    assert (rows[seen, 5:] == 150).all()   # (1 * 100 + 201) / 2 = 150.5, truncated by the uint8 store
