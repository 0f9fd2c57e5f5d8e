"""Scene builders for the TSDF voxel-block-grid tests (inputs of the reference KAT, cpp/tests/
test_non_rigid_surface_voxel_block_grid.cpp:176-341, and a larger synthetic DynamicFusion-like frame)."""
import numpy as np


def simple_intrinsics(f=100.0, cx=50.0, cy=50.0):
    return np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])


def hemisphere_pinch(depth_mm: np.ndarray, radius: int, height_mm: float) -> np.ndarray:
    """HemisphereAtDepthImageCenter (:196-227): float32 tensor math as Open3D, rounded half away from zero."""
    d = int(radius) * 2
    step = 2.0 / (d - 1)
    lin = np.arange(-1.0, 1.0, step).astype(np.float32)
    lin = np.append(lin, np.float32(1.0)).astype(np.float32)
    assert lin.shape[0] == d
    y = (lin.reshape(1, d) * np.float32(radius)).astype(np.float32)
    x = (lin.reshape(d, 1) * np.float32(radius)).astype(np.float32)
    z2 = (np.float32(radius * radius) * np.ones((d, d), np.float32) - x * x - y * y).astype(np.float32)
    z2[z2 < 0] = 0
    z = np.sqrt(z2).astype(np.float32)
    delta = (np.float32(height_mm) * (z / z.max())).astype(np.float32)
    rounded = np.where(delta >= 0, np.floor(delta + 0.5), -np.floor(-delta + 0.5)).astype(np.uint16)
    out = depth_mm.copy()
    H, W = out.shape
    out[H // 2 - radius:H // 2 + radius, W // 2 - radius:W // 2 + radius] += rounded
    return out


def unproject_points(depth_mm: np.ndarray, K, scale=1000.0):
    """Open3D PointCloud::CreateFromDepthImage at stride 1 (all pixels valid here): row-major camera-space points."""
    H, W = depth_mm.shape
    fx, fy, cx, cy = np.float32(K[0, 0]), np.float32(K[1, 1]), np.float32(K[0, 2]), np.float32(K[1, 2])
    v, u = np.mgrid[0:H, 0:W].astype(np.float32)
    d = (depth_mm.astype(np.float32) / np.float32(scale)).astype(np.float32)
    x = ((u - cx) * d / fx).astype(np.float32)
    y = ((v - cy) * d / fy).astype(np.float32)
    return np.stack([x, y, d], -1).reshape(-1, 3).astype(np.float32)


def reference_nonrigid_kat_inputs():
    from golden import kat_literals as L
    plane = np.full((100, 100), 50, np.uint16)
    color = np.full((100, 100, 3), 100, np.uint8)
    K = simple_intrinsics()
    deformed = hemisphere_pinch(plane, 20, 10.0)
    nodes = L.VBG_NR_NODES
    R = np.tile(np.eye(3, dtype=np.float32), (5, 1, 1))
    t = np.zeros((5, 3), np.float32)
    t[0] = L.VBG_NR_NODE0_TRANSLATION
    return plane, color, K, deformed, nodes, R, t


def rotation_vectors_to_matrices(w):
    """Rodrigues' formula in float64 for [N, 3] rotation vectors -> float32 [N, 3, 3]."""
    w = np.asarray(w, np.float64).reshape(-1, 3)
    th = np.linalg.norm(w, axis=1)
    k = w / np.maximum(th, 1e-30)[:, None]
    Kx = np.zeros((len(w), 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0] = -k[:, 2], k[:, 1], k[:, 2]
    Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 0], -k[:, 1], k[:, 0]
    R = np.eye(3)[None] + np.sin(th)[:, None, None] * Kx + (1 - np.cos(th))[:, None, None] * (Kx @ Kx)
    return R.astype(np.float32)


def extrinsic_about_y(degrees=10.0, translation=(0.03, -0.02, 0.05)):
    """A world-to-camera pose: a rotation about y and a translation (float64 4x4)."""
    a = np.deg2rad(degrees)
    E = np.eye(4)
    E[:3, :3] = [[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]
    E[:3, 3] = translation
    return E


SMALL_H, SMALL_W = 48, 64
SMALL_VOXEL = 0.01          # block side 0.08 m at res 8 (a few dozen blocks), 0.16 m at res 16 (a handful)
SMALL_DEPTH_MAX = 0.9
SMALL_TRUNC_MULT = 3.0
SMALL_COVERAGE = 0.08       # node spacing ~0.08 m: about a dozen nodes within 2 c of a surface voxel (K = 8 can fill)


class SmallScene:
    """What small_tsdf_scene returns: depth [48, 64] (float32 metres, or uint16 millimetres), color [48, 64, 3] (float32
    in [0, 1], or uint8), intrinsics K, depth_scale, depth_max, trunc_mult, voxel_size, camera-space nodes [20, 3] with
    their rotations / translations, coverage, per-pixel normals [H * W, 3]."""


def small_tsdf_scene(O, seed=0, u16=False, rough=False, hole=True, far_strip=True, depth_shift=0.0):
    """A 64 x 48 frame for the TSDF tests: a tilted plane z = 0.5 + 0.15 x + 0.1 y with a spherical bump (radius 0.06 m)
    towards the camera, a rectangular hole of zero depth, a strip beyond depth_max, a 5 x 4 node grid on the smooth
    surface with small random rotations (~3 degrees) and translations (<= 5 mm), normals from the oracle's
    ordered_point_cloud_normals. `rough` adds per-pixel depth noise of +-2 voxels; `depth_shift` moves the whole surface
    along z (another frame of the same scene); `u16` gives millimetre depth with uint8 color."""
    rng = np.random.default_rng(seed)
    H, W = SMALL_H, SMALL_W
    s = SmallScene()
    s.H, s.W = H, W
    s.K = np.array([[80.0, 0.0, 31.5], [0.0, 80.0, 23.5], [0.0, 0.0, 1.0]])
    s.voxel_size, s.depth_max, s.trunc_mult, s.coverage = SMALL_VOXEL, SMALL_DEPTH_MAX, SMALL_TRUNC_MULT, SMALL_COVERAGE

    def surface(u, v):
        x, y = (u - s.K[0, 2]) / s.K[0, 0], (v - s.K[1, 2]) / s.K[1, 1]     # ray (x, y, 1) d
        plane = 0.5 / (1.0 - 0.15 * x - 0.1 * y)
        c = np.array([0.03, -0.02, 0.5 + 0.15 * 0.03 - 0.1 * 0.02])        # sphere centre on the plane
        a = x * x + y * y + 1.0
        b = x * c[0] + y * c[1] + c[2]
        disc = b * b - a * (c @ c - 0.06 ** 2)
        hit = (b - np.sqrt(np.maximum(disc, 0.0))) / a
        return np.where(disc > 0, np.minimum(plane, hit), plane)

    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d = surface(u, v) + depth_shift
    if rough:
        d = d + rng.uniform(-2.0, 2.0, d.shape) * SMALL_VOXEL
    if hole:
        d[30:38, 10:20] = 0.0
    if far_strip:
        d[:, 58:] = 1.2
    nu, nv = np.meshgrid(np.linspace(8.0, 55.0, 5), np.linspace(7.0, 40.0, 4))
    nd = surface(nu.ravel(), nv.ravel())
    s.nodes = np.stack([(nu.ravel() - s.K[0, 2]) / s.K[0, 0] * nd, (nv.ravel() - s.K[1, 2]) / s.K[1, 1] * nd, nd], -1).astype(np.float32)
    s.rotations = rotation_vectors_to_matrices(rng.normal(0.0, 0.03, (20, 3)))
    s.translations = rng.uniform(-0.005, 0.005, (20, 3)).astype(np.float32)
    if u16:
        s.depth = np.round(d * 1000.0).astype(np.uint16)
        s.color = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        s.depth_scale = 1000.0
    else:
        s.depth = d.astype(np.float32)
        s.color = rng.random((H, W, 3)).astype(np.float32)
        s.depth_scale = 1.0
    s.normals = O.ordered_point_cloud_normals(unproject_points(s.depth, s.K, s.depth_scale), H, W)
    return s
