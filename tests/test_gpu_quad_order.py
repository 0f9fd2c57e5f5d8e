"""The fused pixel launch's per-frame quadrant table (k_quad_flags, k_quad_order, k_quad_place; on by default for
launches of one residency round, NNRT_QUAD_ORDER=0 / 1 forces): the table against a numpy restatement at ragged and
minimal image sizes, and the iteration with the table against the iteration without it.

The table only changes which wave runs which 8 x 8 quadrant. Every pixel's float operations are the same, and H and g are
float roundings of fp64 sums of the same float products in another order (see test_gpu_fused_valu.py, which demands
equality with the CPU oracle for the same scenes): the tests demand equality element for element.
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from _util import scene_target  # noqa: E402

MODES = ("ALL", "TRANSLATION_ONLY", "ROTATION_ONLY")
SIZES = {"ragged": (40, 72), "tile": (16, 16), "quadrant": (8, 8)}   # (H, W)
MASKS = ("all", "none", "single", "checker", "left")


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import _native
    _native.lib()
    from dynamicfuion_python_amd import nnrt
    return nnrt


@pytest.fixture(scope="module")
def S():
    from dynamicfuion_python_amd import synthetic
    return synthetic


# ---- the table ------------------------------------------------------------------------------------------------------
def quadrant_ids(H, W):
    """[H, W] quadrant id of every pixel: 16 x 16 tiles in raster order, then the tile's four 8 x 8 quadrants, x fastest"""
    tx = (W + 15) // 16
    v, u = np.mgrid[0:H, 0:W]
    return ((v // 16) * tx + u // 16) * 4 + ((v // 8) & 1) * 2 + ((u // 8) & 1)


def make_mask(kind, H, W):
    m = np.zeros((H, W), np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "single":
        m[H - 3, W - 2] = 1
    elif kind == "checker":   # every other 8 x 8 quadrant of the image, each with another number of valid pixels
        v, u = np.mgrid[0:H, 0:W]
        on = ((v // 8 + u // 8) & 1) == 0
        m[on & ((v % 8) * 8 + u % 8 <= (7 * (v // 8) + 11 * (u // 8)) % 64)] = 1
    elif kind == "left":
        m[:, : W // 2] = 1
    return m


def np_counts(mask):
    H, W = mask.shape
    Q = 4 * ((W + 15) // 16) * ((H + 15) // 16)
    return np.bincount(quadrant_ids(H, W).ravel(), weights=mask.ravel(), minlength=Q).astype(np.int32)


def np_blocks(Q):
    """workgroups of the table launch: 8 bands, each holding ceil(w / 8) + ceil(i / 8) <= ceil(Q / 8) + 1 entries in whole
    four-entry workgroups"""
    return 8 * (((Q + 7) // 8 + 1 + 3) // 4)


def np_bands(counts, slots):
    """per band: (working run, idle run) of the table"""
    Q = len(counts)
    work = [q for q in range(Q) if counts[q]]
    idle = [q for q in range(Q) if not counts[q]]
    bands = []
    for x in range(8):
        w = work[x * len(work) // 8: (x + 1) * len(work) // 8]
        i = idle[x * len(idle) // 8: (x + 1) * len(idle) // 8]
        ov = max(0, len(w) - slots // 8)
        light = sorted(w, key=lambda q: (counts[q], q))[:ov]
        bands.append(([q for q in w if q not in light] + light, i))
    return bands


def gpu_table(nn, mask, slots):
    from dynamicfuion_python_amd import _native as N
    H, W = mask.shape
    Q = 4 * ((W + 15) // 16) * ((H + 15) // 16)
    blocks = N.lib().nnrt_fit_quad_order_blocks(Q)
    counts = np.full(Q, -1, np.int32)
    table = np.full(4 * blocks, -1, np.int32)
    m = np.ascontiguousarray(mask, np.uint8)
    N.check(N.lib().nnrt_fit_quad_order_table(m.ctypes.data_as(ctypes.c_void_p), H, W, slots, counts.ctypes.data_as(ctypes.c_void_p),
                                              table.ctypes.data_as(ctypes.c_void_p)))
    return counts, table, blocks


@pytest.mark.parametrize("slots", [4096, 8])
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("size", list(SIZES))
def test_quad_table(nn, size, kind, slots):
    """72 x 40 (5 x 3 tiles, 60 quadrant slots of which some lie outside the image), one tile and one quadrant; with the
    device's slot count (no overflow) and with 8 slots, one per band, so that every band with two working quadrants
    overflows."""
    H, W = SIZES[size]
    mask = make_mask(kind, H, W)
    counts, table, blocks = gpu_table(nn, mask, slots)
    Q = len(counts)
    ref = np_counts(mask)
    assert np.array_equal(counts, ref), "valid pixels per quadrant"
    assert blocks == np_blocks(Q) and blocks % 8 == 0
    per_band = 4 * blocks // 8
    # every quadrant slot of the tile grid, so every quadrant of the image, exactly once
    assert np.array_equal(np.sort(table[table != Q]), np.arange(Q))
    assert ((table >= 0) & (table <= Q)).all()
    in_image = np.unique(quadrant_ids(H, W))
    assert np.isin(in_image, table).all()
    used = []
    for x, (w, i) in enumerate(np_bands(ref, slots)):
        band = table[x * per_band: (x + 1) * per_band]
        n = int((band != Q).sum())
        assert (band[:n] != Q).all() and (band[n:] == Q).all(), "the sentinel only pads a band's end"
        working = ref[band[:n]] > 0
        nwk = int(working.sum())
        assert working[:nwk].all() and not working[nwk:].any(), "working quadrants first"
        ov = max(0, nwk - slots // 8)
        tail = band[nwk - ov: nwk]
        lightest = sorted(band[:nwk].tolist(), key=lambda q: (ref[q], q))[:ov]
        assert tail.tolist() == lightest, "the overflow is the band's lightest working quadrants, ascending"
        assert (np.diff(band[: nwk - ov]) > 0).all() and (np.diff(band[nwk:n]) > 0).all(), "the rest keeps the id order"
        assert band[:n].tolist() == w + i
        used.append((n + 3) // 4)
    assert max(used) - min(used) <= 1, "band sizes within one workgroup"
    if slots == 8 and kind == "all" and size == "ragged":
        assert any(len(w) > 1 for w, _ in np_bands(ref, slots)), "no band overflows"


# ---- the iteration --------------------------------------------------------------------------------------------------
def ragged_scene(S):
    """the 72 x 40 scene of test_gpu_fused_valu.py: no multiple of 16 either way, the mesh leaves the left columns of
    quadrants empty and crosses the right, top and bottom image edges"""
    H, W, fx = 40, 72, 65.0
    K = np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], np.float64)
    points, normals, faces = S.grid_mesh(37, 29)
    nodes, uv = S.node_grid(6, 4, seed=0)
    d = np.array([0.25, 0.0, 0.0], np.float32)
    w, t = S.ground_truth_motion(uv, seed=0)
    return S.Scene("ragged", H, W, K, points + d, normals, faces, nodes + d, 0.25, 1, 1, S.rodrigues_np(w), t, {}, w)


_SCENES = {}


def scene(S, O, name):
    if name not in _SCENES:
        sc = S.make_scene("S1") if name == "S1" else ragged_scene(S)
        depth = scene_target(O, sc)
        depth.setflags(write=False)
        _SCENES[name] = (sc, depth)
    return _SCENES[name]


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


FIELDS = ("pixel_faces", "residual_mask", "residuals", "hessian", "gradient", "updates")


def iterations(nn, sc, depth, mode, quad, wpe4, count=1, graph=0):
    """diagnostics after each of `count` iterations of a fresh fitter (the selection is read in prepare())"""
    G, A = nn.geometry, nn.alignment
    out = []
    with _env(NNRT_QUAD_ORDER=quad, NNRT_PIX_WPE4=wpe4):
        wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, 1)
        ft = A.DeformableMeshToImageFitter(1, [A.IterationMode[mode]], preconditioning_dampening_factor=0.001, use_hip_graph=graph)
        ft.prepare(wf, G.TriangleMesh(sc.points, sc.normals, sc.faces), np.array(depth), None, sc.K)
        plan = ft.launch_plan()   # the forced choices are the ones the frame runs with
        assert plan["quad_order"] == int(quad) and plan["tile_order"] == 0
        assert wpe4 is None or plan["pix_low_occupancy"] == int(wpe4)
        for _ in range(count):
            ft.iterate(wf, 0, 1)
            dg = ft.diagnostics()
            torch.cuda.synchronize()
            n, s = len(sc.nodes), 6 if mode == "ALL" else 3   # the buffers are sized for 6 x 6 blocks
            cut = {"hessian": n * s * s, "gradient": n * s, "updates": n * s}
            out.append({f: np.array(dg[f][: cut[f]] if f in cut else dg[f]) for f in FIELDS})
    return out


def assert_same(a, b, label):
    assert (a["pixel_faces"] >= 0).any() and a["residual_mask"].any(), f"{label}: nothing rendered"
    for f in FIELDS:
        x, y = np.asarray(a[f]), np.asarray(b[f])
        print(f"{label} {f}: {int((x != y).sum())} of {x.size} differ")
    for f in FIELDS:
        assert np.array_equal(np.asarray(a[f]), np.asarray(b[f]), equal_nan=True), f"{label}: {f} differs"


@pytest.mark.parametrize("wpe4", [None, "1"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["S1", "ragged"])
def test_iteration_same_with_table(nn, S, oracle_mod, name, mode, wpe4):
    """One iteration without (NNRT_QUAD_ORDER=0) and with (=1) the table, in the launch's default build and in its
    4-waves-per-SIMD build with register-resident records (NNRT_PIX_WPE4=1)."""
    sc, depth = scene(S, oracle_mod, name)
    off = iterations(nn, sc, depth, mode, "0", wpe4)[0]
    on = iterations(nn, sc, depth, mode, "1", wpe4)[0]
    assert_same(on, off, f"{name} {mode} wpe4={wpe4}")


@pytest.mark.parametrize("name", ["S1", "ragged"])
def test_graph_replay_same_with_table(nn, S, oracle_mod, name):
    """Two iterations replayed from the captured graph: the second rasterizes into the keys the first one's waves reset,
    the waves of idle quadrants included (sentinel waves have no pixels), and equals the second without the table."""
    sc, depth = scene(S, oracle_mod, name)
    off = iterations(nn, sc, depth, "ALL", "0", None, count=2, graph=2)
    on = iterations(nn, sc, depth, "ALL", "1", None, count=2, graph=2)
    assert not np.array_equal(off[0]["residuals"], off[1]["residuals"], equal_nan=True), "the second iteration is to differ from the first"
    assert_same(on[0], off[0], f"{name} first")
    assert_same(on[1], off[1], f"{name} second")
