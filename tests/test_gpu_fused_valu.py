"""The fused pixel launch (k_fit_pixels_fused) at the shapes where its pass-2 bookkeeping can go wrong, against the CPU
oracle's default reference arithmetic (unfused Jacobian products, products summed in double).

Exactness. Rasterized faces, mask and residuals are bit-identical by construction (same float expression order). H and g
are float roundings of fp64 sums of the same float products; the two sides add them in different orders, so the fp64
sums differ by at most a few 2^-53 relative and the float results are equal unless a sum lies that close to a float
rounding boundary -- the tests demand equality. The block solve is bit-exact given equal H and g
(test_gpu_parity.py::test_block_diagonal_update_bit_exact), so the updates are demanded equal too.

Run lengths. A pixel files each distinct anchor node of its face once, so one wave (8 x 8 pixels) holds at most 64
associations of one node: a run of "more than 64" cannot occur. The longest run, 64, is one whole chunk (NG_CAP) when the
node is the wave's first, and crosses the chunk boundary when another node's run precedes it; both are driven here.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from _util import oracle_fit_scene, scene_target  # noqa: E402

MODES = ("ALL", "TRANSLATION_ONLY", "ROTATION_ONLY")


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


def small_scene(S, name, H, W, fx, mesh, node_grid, coverage, shift=(0.0, 0.0), seed=0):
    """A synthetic.Scene of its own size: the grid mesh and node grid of the synthetic surface, moved by `shift` in x, y
    (so the mesh can cross the image edge and leave quadrants empty), one layer, the usual ground-truth motion."""
    K = np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], np.float64)
    points, normals, faces = S.grid_mesh(*mesh)
    nodes, uv = S.node_grid(*node_grid, seed=seed)
    d = np.array([shift[0], shift[1], 0.0], np.float32)
    w, t = S.ground_truth_motion(uv, seed=seed)
    return S.Scene(name, H, W, K, points + d, normals, faces, nodes + d, coverage, 1, 1, S.rodrigues_np(w), t, {}, w)


# name: (H, W, fx, mesh (cols, rows), node grid (nx, ny), coverage, shift)
SCENES = {
    # 72 x 40: no multiple of 16 either way (4.5 x 2.5 tiles); the mesh leaves the left columns of quadrants empty and
    # crosses the right, top and bottom image edges
    "ragged": (40, 72, 65.0, (37, 29), (6, 4), 0.25, (0.25, 0.0)),
    # node-change batches: a small mesh over a node grid, coarse (few nodes per wave, runs up to 64) and fine (many
    # nodes per wave, runs from 1 up)
    "coarse": (48, 64, 58.0, (33, 25), (3, 2), 0.5, (0.0, 0.0)),
    "fine": (48, 64, 58.0, (33, 25), (14, 10), 0.06, (0.0, 0.0)),
    # one node over the whole mesh: every covered quadrant is a single run of 64, one whole chunk
    "one_node": (32, 32, 40.0, (17, 13), (1, 1), 2.0, (0.0, 0.0)),
    # two nodes, both anchoring every vertex: each wave files node 0's run, then node 1's, which crosses the chunk boundary
    # wherever the quadrant is not full
    "two_nodes": (32, 32, 40.0, (17, 13), (2, 1), 2.0, (0.0, 0.0)),
}


def _scene(S, name):
    if name == "S1":
        return S.make_scene("S1")
    H, W, fx, mesh, grid, cov, shift = SCENES[name]
    return small_scene(S, name, H, W, fx, mesh, grid, cov, shift)


_REFERENCE = {}


def reference(S, O, name, mode="ALL", k=4):
    """(scene, target depth, oracle diagnostics) of one GN iteration from the identity, computed once per case. The
    oracle raises if a block's potrf fails; its outputs are asserted finite."""
    key = (name, mode, k)
    if key not in _REFERENCE:
        O.set_fused_jacobians(False)   # the reference CPU path's own arithmetic
        sc = _scene(S, name)
        depth = scene_target(O, sc)
        _, _, dg = oracle_fit_scene(O, sc, depth, 1, modes=(mode,), anchor_count=k)
        assert dg["status"] == 0
        for f in ("residuals", "hessian_diag", "gradient", "updates"):
            assert np.isfinite(dg[f]).all(), f"oracle {f} not finite for {key}"
        assert dg["residual_mask"].any(), f"no contributing pixel in {key}"
        for f in dg:
            if isinstance(dg[f], np.ndarray):
                dg[f].setflags(write=False)
        _REFERENCE[key] = (sc, depth, dg)
    return _REFERENCE[key]


def gpu_iteration(nn, sc, depth, mode="ALL", k=4, graph=True):
    G, A = nn.geometry, nn.alignment
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, k, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, 1)
    ft = A.DeformableMeshToImageFitter(1, [A.IterationMode[mode]], preconditioning_dampening_factor=0.001, use_hip_graph=2 if graph else 0)
    ft.fit_to_image(wf, G.TriangleMesh(sc.points, sc.normals, sc.faces), None, depth, None, sc.K, None, 1.0)
    dg = ft.diagnostics()
    torch.cuda.synchronize()
    return dg


def run_lengths(O, sc, dg_o, k=4):
    """per (8 x 8 quadrant, node): the number of contributing pixels whose face is anchored to the node -- the run the
    quadrant's wave sums for that node; also per quadrant the run lengths in ascending node order"""
    anchors, _ = O.compute_anchors(sc.points, sc.nodes, k, sc.coverage)
    pf = dg_o["pixel_faces"].astype(np.int64).reshape(sc.H, sc.W)
    on = dg_o["residual_mask"].reshape(sc.H, sc.W) & (pf >= 0)
    per_quadrant = []
    for v0 in range(0, sc.H, 8):
        for u0 in range(0, sc.W, 8):
            counts = {}
            for v in range(v0, min(v0 + 8, sc.H)):
                for u in range(u0, min(u0 + 8, sc.W)):
                    if on[v, u]:
                        for n in set(int(a) for a in anchors[sc.faces[pf[v, u]]].ravel() if a >= 0):
                            counts[n] = counts.get(n, 0) + 1
            per_quadrant.append([counts[n] for n in sorted(counts)])
    return per_quadrant


def compare_exact(dg_o, dg_g, s, N, label):
    pf_o, pf_g = dg_o["pixel_faces"].astype(np.int64), dg_g["pixel_faces"].astype(np.int64)
    res_o, res_g = np.asarray(dg_o["residuals"], np.float32), np.asarray(dg_g["residuals"], np.float32)
    H_o, H_g = np.asarray(dg_o["hessian_diag"], np.float32), np.asarray(dg_g["hessian"][: N * s * s], np.float32)
    g_o, g_g = np.asarray(dg_o["gradient"], np.float32), np.asarray(dg_g["gradient"][: N * s], np.float32)
    x_o, x_g = np.asarray(dg_o["updates"], np.float32), np.asarray(dg_g["updates"][: N * s], np.float32)
    print(f"{label}: faces differing {int((pf_o != pf_g).sum())}, mask differing {int((dg_o['residual_mask'] != dg_g['residual_mask']).sum())}, "
          f"residuals differing {int((res_o != res_g).sum())} (max abs {float(np.abs(res_o - res_g).max()):.3g}), "
          f"H differing {int((H_o != H_g).sum())} of {H_o.size} (max abs {float(np.abs(H_o - H_g).max()):.3g}), "
          f"g differing {int((g_o != g_g).sum())} of {g_o.size} (max abs {float(np.abs(g_o - g_g).max()):.3g}), "
          f"updates differing {int((x_o != x_g).sum())} of {x_o.size} (max abs {float(np.abs(x_o - x_g).max()):.3g})")
    assert np.array_equal(pf_o, pf_g)
    assert np.array_equal(dg_o["residual_mask"], dg_g["residual_mask"])
    assert np.array_equal(res_o, res_g)
    assert np.array_equal(H_o, H_g)
    assert np.array_equal(g_o, g_g)
    assert np.array_equal(x_o, x_g)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["S1", "ragged"])
def test_iteration_exact_at_ragged_image(nn, S, oracle_mod, name, mode):
    """One GN iteration on S1 (128 x 96) and on the 72 x 40 scene, whose image is no multiple of the 16 x 16 tile in
    either dimension, whose mesh crosses the image edge and which has empty 8 x 8 quadrants; every iteration mode."""
    sc, depth, dg_o = reference(S, oracle_mod, name, mode)
    if name == "ragged":
        assert sc.W % 16 and sc.H % 16
        runs = run_lengths(oracle_mod, sc, dg_o)
        assert any(len(r) == 0 for r in runs) and any(len(r) > 0 for r in runs), "the scene needs empty and working quadrants"
        pf = dg_o["pixel_faces"].reshape(sc.H, sc.W)
        assert (pf[:, -1] >= 0).any() and (pf[0] >= 0).any() and (pf[-1] >= 0).any(), "the mesh is to cross the image edge"
    dg_g = gpu_iteration(nn, sc, depth, mode)
    compare_exact(dg_o, dg_g, 6 if mode == "ALL" else 3, len(sc.nodes), f"{name} {mode}")


# run lengths each graph has to produce (together: 1, 2, 7, 8, 9 and the longest possible, 64)
NEEDED_RUNS = {"coarse": {64}, "fine": {1, 2, 7, 8, 9}}


@pytest.mark.parametrize("name,k", [("coarse", 4), ("fine", 4), ("fine", 8)])
def test_node_change_batches_exact(nn, S, oracle_mod, name, k):
    """The slot-serial path of the sums: batches of 8 slots in which the node changes. The two graphs together give,
    within single waves, runs of 1, 2, 7, 8, 9 and 64 associations per node (checked on the oracle's association
    counts). H and g equal the oracle's, and the fitter replayed from a captured graph equals the eager one. K = 8 runs
    the MAX_ANCHORS instantiation, which shares the sums' code and its compiler flags (the coarse graph has 6 nodes, too
    few for 8 anchors)."""
    sc, depth, dg_o = reference(S, oracle_mod, name, k=k)
    runs = run_lengths(oracle_mod, sc, dg_o, k)
    seen = set(n for r in runs for n in r)
    print(f"{name} K={k}: run lengths seen {sorted(seen)}; nodes per wave up to {max(len(r) for r in runs)}")
    assert NEEDED_RUNS[name] <= seen
    assert any(len(r) > 1 and any(n % 8 for n in r[:-1]) for r in runs), "no node change inside a batch"
    N = len(sc.nodes)
    dg_g = gpu_iteration(nn, sc, depth, k=k, graph=True)
    compare_exact(dg_o, dg_g, 6, N, f"{name} K={k}")
    dg_e = gpu_iteration(nn, sc, depth, k=k, graph=False)
    for f in ("hessian", "gradient", "updates", "residuals", "pixel_faces", "residual_mask"):
        assert np.array_equal(np.asarray(dg_g[f]), np.asarray(dg_e[f]), equal_nan=True), f"graph and eager {f} differ"


@pytest.mark.parametrize("name,k", [("one_node", 1), ("two_nodes", 2)])
def test_longest_run_exact(nn, S, oracle_mod, name, k):
    """Runs of 64, the most one wave can hold of one node. one_node: a single-node graph, every full quadrant one run that
    is one whole chunk. two_nodes: node 1's run follows node 0's in every wave, so in a quadrant with r < 64 contributing
    pixels it starts at slot r and in a full one it fills the second chunk after node 0 filled the first; partly covered
    quadrants make it continue across the chunk boundary (r + r > 64). One flush per (wave, node) cannot be observed
    from outside; a second flush of a continued run would still add the same two partial sums, so this checks the
    sums, not the flush count. The warp field takes no more anchors than it has nodes, so these graphs run with K = 1
    and K = 2 (the 4-slot instantiation with empty slots)."""
    sc, depth, dg_o = reference(S, oracle_mod, name, k=k)
    runs = run_lengths(oracle_mod, sc, dg_o, k)
    assert any(r and r[0] == 64 for r in runs), "no full quadrant"
    if name == "two_nodes":
        assert all(len(r) in (0, 2) for r in runs)
        assert any(len(r) == 2 and 32 < r[0] < 64 for r in runs), "no run crossing the chunk boundary"
    dg_g = gpu_iteration(nn, sc, depth, k=k)
    compare_exact(dg_o, dg_g, 6, len(sc.nodes), name)
