"""Device memory ownership of the native library (csrc/device_memory.hpp): every handle returns the device memory it
took. nnrt_device_bytes_in_use() counts the bytes held through the library's two owning types (DeviceBuffer,
StreamScratch) process-wide; each case reads it before its handles exist and requires the same value after they are
destroyed. torch's own allocator does not enter the count.

Shapes are the smallest that allocate every buffer: 64 nodes, a 21 x 15 grid mesh (315 vertices, 560 triangles), a
32 x 48 image (six 16 x 16 tiles, two tile rows)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _rigid_align_util as RU  # noqa: E402
from dynamicfuion_python_amd import synthetic as S  # noqa: E402

H, W, FX = 32, 48, 42.0
NODES_X = NODES_Y = 8
COVERAGE = 0.18


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import _native as N
    from dynamicfuion_python_amd.nnrt import alignment as A
    from dynamicfuion_python_amd.nnrt import geometry as G
    from dynamicfuion_python_amd.nnrt import graph_proc as GP
    from dynamicfuion_python_amd.nnrt import voxel_grid as VG

    class Modules:
        pass
    m = Modules()
    m.N, m.A, m.G, m.GP, m.VG = N, A, G, GP, VG
    return m


def in_use(M) -> int:
    return int(M.N.lib().nnrt_device_bytes_in_use())


def destroy(handle_owner):
    """Destroy the native handle now (the wrappers destroy in __del__, which clears the handle: idempotent)."""
    handle_owner.__del__()


def frame(cols, rows, h, w, fx):
    """(mesh, depth [h, w], K): the synthetic surface seen by a pinhole camera, and the surface itself 5 mm nearer."""
    p, n, f = S.grid_mesh(cols, rows)
    K = np.array([[fx, 0, w / 2], [0, fx, h / 2], [0, 0, 1]], np.float64)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = (u - K[0, 2]) * 1.2 / fx, (v - K[1, 2]) * 1.2 / fx
    depth = (S.surface_z(x, y) - 0.005).astype(np.float32)
    return (p, n, f), depth, K


def warp_field(M, layer_count):
    nodes, _ = S.node_grid(NODES_X, NODES_Y)
    return M.G.HierarchicalGraphWarpField(nodes, COVERAGE, False, 4, 0, M.G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, layer_count)


def fitter(M, **kw):
    return M.A.DeformableMeshToImageFitter(2, [M.A.IterationMode.ALL], preconditioning_dampening_factor=0.001,
                                           use_hip_graph=M.A.GRAPH_ALWAYS, **kw)


def fit_sequence(M, ft, wf, frames, from_snapshot=None):
    """prepare (each frame in turn), two iterations, snapshot, one iteration from the snapshot; then the last frame is
    prepared a second time, which must keep every buffer pointer: the captured graph survives it. Returns the number
    of captured graphs. from_snapshot: the call that iterates from the snapshot (step control refuses the default)."""
    if from_snapshot is None:
        from_snapshot = lambda: ft.iterate_from_snapshot(wf, 0, 1)   # noqa: E731
    for mesh, depth, K in frames:
        ft.prepare(wf, M.G.TriangleMesh(*mesh), depth, None, K, None, 1.0)
    ft.iterate(wf, 0, 2)
    ft.snapshot_motion(wf)            # the first snapshot allocates its buffer and drops the graphs
    from_snapshot()
    graphs = ft.graph_count
    assert graphs >= 1                # use_hip_graph always: the sequence was captured
    mesh, depth, K = frames[-1]
    ft.prepare(wf, M.G.TriangleMesh(*mesh), depth, None, K, None, 1.0)
    assert ft.graph_count == graphs   # ensure(n <= count) kept every pointer, so no graph was dropped
    ft.snapshot_motion(wf)
    from_snapshot()
    assert ft.graph_count == graphs   # and the kept graph is the one replayed
    ft.check()
    torch.cuda.synchronize()
    return graphs


def test_fitter_with_arap_returns_its_memory(M):
    """Two layers: E > 0, so the corner solver and the arrowhead buffers exist. The parent of the owning types leaked
    the snapshot buffer ([N,16] floats) here."""
    base = in_use(M)
    wf = warp_field(M, 2)
    assert M.N.lib().nnrt_warp_field_edge_count(wf.handle) > 0
    ft = fitter(M)
    held = in_use(M)
    assert held > base
    fit_sequence(M, ft, wf, [frame(21, 15, H, W, FX)])
    assert in_use(M) > held + 64 * 16 * 4   # the frame's buffers and the snapshot are counted
    destroy(ft)
    destroy(wf)
    assert in_use(M) == base


def test_single_layer_fitter_returns_its_memory_after_growing(M):
    """One layer: E == 0. A smaller frame first, then the full one, so that ensure() reallocates."""
    base = in_use(M)
    wf = warp_field(M, 1)
    assert M.N.lib().nnrt_warp_field_edge_count(wf.handle) == 0
    ft = fitter(M)
    small = frame(11, 9, 16, 32, 28.0)
    ft.prepare(wf, M.G.TriangleMesh(*small[0]), small[1], None, small[2], None, 1.0)
    after_small = in_use(M)
    fit_sequence(M, ft, wf, [small, frame(21, 15, H, W, FX)])
    assert in_use(M) > after_small     # the larger frame took larger buffers
    destroy(ft)
    destroy(wf)
    assert in_use(M) == base


@pytest.mark.parametrize("layer_count", [2, 1], ids=["two_layers", "one_layer"])
def test_coupled_fitter_keeps_its_graphs_and_returns_its_memory(M, layer_count):
    """NNRT_DATA_COUPLED: the pair structure, the solver plan over it and the pair blocks exist; with one layer E == 0,
    so the prepare launch reads the zero incidence offsets and the solve's vectors are the coupled mode's own. The
    repeated prepare() rebuilds the pair structure on the device; it finds the same pairs, so the uploads keep their
    pointers and the plan its generation, and the graph is kept. The graph count (1 after the repeated prepare(), in
    both cases) was taken from the parent of the refactor that gave prepare() its steps, by running this test against
    that library."""
    base = in_use(M)
    wf = warp_field(M, layer_count)
    assert (M.N.lib().nnrt_warp_field_edge_count(wf.handle) > 0) == (layer_count == 2)
    ft = fitter(M)
    ft.set_data_coupling(M.A.DataCoupling.COUPLED)
    held = in_use(M)
    assert fit_sequence(M, ft, wf, [frame(21, 15, H, W, FX)]) == 1
    assert ft.coupled_pair_count > 0
    assert in_use(M) > held + 36 * 8 * ft.coupled_pair_count   # pair_acc (fp64) alone
    destroy(ft)
    destroy(wf)
    assert in_use(M) == base


@pytest.mark.parametrize("robust", [False, True], ids=["square_one_layer", "robust_irls_two_layers"])
def test_step_control_fitter_keeps_its_graphs_and_returns_its_memory(M, robust):
    """Step control on: its state, history, best motion and partial sums exist; under the robust objective (IRLS Tukey
    and Huber penalties, two layers) the raw residuals too. Iterations that restart from the snapshot every time are
    refused in this mode, so the sequence fits from the snapshot instead. The graph count (1) was taken from the parent
    of the refactor that gave prepare() its steps, by running this test against that library."""
    A = M.A
    base = in_use(M)
    wf = warp_field(M, 2 if robust else 1)
    ft = fitter(M, use_tukey_penalty_for_data_term=True, use_huber_penalty_for_arap_term=True, penalty_form=A.PenaltyForm.IRLS,
                step_objective=A.StepObjective.ROBUST) if robust else fitter(M)
    without = in_use(M)
    ft.set_step_control(A.StepControl())
    assert fit_sequence(M, ft, wf, [frame(21, 15, H, W, FX)], from_snapshot=lambda: ft.fit_from_snapshot(wf, 1)) == 1
    assert len(ft.step_history()) == 1
    if robust:
        assert ft.raw_residuals().shape == (H * W,)
    assert in_use(M) > without + 64 * 16 * 4
    destroy(ft)
    destroy(wf)
    assert in_use(M) == base


def test_layer_switch_on_one_fitter_drops_graphs_and_returns_memory(M):
    """Two layers, one layer, two layers again with the same node count on one fitter: each switch changes the frame's
    key (the warp field, E, n0), so the graphs are dropped at each; the arrowhead structure of the first frame is kept
    across the one-layer frame and found unchanged by the third."""
    base = in_use(M)
    wf2, wf1 = warp_field(M, 2), warp_field(M, 1)
    ft = fitter(M)
    mesh, depth, K = frame(21, 15, H, W, FX)

    def fit(wf):
        ft.prepare(wf, M.G.TriangleMesh(*mesh), depth, None, K, None, 1.0)
        dropped = ft.graph_count == 0
        ft.iterate(wf, 0, 2)
        ft.check()
        return dropped, ft.graph_count

    assert fit(wf2) == (True, 1)
    corner = ft.corner_info()
    with_arap = in_use(M)
    assert fit(wf1) == (True, 1)
    assert in_use(M) == with_arap            # nothing of the two-layer frame was released, nothing new was needed
    assert fit(wf2) == (True, 1)
    assert ft.corner_info() == corner and in_use(M) == with_arap
    assert fit(wf2) == (False, 1)            # the same frame again keeps the graph
    torch.cuda.synchronize()
    destroy(ft)
    destroy(wf1)
    destroy(wf2)
    assert in_use(M) == base


def test_failing_warp_field_create_returns_its_memory(M):
    """A create that fails after its argument checks, with device work behind it: a decimation radius too small to
    thin the node set (the hierarchy builder refuses a coarser layer as large as the finer one)."""
    base = in_use(M)
    nodes, _ = S.node_grid(NODES_X, NODES_Y)
    with pytest.raises(M.N.NnrtError, match="coarser layer"):
        M.G.HierarchicalGraphWarpField(nodes, COVERAGE, False, 4, 0, M.G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, 2,
                                       layer_decimation_radii=[COVERAGE, 1e-3])   # nodes stand 0.13 apart
    assert in_use(M) == base


def test_stand_alone_entry_points_return_their_temporaries(M):
    """Entry points that work in stream-ordered temporaries: after the stream is synchronised nothing is held."""
    N, G = M.N, M.G
    base = in_use(M)
    dev = torch.device("cuda", N.current_device())
    (p, n, f), _, _ = frame(21, 15, H, W, FX)
    nodes, uv = S.node_grid(NODES_X, NODES_Y)
    w, t = S.ground_truth_motion(uv)
    R = S.rodrigues_np(w)
    V, K = len(p), 4
    d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)   # noqa: E731
    dp, dn, dg, dR, dt_ = d(p, torch.float32), d(n, torch.float32), d(nodes, torch.float32), d(R, torch.float32), d(t, torch.float32)
    anchors = torch.empty((V, K), dtype=torch.int32, device=dev)
    weights = torch.empty((V, K), dtype=torch.float32, device=dev)
    N.check(N.lib().nnrt_compute_anchors_and_weights(N.ptr(dp), V, N.ptr(dg), len(nodes), K, COVERAGE, None, 0, N.ptr(anchors), N.ptr(weights),
                                                     N.stream_ptr()))
    out_p, out_n = torch.empty_like(dp), torch.empty_like(dn)
    N.check(N.lib().nnrt_warp_mesh(N.ptr(dp), N.ptr(dn), V, N.ptr(dg), N.ptr(dR), N.ptr(dt_), len(nodes), N.ptr(anchors), N.ptr(weights), K,
                                   None, N.ptr(out_p), N.ptr(out_n), N.stream_ptr()))
    mesh = G.TriangleMesh(p, n, f)
    warped = G.warp_triangle_mesh(mesh, nodes, R, t, 4, COVERAGE)          # nnrt_warp_points, online anchors
    cloud = G.warp_point_cloud(G.PointCloud(p), nodes, R, t, anchors, weights, 0)   # nnrt_warp_points, supplied anchors
    eroded = M.GP.get_vertex_erosion_mask(p, f, 2, 4)
    normals = G.compute_vertex_normals(mesh)
    Kc, tp, tn, mp, mn = RU.scene(H, W, 21, 15)
    aligned = M.A.align_rigid_point_to_plane(mp, mn, tp, Kc, iteration_counts=(2, 1), minimum_correspondence_count=10)
    torch.cuda.synchronize()
    assert in_use(M) == base
    # the calls did their work (the count is not at baseline because nothing ran)
    assert torch.isfinite(out_p).all() and torch.isfinite(warped.vertex_positions).all() and torch.isfinite(cloud.point_positions).all()
    assert (out_p - dp).abs().max() > 1e-4
    assert eroded.shape[0] == V and normals.shape == (V, 3) and aligned.log.shape == (3, 2)


def test_voxel_grid_returns_its_memory_after_growing(M):
    base = in_use(M)
    vg = M.VG.VoxelBlockGrid(("tsdf", "weight"), (np.float32, np.float32), (1, 1), voxel_size=0.01, block_resolution=8, block_count=4)
    held = in_use(M)
    assert held > base
    depth = np.full((H, W), 500, np.uint16)
    depth[8:24, 12:36] = 480
    Kd = np.array([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1]])
    blocks = vg.compute_unique_block_coordinates(depth, Kd, np.eye(4), 1000.0, 3.0)
    assert blocks.shape[0] > 4                      # more blocks than the grid was created with: it has to grow
    vg.integrate(blocks, depth, Kd, np.eye(4), 1000.0, 3.0)
    active, capacity, _, _ = vg._info()
    assert active >= blocks.shape[0] and capacity > 4
    mesh = vg.extract_triangle_mesh(weight_threshold=0.5)
    assert mesh.vertex_positions.shape[0] > 0
    torch.cuda.synchronize()
    assert in_use(M) > held
    destroy(vg)
    assert in_use(M) == base
