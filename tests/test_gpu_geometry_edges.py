"""csrc/geometry.hip's anchor search and mesh warp against the CPU oracle, bit for bit, at the batch, slot and tail
edges the scenes of tests/test_gpu_parity.py do not reach. Both sides form every float in the same order (the existing
anchor and warp tests' premise), so every comparison is of bits. tests/test_geometry_edges_cpu.py holds the oracle
against float64 on the same inputs (tests/_geometry_edge_util.py).

k_compute_anchors<K>: nodes in batches of 64, one batch ahead (N = 64: no prefetch; N = 128, 192: prefetch, no tail;
N < 64: tail only), groups of 8 skipped when no lane can use them, a scalar tail of N % 64 nodes, empty slots when N < K.
launch_warp_mesh: k_warp_mesh_quad (K <= 4), k_warp_mesh_vertex<., VEC4> (NNRT_WARP_VERTEX=1; VEC4 needs K = 4 and
16-byte-aligned anchors and weights), k_warp_mesh (K > 4). Every case has V <= 1100 and N <= 192."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _geometry_edge_util as U  # noqa: E402
from _util import scene_target  # noqa: E402


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import _native
    _native.lib()
    from dynamicfuion_python_amd import nnrt
    return nnrt


@pytest.fixture(scope="module")
def native(nn):
    from dynamicfuion_python_amd import _native
    return _native


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def same_bits(a, b):
    a, b = np.ascontiguousarray(_np(a)), np.ascontiguousarray(_np(b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def gpu_anchors(nn, points, nodes, K, minimum_valid=0, coverage=0.0, node_weights=None):
    f = nn.geometry.functional
    if node_weights is None:
        a, w = f.compute_anchors_and_weights_euclidean_fixed_node_weight(points, nodes, K, minimum_valid, coverage)
    else:
        a, w = f.compute_anchors_and_weights_euclidean_variable_node_weight(points, nodes, node_weights, K, minimum_valid)
    return _np(a), _np(w)


def check_anchors(nn, O, points, nodes, K, minimum_valid=0, coverage=0.0, node_weights=None, note=()):
    """The kernel's anchors and weights equal the oracle's, bit for bit; returns the oracle's."""
    a_o, w_o = O.compute_anchors(points, nodes, K, coverage, node_weights=node_weights, minimum_valid_anchor_count=minimum_valid)
    a_g, w_g = gpu_anchors(nn, points, nodes, K, minimum_valid, coverage, node_weights)
    what = (len(nodes), len(points), K, minimum_valid, "variable" if node_weights is not None else coverage) + tuple(note)
    assert same_bits(a_o, a_g), ("anchors", what, np.argwhere(a_o != a_g)[:4].tolist())
    assert same_bits(w_o, w_g), ("weights", what, np.argwhere(w_o.view(np.uint32) != w_g.view(np.uint32))[:4].tolist())
    return a_o, w_o


# ---------------------------------------------------------------------------------------------------------------------
# anchors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", U.BATCH_N)
def test_anchor_batch_boundaries(nn, oracle_mod, N):
    """All eight instantiations k_compute_anchors<1..8> at every batch edge: N = 1, 7, 8, 9, 63 tail only (N < K leaves
    slots empty at 1 and 7); 64 one batch, no prefetch, no tail; 65, 127 one batch and a tail; 128, 192 the prefetch
    guard true then false, no tail; 129 two batches and a one-node tail. V = 65: a full wave and a wave of one lane."""
    points, nodes = U.anchor_case(N, U.BATCH_V, 0, "uniform")
    for K in U.ALL_K:
        a, _ = check_anchors(nn, oracle_mod, points, nodes, K, coverage=U.COVERAGE["uniform"])
        assert np.array_equal(U.valid_counts(a), np.full(U.BATCH_V, min(N, K)))


@pytest.mark.parametrize("N", U.TAIL_N)
@pytest.mark.parametrize("V", U.TAIL_V)
def test_anchor_wave_tail(nn, oracle_mod, V, N):
    """Inactive lanes in the last wave (V = 1, 63, 65, 130), none (64): they take part in every readlane broadcast and
    __any vote, never insert and never store."""
    points, nodes = U.anchor_case(N, V, 0, "uniform")
    check_anchors(nn, oracle_mod, points, nodes, 4, coverage=U.COVERAGE["uniform"])


@pytest.mark.parametrize("layout", U.SKIP_LAYOUTS)
@pytest.mark.parametrize("N", U.SKIP_N)
def test_anchor_group_skipping(nn, oracle_mod, layout, N):
    """Nodes in ascending distance from a tight cloud of points: after the first groups no lane has a distance below its
    maximum and the __any test skips the group; descending: every group inserts, in node order."""
    points, nodes = U.anchor_case(N, U.BATCH_V, 0, layout)
    for K in U.SKIP_K:
        check_anchors(nn, oracle_mod, points, nodes, K, coverage=U.COVERAGE[layout], note=(layout,))


@pytest.mark.parametrize("layout", U.TIE_LAYOUTS)
@pytest.mark.parametrize("N", U.TIE_N)
def test_anchor_exact_ties(nn, oracle_mod, layout, N):
    """Exactly equal squared distances (integer lattice; every node twice): replace-the-current-maximum with a strict
    `<` keeps the earlier node and fills the slots in one order only."""
    points, nodes = U.anchor_case(N, U.BATCH_V, 0, layout)
    for K in U.TIE_K:
        check_anchors(nn, oracle_mod, points, nodes, K, coverage=U.COVERAGE[layout], note=(layout,))


@pytest.mark.parametrize("N", U.FEW_N)
@pytest.mark.parametrize("K", U.FEW_K)
def test_anchor_fewer_nodes_than_slots(nn, oracle_mod, K, N):
    """N < K (and N = 0): empty slots are index -1 at squared distance inf and node_weights is not read for them.
    Unthresholded (weight 0, or 1 / K without any node), thresholded with minimum_valid 1 and K (the empty slots keep
    inf; below the minimum the row stays unnormalised), each with the fixed coverage and with per-node weights."""
    points, nodes = U.anchor_case(N, U.BATCH_V, 0, "uniform")
    coverage = 0.6   # 2 c = 1.2: some of the few nodes pass the distance test, some fail it
    node_weights = np.full(N, np.float32(0.36))
    for nw in (None, node_weights):
        c = coverage if nw is None else 0.0
        a, w = check_anchors(nn, oracle_mod, points, nodes, K, 0, c, nw)
        assert np.array_equal(U.valid_counts(a), np.full(U.BATCH_V, N))
        assert same_bits(w[:, N:], np.full((U.BATCH_V, K - N), np.float32(0 if N else 1) / np.float32(1 if N else K)))
        for minimum_valid in (1, K):
            a, w = check_anchors(nn, oracle_mod, points, nodes, K, minimum_valid, c, nw)
            assert (a[:, N:] == -1).all() and np.isposinf(w[:, N:]).all()
            if N == 3:
                assert (a[:, :N] >= 0).any() and (a[:, :N] == -1).any()


@pytest.mark.parametrize("K", sorted(U.THRESHOLD_COVERAGE))
def test_anchor_threshold_branches(nn, oracle_mod, K):
    """The thresholded search at K = 2, 5, 8: the weight array holds squared distances first, a slot beyond 2 c becomes
    -1 and keeps its squared distance, rows with fewer valid slots than minimum_valid stay unnormalised. The coverage is
    small enough that some points keep no slot, some 1..K-1 and some all K (asserted on the oracle's output)."""
    points, nodes = U.anchor_case(U.THRESHOLD_N, U.THRESHOLD_V, 0, "uniform")
    coverage = U.THRESHOLD_COVERAGE[K]
    for node_weights in (None, oracle_mod.node_coverage_weights(nodes, coverage)):
        c = coverage if node_weights is None else 0.0
        for minimum_valid in sorted({1, 2, K}):
            a, w = check_anchors(nn, oracle_mod, points, nodes, K, minimum_valid, c, node_weights)
            n = U.valid_counts(a)
            assert (n == 0).any() and ((n > 0) & (n < K)).any() and (n == K).any()
            below = n < minimum_valid
            assert below.any() and (~below).any()
            sums = np.where(a >= 0, w, 0).sum(axis=1, dtype=np.float64)
            assert np.abs(sums[~below] - 1).max() < 1e-6       # normalised rows
            assert (w[a < 0] > 0).all()                         # rejected slots: their squared distance, not a weight


def test_anchor_non_finite_points(nn, oracle_mod):
    """A NaN point and a +inf point among ordinary ones in one wave: no distance of theirs compares below inf, so all
    their slots stay -1 (weights 1 / K); their lanes still vote in __any and their neighbours' rows do not change."""
    points, nodes, bad = U.non_finite_cloud()
    a, w = check_anchors(nn, oracle_mod, points, nodes, 4, coverage=U.COVERAGE["uniform"])
    clean, _ = U.anchor_case(129, 65, 0, "uniform")
    a_c, w_c = gpu_anchors(nn, clean, nodes, 4, 0, U.COVERAGE["uniform"])
    keep = np.ones(len(points), bool)
    keep[list(bad)] = False
    assert same_bits(a[keep], a_c[keep]) and same_bits(w[keep], w_c[keep])
    assert (a[~keep] == -1).all() and same_bits(w[~keep], np.full((2, 4), np.float32(0.25)))
    a, w = check_anchors(nn, oracle_mod, points, nodes, 4, 2, 0.2)   # thresholded: -1 and inf, unnormalised
    assert (a[~keep] == -1).all() and np.isposinf(w[~keep]).all()


def test_anchor_input_views(nn, oracle_mod, native):
    """points and nodes as device tensors 4 bytes into a larger buffer (no 16-byte alignment) give the bits of fresh tensors."""
    dev = torch.device("cuda", native.current_device())
    points, nodes = U.anchor_case(129, 65, 0, "uniform")

    def shifted(x):
        buffer = torch.zeros(x.size + 5, dtype=torch.float32, device=dev)
        view = buffer[1:1 + x.size].view(*x.shape)
        view.copy_(torch.as_tensor(x, device=dev))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    for K in (1, 4, 8):
        a_o, w_o = oracle_mod.compute_anchors(points, nodes, K, 0.3)
        a_g, w_g = gpu_anchors(nn, shifted(points), shifted(nodes), K, 0, 0.3)
        assert same_bits(a_o, a_g) and same_bits(w_o, w_g)


# ---------------------------------------------------------------------------------------------------------------------
# warp (the public C entry nnrt_warp_mesh with caller-supplied anchors)
# ---------------------------------------------------------------------------------------------------------------------
class WarpInputs:
    """One warp case on the device; anchors and weights are placed `shift` bytes past a 16-byte boundary."""

    def __init__(self, native, case, shift=0):
        self.N = native
        dev = torch.device("cuda", native.current_device())
        p, n, g, R, t, a, w = case
        self.V, self.K, self.node_count = len(p), a.shape[1], len(g)
        d = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=dev)   # noqa: E731
        self.p, self.n, self.g, self.R, self.t = (d(x, torch.float32) for x in (p, n, g, R, t))
        assert shift % 4 == 0 and 0 <= shift < 16

        def place(x, dt):
            buffer = torch.zeros(x.size + 8, dtype=dt, device=dev)
            view = buffer[shift // 4: shift // 4 + x.size].view(*x.shape)
            view.copy_(d(x, dt))
            assert view.data_ptr() % 16 == shift
            return view

        self.a, self.w = place(a, torch.int32), place(w, torch.float32)
        assert int(self.a.min()) >= -1 and int(self.a.max()) <= self.node_count - 1   # the C entry does not validate anchors

    def run(self, extrinsics=None):
        N = self.N
        out_p = torch.full((self.V, 3), float("nan"), dtype=torch.float32, device=self.p.device)
        out_n = torch.full_like(out_p, float("nan"))
        E = None if extrinsics is None else np.ascontiguousarray(extrinsics, np.float64)
        N.check(N.lib().nnrt_warp_mesh(N.ptr(self.p), N.ptr(self.n), self.V, N.ptr(self.g), N.ptr(self.R), N.ptr(self.t), self.node_count,
                                       N.ptr(self.a), N.ptr(self.w), self.K, N.ptr(E), N.ptr(out_p), N.ptr(out_n), N.stream_ptr()))
        torch.cuda.synchronize()
        return _np(out_p), _np(out_n)


def _check_warp(got, ref, what):
    assert same_bits(got[0], ref[0]), ("positions",) + what + (np.argwhere(got[0] != ref[0])[:4].tolist(),)
    assert same_bits(got[1], ref[1]), ("normals",) + what + (np.argwhere(got[1] != ref[1])[:4].tolist(),)


@pytest.mark.parametrize("V", U.WARP_V)
def test_warp_dispatch_matrix(nn, native, oracle_mod, monkeypatch, V):
    """nnrt_warp_mesh against oracle.warp_mesh on the same anchors and weights. K = 1..4: k_warp_mesh_quad
    (NNRT_WARP_VERTEX=0; clamped loads for k >= K at K < 4) and k_warp_mesh_vertex (=1; without VEC4 at K < 4, with it at
    K = 4, the tensors being 16-byte aligned); K = 5, 6, 8: k_warp_mesh, where the switch changes nothing. With every slot
    valid and with 30 % of them -1 (a == -1 skips; an all-invalid row is exactly zero; invalid slots' weights are inf or
    7.5 and must not reach a sum), identity and rigid extrinsics. V = 1, 63, 65, 257, 1025: partial waves and workgroups.
    Quad and vertex kernels agree with each other as with the oracle."""
    for K in U.WARP_QUAD_K + U.WARP_WIDE_K:
        for share in U.WARP_INVALID:
            case = U.warp_case(V, U.WARP_N, K, 0, share)
            inputs = WarpInputs(native, case)
            empty = (case[5] < 0).all(axis=1)
            assert empty.any() == (share > 0)
            for E in (None, U.warp_extrinsics()):
                ref = oracle_mod.warp_mesh(*case, E)
                got = {}
                for switch in ("0", "1"):
                    monkeypatch.setenv("NNRT_WARP_VERTEX", switch)
                    got[switch] = inputs.run(E)
                    _check_warp(got[switch], ref, (V, K, share, E is not None, switch))
                    assert not got[switch][0][empty].any() and not got[switch][1][empty].any()
                _check_warp(got["0"], got["1"], (V, K, share, E is not None, "quad / wide against vertex"))


@pytest.mark.parametrize("V", (65, 1025))
def test_warp_vec4_selection(nn, native, oracle_mod, monkeypatch, V):
    """K = 4 under NNRT_WARP_VERTEX=1: anchors and weights 4 and 8 bytes past a 16-byte boundary take
    k_warp_mesh_vertex<., false>, 16-byte-aligned ones <., true>; all three give the quad kernel's and the oracle's bits."""
    for share in U.WARP_INVALID:
        case = U.warp_case(V, U.WARP_N, 4, 1, share)
        for E in (None, U.warp_extrinsics()):
            ref = oracle_mod.warp_mesh(*case, E)
            monkeypatch.setenv("NNRT_WARP_VERTEX", "0")
            quad = WarpInputs(native, case).run(E)
            _check_warp(quad, ref, (V, share, E is not None, "quad"))
            monkeypatch.setenv("NNRT_WARP_VERTEX", "1")
            for shift in (0, 4, 8):
                got = WarpInputs(native, case, shift).run(E)
                _check_warp(got, ref, (V, share, E is not None, "vertex", shift))
                _check_warp(got, quad, (V, share, E is not None, "vertex against quad", shift))


def test_warp_default_dispatch(nn, native, oracle_mod, monkeypatch):
    """Without the switch a mesh below 65536 vertices takes the quad kernel (K <= 4) or k_warp_mesh (K > 4)."""
    monkeypatch.delenv("NNRT_WARP_VERTEX", raising=False)
    for K in (3, 4, 7):
        case = U.warp_case(257, U.WARP_N, K, 2, 0.3)
        _check_warp(WarpInputs(native, case).run(), oracle_mod.warp_mesh(*case), (K, "default"))


# ---------------------------------------------------------------------------------------------------------------------
# the fitter's warp with empty anchor slots
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vertex_path,anchors16", [("0", "1"), ("1", "1"), ("1", "0")])
def test_fitter_warp_with_empty_slots(nn, oracle_mod, monkeypatch, vertex_path, anchors16):
    """S1's mesh under a field that thresholds by distance (coverage 0.12, at least two valid anchors): every vertex
    keeps one to four slots, so the fitter's anchors hold -1 in one, two and three slots of a row and some rows stay
    unnormalised. One iteration from the ground-truth motion; the warped mesh the fitter rasterized equals oracle.warp_mesh
    on the fitter's own anchors: by the quad kernel, by the vertex kernel reading the 16-bit anchor copy (-1 <-> 0xFFFF)
    and by the vertex kernel reading the int32 anchors."""
    from dynamicfuion_python_amd import synthetic as S
    monkeypatch.setenv("NNRT_WARP_VERTEX", vertex_path)
    monkeypatch.setenv("NNRT_ANCHORS16", anchors16)
    G, A = nn.geometry, nn.alignment
    sc = S.make_scene("S1")
    depth = scene_target(oracle_mod, sc)
    V = len(sc.points)
    wf = G.HierarchicalGraphWarpField(sc.nodes, 0.12, True, 4, 2, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, 1)
    ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001)
    ft.prepare(wf, G.TriangleMesh(sc.points, sc.normals, sc.faces), depth, None, sc.K)
    a, w = ft.anchors(V, 4)
    empty = 4 - U.valid_counts(a)
    assert (a == -1).any() and set(np.unique(empty)) == {0, 1, 2, 3}
    a_o, w_o = oracle_mod.compute_anchors(sc.points, wf.get_node_positions(True), 4, 0.12, minimum_valid_anchor_count=2)
    assert same_bits(a, a_o) and same_bits(w, w_o)
    wf.set_node_rotations(sc.gt_rotations)
    wf.set_node_translations(sc.gt_translations)
    R0, t0 = wf.get_node_rotations(True), wf.get_node_translations(True)
    ft.iterate(wf, 0, 1)
    p_g, n_g = ft.warped_mesh(V)
    p_o, n_o = oracle_mod.warp_mesh(sc.points, sc.normals, wf.get_node_positions(True), R0, t0, a, w)
    _check_warp((p_g, n_g), (p_o, n_o), (vertex_path, anchors16))
