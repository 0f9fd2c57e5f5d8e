"""SolveBlockSparseArrowheadCholesky on irregular structures: the device paths of the stem kernels (csrc/arap.hip) and
the tile-sparse corner (csrc/corner.hip) that the 2-D grids of test_gpu_arrowhead.py never reach -- stem degrees other
than 4, Schur pair lists at the edges of the 8-pair and 64-pair chunks, a corner node with more incident stem edges
than a wave has lanes and one with none, single-leaf corners at every trimmed row count, the irregular corners the host
plan check emulates, every degenerate split, a failed factorization at each place it can fail, and a family with the
fitter's conditioning. The inputs and the property each exists for are checked in test_arrowhead_structures_cpu.py."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _arrowhead_util as U  # noqa: E402
from _util import rel_err  # noqa: E402


@pytest.fixture(scope="module")
def la():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import _native
    _native.lib()
    from dynamicfuion_python_amd import nnrt
    return nnrt.core.linalg


def solve(la, system):
    return la.SolveBlockSparseArrowheadCholesky(*system).cpu().numpy()


def block_rel_err(x, x64):
    """max over the 6-vectors of the blocks of max|x_i - x64_i| / max|x64_i|"""
    d = np.abs(np.asarray(x, np.float64) - x64).reshape(-1, 6).max(1)
    return float((d / np.abs(x64).reshape(-1, 6).max(1)).max()) if len(d) else 0.0


def check_positive(la, oracle_mod, system, report=None):
    """The four assertions of every positive case; returns (x_gpu, x_fp64)."""
    diag, wing, coords, n0, b = system
    x_g = solve(la, system)
    x64, A = U.fp64_solution(diag, wing, coords, b)
    assert x_g.shape == x64.shape and np.isfinite(x_g).all()
    e64 = rel_err(x_g, x64)
    res = float(np.abs(A @ x_g.astype(np.float64) - b).max() / np.abs(b).max())
    if report:
        print(f"{report}: N = {len(diag)}, rel_err(gpu, fp64) = {e64:.3g}, residual / max|b| = {res:.3g}")
    assert e64 < 1e-5
    if len(diag) <= U.ORACLE_MAX_BLOCKS:
        x_o = oracle_mod.solve_arrowhead(diag, wing, coords, n0, b)
        assert rel_err(x_g, x_o) < 1e-4
        # Per block: the degree term of the diagonal makes x small at a corner node with many wings, so an error there
        # (one pair dropped from a list of 65 moves x by 2e-6 of max|x|, but by 7e-5 of its own block) hides under the
        # bounds above. The yardstick is the oracle's float32 solve, as for the ill-conditioned family: 8 times its
        # error (elimination and accumulation order), with a floor of 1e-6.
        bg, bo = block_rel_err(x_g, x64), block_rel_err(x_o, x64)
        if report:
            print(f"{report}: block rel_err gpu {bg:.3g}, oracle {bo:.3g}")
        assert bg <= 8 * max(bo, 1e-6)
    assert res < 1e-4
    assert np.array_equal(solve(la, system), x_g)   # the cached plan: bit-identical
    return x_g, x64


@pytest.mark.parametrize("name", ["degrees_mixed", "degrees_all_8"])
def test_stem_degrees(la, oracle_mod, name):
    """stem_factor strides a node's wing list by its four lanes: degrees 0, 1, 2, 3, 4, 5 and 8 interleaved, and all 8."""
    (n0, _, se, _), system = U.case_system(name)
    x_g, _ = check_positive(la, oracle_mod, system, name)
    diag, _, _, _, b = system
    for i in np.flatnonzero(U.stem_degrees(n0, se) == 0):   # a stem node without wings: x_i = D_i^-1 b_i
        xi = np.linalg.solve(diag[i].astype(np.float64), b[6 * i:6 * i + 6].astype(np.float64))
        assert rel_err(x_g[6 * i:6 * i + 6], xi) < 1e-5


@pytest.mark.parametrize("L", U.PAIR_LENGTHS)
def test_schur_pair_list_length(la, oracle_mod, L):
    """stem_schur_wave: a target with exactly L pairs (chunks of 64, eight at a time), two more with at least L."""
    check_positive(la, oracle_mod, U.case_system(f"pairs_{L}")[1], f"pairs_{L}")


@pytest.mark.parametrize("H", U.HUB_COUNTS)
def test_hub_corner_node(la, oracle_mod, H):
    """stem_rhs_wave: a corner node with H >= 64 incident stem edges (the stride and the reduction across the wave) and one
    with none."""
    check_positive(la, oracle_mod, U.case_system(f"hub_{H}")[1], f"hub_{H}")


@pytest.mark.parametrize("coupling", ["by_stem", "corner_edges"])
@pytest.mark.parametrize("nc", U.LEAF_SWEEP)
def test_single_leaf_dense_corner(la, oracle_mod, nc, coupling):
    """A complete corner of nc nodes: one nested-dissection group whose last tile has 6 nc mod 64 real rows, every tile
    pair with an update term (trimmed to the source column's real rows); 43 nodes has no separator and stays one group."""
    check_positive(la, oracle_mod, U.case_system(f"leaf_{nc}_{coupling}")[1], f"leaf_{nc}_{coupling}")


@pytest.mark.parametrize("ka,kb", U.CLIQUE_PAIRS)
def test_two_cliques_and_a_separator(la, oracle_mod, ka, kb):
    """Two complete leaves of ka and kb nodes under a one-node separator: the leaves' trimmed last tile columns (4 and 4,
    2 and a full tile, 30 and 36, 32 and 34 real rows) are the source of update terms on the separator's tile."""
    check_positive(la, oracle_mod, U.case_system(f"cliques_{ka}_{kb}")[1], f"cliques_{ka}_{kb}")


@pytest.mark.parametrize("name", U.DEVICE_PLAN_CASES)
def test_irregular_corner(la, oracle_mod, name):
    """The structures whose plan test_corner_plan.py emulates on the host, solved on the device."""
    check_positive(la, oracle_mod, U.case_system(f"plan_{name}")[1], name)


@pytest.mark.parametrize("name", list(U.degenerate_structures()))
def test_degenerate_split(la, oracle_mod, name):
    check_positive(la, oracle_mod, U.case_system(f"split_{name}")[1], name)


def test_empty_system(la):
    """N == 0 (include/nnrt_mi355x.h): NNRT_OK and an empty x, with empty tensors and with NULL pointers."""
    from dynamicfuion_python_amd import _native
    x = la.SolveBlockSparseArrowheadCholesky(np.zeros((0, 6, 6), np.float32), np.zeros((0, 6, 6), np.float32), np.zeros((0, 2), np.int32), 0,
                                             np.zeros(0, np.float32))
    assert tuple(x.shape) == (0,)
    null = ctypes.c_void_p(None)
    assert _native.lib().nnrt_solve_block_sparse_arrowhead_cholesky(null, null, null, 0, 0, 0, null, null, _native.stream_ptr()) == 0


def test_refused_arguments(la):
    """A negative block count, an arrow base beyond N, a NULL pointer to a non-empty array and a wing block of the empty
    system are refused with NNRT_ERROR_ARGUMENT and a message, before anything is read."""
    from dynamicfuion_python_amd import _native
    lib = _native.lib()
    diag, wing, coords, n0, b = U.case_system("pairs_1")[1]
    N, E = len(diag), len(wing)
    dev = torch.device("cuda", torch.cuda.current_device())
    D, W, C, B = (torch.as_tensor(v, device=dev).contiguous() for v in (diag, wing, coords, b))
    X = torch.empty_like(B)
    p = _native.ptr
    null = ctypes.c_void_p(None)
    calls = {
        "negative E": (p(D), p(W), p(C), -1, N, n0, p(B), p(X)),
        "negative N": (p(D), p(W), p(C), 0, -1, 0, p(B), p(X)),
        "arrow base beyond N": (p(D), p(W), p(C), E, N, N + 1, p(B), p(X)),
        "diag NULL": (null, p(W), p(C), E, N, n0, p(B), p(X)),
        "wing NULL": (p(D), null, p(C), E, N, n0, p(B), p(X)),
        "coordinates NULL": (p(D), p(W), null, E, N, n0, p(B), p(X)),
        "b NULL": (p(D), p(W), p(C), E, N, n0, null, p(X)),
        "x NULL": (p(D), p(W), p(C), E, N, n0, p(B), null),
        "wing block of the empty system": (p(D), p(W), p(C), 1, 0, 0, p(B), p(X)),
    }
    for what, args in calls.items():
        with pytest.raises(_native.NnrtError) as ex:
            _native.check(lib.nnrt_solve_block_sparse_arrowhead_cholesky(*args, _native.stream_ptr()))
        assert ex.value.status == 1, what   # NNRT_ERROR_ARGUMENT
        assert len(str(ex.value)) > len("nnrt status 1: "), what
    _native.check(lib.nnrt_solve_block_sparse_arrowhead_cholesky(p(D), p(W), p(C), E, N, n0, p(B), p(X), _native.stream_ptr()))
    assert rel_err(X.cpu().numpy(), U.fp64_solution(diag, wing, coords, b)[0]) < 1e-5


def test_not_positive_definite_each_place(la):
    """One 60-corner-node structure (a separator above two leaves): a negated stem block, a stem block with a NaN, and a
    corner block shrunk to 0.01 I at the lowest, a middle and the highest corner node each give
    NNRT_ERROR_NOT_POSITIVE_DEFINITE; the unmodified system solved right after each failure, from the cached plan, gives
    the bits of the solve made before any failure."""
    from dynamicfuion_python_amd._native import NnrtError
    from dynamicfuion_python_amd.nnrt import core
    n0, nc, se, ce = U.npd_structure()
    system = U.build_system(n0, nc, se, ce, seed=77)
    diag, wing, coords, _, b = system
    core.release_arrowhead_plans()
    x_before = solve(la, system)
    assert rel_err(x_before, U.fp64_solution(diag, wing, coords, b)[0]) < 1e-5
    for name, bad in U.npd_variants(system).items():
        with pytest.raises(NnrtError) as ex:
            la.SolveBlockSparseArrowheadCholesky(bad, wing, coords, n0, b)
        assert ex.value.status == 3, f"{name}: {ex.value}"   # NNRT_ERROR_NOT_POSITIVE_DEFINITE
        assert np.array_equal(solve(la, system), x_before), name


ILL_CASES = [(name, shift) for name in U.ill_structures() for shift in U.ILL_SHIFTS]


@pytest.mark.parametrize("name,shift", ILL_CASES)
def test_ill_conditioned_family(la, oracle_mod, name, shift):
    """The fitter's conditioning: diagonal blocks A A^T + shift I (no degree term), wings scaled so the Schur complement
    stays positive definite. The oracle's float32 dense solve in natural order is the yardstick: the device error may be
    8 times its error (another elimination order, MFMA accumulation order), with a floor of 1e-6.

    Measured on an MI355X (rel_err against the fp64 solution):

    case               shift   oracle     gpu        gpu / max(oracle, 1e-6)
    grid_8x6_knn2      1       6.18e-07   4.90e-07   0.49
    grid_8x6_knn2      0.01    1.84e-05   1.43e-05   0.78
    dense_16_by_stem   1       3.68e-06   1.58e-06   0.43
    dense_16_by_stem   0.01    1.96e-04   5.19e-05   0.27
    """
    system = U.build_ill_system(U.ill_structures()[name], shift, seed=5)
    diag, wing, coords, n0, b = system
    x64, _ = U.fp64_solution(diag, wing, coords, b)
    e_o = rel_err(oracle_mod.solve_arrowhead(diag, wing, coords, n0, b), x64)
    x_g = solve(la, system)
    e_g = rel_err(x_g, x64)
    print(f"ill {name} shift {shift:g}: oracle {e_o:.3g}, gpu {e_g:.3g}, ratio {e_g / max(e_o, 1e-6):.3g}")
    assert np.isfinite(x_g).all()
    assert e_g <= 8 * max(e_o, 1e-6)
    assert np.array_equal(solve(la, system), x_g)
