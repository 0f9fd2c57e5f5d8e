"""The inputs of test_gpu_arrowhead_structures.py, checked without a GPU: every case has the property it is named for
(stem degrees, Schur pair-list lengths, incident stem edges per corner node, rows in the last tile, the split of the
degenerate systems, indefiniteness of the failing variants), and the oracle's float restatement of the solve agrees with
the fp64 solution on it, so a device test whose inputs drift fails here instead of silently testing nothing."""
import numpy as np
import pytest

import _arrowhead_util as U
from _util import rel_err
from test_corner_plan import checker, run  # noqa: F401  (the host plan checker: its fixture and its runner)


@pytest.fixture(scope="module")
def solved():
    """(structure, system, x_fp64) per positive case, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            struct, system = U.case_system(name)
            diag, wing, coords, n0, b = system
            cache[name] = (struct, system, U.fp64_solution(diag, wing, coords, b)[0])
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(U.POSITIVE_CASES))
def test_oracle_agrees_with_fp64(oracle_mod, solved, name):
    (n0, nc, _, _), (diag, wing, coords, _, b), x64 = solved(name)
    assert len(x64) == 6 * (n0 + nc) and np.isfinite(x64).all()
    if n0 + nc > U.ORACLE_MAX_BLOCKS:
        return
    assert rel_err(oracle_mod.solve_arrowhead(diag, wing, coords, n0, b), x64) < 1e-5


def test_build_system_values():
    """grid_arrowhead's rule: diagonal blocks symmetric with the 30 + 6 degree shift, the edge order kept."""
    n0, nc, se, ce = U.hub_structure(64)
    diag, wing, coords, n0_, b = U.build_system(n0, nc, se, ce, seed=1)
    assert n0_ == n0 and coords.dtype == np.int32 and np.array_equal(coords, np.array(se + ce, np.int32))
    assert diag.dtype == wing.dtype == b.dtype == np.float32
    assert diag.shape == (n0 + nc, 6, 6) and wing.shape == (len(coords), 6, 6) and b.shape == (6 * (n0 + nc),)
    assert np.array_equal(diag, diag.transpose(0, 2, 1))
    deg = np.bincount(coords.ravel(), minlength=n0 + nc)
    assert (np.linalg.eigvalsh(diag.astype(np.float64)).min(1) >= 30 + 6 * deg - 1e-3).all()
    assert 0.25 < wing.std() < 0.35


def test_mixed_degrees():
    n0, nc, se, _ = U.POSITIVE_CASES["degrees_mixed"]()
    deg = U.stem_degrees(n0, se)
    assert nc == 12
    assert U.stem_degree_histogram(n0, se) == {d: 4 for d in (0, 1, 2, 3, 4, 5, 8)}
    assert [int(d) for d in deg[:7]] == [0, 1, 2, 3, 4, 5, 8]   # interleaved in index order
    for i in range(n0):   # distinct corner targets per node
        ts = [j for s, j in se if s == i]
        assert len(set(ts)) == len(ts) == deg[i]
    order = [s for s, _ in se]
    assert order != sorted(order)   # a node's wings are not contiguous in the edge list


def test_all_degrees_eight():
    n0, nc, se, _ = U.POSITIVE_CASES["degrees_all_8"]()
    assert nc == 12 and n0 == U.POSITIVE_CASES["degrees_mixed"]()[0]
    assert U.stem_degree_histogram(n0, se) == {8: n0}
    assert all(len({j for s, j in se if s == i}) == 8 for i in range(n0))


@pytest.mark.parametrize("L", U.PAIR_LENGTHS)
def test_pair_list_lengths(L):
    n0, nc, se, ce = U.POSITIVE_CASES[f"pairs_{L}"]()
    lengths = U.pair_list_lengths(n0, se)
    assert nc > 2 and not ce
    assert lengths[(U.PAIR_A, U.PAIR_B)] == L   # some target's pair list has exactly L entries
    assert lengths[(U.PAIR_A, U.PAIR_A)] >= L and lengths[(U.PAIR_B, U.PAIR_B)] >= L
    assert all(a >= b for a, b in lengths)
    assert {a for a, _ in lengths} | {b for _, b in lengths} == set(range(nc))   # every corner node takes part


def test_pair_lengths_cover_the_chunk_edges():
    assert set(U.PAIR_LENGTHS) == {1, 7, 8, 9, 63, 64, 65, 129}


@pytest.mark.parametrize("H", U.HUB_COUNTS)
def test_hub_incident_counts(H):
    n0, nc, se, ce = U.POSITIVE_CASES[f"hub_{H}"]()
    inc = U.corner_incident_counts(n0, nc, se)
    assert inc[U.HUB] == H and inc[U.HUB_LONER] == 0
    assert U.stem_degree_histogram(n0, se) == {2: H}   # the hub and one further wing each
    touching = [tuple(int(v) - n0 for v in e) for e in ce if n0 + U.HUB_LONER in e]
    assert len(touching) == 2                            # the loner has corner-corner edges only
    assert U.pair_list_lengths(n0, se)[(U.HUB, U.HUB)] == H


def test_hub_counts_cover_the_stride():
    assert set(U.HUB_COUNTS) == {64, 65, 200}


@pytest.mark.parametrize("by_stem", [True, False], ids=["by_stem", "corner_edges"])
@pytest.mark.parametrize("nc", U.LEAF_SWEEP)
def test_leaf_sweep_is_dense_with_the_named_tail(nc, by_stem):
    n0, nc_, se, ce = U.POSITIVE_CASES[f"leaf_{nc}_{'by_stem' if by_stem else 'corner_edges'}"]()
    assert nc_ == nc
    assert U.corner_is_complete(n0, nc, se, ce)
    assert U.last_tile_rows(nc) == U.LEAF_LAST_TILE_ROWS[nc] == (6 * nc) % 64
    if by_stem:
        assert not ce and n0 == nc * (nc + 1) // 2
        assert all(v == 1 for k, v in U.pair_list_lengths(n0, se).items() if k[0] != k[1])
    else:
        assert n0 == 0 and not se and len(ce) == nc * (nc - 1) // 2


def test_leaf_sweep_reaches_every_trimmed_row_count():
    """The real-row counts of the last tile the sweep exists for: 2, 4, 6, 30, 32, 36 and a full tile; one size above a leaf."""
    assert set(U.LEAF_SWEEP) == {1, 5, 6, 10, 11, 16, 17, 21, 22, 32, 42, 43}
    assert {2, 4, 6, 30, 32, 36, 0} <= {U.LEAF_LAST_TILE_ROWS[nc] for nc in U.LEAF_SWEEP}
    assert max(U.LEAF_SWEEP) == U.ND_LEAF + 1
    assert any((6 * k) % 64 > 58 for k in range(1, 43))   # 6-row nodes straddle tiles inside the larger leaves


def _plan_size(checker, tmp_path, struct):
    """(ld, T) of the structure's plan without positions (the C-ABI path), from the host plan checker; the checker also
    emulates the plan's launches in double precision."""
    n0, nc, se, ce = struct
    edges = np.concatenate([np.reshape(se, (-1, 2)), np.reshape(ce, (-1, 2))]).astype(np.int32)
    out = run(checker, tmp_path, edges, n0, n0 + nc, None)
    assert "residual" in out
    words = next(line for line in out.splitlines() if line.startswith("nc ")).split()
    assert int(words[1]) == nc
    return int(words[3]), int(words[5])


@pytest.mark.parametrize("ka,kb", U.CLIQUE_PAIRS)
def test_two_cliques_are_two_leaves_and_a_separator(checker, tmp_path, ka, kb):
    struct = U.POSITIVE_CASES[f"cliques_{ka}_{kb}"]()
    n0, nc, se, ce = struct
    adj = U.corner_adjacency(n0, nc, se, ce)
    A, B, S = range(ka), range(ka, ka + kb), nc - 1
    assert nc == ka + kb + 1 > U.ND_LEAF
    assert all((b, a) in adj for a in A for b in A if b > a) and all((b, a) in adj for a in B for b in B if b > a)
    assert all((S, a) in adj for a in range(nc - 1))
    assert not any((b, a) in adj for a in A for b in B)
    assert len(adj) == ka * (ka - 1) // 2 + kb * (kb - 1) // 2 + nc - 1
    # each leaf starts on a tile boundary, so its last tile is trimmed to 6 k mod 64 rows; the separator has a tile of its own
    tiles = -(-6 * ka // 64) + -(-6 * kb // 64) + 1
    assert _plan_size(checker, tmp_path, struct) == (64 * tiles, tiles)
    assert {(6 * ka) % 64, (6 * kb) % 64} == {(22, 22): {4}, (11, 32): {2, 0}, (5, 38): {30, 36}, (16, 27): {32, 34}}[(ka, kb)]


def test_complete_corner_above_a_leaf_stays_one_group(checker, tmp_path):
    """43 coupled nodes have no separator: one group of 258 rows, five tiles, the last with two real rows."""
    for coupling in ("by_stem", "corner_edges"):
        assert _plan_size(checker, tmp_path, U.POSITIVE_CASES[f"leaf_43_{coupling}"]()) == (320, 5)


@pytest.mark.parametrize("name", U.DEVICE_PLAN_CASES)
def test_plan_structures_are_the_host_check_s(name):
    make_pos, spc, knn, seed = U.PLAN_CASES[name]
    edges, n0, N = U.structure(make_pos(), spc, knn, seed)
    n0_, nc, se, ce = U.POSITIVE_CASES[f"plan_{name}"]()
    assert (n0_, nc) == (n0, N - n0)
    assert sorted(map(tuple, np.concatenate([np.reshape(se, (-1, 2)), np.reshape(ce, (-1, 2))]).tolist())) == sorted(map(tuple, edges.tolist()))


def test_degenerate_splits():
    S = {k: U.POSITIVE_CASES[f"split_{k}"]() for k in U.degenerate_structures()}
    n0, nc, se, ce = S["block_diagonal_no_corner"]
    assert n0 > 0 and nc == 0 and not se and not ce
    n0, nc, se, ce = S["corner_only_no_edges"]
    assert n0 == 0 and nc > 0 and not se and not ce
    n0, nc, se, ce = S["corner_only_with_edges"]
    assert n0 == 0 and nc > 0 and not se and ce
    n0, nc, se, ce = S["no_edges_stem_and_corner"]
    assert n0 > 0 and nc > 0 and not se and not ce
    n0, nc, se, ce = S["corner_edges_only_with_stem"]
    assert n0 > 0 and nc > 0 and not se and ce and not U.pair_list_lengths(n0, se)


def test_not_positive_definite_variants():
    n0, nc, se, ce = U.npd_structure()
    assert nc == 60 and nc > U.ND_LEAF and len(ce) > 0 and n0 > 0
    system = U.build_system(n0, nc, se, ce, seed=77)
    diag, wing, coords, _, _ = system
    assert U.is_positive_definite(diag, wing, coords)
    variants = U.npd_variants(system)
    assert set(variants) == {"stem_block_negated", "stem_block_nan", "corner_block_shrunk_lowest", "corner_block_shrunk_middle",
                             "corner_block_shrunk_highest"}
    for name, d in variants.items():
        changed = np.flatnonzero((d != diag).reshape(len(d), -1).any(1))
        assert len(changed) == 1, name
        assert (changed[0] < n0) == name.startswith("stem"), name
        if name == "stem_block_nan":
            assert np.isnan(d).sum() == 2 and np.isnan(np.tril(d[changed[0]], -1)).any()   # in the triangle a Cholesky reads
            continue
        assert not U.is_positive_definite(d, wing, coords), name
    shrunk = sorted(int(np.flatnonzero((variants[f"corner_block_shrunk_{t}"] != diag).reshape(len(diag), -1).any(1))[0]) - n0
                    for t in ("lowest", "middle", "highest"))
    assert shrunk == [0, nc // 2, nc - 1]


@pytest.mark.parametrize("shift", U.ILL_SHIFTS)
@pytest.mark.parametrize("name", list(U.ill_structures()))
def test_ill_conditioned_family(oracle_mod, name, shift):
    """Positive definite in fp64 (numpy.linalg.cholesky), wings not scaled away, and the float32 yardstick (the oracle's
    dense solve in natural order) itself below 1e-2, so that a multiple of its error means something."""
    struct = U.ill_structures()[name]
    diag, wing, coords, n0, b = U.build_ill_system(struct, shift, seed=5)
    assert len(diag) <= U.ORACLE_MAX_BLOCKS
    assert U.is_positive_definite(diag, wing, coords)
    assert np.abs(wing).max() > 0
    floor = np.linalg.eigvalsh(diag.astype(np.float64)).min()
    # the shift sets the smallest block eigenvalue (A A^T adds next to nothing), up to the blocks' rounding to float32
    assert shift - 1e-4 <= floor < shift + 0.5
    x64, _ = U.fp64_solution(diag, wing, coords, b)
    err = rel_err(oracle_mod.solve_arrowhead(diag, wing, coords, n0, b), x64)
    assert err < 1e-2, err
