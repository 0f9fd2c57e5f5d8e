"""Arrowhead systems with explicit, irregular block structures, shared by the host plan check (test_corner_plan.py), the
structure check that runs without a GPU (test_arrowhead_structures_cpu.py) and the device tests
(test_gpu_arrowhead.py, test_gpu_arrowhead_structures.py).

A structure is (n0, nc, stem_edges, corner_edges): n0 stem nodes (block indices 0 .. n0-1), nc corner nodes
(n0 .. n0+nc-1), stem_edges [(stem node, corner node)] and corner_edges [(corner node, corner node)] as (row, column)
block coordinates. build_system gives it the values of test_gpu_arrowhead.py's grid_arrowhead (wings N(0, 0.3), diagonal
blocks A A^T + 30 I + 6 degree I, b normal), the conditioning the project's tolerances were set for.

Every structure builder has a property function next to it that returns what the case exists for (stem degrees, Schur
pair-list lengths by build_stem_schur_lists' (a >= b) rule, incident stem edges per corner node, rows in the last tile):
test_arrowhead_structures_cpu.py asserts them, so a builder that drifts says so instead of testing nothing.
"""
from collections import Counter

import numpy as np

TILE = 64      # csrc/corner.hip: rows per tile; every nested-dissection group starts on a tile boundary
ND_LEAF = 42   # csrc/corner.hip: nodes per nested-dissection leaf


# ---- values ---------------------------------------------------------------------------------------------------------
def _coords(n0, nc, stem_edges, corner_edges):
    se = np.asarray(stem_edges, np.int64).reshape(-1, 2)
    ce = np.asarray(corner_edges, np.int64).reshape(-1, 2)
    N = n0 + nc
    assert ((se[:, 0] >= 0) & (se[:, 0] < n0) & (se[:, 1] >= n0) & (se[:, 1] < N)).all(), "stem edge outside stem x corner"
    assert ((ce >= n0) & (ce < N)).all() and (ce[:, 0] != ce[:, 1]).all(), "corner edge outside corner x corner"
    return np.concatenate([se, ce], 0).astype(np.int32)


def build_system(n0, nc, stem_edges, corner_edges, seed, shift=None, wing_scale=0.3):
    """(diag [N,6,6], wing [E,6,6], coords [E,2] int32, n0, b [6N]) float32 for the structure: wing blocks
    N(0, wing_scale), diagonal blocks A A^T + 30 I + 6 degree I (shift=None, grid_arrowhead's rule) or A A^T + shift I,
    b normal. Edges keep the order given (stem edges first)."""
    rng = np.random.default_rng(seed)
    N = n0 + nc
    coords = _coords(n0, nc, stem_edges, corner_edges)
    wing = rng.normal(0, 0.3, (len(coords), 6, 6))
    wing = (wing * (wing_scale / 0.3)).astype(np.float32)
    A = rng.normal(size=(N, 6, 6))
    eye = np.eye(6)
    if shift is None:
        diag = (A @ A.transpose(0, 2, 1) + 30.0 * eye).astype(np.float32)
        deg = np.bincount(coords.ravel(), minlength=N)
        diag += (6.0 * deg)[:, None, None].astype(np.float32) * np.eye(6, dtype=np.float32)
    else:
        diag = (A @ A.transpose(0, 2, 1) + float(shift) * eye).astype(np.float32)
    b = rng.normal(size=6 * N).astype(np.float32)
    return diag, wing, coords, n0, b


def sparse_matrix(diag, wing, edges):
    """The symmetric fp64 matrix of the blocks (scipy CSC)."""
    import scipy.sparse as sp
    N = len(diag)
    edges = np.asarray(edges).reshape(-1, 2)
    bi, bj = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    rows = [6 * np.arange(N)[:, None] + bi.ravel()[None], 6 * edges[:, :1] + bi.ravel()[None], 6 * edges[:, 1:] + bi.ravel()[None]]
    cols = [6 * np.arange(N)[:, None] + bj.ravel()[None], 6 * edges[:, 1:] + bj.ravel()[None], 6 * edges[:, :1] + bj.ravel()[None]]
    vals = [diag.reshape(N, 36), wing.reshape(-1, 36), wing.transpose(0, 2, 1).reshape(-1, 36)]
    return sp.csc_matrix((np.concatenate([v.ravel() for v in vals]).astype(np.float64),
                          (np.concatenate([r.ravel() for r in rows]), np.concatenate([c.ravel() for c in cols]))), shape=(6 * N, 6 * N))


def fp64_solution(diag, wing, edges, b):
    """(x, A): the sparse fp64 solution of the float32 blocks' system and its matrix."""
    import scipy.sparse.linalg as spl
    A = sparse_matrix(diag, wing, edges)
    if A.shape[0] == 0:
        return np.zeros(0), A
    return spl.spsolve(A, b.astype(np.float64)), A


def is_positive_definite(diag, wing, edges):
    """numpy.linalg.cholesky of the dense fp64 matrix succeeds (small systems only)."""
    try:
        np.linalg.cholesky(sparse_matrix(diag, wing, edges).toarray())
        return True
    except np.linalg.LinAlgError:
        return False


# ---- the properties the cases are built for -----------------------------------------------------------------------------
def stem_degrees(n0, stem_edges):
    """[n0] wings per stem node."""
    se = np.asarray(stem_edges, np.int64).reshape(-1, 2)
    return np.bincount(se[:, 0], minlength=n0)[:n0]


def stem_degree_histogram(n0, stem_edges):
    """{degree: stem nodes with it}"""
    return dict(Counter(int(d) for d in stem_degrees(n0, stem_edges)))


def pair_list_lengths(n0, stem_edges):
    """{(a, b): pairs}, a >= b corner nodes counted from 0: the pair list of every Schur target as
    build_stem_schur_lists (csrc/arap.hip) forms it -- one pair (e1, e2) per stem node and ordered pair of its wings
    with corner(e1) >= corner(e2)."""
    by_stem = {}
    for i, j in np.asarray(stem_edges, np.int64).reshape(-1, 2):
        by_stem.setdefault(int(i), []).append(int(j) - n0)
    out = Counter()
    for ts in by_stem.values():
        for a in ts:
            for b in ts:
                if a >= b:
                    out[(a, b)] += 1
    return dict(out)


def corner_incident_counts(n0, nc, stem_edges):
    """[nc] stem edges incident to each corner node (the list stem_rhs_wave strides over)."""
    se = np.asarray(stem_edges, np.int64).reshape(-1, 2)
    return np.bincount(se[:, 1] - n0, minlength=nc)


def last_tile_rows(nc):
    """Real rows in the last 64-row tile of a single-leaf corner of nc <= 42 nodes: 6 nc mod 64 (0: the tile is full)."""
    assert nc <= ND_LEAF + 1   # (43: a complete corner has no separator and stays one group)
    return (6 * nc) % TILE


def corner_is_complete(n0, nc, stem_edges, corner_edges):
    """Every pair of corner nodes is coupled: by a corner edge or by a stem node attached to both."""
    return len(corner_adjacency(n0, nc, stem_edges, corner_edges)) == nc * (nc - 1) // 2


# ---- structure builders -------------------------------------------------------------------------------------------------
STEM_DEGREE_CYCLE = (0, 1, 2, 3, 4, 5, 8)


def stem_degree_structure(degrees, nc=12, seed=0):
    """Stem node i has degrees[i] wings to distinct corner nodes, drawn at random; the edge list is shuffled (a node's
    wings are not contiguous in it)."""
    rng = np.random.default_rng(seed)
    se = []
    for i, d in enumerate(degrees):
        assert d <= nc
        se += [(i, len(degrees) + int(a)) for a in rng.choice(nc, d, replace=False)]
    se = [se[k] for k in rng.permutation(len(se))]
    return len(degrees), nc, se, []


def mixed_degree_structure(repeats=4):
    """Degrees 0, 1, 2, 3, 4, 5, 8 interleaved in index order, `repeats` nodes of each."""
    return stem_degree_structure(list(STEM_DEGREE_CYCLE) * repeats, seed=101)


def all_eight_structure(repeats=4):
    return stem_degree_structure([8] * (len(STEM_DEGREE_CYCLE) * repeats), seed=102)


PAIR_A, PAIR_B = 3, 1      # the two corner nodes of pair_list_structure (counted from 0), target (PAIR_A, PAIR_B)
PAIR_LENGTHS = (1, 7, 8, 9, 63, 64, 65, 129)


def pair_list_structure(L, nc=5):
    """Exactly L stem nodes attach to both corner nodes PAIR_A and PAIR_B; four more stem nodes tie the other corner
    nodes in, so the corner is not trivial: target (PAIR_A, PAIR_B) has L pairs, (PAIR_A, PAIR_A) and (PAIR_B, PAIR_B)
    at least L."""
    others = [(0, PAIR_A), (2, PAIR_B), (4, 0), (2, 4)]
    n0 = L + len(others)
    se = []
    for i in range(L):
        # alternate the order of the two wings in the edge list: pairs come out (e1, e2) with corner(e1) >= corner(e2) either way
        pair = (PAIR_A, PAIR_B) if i % 2 == 0 else (PAIR_B, PAIR_A)
        se += [(i, n0 + pair[0]), (i, n0 + pair[1])]
    for k, (a, b) in enumerate(others):
        se += [(L + k, n0 + a), (L + k, n0 + b)]
    return n0, nc, se, []


HUB, HUB_LONER = 2, 5
HUB_COUNTS = (64, 65, 200)


def hub_structure(H, nc=6):
    """Corner node HUB is incident to H stem nodes, each with one further wing to another corner node in turn; corner
    node HUB_LONER has no stem edge, only corner-corner edges."""
    spokes = [a for a in range(nc) if a not in (HUB, HUB_LONER)]
    se = []
    for i in range(H):
        se += [(i, H + HUB), (i, H + spokes[i % len(spokes)])]
    ce = [(H + HUB_LONER, H + 0), (H + 3, H + HUB_LONER)]   # one in each (row, column) order
    return H, nc, se, ce


LEAF_SWEEP = (1, 5, 6, 10, 11, 16, 17, 21, 22, 32, 42, 43)
# real rows of the last tile for each size (0: full), written out: 6 nc mod 64
LEAF_LAST_TILE_ROWS = {1: 6, 5: 30, 6: 36, 10: 60, 11: 2, 16: 32, 17: 38, 21: 62, 22: 4, 32: 0, 42: 60, 43: 2}


def dense_corner_structure(nc, by_stem):
    """A complete corner of nc nodes. by_stem: one stem node per pair a <= b of corner nodes (wings to a and b; a == b: one
    wing), so every tile pair gets a Schur update; else n0 = 0 and one corner-corner edge per pair."""
    if by_stem:
        pairs = [(a, b) for a in range(nc) for b in range(a, nc)]
        n0 = len(pairs)
        se = []
        for i, (a, b) in enumerate(pairs):
            se.append((i, n0 + a))
            if b != a:
                se.append((i, n0 + b))
        return n0, nc, se, []
    return 0, nc, [], [(b, a) for a in range(nc) for b in range(a + 1, nc)]


# (clique A, clique B) sizes: the last tile of each leaf has 6 k mod 64 real rows -- 4 and 4, 2 and a full tile, 30 and 36, 32 and 34
CLIQUE_PAIRS = ((22, 22), (11, 32), (5, 38), (16, 27))


def two_cliques_structure(ka, kb):
    """Two complete sets of corner nodes, A (ka nodes, coupled by one stem node per pair) and B (kb nodes, coupled by
    corner-corner edges), and one corner node S coupled to every other by corner-corner edges; no coupling between A
    and B. With ka + kb + 1 > ND_LEAF the nested dissection finds S as the separator: A and B are leaves, so their
    trimmed last tile columns are the *source* of update terms on S's tile (in a single-leaf corner the trimmed tile is
    the last column and updates nothing)."""
    assert ka + kb + 1 > ND_LEAF and ka <= ND_LEAF and kb <= ND_LEAF
    nc = ka + kb + 1
    pairs = [(a, b) for a in range(ka) for b in range(a + 1, ka)]
    n0 = len(pairs)
    se = []
    for i, (a, b) in enumerate(pairs):
        se += [(i, n0 + a), (i, n0 + b)]
    ce = [(n0 + b, n0 + a) for a in range(ka, ka + kb) for b in range(a + 1, ka + kb)]
    ce += [(n0 + nc - 1, n0 + a) for a in range(nc - 1)]
    return n0, nc, se, ce


def corner_adjacency(n0, nc, stem_edges, corner_edges):
    """Coupled pairs {(a, b), a > b} of corner nodes: corner edges and pairs sharing a stem node (plan_corner's rule)."""
    seen = set()
    for a, b in np.asarray(corner_edges, np.int64).reshape(-1, 2):
        seen.add((int(max(a, b)) - n0, int(min(a, b)) - n0))
    return seen | {k for k in pair_list_lengths(n0, stem_edges) if k[0] != k[1]}


# ---- the host plan check's structures (test_corner_plan.py) ----------------------------------------------------------
def _nearest(points, centres, k):
    d = ((points[:, None, :] - centres[None]) ** 2).sum(2)
    k = min(k, len(centres))
    return np.argsort(d, axis=1, kind="stable")[:, :k]


def structure(corner_pos, stem_per_corner, corner_knn, seed):
    """Arrowhead edges of a two-layer hierarchy: corner nodes at corner_pos [n1, 3], n0 = stem_per_corner * n1 stem
    nodes scattered among them, each with edges to its 4 nearest corner nodes; corner_knn > 0 adds edges from every
    corner node to its corner_knn nearest corner nodes (the corner-corner blocks of >= 3 layers)."""
    rng = np.random.default_rng(seed)
    n1 = len(corner_pos)
    n0 = stem_per_corner * n1
    lo, hi = corner_pos.min(0), corner_pos.max(0)
    stem = rng.uniform(lo, np.maximum(hi, lo + 1e-3), (n0, 3))
    edges = []
    if n0:
        near = _nearest(stem, corner_pos, 4)
        edges.append(np.stack([np.repeat(np.arange(n0), near.shape[1]), n0 + near.ravel()], 1))
    if corner_knn and n1 > 1:
        near = _nearest(corner_pos, corner_pos, corner_knn + 1)[:, 1:]
        pairs = {(max(a, b), min(a, b)) for a in range(n1) for b in near[a] if a != b}
        edges.append(np.array([(n0 + a, n0 + b) for a, b in sorted(pairs)], np.int64).reshape(-1, 2))
    e = np.concatenate(edges, 0).astype(np.int32) if edges else np.zeros((0, 2), np.int32)
    return e, n0, n0 + n1


def grid(cx, cy, jitter, seed):
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(cx, dtype=np.float32), np.arange(cy, dtype=np.float32), indexing="xy")
    p = np.stack([gx.ravel(), gy.ravel(), np.zeros(cx * cy, np.float32)], 1)
    return (p + rng.normal(0, jitter, p.shape)).astype(np.float32)


PLAN_CASES = {
    # name: (corner positions, stem nodes per corner node, corner-corner K-NN, seed)
    "grid_12x8": (lambda: grid(12, 8, 0.0, 0), 4, 0, 1),
    "grid_12x8_corner_edges": (lambda: grid(12, 8, 0.0, 0), 4, 2, 2),
    "grid_26x15_c5_like": (lambda: grid(26, 15, 0.1, 3), 12, 0, 3),
    "grid_30x3_strip": (lambda: grid(30, 3, 0.05, 4), 4, 2, 4),
    "random_cloud_300": (lambda: np.random.default_rng(5).uniform(0, 10, (300, 3)).astype(np.float32), 6, 0, 5),
    "random_cloud_150_knn3": (lambda: np.random.default_rng(6).uniform(0, 5, (150, 3)).astype(np.float32), 3, 3, 6),
    "two_clusters": (lambda: np.concatenate([grid(8, 8, 0.0, 7), grid(8, 8, 0.0, 8) + np.float32([100, 0, 0])]), 3, 0, 7),
    "leaf_sized_42": (lambda: grid(7, 6, 0.0, 9), 3, 1, 9),
    "just_above_leaf_43": (lambda: grid(43, 1, 0.0, 10), 2, 1, 10),
    "single_corner_node": (lambda: grid(1, 1, 0.0, 11), 5, 0, 11),
    "two_corner_nodes_no_stem": (lambda: grid(2, 1, 0.0, 12), 0, 1, 12),
}
DEVICE_PLAN_CASES = ("random_cloud_300", "random_cloud_150_knn3", "two_clusters", "just_above_leaf_43", "two_corner_nodes_no_stem")


def split_edges(edges, n0):
    """structure()'s edge array as (stem_edges, corner_edges)."""
    edges = np.asarray(edges).reshape(-1, 2)
    stem = edges[:, 0] < n0
    return edges[stem], edges[~stem]


def plan_like(pos, spc, knn, seed):
    """structure() as (n0, nc, stem_edges, corner_edges)."""
    edges, n0, N = structure(pos, spc, knn, seed)
    se, ce = split_edges(edges, n0)
    return n0, N - n0, se, ce


def plan_case_structure(name):
    make_pos, spc, knn, seed = PLAN_CASES[name]
    return plan_like(make_pos(), spc, knn, seed)


# ---- degenerate splits ------------------------------------------------------------------------------------------------
def degenerate_structures():
    """{name: structure} for every split arrowhead_solve_core branches on (N == 0 apart)."""
    ring = [(a, (a + 1) % 7) for a in range(7)]
    return {
        "block_diagonal_no_corner": (9, 0, [], []),                                        # n0 == N, E == 0
        "corner_only_no_edges": (0, 7, [], []),                                            # n0 == 0, E == 0
        "corner_only_with_edges": (0, 7, [], ring),                                        # n0 == 0, corner edges
        "no_edges_stem_and_corner": (9, 7, [], []),                                        # E == 0
        "corner_edges_only_with_stem": (9, 7, [], [(9 + a, 9 + b) for a, b in ring]),      # targets == 0
    }


# ---- every positive case by name --------------------------------------------------------------------------------------
def _positive_cases():
    cases = {"degrees_mixed": mixed_degree_structure, "degrees_all_8": all_eight_structure}
    for L in PAIR_LENGTHS:
        cases[f"pairs_{L}"] = lambda L=L: pair_list_structure(L)
    for H in HUB_COUNTS:
        cases[f"hub_{H}"] = lambda H=H: hub_structure(H)
    for nc in LEAF_SWEEP:
        cases[f"leaf_{nc}_by_stem"] = lambda nc=nc: dense_corner_structure(nc, True)
        cases[f"leaf_{nc}_corner_edges"] = lambda nc=nc: dense_corner_structure(nc, False)
    for ka, kb in CLIQUE_PAIRS:
        cases[f"cliques_{ka}_{kb}"] = lambda ka=ka, kb=kb: two_cliques_structure(ka, kb)
    for name in DEVICE_PLAN_CASES:
        cases[f"plan_{name}"] = lambda name=name: plan_case_structure(name)
    for name in degenerate_structures():
        cases[f"split_{name}"] = lambda name=name: degenerate_structures()[name]
    return cases


POSITIVE_CASES = _positive_cases()   # name -> function returning (n0, nc, stem_edges, corner_edges)
ORACLE_MAX_BLOCKS = 600              # the oracle's dense restatement is compared up to this many blocks


def case_system(name):
    """(structure, system) of a positive case; the seed is the case's position in POSITIVE_CASES."""
    struct = POSITIVE_CASES[name]()
    n0, nc, se, ce = struct
    return struct, build_system(n0, nc, se, ce, seed=1000 + list(POSITIVE_CASES).index(name))


# ---- not positive definite ----------------------------------------------------------------------------------------------
def npd_structure():
    """60 corner nodes on a 10 x 6 grid (more than a leaf, so the plan has a separator) with corner-corner edges and two
    stem nodes per corner node."""
    return plan_like(grid(10, 6, 0.0, 31), 2, 2, 31)


def npd_variants(system):
    """{name: diag'} the failing variants of a system: diag with one block made indefinite."""
    diag, _, _, n0, _ = system
    N = len(diag)
    nc = N - n0
    out = {}
    d = diag.copy()
    d[n0 // 2] = -d[n0 // 2]
    out["stem_block_negated"] = d
    d = diag.copy()
    d[n0 // 3, 3, 1] = d[n0 // 3, 1, 3] = np.nan
    out["stem_block_nan"] = d
    for tag, a in (("lowest", 0), ("middle", nc // 2), ("highest", nc - 1)):
        d = diag.copy()
        d[n0 + a] = 0.01 * np.eye(6, dtype=np.float32)
        out[f"corner_block_shrunk_{tag}"] = d
    return out


# ---- ill-conditioned family ---------------------------------------------------------------------------------------------
ILL_SHIFTS = (1.0, 1e-2)


def ill_structures():
    return {
        "grid_8x6_knn2": plan_like(grid(8, 6, 0.0, 41), 2, 2, 41),
        "dense_16_by_stem": dense_corner_structure(16, True),
    }


def build_ill_system(struct, shift, seed):
    """The system of build_system with the diagonal shift 30 I + 6 degree I replaced by shift I, and the wings scaled
    down from N(0, 0.3) by halving until the matrix keeps at least half the smallest eigenvalue of its diagonal blocks:
    the Schur complement then stays positive definite in fp64 with the wings as strong as that allows."""
    n0, nc, se, ce = struct
    scale = 0.3
    for _ in range(40):
        system = build_system(n0, nc, se, ce, seed, shift=shift, wing_scale=scale)
        diag, wing, coords = system[:3]
        floor = np.linalg.eigvalsh(diag.astype(np.float64)).min()
        if np.linalg.eigvalsh(sparse_matrix(diag, wing, coords).toarray()).min() >= 0.5 * floor:
            return system
        scale *= 0.5
    raise AssertionError("no wing scale keeps the system positive definite")
