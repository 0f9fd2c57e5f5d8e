"""Expected values for the fitter's coupled data term (nnrt_fitter_set_data_coupling): the full
Gauss-Newton system H = sum_p J_p^T J_p assembled in float64 from the CPU oracle's existing stage functions (the same
calls, in the same order, as tests/_robust_util.py's data_term / arap_term), its dense fp64 solve and one coupled GN step.

Block layout, as the fitter exports it: diagonal blocks [N,6,6] (data + ARAP + LM), the pairs (i, j), i < j, ascending,
block (i, j) of each pair (its transpose sits at (j, i)), right-hand side = negative gradient [6N]."""
import numpy as np

from _robust_util import F32, arap_term, huber_scale, identity_motion, virtual_nodes   # noqa: F401
from _util import rodrigues64


def face_pairs(O, sc, anchor_count=4):
    """The sorted unique node pairs (i < j) that share a face, from the oracle's associate_faces_with_anchors table."""
    nodes = virtual_nodes(sc)
    a, _ = O.compute_anchors(sc.points, nodes, anchor_count, sc.coverage)
    fnodes, _, fcounts = O.associate_faces_with_anchors(sc.faces, a)
    S = fnodes.shape[1]
    out = set()
    for x in range(S):
        for y in range(x + 1, S):
            ok = fcounts > y
            i, j = fnodes[ok, x], fnodes[ok, y]
            out.update(zip(np.minimum(i, j).tolist(), np.maximum(i, j).tolist()))
    out = {(i, j) for i, j in out if i != j}
    return np.array(sorted(out), np.int32).reshape(-1, 2)


def edge_pairs(sc):
    """The hierarchy's edges as unordered pairs (i < j); empty without a hierarchy."""
    if not sc.hierarchy:
        return np.zeros((0, 2), np.int32)
    e = np.asarray(sc.hierarchy["edges"], np.int32).reshape(-1, 2)
    return np.stack([e.min(axis=1), e.max(axis=1)], axis=1)


def union_pairs(*lists):
    s = set()
    for l in lists:
        s.update(map(tuple, np.asarray(l).reshape(-1, 2).tolist()))
    return np.array(sorted(s), np.int32).reshape(-1, 2)


def data_system(O, sc, depth, R=None, t=None, anchor_count=4, tukey_c=None):
    """One iteration's data term at node motion (R, t) (virtual order; default the identity), float64 sums of the
    oracle's float32 pixel-node Jacobian rows: dense block array Hfull [N,N,6,6] (all blocks, both triangles), the
    negative gradient g [6N], plus the stage outputs the checks need (pj, pc, face table, pixel faces, residuals, masks,
    the oracle's own float32 diagonal blocks and gradient, `touched` [N,N] = some pixel contributes to the block)."""
    nodes = virtual_nodes(sc)
    N, H, W = len(nodes), sc.H, sc.W
    P = H * W
    if R is None:
        R, t = identity_motion(N)
    R = np.ascontiguousarray(R, F32).reshape(N, 3, 3)
    t = np.ascontiguousarray(t, F32).reshape(N, 3)
    refp, refm = O.unproject(depth, sc.K, 1.0, 10.0)
    a, w = O.compute_anchors(sc.points, nodes, anchor_count, sc.coverage)
    fnodes, fslots, fcounts = O.associate_faces_with_anchors(sc.faces, a)
    wp, wn = O.warp_mesh(sc.points, sc.normals, nodes, R, t, a, w)
    fndc, fm = O.extract_face_ndc(wp, sc.faces, sc.K, H, W, 0.0, 10.0)
    fi, dep, bary, _ = O.rasterize_k1_fast(fndc, fm, H, W, 0.5, True, True)
    rnorm = O.interpolate_face_attributes(fi, bary, wn[sc.faces]).reshape(P, 3)
    rpts, rmask = O.unproject(np.ascontiguousarray(dep[..., 0]), sc.K, 1.0, 10.0)
    pmv = (rpts - refp).astype(F32)
    mask = refm & rmask
    with np.errstate(invalid="ignore", over="ignore"):
        r = ((rnorm[:, 0] * pmv[:, 0] + rnorm[:, 1] * pmv[:, 1]) + rnorm[:, 2] * pmv[:, 2]).astype(F32)
    r[~mask] = 0.0
    if tukey_c is None:
        s = np.ones(P, F32)
        contributes = mask.copy()
    else:
        c = F32(tukey_c)
        contributes = mask & (np.abs(r) <= c)
        q = (r / c).astype(F32)
        s = (F32(1.0) - q * q).astype(F32)
    residuals = np.where(contributes, (s * r).astype(F32), F32(0.0)).astype(F32)
    vj, nj = O.warped_surface_jacobians(sc.points, sc.normals, nodes, R, a, w)
    rvj, rnj = O.rasterized_surface_jacobians(wp, wn, sc.faces, fi, bary, sc.K, True)
    pj, pc = O.pixel_vertex_anchor_jacobians(rvj, rnj, vj, nj, (pmv * s[:, None]).astype(F32), (rnorm * s[:, None]).astype(F32),
                                             contributes, fi, sc.faces, fnodes, fslots, fcounts, False, 0.01, "ALL")
    Hd, g = O.data_hessian_gradient(pj, pc, fi, fnodes, residuals, contributes, N, "ALL")
    pf = fi.reshape(P).astype(np.int64)
    px = np.nonzero(contributes & (pf >= 0))[0]
    J = pj[px].astype(np.float64)              # [n, S, 6]
    fn = fnodes[pf[px]].astype(np.int64)       # [n, S]
    cnt = fcounts[pf[px]]
    S = fn.shape[1]
    Hfull = np.zeros((N, N, 6, 6))
    touched = np.zeros((N, N), bool)
    g64 = np.zeros((N, 6))
    for x in range(S):
        okx = cnt > x
        np.add.at(g64, fn[okx, x], -J[okx, x] * residuals[px][okx, None].astype(np.float64))
        for y in range(S):
            ok = okx & (cnt > y)
            if not ok.any():
                continue
            np.add.at(Hfull, (fn[ok, x], fn[ok, y]), J[ok, x, :, None] * J[ok, y, None, :])
            touched[fn[ok, x], fn[ok, y]] = True
    return dict(Hfull=Hfull, g=g64.reshape(-1), touched=touched, pj=pj, pc=pc, face_nodes=fnodes, face_counts=fcounts, pixel_faces=pf,
                residual_mask=mask, residuals=residuals, contributes=contributes, hessian_diag=Hd, gradient=g, r=r, s=s,
                cost=float((residuals[mask].astype(np.float64) ** 2).sum()))


def coupled_system(O, sc, depth, R=None, t=None, anchor_count=4, tukey_c=None, lm=0.001, arap_weight=200.0, huber_delta=None,
                   with_arap=None):
    """The block system of one coupled iteration: dict(diag [N,6,6], pairs [M,2], blocks [M,6,6], rhs [6N], data) in float64.
    pairs = the oracle table's face pairs, united with the hierarchy's edges when the scene has one."""
    N = len(sc.nodes)
    if R is None:
        R, t = identity_motion(N)
    d = data_system(O, sc, depth, R, t, anchor_count, tukey_c)
    with_arap = bool(sc.hierarchy) if with_arap is None else with_arap
    pairs = union_pairs(face_pairs(O, sc, anchor_count), edge_pairs(sc) if with_arap else [])
    Hf = d["Hfull"].copy()
    rhs = d["g"].copy()
    if with_arap:
        ar = arap_term(O, sc, R, t, arap_weight, huber_delta)
        for n in range(N):
            Hf[n, n] += ar["diag"][n].astype(np.float64)
        for e, (i, j) in enumerate(np.asarray(sc.hierarchy["edges"]).reshape(-1, 2)):
            Hf[i, j] += ar["wing"][e].astype(np.float64)
            Hf[j, i] += ar["wing"][e].astype(np.float64).T
        rhs = rhs + ar["gradient"].astype(np.float64)
    diag = Hf[np.arange(N), np.arange(N)] + lm * np.eye(6)
    blocks = Hf[pairs[:, 0], pairs[:, 1]] if len(pairs) else np.zeros((0, 6, 6))
    # nothing outside the pair list
    off = Hf.copy()
    off[np.arange(N), np.arange(N)] = 0
    if len(pairs):
        off[pairs[:, 0], pairs[:, 1]] = 0
        off[pairs[:, 1], pairs[:, 0]] = 0
    assert not off.any(), "a block outside the pair structure is non-zero"
    return dict(diag=diag, pairs=pairs, blocks=blocks, rhs=rhs, data=d)


def dense_matrix(diag, pairs, blocks):
    N = len(diag)
    A = np.zeros((6 * N, 6 * N))
    for n in range(N):
        A[6 * n:6 * n + 6, 6 * n:6 * n + 6] = diag[n]
    for (i, j), b in zip(np.asarray(pairs).reshape(-1, 2), np.asarray(blocks, np.float64).reshape(-1, 6, 6)):
        A[6 * i:6 * i + 6, 6 * j:6 * j + 6] = b
        A[6 * j:6 * j + 6, 6 * i:6 * i + 6] = b.T
    return A


def solve_dense(diag, pairs, blocks, rhs):
    """fp64 dense solution of a block system, and its 2-norm condition number."""
    A = dense_matrix(np.asarray(diag, np.float64), pairs, blocks)
    return np.linalg.solve(A, np.asarray(rhs, np.float64)), float(np.linalg.cond(A))


def solve_float32(diag, pairs, blocks, rhs):
    """A plain float32 numpy Cholesky solve of the same system (the yardstick for a float32 solver's error)."""
    A = dense_matrix(np.asarray(diag, np.float64), pairs, blocks).astype(F32)
    L = np.linalg.cholesky(A)
    y = np.linalg.solve(L, np.asarray(rhs, F32)).astype(F32)
    return np.linalg.solve(L.T, y).astype(F32)


def apply_update(R, t, x):
    """R <- R Rodrigues(w), t <- t + dt (fp64 arithmetic, float32 result) of the updates x [6N] = (w, dt) per node."""
    N = len(t)
    x = np.asarray(x, np.float64).reshape(N, 6)
    dR = rodrigues64(x[:, :3])
    dR[np.linalg.norm(x[:, :3], axis=1) == 0] = np.eye(3)   # a zero rotation update keeps R (the zero-rotation guard)
    Rn = np.asarray(R, np.float64).reshape(N, 3, 3) @ dR
    return Rn.astype(F32), (np.asarray(t, np.float64).reshape(N, 3) + x[:, 3:]).astype(F32)


def coupled_step(O, sc, depth, R, t, **kw):
    """One coupled GN step from (R, t): (R', t', system, updates)."""
    sysm = coupled_system(O, sc, depth, R, t, **kw)
    x, _ = solve_dense(sysm["diag"], sysm["pairs"], sysm["blocks"], sysm["rhs"])
    Rn, tn = apply_update(R, t, x)
    return Rn, tn, sysm, x


def block_diagonal_step(O, sc, depth, R, t, lm=0.001, **kw):
    """The reference's step from the same assembly: every node solves its own diagonal block."""
    d = data_system(O, sc, depth, R, t, **kw)
    N = len(t)
    Hd = d["Hfull"][np.arange(N), np.arange(N)] + lm * np.eye(6)
    x = np.stack([np.linalg.solve(Hd[n], d["g"].reshape(N, 6)[n]) for n in range(N)]).reshape(-1)
    Rn, tn = apply_update(R, t, x)
    return Rn, tn, d, x


def gt_translations_virtual(sc):
    h = sc.hierarchy
    return sc.gt_translations[h["virtual_indices"]] if h else sc.gt_translations
