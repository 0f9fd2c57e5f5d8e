"""Expected values for the fitter's robust options (nnrt_fitter_set_robust_options), assembled from the CPU oracle's
existing stage functions in the order its own FitToImage loop (orc_fit) calls them. The re-weighting itself is restated
here in float32 numpy, one IEEE operation at a time and in the documented expression order, so it matches the kernels'
arithmetic (no contraction, correctly rounded divide and sqrt):

* data term, Tukey biweight: r = n_l . d, contributes = mask and |r| <= c, q = r / c, s = 1 - q q; the point-map vectors
  d and the rasterized normals n_l go into pixel_vertex_anchor_jacobians multiplied by s, the residuals into
  data_hessian_gradient as s r, both with the contributing mask;
* ARAP term, Huber on the edge's 3-vector: n = sqrt((r0 r0 + r1 r1) + r2 r2), s = 1 if n <= delta else sqrt(delta / n);
  the square-penalty residuals and the edge Jacobians are multiplied by s before arap_hessian / arap_gradient.
"""
import numpy as np

F32 = np.float32


def virtual_nodes(sc):
    h = sc.hierarchy
    return sc.nodes[h["virtual_indices"]] if h else sc.nodes


def identity_motion(N):
    return np.tile(np.eye(3, dtype=F32), (N, 1, 1)), np.zeros((N, 3), F32)


def data_term(O, sc, depth, R=None, t=None, mode="ALL", anchor_count=4, tukey_c=None, lm=0.001):
    """One iteration's data term from node motion (R, t) (virtual order; default the identity): the diagnostics
    oracle.fit reports (pixel_faces, residual_mask, residuals, hessian_diag, gradient, updates of the block-diagonal
    solve, status) plus `r` (the signed distances, 0 outside the mask), `contributes` and `s`. tukey_c None: the
    square penalty (s = 1, every masked pixel contributes)."""
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
    pj, pc = O.pixel_vertex_anchor_jacobians(rvj, rnj, w if mode == "TRANSLATION_ONLY" else vj, nj, (pmv * s[:, None]).astype(F32),
                                             (rnorm * s[:, None]).astype(F32), contributes, fi, sc.faces, fnodes, fslots, fcounts,
                                             False, 0.01, mode)
    Hd, g = O.data_hessian_gradient(pj, pc, fi, fnodes, residuals, contributes, N, mode)
    x, rc = O.solve_block_diagonal(Hd, g, lm)
    return dict(pixel_faces=fi.reshape(P).astype(np.int64), residual_mask=mask, residuals=residuals, hessian_diag=Hd.reshape(-1),
                gradient=g, updates=x, status=rc, r=r, contributes=contributes, s=s)


def huber_scale(res3, delta):
    """The IRLS Huber factor per edge, float32: sqrt of min(1, delta / |r|)."""
    r = np.ascontiguousarray(res3, F32).reshape(-1, 3)
    n = np.sqrt(((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]).astype(F32)).astype(F32)
    with np.errstate(divide="ignore"):
        big = np.sqrt((F32(delta) / n).astype(F32)).astype(F32)
    return np.where(n <= F32(delta), F32(1.0), big).astype(F32), n


def arap_term(O, sc, R, t, weight=200.0, huber_delta=None):
    """The ARAP term at node motion (R, t) (virtual order): diagonal blocks [N,6,6] (ARAP part only), wing blocks
    [E,6,6], the ARAP part of the negative gradient [6N], the (scaled) edge residuals [E,3], and the unscaled edge
    residual norms. huber_delta None: the square penalty."""
    h = sc.hierarchy
    nodes = virtual_nodes(sc)
    N = len(nodes)
    edges = np.asarray(h["edges"], np.int32)
    R = np.ascontiguousarray(R, F32).reshape(N, 3, 3)
    t = np.ascontiguousarray(t, F32).reshape(N, 3)
    res = O.arap_residuals(edges, h["edge_layers"], h["radii"], h.get("node_weights"), nodes, R, t, weight, False).reshape(-1, 3)
    ej = O.arap_edge_jacobians(edges, h["edge_layers"], h["radii"], h.get("node_weights"), nodes, R, weight)
    s, norms = huber_scale(res, np.inf if huber_delta is None else huber_delta)
    res = (res * s[:, None]).astype(F32)
    ej = (ej * s[:, None]).astype(F32)
    adiag, wing = O.arap_hessian(edges, ej, N)
    g = O.arap_gradient(edges, ej, res.reshape(-1), np.zeros(6 * N, F32))
    return dict(diag=adiag, wing=wing, gradient=g, residuals=res, norms=norms, s=s)


def patch_targets(depth, size=12, push=0.5):
    """Target A: a size x size patch of valid pixels pushed `push` m back; target B: the same patch set to depth 0
    (invalid). Returns (A, B, patch mask)."""
    H, W = depth.shape
    valid = depth > 0
    v0, u0 = None, None
    for v in range(H // 2 - size // 2, H - size):
        for u in range(W // 2 - size // 2, W - size):
            if valid[v:v + size, u:u + size].all():
                v0, u0 = v, u
                break
        if v0 is not None:
            break
    assert v0 is not None, "no fully valid patch in the target depth"
    patch = np.zeros_like(valid)
    patch[v0:v0 + size, u0:u0 + size] = True
    A = depth.copy()
    A[patch] += F32(push)
    B = depth.copy()
    B[patch] = 0.0
    return A, B, patch
