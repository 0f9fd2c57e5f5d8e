"""Numpy restatement of the fitter's landmark term (nnrt_fitter_set_landmarks).

Given the node state (g, R, t; virtual order), the canonical vertices, their anchors and weights (fitter.anchors()), the
extrinsics and the landmarks, landmark_term returns the distances, the gate, the per-node H and g, the pair blocks and
the cost. dtype=np.float32 performs the kernel's float operations in the kernel's order (every product and sum rounded
to float32, the sums of products over associations in float64, in association order: ascending node, then landmark,
then slot); dtype=np.float64 is the same mathematics in double. Whole steps reuse tests/_coupled_util.py."""
import numpy as np

F32 = np.float32


def skew(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def _matvec(R, v, T):
    R, v = R.astype(T), v.astype(T)
    return np.array([T(T(R[r, 0] * v[0]) + T(R[r, 1] * v[1])) + T(R[r, 2] * v[2]) for r in range(3)], T)


def apply_extrinsics(E, p, T):
    if E is None:
        return p.astype(T)
    E = np.asarray(E, np.float64).astype(F32).astype(T)
    p = p.astype(T)
    return np.array([T(T(T(E[r, 0] * p[0]) + T(E[r, 1] * p[1])) + T(E[r, 2] * p[2])) + E[r, 3] for r in range(3)], T)


def warp_vertex(p, nodes, R, t, anchors, weights, E=None, T=F32):
    """The blended warp of one stored vertex: sum over its valid slots, in slot order, of w ((g + R (pc - g)) + t)."""
    pc = apply_extrinsics(E, np.asarray(p), T)
    out = np.zeros(3, T)
    for k, n in enumerate(anchors):
        if n < 0:
            continue
        g, w = nodes[n].astype(T), T(weights[k])
        Rd = _matvec(R[n], (pc - g).astype(T), T)
        out = (out + (w * ((g + Rd).astype(T) + t[n].astype(T)).astype(T)).astype(T)).astype(T)
    return out


def landmark_rows(p, g, Rn, w, coef, T=F32):
    """J [3, 6] of one (landmark, slot): row c = (coef e_c) x (-w R (p - g)) for the rotation, coef w e_c for the
    translation; p is the vertex as stored."""
    Rj = _matvec(Rn, (p.astype(T) - g.astype(T)).astype(T), T)
    jv = (-T(w) * Rj).astype(T)
    J = np.zeros((3, 6), T)
    for c in range(3):
        dv = np.zeros(3, T)
        dv[c] = T(coef)
        J[c, 0] = T(dv[1] * jv[2]) - T(dv[2] * jv[1])
        J[c, 1] = T(dv[2] * jv[0]) - T(dv[0] * jv[2])
        J[c, 2] = T(dv[0] * jv[1]) - T(dv[1] * jv[0])
        J[c, 3:] = (dv * T(w)).astype(T)
    return J


def gate(d, s, q, term_weight, cutoff, T=F32):
    """(active, dropped, rho) of one landmark with distance vector d."""
    d = d.astype(T)
    dist = np.sqrt(T(T(d[0] * d[0]) + T(d[1] * d[1])) + T(d[2] * d[2]))
    on = bool(s > 0) and bool(np.isfinite(q).all())
    with np.errstate(invalid="ignore"):
        within = cutoff <= 0 or bool(dist <= T(cutoff))
    coef = T(T(term_weight) * T(s)) if np.isfinite(s) else T(0)
    if on and within:
        r = (coef * d).astype(T).astype(np.float64)
        return True, False, float((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    if on:
        return False, True, float((float(coef) * float(T(cutoff))) ** 2)
    return False, False, 0.0


def landmark_term(points, nodes, R, t, anchors, weights, vertex_indices, targets, landmark_weights=None, term_weight=1.0, cutoff=0.0,
                  extrinsics=None, dtype=F32):
    """dict(d [L,3], active [L], dropped [L], H [N,6,6], g [N,6] (the negative gradient -J^T r), pairs {(i, j): [6,6]},
    i < j, block J_i^T J_j, cost, rows {(l, k): (node, J, r)})."""
    T = dtype
    nodes, R, t = np.asarray(nodes, F32), np.asarray(R, F32).reshape(-1, 3, 3), np.asarray(t, F32).reshape(-1, 3)
    N, L = len(nodes), len(vertex_indices)
    s_all = np.ones(L, F32) if landmark_weights is None else np.asarray(landmark_weights, F32)
    targets = np.asarray(targets, F32).reshape(L, 3)
    d, active, dropped, cost = np.zeros((L, 3), T), np.zeros(L, bool), np.zeros(L, bool), 0.0
    assoc = []
    rows = {}
    for l in range(L):
        v = int(vertex_indices[l])
        a, w = anchors[v], weights[v]
        d[l] = (warp_vertex(points[v], nodes, R, t, a, w, extrinsics, T) - targets[l].astype(T)).astype(T)
        active[l], dropped[l], rho = gate(d[l], s_all[l], targets[l], term_weight, cutoff, T)
        cost += rho
        if not active[l]:
            continue
        coef = T(T(term_weight) * T(s_all[l]))
        r = (coef * d[l]).astype(T)
        for k, n in enumerate(a):
            if n < 0:
                continue
            J = landmark_rows(np.asarray(points[v], F32), nodes[n], R[n], w[k], coef, T)
            rows[(l, k)] = (int(n), J, r)
            assoc.append((int(n), l, k))
    H, g, pairs = np.zeros((N, 6, 6)), np.zeros((N, 6)), {}
    for n, l, k in sorted(assoc):
        _, J, r = rows[(l, k)]
        J64, r64 = J.astype(np.float64), r.astype(np.float64)
        H[n] += J64.T @ J64
        g[n] -= J64.T @ r64
    for l in range(L):
        ks = sorted((rows[(ll, k)][0], k) for (ll, k) in rows if ll == l)
        for x in range(len(ks)):
            for y in range(x + 1, len(ks)):
                (i, ka), (j, kb) = ks[x], ks[y]
                if i == j:
                    continue
                pairs.setdefault((i, j), np.zeros((6, 6)))
                pairs[(i, j)] += rows[(l, ka)][1].astype(np.float64).T @ rows[(l, kb)][1].astype(np.float64)
    return dict(d=d, active=active, dropped=dropped, H=H, g=g, pairs=pairs, cost=cost, rows=rows)


def residual64(points, nodes, R, t, anchors, weights, vertex_indices, targets, landmark_weights, term_weight, x=None):
    """The stacked float64 residual [3 L] at the state perturbed by x [6 N] = (w, dt) per node, the perturbation the data
    and ARAP rows share: R <- Rodrigues(w) R about the node (the warped offset R (v - g) rotates), t <- t + dt."""
    nodes, R, t = np.asarray(nodes, np.float64), np.asarray(R, np.float64).reshape(-1, 3, 3), np.asarray(t, np.float64).reshape(-1, 3)
    N = len(nodes)
    x = np.zeros((N, 6)) if x is None else np.asarray(x, np.float64).reshape(N, 6)
    out = []
    for l, v in enumerate(vertex_indices):
        p = np.asarray(points[v], np.float64)
        wp = np.zeros(3)
        for k, n in enumerate(anchors[v]):
            if n < 0:
                continue
            wp += float(weights[v][k]) * (nodes[n] + _rodrigues(x[n, :3]) @ (R[n] @ (p - nodes[n])) + t[n] + x[n, 3:])
        s = 1.0 if landmark_weights is None else float(landmark_weights[l])
        out.append(term_weight * s * (wp - np.asarray(targets[l], np.float64)))
    return np.concatenate(out)


def _rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    K = skew(w / th)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def dense_jacobian(term, L, N):
    """[3 L, 6 N] from landmark_term's rows."""
    J = np.zeros((3 * L, 6 * N))
    for (l, k), (n, Jn, _) in term["rows"].items():
        J[3 * l:3 * l + 3, 6 * n:6 * n + 6] += Jn.astype(np.float64)
    return J


def add_to_system(sysm, term):
    """A _coupled_util.coupled_system dict with the landmark term added (its pairs must be in the system's pair list)."""
    diag, blocks, rhs = sysm["diag"].copy(), np.array(sysm["blocks"], np.float64), sysm["rhs"].copy()
    diag += term["H"]
    rhs += term["g"].reshape(-1)
    index = {tuple(p): m for m, p in enumerate(np.asarray(sysm["pairs"]).reshape(-1, 2).tolist())}
    for ij, b in term["pairs"].items():
        blocks[index[ij]] += b
    return dict(sysm, diag=diag, blocks=blocks, rhs=rhs)
