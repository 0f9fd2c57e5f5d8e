"""The landmark term's restatement (tests/_landmark_util.py) on the CPU: its Jacobian against
central differences of its own float64 residual, the gate and the cost, the two precisions against each other, and
landmarks_from_pixel_matches on a hand-made raster."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _landmark_util as LU   # noqa: E402

F32 = np.float32


def _problem(seed=3):
    """3 nodes, 6 vertices with 4 anchor slots each (some empty), a non-identity state, 5 landmarks (two on one vertex)."""
    rng = np.random.default_rng(seed)
    nodes = np.array([[0.0, 0.0, 1.0], [0.3, 0.05, 1.1], [-0.2, 0.25, 0.9]], F32)
    points = (nodes[rng.integers(0, 3, 6)] + rng.normal(0, 0.08, (6, 3))).astype(F32)
    anchors = np.array([[0, 1, 2, -1], [1, 0, -1, -1], [2, 1, 0, -1], [0, -1, -1, -1], [1, 2, -1, -1], [2, 0, 1, -1]], np.int32)
    weights = np.where(anchors >= 0, rng.uniform(0.2, 1.0, anchors.shape), 0).astype(F32)
    weights = (weights / weights.sum(axis=1, keepdims=True)).astype(F32)
    R = np.stack([LU._rodrigues(w) for w in rng.normal(0, 0.2, (3, 3))]).astype(F32)
    t = rng.normal(0, 0.03, (3, 3)).astype(F32)
    idx = np.array([0, 2, 2, 4, 5], np.int32)
    targets = (points[idx] + rng.normal(0, 0.02, (5, 3))).astype(F32)
    s = np.array([1.0, 0.5, 2.0, 1.0, 0.25], F32)
    return dict(points=points, nodes=nodes, R=R, t=t, anchors=anchors, weights=weights, idx=idx, targets=targets, s=s)


def _term(p, dtype, **kw):
    return LU.landmark_term(p["points"], p["nodes"], p["R"], p["t"], p["anchors"], p["weights"], p["idx"], p["targets"],
                            kw.pop("s", p["s"]), dtype=dtype, **kw)


def test_jacobian_matches_central_differences():
    p = _problem()
    wL = 1.7
    term = _term(p, np.float64, term_weight=wL)
    N, L = len(p["nodes"]), len(p["idx"])
    J = LU.dense_jacobian(term, L, N)

    def res(x):
        return LU.residual64(p["points"], p["nodes"], p["R"], p["t"], p["anchors"], p["weights"], p["idx"], p["targets"], p["s"], wL, x)

    r0 = res(None)
    stacked = np.concatenate([term["rows"][(l, min(k for (ll, k) in term["rows"] if ll == l))][2] for l in range(L)])
    assert np.allclose(stacked, r0, rtol=1e-12, atol=1e-14)
    h = 1e-4
    Jn = np.zeros_like(J)
    for q in range(6 * N):
        e = np.zeros(6 * N)
        e[q] = h
        Jn[:, q] = (res(e) - res(-e)) / (2 * h)
    err = np.abs(J - Jn).max() / np.abs(Jn).max()
    print(f"landmark Jacobian against central differences at h = {h:g}: {err:.3g} of max |J|")
    assert err < 1e-6
    # H, g and the pair blocks are that Jacobian's normal equations
    Hd = J.T @ J
    g = -J.T @ r0
    for n in range(N):
        assert np.allclose(term["H"][n], Hd[6 * n:6 * n + 6, 6 * n:6 * n + 6], rtol=1e-12, atol=1e-15)
    assert np.allclose(term["g"].reshape(-1), g, rtol=1e-12, atol=1e-15)
    assert set(term["pairs"]) == {(0, 1), (0, 2), (1, 2)}
    for (i, j), b in term["pairs"].items():
        assert np.allclose(b, Hd[6 * i:6 * i + 6, 6 * j:6 * j + 6], rtol=1e-12, atol=1e-15)
    assert np.isclose(term["cost"], float(r0 @ r0), rtol=1e-12)


def test_float32_order_agrees_with_float64():
    p = _problem()
    a, b = _term(p, F32, term_weight=1.7), _term(p, np.float64, term_weight=1.7)
    scale = np.abs(b["H"]).max()
    assert np.abs(a["H"] - b["H"]).max() < 1e-5 * scale
    assert np.abs(a["g"] - b["g"]).max() < 1e-5 * max(np.abs(b["g"]).max(), scale)
    assert abs(a["cost"] - b["cost"]) < 1e-5 * b["cost"]
    assert a["d"].dtype == F32 and np.abs(a["d"] - b["d"]).max() < 1e-6


@pytest.mark.parametrize("dtype", [F32, np.float64])
def test_gate_and_cost(dtype):
    p = _problem()
    wL = 2.0
    full = _term(p, dtype, term_weight=wL)
    dist = np.linalg.norm(full["d"].astype(np.float64), axis=1)
    cutoff = float(np.sort(dist)[-2] + np.sort(dist)[-1]) / 2   # drops the farthest landmark only
    far = int(np.argmax(dist))
    s = p["s"].copy()
    off = (far + 1) % 5
    s[off] = 0.0
    targets = p["targets"].copy()
    nan = (far + 2) % 5
    targets[nan, 1] = np.nan
    q = dict(p, targets=targets)
    term = _term(q, dtype, s=s, term_weight=wL, cutoff=cutoff)
    want_active = np.ones(5, bool)
    want_active[[far, off, nan]] = False
    assert np.array_equal(term["active"], want_active)
    assert np.array_equal(term["dropped"], np.arange(5) == far)
    # the cost: |r|^2 of the active ones, (w_L s cutoff)^2 of the dropped one, nothing of the two that are off
    cost = sum(float(((wL * s[l] * full["d"][l].astype(np.float64)) ** 2).sum()) for l in np.nonzero(want_active)[0])
    cost += (wL * float(s[far]) * cutoff) ** 2
    assert np.isclose(term["cost"], cost, rtol=1e-5)
    # an inactive landmark contributes no rows
    assert {l for (l, _) in term["rows"]} == set(np.nonzero(want_active)[0].tolist())
    # cutoff <= 0: no cutoff; the same sums as the active landmarks alone
    assert _term(p, dtype, term_weight=wL, cutoff=0.0)["active"].all() and _term(p, dtype, term_weight=wL, cutoff=-1.0)["active"].all()
    only = np.nonzero(want_active)[0]
    alone = LU.landmark_term(p["points"], p["nodes"], p["R"], p["t"], p["anchors"], p["weights"], p["idx"][only], p["targets"][only], s[only],
                             term_weight=wL, dtype=dtype)
    assert np.array_equal(alone["H"], term["H"]) and np.array_equal(alone["g"], term["g"])


def test_landmarks_from_pixel_matches():
    from dynamicfuion_python_amd.nnrt.alignment import landmarks_from_pixel_matches
    # a 2 x 2 render of two faces: pixel (v, u) = (0, 0) and (0, 1) see face 0, (1, 0) sees face 1, (1, 1) is background
    faces = torch.tensor([[0, 0], [1, -1]])
    bary = torch.tensor([[[0.2, 0.7, 0.1], [0.6, 0.3, 0.1]], [[0.1, 0.1, 0.8], [0.0, 0.0, 0.0]]])
    tri = torch.tensor([[10, 11, 12], [12, 11, 13]])
    points = torch.tensor([[[0.0, 0.0, 1.0], [0.1, 0.0, 1.1]], [[0.0, 0.1, 0.0], [float("nan"), 0.1, 1.3]]])
    source = torch.tensor([[0, 0], [1, 0], [0, 1], [1, 1], [0, 0], [0, 0], [5, 0]])   # (u, v)
    target = torch.tensor([[1, 0], [0, 0], [1, 0], [0, 0], [0, 1], [1, 1], [0, 0]])
    w = torch.arange(7, dtype=torch.float32) + 1
    idx, q, ws = landmarks_from_pixel_matches(faces, bary, tri, source, target, points, w)
    # match 3: background source; 4: target z = 0; 5: NaN target; 6: source off the render
    assert idx.dtype == torch.int32 and idx.tolist() == [11, 10, 13]
    assert torch.equal(q, torch.tensor([[0.1, 0.0, 1.1], [0.0, 0.0, 1.0], [0.1, 0.0, 1.1]]))
    assert ws.tolist() == [1.0, 2.0, 3.0]
    idx2, q2, none = landmarks_from_pixel_matches(faces[..., None], bary[:, :, None, :], tri, source, target, points)
    assert none is None and torch.equal(idx2, idx) and torch.equal(q2, q)
    empty = landmarks_from_pixel_matches(faces, bary, tri, source[3:4], target[3:4], points)
    assert len(empty[0]) == 0 and empty[1].shape == (0, 3)
