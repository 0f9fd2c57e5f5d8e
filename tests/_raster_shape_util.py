"""Inputs for the rasterizer / fused-fit tests at portrait, odd and thin image sizes, and a numpy restatement of the
scatter's branch conditions.

shape_soup: a face soup in NDC built for an image size -- a coherent patch (what lets a wave stage its tile), a random
soup hanging off every edge, and a handful of special faces (whole-image, degenerate, tied, non-finite).
branch_census: which branch of csrc/raster.hip each face and each wave of such a soup takes, restated in float32 numpy
from the comments and formulas of raster.hip and common.hpp. It calls neither the oracle nor the library: it is a
statement about the inputs, so a test can show that a size reaches the code it is there for.
shape_scene: a synthetic.Scene at a chosen image size.
"""
import numpy as np

from dynamicfuion_python_amd import synthetic

F32 = np.float32
K_EPSILON = F32(1e-8)          # common.hpp
FACES_PER_WAVE = 32            # raster.hip SCATTER_FPW (lane-pair and NDC paths)
TILE_KEYS = 512                # raster.hip SCATTER_TILE_KEYS
DENSE_FACES_PER_WAVE = 64      # raster.hip DENSE_FPW
DENSE_TILE_KEYS = 256          # raster.hip DENSE_TILE_KEYS
DEAL_ROUND = 64                # raster.hip scatter_rows: one row per lane per round

# image sizes of the standalone rasterizer tests and what each is there to reach
RASTER_SIZES = [(1, 1), (1, 7), (7, 1), (37, 53), (53, 37), (65, 63), (63, 65), (17, 129), (129, 17), (3, 200), (200, 3), (107, 75)]
# (blur in pixels, perspective-correct, clip barycentrics) of the K = 1 runs; the K > 1 runs use the first
RASTER_OPTIONS = [(0.5, True, False), (0.0, False, False), (0.5, True, True)]
# fused-iteration scenes: (H, W, fx)
FIT_SHAPES = [(53, 37, 45.0), (37, 53, 45.0), (107, 75, 90.0), (17, 129, 30.0), (129, 17, 30.0), (33, 47, 40.0)]


def ndc_range(d1, d2):
    """common.hpp ndc_range: 2 along the short axis, 2 d1 / d2 along the long one (float32)."""
    r = F32(2.0)
    if d1 > d2:
        r = (F32(d1) * r) / F32(d2)
    return r


def pixel_centres(d1, d2):
    """common.hpp pixel_to_ndc(i, d1, d2) for i = 0 .. d1 - 1, in float32 and its expression order."""
    r = ndc_range(d1, d2)
    off = r / F32(2.0)
    i = np.arange(d1, dtype=np.float32)
    return (-off + (r * i + off) / F32(d1)).astype(np.float32)


def blur_ndc(blur_px, H, W):
    """capi.hip / fitter.hip: blur_px / (min(H, W) / 2) in float32"""
    return F32(blur_px) / (F32(min(H, W)) / F32(2.0))


def near_all_side(H, W, blur_px):
    """Largest box side s (square box, NDC) at which near_all holds: 2 (s + 2 b)^2 < b / 2. <= 0: no face can be near_all
    at this size (8 b^2 >= b / 2, i.e. min(H, W) <= 16 blur_px)."""
    b = float(blur_ndc(blur_px, H, W))
    return float(np.sqrt(0.25 * b) - 2.0 * b) if b > 0 else 0.0


def _front(tri):
    """tri [n,3,3] with every face front-facing (clockwise area > 0 under spa_cw): swap two vertices where not"""
    tri = np.array(tri, np.float64)
    a = (tri[:, 0, 0] - tri[:, 1, 0]) * (tri[:, 1, 1] - tri[:, 2, 1]) - (tri[:, 0, 1] - tri[:, 1, 1]) * (tri[:, 1, 0] - tri[:, 2, 0])
    back = a < 0
    tri[back] = tri[back][:, [0, 2, 1]]
    return tri


def _block_patch(x0, x1, y0, y1, bx, by, z):
    """Front-facing grid of 4 bx x 4 by cells (two triangles each) over [x0, x1] x [y0, y1], laid out block by block
    (row-major blocks of 4 x 4 cells = 32 consecutive faces covering a small box)."""
    xs = np.linspace(x0, x1, 4 * bx + 1)
    ys = np.linspace(y0, y1, 4 * by + 1)
    out = []
    for j in range(by):
        for i in range(bx):
            for cj in range(4 * j, 4 * j + 4):
                for ci in range(4 * i, 4 * i + 4):
                    a, b, c, d = (xs[ci], ys[cj]), (xs[ci + 1], ys[cj]), (xs[ci], ys[cj + 1]), (xs[ci + 1], ys[cj + 1])
                    out.append([a + (z,), b + (z,), c + (z,)])
                    out.append([b + (z,), d + (z,), c + (z,)])
    return _front(np.array(out, np.float64))


def shape_soup(H, W, seed=0, blur_px=0.5):
    """(face_ndc [F,3,3] float32, mask [F] uint8) for an H x W image: coherent patch, random soup, specials, in that order
    (see the module docstring). `blur_px` only sizes the faces meant to be near_all (their box far below the blur
    radius); the soup is the same for every option set of a size. F is no multiple of 128."""
    rng = np.random.default_rng(1000 * H + W + 7919 * seed)
    rx, ry = max(W / H, 1.0), max(H / W, 1.0)          # half extents of the image rectangle in NDC
    px = 2.0 / min(H, W)                                # one pixel in NDC
    short = min(H, W)
    s_max = near_all_side(H, W, blur_px)

    # -- coherent patch: blocks of about 6 x 6 pixels over the central 60 % of the image, depth 2
    bx = int(np.clip(round(0.6 * W / 6.0), 1, 5))
    by = int(np.clip(round(0.6 * H / 6.0), 1, 5))
    parts = [_block_patch(-0.6 * rx, 0.6 * rx, -0.6 * ry, 0.6 * ry, bx, by, 2.0)]
    # a fine patch of faces small enough to be near_all (two blocks side by side), depth 1.5
    if s_max > 0:
        c = 0.6 * s_max
        parts.append(_block_patch(0.3 * rx, 0.3 * rx + 8 * c, 0.3 * ry, 0.3 * ry + 4 * c, 2, 1, 1.5))

    # -- random soup: centres over the image rectangle extended by 10 %, sizes log-uniform 0.1 px .. short / 3 px (at
    # least 4 px, so that the faces of a thin image still cross several pixel centres)
    n = 480
    cx = rng.uniform(-1.1 * rx, 1.1 * rx, n)
    cy = rng.uniform(-1.1 * ry, 1.1 * ry, n)
    size = px * np.exp(rng.uniform(np.log(0.1), np.log(max(short / 3.0, 4.0)), n))
    # every fourth face small enough to be near_all; every second of those at a depth beyond face_rows_fast's range
    tiny = (np.arange(n) % 4 == 0) & (s_max > 0)
    size = np.where(tiny, s_max * rng.uniform(0.25, 0.7, n), size)
    ang = rng.uniform(0, 2 * np.pi, (n, 1)) + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.4, 0.4, (n, 3))
    rad = 0.5 * size[:, None] * rng.uniform(0.7, 1.0, (n, 3))
    soup = np.empty((n, 3, 3))
    soup[:, :, 0] = cx[:, None] + rad * np.cos(ang)
    soup[:, :, 1] = cy[:, None] + rad * np.sin(ang)
    soup[:, :, 2] = rng.uniform(0.5, 3.0, (n, 3))
    far = tiny & (np.arange(n) % 8 == 0)
    # (one depth per far face: with three different depths of 1e10 the perspective denominator can cancel to K_EPSILON at
    # a pixel far outside a tiny face, and the depth becomes inf - inf on every implementation)
    soup[far, :, 2] = 2e10 * rng.uniform(1.0, 1.5, (int(far.sum()), 1))
    flip = rng.uniform(0, 1, n) < 0.5                   # both windings
    soup[flip] = soup[flip][:, [0, 2, 1]]
    soup[tiny] = _front(soup[tiny])                     # the tiny faces all render
    parts.append(soup)

    # -- 64 consecutive slivers, each as tall as the image: whatever the alignment, one wave of 32 holds only such faces
    # and deals min(H, ...) rows for each, i.e. more than one round of 64 rows from H = 3 on. Depth 2.5.
    tx = np.linspace(-0.95 * rx, 0.95 * rx, 64)
    tall = np.empty((64, 3, 3))
    tall[:, 0] = np.stack([tx - 0.8 * px, np.full(64, -1.2 * ry), np.full(64, 2.5)], 1)
    tall[:, 1] = np.stack([tx + 0.8 * px, np.full(64, -1.2 * ry), np.full(64, 2.5)], 1)
    tall[:, 2] = np.stack([tx, np.full(64, 1.2 * ry), np.full(64, 2.5)], 1)
    parts.append(_front(tall))

    # -- specials
    xc, yc = pixel_centres(W, H), pixel_centres(H, W)
    m = max(0.35 * min(rx, ry), 2.2 * px)
    sp = [
        _front([[(-4 * rx, -4 * ry, 2.9), (4 * rx, -4 * ry, 2.9), (0.0, 8 * ry, 2.9)]])[0],             # covers the whole image
        np.array([(0.0, 0.0, 1.0), (0.0, 0.0, 1.0), (0.1, 0.1, 1.0)]),                               # zero area
        _front([[(-m, -m, 1e-9), (m, -m, 0.0), (0.0, m, -1.0)]])[0],                                 # every z below K_EPSILON
        # its box ends exactly on the centres of the last pixel column and row
        _front([[(float(xc[-1]) - 3 * px, float(yc[-1]) - 3 * px, 1.2), (float(xc[-1]), float(yc[-1]) - 3 * px, 1.2),
                 (float(xc[-1]) - 1.5 * px, float(yc[-1]), 1.2)]])[0],
        _front([[(-m, -m, 1.0), (m, -m, 1.0), (0.0, m, 1.0)]])[0],                                   # two coincident faces, equal depth:
        _front([[(-m, -m, 1.0), (m, -m, 1.0), (0.0, m, 1.0)]])[0],                                   # the lower index wins the tie
        _front([[(-0.8 * m, -0.8 * m, 0.6), (0.8 * m, -0.8 * m, 0.7), (0.0, 0.8 * m, 0.65)]])[0],    # nearer, later: replaces a queue entry
        _front([[(5 * rx, 5 * ry, 1.0), (5.2 * rx, 5 * ry, 1.0), (5.1 * rx, 5.2 * ry, 1.0)]])[0],    # wholly off the image
    ]
    bad = [_front([[(-m, -m, 0.4), (m, -m, 0.4), (0.0, m, 0.4)]])[0] for _ in range(4)]          # nearest of all, were they drawn
    bad[0][0, 0] = np.nan
    bad[1][2, 2] = np.inf
    bad[2][1, 1] = -np.inf
    bad[3][:, 2] = np.nan
    parts.append(np.array(sp + bad))

    face_ndc = np.concatenate(parts).astype(np.float32)
    F = len(face_ndc)
    if F % 128 == 0:
        face_ndc = np.concatenate([face_ndc, face_ndc[-9:-8]])   # (a second wholly-off face)
        F += 1
    mask = (rng.uniform(0, 1, F) >= 0.1).astype(np.uint8)
    mask[F - len(sp) - len(bad):] = 1                   # the specials stay in
    return face_ndc, mask


def _max3(a):
    return np.maximum(np.maximum(a[:, 0], a[:, 1]), a[:, 2])


def _min3(a):
    return np.minimum(np.minimum(a[:, 0], a[:, 1]), a[:, 2])


def branch_census(face_ndc, mask, H, W, blur_px, clip, cull=True):
    """Counts of the branches raster.hip takes on these faces at this image size and these options (see the module
    docstring): dict with `mode` [3] (faces per scatter_row mode: 0 full test, 1 near_all on guarded quotients, 2 near_all
    on the fast path), `rejected` {cause: faces}, `drawn` (faces with a non-empty pixel range), and per grouping g in
    (32, 64): `staged{g}`, `unstaged{g}` (waves whose box is within / beyond the wave's LDS tile), `multi_round{g}` (waves
    with more than 64 face rows), `empty{g}` (waves none of whose faces covers a pixel)."""
    f = np.ascontiguousarray(face_ndc, np.float32).reshape(-1, 3, 3)
    F = len(f)
    x, y, z = f[:, :, 0], f[:, :, 1], f[:, :, 2]
    blur = blur_ndc(blur_px, H, W)
    with np.errstate(invalid="ignore", over="ignore"):
        # face_finite: the sum of the nine coordinates in the kernel's order
        s = ((x[:, 0] + x[:, 1]) + (x[:, 2] + y[:, 0])) + ((y[:, 1] + y[:, 2]) + (z[:, 0] + z[:, 1])) + z[:, 2]
        finite = np.isfinite(s)
        # spa_cw(v0, v1, v2) = (x0 - x1) (y1 - y2) - (y0 - y1) (x1 - x2)
        area = (x[:, 0] - x[:, 1]) * (y[:, 1] - y[:, 2]) - (y[:, 0] - y[:, 1]) * (x[:, 1] - x[:, 2])
        back = area < 0
        zero_area = (area <= K_EPSILON) & (area >= F32(-1.0) * K_EPSILON)
        zinv = _max3(z) < K_EPSILON
        xlo, xhi = _min3(x), _max3(x)
        ylo, yhi = _min3(y), _max3(y)
        xmin, xmax, ymin, ymax = xlo - blur, xhi + blur, ylo - blur, yhi + blur
        # exact pixel ranges: first centre >= lo, last centre <= hi (pixel_first / pixel_last)
        xc, yc = pixel_centres(W, H), pixel_centres(H, W)
        u0 = np.searchsorted(xc, np.nan_to_num(xmin), side="left")
        u1 = np.searchsorted(xc, np.nan_to_num(xmax), side="right") - 1
        v0 = np.searchsorted(yc, np.nan_to_num(ymin), side="left")
        v1 = np.searchsorted(yc, np.nan_to_num(ymax), side="right") - 1
        bw = (xhi - xlo) + F32(2.0) * blur
        bh = (yhi - ylo) + F32(2.0) * blur
        near_all = (bw * bw + bh * bh) < F32(0.5) * blur
        A = area + K_EPSILON
        fast = (not clip) & (blur < F32(1e20)) & (np.abs(A) > F32(1e-30)) & (np.abs(A) < F32(1e30)) & (_max3(np.abs(z)) < F32(1e10))
    assert bw.dtype == np.float32 and area.dtype == np.float32 and xc.dtype == np.float32
    masked = np.zeros(F, bool) if mask is None else (np.asarray(mask).reshape(-1) == 0)
    # the causes in the kernel's order; each face is counted under the first that rejects it
    causes = [("masked", masked), ("non_finite", ~finite), ("back_facing", back & bool(cull)), ("zero_area", zero_area),
              ("z_behind", zinv), ("off_image", (u0 > u1) | (v0 > v1))]
    ok = np.ones(F, bool)
    rejected = {}
    for name, c in causes:
        rejected[name] = int((ok & c).sum())
        ok &= ~c
    mode = np.where(~near_all, 0, np.where(fast, 2, 1))
    out = {"faces": F, "drawn": int(ok.sum()), "rejected": rejected, "mode": [int((ok & (mode == m)).sum()) for m in range(3)],
           "box_pixels": int(((u1 - u0 + 1) * (v1 - v0 + 1))[ok].sum())}
    rows = np.where(ok, v1 - v0 + 1, 0)
    for g, keys in ((FACES_PER_WAVE, TILE_KEYS), (DENSE_FACES_PER_WAVE, DENSE_TILE_KEYS)):
        staged = unstaged = multi = empty = 0
        for b in range(0, F, g):
            sel = ok[b:b + g]
            if not sel.any():
                empty += 1
                continue
            tw = int(u1[b:b + g][sel].max() - u0[b:b + g][sel].min() + 1)
            th = int(v1[b:b + g][sel].max() - v0[b:b + g][sel].min() + 1)
            if tw * th <= keys:
                staged += 1
            else:
                unstaged += 1
            multi += int(rows[b:b + g].sum() > DEAL_ROUND)
        out.update({f"staged{g}": staged, f"unstaged{g}": unstaged, f"multi_round{g}": multi, f"empty{g}": empty})
    return out


def shape_scene(H, W, fx, seed=0, mesh=(49, 37), node_dims=(6, 4), coverage=0.25, layer_count=1, iterations=2):
    """A synthetic.Scene at image size H x W with focal length fx (principal point at the image centre), built as
    synthetic.make_scene builds its single-layer scenes: S1's mesh, nodes and coverage by default."""
    K = np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], np.float64)
    points, normals, faces = synthetic.grid_mesh(*mesh)
    nodes, uv = synthetic.node_grid(*node_dims, seed=seed)
    w, t = synthetic.ground_truth_motion(uv, seed=seed)
    return synthetic.Scene(f"{H}x{W}", H, W, K, points, normals, faces, nodes, coverage, layer_count, iterations, synthetic.rodrigues_np(w), t,
                           {}, w)
