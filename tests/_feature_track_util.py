"""Numpy restatement of the sparse feature tracker (include/nnrt_mi355x.h: nnrt_corner_scores, nnrt_select_features,
nnrt_track_features), following the header's order: float32 where it says float, float64 where it
says float64. The float64 sums run in row-major order over the window (the kernel's lane partials and butterfly differ
from that in the last bits of a float64 only). track() also returns, per feature, how far each of its decisions lay from
its threshold, which tests/test_feature_track_cpu.py holds to a margin so that the GPU tests can demand equal status.

The input sets of the GPU tests are built here (track_case, special_case), by a fixed seed and, where a random point would
sit close to a decision, by drawing another: both test files see the same sets."""
import functools

import numpy as np

F32 = np.float32
TRACKED, OUT_OF_IMAGE, FLAT, RESIDUAL, NON_FINITE, FB_FAILED = range(6)
EDGE_MARGIN, RELATIVE_MARGIN = 0.25, 0.10   # pixels of the level; share of the threshold


# ---- images ---------------------------------------------------------------------------------------------------------------
def _f(x, y):
    """A smooth texture in (0, 1): two strong sinusoids of wavelengths about 7 pixels, which a shift of half of that takes
    out of a single-level tracker's reach, and three weaker, longer ones that survive the pyramid's upper levels."""
    two_pi = 2.0 * np.pi
    return (0.5 + 0.10 * np.sin(two_pi * (x / 9.3 + y / 13.1) + 0.3) + 0.10 * np.sin(two_pi * (x / 11.7 - y / 8.3) + 1.1)
            + 0.06 * np.sin(two_pi * (x / 37.0 + y / 53.0) + 2.0) + 0.06 * np.sin(two_pi * (-x / 45.0 + y / 31.0) + 0.7)
            + 0.04 * np.sin(two_pi * (x / 19.0 + y / 23.0) + 1.7))


def texture(W, H, shift=(0.0, 0.0), angle=0.0):
    """float32 [H, W]: the texture moved by `shift` pixels and turned by `angle` about the image centre, so that what
    texture(W, H) shows at p it shows at motion(p)."""
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    dx, dy = x - shift[0] - cx, y - shift[1] - cy
    c, s = np.cos(angle), np.sin(angle)
    return _f(cx + c * dx + s * dy, cy - s * dx + c * dy).astype(F32)


def motion(points, W, H, shift=(0.0, 0.0), angle=0.0):
    p = np.asarray(points, np.float64)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    c, s = np.cos(angle), np.sin(angle)
    dx, dy = p[:, 0] - cx, p[:, 1] - cy
    return np.stack([cx + c * dx - s * dy + shift[0], cy + s * dx + c * dy + shift[1]], axis=1)


def halve(img):
    """nnrt_intensity_halve in float32."""
    img = np.asarray(img, F32)
    H, W = img.shape
    ys, xs = 2 * np.arange((H + 1) // 2), 2 * np.arange((W + 1) // 2)
    x0, x2 = np.maximum(xs - 1, 0), np.minimum(xs + 1, W - 1)
    y0, y2 = np.maximum(ys - 1, 0), np.minimum(ys + 1, H - 1)
    h = ((img[:, x0] + F32(2) * img[:, xs]) + img[:, x2]) * F32(0.25)
    return ((h[y0] + F32(2) * h[ys]) + h[y2]) * F32(0.25)


def pyramid(img, levels):
    out = [np.ascontiguousarray(img, F32)]
    for _ in range(levels - 1):
        out.append(np.ascontiguousarray(halve(out[-1])))
    return out


# ---- scores and selection ---------------------------------------------------------------------------------------------------
def corner_scores(img, r):
    img = np.asarray(img, F32)
    H, W = img.shape
    out = np.zeros((H, W), F32)
    h, w = H - 2 * r - 2, W - 2 * r - 2   # scored pixels
    if h <= 0 or w <= 0:
        return out
    ix, iy = np.zeros((H, W), F32), np.zeros((H, W), F32)
    ix[:, 1:-1] = F32(0.5) * (img[:, 2:] - img[:, :-2])
    iy[1:-1, :] = F32(0.5) * (img[2:, :] - img[:-2, :])
    ix, iy = ix.astype(np.float64), iy.astype(np.float64)
    a, b, c = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
    for j in range(2 * r + 1):
        for i in range(2 * r + 1):
            gx, gy = ix[1 + j:1 + j + h, 1 + i:1 + i + w], iy[1 + j:1 + j + h, 1 + i:1 + i + w]
            a += gx * gx
            b += gx * gy
            c += gy * gy
    with np.errstate(invalid="ignore", over="ignore"):
        lam = (0.5 * ((a + c) - np.sqrt((a - c) * (a - c) + 4.0 * b * b)) / float((2 * r + 1) ** 2)).astype(F32)
    out[r + 1:r + 1 + h, r + 1:r + 1 + w] = np.where(np.isfinite(lam), lam, F32(0))
    return out


def select_features(scores, max_count, quality, nms_radius, mask=None):
    """float32 [n, 2] (u, v), strongest first."""
    scores = np.asarray(scores, F32)
    H, W = scores.shape
    good = np.isfinite(scores) & (scores > 0)
    if not good.any():
        return np.zeros((0, 2), F32)
    bar = F32(quality) * scores[good].max()
    keep = good & (scores >= bar)
    if mask is not None:
        keep &= np.asarray(mask) != 0
    index = np.arange(H * W).reshape(H, W)
    found = []
    for y, x in zip(*np.nonzero(keep)):
        y0, y1, x0, x1 = max(y - nms_radius, 0), min(y + nms_radius, H - 1), max(x - nms_radius, 0), min(x + nms_radius, W - 1)
        nb, ni = scores[y0:y1 + 1, x0:x1 + 1], index[y0:y1 + 1, x0:x1 + 1]
        s = scores[y, x]
        if not ((nb > s) | ((nb == s) & (ni < index[y, x]))).any():
            found.append(((~s.view(np.uint32)) & np.uint32(0xffffffff), int(index[y, x])))
    found.sort()
    return np.array([[i % W, i // W] for _, i in found[:max_count]], F32).reshape(-1, 2)


# ---- the tracker --------------------------------------------------------------------------------------------------------------
def bilinear(img, x, y):
    H, W = img.shape
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    x0 = np.clip(np.floor(x).astype(np.int64), 0, W - 2)
    y0 = np.clip(np.floor(y).astype(np.int64), 0, H - 2)
    a, b = x - x0.astype(F32), y - y0.astype(F32)
    i00, i01, i10, i11 = img[y0, x0], img[y0, x0 + 1], img[y0 + 1, x0], img[y0 + 1, x0 + 1]
    top = i00 + a * (i01 - i00)
    bot = i10 + a * (i11 - i10)
    return top + b * (bot - top)


def _slack(x, y, m, W, H):
    """The smallest of the four float32 slacks of the header's "inside" test: inside iff >= 0."""
    m = F32(m)
    return min(F32(x - m), F32(F32(W - 1) - F32(x + m)), F32(y - m), F32(F32(H - 1) - F32(y + m)))


def _inside(x, y, m, W, H):
    m = F32(m)
    return bool(x - m >= 0 and x + m <= F32(W - 1) and y - m >= 0 and y + m <= F32(H - 1))


def track_one(pyr_a, pyr_b, p, r, max_iterations, epsilon=0.0, min_eigen_threshold=0.0, max_residual=0.0, flow=None, reference=None,
              forward_backward_threshold=0.0):
    """(point [2] float32, status, residual float32, margins) of one feature; margins: dict(edge=smallest |slack| in
    pixels of its level, relative=smallest |quantity / threshold - 1|) over the decisions taken."""
    L = len(pyr_a)
    px, py = F32(p[0]), F32(p[1])
    margins = dict(edge=np.inf, relative=np.inf)

    def lost(status, residual=F32(0)):
        return np.array([px, py], F32), status, F32(residual), margins

    def edge(x, y, m, W, H):
        margins["edge"] = min(margins["edge"], abs(float(_slack(x, y, m, W, H))))
        return _inside(x, y, m, W, H)

    def relative(value, threshold):
        margins["relative"] = min(margins["relative"], abs(float(value) / float(threshold) - 1.0))

    gx, gy = F32(0), F32(0)
    if flow is not None:
        top = F32(1.0) / F32(1 << (L - 1))
        gx, gy = F32(flow[0]) * top, F32(flow[1]) * top
    if not np.isfinite([px, py, gx, gy]).all():
        return lost(NON_FINITE)
    side = 2 * r + 1
    n = side * side
    wi = (np.arange(n) % side - r).astype(F32)
    wj = (np.arange(n) // side - r).astype(F32)
    one, half, two = F32(1), F32(0.5), F32(2)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for l in range(L - 1, -1, -1):
            scale = F32(1.0) / F32(1 << l)
            plx, ply = px * scale, py * scale
            A, B = pyr_a[l], pyr_b[l]
            H, W = A.shape
            skip = False
            if not edge(plx, ply, r + 1, W, H):
                if l == 0:
                    return lost(OUT_OF_IMAGE)
                skip = True
            else:
                x, y = plx + wi, ply + wj
                T = bilinear(A, x, y)
                Tx = half * (bilinear(A, x + one, y) - bilinear(A, x - one, y))
                Ty = half * (bilinear(A, x, y + one) - bilinear(A, x, y - one))
                tx, ty = Tx.astype(np.float64), Ty.astype(np.float64)
                gxx, gxy, gyy = _sum(tx * tx), _sum(tx * ty), _sum(ty * ty)
                e_min = 0.5 * ((gxx + gyy) - np.sqrt((gxx - gyy) * (gxx - gyy) + 4.0 * gxy * gxy)) / float(n)
                if not np.isfinite(e_min):
                    return lost(NON_FINITE)
                if min_eigen_threshold > 0:
                    relative(e_min, F32(min_eigen_threshold))
                if e_min < float(F32(min_eigen_threshold)):
                    if l == 0:
                        return lost(FLAT)
                    skip = True
            if skip:
                gx, gy = two * gx, two * gy
                continue
            det = gxx * gyy - gxy * gxy
            vx, vy = F32(0), F32(0)
            for _ in range(max_iterations):
                qx, qy = (plx + gx) + vx, (ply + gy) + vy
                if not (np.isfinite(qx) and np.isfinite(qy)):
                    return lost(NON_FINITE)
                if not edge(qx, qy, r, W, H):
                    return lost(OUT_OF_IMAGE)
                e = (T - bilinear(B, qx + wi, qy + wj)).astype(np.float64)
                bx, by = _sum(e * tx), _sum(e * ty)
                dx, dy = (gyy * bx - gxy * by) / det, (gxx * by - gxy * bx) / det
                if not (np.isfinite(dx) and np.isfinite(dy)):
                    return lost(NON_FINITE)
                vx, vy = vx + F32(dx), vy + F32(dy)
                if epsilon > 0 and dx * dx + dy * dy < float(F32(epsilon)) ** 2:
                    break
            if l > 0:
                gx, gy = two * (gx + vx), two * (gy + vy)
                continue
            rx, ry = (px + gx) + vx, (py + gy) + vy
            if not (np.isfinite(rx) and np.isfinite(ry)):
                return lost(NON_FINITE)
            if not edge(rx, ry, r, W, H):
                return lost(OUT_OF_IMAGE)
            e = T - bilinear(B, rx + wi, ry + wj)
            residual = F32(_sum(np.abs(e).astype(np.float64)) / float(n))
            if not np.isfinite(residual):
                return lost(NON_FINITE)
            if max_residual > 0:
                relative(residual, F32(max_residual))
                if residual > F32(max_residual):
                    return lost(RESIDUAL, residual)
            if reference is not None:
                ex, ey = rx - F32(reference[0]), ry - F32(reference[1])
                d2, bar = ex * ex + ey * ey, F32(forward_backward_threshold) * F32(forward_backward_threshold)
                if bar > 0:
                    relative(np.sqrt(float(d2)), F32(forward_backward_threshold))
                if not d2 <= bar:
                    return lost(FB_FAILED, residual)
            return np.array([rx, ry], F32), TRACKED, residual, margins


def _sum(values):
    """float64 sum in index (row-major window) order."""
    total = 0.0
    for v in values.tolist():
        total += v
    return total


def track(pyr_a, pyr_b, points, r, max_iterations, flow=None, reference=None, **kw):
    """(points [n, 2] float32, status [n] uint8, residual [n] float32, margins: list of dicts)."""
    points = np.asarray(points, F32).reshape(-1, 2)
    out = [track_one(pyr_a, pyr_b, points[k], r, max_iterations, flow=None if flow is None else flow[k],
                     reference=None if reference is None else reference[k], **kw) for k in range(len(points))]
    return (np.array([o[0] for o in out], F32).reshape(-1, 2), np.array([o[1] for o in out], np.uint8), np.array([o[2] for o in out], F32),
            [o[3] for o in out])


def track_forward_backward(pyr_a, pyr_b, points, r, max_iterations, forward_backward_threshold, **kw):
    """nnrt.image_proc.track_features with a forward_backward_threshold: the forward pass, the backward pass from its
    results with the original points as reference, and their combination. The margins are each feature's smaller ones."""
    points = np.asarray(points, F32).reshape(-1, 2)
    q, status, residual, m_f = track(pyr_a, pyr_b, points, r, max_iterations, **kw)
    _, back, _, m_b = track(pyr_b, pyr_a, q, r, max_iterations, reference=points, forward_backward_threshold=forward_backward_threshold, **kw)
    failed = (status == TRACKED) & (back != TRACKED)
    # a feature the forward pass lost is decided by the forward pass alone; every other one by both
    margins = [dict(edge=min(a["edge"], b["edge"]), relative=min(a["relative"], b["relative"])) if fs == TRACKED else a
               for a, b, fs in zip(m_f, m_b, status)]
    status = np.where(failed, FB_FAILED, status).astype(np.uint8)
    return np.where(failed[:, None], points, q).astype(F32), status, residual, margins


def clear_of_thresholds(m):
    return m["edge"] >= EDGE_MARGIN and m["relative"] >= RELATIVE_MARGIN


# ---- the GPU tests' input sets ------------------------------------------------------------------------------------------------
MOTIONS = dict(still=dict(shift=(0.0, 0.0)), small=dict(shift=(0.5, 0.25)), shift=dict(shift=(2.3, -1.6)), turn=dict(shift=(0.4, -0.3), angle=0.01))
ITERATIONS = 10
MIN_EIGEN = 1e-7

# (W, H, motion, levels, window radius, feature count)
TRACK_CASES = [(72, 40, "still", 1, 1, 1), (72, 40, "small", 3, 3, 64), (72, 40, "shift", 3, 7, 65), (72, 40, "turn", 3, 3, 65),
               (72, 40, "shift", 1, 7, 64), (64, 48, "shift", 1, 3, 64), (64, 48, "small", 1, 7, 65), (64, 48, "turn", 3, 7, 64),
               (64, 48, "still", 3, 1, 65), (64, 48, "shift", 3, 3, 1), (17, 13, "small", 3, 3, 1), (17, 13, "still", 3, 1, 64),
               (17, 13, "small", 1, 1, 65)]


def _draw_points(rng, count, W, H, accept):
    """`count` points uniform over the image (a pixel beyond it on every side), each kept only if accept(point) says its
    decisions are clear of their thresholds."""
    points = []
    for _ in range(200 * count + 200):
        if len(points) == count:
            break
        p = np.array([rng.uniform(-1.0, W), rng.uniform(-1.0, H)], F32)
        if accept(p):
            points.append(p)
    assert len(points) == count, "could not draw enough points clear of the thresholds"
    return np.array(points, F32)


@functools.lru_cache(maxsize=None)
def track_case(W, H, motion_name, levels, r, count):
    """dict(pyr_a, pyr_b, points, want=(points, status, residual, margins), options) of one TRACK_CASES row."""
    mo = MOTIONS[motion_name]
    pyr_a, pyr_b = pyramid(texture(W, H), levels), pyramid(texture(W, H, **mo), levels)
    options = dict(epsilon=0.0, min_eigen_threshold=MIN_EIGEN, max_residual=0.0)
    rng = np.random.default_rng(1000 * W + 10 * r + levels + count)

    def clear(p):
        return clear_of_thresholds(track_one(pyr_a, pyr_b, p, r, ITERATIONS, **options)[3])
    if count == 1:   # one feature: near the middle, where it is tracked
        points = np.array([[W / 2 + 0.25, H / 2 - 0.25]], F32)
        assert clear(points[0])
    else:
        points = _draw_points(rng, count, W, H, clear)
    return dict(pyr_a=pyr_a, pyr_b=pyr_b, points=points, r=r, options=options, want=track(pyr_a, pyr_b, points, r, ITERATIONS, **options))


SPECIAL_CASES = ("flat", "out_of_image", "walks_out", "nan_pixel", "max_residual", "forward_backward")


@functools.lru_cache(maxsize=None)
def special_case(name):
    """One input set per cause of loss: dict(pyr_a, pyr_b, points, r, options, want, expect) where expect maps a feature's
    row to the status the case is about. forward_backward: options hold forward_backward_threshold and want comes from
    track_forward_backward."""
    W, H, r, levels = 64, 48, 3, 1
    a, b = texture(W, H), texture(W, H, shift=(0.5, 0.25))
    options = dict(epsilon=0.0, min_eigen_threshold=MIN_EIGEN, max_residual=0.0)
    good = np.array([[20.5, 20.25], [40.25, 30.5]], F32)
    if name == "flat":
        a, b = a.copy(), b.copy()
        a[8:28, 30:50] = F32(0.5)
        b[8:28, 30:50] = F32(0.5)
        points, expect = np.concatenate([good[:1], np.array([[40.25, 18.5]], F32)]), {1: FLAT}
        options["min_eigen_threshold"] = 1e-6
    elif name == "out_of_image":
        points, expect = np.concatenate([good, np.array([[2.5, 20.25], [30.5, 45.5]], F32)]), {2: OUT_OF_IMAGE, 3: OUT_OF_IMAGE}
    elif name == "walks_out":
        # the template fits at x = 58.6 (58.6 + 4 <= 63); the texture has moved 2.3 to the right, and 58.6 + 2.3 + 3 > 63
        b = texture(W, H, shift=(2.3, 0.0))
        points, expect = np.concatenate([good[:1], np.array([[58.6, 20.25]], F32)]), {1: OUT_OF_IMAGE}
    elif name == "nan_pixel":
        a = a.copy()
        a[31, 42] = np.nan
        b2 = b.copy()
        b2[10, 12] = np.nan
        b = b2
        points, expect = np.array([[20.5, 20.25], [40.25, 30.5], [12.5, 11.25]], F32), {1: NON_FINITE, 2: NON_FINITE}
    elif name == "max_residual":
        # the right half of B is brighter by 0.05: the residual there is about 0.05, elsewhere that of the interpolation
        b = b.copy()
        b[:, 32:] += F32(0.05)
        points, expect = np.array([[12.5, 20.25], [18.25, 30.5], [44.5, 16.25], [52.25, 34.5]], F32), {2: RESIDUAL, 3: RESIDUAL}
        options["max_residual"] = 0.02
    elif name == "forward_backward":
        # an occluding square of another texture pasted into B; the points are drawn as in track_case
        levels, r = 2, 3
        b = b.copy()
        b[20:42, 34:58] = texture(24, 22, shift=(7.0, 3.0), angle=0.9) * F32(0.6) + F32(0.3)
        options["forward_backward_threshold"] = 0.3
        pa, pb = pyramid(a, levels), pyramid(b, levels)
        points = _draw_points(np.random.default_rng(7), 24, W, H, lambda p: 8 <= p[0] <= 55 and 8 <= p[1] <= 39 and clear_of_thresholds(
            track_forward_backward(pa, pb, p[None], r, ITERATIONS, **options)[3][0]))
        expect = None   # whatever the restatement says: the CPU test checks that both outcomes occur and where
    else:
        raise KeyError(name)
    pyr_a, pyr_b = pyramid(a, levels), pyramid(b, levels)
    if name == "forward_backward":
        want = track_forward_backward(pyr_a, pyr_b, points, r, ITERATIONS, **options)
    else:
        want = track(pyr_a, pyr_b, points, r, ITERATIONS, **options)
    if expect is None:
        expect = {int(k): FB_FAILED for k in np.nonzero(want[1] == FB_FAILED)[0]}
    return dict(pyr_a=pyr_a, pyr_b=pyr_b, points=points, r=r, options=options, want=want, expect=expect)


# ---- the score and selection tests' images ----------------------------------------------------------------------------------------
def lattice_image(W, H, seed):
    """Values that are multiples of 1/256 in [0, 1): smoothed noise, so that corners stand out, quantised. Gradients,
    their products and the float64 sums over a window are then exact, whatever the order."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.0, 1.0, (H, W))
    for _ in range(2):   # a 3 x 3 box blur, edges repeated
        p = np.pad(v, 1, mode="edge")
        v = sum(p[j:j + H, i:i + W] for j in range(3) for i in range(3)) / 9.0
    v = (v - v.min()) / max(v.max() - v.min(), 1e-12)
    return (np.minimum(np.floor(v * 256.0), 255.0) / 256.0).astype(F32)
