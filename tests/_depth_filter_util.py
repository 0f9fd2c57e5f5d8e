"""numpy restatements of the depth filters and the noisy plane the loop tests track.

median_restatement gathers every window into a Python list and sorts it: a different algorithm from the kernel's
bisection. bilateral_restatement runs the documented loop in np.float32 scalars, in the documented order;
bilateral_restatement_images runs the same per-pixel sequence of float32 operations for all pixels at once (one image-wide
step per (dy, dx), dy outer), which tests/test_depth_filter_cpu.py holds equal to the scalar loop bit for bit and the GPU
tests use for their larger images."""
import numpy as np

F32 = np.float32


def median_restatement(depth, radius, preserve_zero=False):
    depth = np.asarray(depth)
    assert depth.dtype == np.uint16 and depth.ndim == 2
    H, W = depth.shape
    rows = depth.tolist()
    out = np.zeros((H, W), np.uint16)
    for y in range(H):
        y0, y1 = max(y - radius, 0), min(y + radius, H - 1)
        for x in range(W):
            if preserve_zero and rows[y][x] == 0:
                continue
            x0, x1 = max(x - radius, 0), min(x + radius, W - 1)
            window = sorted(v for yy in range(y0, y1 + 1) for v in rows[yy][x0:x1 + 1] if v > 0)
            if window:
                out[y, x] = window[len(window) // 2]
    return out


def _valid(v):
    return bool(v > 0) and bool(np.isfinite(v))


def bilateral_restatement(depth, radius, spatial, range_weights, range_index_scale, depth_scale):
    """depth [H, W] uint16 or float32; spatial [(2r+1), (2r+1)] and range_weights [n] float32 -> float32 [H, W]."""
    depth = np.asarray(depth)
    image = depth.astype(F32)
    spatial = np.asarray(spatial, F32).reshape(2 * radius + 1, 2 * radius + 1)
    range_weights = np.asarray(range_weights, F32)
    count = len(range_weights)
    scale, out_scale = F32(range_index_scale), F32(depth_scale)
    H, W = image.shape
    out = np.zeros((H, W), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for y in range(H):
            for x in range(W):
                c = image[y, x]
                if not _valid(c):
                    continue
                s_w, s_v = F32(0), F32(0)
                for dy in range(-radius, radius + 1):
                    if not 0 <= y + dy < H:
                        continue
                    for dx in range(-radius, radius + 1):
                        if not 0 <= x + dx < W:
                            continue
                        v = image[y + dy, x + dx]
                        if not _valid(v):
                            continue
                        f = F32(np.abs(F32(v - c)) * scale)
                        if not f < count:     # int(f) >= count, or an overflowed difference
                            continue
                        w = F32(spatial[dy + radius, dx + radius] * range_weights[int(f)])
                        s_w = F32(s_w + w)
                        s_v = F32(s_v + F32(w * v))
                if s_w > 0:
                    out[y, x] = F32(F32(s_v / s_w) / out_scale)
    return out


def bilateral_restatement_images(depth, radius, spatial, range_weights, range_index_scale, depth_scale):
    """The same float32 operations per pixel, in the same order, as bilateral_restatement."""
    depth = np.asarray(depth)
    image = depth.astype(F32)
    spatial = np.asarray(spatial, F32).reshape(2 * radius + 1, 2 * radius + 1)
    range_weights = np.asarray(range_weights, F32)
    count = len(range_weights)
    scale, out_scale = F32(range_index_scale), F32(depth_scale)
    H, W = image.shape
    with np.errstate(over="ignore", invalid="ignore"):
        valid = (image > 0) & np.isfinite(image)
        padded = np.zeros((H + 2 * radius, W + 2 * radius), F32)     # 0 is invalid: a position outside the image is skipped
        padded[radius:radius + H, radius:radius + W] = np.where(valid, image, F32(0))
        s_w, s_v = np.zeros((H, W), F32), np.zeros((H, W), F32)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                v = padded[radius + dy:radius + dy + H, radius + dx:radius + dx + W]
                f = (np.abs(v - image) * scale).astype(F32)
                use = valid & (v > 0) & (f < count)
                index = np.where(use, f, F32(0)).astype(np.int64)
                w = (spatial[dy + radius, dx + radius] * range_weights[index]).astype(F32)
                s_w = np.where(use, (s_w + w).astype(F32), s_w)
                s_v = np.where(use, (s_v + (w * v).astype(F32)).astype(F32), s_v)
        positive = valid & (s_w > 0)
        quotient = np.divide(s_v, s_w, out=np.zeros((H, W), F32), where=positive)
        return np.where(positive, (quotient / out_scale).astype(F32), F32(0)).astype(F32)


# ---- the loop tests' scene: a tilted plane seen by a 256 x 192 camera -----------------------------------------------
PLANE_H, PLANE_W = 192, 256
PLANE_K = np.array([[320.0, 0.0, 127.5], [0.0, 320.0, 95.5], [0.0, 0.0, 1.0]])
PLANE = (0.5, 0.15, 0.1)   # z = 0.5 + 0.15 x + 0.1 y, camera coordinates, metres
NOISE_MM = 3


def plane_depth_mm():
    """uint16 millimetre depth [192, 256] of the plane, noise-free."""
    v, u = np.mgrid[0:PLANE_H, 0:PLANE_W].astype(np.float64)
    x, y = (u - PLANE_K[0, 2]) / PLANE_K[0, 0], (v - PLANE_K[1, 2]) / PLANE_K[1, 1]
    z = PLANE[0] / (1.0 - PLANE[1] * x - PLANE[2] * y)
    return np.round(z * 1000.0).astype(np.uint16)


def plane_normal():
    n = np.array([PLANE[1], PLANE[2], -1.0])
    return n / np.linalg.norm(n)


def noisy_plane_depth_mm(seed):
    """The plane with seeded integer noise of +-3 mm on every pixel and a few pixels zeroed."""
    rng = np.random.default_rng(seed)
    d = plane_depth_mm().astype(np.int64) + rng.integers(-NOISE_MM, NOISE_MM + 1, (PLANE_H, PLANE_W))
    holes = rng.integers(0, PLANE_H * PLANE_W, 40)
    d.reshape(-1)[holes] = 0
    return d.astype(np.uint16)


def backproject(depth_metres):
    """[H, W] metres -> [H, W, 3] float64 points with PLANE_K (0 stays at the origin)."""
    H, W = depth_metres.shape
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    z = depth_metres.astype(np.float64)
    return np.stack([z * (u - PLANE_K[0, 2]) / PLANE_K[0, 0], z * (v - PLANE_K[1, 2]) / PLANE_K[1, 1], z], -1)


def mean_angle_to_plane_normal(normals, margin=8):
    """Mean angle in degrees between unit normals [H, W, 3] and the plane's, over the pixels `margin` away from the image
    border that have a normal; the sign of a normal is not counted."""
    n = np.asarray(normals, np.float64).reshape(PLANE_H, PLANE_W, 3)[margin:-margin, margin:-margin].reshape(-1, 3)
    length = np.linalg.norm(n, axis=1)
    have = length > 0.5
    cosine = np.abs((n[have] / length[have, None]) @ plane_normal())
    return float(np.degrees(np.arccos(np.clip(cosine, 0.0, 1.0))).mean()), int(have.sum())
