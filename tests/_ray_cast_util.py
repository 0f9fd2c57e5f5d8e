"""VoxelBlockGrid.ray_cast restated in float32 numpy from the text of DESIGN.md section 19 (not from the kernel): the
yardstick of tests/test_ray_cast_cpu.py (against analytic surfaces) and tests/test_gpu_ray_cast.py (bit for bit).

Inputs are what the grids already export: the voxel rows (x, y, z, tsdf, weight[, r, g, b]) in buffer order
(OracleGrid.values_all / NonRigidSurfaceVoxelBlockGrid.extract_voxel_values_and_coordinates) and the block coordinates in
the same order (OracleGrid.block_coords / get_block_coordinates). Every operation is one float32 numpy ufunc, so every
intermediate is rounded to float32 exactly where the text says so; no fused multiply-add can appear."""
import math

import numpy as np

F = np.float32
ATTRIBUTES = ("depth", "vertex", "normal", "color")


def invert4(a):
    """Gauss-Jordan with partial pivoting in float64, the operation order of the library's host-side invert4; None for a
    singular matrix."""
    m = [[float(a[r][c]) if c < 4 else (1.0 if c - 4 == r else 0.0) for c in range(8)] for r in range(4)]
    for c in range(4):
        p = c
        for r in range(c + 1, 4):
            if abs(m[r][c]) > abs(m[p][c]):
                p = r
        if m[p][c] == 0.0:
            return None
        if p != c:
            m[p], m[c] = m[c], m[p]
        d = m[c][c]
        for k in range(8):
            m[c][k] /= d
        for r in range(4):
            if r != c:
                f = m[r][c]
                for k in range(8):
                    m[r][k] -= f * m[c][k]
    return np.array([row[4:] for row in m], np.float64)


def step_bound(depth_min, depth_max, voxel_size):
    """max_steps = ceil(2 (depth_max - depth_min) / voxel_size) + 2, from the float32 values, in float64."""
    return int(math.ceil(2.0 * (float(F(depth_max)) - float(F(depth_min))) / float(F(voxel_size)))) + 2


class _Volume:
    """Voxel rows by (block index, z, y, x) and a dense block-key -> block-index table (-1: absent)."""

    def __init__(self, rows, blocks, res):
        blocks = np.asarray(blocks, np.int64).reshape(-1, 3)
        self.res = res
        self.count = len(blocks)
        rows = np.asarray(rows, np.float32)
        self.channels = rows.shape[1] if rows.ndim == 2 and rows.size else 5
        self.rows = rows.reshape(self.count, res, res, res, self.channels)
        if self.count:
            self.low = blocks.min(0)
            self.table = np.full(tuple(blocks.max(0) - self.low + 1), -1, np.int64)
            self.table[tuple((blocks - self.low).T)] = np.arange(self.count)
        else:
            self.low = np.zeros(3, np.int64)
            self.table = np.full((0, 0, 0), -1, np.int64)

    def find(self, b):
        """block index of every key b [N, 3] (-1 where the block is absent)"""
        rel = b - self.low
        inside = ((rel >= 0) & (rel < np.array(self.table.shape))).all(1)
        out = np.full(len(b), -1, np.int64)
        out[inside] = self.table[tuple(rel[inside].T)]
        return out

    def voxel(self, q):
        """(block index, rows [N, C]) of the global voxel coordinates q [N, 3]; rows are 0 where the block is absent"""
        b = q // self.res                   # floor division
        l = q - b * self.res
        idx = self.find(b)
        rows = np.zeros((len(q), self.channels), np.float32)
        ok = idx >= 0
        rows[ok] = self.rows[idx[ok], l[ok, 2], l[ok, 1], l[ok, 0]]
        return b, idx, rows


def range_map(vol, voxel_size, cast_blocks, K, E, width, height, depth_min, depth_max, f):
    """(a): float32 [ceil(H/f), ceil(W/f), 2], (depth_max, depth_min) where no block reaches."""
    TH, TW = -(-height // f), -(-width // f)
    rng = np.empty((TH, TW, 2), np.float32)
    rng[..., 0], rng[..., 1] = F(depth_max), F(depth_min)
    cast = np.asarray(cast_blocks, np.int64).reshape(-1, 3)
    if len(cast) == 0 or vol.count == 0:
        return rng
    cast = cast[vol.find(cast) >= 0]       # inactive rows contribute nothing
    if len(cast) == 0:
        return rng
    m = np.asarray(E, np.float64)[:3, :4].astype(np.float32)
    fx, fy, cx, cy = F(K[0][0]), F(K[1][1]), F(K[0][2]), F(K[1][2])
    side = F(vol.res) * F(voxel_size)
    offs = np.array([[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)], np.int64)
    corners = (cast[:, None, :] + offs[None]).astype(np.float32) * side          # [B, 8, 3]
    x, y, z = corners[..., 0], corners[..., 1], corners[..., 2]
    cam = [((x * m[r, 0] + y * m[r, 1]) + z * m[r, 2]) + m[r, 3] for r in range(3)]
    xc, yc, zc = cam
    with np.errstate(all="ignore"):
        inv_z = F(1.0) / zc
        u = (fx * xc) * inv_z + cx
        v = (fy * yc) * inv_z + cy
    ff = F(f)
    for i in range(len(cast)):
        behind = zc[i] <= 0
        if behind.all():
            continue
        z_hi = np.fmin(zc[i].max(), F(depth_max))
        if behind.any():
            x0, x1, y0, y1, z_lo = 0, TW - 1, 0, TH - 1, F(depth_min)
        else:
            fx0, fx1 = np.fmax(np.floor(u[i].min() / ff), F(0)), np.fmin(np.floor(u[i].max() / ff), F(TW - 1))
            fy0, fy1 = np.fmax(np.floor(v[i].min() / ff), F(0)), np.fmin(np.floor(v[i].max() / ff), F(TH - 1))
            if not (fx0 <= fx1 and fy0 <= fy1):
                continue
            x0, x1, y0, y1 = int(fx0), int(fx1), int(fy0), int(fy1)
            z_lo = np.fmax(zc[i].min(), F(depth_min))
        if not z_lo < z_hi:
            continue
        rng[y0:y1 + 1, x0:x1 + 1, 0] = np.minimum(rng[y0:y1 + 1, x0:x1 + 1, 0], z_lo)
        rng[y0:y1 + 1, x0:x1 + 1, 1] = np.maximum(rng[y0:y1 + 1, x0:x1 + 1, 1], z_hi)
    return rng


def ray_cast(rows, grid_blocks, res, voxel_size, cast_blocks, K, E, width, height, attributes=ATTRIBUTES, depth_scale=1000.0, depth_min=0.1,
             depth_max=3.0, weight_threshold=3.0, trunc_voxel_multiplier=8.0, range_map_down_factor=8):
    """The whole call. Returns {"range", "hit" (bool [H, W]), and per requested attribute its map}; "steps" is the largest
    number of steps any ray took (for the tests' check of the step bound)."""
    H, W, f = int(height), int(width), int(range_map_down_factor)
    vol = _Volume(rows, grid_blocks, int(res))
    vs = F(voxel_size)
    out = {"range": range_map(vol, vs, cast_blocks, K, E, W, H, depth_min, depth_max, f)}
    pose = invert4(np.asarray(E, np.float64))
    assert pose is not None, "singular extrinsic"
    m = pose[:3, :4].astype(np.float32)
    fx, fy, cx, cy = F(K[0][0]), F(K[1][1]), F(K[0][2]), F(K[1][2])
    half, side, trunc = F(0.5) * vs, F(vol.res) * vs, vs * F(trunc_voxel_multiplier)
    wt = F(weight_threshold)
    max_steps = step_bound(depth_min, depth_max, vs)

    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.ravel(), ys.ravel()
    P = H * W
    ca, cb = (xs.astype(np.float32) - cx) / fx, (ys.astype(np.float32) - cy) / fy
    dw = np.stack([(ca * m[r, 0] + cb * m[r, 1]) + m[r, 2] for r in range(3)], 1)      # [P, 3]
    o = m[:, 3]
    t = out["range"][ys // f, xs // f, 0].copy()
    t_max = out["range"][ys // f, xs // f, 1].copy()
    alive = np.ones(P, bool)
    hit = np.zeros(P, bool)
    have_prev = np.zeros(P, bool)
    t_prev, tsdf_prev, t_hit = np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32)
    steps = 0
    with np.errstate(all="ignore"):
        for _ in range(max_steps):
            alive &= t < t_max
            a = np.flatnonzero(alive)
            if len(a) == 0:
                break
            steps += 1
            ta = t[a]
            p = o[None, :] + ta[:, None] * dw[a]
            q = np.floor(p / vs).astype(np.int64)
            b, idx, vox = vol.voxel(q)
            absent = idx < 0
            unseen = ~absent & (vox[:, 4] < wt)
            seen = ~absent & ~unseen
            # block absent: leave its box, plus half a voxel
            if absent.any():
                s = a[absent]
                t_exit = np.full(len(s), np.inf, np.float32)
                for k in range(3):
                    d = dw[s, k]
                    plane = (b[absent, k] + (d > 0)).astype(np.float32) * side
                    te = (plane - o[k]) / d
                    t_exit = np.where(d != 0, np.fmin(t_exit, te), t_exit)
                t[s] = np.fmax(t_exit, t[s]) + half
                have_prev[s] = False
            # voxel below the weight threshold
            s = a[unseen]
            t[s] = t[s] + vs
            have_prev[s] = False
            # observed voxel
            s = a[seen]
            tsdf = vox[seen, 3]
            cross = have_prev[s] & (tsdf_prev[s] > 0) & (tsdf <= 0)
            sc = s[cross]
            t_hit[sc] = (t[sc] * tsdf_prev[sc] - t_prev[sc] * tsdf[cross]) / (tsdf_prev[sc] - tsdf[cross])
            hit[sc] = True
            alive[sc] = False
            sn, tn = s[~cross], tsdf[~cross]
            tsdf_prev[sn], t_prev[sn], have_prev[sn] = tn, t[sn], True
            d = tn * trunc
            t[sn] = t[sn] + np.where(d < vs, vs, d)
    out["hit"] = hit.reshape(H, W)
    out["steps"] = steps

    h = np.flatnonzero(hit)
    depth = np.zeros(P, np.float32)
    vertex, normal, color = (np.zeros((P, 3), np.float32) for _ in range(3))
    depth[h] = t_hit[h] * F(depth_scale)
    vtx = o[None, :] + t_hit[h, None] * dw[h]
    vertex[h] = vtx
    if len(h) and ("normal" in attributes or "color" in attributes):
        g = vtx / vs
        base = np.floor(g)
        r = g - base
        u = F(1.0) - r
        base = base.astype(np.int64)
        T = np.zeros((8, len(h)), np.float32)
        wsum = np.zeros(len(h), np.float32)
        csum = np.zeros((len(h), 3), np.float32)
        all_valid = np.ones(len(h), bool)
        for c in range(8):                    # corner c = i + 2 j + 4 k, weight (wx_i wy_j) wz_k
            i, j, k = c & 1, (c >> 1) & 1, c >> 2
            _, idx, vox = vol.voxel(base + np.array([i, j, k]))
            valid = (idx >= 0) & (vox[:, 4] >= wt)
            T[c] = np.where(valid, vox[:, 3], F(0))
            all_valid &= valid
            if "color" in attributes:
                w = ((r[:, 0] if i else u[:, 0]) * (r[:, 1] if j else u[:, 1])) * (r[:, 2] if k else u[:, 2])
                wsum = np.where(valid, wsum + w, wsum)
                for ch in range(3):
                    csum[:, ch] = np.where(valid, csum[:, ch] + w * vox[:, 5 + ch], csum[:, ch])
        if "color" in attributes:
            with np.errstate(all="ignore"):
                col = (csum / wsum[:, None]) / F(255.0)
            color[h] = np.where((wsum > 0)[:, None], col, F(0))
        if "normal" in attributes:
            rx, ry, rz, ux, uy, uz = r[:, 0], r[:, 1], r[:, 2], u[:, 0], u[:, 1], u[:, 2]
            gx = (((T[1] - T[0]) * uy) * uz + ((T[3] - T[2]) * ry) * uz) + (((T[5] - T[4]) * uy) * rz + ((T[7] - T[6]) * ry) * rz)
            gy = (((T[2] - T[0]) * ux) * uz + ((T[3] - T[1]) * rx) * uz) + (((T[6] - T[4]) * ux) * rz + ((T[7] - T[5]) * rx) * rz)
            gz = (((T[4] - T[0]) * ux) * uy + ((T[5] - T[1]) * rx) * uy) + (((T[6] - T[2]) * ux) * ry + ((T[7] - T[3]) * rx) * ry)
            length = np.sqrt((gx * gx + gy * gy) + gz * gz)
            with np.errstate(all="ignore"):
                n = np.stack([gx / length, gy / length, gz / length], 1)
            normal[h] = np.where((all_valid & (length > 0))[:, None], n, F(0))
    for name, arr, ch in (("depth", depth, 1), ("vertex", vertex, 3), ("normal", normal, 3), ("color", color, 3)):
        if name in attributes:
            out[name] = arr.reshape(H, W, ch)
    return out


# ---- the small TSDF scene's analytic surface, for the checks against it -------------------------------------------------
def small_scene_surface(K):
    """The surface of _tsdf_util.small_tsdf_scene (hole=False, far_strip=False, no shift) as depth(u, v) over the
    integration camera's pixel coordinates, in float64: the tilted plane with its spherical bump. Restated here because
    the scene builder keeps it local; the CPU test checks that it reproduces the scene's depth image."""
    def surface(u, v):
        x, y = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
        plane = 0.5 / (1.0 - 0.15 * x - 0.1 * y)
        c = np.array([0.03, -0.02, 0.5 + 0.15 * 0.03 - 0.1 * 0.02])
        a = x * x + y * y + 1.0
        b = x * c[0] + y * c[1] + c[2]
        disc = b * b - a * (c @ c - 0.06 ** 2)
        hit = (b - np.sqrt(np.maximum(disc, 0.0))) / a
        return np.where(disc > 0, np.minimum(plane, hit), plane)
    return surface


def analytic_depth_along_rays(surface, K, E, width, height, t_low, t_high):
    """Where each pixel's ray of the camera E (world -> camera; the world is the integration camera's frame) meets the
    surface: the ray parameter t (camera-space depth) by bisection in float64, and the integration-camera pixel (u, v) of
    that point. t is NaN where the ray does not cross the surface inside [t_low, t_high]."""
    pose = np.linalg.inv(np.asarray(E, np.float64))
    ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)
    dc = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1)
    dw = dc @ pose[:3, :3].T
    o = pose[:3, 3]

    def side(t):
        p = o + t[..., None] * dw
        z = np.maximum(p[..., 2], 1e-9)
        u, v = K[0, 0] * p[..., 0] / z + K[0, 2], K[1, 1] * p[..., 1] / z + K[1, 2]
        return p[..., 2] - surface(u, v), u, v   # < 0 in front of the surface
    lo, hi = np.full(xs.shape, float(t_low)), np.full(xs.shape, float(t_high))
    crosses = (side(lo)[0] < 0) & (side(hi)[0] > 0)
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        front = side(mid)[0] < 0
        lo, hi = np.where(front, mid, lo), np.where(front, hi, mid)
    t = 0.5 * (lo + hi)
    _, u, v = side(t)
    return np.where(crosses, t, np.nan), u, v


# The depth tolerance cannot be derived (nearest-pixel depth lookup during integration makes the zero-crossing error
# slope-dependent), so it is measured: the restatement's largest |ray-cast depth - analytic depth| on the small scene on
# the CPU, over voxel 0.01 m volumes of block resolution 8 and 16 integrated three times, cast from the integration camera
# and from extrinsic_about_y(), was MEASURED_MAX_DEPTH_ERROR metres; the tolerance is twice that.
# Measured per case (block resolution, camera): 8 integration 0.044673, 8 about-y 0.037115, 16 integration 0.049053,
# 16 about-y 0.040435 (rounded up below). The largest errors sit on the bump's silhouette, a 6 cm depth step; the median
# error is 3.5 mm, a third of a voxel.
MEASURED_MAX_DEPTH_ERROR = 0.04906
DEPTH_TOLERANCE = 2.0 * MEASURED_MAX_DEPTH_ERROR
MISS_CAP = 0.05    # at most this share of the pixels that should see the surface may miss
BORDER_CUT = 4     # pixels cut at each border of the integration image before the cap is evaluated


def compare_with_surface(result, surface, K, E, depth_scale, depth_min, depth_max, width, height, image_hw):
    """(largest depth error over the hit pixels in metres, share of expected pixels that miss, expected pixel count,
    hit count). Expected: the pixel's ray meets the surface inside [depth_min, depth_max] at a point the integration
    camera saw at least BORDER_CUT pixels inside its image [H, W] = image_hw."""
    t, u, v = analytic_depth_along_rays(surface, K, E, width, height, depth_min, depth_max)
    hit = result["hit"]
    got = result["depth"][..., 0].astype(np.float64) / depth_scale
    H, W = image_hw
    inside = (u >= BORDER_CUT) & (u <= W - 1 - BORDER_CUT) & (v >= BORDER_CUT) & (v <= H - 1 - BORDER_CUT)
    expected = np.isfinite(t) & inside
    both = hit & np.isfinite(t)
    err = float(np.abs(got[both] - t[both]).max()) if both.any() else 0.0
    stray = int((hit & ~np.isfinite(t)).sum())    # hits where the surface is not: none are allowed
    missed = float((expected & ~hit).sum()) / max(int(expected.sum()), 1)
    return err, missed, int(expected.sum()), int(hit.sum()), stray


def analytic_incidence(surface, K, E, width, height, u, v):
    """cos of the angle between each pixel's ray (camera E) and the analytic surface's normal at the integration-camera
    pixel (u, v) its ray meets, from central differences of the surface over the neighbouring pixels (float64), the
    resolution the volume was integrated at; near 0 at grazing incidence and next to the bump's silhouette, where the
    difference straddles the depth step."""
    def point(uu, vv):
        d = surface(uu, vv)
        return np.stack([(uu - K[0, 2]) / K[0, 0] * d, (vv - K[1, 2]) / K[1, 1] * d, d], -1)
    h = 1.0
    n = np.cross(point(u + h, v) - point(u - h, v), point(u, v + h) - point(u, v - h))
    n /= np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-300)
    pose = np.linalg.inv(np.asarray(E, np.float64))
    ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)
    dc = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1)
    dw = dc @ pose[:3, :3].T
    dw /= np.linalg.norm(dw, axis=-1, keepdims=True)
    return np.abs((n * dw).sum(-1))


def compare_with_input_depth(result, depth_metres, depth_min, depth_max, depth_scale):
    """Against the depth image a volume was integrated from, cast from the integration camera: (largest |ray-cast depth -
    input depth| over the hit pixels with valid input, share of the valid interior pixels that miss, their count). Valid:
    input depth inside [depth_min, depth_max]; interior: BORDER_CUT pixels in from each border."""
    d = np.asarray(depth_metres, np.float64)
    got = result["depth"][..., 0].astype(np.float64) / depth_scale
    hit = got > 0
    valid = (d >= depth_min) & (d <= depth_max)
    interior = np.zeros_like(valid)
    interior[BORDER_CUT:-BORDER_CUT, BORDER_CUT:-BORDER_CUT] = True
    both = hit & valid
    err = float(np.abs(got[both] - d[both]).max()) if both.any() else 0.0
    expected = valid & interior
    return err, float((expected & ~hit).sum()) / max(int(expected.sum()), 1), int(expected.sum())
