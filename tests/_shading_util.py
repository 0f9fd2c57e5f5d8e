"""numpy restatements of csrc/shading.hip: the three shaders, the mesh join and the depth comparison. The
shaders use float32 and the kernel's operation order (numpy rounds every float32 product and sum on its own, like the
unfused build); the head-lit shader is also restated in float64. The comparison's sums use math.fsum."""
import math
import os

import numpy as np

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the reference's shader tests (cpp/tests/test_flat_edge_shader.cpp, test_vertex_color_shader.cpp)
TRIANGLE_VERTICES = np.array([[-1.5, -2.2, 5.0], [-1.5, 2.2, 5.0], [2.0, 0.0, 5.0]], F32)
TRIANGLE_FACES = np.array([[0, 1, 2]], np.int64)
TRIANGLE_COLORS = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], F32)
TRIANGLE_K = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])
TRIANGLE_SIZE = (480, 640)
VERTEX_COLOR_COVERED, FLAT_EDGE_LIT = 77000, 4624   # pixels of the two reference images that are not black


def golden_image(name):
    from PIL import Image
    return np.array(Image.open(os.path.join(GOLDEN, name)).convert("RGB"), np.uint8)


def to_byte(x):
    """Truncation toward zero of a float32 array; <= 0 and NaN give 0, >= 255 gives 255."""
    x = np.asarray(x, F32)
    out = np.zeros(x.shape, np.uint8)
    with np.errstate(invalid="ignore"):
        high = x >= F32(255)
        middle = (x > 0) & ~high
    out[high] = 255
    out[middle] = x[middle].astype(np.int32).astype(np.uint8)
    return out


def _front(pixel_faces, triangles, vertex_count):
    """Slot-0 face per pixel, which pixels are drawn, and their faces' vertex indices [H, W, 3] (0 where not drawn)."""
    face = np.asarray(pixel_faces)[..., 0]
    triangles = np.asarray(triangles, np.int64).reshape(-1, 3)
    drawn = (face >= 0) & (face < len(triangles))
    corners = np.zeros(face.shape + (3,), np.int64)
    if len(triangles):
        corners[drawn] = triangles[face[drawn]]
    inside = ((corners >= 0) & (corners < vertex_count)).all(-1)
    drawn &= inside
    corners[~drawn] = 0
    return drawn, corners


def shade_vertex_color(pixel_faces, barycentrics, triangles, colors):
    colors = np.asarray(colors, F32).reshape(-1, 3)
    drawn, corners = _front(pixel_faces, triangles, len(colors))
    b = np.asarray(barycentrics, F32)[..., 0, :]
    image = np.zeros(drawn.shape + (3,), np.uint8)
    if not len(colors):
        return image
    a = np.zeros(drawn.shape + (3,), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            a = a + b[..., k, None] * colors[corners[..., k]]
        value = to_byte(a * F32(255))
    image[drawn] = value[drawn]
    return image


def ndc_line_width(pixel_line_width, H, W):
    return F32(pixel_line_width) / (F32(min(H, W)) / F32(2))


def shade_flat_edge(pixel_faces, distances, pixel_line_width, color):
    face = np.asarray(pixel_faces)[..., 0]
    H, W = face.shape
    image = np.zeros((H, W, 3), np.uint8)
    if H * W == 0:
        return image
    w = ndc_line_width(pixel_line_width, H, W)
    w2 = w * w
    d = np.abs(np.asarray(distances, F32)[..., 0])
    with np.errstate(invalid="ignore"):
        lit = (face >= 0) & (d < w2)
        factor = (w2 - d) / w2
        for c in range(3):
            channel = to_byte((F32(255) * F32(color[c])) * factor)
            image[..., c][lit] = channel[lit]
    return image


def shade_headlight(pixel_faces, barycentrics, triangles, normals, color, ambient, dtype=np.float64):
    """dtype float64: the exact-arithmetic yardstick (the kernel's float32 colour and ambient, widened); float32: the
    kernel's own order."""
    normals32 = np.asarray(normals, F32).reshape(-1, 3)
    drawn, corners = _front(pixel_faces, triangles, len(normals32))
    image = np.zeros(drawn.shape + (3,), np.uint8)
    if not len(normals32):
        return image
    T = dtype
    b = np.asarray(barycentrics, F32)[..., 0, :].astype(T)
    nv = normals32.astype(T)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n = (b[..., 0, None] * nv[corners[..., 0]] + b[..., 1, None] * nv[corners[..., 1]]) + b[..., 2, None] * nv[corners[..., 2]]
        length = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
        usable = (length > 0) & np.isfinite(length)
        s = np.where(usable, np.maximum(T(0), -n[..., 2] / np.where(usable, length, T(1))), T(0))
        shade = T(F32(ambient)) + (T(1) - T(F32(ambient))) * s
        for c in range(3):
            value = (T(255) * T(F32(color[c]))) * shade
            channel = to_byte(value.astype(F32)) if T is F32 else np.clip(np.floor(np.nan_to_num(value, nan=0.0)), 0, 255).astype(np.uint8)
            image[..., c][drawn] = channel[drawn]
    return image


def join(meshes):
    """Dicts with "vertex_positions", "triangle_indices" and optional "vertex_normals" / "vertex_colors" -> one dict:
    arrays concatenated in order, indices offset, an attribute not every mesh has dropped."""
    offsets = np.concatenate([[0], np.cumsum([len(m["vertex_positions"]) for m in meshes])[:-1]])
    out = {"vertex_positions": np.concatenate([np.asarray(m["vertex_positions"], F32).reshape(-1, 3) for m in meshes]),
           "triangle_indices": np.concatenate([np.asarray(m["triangle_indices"], np.int64).reshape(-1, 3) + o for m, o in zip(meshes, offsets)])}
    for name in ("vertex_normals", "vertex_colors"):
        if all(m.get(name) is not None for m in meshes):
            out[name] = np.concatenate([np.asarray(m[name], F32).reshape(-1, 3) for m in meshes])
        else:
            out[name] = None
    return out


def compare_depth(pixel_faces, pixel_depths, depth, depth_scale=1000.0, depth_max=3.0, inlier_threshold=0.01):
    """(record dict, difference image float32): model - frame where both are valid, NaN elsewhere."""
    model = np.asarray(pixel_faces)[..., 0] >= 0
    with np.errstate(invalid="ignore"):
        z = np.asarray(depth).astype(F32) / F32(depth_scale)
        seen = (z > 0) & (z < F32(depth_max))
    both = model & seen
    difference = np.full(model.shape, np.nan, F32)
    difference[both] = np.asarray(pixel_depths, F32)[..., 0][both] - z[both]
    magnitude = np.abs(difference[both])
    wide = [float(m) for m in magnitude]
    record = {"both": int(both.sum()), "model_only": int((model & ~seen).sum()), "frame_only": int((seen & ~model).sum()),
              "inliers": int((magnitude <= F32(inlier_threshold)).sum()), "sum_abs": math.fsum(wide),
              "sum_sq": math.fsum(m * m for m in wide),   # the double product of two float32 values is exact
              "max_abs": float(magnitude.max()) if len(magnitude) else 0.0}
    return record, difference
