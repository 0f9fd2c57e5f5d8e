"""Top-level `nnrt` image functions on the fusion app's input path (cpp/pybind/nnrt_pybind.cpp:50-67, :97-104): depth image ->
ordered point image, and the depth filters ahead of it, on the GPU. Inputs may be numpy or torch; outputs are device
tensors ([H, W, 3] float32 point images, [H, W] uint16 or float32 depth)."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from .. import _native as N
from ._overloads import Overloaded, is_int, is_tensor
from ._tensors import device_of
from .voxel_grid import DTYPE_FLOAT32, DTYPE_UINT16


def _depth_on_device(image_in, dtype: torch.dtype):
    """Device copy of a [H, W] depth image; uint16 depth travels as its int16 bit pattern (int32 -> int16 casts wrap)."""
    dev = device_of(N.current_device())
    if isinstance(image_in, np.ndarray):
        a = np.ascontiguousarray(image_in)
        t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    else:
        t = image_in.view(torch.int16) if image_in.dtype == torch.uint16 else image_in
    if t.dim() != 2:
        raise ValueError(f"depth image must be [H, W], got {tuple(t.shape)}")
    if dtype == torch.int16 and t.dtype != torch.int16:
        t = t.to(torch.int32).to(torch.int16)
    return t.to(device=dev, dtype=dtype).contiguous()


def _out(point_image_out, H, W, dev):
    if point_image_out is None:
        return torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    if not isinstance(point_image_out, torch.Tensor) or point_image_out.device != dev or point_image_out.dtype != torch.float32 \
            or tuple(point_image_out.shape) != (H, W, 3) or not point_image_out.is_contiguous():
        raise ValueError(f"point_image_out must be a contiguous float32 [{H}, {W}, 3] tensor on {dev}")
    return point_image_out


def backproject_depth_ushort(image_in, fx: float, fy: float, cx: float, cy: float, normalizer: float,
                             point_image_out: torch.Tensor | None = None) -> torch.Tensor:
    """uint16 depth (e.g. mm) -> [H, W, 3] metres (image_proc.cpp:275-309)."""
    N.require_gpu()
    d = _depth_on_device(image_in, torch.int16)
    H, W = d.shape
    out = _out(point_image_out, H, W, d.device)
    N.check(N.lib().nnrt_backproject_depth_ushort(N.ptr(d), H, W, float(fx), float(fy), float(cx), float(cy), float(normalizer),
                                                  N.ptr(out), N.stream_ptr()))
    return out


def backproject_depth_float(image_in, fx: float, fy: float, cx: float, cy: float,
                            point_image_out: torch.Tensor | None = None) -> torch.Tensor:
    """float depth in metres -> [H, W, 3] (image_proc.cpp:312-339)."""
    N.require_gpu()
    d = _depth_on_device(image_in, torch.float32)
    H, W = d.shape
    out = _out(point_image_out, H, W, d.device)
    N.check(N.lib().nnrt_backproject_depth_float(N.ptr(d), H, W, float(fx), float(fy), float(cx), float(cy), N.ptr(out), N.stream_ptr()))
    return out


def compute_mesh_from_depth(point_image, max_triangle_edge_distance):
    """compute_mesh_from_depth (nnrt_pybind.cpp:79-80 -> image_proc.cpp:341-482; csrc/depth_graph.hip): the pixel-connected
    mesh of an [H, W, 3] float32 point image as (vertices (V, 3) float32, vertex_pixels (V, 2) int32 as (x, y), faces (F, 3)
    int32), device tensors, equal to the reference's sequential loop bit for bit (vertex numbering and face order included).
    An image with H < 2 or W < 2, or without a valid triangle, gives empty tensors (the reference leaves its outputs
    unsized). Input that is not [H, W, 3] float32 is refused."""
    N.require_gpu()
    dev = device_of(N.current_device())
    if isinstance(point_image, np.ndarray):
        if point_image.dtype != np.float32:
            raise ValueError(f"point image must be float32, got {point_image.dtype}")
        p = torch.from_numpy(np.ascontiguousarray(point_image))
    elif isinstance(point_image, torch.Tensor):
        if point_image.dtype != torch.float32:
            raise ValueError(f"point image must be float32, got {point_image.dtype}")
        p = point_image
    else:
        raise ValueError("point image must be a numpy array or a torch tensor")
    if p.dim() != 3 or p.shape[2] != 3:
        raise ValueError(f"point image must be [H, W, 3], got {tuple(p.shape)}")
    p = p.to(dev).contiguous()
    H, W = int(p.shape[0]), int(p.shape[1])
    vertex_capacity = H * W if H >= 2 and W >= 2 else 0
    face_capacity = 2 * (H - 1) * (W - 1) if vertex_capacity else 0
    vertices = torch.empty((vertex_capacity, 3), dtype=torch.float32, device=dev)
    pixels = torch.empty((vertex_capacity, 2), dtype=torch.int32, device=dev)
    faces = torch.empty((face_capacity, 3), dtype=torch.int32, device=dev)
    counts = np.zeros(2, np.int64)
    N.check(N.lib().nnrt_compute_mesh_from_depth(N.ptr(p), H, W, float(max_triangle_edge_distance), N.ptr(vertices), N.ptr(pixels),
                                                 vertex_capacity, N.ptr(faces), face_capacity, N.ptr(counts[0:1]), N.ptr(counts[1:2]),
                                                 N.stream_ptr()))
    nv, nf = int(counts[0]), int(counts[1])
    return vertices[:nv].clone(), pixels[:nv].clone(), faces[:nf].clone()


def _is_depth_u16(image) -> bool:
    return (isinstance(image, np.ndarray) and image.dtype == np.uint16) or \
           (isinstance(image, torch.Tensor) and image.dtype in (torch.uint16, torch.int16))


def _median(depth_image_in, depth_image_out, radius, preserve_zero) -> torch.Tensor:
    N.require_gpu()
    if not _is_depth_u16(depth_image_in):
        raise ValueError("depth_image_in must be uint16 (numpy or torch; a torch.int16 tensor is taken as the uint16 bit pattern)")
    d = _depth_on_device(depth_image_in, torch.int16)
    H, W = d.shape
    if depth_image_out is None:
        out = torch.empty((H, W), dtype=torch.int16, device=d.device)
    else:
        out = depth_image_out
        if not isinstance(out, torch.Tensor) or out.device != d.device or out.dtype not in (torch.uint16, torch.int16) \
                or tuple(out.shape) != (H, W) or not out.is_contiguous():
            raise ValueError(f"depth_image_out must be a contiguous uint16 [{H}, {W}] tensor on {d.device}")
    N.check(N.lib().nnrt_filter_depth(N.ptr(d), H, W, int(radius), int(bool(preserve_zero)), N.ptr(out), N.stream_ptr()))
    return out if out.dtype == torch.uint16 else out.view(torch.uint16)


filter_depth = Overloaded(
    "filter_depth",
    "filter_depth (nnrt_pybind.cpp:97-104 -> image_proc.cpp:837-887; csrc/depth_filter.hip): zero-skipping median of a uint16 depth "
    "image over a (2 radius + 1)^2 window clipped to the image, 0 <= radius <= 8. The output is the element of index n / 2 of the n "
    "window values > 0 in ascending order, exactly. Deviations: an empty window gives 0 (the reference indexes an empty vector); "
    "preserve_zero=True (ours) keeps a pixel that is 0 at 0, where the reference fills it from its neighbours. The result is a "
    "device tensor viewed as torch.uint16; depth_image_out must be a contiguous device tensor of the input's shape.")


@filter_depth.overload(lambda a: is_tensor(a["depth_image_in"]) and is_tensor(a["depth_image_out"]) and is_int(a["radius"]))
def _filter_depth_into(depth_image_in, depth_image_out, radius, *, preserve_zero=False):
    _median(depth_image_in, depth_image_out, radius, preserve_zero)


@filter_depth.overload(lambda a: is_tensor(a["depth_image_in"]) and is_int(a["radius"]))
def _filter_depth_new(depth_image_in, radius, *, preserve_zero=False):
    return _median(depth_image_in, None, radius, preserve_zero)


def bilateral_weight_tables(radius: int, spatial_sigma: float, range_sigma: float, range_cutoff=None):
    """The two float32 tables of bilateral_filter_depth: spatial [(2 radius + 1), (2 radius + 1)] over (dy, dx),
    exp(-(dx^2 + dy^2) / (2 spatial_sigma^2)), and range [range_cutoff + 1], exp(-i^2 / (2 range_sigma^2)) for a depth
    difference of i units; range_cutoff defaults to ceil(3 range_sigma). Computed in float64 and rounded once."""
    if not is_int(radius) or radius < 0:
        raise ValueError(f"radius must be a non-negative integer, got {radius!r}")
    if not (spatial_sigma > 0 and math.isfinite(spatial_sigma)) or not (range_sigma > 0 and math.isfinite(range_sigma)):
        raise ValueError("spatial_sigma and range_sigma must be positive")
    if range_cutoff is None:
        range_cutoff = int(math.ceil(3.0 * range_sigma))
    if not is_int(range_cutoff) or range_cutoff < 0:
        raise ValueError(f"range_cutoff must be a non-negative integer, got {range_cutoff!r}")
    offsets = np.arange(-radius, radius + 1, dtype=np.float64)
    squared = offsets[:, None] ** 2 + offsets[None, :] ** 2
    spatial = np.exp(-squared / (2.0 * float(spatial_sigma) ** 2)).astype(np.float32)
    steps = np.arange(range_cutoff + 1, dtype=np.float64)
    weights = np.exp(-steps ** 2 / (2.0 * float(range_sigma) ** 2)).astype(np.float32)
    return np.ascontiguousarray(spatial), np.ascontiguousarray(weights)


def bilateral_filter_depth(depth, radius: int, spatial_sigma: float, range_sigma: float, range_cutoff=None,
                           depth_scale: float = 1000.0) -> torch.Tensor:
    """Edge-preserving smoothing of a depth image (csrc/depth_filter.hip; the reference has no such filter):
    [H, W] uint16 in sensor units or float32 in metres -> [H, W] float32 metres on the device, 0 where the input is not a
    positive finite depth. A neighbour contributes with bilateral_weight_tables' spatial weight times the range weight of
    its truncated depth difference in sensor units (float32 input: metres * depth_scale), and not at all beyond
    range_cutoff units, so a depth step larger than that is not blurred. range_sigma and range_cutoff are in sensor units
    for both input types; 0 <= radius <= 8, range_cutoff <= 4095."""
    N.require_gpu()
    spatial, weights = bilateral_weight_tables(radius, spatial_sigma, range_sigma, range_cutoff)
    if _is_depth_u16(depth):
        d, code, index_scale, out_scale = _depth_on_device(depth, torch.int16), DTYPE_UINT16, 1.0, float(depth_scale)
    elif (isinstance(depth, np.ndarray) and depth.dtype == np.float32) or (isinstance(depth, torch.Tensor) and depth.dtype == torch.float32):
        d, code, index_scale, out_scale = _depth_on_device(depth, torch.float32), DTYPE_FLOAT32, float(depth_scale), 1.0
    else:
        raise ValueError("depth must be a uint16 or float32 image (numpy or torch)")
    H, W = d.shape
    out = torch.empty((H, W), dtype=torch.float32, device=d.device)
    N.check(N.lib().nnrt_bilateral_filter_depth(N.ptr(d), code, H, W, int(radius), N.ptr(spatial), N.ptr(weights), int(weights.shape[0]),
                                                index_scale, out_scale, N.ptr(out), N.stream_ptr()))
    return out


def intensity_from_rgb8(color) -> torch.Tensor:
    """uint8 [H, W, 3] RGB (numpy or torch) -> float32 [H, W] luminance in [0, 1] on the device
    (csrc/photometric.hip): I = ((0.299 R + 0.587 G) + 0.114 B) / 255 in float32."""
    dtype = color.dtype if isinstance(color, torch.Tensor) else np.asarray(color).dtype
    if dtype not in (torch.uint8, np.dtype(np.uint8)) or len(color.shape) != 3 or color.shape[2] != 3:
        raise ValueError(f"color must be a uint8 [H, W, 3] image, got {dtype} {tuple(color.shape)}")
    N.require_gpu()
    dev = device_of(N.current_device())
    c = (color if isinstance(color, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(color))).to(dev).contiguous()
    H, W = int(c.shape[0]), int(c.shape[1])
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    N.check(N.lib().nnrt_intensity_from_rgb8(N.ptr(c), H, W, N.ptr(out), N.stream_ptr()))
    return out


def halve_intensity(intensity) -> torch.Tensor:
    """float32 [H, W] -> [ceil(H / 2), ceil(W / 2)] on the device (csrc/photometric.hip): output pixel (i, j)
    is the 3 x 3 binomial mean, weights (1, 2, 1) / 4 per axis, centred on input pixel (2i, 2j), indices clamped to the
    image. Level pixel (i, j) stays image pixel (2i, 2j), as when a point image is decimated by [::2, ::2]."""
    dtype = intensity.dtype if isinstance(intensity, torch.Tensor) else np.asarray(intensity).dtype
    if dtype not in (torch.float32, np.dtype(np.float32)) or len(intensity.shape) != 2:
        raise ValueError(f"intensity must be a float32 [H, W] image, got {dtype} {tuple(intensity.shape)}")
    N.require_gpu()
    dev = device_of(N.current_device())
    a = (intensity if isinstance(intensity, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(intensity))).to(dev).contiguous()
    H, W = int(a.shape[0]), int(a.shape[1])
    out = torch.empty(((H + 1) // 2, (W + 1) // 2), dtype=torch.float32, device=dev)
    N.check(N.lib().nnrt_intensity_halve(N.ptr(a), H, W, N.ptr(out), N.stream_ptr()))
    return out


# include/nnrt_mi355x.h NNRT_FEATURE_*
FEATURE_MAX_WINDOW_RADIUS, FEATURE_MAX_NMS_RADIUS, FEATURE_MAX_LEVELS, FEATURE_MAX_ITERATIONS = 7, 15, 4, 30
FEATURE_TRACKED, FEATURE_OUT_OF_IMAGE, FEATURE_FLAT, FEATURE_RESIDUAL, FEATURE_NON_FINITE, FEATURE_FB_FAILED = range(6)


def intensity_pyramid(intensity, levels: int) -> list:
    """[level 0, .., level levels - 1] of a float32 [H, W] intensity image: level l is halve_intensity of level l - 1, so
    level pixel (i, j) is image pixel (2^l i, 2^l j). The pyramid track_features takes."""
    if not 1 <= int(levels) <= FEATURE_MAX_LEVELS:
        raise ValueError(f"levels must be in [1, {FEATURE_MAX_LEVELS}], got {levels}")
    dtype = intensity.dtype if isinstance(intensity, torch.Tensor) else np.asarray(intensity).dtype
    if dtype not in (torch.float32, np.dtype(np.float32)) or len(intensity.shape) != 2:
        raise ValueError(f"intensity must be a float32 [H, W] image, got {dtype} {tuple(intensity.shape)}")
    N.require_gpu()
    dev = device_of(N.current_device())
    pyramid = [(intensity if isinstance(intensity, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(intensity))).to(dev).contiguous()]
    for _ in range(int(levels) - 1):
        pyramid.append(halve_intensity(pyramid[-1]))
    return pyramid


def _image_f32(image, name):
    dtype = image.dtype if isinstance(image, torch.Tensor) else np.asarray(image).dtype
    if dtype not in (torch.float32, np.dtype(np.float32)) or len(image.shape) != 2:
        raise ValueError(f"{name} must be a float32 [H, W] image, got {dtype} {tuple(image.shape)}")
    dev = device_of(N.current_device())
    return (image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))).to(dev).contiguous()


def _points_f32(points, name, dev):
    t = torch.as_tensor(points).to(device=dev, dtype=torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError(f"{name} must be [n, 2] (u, v), got {tuple(t.shape)}")
    return t


def corner_scores(intensity, window_radius: int = 3) -> torch.Tensor:
    """Shi-Tomasi score of every pixel of a float32 [H, W] image (nnrt_corner_scores): the smaller eigenvalue
    of the gradient matrix summed over the (2 window_radius + 1)^2 window, divided by the window's pixel count; central
    differences in float32, the sums in float64. Pixels whose window (with the gradients' taps) leaves the image score 0."""
    N.require_gpu()
    a = _image_f32(intensity, "intensity")
    H, W = int(a.shape[0]), int(a.shape[1])
    out = torch.empty((H, W), dtype=torch.float32, device=a.device)
    N.check(N.lib().nnrt_corner_scores(N.ptr(a), H, W, int(window_radius), N.ptr(out), N.stream_ptr()))
    return out


def select_features(scores, max_count: int, quality: float = 0.01, nms_radius: int = 3, mask=None) -> torch.Tensor:
    """The strongest separated corners of a score image as float32 [n, 2] (u, v) = (column, row), n <= max_count, by
    descending score and ascending pixel index (nnrt_select_features). A pixel qualifies with a finite score
    > 0 and >= quality times the largest, a non-zero `mask` (uint8 or bool [H, W], optional) and no stronger pixel (or
    equal one of lower index) within nms_radius. Reads the count back once: synchronizes the stream."""
    N.require_gpu()
    s = _image_f32(scores, "scores")
    H, W = int(s.shape[0]), int(s.shape[1])
    m = None
    if mask is not None:
        m = torch.as_tensor(mask).to(s.device)
        if tuple(m.shape) != (H, W) or m.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"mask must be a uint8 or bool [{H}, {W}] image, got {m.dtype} {tuple(m.shape)}")
        m = m.to(torch.uint8).contiguous()
    out = torch.empty((int(max_count) if max_count >= 1 else 1, 2), dtype=torch.float32, device=s.device)
    count = ctypes.c_int64(0)
    N.check(N.lib().nnrt_select_features(N.ptr(s), N.ptr(m), H, W, float(quality), int(nms_radius), int(max_count), N.ptr(out),
                                         ctypes.addressof(count), N.stream_ptr()))
    return out[:count.value]


def _track_pass(pyramid_a, pyramid_b, points, initial_flow, reference, window_radius, max_iterations, epsilon, min_eigen_threshold, max_residual,
                forward_backward_threshold):
    L, n, dev = len(pyramid_a), int(points.shape[0]), points.device
    out_points = torch.empty((n, 2), dtype=torch.float32, device=dev)
    status = torch.empty((n,), dtype=torch.uint8, device=dev)
    residual = torch.empty((n,), dtype=torch.float32, device=dev)
    pa = (N.c_void_p * L)(*[a.data_ptr() for a in pyramid_a])
    pb = (N.c_void_p * L)(*[b.data_ptr() for b in pyramid_b])
    hs = (N.c_int32 * L)(*[int(a.shape[0]) for a in pyramid_a])
    ws = (N.c_int32 * L)(*[int(a.shape[1]) for a in pyramid_a])
    N.check(N.lib().nnrt_track_features(pa, pb, hs, ws, L, N.ptr(points), N.ptr(initial_flow), N.ptr(reference), n, int(window_radius),
                                        int(max_iterations), float(epsilon), float(min_eigen_threshold), float(max_residual),
                                        float(forward_backward_threshold), N.ptr(out_points), N.ptr(status), N.ptr(residual), N.stream_ptr()))
    return out_points, status, residual


def track_features(pyramid_a, pyramid_b, points, window_radius: int = 7, max_iterations: int = 10, epsilon: float = 0.0,
                   min_eigen_threshold: float = 1e-6, max_residual: float = 0.0, forward_backward_threshold=None, initial_flow=None):
    """Pyramidal Lucas-Kanade tracking of `points` [n, 2] (u, v) from pyramid_a to pyramid_b, two intensity_pyramid lists of
    equal sizes (nnrt_track_features): (points [n, 2] float32, status [n] uint8, residual [n] float32) on the
    device. status 0 (FEATURE_TRACKED) or the cause a feature was lost for (FEATURE_*); a lost feature keeps its input
    point. residual: the mean absolute intensity difference over the window at the result. epsilon 0 runs exactly
    max_iterations per level; max_residual <= 0 keeps every residual. `initial_flow` [n, 2]: a first guess in level-0 pixels.

    forward_backward_threshold (pixels, None: off): a second pass tracks the forward results back from pyramid_b to
    pyramid_a; a feature the forward pass tracked whose way back fails, or ends farther than the threshold from where it
    started, becomes FEATURE_FB_FAILED and keeps its input point. Nothing is read back: asynchronous on the stream."""
    N.require_gpu()
    if len(pyramid_a) != len(pyramid_b) or not 1 <= len(pyramid_a) <= FEATURE_MAX_LEVELS:
        raise ValueError(f"the pyramids must have the same number of levels, 1 to {FEATURE_MAX_LEVELS}: got {len(pyramid_a)} and {len(pyramid_b)}")
    pa = [_image_f32(a, "pyramid_a level") for a in pyramid_a]
    pb = [_image_f32(b, "pyramid_b level") for b in pyramid_b]
    for l, (a, b) in enumerate(zip(pa, pb)):
        if a.shape != b.shape:
            raise ValueError(f"level {l}: pyramid_a is {tuple(a.shape)}, pyramid_b {tuple(b.shape)}")
    dev = pa[0].device
    p = _points_f32(points, "points", dev)
    flow = None if initial_flow is None else _points_f32(initial_flow, "initial_flow", dev)
    if flow is not None and flow.shape != p.shape:
        raise ValueError(f"{p.shape[0]} points but {flow.shape[0]} initial flows")
    options = (window_radius, max_iterations, epsilon, min_eigen_threshold, max_residual)
    forward = _track_pass(pa, pb, p, flow, None, *options, 0.0)
    if forward_backward_threshold is None:
        return forward
    q, status, residual = forward
    _, back_status, _ = _track_pass(pb, pa, q, None, p, *options, float(forward_backward_threshold))
    failed = (status == FEATURE_TRACKED) & (back_status != FEATURE_TRACKED)
    status = torch.where(failed, torch.full_like(status, FEATURE_FB_FAILED), status)
    return torch.where(failed[:, None], p, q), status, residual


def backproject_depth(depth_image, fx, fy, cx, cy, depth_scale: float = 1000.0) -> torch.Tensor:
    """image_processing/__init__.py:333-344: float32 depth is taken as metres, anything else as integer units / depth_scale."""
    is_float = (isinstance(depth_image, np.ndarray) and depth_image.dtype == np.float32) or \
               (isinstance(depth_image, torch.Tensor) and depth_image.dtype == torch.float32)
    if is_float:
        return backproject_depth_float(depth_image, fx, fy, cx, cy)
    return backproject_depth_ushort(depth_image, fx, fy, cx, cy, depth_scale)
