"""Top-level `nnrt` image functions on the fusion app's input path (cpp/pybind/nnrt_pybind.cpp:50-67, :97-104): depth image ->
ordered point image, and the depth filters ahead of it, on the GPU. Inputs may be numpy or torch; outputs are device
tensors ([H, W, 3] float32 point images, [H, W] uint16 or float32 depth)."""
from __future__ import annotations

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


def backproject_depth(depth_image, fx, fy, cx, cy, depth_scale: float = 1000.0) -> torch.Tensor:
    """image_processing/__init__.py:333-344: float32 depth is taken as metres, anything else as integer units / depth_scale."""
    is_float = (isinstance(depth_image, np.ndarray) and depth_image.dtype == np.float32) or \
               (isinstance(depth_image, torch.Tensor) and depth_image.dtype == torch.float32)
    if is_float:
        return backproject_depth_float(depth_image, fx, fy, cx, cy)
    return backproject_depth_ushort(depth_image, fx, fy, cx, cy, depth_scale)
