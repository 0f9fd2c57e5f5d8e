"""Rigid frame-to-model alignment: coarse-to-fine, dense, projective point-to-plane Gauss-Newton of model
vertices and normals against an organized live point image, on the GPU (csrc/rigid_align.hip,
nnrt_rigid_align_point_to_plane). The rigid step the reference loop delegates to Open3D
(apps/fusion/pipeline.py:338-354, `rgbd_odometry_multi_scale`); here the model is a mesh, not a rendered image.
align_rigid_hybrid (nnrt_rigid_align_hybrid) adds a photometric term, the role of Open3D's Method.Hybrid."""
from __future__ import annotations

import contextlib
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from .. import _native as N
from ._tensors import to_device
from .geometry import compute_ordered_point_cloud_normals

DEGENERATE = 1   # include/nnrt_mi355x.h NNRT_RIGID_ALIGN_DEGENERATE


@dataclass
class RigidAlignmentResult:
    """Figures of the last iteration that ran (its log row: what that iteration found before it moved the pose)."""
    transformation: np.ndarray      # [4,4] float64, model -> live camera
    correspondence_count: int
    fitness: float                  # correspondence_count / V (0 for V = 0)
    inlier_rmse: float              # sqrt(sum r^2 / correspondence_count) (0 without correspondences)
    status: int                     # 0, or DEGENERATE if any iteration of any level left the pose as it was
    log: np.ndarray                 # [sum of iterations, 2] float64 (count, sum r^2), coarse to fine; align_rigid_hybrid:
                                    # [sum of iterations, 4], (count, sum r^2, photometric count, sum rI^2)
    levels: tuple                   # per level that ran, coarse to fine: (stride, height, width, iterations)
    # what a geometric result answers for the photometric figures (plain class attributes: the dataclass keeps its seven
    # fields and its construction); align_rigid_hybrid returns the subclass below, where they are fields
    photometric_count = 0
    photometric_rmse = 0.0


@dataclass
class HybridRigidAlignmentResult(RigidAlignmentResult):
    """RigidAlignmentResult of align_rigid_hybrid: `log` is [sum of iterations, 4]."""
    photometric_count: int = 0      # vertices of the last iteration that also gave a photometric row
    photometric_rmse: float = 0.0   # sqrt(sum rI^2 / photometric_count), in units of intensity (0 without such rows)


def _shape_dtype(x):
    if isinstance(x, torch.Tensor):
        return tuple(x.shape), x.dtype == torch.float32
    a = np.asarray(x)
    return a.shape, a.dtype == np.float32


def _validate(points, normals, target_points, intrinsic_matrix, initial_transformation, iteration_counts, distance_threshold,
              normal_agreement_cos, minimum_correspondence_count, target_normals):
    for name, x in (("points", points), ("normals", normals)):
        shape, f32 = _shape_dtype(x)
        if not f32 or len(shape) != 2 or shape[1] != 3:
            raise ValueError(f"`{name}` must be a float32 array of shape [V, 3]")
    if _shape_dtype(points)[0] != _shape_dtype(normals)[0]:
        raise ValueError(f"`normals` must have one row per point: {_shape_dtype(normals)[0]} vs {_shape_dtype(points)[0]}")
    tshape, f32 = _shape_dtype(target_points)
    if not f32 or len(tshape) != 3 or tshape[2] != 3 or tshape[0] < 1 or tshape[1] < 1:
        raise ValueError("`target_points` must be an organized float32 point image of shape [H, W, 3]")
    if target_normals is not None:
        nshape, f32 = _shape_dtype(target_normals)
        if not f32 or nshape != tshape:
            raise ValueError(f"`target_normals` must be a float32 image of the shape of `target_points`, {tshape}")
    K = np.asarray(intrinsic_matrix.detach().cpu() if isinstance(intrinsic_matrix, torch.Tensor) else intrinsic_matrix, np.float64)
    if K.shape != (3, 3) or not np.isfinite(K).all():
        raise ValueError("`intrinsic_matrix` must be a finite 3 x 3 matrix")
    T = np.asarray(initial_transformation.detach().cpu() if isinstance(initial_transformation, torch.Tensor) else initial_transformation,
                   np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all() or not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError("`initial_transformation` must be a finite 4 x 4 matrix with last row (0, 0, 0, 1)")
    try:
        counts = tuple(int(c) for c in iteration_counts)
        integral = all(int(c) == c for c in iteration_counts)
    except (TypeError, ValueError):
        counts, integral = (), False
    if not counts or not integral or min(counts) < 0 or max(counts) < 1:
        raise ValueError("`iteration_counts` must be a non-empty sequence of non-negative integers, coarse to fine, at least one positive")
    stride = 1 << (len(counts) - 1)
    if (tshape[0] + stride - 1) // stride < 1 or (tshape[1] + stride - 1) // stride < 1:
        raise ValueError("`iteration_counts` has more levels than the image can be halved")
    if not (np.isfinite(distance_threshold) and distance_threshold > 0):
        raise ValueError("`distance_threshold` must be positive and finite")
    if np.isnan(normal_agreement_cos):
        raise ValueError("`normal_agreement_cos` is NaN")
    if int(minimum_correspondence_count) != minimum_correspondence_count or minimum_correspondence_count < 0:
        raise ValueError("`minimum_correspondence_count` must be a non-negative integer")
    return K, np.ascontiguousarray(T), counts


def align_rigid_point_to_plane(points, normals, target_points, intrinsic_matrix, initial_transformation=np.eye(4),
                               iteration_counts=(6, 3, 1), distance_threshold=0.07, normal_agreement_cos=0.5, cull_back_faces=False,
                               minimum_correspondence_count=50, target_normals=None, stream=None) -> RigidAlignmentResult:
    """Align model `points` / `normals` ([V,3] float32) to the live point image `target_points` ([H,W,3] float32, camera
    frame; z <= 0 or non-finite = no target). `initial_transformation` and the result map model to live-camera coordinates.

    `iteration_counts` runs coarse to fine (the reference's criteria list): with L entries, entry k runs on level
    l = L - 1 - k, the image decimated by s = 2^l (`target_points[::s, ::s]`, intrinsics divided by s, normals from
    compute_ordered_point_cloud_normals on the decimated image); an entry of 0 skips its level. `target_normals`
    ([H,W,3]) replaces the computed normals of level 0 only. A vertex pairs with the pixel it projects to; the pair is
    dropped beyond `distance_threshold` (metres), where the rotated model normal and the target normal agree by less than
    `normal_agreement_cos` in absolute value (<= 0: no test) and, with `cull_back_faces`, where the model normal faces away
    from the camera. An iteration with fewer than `minimum_correspondence_count` pairs, or a singular system, keeps the
    pose and sets DEGENERATE in `status`. Sums are float64 in a fixed order: the result is bit-reproducible."""
    K, T, counts = _validate(points, normals, target_points, intrinsic_matrix, initial_transformation, iteration_counts, distance_threshold,
                             normal_agreement_cos, minimum_correspondence_count, target_normals)
    N.require_gpu()
    dev = torch.device("cuda", N.current_device())
    p = to_device(points, torch.float32, dev)
    n = to_device(normals, torch.float32, dev)
    tp = to_device(target_points, torch.float32, dev)
    tn0 = None if target_normals is None else to_device(target_normals, torch.float32, dev)
    V = p.shape[0]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    status, logs, levels = 0, [], []
    # the levels' normals run on torch's current stream: make `stream` that stream for the duration
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        for k, iterations in enumerate(counts):
            level = len(counts) - 1 - k
            if iterations == 0:
                continue
            s = 1 << level
            tpl = tp if s == 1 else tp[::s, ::s].contiguous()
            h, w = int(tpl.shape[0]), int(tpl.shape[1])
            tnl = tn0 if (level == 0 and tn0 is not None) else compute_ordered_point_cloud_normals(tpl.reshape(-1, 3), (h, w))
            T_out = np.empty((4, 4), np.float64)
            log = np.zeros((iterations, 2), np.float64)
            st = ctypes.c_int32(0)
            N.check(N.lib().nnrt_rigid_align_point_to_plane(
                N.ptr(p), N.ptr(n), V, N.ptr(tpl), N.ptr(tnl), h, w, float(fx / s), float(fy / s), float(cx / s), float(cy / s), N.ptr(T),
                iterations, float(distance_threshold), float(normal_agreement_cos), int(bool(cull_back_faces)),
                int(minimum_correspondence_count), N.ptr(T_out), N.ptr(log), iterations, ctypes.byref(st), N.stream_ptr(stream)))
            T = T_out   # the pose is carried to the next level on the host
            status |= int(st.value)
            logs.append(log)
            levels.append((s, h, w, iterations))
    log = np.concatenate(logs, 0)
    count = int(log[-1, 0])
    return RigidAlignmentResult(transformation=T, correspondence_count=count, fitness=count / V if V else 0.0,
                                inlier_rmse=float(np.sqrt(log[-1, 1] / count)) if count else 0.0, status=status, log=log, levels=tuple(levels))


def _validate_photometric(points, colors, target_points, target_color, photometric_weight, photometric_residual_threshold):
    shape, f32 = _shape_dtype(colors)
    if not f32 or len(shape) != 2 or shape[1] != 3 or shape[0] != _shape_dtype(points)[0][0]:
        raise ValueError(f"`colors` must be a float32 array of shape [V, 3] with one row per point, got {shape}")
    cshape = tuple(target_color.shape) if isinstance(target_color, torch.Tensor) else np.asarray(target_color).shape
    cdtype = target_color.dtype if isinstance(target_color, torch.Tensor) else np.asarray(target_color).dtype
    if cdtype not in (torch.uint8, np.dtype(np.uint8)):
        raise ValueError(f"`target_color` must be a uint8 image, got {cdtype}")
    tshape = _shape_dtype(target_points)[0]
    if len(cshape) != 3 or cshape[2] != 3 or tuple(cshape[:2]) != tuple(tshape[:2]):
        raise ValueError(f"`target_color` must be [H, W, 3] of the size of `target_points`, {tuple(tshape[:2])}; got {tuple(cshape)}")
    if not (np.isfinite(photometric_weight) and photometric_weight > 0):
        raise ValueError("`photometric_weight` must be positive and finite")
    if np.isnan(photometric_residual_threshold):
        raise ValueError("`photometric_residual_threshold` is NaN")


def align_rigid_hybrid(points, normals, colors, target_points, target_color, intrinsic_matrix, initial_transformation=np.eye(4),
                       iteration_counts=(6, 3, 1), distance_threshold=0.07, normal_agreement_cos=0.5, cull_back_faces=False,
                       minimum_correspondence_count=50, target_normals=None, photometric_weight=0.1, photometric_residual_threshold=0.0,
                       stream=None) -> HybridRigidAlignmentResult:
    """align_rigid_point_to_plane with a photometric term (the role of Method.Hybrid in the Open3D call of the
    reference loop): `colors` ([V,3] float32 in [0, 1], e.g. TriangleMesh.vertex_colors) are the model's, `target_color`
    (uint8 [H,W,3], the size of `target_points`) the live frame's. Every other parameter is align_rigid_point_to_plane's.

    A vertex whose geometric row is kept also compares its luminance c with the live intensity image sampled bilinearly
    at its unrounded pixel: residual rI = I(u, v) - c, row [q x gI, gI] with gI = dI/dq through the projection, both times
    `photometric_weight`, added to the same normal equations. The row is left out where c is not finite, where the four
    taps do not all lie in the image on valid target points, and, with `photometric_residual_threshold` > 0, where |rI|
    exceeds it. The term constrains the directions point-to-plane slides along (planes, cylinders, spheres). The intensity
    image is built once; each coarser level's is the next finer one's halved by a 3 x 3 binomial kernel centred on (2i, 2j).

    `photometric_weight` is in metres per unit of intensity. The default 0.1 is the ratio of an assumed 5 mm depth noise
    to an assumed 0.05 intensity noise; nobody has tuned it on a sequence. The result's `log` is [iterations, 4]:
    (count, sum r^2, photometric count, sum rI^2 unscaled)."""
    K, T, counts = _validate(points, normals, target_points, intrinsic_matrix, initial_transformation, iteration_counts, distance_threshold,
                             normal_agreement_cos, minimum_correspondence_count, target_normals)
    _validate_photometric(points, colors, target_points, target_color, photometric_weight, photometric_residual_threshold)
    N.require_gpu()
    from .image_proc import halve_intensity, intensity_from_rgb8
    dev = torch.device("cuda", N.current_device())
    p = to_device(points, torch.float32, dev)
    n = to_device(normals, torch.float32, dev)
    c = to_device(colors, torch.float32, dev)
    tp = to_device(target_points, torch.float32, dev)
    tn0 = None if target_normals is None else to_device(target_normals, torch.float32, dev)
    V = p.shape[0]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    status, logs, levels = 0, [], []
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        # the intensity pyramid, finest first: level l from level l - 1, whether or not level l - 1 iterates
        intensity = [intensity_from_rgb8(target_color)]
        for _ in range(len(counts) - 1):
            intensity.append(halve_intensity(intensity[-1]))
        for k, iterations in enumerate(counts):
            level = len(counts) - 1 - k
            if iterations == 0:
                continue
            s = 1 << level
            tpl = tp if s == 1 else tp[::s, ::s].contiguous()
            h, w = int(tpl.shape[0]), int(tpl.shape[1])
            til = intensity[level]
            assert tuple(til.shape) == (h, w)
            tnl = tn0 if (level == 0 and tn0 is not None) else compute_ordered_point_cloud_normals(tpl.reshape(-1, 3), (h, w))
            T_out = np.empty((4, 4), np.float64)
            log = np.zeros((iterations, 4), np.float64)
            st = ctypes.c_int32(0)
            N.check(N.lib().nnrt_rigid_align_hybrid(
                N.ptr(p), N.ptr(n), N.ptr(c), V, N.ptr(tpl), N.ptr(tnl), N.ptr(til), h, w, float(fx / s), float(fy / s), float(cx / s),
                float(cy / s), N.ptr(T), iterations, float(distance_threshold), float(normal_agreement_cos), int(bool(cull_back_faces)),
                int(minimum_correspondence_count), float(photometric_weight), float(photometric_residual_threshold), N.ptr(T_out), N.ptr(log),
                iterations, ctypes.byref(st), N.stream_ptr(stream)))
            T = T_out
            status |= int(st.value)
            logs.append(log)
            levels.append((s, h, w, iterations))
    log = np.concatenate(logs, 0)
    count, photometric = int(log[-1, 0]), int(log[-1, 2])
    return HybridRigidAlignmentResult(transformation=T, correspondence_count=count, fitness=count / V if V else 0.0,
                                      inlier_rmse=float(np.sqrt(log[-1, 1] / count)) if count else 0.0, status=status, log=log,
                                      levels=tuple(levels), photometric_count=photometric,
                                      photometric_rmse=float(np.sqrt(log[-1, 3] / photometric)) if photometric else 0.0)
