"""The sparse feature tracker without a GPU: the three entry points are declared, exported and refuse
bad arguments on the host; the numpy restatement of tests/_feature_track_util.py recovers a known shift; and every input
set the GPU tests use keeps its decisions clear of their thresholds, which is what lets tests/test_gpu_feature_track.py
demand equal status without exception."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _feature_track_util as U   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7f0000000000   # never dereferenced
NAMES = ("nnrt_corner_scores", "nnrt_select_features", "nnrt_track_features")


@pytest.fixture(scope="module")
def native():
    from dynamicfuion_python_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_off_by_default(native):
    header = open(os.path.join(ROOT, "include", "nnrt_mi355x.h")).read()
    lib = native.lib()
    for name in NAMES:
        assert f"nnrt_status {name}(" in header
        assert name in native.exported_symbols() and getattr(lib, name) is not None
    from dynamicfuion_python_amd.fusion import FusionParameters
    assert FusionParameters().landmark_tracking is None


def test_entry_points_refuse_bad_arguments_on_the_host(native):
    lib = native.lib()
    nan = float("nan")

    def scores(d_in=FAKE, height=48, width=64, radius=3, d_out=FAKE + 0x100000):
        return lib.nnrt_corner_scores(ctypes.c_void_p(d_in), height, width, radius, ctypes.c_void_p(d_out), None), lib.nnrt_last_error()

    for kw, text in ((dict(radius=0), b"window_radius"), (dict(radius=8), b"window_radius"), (dict(height=-1), b"height or width"),
                     (dict(height=1 << 16, width=1 << 15), b"2^31"), (dict(d_in=None), b"null d_intensity"), (dict(d_out=None), b"null d_out_scores"),
                     (dict(d_out=FAKE + 64), b"overlap")):
        st, msg = scores(**kw)
        assert st == 1 and text in msg, (kw, st, msg)
    assert scores(height=0, d_in=None, d_out=None)[0] == 0

    count = ctypes.c_int64(-1)

    def select(d_scores=FAKE, d_mask=None, height=48, width=64, quality=0.01, m=3, max_count=64, d_out=FAKE + 0x100000, h_count=count):
        st = lib.nnrt_select_features(ctypes.c_void_p(d_scores), ctypes.c_void_p(d_mask), height, width, quality, m, max_count, ctypes.c_void_p(d_out),
                                      ctypes.addressof(h_count) if h_count is not None else None, None)
        return st, lib.nnrt_last_error()

    for kw, text in ((dict(quality=nan), b"quality"), (dict(quality=-0.1), b"quality"), (dict(quality=1.5), b"quality"), (dict(m=-1), b"nms_radius"),
                     (dict(m=16), b"nms_radius"), (dict(max_count=0), b"max_count"), (dict(width=-3), b"height or width"),
                     (dict(d_scores=None), b"null d_scores"), (dict(d_out=None), b"null d_out_points"), (dict(h_count=None), b"null h_out_count"),
                     (dict(d_out=FAKE + 8), b"overlap"), (dict(d_mask=FAKE + 0x100000), b"overlap")):
        st, msg = select(**kw)
        assert st == 1 and text in msg, (kw, st, msg)
    assert select(width=0, d_scores=None, d_out=None)[0] == 0 and count.value == 0

    def track(levels=2, heights=(48, 24), widths=(64, 32), a=(FAKE, FAKE + 0x10000), b=(FAKE + 0x20000, FAKE + 0x30000), points=FAKE + 0x40000,
              flow=None, reference=None, n=8, r=3, iterations=10, epsilon=0.0, min_eigen=1e-6, max_residual=0.0, fb=0.0, out=FAKE + 0x50000,
              status=FAKE + 0x60000, residual=FAKE + 0x70000):
        L = len(heights)
        st = lib.nnrt_track_features((ctypes.c_void_p * L)(*a), (ctypes.c_void_p * L)(*b), (ctypes.c_int32 * L)(*heights), (ctypes.c_int32 * L)(*widths),
                                     levels, ctypes.c_void_p(points), ctypes.c_void_p(flow), ctypes.c_void_p(reference), n, r, iterations, epsilon,
                                     min_eigen, max_residual, fb, ctypes.c_void_p(out), ctypes.c_void_p(status), ctypes.c_void_p(residual), None)
        return st, lib.nnrt_last_error()

    for kw, text in ((dict(n=-1), b"count"), (dict(levels=0), b"levels"), (dict(levels=5), b"levels"), (dict(r=0), b"window_radius"),
                     (dict(r=8), b"window_radius"), (dict(iterations=0), b"max_iterations"), (dict(iterations=31), b"max_iterations"),
                     (dict(epsilon=nan), b"epsilon"), (dict(epsilon=-1.0), b"epsilon"), (dict(min_eigen=nan), b"min_eigen_threshold"),
                     (dict(max_residual=nan), b"max_residual"), (dict(fb=nan), b"forward_backward_threshold"),
                     (dict(reference=FAKE + 0x80000, fb=-1.0), b"forward_backward_threshold"), (dict(heights=(48, 23)), b"not ceil(half)"),
                     (dict(widths=(64, 33)), b"not ceil(half)"), (dict(heights=(0, 0)), b"positive"), (dict(a=(FAKE, None)), b"null image"),
                     (dict(points=None), b"null d_points"), (dict(status=None), b"null output"), (dict(out=FAKE + 0x40000 + 8), b"overlap"),
                     (dict(status=FAKE + 0x50000 + 4), b"overlap"), (dict(residual=FAKE + 16), b"pyramid level"),
                     (dict(flow=FAKE + 0x70000), b"overlap")):
        st, msg = track(**kw)
        assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (kw, st, msg)
    assert track(n=0, points=None, out=None, status=None, residual=None)[0] == 0   # nothing to track launches nothing
    with pytest.raises(native.NnrtError):
        native.check(track(r=0)[0])


# ---- the restatement against ground truth ----------------------------------------------------------------------------------------
W, H = 64, 48


def _selected():
    """The features the restatement selects on the analytic texture, under a mask that keeps every level's window inside
    its image for L = 3, r = 3 and for L = 3, r = 7 (level 1 of the latter; its level 2 is too small and is skipped)."""
    a = U.texture(W, H)
    mask = np.zeros((H, W), np.uint8)
    mask[17:28, 17:38] = 1
    points = U.select_features(U.corner_scores(a, 3), 64, 0.01, 1, mask)
    assert len(points) >= 6
    return a, points


def _errors(a, points, shift, levels, r):
    b = U.texture(W, H, shift=shift)
    q, status, _, _ = U.track(U.pyramid(a, levels), U.pyramid(b, levels), points, r, 10, min_eigen_threshold=U.MIN_EIGEN)
    return np.abs(q.astype(np.float64) - (points + np.array(shift))).max(axis=1), status


# the restatement's largest error over the selected features at shift (2.3, -1.6), L = 3, r = 7, measured on the CPU this test
# was written on: 0.0082 px (the bilinear template against the analytic texture). The bound is twice that.
MEASURED_MAX_ERROR = 0.0082


def test_restatement_recovers_a_known_shift():
    a, points = _selected()
    err, status = _errors(a, points, (2.3, -1.6), 3, 7)
    print(f"{len(points)} features, shift (2.3, -1.6), L = 3, r = 7: max error {err.max():.4g} px (bound {2 * MEASURED_MAX_ERROR:.4g})")
    assert (status == U.TRACKED).all() and err.max() <= 2 * MEASURED_MAX_ERROR


def test_the_pyramid_does_something():
    """A shift of 6 px, (4.8, 3.6), is about the strong sinusoids' wavelength over 2 to 1.5: one level with a 7 x 7 window
    ends several pixels off on every feature, three levels recover it."""
    a, points = _selected()
    one, _ = _errors(a, points, (4.8, 3.6), 1, 3)
    three, status = _errors(a, points, (4.8, 3.6), 3, 3)
    print(f"6 px shift, r = 3: L = 1 errors {np.round(one, 2).tolist()}; L = 3 max error {three.max():.3g}")
    assert one.min() > 3.0
    assert (status == U.TRACKED).all() and three.max() < 0.1


# ---- threshold margins of the GPU tests' inputs -----------------------------------------------------------------------------------
def _check_margins(label, want):
    _, status, _, margins = want
    edge, relative = min(m["edge"] for m in margins), min(m["relative"] for m in margins)
    print(f"{label}: status counts {np.bincount(status, minlength=6).tolist()}, smallest edge margin {edge:.3g} px, relative {relative:.3g}")
    assert edge >= U.EDGE_MARGIN and relative >= U.RELATIVE_MARGIN


@pytest.mark.parametrize("case", U.TRACK_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_track_case_margins(case):
    data = U.track_case(*case)
    assert len(data["points"]) == case[5]
    _check_margins(str(case), data["want"])
    if case[5] >= 64:   # the big sets hold tracked and lost features
        assert (data["want"][1] == U.TRACKED).sum() >= 8 and (data["want"][1] != U.TRACKED).sum() >= 1


@pytest.mark.parametrize("name", U.SPECIAL_CASES)
def test_special_case_margins(name):
    data = U.special_case(name)
    _, status, residual, _ = data["want"]
    _check_margins(name, data["want"])
    assert data["expect"] and all(status[k] == code for k, code in data["expect"].items())
    assert (status == U.TRACKED).any() and np.isfinite(data["want"][0]).all() and np.isfinite(residual).all()
    if name == "forward_backward":
        failed = status == U.FB_FAILED
        assert failed.sum() >= 2 and (status == U.TRACKED).sum() >= 2
        # the failures are the features whose window touches the occluding square (rows 20..41, columns 34..57)
        p = data["points"]
        near = (p[:, 0] > 34 - 4) & (p[:, 0] < 58 + 4) & (p[:, 1] > 20 - 4) & (p[:, 1] < 42 + 4)
        assert near[failed].all()


def test_small_image_skips_its_upper_levels():
    """17 x 13: with r = 3 no upper level holds a 9 x 9 template ring, with r = 1 level 1 (9 x 7) does and level 2 (5 x 4)
    does not; tracked features exist in both, so the skip carried the guess down."""
    for case in [c for c in U.TRACK_CASES if c[0] == 17 and c[3] == 3]:
        data = U.track_case(*case)
        sizes = [a.shape for a in data["pyr_a"]]
        assert sizes == [(13, 17), (7, 9), (4, 5)]
    big = U.track_case(17, 13, "still", 3, 1, 64)
    assert (big["want"][1] == U.TRACKED).sum() >= 8
