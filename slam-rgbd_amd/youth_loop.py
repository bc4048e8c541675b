"""Python host mirror of include/youth_loop.h (ctypes, no torch): loop closing
(DESIGN.md §15).

``LoopCloser`` keeps keyframes on the GPU, retrieves earlier keyframes that
look like a new one (an integer signature of 300 cells per frame), verifies
each candidate with the RGB-D alignment run forward and backward, and reports
the pairs that pass as edges.  ``optimize_pose_graph`` (host, fp64) spreads the
edges' corrections over the keyframe poses; ``interpolate`` re-hangs the frames
in between.

Lives in libyouth_icp.so; no CPU fallback (a missing library raises, a
machine without a HIP device raises ``IcpError(YOUTH_ENODEV)``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int16, c_int32, c_uint8, \
    c_uint32, c_void_p

import numpy as np

import youth_icp
import youth_rgbd
from youth_icp import YOUTH_EHIP, YOUTH_EINVAL, YOUTH_ENODEV, YOUTH_ENOMEM, IcpError, Intrinsics

HEADER_PATH = os.path.join(os.path.dirname(youth_icp.HERE), "include", "youth_loop.h")

GX, GY, CELLS = 20, 15, 300
MAX_KEYFRAMES = 512
MAX_CANDIDATES = 16

# youth_loop_edge
EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("Z", "<f8", (4, 4)), ("w", "<f8"),
                       ("overlap", "<f8"), ("gray_rms", "<f8"), ("fb_rot_deg", "<f8"),
                       ("fb_trans_m", "<f8")])
assert EDGE_DTYPE.itemsize == 176


class LoopParams(ctypes.Structure):
    """youth_loop_params."""
    _fields_ = [("min_gap", c_int), ("max_candidates", c_int), ("max_cell_dist", c_uint32),
                ("cap", c_uint32), ("ly", c_uint32), ("min_overlap", c_float),
                ("max_gray_rms", c_float), ("fb_rot_deg", c_float), ("fb_trans_m", c_float)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class PoseGraphParams(ctypes.Structure):
    """youth_posegraph_params."""
    _fields_ = [("w_rot", c_double), ("w_trans", c_double), ("max_iters", c_int)]


_PI, _PD, _PU32 = POINTER(Intrinsics), POINTER(c_double), POINTER(c_uint32)
_SIGS = {
    "youth_loop_default_params": (LoopParams, []),
    "youth_loop_create": (c_void_p, [c_int, c_int, c_int, c_int, _PI, POINTER(LoopParams)]),
    "youth_loop_destroy": (None, [c_void_p]),
    "youth_loop_last_error": (c_char_p, []),
    "youth_loop_signature_device": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                            c_void_p]),
    "youth_loop_distances": (c_int, [c_void_p, _PU32, c_int, _PU32]),
    "youth_loop_add_keyframe_device": (c_int, [c_void_p, c_void_p, c_void_p, _PD, c_uint32]),
    "youth_loop_add_keyframe_host": (c_int, [c_void_p, POINTER(c_int16), POINTER(c_uint8), _PD,
                                             c_uint32]),
    "youth_loop_candidates": (c_int, [c_void_p, c_int, c_int, POINTER(c_int), _PU32]),
    "youth_loop_close": (c_int, [c_void_p, c_int]),
    "youth_loop_set_levels": (c_int, [c_void_p, POINTER(youth_rgbd.RgbdLevel), c_int]),
    "youth_loop_get_levels": (c_int, [c_void_p, POINTER(youth_rgbd.RgbdLevel), c_int]),
    "youth_loop_last_verified": (c_int, [c_void_p, c_void_p, c_int]),
    "youth_loop_keyframes": (c_int, [c_void_p]),
    "youth_loop_edges": (c_int, [c_void_p, c_void_p, c_int]),
    "youth_loop_get_keyframe": (c_int, [c_void_p, c_int, _PD, _PU32]),
    "youth_loop_clear": (c_int, [c_void_p]),
    "youth_posegraph_default_params": (PoseGraphParams, []),
    "youth_posegraph_optimize": (c_int, [c_int, _PD, c_int, c_void_p, POINTER(PoseGraphParams), _PD,
                                         _PD]),
    "youth_posegraph_last_error": (c_char_p, []),
    "youth_posegraph_interpolate": (c_int, [c_int, _PD, c_int, POINTER(c_int32), _PD, _PD]),
    "youth_slam_loop_keyframes": (c_int, []),
    "youth_slam_loop_edges": (c_int, [c_void_p, c_int]),
    "youth_slam_loop_keyframe_frames": (c_int, [POINTER(c_int32), c_int]),
    "youth_slam_loop_trajectory": (c_int, [c_int, _PD]),
}


def load_library() -> ctypes.CDLL:
    return youth_icp.bind(youth_icp.load_library(), _SIGS)


def _check(lib, code: int) -> int:
    return youth_icp.check(code, lib.youth_loop_last_error)


def default_params() -> LoopParams:
    return load_library().youth_loop_default_params()


def _pose16(T) -> np.ndarray:
    out = np.zeros(16, np.float64)
    out[:12] = np.asarray(T, np.float64).reshape(-1)[:12]
    out[15] = 1.0
    return out


def make_edges(pairs) -> np.ndarray:
    """[(i, j, Z [4, 4], w), ...] -> EDGE_DTYPE records (the measures zero)."""
    e = np.zeros(len(pairs), EDGE_DTYPE)
    for k, (i, j, Z, w) in enumerate(pairs):
        e[k]["i"], e[k]["j"], e[k]["w"] = i, j, w
        e[k]["Z"] = np.asarray(Z, np.float64).reshape(4, 4)
    return e


def signature_device(d_depth: int, d_gray: int, n: int, W: int, H: int, d_sig: int,
                     device: int = 0, stream: int = 0) -> None:
    """youth_loop_signature_device on device pointers (ints); asynchronous."""
    lib = load_library()
    _check(lib, lib.youth_loop_signature_device(device, d_depth or None, d_gray or None, n, W, H,
                                                d_sig or None, stream or None))


def optimize_pose_graph(X, edges: np.ndarray, w_rot: float = 1.0, w_trans: float = 1.0,
                        max_iters: int = 20):
    """youth_posegraph_optimize: camera -> world poses X [n, 4, 4] and EDGE_DTYPE
    edges -> (X_opt [n, 4, 4], cost_before, cost_after).  Host only."""
    lib = load_library()
    Xo = np.array(X, np.float64).reshape(-1, 4, 4).copy()
    e = np.ascontiguousarray(edges, EDGE_DTYPE)
    P = PoseGraphParams(w_rot, w_trans, max_iters)
    c0, c1 = c_double(0.0), c_double(0.0)
    youth_icp.check(lib.youth_posegraph_optimize(Xo.shape[0], Xo.ctypes.data_as(_PD), e.shape[0],
                                                 e.ctypes.data, ctypes.byref(P), ctypes.byref(c0),
                                                 ctypes.byref(c1)),
                    lib.youth_posegraph_last_error)
    return Xo, c0.value, c1.value


def interpolate(X, kf_frame, X_kf_old, X_kf_new) -> np.ndarray:
    """youth_posegraph_interpolate: every frame re-hung on its preceding keyframe."""
    lib = load_library()
    Xo = np.array(X, np.float64).reshape(-1, 4, 4).copy()
    kf = np.ascontiguousarray(kf_frame, np.int32)
    a = np.ascontiguousarray(X_kf_old, np.float64).reshape(-1, 4, 4)
    b = np.ascontiguousarray(X_kf_new, np.float64).reshape(-1, 4, 4)
    if not a.shape[0] == b.shape[0] == kf.shape[0]:
        raise ValueError("interpolate: one old and one new pose per keyframe")
    youth_icp.check(lib.youth_posegraph_interpolate(Xo.shape[0], Xo.ctypes.data_as(_PD), kf.shape[0],
                                                    kf.ctypes.data_as(POINTER(c_int32)),
                                                    a.ctypes.data_as(_PD), b.ctypes.data_as(_PD)),
                    lib.youth_posegraph_last_error)
    return Xo


def slam_loop_keyframes() -> int:
    """Keyframes of the SLAM module's loop closer (0 without YOUTH_SLAM_LOOP=1)."""
    return int(load_library().youth_slam_loop_keyframes())


def slam_loop_keyframe_frames() -> np.ndarray:
    lib = load_library()
    out = np.zeros(MAX_KEYFRAMES, np.int32)
    m = lib.youth_slam_loop_keyframe_frames(out.ctypes.data_as(POINTER(c_int32)), out.shape[0])
    return out[:m]


def slam_loop_edges() -> np.ndarray:
    lib = load_library()
    n = lib.youth_slam_loop_edges(None, 0)
    out = np.zeros(max(n, 0), EDGE_DTYPE)
    if n > 0:
        n = min(n, lib.youth_slam_loop_edges(out.ctypes.data, out.shape[0]))
    return out[:max(n, 0)]


def slam_loop_trajectory() -> np.ndarray:
    """The corrected trajectory [n, 4, 4] (empty without YOUTH_SLAM_LOOP=1)."""
    lib = load_library()
    n = lib.youth_slam_trajectory_length()
    T = np.zeros((max(n, 1), 4, 4), np.float64)
    m = lib.youth_slam_loop_trajectory(n, T.ctypes.data_as(_PD))
    return T[:m]


class LoopCloser:
    """A keyframe store for ``max_keyframes`` frames of W x H on HIP device
    ``device`` (youth_loop_create); ``params``: keyword overrides of
    youth_loop_default_params."""

    def __init__(self, W: int, H: int, max_keyframes: int = 64, K: Intrinsics | None = None,
                 device: int = 0, **params):
        self._lib = load_library()
        self.W, self.H = W, H
        P = self._lib.youth_loop_default_params()
        for name, v in params.items():
            if name not in dict(P._fields_):
                raise TypeError(f"LoopCloser: no parameter {name!r}")
            setattr(P, name, v)
        self.params = P
        self._lp = self._lib.youth_loop_create(device, W, H, max_keyframes,
                                               None if K is None else ctypes.byref(K),
                                               ctypes.byref(P))
        if not self._lp:
            msg = (self._lib.youth_loop_last_error() or b"").decode()
            code = (YOUTH_ENODEV if "no HIP device" in msg else
                    YOUTH_ENOMEM if "allocation failed" in msg else
                    YOUTH_EHIP if "(line " in msg else YOUTH_EINVAL)
            raise IcpError(code, msg)

    def close_object(self):
        if getattr(self, "_lp", None):
            self._lib.youth_loop_destroy(self._lp)
            self._lp = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close_object()

    def __del__(self):
        self.close_object()

    def add_keyframe(self, depth: np.ndarray, rgb: np.ndarray, T_wc, tag: int = 0) -> int:
        """A host keyframe (depth int16 [H, W], rgb uint8 [H, W, 3]) -> its index."""
        d = np.ascontiguousarray(depth, np.int16).reshape(self.H, self.W)
        c = np.ascontiguousarray(rgb, np.uint8).reshape(self.H, self.W, 3)
        T = _pose16(T_wc)
        return _check(self._lib, self._lib.youth_loop_add_keyframe_host(
            self._lp, d.ctypes.data_as(POINTER(c_int16)), c.ctypes.data_as(POINTER(c_uint8)),
            T.ctypes.data_as(_PD), tag))

    def add_keyframe_device(self, d_depth: int, d_gray: int, T_wc, tag: int = 0) -> int:
        """Device pointers (ints): depth int16 [H, W] and intensity uint8 [H, W]."""
        T = _pose16(T_wc)
        return _check(self._lib, self._lib.youth_loop_add_keyframe_device(
            self._lp, d_depth or None, d_gray or None, T.ctypes.data_as(_PD), tag))

    def keyframes(self) -> int:
        return int(self._lib.youth_loop_keyframes(self._lp))

    def keyframe(self, kf: int):
        """-> (T_wc [4, 4], tag)."""
        T = np.zeros((4, 4), np.float64)
        tag = c_uint32(0)
        _check(self._lib, self._lib.youth_loop_get_keyframe(self._lp, kf, T.ctypes.data_as(_PD),
                                                            ctypes.byref(tag)))
        return T, tag.value

    def distances(self, sig_q: np.ndarray) -> np.ndarray:
        """Host records [nq, 300] uint32 against the stored keyframes -> D [nq, n_kf]."""
        q = np.ascontiguousarray(sig_q, np.uint32).reshape(-1, CELLS)
        D = np.zeros((q.shape[0], self.keyframes()), np.uint32)
        _check(self._lib, self._lib.youth_loop_distances(self._lp, q.ctypes.data_as(_PU32), q.shape[0],
                                                         D.ctypes.data_as(_PU32)))
        return D

    def candidates(self, kf: int, k: int = MAX_CANDIDATES):
        """-> (indices, distances) of keyframe kf's candidates, best first."""
        idx = np.zeros(max(k, 1), np.int32)
        dist = np.zeros(max(k, 1), np.uint32)
        m = _check(self._lib, self._lib.youth_loop_candidates(
            self._lp, kf, k, idx.ctypes.data_as(POINTER(c_int)), dist.ctypes.data_as(_PU32)))
        return idx[:m], dist[:m]

    def close(self, kf: int) -> int:
        """Retrieve and verify keyframe kf's candidates; returns the edges added."""
        return _check(self._lib, self._lib.youth_loop_close(self._lp, kf))

    def set_levels(self, levels) -> None:
        """Verify coarse to fine: [(stride, iters), ...] ending at stride 1
        (DESIGN.md §16); empty or None: off."""
        arr, n = youth_rgbd.level_array(levels)
        _check(self._lib, self._lib.youth_loop_set_levels(self._lp, arr, n))

    def levels(self) -> list[tuple[int, int]]:
        out = (youth_rgbd.RgbdLevel * youth_rgbd.MAX_LEVELS)()
        n = _check(self._lib, self._lib.youth_loop_get_levels(self._lp, out, youth_rgbd.MAX_LEVELS))
        return [(out[k].stride, out[k].iters) for k in range(n)]

    def last_verified(self) -> np.ndarray:
        """The measures of every candidate the last close verified (w: 1 accepted)."""
        out = np.zeros(MAX_CANDIDATES, EDGE_DTYPE)
        m = _check(self._lib, self._lib.youth_loop_last_verified(self._lp, out.ctypes.data,
                                                                 out.shape[0]))
        return out[:m]

    def edges(self) -> np.ndarray:
        n = _check(self._lib, self._lib.youth_loop_edges(self._lp, None, 0))
        out = np.zeros(n, EDGE_DTYPE)
        if n:
            _check(self._lib, self._lib.youth_loop_edges(self._lp, out.ctypes.data, n))
        return out

    def clear(self) -> None:
        _check(self._lib, self._lib.youth_loop_clear(self._lp))
