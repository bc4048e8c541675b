"""Python host mirror of include/youth_rgbd.h (ctypes): RGB-D alignment, a
photometric term beside point-to-plane ICP.

``RgbdContext`` owns the device workspace.  Its device entry points take torch
tensors (int16 depth, uint8 intensity) and run asynchronously; the host entry
points take numpy frames.  Lives in libyouth_icp.so; no CPU fallback (a missing
library raises, a machine without a HIP device raises
``IcpError(YOUTH_ENODEV)``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int16, c_int32, c_uint8, c_void_p

import numpy as np

import youth_icp
from youth_icp import IcpError, Intrinsics

HEADER_PATH = os.path.join(os.path.dirname(youth_icp.HERE), "include", "youth_rgbd.h")
NEQ = 31
PHOTO_VALID = 0x80000000


class RgbdParams(ctypes.Structure):
    _fields_ = [("iters", c_int), ("dist_thresh", c_float), ("lam", c_float)]


class RgbdLevel(ctypes.Structure):
    """youth_rgbd_level."""
    _fields_ = [("stride", c_int), ("iters", c_int)]


MAX_LEVELS = 4  # YOUTH_RGBD_MAX_LEVELS

_PD = POINTER(c_double)
_SIGS = {
    "youth_rgbd_default_levels": (c_int, [c_int, c_int, POINTER(RgbdLevel)]),
    "youth_rgbd_set_levels": (c_int, [c_void_p, POINTER(RgbdLevel), c_int]),
    "youth_rgbd_get_levels": (c_int, [c_void_p, POINTER(RgbdLevel), c_int]),
    "youth_rgbd_get_level_poses": (c_int, [c_void_p, c_int, c_int, _PD, POINTER(c_int32)]),
    "youth_rgbd_get_level_stats": (c_int, [c_void_p, c_int, c_int, c_int, _PD]),
    "youth_rgbd_decimate_device": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                           c_void_p, c_void_p, c_void_p]),
    "youth_rgbd_default_params": (RgbdParams, []),
    "youth_rgbd_last_error": (c_char_p, []),
    "youth_rgbd_create": (c_void_p, [c_int, c_int, c_int, c_int, POINTER(Intrinsics),
                                     POINTER(RgbdParams)]),
    "youth_rgbd_destroy": (None, [c_void_p]),
    "youth_rgbd_luma_device": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                       c_void_p]),
    "youth_rgbd_align_pairs_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_int, _PD, c_void_p, c_void_p]),
    "youth_rgbd_align_sequence_device": (c_int, [c_void_p, c_void_p, c_void_p, c_int,
                                                 c_void_p, c_void_p]),
    "youth_rgbd_sync": (c_int, [c_void_p, c_void_p]),
    "youth_rgbd_get_poses": (c_int, [c_void_p, c_int, _PD, POINTER(c_float),
                                     POINTER(c_int32)]),
    "youth_rgbd_get_stats": (c_int, [c_void_p, c_int, c_int, _PD]),
    "youth_rgbd_prep_device": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p,
                                       c_void_p, c_void_p]),
    "youth_rgbd_reduce_host": (c_int, [c_void_p, POINTER(c_int16), POINTER(c_uint8),
                                       POINTER(c_int16), POINTER(c_uint8),
                                       POINTER(c_float), _PD]),
    "youth_rgbd_track_host_sequence": (c_int, [c_void_p, POINTER(c_int16),
                                               POINTER(c_uint8), c_int, _PD,
                                               POINTER(c_int32)]),
    "youth_rgbd_track_set_batch": (c_int, [c_void_p, c_int]),
    "youth_rgbd_track_set_depth_filter": (c_int, [c_void_p, POINTER(youth_icp.FilterParams)]),
    "youth_rgbd_track_submit": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_int]),
    "youth_rgbd_track_collect": (c_int, [c_void_p, _PD, POINTER(c_int)]),
    "youth_rgbd_track_pending": (c_int, [c_void_p]),
    "youth_rgbd_track_reset": (c_int, [c_void_p]),
    "youth_rgbd_pull_host": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_int,
                                     c_void_p, c_void_p, c_void_p, c_void_p]),
    "youth_rgbd_track_set_levels": (c_int, [c_void_p, POINTER(RgbdLevel), c_int]),
    "youth_rgbd_track_get_levels": (c_int, [c_void_p, POINTER(RgbdLevel), c_int]),
    "youth_rgbd_track_last_levels": (c_int, [c_void_p, _PD, POINTER(c_int32)]),
}


def load_library() -> ctypes.CDLL:
    return youth_icp.bind(youth_icp.load_library(), _SIGS)


def _last_error(lib) -> str:
    return (lib.youth_rgbd_last_error() or b"").decode()


def _check(lib, code: int) -> int:
    return youth_icp.check(code, lib.youth_rgbd_last_error)


def default_params() -> tuple[int, float, float]:
    p = load_library().youth_rgbd_default_params()
    return p.iters, p.dist_thresh, p.lam


def unpack_photo(words: np.ndarray):
    """A packed photometric word array -> (Y, gx, gy, valid)."""
    w = np.asarray(words, np.uint32)
    return ((w & 255).astype(np.uint8), ((w >> 8) & 511).astype(np.int32) - 255,
            ((w >> 17) & 511).astype(np.int32) - 255, (w & PHOTO_VALID) != 0)


def _ptr(t):
    return None if t is None else (t.data_ptr() or None)


def luma_device(d_rgb, d_gray=None, stream: int = 0):
    """youth_rgbd_luma_device on torch uint8 tensors: [n][H][W][3] (or
    [H][W][3]) -> [n][H][W]; asynchronous on ``stream``.  Returns ``d_gray``."""
    import torch

    lib = load_library()
    if d_rgb.dtype != torch.uint8 or not d_rgb.is_cuda or not d_rgb.is_contiguous() \
            or d_rgb.shape[-1] != 3 or d_rgb.ndim not in (3, 4):
        raise ValueError("d_rgb: a contiguous uint8 [n][H][W][3] tensor on the GPU")
    if d_gray is None:
        d_gray = torch.empty(d_rgb.shape[:-1], dtype=torch.uint8, device=d_rgb.device)
    if d_gray.dtype != torch.uint8 or d_gray.device != d_rgb.device or not d_gray.is_contiguous() \
            or tuple(d_gray.shape) != tuple(d_rgb.shape[:-1]):
        raise ValueError("d_gray: a contiguous uint8 tensor of d_rgb's frames and device")
    n = 1 if d_rgb.ndim == 3 else d_rgb.shape[0]
    H, W = d_rgb.shape[-3], d_rgb.shape[-2]
    _check(lib, lib.youth_rgbd_luma_device(d_rgb.device.index or 0, _ptr(d_rgb), _ptr(d_gray), n,
                                           W, H, stream or None))
    return d_gray


def level_array(levels):
    """[(stride, iters), ...] -> (a ctypes array of youth_rgbd_level or None, its length)."""
    lv = [tuple(int(v) for v in l) for l in (levels or ())]
    if not lv:
        return None, 0
    return (RgbdLevel * len(lv))(*[RgbdLevel(s, it) for s, it in lv]), len(lv)


def parse_levels(text: str, W: int, H: int):
    """``auto`` -> default_levels(W, H); ``8:10,1:10`` -> [(8, 10), (1, 10)];
    empty or ``none`` -> [] (the tools' --levels option)."""
    if not text or text == "none":
        return []
    if text == "auto":
        return default_levels(W, H)
    return [tuple(int(v) for v in item.split(":")) for item in text.split(",")]


def default_levels(W: int, H: int) -> list[tuple[int, int]]:
    """youth_rgbd_default_levels -> [(stride, iters), ...]."""
    lib = load_library()
    out = (RgbdLevel * MAX_LEVELS)()
    n = _check(lib, lib.youth_rgbd_default_levels(W, H, out))
    return [(out[k].stride, out[k].iters) for k in range(n)]


def decimate_device(d_depth, d_gray, n: int, W: int, H: int, stride: int, d_depth_out,
                    d_gray_out, device: int = 0, stream: int = 0) -> None:
    """youth_rgbd_decimate_device on device pointers (ints): [n][H][W] int16 /
    uint8 -> [n][H_s][W_s]; asynchronous on ``stream``."""
    lib = load_library()
    _check(lib, lib.youth_rgbd_decimate_device(device, d_depth or None, d_gray or None, n, W, H,
                                               stride, d_depth_out or None, d_gray_out or None,
                                               stream or None))


class PinnedColor:
    """One page-locked RGB frame [H][W][3] uint8 (a youth_icp_host_alloc buffer)
    as a numpy view; ``youth_icp.PinnedFrame`` is its depth counterpart."""

    def __init__(self, height: int, width: int):
        self._lib = youth_icp.load_library()
        n = height * width * 3
        self.ptr = self._lib.youth_icp_host_alloc((n + 1) // 2)
        if not self.ptr:
            raise IcpError(youth_icp.YOUTH_ENOMEM, "youth_icp_host_alloc failed")
        raw = np.ctypeslib.as_array(ctypes.cast(self.ptr, POINTER(c_uint8)), shape=(n,))
        self.array = raw.reshape(height, width, 3)

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            self._lib.youth_icp_host_free(self.ptr)
            self.ptr = None

    __del__ = close


def _frame_ptrs(frames, dtype, shape, what):
    """(c_void_p array, the arrays it points into) of host frames used in place."""
    keep = []
    for f in frames:
        if f is None:
            keep.append(None)
            continue
        if not isinstance(f, np.ndarray) or f.dtype != dtype or f.shape != shape \
                or not f.flags["C_CONTIGUOUS"]:
            raise ValueError(f"{what}: C-contiguous {np.dtype(dtype).name} arrays of shape {shape}")
        keep.append(f)
    arr = (c_void_p * max(len(keep), 1))(*[None if f is None else f.ctypes.data for f in keep])
    return arr, keep


class RgbdContext:
    """Device workspace for max_frames pairs of W x H (youth_rgbd_create)."""

    def __init__(self, width: int, height: int, max_frames: int, K: Intrinsics | None = None,
                 iters: int = 10, dist_thresh: float = 0.10, lam: float = 0.1, device: int = 0):
        self._lib = load_library()
        self.W, self.H, self.max_frames, self.iters = width, height, max_frames, iters
        self.K = K if K is not None else youth_icp.default_intrinsics(width, height)
        self.params = RgbdParams(iters, dist_thresh, lam)
        self._ctx = self._lib.youth_rgbd_create(device, width, height, max_frames,
                                                ctypes.byref(self.K), ctypes.byref(self.params))
        if not self._ctx:
            msg = _last_error(self._lib)
            code = (youth_icp.YOUTH_ENODEV if "no HIP device" in msg
                    else youth_icp.YOUTH_EINVAL if ": bad " in msg else youth_icp.YOUTH_EHIP)
            raise IcpError(code, msg)

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.youth_rgbd_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    # ---- device entry points (torch tensors) ----
    def align_pairs_device(self, d_src_depth, d_src_gray, d_dst_depth, d_dst_gray, n_pairs=None,
                           T_init=None, d_T_out=None, stream: int = 0):
        n = d_src_depth.shape[0] if n_pairs is None else n_pairs
        Ti = None
        if T_init is not None:
            Ti = np.ascontiguousarray(T_init, np.float64).reshape(-1, 16)
        _check(self._lib, self._lib.youth_rgbd_align_pairs_device(
            self._ctx, _ptr(d_src_depth), _ptr(d_src_gray), _ptr(d_dst_depth), _ptr(d_dst_gray), n,
            None if Ti is None else Ti.ctypes.data_as(POINTER(c_double)), _ptr(d_T_out),
            stream or None))

    def align_sequence_device(self, d_depth, d_gray, n_frames=None, d_T_out=None, stream: int = 0):
        n = d_depth.shape[0] if n_frames is None else n_frames
        _check(self._lib, self._lib.youth_rgbd_align_sequence_device(
            self._ctx, _ptr(d_depth), _ptr(d_gray), n, _ptr(d_T_out), stream or None))

    def prep_device(self, d_in, channels: int, n: int, d_gray=None, d_photo=None, stream: int = 0):
        _check(self._lib, self._lib.youth_rgbd_prep_device(
            self._ctx, _ptr(d_in), channels, n, _ptr(d_gray), _ptr(d_photo), stream or None))

    def sync(self, stream: int = 0):
        _check(self._lib, self._lib.youth_rgbd_sync(self._ctx, stream or None))

    def poses(self, n: int):
        """-> (T64 [n,4,4], T32 [n,4,4], status [n]) of the last align."""
        T64 = np.zeros((n, 4, 4), np.float64)
        T32 = np.zeros((n, 4, 4), np.float32)
        st = np.zeros(n, np.int32)
        _check(self._lib, self._lib.youth_rgbd_get_poses(
            self._ctx, n, T64.ctypes.data_as(POINTER(c_double)),
            T32.ctypes.data_as(POINTER(c_float)), st.ctypes.data_as(POINTER(c_int32))))
        T64[:, 3, :] = (0.0, 0.0, 0.0, 1.0)
        return T64, T32, st

    def stats(self, n: int, iters: int | None = None):
        """-> [n, iters, 4]: sum r^2, geometric count, sum rp^2, photometric count."""
        iters = self.iters if iters is None else iters
        out = np.zeros((n, iters, 4), np.float64)
        _check(self._lib, self._lib.youth_rgbd_get_stats(self._ctx, n, iters,
                                                         out.ctypes.data_as(POINTER(c_double))))
        return out

    # ---- level schedule ----
    def set_levels(self, levels) -> None:
        """[(stride, iters), ...], coarse to fine; empty or None: off."""
        arr, n = level_array(levels)
        _check(self._lib, self._lib.youth_rgbd_set_levels(self._ctx, arr, n))

    def levels(self) -> list[tuple[int, int]]:
        out = (RgbdLevel * MAX_LEVELS)()
        n = _check(self._lib, self._lib.youth_rgbd_get_levels(self._ctx, out, MAX_LEVELS))
        return [(out[k].stride, out[k].iters) for k in range(n)]

    def level_poses(self, level: int, n: int):
        """-> (T64 [n,4,4], status [n]) of one level of the last scheduled align."""
        T64 = np.zeros((n, 4, 4), np.float64)
        st = np.zeros(n, np.int32)
        _check(self._lib, self._lib.youth_rgbd_get_level_poses(
            self._ctx, level, n, T64.ctypes.data_as(POINTER(c_double)),
            st.ctypes.data_as(POINTER(c_int32))))
        T64[:, 3, :] = (0.0, 0.0, 0.0, 1.0)
        return T64, st

    def level_stats(self, level: int, n: int, iters: int):
        """-> [n, iters, 4] of one level, as ``stats``."""
        out = np.zeros((n, iters, 4), np.float64)
        _check(self._lib, self._lib.youth_rgbd_get_level_stats(
            self._ctx, level, n, iters, out.ctypes.data_as(POINTER(c_double))))
        return out

    # ---- host entry points (numpy frames) ----
    def reduce_host(self, src_depth, src_gray, dst_depth, dst_gray, T12) -> np.ndarray:
        s = np.ascontiguousarray(src_depth, np.int16)
        d = np.ascontiguousarray(dst_depth, np.int16)
        sg = np.ascontiguousarray(src_gray, np.uint8)
        dg = np.ascontiguousarray(dst_gray, np.uint8)
        for a in (s, d, sg, dg):
            if a.shape != (self.H, self.W):
                raise ValueError("frames: [H][W] of the context's size")
        T = np.ascontiguousarray(np.asarray(T12, np.float32).reshape(-1)[:12])
        out = np.zeros(NEQ, np.float64)
        _check(self._lib, self._lib.youth_rgbd_reduce_host(
            self._ctx, s.ctypes.data_as(POINTER(c_int16)), sg.ctypes.data_as(POINTER(c_uint8)),
            d.ctypes.data_as(POINTER(c_int16)), dg.ctypes.data_as(POINTER(c_uint8)),
            T.ctypes.data_as(POINTER(c_float)), out.ctypes.data_as(POINTER(c_double))))
        return out

    def track_host_sequence(self, depth, rgb):
        """-> (T_rel [n-1,4,4] fp64 with P_k = T_rel[k] P_{k+1}, status [n-1])."""
        d = np.ascontiguousarray(depth, np.int16)
        c = np.ascontiguousarray(rgb, np.uint8)
        n = d.shape[0]
        if d.shape != (n, self.H, self.W) or c.shape != (n, self.H, self.W, 3):
            raise ValueError("depth [n][H][W] and rgb [n][H][W][3] of the context's size")
        T = np.zeros((max(n - 1, 0), 4, 4), np.float64)
        st = np.zeros(max(n - 1, 0), np.int32)
        _check(self._lib, self._lib.youth_rgbd_track_host_sequence(
            self._ctx, d.ctypes.data_as(POINTER(c_int16)), c.ctypes.data_as(POINTER(c_uint8)), n,
            T.ctypes.data_as(POINTER(c_double)), st.ctypes.data_as(POINTER(c_int32))))
        return T, st

    # ---- streaming tracker (host frames, used in place) ----
    def track_set_batch(self, b: int) -> int:
        return _check(self._lib, self._lib.youth_rgbd_track_set_batch(self._ctx, b))

    def track_set_depth_filter(self, t0: int | None = 8, t2: int = 96):
        """``t0=None`` switches the filter off."""
        P = None if t0 is None else ctypes.byref(youth_icp.FilterParams(t0, t2))
        _check(self._lib, self._lib.youth_rgbd_track_set_depth_filter(self._ctx, P))

    def track_set_levels(self, levels) -> None:
        """The tracker's own schedule [(stride, iters), ...], coarse to fine, the
        last stride 1; empty or None: off."""
        arr, n = level_array(levels)
        _check(self._lib, self._lib.youth_rgbd_track_set_levels(self._ctx, arr, n))

    def track_levels(self) -> list[tuple[int, int]]:
        out = (RgbdLevel * MAX_LEVELS)()
        n = _check(self._lib, self._lib.youth_rgbd_track_get_levels(self._ctx, out, MAX_LEVELS))
        return [(out[k].stride, out[k].iters) for k in range(n)]

    def track_last_levels(self):
        """-> (T64 [n_levels,4,4], status [n_levels]) of the frame collected last
        (n_levels 0: it had no reference, or no schedule is set)."""
        T64 = np.zeros((MAX_LEVELS, 4, 4), np.float64)
        st = np.zeros(MAX_LEVELS, np.int32)
        n = _check(self._lib, self._lib.youth_rgbd_track_last_levels(
            self._ctx, T64.ctypes.data_as(POINTER(c_double)), st.ctypes.data_as(POINTER(c_int32))))
        return T64[:n], st[:n]

    def track_submit(self, depth, rgb):
        """Lists of [H][W] int16 and [H][W][3] uint8 frames, read in place: they
        stay unchanged (and are kept alive here) until collected."""
        if len(depth) != len(rgb):
            raise ValueError("as many colour frames as depth frames")
        dp, kd = _frame_ptrs(depth, np.int16, (self.H, self.W), "depth")
        cp, kc = _frame_ptrs(rgb, np.uint8, (self.H, self.W, 3), "rgb")
        _check(self._lib, self._lib.youth_rgbd_track_submit(self._ctx, dp, cp, len(depth)))
        self._held = getattr(self, "_held", [])
        self._held.extend(zip(kd, kc))

    def track_collect(self):
        """-> (T_rel [4,4] fp64 with P_ref = T_rel P_new, has_ref, status)."""
        T = np.zeros((4, 4), np.float64)
        has = c_int(0)
        st = _check(self._lib, self._lib.youth_rgbd_track_collect(
            self._ctx, T.ctypes.data_as(POINTER(c_double)), ctypes.byref(has)))
        if getattr(self, "_held", None):
            self._held.pop(0)
        return T, has.value, st

    def track_pending(self) -> int:
        return self._lib.youth_rgbd_track_pending(self._ctx)

    def track_reset(self):
        _check(self._lib, self._lib.youth_rgbd_track_reset(self._ctx))

    def pull_host(self, depth, rgb, d_depth, d_gray, d_rgb=None, stream: int = 0):
        """youth_rgbd_pull_host: host frame lists -> torch tensors on the GPU
        (int16 [m][H][W], uint8 [m][H][W], optional uint8 [m][H][W][3]);
        asynchronous on ``stream``: keep the frames alive until it has run."""
        if len(depth) != len(rgb):
            raise ValueError("as many colour frames as depth frames")
        dp, _kd = _frame_ptrs(depth, np.int16, (self.H, self.W), "depth")
        cp, _kc = _frame_ptrs(rgb, np.uint8, (self.H, self.W, 3), "rgb")
        _check(self._lib, self._lib.youth_rgbd_pull_host(
            self._ctx, dp, cp, len(depth), _ptr(d_depth), _ptr(d_gray), _ptr(d_rgb),
            stream or None))
