"""Python host mirror of include/youth_rectify.h (ctypes): the lens rectifier
(DESIGN.md §17).

``Rectifier`` resamples depth and colour frames taken through a lens with
Brown-Conrady distortion (k1 k2 p1 p2 k3, OpenCV order) into the frames of an
ideal pinhole camera: ``device`` on torch tensors (asynchronous on a stream),
``host`` on numpy frames, ``host_frames`` on separate per-frame numpy buffers in
place, ``map_device`` for the map as data.  ``parse_distortion_yaml`` reads the
coefficients of an ORB-SLAM3-style YAML.

Lives in libyouth_icp.so; no CPU fallback (a missing library raises, a machine
without a HIP device raises ``IcpError(YOUTH_ENODEV)``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int16, c_longlong, c_uint8, c_void_p

import numpy as np

import youth_icp
from youth_icp import Intrinsics

HEADER_PATH = os.path.join(os.path.dirname(youth_icp.HERE), "include", "youth_rectify.h")


class Distortion(ctypes.Structure):
    """youth_distortion: k1, k2, p1, p2, k3 (OpenCV order and meaning)."""
    _fields_ = [("k1", c_float), ("k2", c_float), ("p1", c_float), ("p2", c_float), ("k3", c_float)]

    def as_tuple(self):
        return (self.k1, self.k2, self.p1, self.p2, self.k3)


_PK, _PD = POINTER(Intrinsics), POINTER(Distortion)
_PP16, _PP8 = POINTER(POINTER(c_int16)), POINTER(POINTER(c_uint8))
_SIGS = {
    "youth_parse_camera_yaml_distortion": (c_int, [c_char_p, _PD]),
    "youth_rectify_create": (c_int, [c_int, c_int, c_int, _PK, _PD, _PK, POINTER(c_void_p)]),
    "youth_rectify_destroy": (None, [c_void_p]),
    "youth_rectify_covered": (c_longlong, [c_void_p]),
    "youth_rectify_map_device": (c_int, [c_void_p, c_void_p, c_void_p]),
    "youth_rectify_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                     c_void_p]),
    "youth_rectify_host": (c_int, [c_void_p, POINTER(c_int16), POINTER(c_int16), POINTER(c_uint8),
                                   POINTER(c_uint8), c_int, c_int]),
    "youth_rectify_host_frames": (c_int, [c_void_p, _PP16, _PP8, c_int]),
    "youth_rectify_last_error": (c_char_p, []),
    "youth_slam_rectify_active": (c_int, []),
}


def load_library() -> ctypes.CDLL:
    return youth_icp.bind(youth_icp.load_library(), _SIGS)


def _check(lib, code: int) -> int:
    return youth_icp.check(code, lib.youth_rectify_last_error)


def as_distortion(D) -> Distortion:
    return D if isinstance(D, Distortion) else Distortion(*[float(v) for v in D])


def parse_distortion_yaml(path: str):
    """Distortion from the YAML's Camera.k1 / k2 / p1 / p2 / k3 (a missing key
    is 0); None if unreadable."""
    D = Distortion()
    return D if load_library().youth_parse_camera_yaml_distortion(path.encode(), ctypes.byref(D)) else None


def slam_rectify_active() -> int:
    """1 while the SLAM module rectifies its frames (YOUTH_SLAM_RECTIFY=1 and a
    YAML with distortion)."""
    return load_library().youth_slam_rectify_active()


def _ptr(t):
    return t.data_ptr() if t is not None else None


class Rectifier:
    """youth_rectify: frames of ``width`` x ``height`` from the camera ``K``
    with distortion ``D`` (a Distortion or 5 numbers) to the pinhole camera
    ``Ko`` (None: ``K``)."""

    def __init__(self, width: int, height: int, K: Intrinsics, D, Ko: Intrinsics | None = None,
                 device: int = 0):
        self._lib = load_library()
        self._h = c_void_p()
        self.width, self.height, self.device = int(width), int(height), int(device)
        D = as_distortion(D)
        _check(self._lib, self._lib.youth_rectify_create(
            self.device, self.width, self.height, ctypes.byref(K), ctypes.byref(D),
            ctypes.byref(Ko) if Ko is not None else None, ctypes.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.youth_rectify_destroy(self._h)
            self._h = c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def covered(self) -> int:
        return int(self._lib.youth_rectify_covered(self._h))

    def map_device(self, d_map=None, stream: int = 0):
        """The map words, a torch int32 tensor [H][W][2] on the GPU (bit
        patterns of the uint32 words); allocated when None."""
        import torch

        if d_map is None:
            d_map = torch.empty((self.height, self.width, 2), dtype=torch.int32,
                                device=f"cuda:{self.device}")
        if (d_map.dtype != torch.int32 or not d_map.is_cuda or not d_map.is_contiguous()
                or tuple(d_map.shape) != (self.height, self.width, 2)):
            raise ValueError("d_map: a contiguous int32 tensor [H][W][2] on the GPU")
        _check(self._lib, self._lib.youth_rectify_map_device(self._h, d_map.data_ptr(), stream or None))
        return d_map

    def map(self) -> np.ndarray:
        """The map words as numpy uint32 [H][W][2]."""
        import torch

        m = self.map_device()
        torch.cuda.synchronize()
        return m.cpu().numpy().view(np.uint32)

    def _frames(self, depth, rgb):
        """(n, channels) of depth [n][H][W] / [H][W] and colour [n][H][W][c] /
        [H][W][c] / [n][H][W] (one channel: pass [n][H][W][1] or [H][W][1])."""
        H, W = self.height, self.width
        n = ch = None
        if depth is not None:
            s = tuple(depth.shape)
            if s[-2:] != (H, W) or len(s) not in (2, 3):
                raise ValueError("depth: [H][W] or [n][H][W]")
            n = 1 if len(s) == 2 else s[0]
        if rgb is not None:
            s = tuple(rgb.shape)
            if len(s) not in (3, 4) or s[-3:-1] != (H, W):
                raise ValueError("rgb: [H][W][c] or [n][H][W][c]")
            ch = s[-1]
            nc = 1 if len(s) == 3 else s[0]
            if n is not None and nc != n:
                raise ValueError("depth and rgb differ in their frame counts")
            n = nc
        return n or 0, ch or 0

    def device_frames(self, d_depth_in=None, d_depth_out=None, d_rgb_in=None, d_rgb_out=None,
                      stream: int = 0):
        """youth_rectify_device on torch tensors (contiguous, on the GPU): depth
        int16 [n][H][W], colour uint8 [n][H][W][c].  Outputs are allocated when
        None.  Asynchronous on ``stream``.  Returns (depth_out, rgb_out)."""
        import torch

        for t, dt, what in ((d_depth_in, torch.int16, "d_depth_in"), (d_rgb_in, torch.uint8, "d_rgb_in")):
            if t is not None and (t.dtype != dt or not t.is_cuda or not t.is_contiguous()):
                raise ValueError(f"{what}: a contiguous {dt} tensor on the GPU")
        n, ch = self._frames(d_depth_in, d_rgb_in)
        if d_depth_in is not None and d_depth_out is None:
            d_depth_out = torch.empty_like(d_depth_in)
        if d_rgb_in is not None and d_rgb_out is None:
            d_rgb_out = torch.empty_like(d_rgb_in)
        for i, o in ((d_depth_in, d_depth_out), (d_rgb_in, d_rgb_out)):
            if i is not None and (o.dtype != i.dtype or o.device != i.device or not o.is_contiguous()
                                  or o.shape != i.shape):
                raise ValueError("an output: a contiguous tensor of its input's type, shape and device")
        _check(self._lib, self._lib.youth_rectify_device(
            self._h, _ptr(d_depth_in), _ptr(d_depth_out), _ptr(d_rgb_in), _ptr(d_rgb_out), ch, n,
            stream or None))
        return d_depth_out, d_rgb_out

    def host(self, depth: np.ndarray | None = None, rgb: np.ndarray | None = None, in_place: bool = False):
        """youth_rectify_host: numpy frames -> (depth_out, rgb_out), either
        None with its input; ``in_place`` writes into the (contiguous) inputs."""
        d = None if depth is None else np.ascontiguousarray(depth, np.int16)
        c = None if rgb is None else np.ascontiguousarray(rgb, np.uint8)
        n, ch = self._frames(d, c)
        if in_place and ((d is not None and d is not depth) or (c is not None and c is not rgb)):
            raise ValueError("in_place needs contiguous int16 / uint8 inputs")
        do = d if in_place else (None if d is None else np.empty_like(d))
        co = c if in_place else (None if c is None else np.empty_like(c))
        _check(self._lib, self._lib.youth_rectify_host(
            self._h, youth_icp._p(d, c_int16), youth_icp._p(do, c_int16), youth_icp._p(c, c_uint8),
            youth_icp._p(co, c_uint8), ch, n))
        return do, co

    def host_frames(self, depth: list, rgb: list | None = None) -> None:
        """youth_rectify_host_frames: separate per-frame numpy buffers (int16
        [H][W], uint8 [H][W][3], contiguous), rectified in place."""
        n = len(depth)
        for a in depth:
            if a.dtype != np.int16 or not a.flags.c_contiguous or a.shape != (self.height, self.width):
                raise ValueError("depth frames: contiguous int16 [H][W]")
        if rgb is not None:
            if len(rgb) != n:
                raise ValueError("depth and rgb differ in their frame counts")
            for a in rgb:
                if a.dtype != np.uint8 or not a.flags.c_contiguous or a.shape != (self.height, self.width, 3):
                    raise ValueError("rgb frames: contiguous uint8 [H][W][3]")
        dp = (POINTER(c_int16) * max(n, 1))(*[a.ctypes.data_as(POINTER(c_int16)) for a in depth])
        cp = None
        if rgb is not None:
            cp = (POINTER(c_uint8) * max(n, 1))(*[a.ctypes.data_as(POINTER(c_uint8)) for a in rgb])
        _check(self._lib, self._lib.youth_rectify_host_frames(self._h, dp, cp, n))
