"""Python host mirror of include/youth_map.h (ctypes, no torch): the voxel map,
world-frame point fusion of tracked frames.

``VoxelMap`` accumulates every integrated frame's world points in a sparse
voxel grid on the GPU.  A voxel is a 40-byte record of integers
(``VOXEL_DTYPE``); the map is the same bit pattern for any launch shape, frame
order or split of the frames over calls.  ``points`` and ``write_ply`` are the
derived float forms, computed on the host.

Lives in libyouth_icp.so; no CPU fallback (a missing library raises, a
machine without a HIP device raises ``IcpError(YOUTH_ENODEV)``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int16, c_longlong, c_uint8, \
    c_uint32, c_uint64, c_void_p

import numpy as np

import youth_icp
from youth_icp import YOUTH_EHIP, YOUTH_EINVAL, YOUTH_ENODEV, YOUTH_ENOMEM, IcpError, Intrinsics

HEADER_PATH = os.path.join(os.path.dirname(youth_icp.HERE), "include", "youth_map.h")
REMOVE_HEADER_PATH = os.path.join(os.path.dirname(youth_icp.HERE), "include", "youth_map_remove.h")

# youth_voxel
VOXEL_DTYPE = np.dtype([("ix", "<i4"), ("iy", "<i4"), ("iz", "<i4"), ("count", "<u4"),
                        ("sum_q", "<u4", (3,)), ("sum_c", "<u4", (3,))])
assert VOXEL_DTYPE.itemsize == 40


class MapStats(ctypes.Structure):
    """struct youth_map_stats."""
    _fields_ = [("integrated", c_uint64), ("out_of_range", c_uint64), ("dropped", c_uint64),
                ("occupied", c_uint64), ("direct", c_uint64), ("capacity", c_uint64)]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class MapRemoveStats(ctypes.Structure):
    """struct youth_map_remove_stats."""
    _fields_ = [("removed", c_uint64), ("missing", c_uint64), ("underflow", c_uint64),
                ("live", c_uint64), ("vacant", c_uint64), ("stale", c_uint64)]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class MapView(ctypes.Structure):
    """struct youth_map_view (youth_map_render.h); 0 = the default for the last two."""
    _fields_ = [("W", c_int), ("H", c_int), ("max_splat", c_int), ("min_count", c_uint32)]


_PI, _PV = POINTER(Intrinsics), POINTER(MapView)
_SIGS = {
    "youth_map_create": (c_void_p, [c_int, c_float, c_longlong]),
    "youth_map_destroy": (None, [c_void_p]),
    "youth_map_last_error": (c_char_p, []),
    "youth_map_clear": (c_int, [c_void_p]),
    "youth_map_set_max_depth": (c_int, [c_void_p, c_int]),
    "youth_map_integrate_device": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, _PI,
                                           c_void_p, c_void_p]),
    "youth_map_integrate_host": (c_int, [c_void_p, POINTER(c_int16), POINTER(c_uint8), c_int,
                                         c_int, _PI, POINTER(c_double)]),
    # youth_map_remove.h
    "youth_map_remove_device": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, _PI,
                                        c_void_p, c_void_p]),
    "youth_map_remove_host": (c_int, [c_void_p, POINTER(c_int16), POINTER(c_uint8), c_int, c_int,
                                      _PI, POINTER(c_double)]),
    "youth_map_move_device": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, _PI,
                                      c_void_p, c_void_p, c_void_p]),
    "youth_map_compact": (c_int, [c_void_p]),
    "youth_map_remove_stats": (c_int, [c_void_p, POINTER(MapRemoveStats)]),
    "youth_map_voxels": (c_longlong, [c_void_p]),
    "youth_map_extract": (c_int, [c_void_p, c_void_p, c_int]),
    "youth_map_stats": (c_int, [c_void_p, POINTER(MapStats)]),
    "youth_map_sync": (c_int, [c_void_p, c_void_p]),
    "youth_map_points": (c_int, [c_void_p, c_int, c_float, POINTER(c_float)]),
    "youth_map_write_ply": (c_int, [c_char_p, c_void_p, c_int, c_float]),
    "youth_slam_map_voxels": (c_longlong, []),
    "youth_slam_map_extract": (c_int, [c_void_p, c_int]),
    "youth_slam_map_vpm": (c_float, []),
    "youth_slam_map_reintegrate": (c_int, [c_int, POINTER(c_double)]),
    "youth_slam_map_kept": (c_int, []),
    # youth_map_render.h
    "youth_map_view_from_pose": (c_int, [POINTER(c_double), POINTER(c_float)]),
    "youth_map_render_device": (c_int, [c_void_p, c_int, _PV, _PI, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "youth_map_render_host": (c_int, [c_void_p, _PV, _PI, POINTER(c_double), POINTER(c_int16),
                                      POINTER(c_uint8)]),
    "youth_slam_map_render": (c_int, [_PV, _PI, POINTER(c_double), POINTER(c_int16),
                                      POINTER(c_uint8)]),
}


def load_library() -> ctypes.CDLL:
    return youth_icp.bind(youth_icp.load_library(), _SIGS)


def _check(lib, code: int) -> int:
    return youth_icp.check(code, lib.youth_map_last_error)


def _records(voxels: np.ndarray) -> np.ndarray:
    v = np.ascontiguousarray(voxels, VOXEL_DTYPE)
    if v.ndim != 1:
        raise ValueError("voxels: a 1-D array of VOXEL_DTYPE records")
    return v


def points(voxels: np.ndarray, vpm: float) -> np.ndarray:
    """youth_map_points: records -> [n, 6] float32 {x, y, z, r, g, b} (host only)."""
    lib = load_library()
    v = _records(voxels)
    out = np.empty((v.shape[0], 6), np.float32)
    _check(lib, lib.youth_map_points(v.ctypes.data, v.shape[0], vpm,
                                     out.ctypes.data_as(POINTER(c_float))))
    return out


def write_ply(path: str, voxels: np.ndarray, vpm: float) -> None:
    """youth_map_write_ply: ASCII PLY, one vertex per record (host only)."""
    lib = load_library()
    v = _records(voxels)
    _check(lib, lib.youth_map_write_ply(os.fsencode(path), v.ctypes.data, v.shape[0], vpm))


def slam_map_voxels() -> int:
    """Voxels in the SLAM module's map (0 when YOUTH_SLAM_MAP_VPM was not set)."""
    return int(load_library().youth_slam_map_voxels())


def slam_map_vpm() -> float:
    return float(load_library().youth_slam_map_vpm())


def slam_map_extract() -> np.ndarray:
    """The SLAM module's map, sorted by (iz, iy, ix)."""
    lib = load_library()
    while True:
        n = int(lib.youth_slam_map_voxels())
        out = np.zeros(n, VOXEL_DTYPE)
        m = lib.youth_slam_map_extract(out.ctypes.data, n)
        if m == YOUTH_EINVAL and int(lib.youth_slam_map_voxels()) > n:
            continue   # the worker integrated a frame in between
        return out[:_check(lib, m)]


def slam_map_kept() -> int:
    """Frames in the SLAM module's frame store (YOUTH_SLAM_MAP_KEEP; 0 when off)."""
    return int(load_library().youth_slam_map_kept())


def slam_map_reintegrate(T_wc) -> int:
    """youth_slam_map_reintegrate: the kept frames i < n moved to T_wc[i] (n poses,
    4x4 fp64, e.g. youth_loop.slam_loop_trajectory); returns the number of frames
    whose pose changed (0 when the map or the store is off)."""
    lib = load_library()
    T = np.ascontiguousarray(T_wc, np.float64).reshape(-1, 16)
    return _check(lib, lib.youth_slam_map_reintegrate(T.shape[0], T.ctypes.data_as(POINTER(c_double))))


def _pose16(T_world) -> np.ndarray:
    """A 4x4 or 3x4 pose as 16 fp64 values, last row 0 0 0 1."""
    T = np.zeros(16, np.float64)
    T[:12] = np.asarray(T_world, np.float64).reshape(-1)[:12]
    T[15] = 1.0
    return T


def view_from_pose(T_world) -> np.ndarray:
    """youth_map_view_from_pose: camera -> world (4x4 or 3x4 fp64) to the
    world -> camera view matrix, [3, 4] float32 (host only)."""
    lib = load_library()
    T = _pose16(T_world)
    V = np.zeros((3, 4), np.float32)
    _check(lib, lib.youth_map_view_from_pose(T.ctypes.data_as(POINTER(c_double)),
                                             V.ctypes.data_as(POINTER(c_float))))
    return V


def slam_map_render(W: int, H: int, T_world=None, K: Intrinsics | None = None, max_splat: int = 0,
                    min_count: int = 0, want_rgb: bool = True):
    """youth_slam_map_render: the SLAM module's map seen from T_world (None: the
    last recorded pose) -> (depth [H, W] int16, rgb [H, W, 3] uint8 or None), or
    None when the module keeps no map (or has no pose yet)."""
    lib = load_library()
    view = MapView(W, H, max_splat, min_count)
    depth = np.zeros((H, W), np.int16)
    rgb = np.zeros((H, W, 3), np.uint8) if want_rgb else None
    T = None if T_world is None else _pose16(T_world)
    ok = lib.youth_slam_map_render(
        ctypes.byref(view), None if K is None else ctypes.byref(K),
        None if T is None else T.ctypes.data_as(POINTER(c_double)),
        depth.ctypes.data_as(POINTER(c_int16)),
        None if rgb is None else rgb.ctypes.data_as(POINTER(c_uint8)))
    return (depth, rgb) if ok == 1 else None


class VoxelMap:
    """A map of ``vpm`` voxels per metre with ``slots`` hash slots (rounded up
    to a power of two) on HIP device ``device`` (youth_map_create)."""

    def __init__(self, vpm: float, slots: int = 1 << 20, device: int = 0):
        self._lib = load_library()
        self.vpm = float(np.float32(vpm))
        self._map = self._lib.youth_map_create(device, vpm, slots)
        if not self._map:
            msg = (self._lib.youth_map_last_error() or b"").decode()
            code = (YOUTH_ENODEV if "no HIP device" in msg else
                    YOUTH_ENOMEM if "allocation failed" in msg else
                    YOUTH_EHIP if "(line " in msg else YOUTH_EINVAL)
            raise IcpError(code, msg)

    def close(self):
        if getattr(self, "_map", None):
            self._lib.youth_map_destroy(self._map)
            self._map = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    def clear(self) -> None:
        _check(self._lib, self._lib.youth_map_clear(self._map))

    def set_max_depth(self, max_depth: int) -> None:
        """Pixels deeper than max_depth (raw units) do not contribute; 0 = no gate."""
        _check(self._lib, self._lib.youth_map_set_max_depth(self._map, max_depth))

    def integrate(self, depth: np.ndarray, rgb: np.ndarray | None = None,
                  K: Intrinsics | None = None, T_world: np.ndarray | None = None) -> None:
        """One host frame with its camera -> world pose (4x4 or 3x4, fp64; None =
        identity); synchronous."""
        self._host_frame(self._lib.youth_map_integrate_host, depth, rgb, K, T_world)

    def remove(self, depth: np.ndarray, rgb: np.ndarray | None = None,
               K: Intrinsics | None = None, T_world: np.ndarray | None = None) -> None:
        """youth_map_remove_host: takes out a frame that went in with the same
        arguments (exact iff they are bit-identical and nothing was dropped);
        synchronous."""
        self._host_frame(self._lib.youth_map_remove_host, depth, rgb, K, T_world)

    def _host_frame(self, fn, depth, rgb, K, T_world) -> None:
        d = np.ascontiguousarray(depth, np.int16)
        H, W = d.shape
        c = None if rgb is None else np.ascontiguousarray(rgb, np.uint8).reshape(H, W, 3)
        T = None
        if T_world is not None:
            T = np.zeros(16, np.float64)
            T[:12] = np.asarray(T_world, np.float64).reshape(-1)[:12]
            T[15] = 1.0
        _check(self._lib, fn(
            self._map, d.ctypes.data_as(POINTER(c_int16)),
            None if c is None else c.ctypes.data_as(POINTER(c_uint8)), W, H,
            None if K is None else ctypes.byref(K),
            None if T is None else T.ctypes.data_as(POINTER(c_double))))

    def integrate_device(self, d_depth: int, d_rgb: int, n_frames: int, W: int, H: int,
                         d_T_world: int = 0, K: Intrinsics | None = None,
                         stream: int = 0) -> None:
        """Device pointers (ints, e.g. torch data_ptr()); d_T_world = device
        [n_frames][12] fp32 poses (0: identity); asynchronous on `stream` (0: the
        map's own stream)."""
        _check(self._lib, self._lib.youth_map_integrate_device(
            self._map, d_depth or None, d_rgb or None, n_frames, W, H,
            None if K is None else ctypes.byref(K), d_T_world or None, stream or None))

    def remove_device(self, d_depth: int, d_rgb: int, n_frames: int, W: int, H: int,
                      d_T_world: int = 0, K: Intrinsics | None = None, stream: int = 0) -> None:
        """youth_map_remove_device: as integrate_device, taking the frames out."""
        _check(self._lib, self._lib.youth_map_remove_device(
            self._map, d_depth or None, d_rgb or None, n_frames, W, H,
            None if K is None else ctypes.byref(K), d_T_world or None, stream or None))

    def move_device(self, d_depth: int, d_rgb: int, n_frames: int, W: int, H: int, d_T_old: int,
                    d_T_new: int, K: Intrinsics | None = None, stream: int = 0) -> None:
        """youth_map_move_device: the frames from the poses d_T_old to d_T_new (device
        [n_frames][12] fp32 each); a frame with bitwise equal poses is skipped."""
        _check(self._lib, self._lib.youth_map_move_device(
            self._map, d_depth or None, d_rgb or None, n_frames, W, H,
            None if K is None else ctypes.byref(K), d_T_old or None, d_T_new or None,
            stream or None))

    def compact(self) -> None:
        """youth_map_compact: rebuild the table without the slots removal vacated."""
        _check(self._lib, self._lib.youth_map_compact(self._map))

    def remove_stats(self) -> dict:
        """youth_map_remove_stats: removed / missing / underflow since the last clear,
        live / vacant / stale from a scan of the table."""
        st = MapRemoveStats()
        _check(self._lib, self._lib.youth_map_remove_stats(self._map, ctypes.byref(st)))
        return st.as_dict()

    def render(self, T_world=None, W: int = 640, H: int = 480, K: Intrinsics | None = None,
               max_splat: int = 0, min_count: int = 0, want_rgb: bool = True):
        """The map seen from the camera -> world pose T_world (4x4 or 3x4 fp64;
        None = identity) -> (depth [H, W] int16, rgb [H, W, 3] uint8 or None);
        synchronous (youth_map_render_host)."""
        view = MapView(W, H, max_splat, min_count)
        depth = np.zeros((max(H, 0), max(W, 0)), np.int16)
        rgb = np.zeros((max(H, 0), max(W, 0), 3), np.uint8) if want_rgb else None
        T = None if T_world is None else _pose16(T_world)
        _check(self._lib, self._lib.youth_map_render_host(
            self._map, ctypes.byref(view), None if K is None else ctypes.byref(K),
            None if T is None else T.ctypes.data_as(POINTER(c_double)),
            depth.ctypes.data_as(POINTER(c_int16)),
            None if rgb is None else rgb.ctypes.data_as(POINTER(c_uint8))))
        return depth, rgb

    def render_device(self, d_V: int, d_depth: int, d_rgb: int, n_views: int, W: int, H: int,
                      K: Intrinsics | None = None, max_splat: int = 0, min_count: int = 0,
                      stream: int = 0) -> None:
        """Device pointers (ints): d_V [n_views][12] fp32 world -> camera,
        d_depth [n][H][W] int16, d_rgb [n][H][W][3] uint8 (0: depth only);
        asynchronous on `stream` (0: the map's own stream)."""
        view = MapView(W, H, max_splat, min_count)
        _check(self._lib, self._lib.youth_map_render_device(
            self._map, n_views, ctypes.byref(view), None if K is None else ctypes.byref(K),
            d_V or None, d_depth or None, d_rgb or None, stream or None))

    def voxels(self) -> int:
        return int(_check(self._lib, self._lib.youth_map_voxels(self._map)))

    def extract(self) -> np.ndarray:
        """The map's records (VOXEL_DTYPE) sorted by (iz, iy, ix)."""
        n = self.voxels()
        out = np.zeros(n, VOXEL_DTYPE)
        m = _check(self._lib, self._lib.youth_map_extract(self._map, out.ctypes.data, n))
        return out[:m]

    def points(self) -> np.ndarray:
        """The derived float map: [n, 6] float32 {x, y, z, r, g, b}."""
        return points(self.extract(), self.vpm)

    def stats(self) -> dict:
        st = MapStats()
        _check(self._lib, self._lib.youth_map_stats(self._map, ctypes.byref(st)))
        return st.as_dict()

    def write_ply(self, path: str) -> int:
        """The map as an ASCII PLY; returns the vertex count."""
        v = self.extract()
        write_ply(path, v, self.vpm)
        return int(v.shape[0])

    def sync(self, stream: int = 0) -> None:
        _check(self._lib, self._lib.youth_map_sync(self._map, stream or None))
