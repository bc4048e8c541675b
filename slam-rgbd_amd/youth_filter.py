"""Python host mirror of include/youth_filter.h (ctypes): the edge-preserving
depth filter in front of the ICP tracker.

``depth_filter_device`` filters torch int16 tensors on the GPU in place of the
caller (asynchronous on a stream); ``depth_filter_host`` takes numpy frames
through upload, filter and download.  The tracker's own use of the filter is
``youth_icp.IcpContext.set_depth_filter``.

Lives in libyouth_icp.so; no CPU fallback (a missing library raises, a machine
without a HIP device raises ``IcpError(YOUTH_ENODEV)``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_int, c_int16, c_void_p

import numpy as np

import youth_icp
from youth_icp import FilterParams

HEADER_PATH = os.path.join(os.path.dirname(youth_icp.HERE), "include", "youth_filter.h")

_PP = POINTER(FilterParams)
_SIGS = {
    "youth_depth_filter_default_params": (FilterParams, []),
    "youth_depth_filter_device": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, _PP,
                                          c_void_p]),
    "youth_depth_filter_host": (c_int, [c_int, POINTER(c_int16), POINTER(c_int16), c_int, c_int,
                                        c_int, _PP]),
    "youth_depth_filter_last_error": (c_char_p, []),
}


def load_library() -> ctypes.CDLL:
    return youth_icp.bind(youth_icp.load_library(), _SIGS)


def _check(lib, code: int) -> int:
    return youth_icp.check(code, lib.youth_depth_filter_last_error)


def default_params() -> tuple[int, int]:
    p = load_library().youth_depth_filter_default_params()
    return p.t0, p.t2


def _params(t0, t2):
    return None if t0 is None else ctypes.byref(FilterParams(int(t0), int(t2)))


def _shape(a) -> tuple[int, int, int]:
    if a.ndim == 2:
        return (1,) + tuple(a.shape)
    if a.ndim == 3:
        return tuple(a.shape)
    raise ValueError("depth: [H][W] or [n][H][W]")


def depth_filter_device(d_in, d_out=None, t0: int | None = 8, t2: int = 96, stream: int = 0):
    """youth_depth_filter_device on torch int16 tensors ([H][W] or [n][H][W],
    contiguous, on a HIP device).  ``d_out`` (same shape, must not overlap
    ``d_in``) is allocated when None; ``t0=None`` passes NULL (the defaults).
    Asynchronous on ``stream`` (a raw stream handle; 0: the default stream).
    Returns ``d_out``."""
    import torch

    lib = load_library()
    if d_in.dtype != torch.int16 or not d_in.is_cuda or not d_in.is_contiguous():
        raise ValueError("d_in: a contiguous int16 tensor on the GPU")
    if d_out is None:
        d_out = torch.empty_like(d_in)
    if (d_out.dtype != torch.int16 or d_out.device != d_in.device or not d_out.is_contiguous()
            or d_out.shape != d_in.shape):
        raise ValueError("d_out: a contiguous int16 tensor of d_in's shape and device")
    n, H, W = _shape(d_in)
    _check(lib, lib.youth_depth_filter_device(d_in.device.index or 0, d_in.data_ptr() or None,
                                              d_out.data_ptr() or None, n, W, H, _params(t0, t2),
                                              stream or None))
    return d_out


def depth_filter_host(depth: np.ndarray, t0: int | None = 8, t2: int = 96,
                      device: int = 0) -> np.ndarray:
    """youth_depth_filter_host: numpy int16 frames ([H][W] or [n][H][W]) ->
    the filtered frames; synchronous."""
    lib = load_library()
    d = np.ascontiguousarray(depth, np.int16)
    n, H, W = _shape(d)
    out = np.empty_like(d)
    _check(lib, lib.youth_depth_filter_host(device, d.ctypes.data_as(POINTER(c_int16)),
                                            out.ctypes.data_as(POINTER(c_int16)), n, W, H,
                                            _params(t0, t2)))
    return out
