"""ctypes wrapper of the synthetic depth source (include/youth_synth.h).

Stands in for the reference's Astra SensorModule (sensorModule.c:69-264):
produces int16 [H][W] millimetre depth frames, 0 = invalid.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_double, c_int, c_int16, c_uint8, c_uint64

import numpy as np

from youth_icp import HERE, Intrinsics

LIB_PATH = os.path.join(HERE, "libyouth_synth.so")
PAIR_SEED = 0x5EED0000
SEQ_SEED = 0x5EED1000
NOISE = 1
HOLES = 2
NOISE_SURVEY = 4   # SURVEY §8d sigma = 1.5 mm * Z^2 (instead of NOISE's 0.25)
SURVEY_FLAGS = NOISE_SURVEY | HOLES
DEFAULT_FLAGS = NOISE | HOLES

_lib = None


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise OSError(f"{path} not built: run `make -C {HERE}`")
    lib = ctypes.CDLL(path)
    P16, PD, PK = POINTER(c_int16), POINTER(c_double), POINTER(Intrinsics)
    lib.youth_synth_render.argtypes = [PD, c_int, c_int, PK, c_uint64, c_int, P16]
    lib.youth_synth_render.restype = None
    lib.youth_synth_pair.argtypes = [c_uint64, c_int, c_int, PK, c_int, P16, P16, PD]
    lib.youth_synth_pair.restype = None
    lib.youth_synth_pairs.argtypes = [c_uint64, c_int, c_int, c_int, c_int, PK, c_int, P16, P16,
                                      PD]
    lib.youth_synth_pairs.restype = None
    lib.youth_synth_sequence.argtypes = [c_uint64, c_int, c_int, c_int, c_int, PK, c_int, P16,
                                         PD]
    lib.youth_synth_sequence.restype = None
    P8 = POINTER(c_uint8)
    lib.youth_synth_render_rgb.argtypes = [PD, c_int, c_int, PK, c_uint64, c_int, P16, P8]
    lib.youth_synth_render_rgb.restype = None
    lib.youth_synth_pairs_rgb.argtypes = [c_uint64, c_int, c_int, c_int, c_int, PK, c_int, P16,
                                          P16, PD, P8, P8]
    lib.youth_synth_pairs_rgb.restype = None
    lib.youth_synth_sequence_rgb.argtypes = [c_uint64, c_int, c_int, c_int, c_int, PK, c_int,
                                             P16, PD, P8]
    lib.youth_synth_sequence_rgb.restype = None
    _lib = lib
    return lib


def viewer_intrinsics(width: int, height: int) -> Intrinsics:
    """viewerModule.c:343-345 convention without loading the HIP library."""
    return Intrinsics(570.3, 570.3, float(width // 2), float(height // 2), 1000.0)


def _p(a, t):
    return a.ctypes.data_as(POINTER(t))


def pairs(first_index: int, n: int, width: int = 640, height: int = 480, K=None,
          flags: int = DEFAULT_FLAGS, base_seed: int = PAIR_SEED):
    """n pairs with seeds base_seed + first_index + p -> (src, dst, T_gt)."""
    K = K if K is not None else viewer_intrinsics(width, height)
    src = np.zeros((n, height, width), np.int16)
    dst = np.zeros((n, height, width), np.int16)
    T = np.zeros((n, 4, 4), np.float64)
    load_library().youth_synth_pairs(base_seed, first_index, n, width, height,
                                     ctypes.byref(K), flags, _p(src, c_int16),
                                     _p(dst, c_int16), _p(T, c_double))
    return src, dst, T


def sequence(first_frame: int, n: int, width: int = 640, height: int = 480, K=None,
             flags: int = DEFAULT_FLAGS, seed: int = SEQ_SEED):
    """Frames [first_frame, first_frame+n) of the synthetic sequence -> (frames, T_wc)."""
    K = K if K is not None else viewer_intrinsics(width, height)
    frames = np.zeros((n, height, width), np.int16)
    T = np.zeros((n, 4, 4), np.float64)
    load_library().youth_synth_sequence(seed, first_frame, n, width, height, ctypes.byref(K),
                                        flags, _p(frames, c_int16), _p(T, c_double))
    return frames, T


def render(T_wc: np.ndarray, width: int, height: int, K=None, noise_seed: int = 0,
           flags: int = 0):
    K = K if K is not None else viewer_intrinsics(width, height)
    T = np.ascontiguousarray(T_wc, np.float64)
    out = np.zeros((height, width), np.int16)
    load_library().youth_synth_render(_p(T, c_double), width, height, ctypes.byref(K),
                                      noise_seed, flags, _p(out, c_int16))
    return out


def pairs_rgb(first_index: int, n: int, width: int = 640, height: int = 480, K=None,
              flags: int = DEFAULT_FLAGS, base_seed: int = PAIR_SEED):
    """pairs() with colour -> (src, dst, T_gt, src_rgb, dst_rgb); rgb uint8 [n][H][W][3]."""
    K = K if K is not None else viewer_intrinsics(width, height)
    src = np.zeros((n, height, width), np.int16)
    dst = np.zeros((n, height, width), np.int16)
    T = np.zeros((n, 4, 4), np.float64)
    src_rgb = np.zeros((n, height, width, 3), np.uint8)
    dst_rgb = np.zeros((n, height, width, 3), np.uint8)
    load_library().youth_synth_pairs_rgb(base_seed, first_index, n, width, height,
                                         ctypes.byref(K), flags, _p(src, c_int16),
                                         _p(dst, c_int16), _p(T, c_double), _p(src_rgb, c_uint8),
                                         _p(dst_rgb, c_uint8))
    return src, dst, T, src_rgb, dst_rgb


def sequence_rgb(first_frame: int, n: int, width: int = 640, height: int = 480, K=None,
                 flags: int = DEFAULT_FLAGS, seed: int = SEQ_SEED):
    """sequence() with colour -> (frames, T_wc, rgb); rgb uint8 [n][H][W][3]."""
    K = K if K is not None else viewer_intrinsics(width, height)
    frames = np.zeros((n, height, width), np.int16)
    T = np.zeros((n, 4, 4), np.float64)
    rgb = np.zeros((n, height, width, 3), np.uint8)
    load_library().youth_synth_sequence_rgb(seed, first_frame, n, width, height,
                                            ctypes.byref(K), flags, _p(frames, c_int16),
                                            _p(T, c_double), _p(rgb, c_uint8))
    return frames, T, rgb


def render_rgb(T_wc: np.ndarray, width: int, height: int, K=None, noise_seed: int = 0,
               flags: int = 0):
    """render() with colour -> (depth, rgb)."""
    K = K if K is not None else viewer_intrinsics(width, height)
    T = np.ascontiguousarray(T_wc, np.float64)
    out = np.zeros((height, width), np.int16)
    rgb = np.zeros((height, width, 3), np.uint8)
    load_library().youth_synth_render_rgb(_p(T, c_double), width, height, ctypes.byref(K),
                                          noise_seed, flags, _p(out, c_int16), _p(rgb, c_uint8))
    return out, rgb


def render_distorted_rgb(T_wc: np.ndarray, width: int, height: int, K, D, noise_seed: int = 0,
                          flags: int = 0):
    """render_rgb() through a lens with distortion D (a youth_rectify.Distortion
    or k1, k2, p1, p2, k3) -> (depth, rgb); a pixel the lens model's inverse
    does not reach is 0 in both."""
    from youth_rectify import as_distortion

    lib = load_library()
    D = as_distortion(D)
    lib.youth_synth_render_distorted_rgb.argtypes = [
        POINTER(c_double), c_int, c_int, POINTER(Intrinsics), POINTER(type(D)), c_uint64, c_int,
        POINTER(c_int16), POINTER(c_uint8)]
    lib.youth_synth_render_distorted_rgb.restype = None
    T = np.ascontiguousarray(T_wc, np.float64)
    out = np.zeros((height, width), np.int16)
    rgb = np.zeros((height, width, 3), np.uint8)
    lib.youth_synth_render_distorted_rgb(_p(T, c_double), width, height, ctypes.byref(K),
                                         ctypes.byref(D), noise_seed, flags, _p(out, c_int16),
                                         _p(rgb, c_uint8))
    return out, rgb


def luma(rgb: np.ndarray) -> np.ndarray:
    """Y = (77 R + 150 G + 29 B + 128) >> 8, uint8."""
    c = np.asarray(rgb, np.uint8).astype(np.int32)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)
