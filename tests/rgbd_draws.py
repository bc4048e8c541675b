"""Seeded camera draws for the RGB-D tests away from the viewer's fx == fy:
tests/test_rgbd.py pins the numpy truth on them, tests/test_gpu_rgbd_fuzz.py
runs the GPU path on them.  CPU only.

A camera is the tuple (fx, fy, cx, cy, depth_scale) of float32 values, which
oracle.K_of and rgbd_truth take as it is; intrinsics() makes the library's
struct of it.
"""
import numpy as np

import youth_icp

f32 = np.float32
SEED = 112   # chosen on the host so that the conditions test_gpu_rgbd_fuzz.py asserts hold
RATIOS = (0.6, 0.75, 1.3, 1.6)            # fy / fx: never 1
DEPTH_SCALES = (1000.0, 5000.0, 1000.5)   # the fast-division check decides per camera
FAR_CX = 5.23                             # 160 x 120: a principal point far to one side


def camera_draws(W, H, n=6):
    """n cameras for W x H: fx in [300, 900] W / 640, fy = fx times each of
    RATIOS in turn, the principal point in the middle 40 % of the frame with a
    fractional part, the depth scales in turn.  At 160 x 120 one more, with cx
    far to one side: the aligned loop's exactness guard (icp_api.cpp
    centred_exact) refuses it."""
    rng = np.random.default_rng(SEED + 1000 * W + H)
    out = []
    for d in range(n):
        fx = f32(rng.uniform(300.0, 900.0) * W / 640.0)
        fy = f32(fx * f32(RATIOS[d % 4]))
        cx = f32(rng.uniform(0.3, 0.7) * W)
        cy = f32(rng.uniform(0.3, 0.7) * H)
        out.append(tuple(float(v) for v in (fx, fy, cx, cy, f32(DEPTH_SCALES[d % 3]))))
    if (W, H) == (160, 120):
        fx, fy, _, cy, ds = out[0]
        out.append((fx, fy, float(f32(FAR_CX)), cy, ds))
    for k in out:
        assert k[0] != k[1] and k[2] != int(k[2]) and k[3] != int(k[3])
    return out


def intrinsics(k):
    return youth_icp.Intrinsics(*k)


def centred_exact(cx, W):
    """icp_api.cpp centred_exact in numpy float32: whether ((u & ~3) - cx) +
    (u & 3) equals u - cx for every column."""
    u = np.arange(W)
    cx = f32(cx)
    a = u.astype(f32) - cx
    b = ((u & ~3).astype(f32) - cx) + (u & 3).astype(f32)
    return bool(np.array_equal(a, b))
