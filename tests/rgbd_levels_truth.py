"""The level schedule of DESIGN.md §16 restated in numpy on top of
tests/rgbd_truth.py's align, which stays as it is: a level is that align on
plainly decimated frames under a camera divided by the stride, and a schedule
chains levels through their final fp64 poses.  CPU only.
"""
import numpy as np

import oracle
import rgbd_truth

f32 = np.float32
STRIDES = (1, 2, 4, 8, 16)
MAX_LEVELS = 4


def decimate(a, s):
    """out[..., j, i] = a[..., s j, s i]: W_s = (W + s - 1) // s, H_s likewise."""
    return np.ascontiguousarray(np.asarray(a)[..., ::s, ::s])


def level_K(K, s):
    """K_s = {fx / s, fy / s, cx / s, cy / s, depth_scale}: fp32 divisions by a
    power of two, hence exact."""
    K = oracle.K_of(K)
    d = f32(s)
    return oracle.OracleIntrinsics(f32(K.fx) / d, f32(K.fy) / d, f32(K.cx) / d, f32(K.cy) / d,
                                   K.depth_scale)


def default_levels(W, H):
    """youth_rgbd_default_levels."""
    for s in (8, 4, 2):
        if W // s >= 80 and H // s >= 60:
            return [(s, 10), (1, 10)]
    return [(1, 10)]


def check_schedule(levels, W, H):
    assert 1 <= len(levels) <= MAX_LEVELS
    for k, (s, it) in enumerate(levels):
        assert s in STRIDES and it >= 0
        assert k == 0 or s < levels[k - 1][0]
        assert (W + s - 1) // s >= 3 and (H + s - 1) // s >= 3


def align_levels(src, src_gray, dst, dst_gray, levels, K=None, dist_thresh=0.10, lam=0.1,
                 T_init=None):
    """-> (T64 [4,4], T32 [3,4], status, per_level) with per_level a list of
    rgbd_truth.align's (T64, T32, status, stats) of every level; the status is
    the OR of the levels'."""
    H, W = np.asarray(src).shape
    check_schedule(levels, W, H)
    K = oracle.K_of(K) if K is not None else oracle.viewer_K(W, H)
    T, status, per = T_init, 0, []
    for s, iters in levels:
        res = rgbd_truth.align(decimate(src, s), decimate(src_gray, s), decimate(dst, s),
                               decimate(dst_gray, s), K=level_K(K, s), iters=iters,
                               dist_thresh=dist_thresh, lam=lam, T_init=T)
        per.append(res)
        T = res[0]
        status |= res[2]
    return per[-1][0], per[-1][1], status, per


# The value of the schedule on two pairs of the C5 sequence at 160x120 under
# K160 = (142.575, 142.575, 80, 60, 1000), the later frame the source, lambda
# 0.1, schedule 2:10 -> 1:10 (degrees, millimetres against the ground truth).
# Bounds: 4x the errors measured for align_levels above, rounded up, the
# convention of rgbd_truth.BOUND_*.  From the identity (no schedule) both pairs
# end beyond IDENTITY_FLOOR.
K160 = (142.575, 142.575, 80.0, 60.0, 1000.0)
PAIR_REVISIT = (250, 868)     # target, source: 8.7 deg / 103 mm apart
PAIR_NEAR = (150, 155)
SCHEDULE_160 = [(2, 10), (1, 10)]
# measured: revisit 0.0040 deg / 0.153 mm (identity start 0.246 deg / 11.26 mm),
# near 0.0018 deg / 0.053 mm (identity start 0.096 deg / 2.09 mm)
BOUND_REVISIT = (0.016, 0.62)
BOUND_NEAR = (0.008, 0.22)
IDENTITY_FLOOR = (0.09, 2.0)
