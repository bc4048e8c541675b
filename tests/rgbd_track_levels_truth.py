"""The streaming tracker's level schedule restated in
numpy: every tracked pair, new frame i against frame i - 1, is
rgbd_levels_truth.align_levels of that pair from the identity, and the
sequence's pose is the product of the pairs'.  CPU only.
"""
import functools

import numpy as np

import rgbd_levels_truth as lt
import rgbd_truth
import youth_icp
import youth_synth

# Every tenth frame of the C5 sequence, 100 .. 200, at 160x120 under K160: pairs
# ten frames apart, what a streaming user sees after the queue has dropped frames
# or with a fast camera.
FRAMES = tuple(range(100, 201, 10))
SCHEDULE = [(2, 10), (1, 10)]
FLAT = [(1, 10)]              # the tracker without a schedule
# End pose (frame 200 in frame 100) against the ground truth, degrees and
# millimetres, measured for track() below: 0.54266 deg / 4.1612 mm with the
# schedule, 4.10763 deg / 100.9929 mm without; status 0 on every pair of both.
END_SCHEDULE = (0.543, 4.16)
END_FLAT = (4.108, 100.99)
# The bounds the tests hold both tracks to: the schedule within twice its
# measured error, the flat track beyond half of its own.
BOUND_SCHEDULE = (2 * END_SCHEDULE[0], 2 * END_SCHEDULE[1])
FLOOR_FLAT = (END_FLAT[0] / 2, END_FLAT[1] / 2)


@functools.lru_cache(maxsize=None)
def frames():
    """-> (depth [11][H][W], rgb [11][H][W][3], T_wc [11][4][4]), one call per frame."""
    K = youth_icp.Intrinsics(*lt.K160)
    got = [youth_synth.sequence_rgb(f, 1, 160, 120, K=K) for f in FRAMES]
    return (np.concatenate([g[0] for g in got]), np.concatenate([g[2] for g in got]),
            np.concatenate([g[1] for g in got]))


def compose(T_rel):
    """The pose of the last frame in the first: the product of the pairs' poses."""
    X = np.eye(4)
    for T in T_rel:
        X = X @ T
    return X


def end_error(T_rel):
    """(degrees, millimetres) of the composed pose against the ground truth."""
    X = frames()[2]
    return rgbd_truth.pose_error(compose(T_rel), np.linalg.inv(X[0]) @ X[-1])


@functools.lru_cache(maxsize=None)
def _track(levels):
    depth, rgb, _ = frames()
    gray = rgbd_truth.luma(rgb)
    K = youth_icp.Intrinsics(*lt.K160)
    T, st, per = [], [], []
    for i in range(1, len(FRAMES)):
        T64, _, s, p = lt.align_levels(depth[i], gray[i], depth[i - 1], gray[i - 1], list(levels), K=K)
        T.append(T64)
        st.append(s)
        per.append([(q[0], q[2]) for q in p])
    return np.array(T), np.array(st, np.int32), per


def track(levels):
    """-> (T_rel [10][4][4] with P_{i-1} = T_rel[i-1] P_i, OR status [10], per pair
    a list of every level's (T64, status)); computed once per schedule."""
    return _track(tuple(tuple(l) for l in levels))
