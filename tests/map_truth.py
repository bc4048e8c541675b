"""CPU truth of the voxel map (include/youth_map.h), shared by
test_map.py and test_gpu_map.py: a numpy restatement of the map's definition.

World points come from the C oracle's viewer list (oracle.viewer_cloud with
T_world, negated: the display flip is exact); the key, q and clamp rules are
restated in np.float32; np.unique / np.add.at form the sums and np.lexsort the
(iz, iy, ix) order.  The restatement itself is pinned to a plain Python loop in
test_map.py."""
import numpy as np

import oracle
from youth_map import VOXEL_DTYPE

LIM = np.float32(1048576.0)


def frame_points(depth, rgb=None, K=None, T=None, max_depth=0):
    """(P [n,3] float32 world points, C [n,3] uint8 colours) of the
    contributing pixels of one frame, raster order.  K: an Intrinsics or None
    (viewer default); T: 3x4 / 4x4 camera -> world or None (identity)."""
    d = np.ascontiguousarray(depth, np.int16)
    v = oracle.viewer_cloud(d, None, None if K is None else K.as_tuple(),
                            T_world=None if T is None else np.asarray(T, np.float32))
    P = -v[:, :3]
    valid = d > 0
    dv = d[valid]
    C = (np.zeros((dv.size, 3), np.uint8) if rgb is None
         else np.ascontiguousarray(rgb, np.uint8).reshape(d.shape + (3,))[valid])
    if max_depth:
        keep = dv <= max_depth
        P, C = P[keep], C[keep]
    return np.ascontiguousarray(P, np.float32), C


def keys_of(P, vpm):
    """Per point: in-range mask, voxel index [n,3] int32 and q [n,3] uint32
    (the last two for the in-range points only)."""
    s = np.asarray(P, np.float32) * np.float32(vpm)
    fl = np.floor(s)
    with np.errstate(invalid="ignore"):
        ok = np.all((fl >= -LIM) & (fl < LIM), axis=1)     # NaN fails
    s, fl = s[ok], fl[ok]
    i = fl.astype(np.int32)
    f = (s - fl).astype(np.float32)
    q = np.minimum(np.uint32(255), (f * np.float32(256.0)).astype(np.uint32))
    return ok, i, q


def restate(P, C, vpm):
    """(records sorted by (iz, iy, ix), number of out-of-range points)."""
    ok, i, q = keys_of(P, vpm)
    c = np.asarray(C, np.uint8)[ok].astype(np.uint32)
    cells, inv = np.unique(i, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    n = cells.shape[0]
    rec = np.zeros(n, VOXEL_DTYPE)
    rec["ix"], rec["iy"], rec["iz"] = cells[:, 0], cells[:, 1], cells[:, 2]
    cnt = np.zeros(n, np.uint32)
    np.add.at(cnt, inv, 1)
    sq = np.zeros((n, 3), np.uint32)
    np.add.at(sq, inv, q)
    sc = np.zeros((n, 3), np.uint32)
    np.add.at(sc, inv, c)
    rec["count"], rec["sum_q"], rec["sum_c"] = cnt, sq, sc
    order = np.lexsort((rec["ix"], rec["iy"], rec["iz"]))
    return rec[order], int((~ok).sum())


def restate_frames(frames, vpm, max_depth=0):
    """frames: iterable of (depth, rgb, K, T)."""
    pts = [frame_points(d, c, K, T, max_depth) for d, c, K, T in frames]
    return restate(np.concatenate([p for p, _ in pts]), np.concatenate([c for _, c in pts]), vpm)


def derived_points(rec, vpm):
    """youth_map_points in numpy: fp64, rounded to fp32."""
    vpm = float(np.float32(vpm))
    cnt = rec["count"].astype(np.float64)
    out = np.zeros((rec.shape[0], 6), np.float32)
    for a, name in enumerate(("ix", "iy", "iz")):
        out[:, a] = ((rec[name].astype(np.float64)
                      + (rec["sum_q"][:, a].astype(np.float64) / cnt + 0.5) / 256.0) / vpm)
    out[:, 3:] = rec["sum_c"].astype(np.float64) / cnt[:, None] / 255.0
    return out
