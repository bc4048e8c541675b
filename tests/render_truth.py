"""CPU truth of the map render (include/youth_map_render.h),
shared by test_render.py and test_gpu_render.py: a numpy restatement of the
definition over extracted records (VOXEL_DTYPE).

Everything is np.float32 with one rounding per operation, in the order the
header writes it; the z-buffer is np.minimum.at on the packed int64 value
(depth << 24 | R << 16 | G << 8 | B; depth <= 32767, so it stays positive).
The restatement itself is pinned to a plain Python loop in test_render.py."""
import numpy as np

F = np.float32
FAR = np.int64(np.iinfo(np.int64).max)


def view_from_pose(T_world):
    """youth_map_view_from_pose in fp64: [3, 4] float32 world -> camera."""
    T = np.asarray(T_world, np.float64).reshape(-1)[:12].reshape(3, 4)
    V = np.zeros((3, 4), np.float64)
    V[:, :3] = T[:, :3].T
    for r in range(3):
        V[r, 3] = -((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3])
    return V.astype(np.float32)


def project(rec, vpm, V, K, W, H, max_splat=16, min_count=1, why=None):
    """Per surviving voxel: (u0, v0, s, value) as int64 arrays; the footprint is
    [u0, u0+s) x [v0, v0+s) before clipping.  `why` (a dict) receives how many
    voxels each rule removed."""
    V = np.asarray(V, np.float32).reshape(3, 4)
    vpm = F(vpm)
    fx, fy, cx, cy, ds = (F(a) for a in K.as_tuple())
    rec = rec[rec["count"] >= max(1, min_count)]
    fc = rec["count"].astype(np.float32)
    p = []
    for a, name in enumerate(("ix", "iy", "iz")):
        c = rec["sum_q"][:, a].astype(np.float32) / fc
        p.append((rec[name].astype(np.float32) + (c + F(0.5)) * F(0.00390625)) / vpm)
    with np.errstate(all="ignore"):
        cam = [((V[r, 0] * p[0] + V[r, 1] * p[1]) + V[r, 2] * p[2]) + V[r, 3] for r in range(3)]
        xc, yc, zc = cam
        df = np.rint(zc * ds)
        uf = (xc * fx) / zc + cx
        vf = (yc * fy) / zc + cy
        keep = (zc > 0) & (df >= 1) & (df <= 32767)                     # NaN fails
        keep &= (uf > -32) & (uf < F(W + 32)) & (vf > -32) & (vf < F(H + 32))
        sf = np.minimum(np.maximum(np.ceil(fx / (vpm * zc)), F(1.0)), F(max_splat))
    assert all(a.dtype == np.float32 for a in (xc, yc, zc, df, uf, vf, sf))
    if why is not None:
        front = zc > 0
        why.update(behind=int((~front).sum()),
                   d_zero=int((front & (df < 1)).sum()), d_far=int((front & (df > 32767)).sum()),
                   off_frame=int((front & (df >= 1) & (df <= 32767) & ~keep).sum()))
    rec, df, uf, vf, sf = rec[keep], df[keep], uf[keep], vf[keep], sf[keep]
    s = sf.astype(np.int64)
    h = F(0.5) * (s - 1).astype(np.float32)
    u0 = np.floor((uf - h) + F(0.5)).astype(np.int64)
    v0 = np.floor((vf - h) + F(0.5)).astype(np.int64)
    cnt = rec["count"].astype(np.uint32)
    col = (rec["sum_c"].astype(np.uint32) + (cnt // 2)[:, None]) // cnt[:, None]
    val = (df.astype(np.int64) << 24) | (col[:, 0].astype(np.int64) << 16) | \
          (col[:, 1].astype(np.int64) << 8) | col[:, 2].astype(np.int64)
    return u0, v0, s, val


def candidates(u0, v0, s, val, W, H):
    """Every (pixel index, value) pair the footprints put forward, clipped."""
    pix, vals = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for dy in range(int(s.max()) if s.size else 0):
        for dx in range(int(s.max())):
            x, y = u0 + dx, v0 + dy
            on = (dx < s) & (dy < s) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            pix.append(y[on] * W + x[on])
            vals.append(val[on])
    return np.concatenate(pix), np.concatenate(vals)


def render(rec, vpm, V, K, W, H, max_splat=16, min_count=1):
    """(depth [H, W] int16, rgb [H, W, 3] uint8) of the records seen through V."""
    u0, v0, s, val = project(rec, vpm, V, K, W, H, max_splat or 16, min_count or 1)
    z = np.full(W * H, FAR, np.int64)
    np.minimum.at(z, *candidates(u0, v0, s, val, W, H))
    hit = z != FAR
    depth = np.where(hit, z >> 24, 0).astype(np.int16).reshape(H, W)
    rgb = np.zeros((W * H, 3), np.uint8)
    for j, sh in enumerate((16, 8, 0)):
        rgb[:, j] = np.where(hit, (z >> sh) & 255, 0)
    return depth, rgb.reshape(H, W, 3)
