"""The RGB-D alignment of DESIGN.md §13 restated in numpy: the checker of the
GPU path (youth_rgbd.h) and of the definition's own accuracy.  CPU only.

The geometric term is spec a7/a8 in the survey arithmetic, written as in
tests/test_oracle_numpy.py: numpy float32, one rounding per operation, no
contraction, IEEE division.  Back-projection and normals (a2, a6) come from
the C oracle, which that file pins bit for bit.  The photometric term follows
§13 word for word.  The 31 sums are exact float64 products added in pixel
order, a pixel's geometric products before its photometric ones (np.cumsum).
"""
import numpy as np

import oracle

f32, f64 = np.float32, np.float64
NEQ = 31


def luma(rgb):
    """Y = (77 R + 150 G + 29 B + 128) >> 8, uint8 [..., H, W]."""
    c = np.asarray(rgb, np.uint8).astype(np.int32)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def photo_record(gray):
    """-> (gx, gy, valid): central differences of Y, 0 and invalid on the
    1-px border."""
    y = np.asarray(gray, np.uint8).astype(np.int32)
    H, W = y.shape
    gx = np.zeros((H, W), np.int32)
    gy = np.zeros((H, W), np.int32)
    valid = np.zeros((H, W), bool)
    valid[1:H - 1, 1:W - 1] = True
    gx[1:H - 1, 1:W - 1] = y[1:H - 1, 2:] - y[1:H - 1, :W - 2]
    gy[1:H - 1, 1:W - 1] = y[2:, 1:W - 1] - y[:H - 2, 1:W - 1]
    return gx, gy, valid


def photo_consts(lam, K):
    w = f32(lam) / f32(255.0)
    return w, (f32(0.5) * w) * f32(K.fx), (f32(0.5) * w) * f32(K.fy)


def terms(src, src_gray, dst, dst_gray, T12, K=None, dist_thresh=0.10, lam=0.1):
    """Per matched pixel, in raster order of the source: the geometric (J, r)
    and the photometric (Jp, rp, pvalid) as float32 arrays."""
    src = np.ascontiguousarray(src, np.int16)
    dst = np.ascontiguousarray(dst, np.int16)
    H, W = src.shape
    K = oracle.K_of(K) if K is not None else oracle.viewer_K(W, H)
    sx, sy, sz = (a.ravel() for a in oracle.backproject(src, K))
    tP = oracle.backproject(dst, K)
    tX, tY, tZ = (a.ravel() for a in tP)
    nX, nY, nZ = (a.ravel() for a in oracle.normals(*tP))
    T = np.asarray(T12, f32).ravel()[:12]
    fx, fy, cx, cy = f32(K.fx), f32(K.fy), f32(K.cx), f32(K.cy)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        qx = ((T[0] * sx + T[1] * sy) + T[2] * sz) + T[3]
        qy = ((T[4] * sx + T[5] * sy) + T[6] * sz) + T[7]
        qz = ((T[8] * sx + T[9] * sy) + T[10] * sz) + T[11]
        ok = (sz > 0) & (qz > 0)
        uf = (fx * qx) / qz + cx
        vf = (fy * qy) / qz + cy
        fu = np.floor(uf + f32(0.5))
        fv = np.floor(vf + f32(0.5))
    ok &= (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
    j = np.where(ok, np.where(ok, fv, 0).astype(np.int64) * W + np.where(ok, fu, 0).astype(np.int64), 0)
    ok &= tZ[j] > 0
    ok &= ~((nX[j] == 0) & (nY[j] == 0) & (nZ[j] == 0))
    dx, dy, dz = qx - tX[j], qy - tY[j], qz - tZ[j]
    d2 = (dx * dx + dy * dy) + dz * dz
    ok &= d2 < f32(dist_thresh) * f32(dist_thresh)
    m = np.flatnonzero(ok)
    j = j[m]
    q0, q1, q2 = qx[m], qy[m], qz[m]
    nx, ny, nz = nX[j], nY[j], nZ[j]
    dx, dy, dz = dx[m], dy[m], dz[m]
    r = (nx * dx + ny * dy) + nz * dz
    J = [q1 * nz - q2 * ny, q2 * nx - q0 * nz, q0 * ny - q1 * nx, nx, ny, nz]
    # photometric term
    gx, gy, pv = (a.ravel()[j] for a in photo_record(dst_gray))
    Yt = np.asarray(dst_gray, np.uint8).ravel()[j].astype(f32)
    Ys = np.asarray(src_gray, np.uint8).ravel()[m].astype(f32)
    w, kx, ky = photo_consts(lam, K)
    gxf, gyf = gx.astype(f32), gy.astype(f32)
    du = uf[m] - fu[m]
    dv = vf[m] - fv[m]
    It = Yt + f32(0.5) * (gxf * du + gyf * dv)
    rp = (It - Ys) * w
    hx = (gxf * kx) / q2
    hy = (gyf * ky) / q2
    hz = -((hx * q0 + hy * q1) / q2)
    Jp = [q1 * hz - q2 * hy, q2 * hx - q0 * hz, q0 * hy - q1 * hx, hx, hy, hz]
    return J, r, Jp, rp, pv, m, j


def reduce(src, src_gray, dst, dst_gray, T12, K=None, dist_thresh=0.10, lam=0.1):
    """The 31 sums of §13 at the fp32 pose T12."""
    J, r, Jp, rp, pv, m, _ = terms(src, src_gray, dst, dst_gray, T12, K, dist_thresh, lam)
    out = np.zeros(NEQ, f64)
    if m.size == 0:
        return out
    J64 = [a.astype(f64) for a in J]
    Jp64 = [np.where(pv, a, f32(0)).astype(f64) for a in Jp]
    r64 = r.astype(f64)
    rp64 = np.where(pv, rp, f32(0)).astype(f64)

    def both(g, p):   # pixel order, geometric before photometric
        t = np.empty(2 * g.size, f64)
        t[0::2] = g
        t[1::2] = p
        return np.cumsum(t)[-1]

    k = 0
    for a in range(6):
        for b in range(a, 6):
            out[k] = both(J64[a] * J64[b], Jp64[a] * Jp64[b])
            k += 1
    for a in range(6):
        out[21 + a] = both(J64[a] * r64, Jp64[a] * rp64)
    out[27] = np.cumsum(r64 * r64)[-1]
    out[28] = float(m.size)
    out[29] = np.cumsum(rp64 * rp64)[-1]
    out[30] = float(pv.sum())
    return out


def align(src, src_gray, dst, dst_gray, K=None, iters=10, dist_thresh=0.10, lam=0.1,
          T_init=None):
    """-> (T64 [4,4], T32 [3,4], status, stats [iters, 4] = values 27..30)."""
    T = np.eye(4) if T_init is None else np.array(T_init, f64).reshape(4, 4)
    status = 0
    stats = np.zeros((iters, 4), f64)
    for it in range(iters):
        neq = reduce(src, src_gray, dst, dst_gray, T[:3].astype(f32), K, dist_thresh, lam)
        stats[it] = neq[27:31]
        xi, st = oracle.solve(neq[:29])
        status |= st
        if st == 0:
            T = oracle.se3_exp(xi) @ T
    return T, T[:3].astype(f32), status, stats


def pose_error(T, T_gt):
    """(degrees, millimetres) between two 4x4 poses."""
    D = np.linalg.inv(T_gt) @ T
    c = np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.degrees(np.arccos(c))), float(np.linalg.norm(D[:3, 3]) * 1000.0)


# Accuracy bounds of the definition on the 640x480 synthetic sequence, lambda =
# 0.1 (degrees, millimetres against T_wc): 4x the errors measured for align()
# above, rounded up.  Measured: pair 0->1 0.0052 deg / 0.041 mm,
# pair 3->4 0.0277 deg / 0.248 mm, composed pose at frame 7 0.0545 deg / 0.840 mm.
# Each stays below a tenth of the geometry-only error on the same input
# (1.78 deg / 20.3 mm, 1.17 deg / 16.7 mm, 7.87 deg / 109 mm).
BOUND_PAIR_0_1 = (0.021, 0.17)
BOUND_PAIR_3_4 = (0.111, 1.0)
BOUND_FRAME_7 = (0.22, 3.4)
