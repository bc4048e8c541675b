"""The numpy restatement of spec a2 and a6-a9 that pins the C oracle
(oracle/icp_oracle.c) bit for bit: whole-frame array expressions in numpy
float32 (IEEE single, one rounding per operation, no contraction) and an exact
emulation of fmaf.  Written from the spec text,
not from the C code's structure.  tests/test_oracle_numpy.py holds it to the
oracle on synthetic and golden frames, tests/test_oracle_hostile.py on hostile
depth and at the corners of the accepted intrinsics."""
import numpy as np

f32, f64 = np.float32, np.float64


def fma32(a, b, c):
    """Correctly rounded float32 fma(a, b, c), elementwise.  a*b is exact in
    float64; s = a*b + c rounds once in float64 and e (TwoSum) is its exact
    error.  round32(s + e) == round32(s) unless s sits exactly on a float32
    midpoint, where the sign of e breaks the tie."""
    a, b, c = (np.asarray(x, f32) for x in (a, b, c))
    p = a.astype(f64) * b.astype(f64)
    c64 = c.astype(f64)
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)
    r = s.astype(f32)
    r64 = r.astype(f64)
    up = np.nextafter(r, f32(np.inf))
    dn = np.nextafter(r, f32(-np.inf))
    tie_up = (s == (r64 + up.astype(f64)) / 2) & (e > 0)   # rounded down at a tie, true value above
    tie_dn = (s == (r64 + dn.astype(f64)) / 2) & (e < 0)   # rounded up at a tie, true value below
    return np.where(tie_up, up, np.where(tie_dn, dn, r)).astype(f32)


def backproject_np(depth, K):
    """Spec a2: z = d / depth_scale; x = ((u - cx) * z) / fx; y likewise."""
    H, W = depth.shape
    d = depth.astype(f32)
    valid = depth > 0
    z = np.where(valid, d / f32(K.depth_scale), f32(0)).astype(f32)
    u = np.arange(W, dtype=f32)[None, :]
    v = np.arange(H, dtype=f32)[:, None]
    x = np.where(valid, ((u - f32(K.cx)) * z) / f32(K.fx), f32(0)).astype(f32)
    y = np.where(valid, ((v - f32(K.cy)) * z) / f32(K.fy), f32(0)).astype(f32)
    return x, y, z


def normals_np(X, Y, Z):
    """Spec a6: n = normalize((P(u+1)-P(u-1)) x (P(v+1)-P(v-1))), zero on the
    1-px border, where the centre or a 4-neighbour is invalid, or where the
    cross product vanishes; oriented so n . P <= 0."""
    H, W = Z.shape
    N = [np.zeros((H, W), f32) for _ in range(3)]
    c = (slice(1, H - 1), slice(1, W - 1))
    l, r = (slice(1, H - 1), slice(0, W - 2)), (slice(1, H - 1), slice(2, W))
    up, dn = (slice(0, H - 2), slice(1, W - 1)), (slice(2, H), slice(1, W - 1))
    ok = (Z[c] > 0) & (Z[l] > 0) & (Z[r] > 0) & (Z[up] > 0) & (Z[dn] > 0)
    ax, ay, az = X[r] - X[l], Y[r] - Y[l], Z[r] - Z[l]
    bx, by, bz = X[dn] - X[up], Y[dn] - Y[up], Z[dn] - Z[up]
    cx = ay * bz - az * by
    cy = az * bx - ax * bz
    cz = ax * by - ay * bx
    len2 = (cx * cx + cy * cy) + cz * cz
    ok &= len2 > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt(len2)
        nx, ny, nz = cx / ln, cy / ln, cz / ln
    flip = ((nx * X[c] + ny * Y[c]) + nz * Z[c]) > 0
    for k, n in enumerate((nx, ny, nz)):
        N[k][c] = np.where(ok, np.where(flip, -n, n), f32(0))
    return N


def transform_np(S, T12, spec="fma"):
    """Spec a7's P' = R P + t for every source pixel (raster order)."""
    sx, sy, sz = (a.ravel() for a in S)
    T = np.asarray(T12, f32).ravel()
    if spec == "survey":
        # P' = R P + t, fixed order, no FMA
        qx = ((T[0] * sx + T[1] * sy) + T[2] * sz) + T[3]
        qy = ((T[4] * sx + T[5] * sy) + T[6] * sz) + T[7]
        qz = ((T[8] * sx + T[9] * sy) + T[10] * sz) + T[11]
    else:
        qx = fma32(T[2], sz, fma32(T[1], sy, fma32(T[0], sx, T[3])))
        qy = fma32(T[6], sz, fma32(T[5], sy, fma32(T[4], sx, T[7])))
        qz = fma32(T[10], sz, fma32(T[9], sy, fma32(T[8], sx, T[11])))
    return qx, qy, qz


def associate_np(S, Tg, Nt, T12, K, thr, spec="fma"):
    """Spec a7 for every source pixel: target index or -1, and P'.
    SURVEY §8a a7: u' = floor(fx P'x / P'z + cx + 0.5), left to right, IEEE
    division; the fma form takes one reciprocal and an fma."""
    sz = S[2].ravel()
    tX, tY, tZ = (a.ravel() for a in Tg)
    nX, nY, nZ = (a.ravel() for a in Nt)
    H, W = S[2].shape
    qx, qy, qz = transform_np(S, T12, spec)
    ok = (sz > 0) & (qz > 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if spec == "survey":
            fu = np.floor(((f32(K.fx) * qx) / qz + f32(K.cx)) + f32(0.5))
            fv = np.floor(((f32(K.fy) * qy) / qz + f32(K.cy)) + f32(0.5))
        else:
            rz = f32(1) / qz
            fu = np.floor(fma32(f32(K.fx) * qx, rz, f32(K.cx) + f32(0.5)))
            fv = np.floor(fma32(f32(K.fy) * qy, rz, f32(K.cy) + f32(0.5)))
    ok &= (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
    j = np.where(ok, np.where(ok, fv, 0).astype(np.int64) * W + np.where(ok, fu, 0).astype(np.int64), 0)
    ok &= tZ[j] > 0
    ok &= ~((nX[j] == 0) & (nY[j] == 0) & (nZ[j] == 0))
    dx, dy, dz = qx - tX[j], qy - tY[j], qz - tZ[j]
    d2 = (dx * dx + dy * dy) + dz * dz if spec == "survey" else fma32(dz, dz, fma32(dy, dy, dx * dx))
    thr2 = f32(thr) * f32(thr)
    ok &= d2 < thr2
    return np.where(ok, j, -1).astype(np.int32), (qx, qy, qz)


def reduce_np(S, Tg, Nt, T12, K, thr, spec="fma"):
    """Spec a8-a9: r = n . (P' - P_t), J = [P' x n, n]; the 21 + 6 + 1 + 1
    sums of exact float64 products in pixel order, each from +0 (so a sum of
    -0 terms, r = -0 on a frame aligned to itself, is +0 as an accumulator's)."""
    idx, (qx, qy, qz) = associate_np(S, Tg, Nt, T12, K, thr, spec)
    m = idx >= 0
    j = idx[m]
    tX, tY, tZ = (a.ravel()[j] for a in Tg)
    nx, ny, nz = (a.ravel()[j] for a in Nt)
    q0, q1, q2 = qx[m], qy[m], qz[m]
    dx, dy, dz = q0 - tX, q1 - tY, q2 - tZ
    if spec == "survey":
        r = (nx * dx + ny * dy) + nz * dz
        J = [q1 * nz - q2 * ny, q2 * nx - q0 * nz, q0 * ny - q1 * nx, nx, ny, nz]
    else:
        r = fma32(nz, dz, fma32(ny, dy, nx * dx))
        J = [fma32(q1, nz, -(q2 * ny)), fma32(q2, nx, -(q0 * nz)), fma32(q0, ny, -(q1 * nx)),
             nx, ny, nz]
    J64 = [a.astype(f64) for a in J]
    r64 = r.astype(f64)
    terms = [J64[a] * J64[b] for a in range(6) for b in range(a, 6)]
    terms += [J64[a] * r64 for a in range(6)] + [r64 * r64, np.ones_like(r64)]
    return np.array([np.cumsum(np.r_[0.0, t])[-1] for t in terms], f64), idx
