"""Loop closing (include/youth_loop.h) restated in numpy: the
checker of the signature and distance kernels and of the pose graph.  CPU only.

signature / distance follow the integer definitions word for word (Python
integers where 32 bits would not do).  gates restates the four measures of a
verified pair from the two alignments' poses and statistics.  optimize is an
independent Gauss-Newton: the same residual and cost, the same move
X <- X [exp(w), v] of a node, but Jacobians by central differences and numpy's
solver.
"""
import numpy as np

GX, GY, CELLS = 20, 15, 300
CAP, LY = 1000, 4


def signature(depth, gray):
    """depth int16 [H, W], gray uint8 [H, W] -> 300 uint32 records, cell (i, j)
    at j * GX + i: bits 0-15 dm, 16-23 ym, bit 31 valid."""
    d = np.asarray(depth, np.int16)
    y = np.asarray(gray, np.uint8)
    H, W = d.shape
    assert W >= GX and H >= GY and y.shape == (H, W)
    out = np.zeros(CELLS, np.uint32)
    for j in range(GY):
        r0, r1 = j * H // GY, (j + 1) * H // GY
        for i in range(GX):
            c0, c1 = i * W // GX, (i + 1) * W // GX
            dc, yc = d[r0:r1, c0:c1], y[r0:r1, c0:c1]
            n = int(dc.size)
            ok = dc > 0
            cnt = int(ok.sum())
            sum_d = int(dc[ok].sum(dtype=np.int64))   # 896 K pixels of 32767 pass 32 bits
            sum_y = int(yc.sum(dtype=np.int64))
            valid = cnt > 0 and 4 * cnt >= n
            dm = (sum_d + cnt // 2) // cnt if valid else 0
            ym = (sum_y + n // 2) // n
            assert 0 <= dm < 65536 and 0 <= ym < 256
            out[j * GX + i] = dm | (ym << 16) | ((1 << 31) if valid else 0)
    return out


def fields(sig):
    """-> (dm, ym, valid) of records."""
    s = np.asarray(sig, np.uint32).astype(np.int64)
    return s & 0xFFFF, (s >> 16) & 0xFF, (s >> 31).astype(bool)


def distance(sig_q, sig_k, cap=CAP, ly=LY):
    """D(q, k) of two records of 300 cells."""
    dq, yq, vq = fields(sig_q)
    dk, yk, vk = fields(sig_k)
    c = np.where(vq & vk, np.minimum(np.abs(dq - dk), cap), np.where(vq ^ vk, cap, 0))
    return int((c + ly * np.abs(yq - yk)).sum())


def candidates(D_row, q, min_gap, max_cell_dist, max_candidates):
    """Indices k with q - k >= min_gap and D <= max_cell_dist * 300, lowest D
    first, ties by the lower index."""
    ks = [k for k in range(0, q - min_gap + 1) if int(D_row[k]) <= max_cell_dist * CELLS]
    ks.sort(key=lambda k: (int(D_row[k]), k))
    return ks[:max_candidates]


def gates(T_fwd, stats_fwd, T_bwd, stats_bwd, n_pixels, lam):
    """The four measures of a verified pair (youth_loop_edge) from the two
    alignments: poses [4, 4] (or [3, 4]) and statistics rows [sum r^2, cnt_g,
    sum rp^2, cnt_p]; a [iters, 4] array stands for its last row.
    -> (overlap, gray_rms, fb_rot_deg, fb_trans_m), fp64."""
    rows = [np.asarray(s, np.float64).reshape(-1, 4)[-1] for s in (stats_fwd, stats_bwd)]
    overlap = min(float(s[1]) for s in rows) / float(n_pixels)
    rms = [(255.0 / float(lam)) * float(np.sqrt(s[2] / s[3])) if s[3] > 0 else float("inf")
           for s in rows]
    T = []
    for P in (T_fwd, T_bwd):
        M = np.eye(4)
        M[:3] = np.asarray(P, np.float64).reshape(-1, 4)[:3]   # the last row is (0, 0, 0, 1)
        T.append(M)
    E = T[0] @ T[1]
    v = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    ang = np.arctan2(np.linalg.norm(v), 0.5 * (E[0, 0] + E[1, 1] + E[2, 2] - 1.0))
    return overlap, max(rms), float(np.degrees(ang)), float(np.linalg.norm(E[:3, 3]))


# ---------------------------------------------------------------- SO(3) / SE(3)
def _skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_so3(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    S = _skew(w)
    if th < 1e-8:
        return np.eye(3) + S + 0.5 * S @ S
    return np.eye(3) + np.sin(th) / th * S + (1.0 - np.cos(th)) / th ** 2 * S @ S


def log_so3(R):
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = float(np.linalg.norm(v))
    th = float(np.arctan2(s, 0.5 * (np.trace(R) - 1.0)))
    return v if s < 1e-12 else v * (th / s)


def se3_exp(xi):
    """exp of the twist xi = (w, v), rotation first (the project's order)."""
    xi = np.asarray(xi, np.float64)
    w, v = xi[:3], xi[3:]
    th = float(np.linalg.norm(w))
    S = _skew(w)
    if th < 1e-8:
        V = np.eye(3) + 0.5 * S
    else:
        V = np.eye(3) + (1.0 - np.cos(th)) / th ** 2 * S + (th - np.sin(th)) / th ** 3 * S @ S
    T = np.eye(4)
    T[:3, :3] = exp_so3(w)
    T[:3, 3] = V @ v
    return T


def residual(Xi, Xj, Z):
    E = np.linalg.inv(Z) @ np.linalg.inv(Xi) @ Xj
    return np.concatenate([log_so3(E[:3, :3]), E[:3, 3]])


def cost(X, edges, w_rot=1.0, w_trans=1.0):
    c = 0.0
    for i, j, Z, w in edges:
        e = residual(X[i], X[j], Z)
        c += w * (w_rot * float(e[:3] @ e[:3]) + w_trans * float(e[3:] @ e[3:]))
    return c


def _move(X, d):
    out = X.copy()
    out[:3, :3] = X[:3, :3] @ exp_so3(d[:3])
    out[:3, 3] = X[:3, 3] + X[:3, :3] @ d[3:]
    return out


def optimize(X, edges, w_rot=1.0, w_trans=1.0, iters=20, h=1e-6):
    """edges: [(i, j, Z [4, 4], w)].  Node 0 fixed.  -> optimised X [n, 4, 4]."""
    X = np.array(X, np.float64).reshape(-1, 4, 4).copy()
    n = X.shape[0]
    m = 6 * (n - 1)
    sw = np.sqrt(np.array([w_rot] * 3 + [w_trans] * 3))
    for _ in range(iters):
        Hm = np.zeros((m, m))
        g = np.zeros(m)
        for i, j, Z, w in edges:
            e = residual(X[i], X[j], Z) * sw * np.sqrt(w)
            J = {}
            for node in (i, j):
                if node == 0:
                    continue
                Jn = np.zeros((6, 6))
                for a in range(6):
                    d = np.zeros(6)
                    d[a] = h
                    Xp = {i: X[i], j: X[j]}
                    Xm = dict(Xp)
                    Xp[node] = _move(X[node], d)
                    Xm[node] = _move(X[node], -d)
                    Jn[:, a] = (residual(Xp[i], Xp[j], Z) - residual(Xm[i], Xm[j], Z)) / (2.0 * h)
                J[node] = Jn * (sw * np.sqrt(w))[:, None]
            for a, Ja in J.items():
                ra = 6 * (a - 1)
                g[ra:ra + 6] += Ja.T @ e
                for b, Jb in J.items():
                    rb = 6 * (b - 1)
                    Hm[ra:ra + 6, rb:rb + 6] += Ja.T @ Jb
        delta = np.linalg.solve(Hm, -g)
        for k in range(1, n):
            X[k] = _move(X[k], delta[6 * (k - 1):6 * k])
            U, _, Vt = np.linalg.svd(X[k][:3, :3])
            X[k][:3, :3] = U @ Vt
        if np.abs(delta).max() < 1e-12:
            break
    return X


def pose_error(T, T_gt):
    """(degrees, millimetres) between two 4x4 poses."""
    D = np.linalg.inv(T_gt) @ T
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    ang = np.arctan2(np.linalg.norm(v), 0.5 * (np.trace(D[:3, :3]) - 1.0))
    return float(np.degrees(ang)), float(np.linalg.norm(D[:3, 3]) * 1000.0)


# ------------------------------------------------------- the C5 keyframe graph
KF_FRAMES = list(range(0, 601, 40)) + [630]   # 17 keyframes; 630 revisits 0
BIAS = (0.004, -0.006, 0.005, 0.006, -0.004, 0.008)


def odometry_edges(X, bias=None):
    """Consecutive-node edges of the poses X; with `bias` every step is
    right-multiplied by exp(bias)."""
    B = np.eye(4) if bias is None else se3_exp(bias)
    return [(k - 1, k, np.linalg.inv(X[k - 1]) @ X[k] @ B, 1.0) for k in range(1, len(X))]


def compose(edges, X0):
    """The poses the odometry edges compose to, from X0."""
    X = [np.array(X0, np.float64)]
    for _, _, Z, _ in edges:
        X.append(X[-1] @ Z)
    return np.array(X)
