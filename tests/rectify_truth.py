"""numpy restatement of the lens rectifier (include/youth_rectify.h, DESIGN.md
§17), written from the definition, not from the kernel: the truth of
test_rectify.py, test_gpu_rectify.py and test_gpu_slam_rectify.py.

The map is fp32, every operation rounded as written (numpy rounds each float32
operation once; there is no FMA), then 1/32-px fixed point; the apply is all
integer.  Cameras are (fx, fy, cx, cy, ds) tuples or youth_icp.Intrinsics,
distortions (k1, k2, p1, p2, k3) tuples or youth_rectify.Distortion."""
import numpy as np

F = np.float32
COVERED = np.uint32(1 << 31)


def _cam(K):
    t = K.as_tuple() if hasattr(K, "as_tuple") else tuple(K)
    return tuple(F(v) for v in t)


def source_position(W, H, K, D, Ko=None):
    """(us, vs), float32 [H][W]: where output pixel (u, v) lies in the sensor's
    frame."""
    fx, fy, cx, cy, ds = _cam(K)
    fxo, fyo, cxo, cyo, dso = _cam(Ko if Ko is not None else K)
    assert ds == dso
    k1, k2, p1, p2, k3 = _cam(D)
    one, two = F(1), F(2)
    with np.errstate(all="ignore"):
        u = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
        v = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
        x = (u - cxo) / fxo
        y = (v - cyo) / fyo
        r2 = x * x + y * y
        rad = one + r2 * (k1 + r2 * (k2 + r2 * k3))
        xy = x * y
        tx = (two * p1) * xy + p2 * (r2 + two * (x * x))
        ty = p1 * (r2 + two * (y * y)) + (two * p2) * xy
        us = fx * (x * rad + tx) + cx
        vs = fy * (y * rad + ty) + cy
    for a in (x, r2, rad, tx, us, vs):
        assert a.dtype == F
    return us, vs


def map_parts(W, H, K, D, Ko=None):
    """(covered bool, ix, iy, a, b), [H][W]; the integers are 0 where the
    pixel is not covered."""
    assert W >= 2 and H >= 2
    us, vs = source_position(W, H, K, D, Ko)
    with np.errstate(all="ignore"):
        cov = (us >= F(0)) & (us <= F(W - 1)) & (vs >= F(0)) & (vs <= F(H - 1))
        U = np.where(cov, np.floor(np.where(cov, us, F(0)) * F(32) + F(0.5)), 0).astype(np.int64)
        V = np.where(cov, np.floor(np.where(cov, vs, F(0)) * F(32) + F(0.5)), 0).astype(np.int64)
    ix = np.minimum(U >> 5, W - 2)
    iy = np.minimum(V >> 5, H - 2)
    a, b = U - 32 * ix, V - 32 * iy
    assert a.min() >= 0 and a.max() <= 32 and b.min() >= 0 and b.max() <= 32
    z = np.zeros_like(ix)
    return cov, np.where(cov, ix, z), np.where(cov, iy, z), np.where(cov, a, z), np.where(cov, b, z)


def map_words(W, H, K, D, Ko=None):
    """The map as youth_rectify_map_device writes it: uint32 [H][W][2]."""
    cov, ix, iy, a, b = map_parts(W, H, K, D, Ko)
    w = np.zeros((H, W, 2), np.uint32)
    w[..., 0] = np.where(cov, COVERED | (b << 6).astype(np.uint32) | a.astype(np.uint32), 0)
    w[..., 1] = np.where(cov, iy * W + ix, 0).astype(np.uint32)
    return w


def covered_count(W, H, K, D, Ko=None):
    return int(map_parts(W, H, K, D, Ko)[0].sum())


def _taps(plane, ix, iy):
    """The four taps t00, t10, t01, t11 of a [H][W]... plane, int64."""
    p = plane.astype(np.int64)
    return p[iy, ix], p[iy, ix + 1], p[iy + 1, ix], p[iy + 1, ix + 1]


def _weights(a, b):
    return (32 - a) * (32 - b), a * (32 - b), (32 - a) * b, a * b


def rectify_color(rgb, parts):
    """uint8 [H][W] or [H][W][c] -> the rectified plane."""
    cov, ix, iy, a, b = parts
    c = np.asarray(rgb)
    assert c.dtype == np.uint8
    w = _weights(a, b)
    if c.ndim == 3:
        w = [x[..., None] for x in w]
        cov = cov[..., None]
    t = _taps(c, ix, iy)
    out = (w[0] * t[0] + w[1] * t[1] + w[2] * t[2] + w[3] * t[3] + 512) >> 10
    return np.where(cov, out, 0).astype(np.uint8)


def gate(n):
    n = np.asarray(n, np.int64)
    return np.minimum(255, 8 + ((96 * (n >> 4) ** 2) >> 16))


def rectify_depth(depth, parts):
    """int16 [H][W] -> the rectified frame."""
    cov, ix, iy, a, b = parts
    d = np.asarray(depth)
    assert d.dtype == np.int16
    t = _taps(d, ix, iy)
    w = _weights(a, b)
    right, down = a >= 16, b >= 16
    n = np.where(down, np.where(right, t[3], t[2]), np.where(right, t[1], t[0]))
    valid = n > 0
    T = gate(np.where(valid, n, 1))
    den = np.zeros_like(n)
    num = np.zeros_like(n)
    for tk, wk in zip(t, w):
        on = (tk > 0) & (np.abs(tk - n) < T)
        wk = np.where(on, wk, 0)
        den += wk
        num += wk * (tk - n + T)
    assert (den[valid & cov] >= 256).all() and int(num.max(initial=0)) < 2 ** 32
    den = np.where(valid, den, 1)
    out = n - T + (num + (den >> 1)) // den
    out = np.where(valid, out, n)
    assert np.array_equal(out > 0, valid)
    return np.where(cov, out, 0).astype(np.int16)


def rectify(depth, rgb, W, H, K, D, Ko=None):
    """Frames or stacks of frames -> (depth_out, rgb_out); either may be None.
    depth int16 [H][W] / [n][H][W]; rgb uint8 [H][W][c] / [n][H][W][c]."""
    parts = map_parts(W, H, K, D, Ko)
    do = co = None
    if depth is not None:
        d = np.asarray(depth)
        assert d.shape[-2:] == (H, W)
        do = (rectify_depth(d, parts) if d.ndim == 2
              else np.stack([rectify_depth(f, parts) for f in d]) if len(d) else d.copy())
    if rgb is not None:
        c = np.asarray(rgb)
        assert c.shape[-3:-1] == (H, W)
        co = (rectify_color(c, parts) if c.ndim == 3
              else np.stack([rectify_color(f, parts) for f in c]) if len(c) else c.copy())
    return do, co


def source_position_f64(W, H, K, D, Ko=None):
    """The model evaluated independently in fp64 from the stored fp32
    parameters: (us, vs) float64 [H][W]."""
    fx, fy, cx, cy, _ = [float(v) for v in _cam(K)]
    fxo, fyo, cxo, cyo, _ = [float(v) for v in _cam(Ko if Ko is not None else K)]
    k1, k2, p1, p2, k3 = [float(v) for v in _cam(D)]
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    x, y = (u - cxo) / fxo, (v - cyo) / fyo
    r2 = x ** 2 + y ** 2
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x ** 2)
    yd = y * rad + p1 * (r2 + 2 * y ** 2) + 2 * p2 * x * y
    return fx * xd + cx, fy * yd + cy
