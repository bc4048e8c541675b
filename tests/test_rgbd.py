"""RGB-D alignment, CPU side: the numpy truth
(tests/rgbd_truth.py) pinned against a plain pixel loop and, at lambda = 0,
against the C oracle bit for bit; the colour generators of the synthetic
source; and the accuracy of the definition itself on the synthetic sequence.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle
import rgbd_draws
import rgbd_truth
import youth_synth
from conftest import GOLDEN

f32, f64 = np.float32, np.float64


# ------------------------------------------------------------ truth pinned --
def _hand_pair():
    """12 x 9: a wall at 1000 mm with a 50 mm step (inside the gate), a 200 mm
    step (outside it) and a hole; intensity columns of 0 and 255 (gradients of
    +-255) beside a ramp."""
    H, W = 9, 12
    dst = np.full((H, W), 1000, np.int16)
    dst[:, 7:] = 1050
    dst[:, 10:] = 1250
    dst[4, 3] = 0
    src = dst.copy()
    src[2, 5] = 0
    src[:, :2] += 3
    dg = np.zeros((H, W), np.uint8)
    dg[:, 2:4] = 255
    dg[:, 6:] = (np.arange(6) * 40 + 10)[None, :]
    dg[5:, :] = dg[5:, :] // 2 + 17
    sg = np.roll(dg, 1, axis=1)
    sg[0, :] = 255
    return src, sg, dst, dg


def _reduce_loop(src, sg, dst, dg, T12, K, thr, lam):
    """§13 pixel by pixel with numpy float32 scalars."""
    H, W = src.shape
    sX, sY, sZ = oracle.backproject(src, K)
    tX, tY, tZ = oracle.backproject(dst, K)
    nX, nY, nZ = oracle.normals(tX, tY, tZ)
    T = [f32(v) for v in np.asarray(T12, f32).ravel()[:12]]
    fx, fy, cx, cy = f32(K.fx), f32(K.fy), f32(K.cx), f32(K.cy)
    w = f32(lam) / f32(255.0)
    kx, ky = (f32(0.5) * w) * fx, (f32(0.5) * w) * fy
    half = f32(0.5)
    out = np.zeros(31, f64)
    Y = dg.astype(np.int32)
    for v in range(H):
        for u in range(W):
            x, y, z = sX[v, u], sY[v, u], sZ[v, u]
            qx = ((T[0] * x + T[1] * y) + T[2] * z) + T[3]
            qy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7]
            qz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11]
            if not (z > 0 and qz > 0):
                continue
            uf = (fx * qx) / qz + cx
            vf = (fy * qy) / qz + cy
            fu, fv = np.floor(uf + half), np.floor(vf + half)
            if not (0 <= fu < W and 0 <= fv < H):
                continue
            iu, iv = int(fu), int(fv)
            n = (nX[iv, iu], nY[iv, iu], nZ[iv, iu])
            if not tZ[iv, iu] > 0 or (n[0] == 0 and n[1] == 0 and n[2] == 0):
                continue
            dx, dy, dz = qx - tX[iv, iu], qy - tY[iv, iu], qz - tZ[iv, iu]
            if not (dx * dx + dy * dy) + dz * dz < f32(thr) * f32(thr):
                continue
            r = (n[0] * dx + n[1] * dy) + n[2] * dz
            J = [qy * n[2] - qz * n[1], qz * n[0] - qx * n[2], qx * n[1] - qy * n[0], *n]

            def add(Jv, rv):
                k = 0
                for a in range(6):
                    for b in range(a, 6):
                        out[k] += f64(Jv[a]) * f64(Jv[b])
                        k += 1
                for a in range(6):
                    out[21 + a] += f64(Jv[a]) * f64(rv)

            add(J, r)
            out[27] += f64(r) * f64(r)
            out[28] += 1
            if not (1 <= iu <= W - 2 and 1 <= iv <= H - 2):
                continue
            gx = f32(Y[iv, iu + 1] - Y[iv, iu - 1])
            gy = f32(Y[iv + 1, iu] - Y[iv - 1, iu])
            du, dv = uf - fu, vf - fv
            It = f32(Y[iv, iu]) + half * (gx * du + gy * dv)
            rp = (It - f32(sg[v, u])) * w
            hx = (gx * kx) / qz
            hy = (gy * ky) / qz
            hz = -((hx * qx + hy * qy) / qz)
            add([qy * hz - qz * hy, qz * hx - qx * hz, qx * hy - qy * hx, hx, hy, hz], rp)
            out[29] += f64(rp) * f64(rp)
            out[30] += 1
    return out


def test_truth_equals_pixel_loop():
    src, sg, dst, dg = _hand_pair()
    K = oracle.viewer_K(12, 9)
    gx, gy, _ = rgbd_truth.photo_record(dg)
    assert gx.max() == 255 and gx.min() == -255
    for T in (np.eye(4)[:3], np.hstack([np.eye(3), [[0.0021], [-0.0013], [0.004]]])):
        for lam in (0.1, 0.0):
            want = _reduce_loop(src, sg, dst, dg, T, K, 0.10, lam)
            got = rgbd_truth.reduce(src, sg, dst, dg, T, K, 0.10, lam)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
            assert 6 <= got[28] < 12 * 9 and got[30] == got[28]
            if lam:
                assert got[29] > 0


@pytest.mark.parametrize("name", ["pair_80x60", "pair_97x53"])
def test_truth_at_lambda_zero_equals_oracle_bitwise(name):
    g = np.load(f"{GOLDEN}/{name}.npz")
    src, dst, K, thr = g["src"], g["dst"], oracle.K_of(g["K"]), float(g["dist_thresh"])
    rng = np.random.default_rng(5)
    sg = rng.integers(0, 256, src.shape, dtype=np.uint8)
    dg = rng.integers(0, 256, src.shape, dtype=np.uint8)
    th = np.deg2rad(3.0)
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    for T in (np.eye(4)[:3], np.hstack([np.eye(3), [[0.004], [-0.002], [0.003]]]),
              np.hstack([R, [[0.04], [0.01], [-0.02]]])):
        T12 = T.astype(f32)
        got = rgbd_truth.reduce(src, sg, dst, dg, T12, K, thr, lam=0.0)
        with oracle.spec("survey"):
            want = oracle.reduce(src, dst, T12, K, thr)
        assert np.array_equal(got[:29].view(np.uint64), want.view(np.uint64))
        assert got[28] > 0 and got[29] == 0.0 and got[30] == got[28]


@pytest.mark.parametrize("W,H", [(97, 53), (160, 120)])
def test_truth_at_lambda_zero_equals_oracle_bitwise_random_intrinsics(W, H):
    """The geometric half under the cameras of tests/rgbd_draws.py (fx != fy,
    fractional principal points, three depth scales), scenes rendered with the
    same camera."""
    rng = np.random.default_rng(7 + W)
    th = np.deg2rad(3.0)
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    draws = rgbd_draws.camera_draws(W, H)
    assert len(draws) >= 6
    for d, k in enumerate(draws):
        src, dst, _ = youth_synth.pairs(400 + d, 1, W, H, K=rgbd_draws.intrinsics(k))
        src, dst = src[0], dst[0]
        sg = rng.integers(0, 256, src.shape, dtype=np.uint8)
        dg = rng.integers(0, 256, src.shape, dtype=np.uint8)
        for T in (np.eye(4)[:3], np.hstack([np.eye(3), [[0.004], [-0.002], [0.003]]]),
                  np.hstack([R, [[0.04], [0.01], [-0.02]]])):
            T12 = T.astype(f32)
            got = rgbd_truth.reduce(src, sg, dst, dg, T12, k, 0.10, lam=0.0)
            with oracle.spec("survey"):
                want = oracle.reduce(src, dst, T12, oracle.K_of(k), 0.10)
            assert np.array_equal(got[:29].view(np.uint64), want.view(np.uint64)), (d, k)
            assert got[28] > 0 and got[29] == 0.0 and got[30] == got[28], (d, k)


def test_photometric_jacobian_is_the_derivative_of_the_residual():
    """Jp against central differences of rp, under a camera with fx != fy: the
    check that §13's constants kx = 0.5 w fx and ky = 0.5 w fy are the right
    ones, which restating the definition cannot give.  The target intensity is
    the integer ramp Y = 2u - v + 80 (gx = 4 and gy = -2 exactly), so It = 2 uf -
    vf + 80 is linear in the projection whichever pixel it rounds to, and rp is
    smooth in the pose.  Measured: differences of at most 2.1e-5 against |Jp| up
    to 0.47; exchanging kx and ky moves the y-dependent part by 1 - 61.7 / 92.3
    = 33 %.  1e-3 leaves 50x for the fp32 noise of rp over 2 eps."""
    W, H, lam, eps = 64, 48, 0.7, 2e-3
    k = (61.7, 92.3, 29.4, 26.2, 1000.0)
    src, dst, _, srgb, _ = youth_synth.pairs_rgb(300, 1, W, H, K=rgbd_draws.intrinsics(k))
    src, dst, sg = src[0], dst[0], rgbd_truth.luma(srgb[0])
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    ramp = 2 * u - v + 80
    assert ramp.min() >= 0 and ramp.max() <= 255
    dg = ramp.astype(np.uint8)
    gx, gy, valid = rgbd_truth.photo_record(dg)
    assert (gx[valid] == 4).all() and (gy[valid] == -2).all()
    T = np.eye(4)
    T[:3, 3] = (0.004, -0.002, 0.003)

    def at(Tp):
        _, _, Jp, rp, pv, m, _ = rgbd_truth.terms(src, sg, dst, dg, Tp[:3].astype(f32), k, 0.10, lam)
        return m[pv], rp[pv].astype(f64), [a[pv].astype(f64) for a in Jp]

    m0, _, Jp0 = at(T)
    assert m0.size >= 1000
    worst, big = 0.0, 0.0
    for c in range(6):
        xi = np.zeros(6)
        xi[c] = eps
        mp, rp_p, _ = at(oracle.se3_exp(xi) @ T)
        mm, rp_m, _ = at(oracle.se3_exp(-xi) @ T)
        both = np.intersect1d(np.intersect1d(m0, mp), mm)      # matched in all three
        assert both.size >= m0.size / 2, (c, both.size, m0.size)
        diff = (rp_p[np.searchsorted(mp, both)] - rp_m[np.searchsorted(mm, both)]) / (2 * eps)
        Jc = Jp0[c][np.searchsorted(m0, both)]
        err = float(np.abs(diff - Jc).max())
        print(f"twist {c}: {both.size} of {m0.size} pixels, max |Jp| {np.abs(Jc).max():.3f}, "
              f"max |difference - Jp| {err:.2e}")
        assert err <= 1e-3, (c, err)
        worst, big = max(worst, err), max(big, float(np.abs(Jc).max()))
    assert big >= 0.1          # the bound is far below the Jacobian it checks


# ------------------------------------------------------------------- synth --
def test_rgb_generators_leave_depth_unchanged_and_are_deterministic():
    W, H = 160, 120
    src, dst, T = youth_synth.pairs(3, 1, W, H)
    s2, d2, T2, srgb, drgb = youth_synth.pairs_rgb(3, 1, W, H)
    assert np.array_equal(src, s2) and np.array_equal(dst, d2) and np.array_equal(T, T2)
    fr, Twc = youth_synth.sequence(5, 3, W, H)
    f2, Twc2, rgb = youth_synth.sequence_rgb(5, 3, W, H)
    assert np.array_equal(fr, f2) and np.array_equal(Twc, Twc2)
    d = youth_synth.render(Twc[1], W, H, noise_seed=9, flags=youth_synth.DEFAULT_FLAGS)
    d3, c3 = youth_synth.render_rgb(Twc[1], W, H, noise_seed=9, flags=youth_synth.DEFAULT_FLAGS)
    assert np.array_equal(d, d3)
    # deterministic, and independent of the noise seed and the flags
    assert np.array_equal(youth_synth.pairs_rgb(3, 1, W, H)[3], srgb)
    assert np.array_equal(youth_synth.sequence_rgb(5, 3, W, H)[2], rgb)
    assert np.array_equal(c3, rgb[1])
    assert np.array_equal(youth_synth.render_rgb(Twc[1], W, H, noise_seed=1, flags=0)[1], c3)
    assert np.array_equal(
        youth_synth.sequence_rgb(5, 3, W, H, flags=youth_synth.SURVEY_FLAGS)[2], rgb)
    # a colour camera has no holes: every ray of this closed room hits
    assert (fr == 0).any() and rgb.min() >= 32 and rgb.max() <= 224
    assert len(np.unique(rgb)) > 100


def test_texture_definition():
    """The texture at the centre pixel's hit point, from the header's formula."""
    W, H = 160, 120
    _, Twc = youth_synth.sequence(0, 1, W, H)
    d, c = youth_synth.render_rgb(Twc[0], W, H)
    K = youth_synth.viewer_intrinsics(W, H)
    want = np.zeros((H, W, 3), np.int64)
    u, v = np.meshgrid(np.arange(W, dtype=f64), np.arange(H, dtype=f64))
    z = d.astype(f64) / 1000.0                       # quantised: within 0.5 mm of the hit
    pc = np.stack([(u - K.cx) / K.fx * z, (v - K.cy) / K.fy * z, z], -1)
    p = pc @ Twc[0][:3, :3].T + Twc[0][:3, 3]
    bump = lambda t: 4 * (t - np.floor(t)) * (1 - (t - np.floor(t)))
    b4 = bump(p[..., :3].sum(-1) / 0.9)
    x, y, zz = p[..., 0], p[..., 1], p[..., 2]
    for k, t in enumerate(((x + 0.3 * zz) / 0.23, (y - 0.4 * x) / 0.31, (zz + 0.5 * y) / 0.27)):
        want[..., k] = np.floor(32 + 192 * (0.5 * bump(t) + 0.5 * b4) + 0.5)
    # 0.5 mm along the ray moves a channel by at most 192 * 0.5 * 4 * 0.0005 / 0.23 * 2 < 2
    assert np.abs(want - c.astype(np.int64))[d > 0].max() <= 2


# ---------------------------------------------- accuracy of the definition --
@pytest.fixture(scope="module")
def seq8():
    fr, Twc, rgb = youth_synth.sequence_rgb(0, 8)
    g = rgbd_truth.luma(rgb)
    with ThreadPoolExecutor(7) as pool:   # numpy and the oracle release the GIL
        rel = list(pool.map(
            lambda k: rgbd_truth.align(fr[k + 1], g[k + 1], fr[k], g[k], lam=0.1)[0], range(7)))
    geo = [oracle.align(fr[k + 1], fr[k])[0] for k in range(7)]
    return Twc, rel, geo


def _gt(Twc, a, b):
    return np.linalg.inv(Twc[a]) @ Twc[b]


def _within(err, bound):
    return err[0] <= bound[0] and err[1] <= bound[1]


def test_definition_accuracy_pairs(seq8):
    Twc, rel, geo = seq8
    for k, bound in ((0, rgbd_truth.BOUND_PAIR_0_1), (3, rgbd_truth.BOUND_PAIR_3_4)):
        e_geo = rgbd_truth.pose_error(geo[k], _gt(Twc, k, k + 1))
        e = rgbd_truth.pose_error(rel[k], _gt(Twc, k, k + 1))
        print(f"pair {k}->{k + 1}: rgbd {e[0]:.4f} deg / {e[1]:.3f} mm, "
              f"geometry only {e_geo[0]:.3f} deg / {e_geo[1]:.2f} mm")
        assert bound[0] < e_geo[0] / 10 and bound[1] < e_geo[1] / 10
        assert _within(e, bound)
        if k == 0:
            assert e_geo[0] >= 1.0          # the valley: depth alone is 1.78 deg off


def test_definition_accuracy_composed(seq8):
    Twc, rel, geo = seq8
    T, T0 = np.eye(4), np.eye(4)
    for k in range(7):
        T, T0 = T @ rel[k], T0 @ geo[k]
    e = rgbd_truth.pose_error(T, _gt(Twc, 0, 7))
    e_geo = rgbd_truth.pose_error(T0, _gt(Twc, 0, 7))
    print(f"frame 7: rgbd {e[0]:.4f} deg / {e[1]:.3f} mm, geometry only {e_geo[0]:.3f} deg / "
          f"{e_geo[1]:.2f} mm")
    assert e_geo[0] >= 5.0
    bound = rgbd_truth.BOUND_FRAME_7
    assert bound[0] < e_geo[0] / 10 and bound[1] < e_geo[1] / 10
    assert _within(e, bound)
