"""Seeded hostile inputs for the depth-only ICP core, and numpy counters that
say how many pixels of an input take each of the core's rare branches
(csrc/icp_device.h): prep_record's IEEE fallback and the projection's path for
a valid source behind the camera.  The counters restate the branch conditions
in float32 in the order the spec writes the operations; the tests assert them,
so no case passes without reaching the branch it is there for.  Nothing is
read back from a kernel.

Used by tests/test_oracle_hostile.py (CPU) and tests/test_gpu_icp_hostile.py.
"""
import functools
from collections import namedtuple

import numpy as np

import youth_synth
from oracle_np import backproject_np, transform_np

f32 = np.float32
Camera = namedtuple("Camera", "fx fy cx cy depth_scale")
SIZES = ((97, 53), (160, 120))
ISLAND_W, ISLAND_H = 97, 53
TINY_SCALE = float(2.0 ** 20)
VIEWER_F, VIEWER_SCALE = float(f32(570.3)), 1000.0
PATCH_H, PATCH_W = 10, 32       # the near-sensor patch
HOSTILE_SEED = 41               # the youth_synth pair under hostile_pair (tests use this one)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def viewer_camera(W, H):
    return Camera(VIEWER_F, VIEWER_F, float(W // 2), float(H // 2), VIEWER_SCALE)


def patch_box(W, H):
    """(v0, v1, u0, u1) of hostile_pair's near-sensor patch: PATCH_H x PATCH_W
    pixels, right of the pushed-back band, off the border."""
    u0 = W - PATCH_W - 3
    v0 = H // 4
    return v0, v0 + PATCH_H, u0, u0 + PATCH_W


def band_cols(W):
    """Columns of hostile_pair's band 3 m behind the surface."""
    return W // 2, W // 2 + W // 8


def _overlay(d, rng):
    """tests/test_rectify.py::hostile_depth's values on a rendered frame, plus a
    depth cliff and depths of a few millimetres."""
    H, W = d.shape
    b0, b1 = band_cols(W)
    d[:, b0:b1] += 3000                                  # a cliff on both sides (3 m at scale 1000)
    v0, v1, u0, u1 = patch_box(W, H)
    d[v0:v1, u0:u1] = rng.integers(1, 6, size=(v1 - v0, u1 - u0))
    d[rng.random((H, W)) < 0.05] = 0
    d[rng.random((H, W)) < 0.02] = -1
    d[rng.random((H, W)) < 0.01] = -32768
    d[rng.random((H, W)) < 0.01] = 32767
    v, u = np.mgrid[0:H, 0:W]
    w = W // 3                                           # the left third: no pixel keeps four neighbours
    board = ((u + v) & 1).astype(bool)[:, :w]
    d[:, :w] = np.where(board, d[:, :w], 0)


@functools.lru_cache(maxsize=None)
def hostile_pair(W, H, seed=HOSTILE_SEED):
    """(src, dst): pair `seed` of youth_synth.pairs, each frame overlaid on its
    own with 5 % holes, 2 % -1, 1 % -32768, 1 % 32767, a valid / invalid
    checkerboard over the left third, a vertical band 3 m further away and a
    near-sensor patch of depths 1..5."""
    src, dst, _ = youth_synth.pairs(seed, 1, W, H)
    rng = np.random.default_rng(0x405711E + 7919 * seed + W)
    out = []
    for frame in (src[0], dst[0]):
        d = frame.astype(np.int16).copy()
        assert d.max() < 32767 - 3000
        _overlay(d, rng)
        out.append(d)
    return _frozen(*out)


@functools.lru_cache(maxsize=None)
def hostile_sequence(W, H, n=5, seed=HOSTILE_SEED):
    """n frames [n, H, W]: hostile_pair's target, its source, and so on in
    turn with fresh hostile values, so that frame k + 1 aligns to frame k."""
    rng = np.random.default_rng(0x5E9 + seed + W)
    frames, _ = youth_synth.sequence(seed, n, W, H)
    out = frames.astype(np.int16).copy()
    for d in out:
        _overlay(d, rng)
    return _frozen(out)[0]


@functools.lru_cache(maxsize=None)
def island_pair(k):
    """(frame, frame): all zero but one 3 x (k + 2) island of sloped, curved
    depth around 1500; only the k pixels of its middle row have four valid
    neighbours, so an align of the frame to itself has exactly k matches."""
    d = np.zeros((ISLAND_H, ISLAND_W), np.int16)
    v, u = np.mgrid[0:3, 0:k + 2]
    d[20:23, 40:40 + k + 2] = 1500 + 7 * u + 5 * v * v + 3 * u * v
    d, = _frozen(d)
    return d, d


@functools.lru_cache(maxsize=None)
def tiny_scale_pair(W, H, seed=0):
    """(src, dst) of depths 1..3 everywhere, 5 % holes in the target only; for
    depth scale TINY_SCALE = 2^20, where cross products fall below 2^-96."""
    rng = np.random.default_rng(0x71A9 + seed + W)
    src = rng.integers(1, 4, size=(H, W)).astype(np.int16)
    dst = rng.integers(1, 4, size=(H, W)).astype(np.int16)
    dst[rng.random((H, W)) < 0.05] = 0
    return _frozen(src, dst)


def tiny_scale_camera(W, H):
    return viewer_camera(W, H)._replace(depth_scale=TINY_SCALE)


def corner_intrinsics(W, H):
    """[(name, Camera, inside)]: the corners of icp_api.cpp's ident_first_ok
    gate (fx = fy, the depth scale and cx each at the viewer's value or at an
    end of its accepted range: 27 cameras, the viewer's own among them, all
    with cy = H/2 - 0.25), then the first values outside it."""
    lo, hi = float(2.0 ** -20), float(2.0 ** 20)
    cy = H / 2 - 0.25
    cams = []
    for fn, fv in (("f=lo", lo), ("f=v", VIEWER_F), ("f=hi", hi)):
        for sn, sv in (("s=lo", lo), ("s=v", VIEWER_SCALE), ("s=hi", hi)):
            for cn, cv in (("cx=-", -65536.0), ("cx=v", float(W // 2)), ("cx=+", 65536.0)):
                cams.append((f"{fn},{sn},{cn}", Camera(fv, fv, cv, cy, sv), True))
    v = Camera(VIEWER_F, VIEWER_F, float(W // 2), cy, VIEWER_SCALE)
    cams.append(("s=2^21", v._replace(depth_scale=float(2.0 ** 21)), False))
    cams.append(("f=2^-21", v._replace(fx=float(2.0 ** -21), fy=float(2.0 ** -21)), False))
    cams.append(("cx=65537", v._replace(cx=65537.0), False))
    return cams


@functools.lru_cache(maxsize=None)
def lemma_frame(W, H, seed=0):
    """Random depths 1..32767 that also hold 1, 2, 3, 255, 256, 16384, 32766
    and 32767, each with four valid neighbours: no holes."""
    rng = np.random.default_rng(0x1E33A + seed + W)
    d = rng.integers(1, 32768, size=(H, W)).astype(np.int16)
    special = (1, 2, 3, 255, 256, 16384, 32766, 32767)
    assert H >= 3 and W >= 2 * len(special) + 2
    d[H // 2, 1:1 + 2 * len(special):2] = special
    return _frozen(d)[0]


# ------------------------------------------------------------------ poses --
def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


BEHIND_TZ = -0.003
POSES = {   # fp64 4 x 4, source -> target
    "identity": np.eye(4),
    "small": _pose(_rot((1.0, 2.0, 0.5), 2.0), (0.012, -0.010, 0.012)),      # 2 degrees, 2 cm
    "behind": _pose(np.eye(3), (0.0, 0.0, BEHIND_TZ)),      # depths 1..3 mm end at P'z <= 0
    "half_turn": _pose(np.diag([-1.0, 1.0, -1.0]), (0.0, 0.0, 0.0)),        # every source behind
}
for _T in POSES.values():
    _T.setflags(write=False)


def pose32(name):
    return POSES[name][:3].astype(f32)


# --------------------------------------------------------------- counters --
def fallback_count(depth, K):
    """Pixels whose normal exists (has_n) but lies outside the fast
    normalisation's range (not norm_fast_ok: |c|^2 outside [2^-96, 2^118] or a
    component with 0 < |c_i| < 2^-64): prep_record's IEEE fallback."""
    X, Y, Z = backproject_np(depth, K)
    H, W = Z.shape
    c = (slice(1, H - 1), slice(1, W - 1))
    l, r = (slice(1, H - 1), slice(0, W - 2)), (slice(1, H - 1), slice(2, W))
    up, dn = (slice(0, H - 2), slice(1, W - 1)), (slice(2, H), slice(1, W - 1))
    with np.errstate(all="ignore"):
        ax, ay, az = X[r] - X[l], Y[r] - Y[l], Z[r] - Z[l]
        bx, by, bz = X[dn] - X[up], Y[dn] - Y[up], Z[dn] - Z[up]
        cx = ay * bz - az * by
        cy = az * bx - ax * bz
        cz = ax * by - ay * bx
        len2 = (cx * cx + cy * cy) + cz * cz
    has_n = (Z[c] > 0) & (Z[l] > 0) & (Z[r] > 0) & (Z[up] > 0) & (Z[dn] > 0) & (len2 > 0)
    tiny = f32(2.0 ** -64)
    comp_ok = np.ones_like(has_n)
    for comp in (cx, cy, cz):
        comp_ok &= ~((np.abs(comp) < tiny) & (comp != 0))
    fast_ok = (len2 >= f32(2.0 ** -96)) & (len2 <= f32(2.0 ** 118)) & comp_ok
    return int((has_n & ~fast_ok).sum())


def behind_mask(depth, K, T12, spec="survey"):
    """Valid sources (z > 0) whose P'z is <= 0 under T12, [H, W] bool."""
    S = backproject_np(depth, K)
    with np.errstate(all="ignore"):
        _, _, qz = transform_np(S, T12, spec)
    return (S[2] > 0) & (qz.reshape(S[2].shape) <= 0)


def behind_count(depth, K, T12, spec="survey"):
    return int(behind_mask(depth, K, T12, spec).sum())
