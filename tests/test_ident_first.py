"""CPU checks of the identity-pose form of the first ICP iteration (DESIGN.md
§2 "the identity lemma"; icp_device.h ident_accumulate), through the committed
oracle only.

  * The lemma: at T = I every source pixel that the oracle associates is
    associated with ITS OWN pixel of the target frame.  Checked with the
    source frame as its own target (so the distance gate never rejects) on
    three depth images that stress the projection's roundings: every value
    1 .. 32767 in turn, row-constant depths, and 1 mm / 32767 mm spikes; in
    both arithmetics, at a W that is no multiple of 4, an odd W and 640x480.
  * The shortcut step restated in numpy (no transform, no projection, no
    gather: the target record of the same pixel), summed in pixel order,
    equals oracle.reduce(src, dst, I) bit for bit.
"""
import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from test_oracle_numpy import backproject_np, f32, f64, fma32, normals_np

SIZES = [(97, 53), (161, 122), (640, 480)]
EYE = np.eye(4, dtype=np.float32)[:3]


def _depth_images(W, H):
    i = np.arange(W * H, dtype=np.int64)
    # every value 1 .. 32767 in turn (a frame smaller than 32767 pixels
    # strides through the range, so it still spans 1 mm .. 32.7 m)
    step = max(1, 32767 // (W * H))
    yield "ramp", (1 + (i * step) % 32767).astype(np.int16).reshape(H, W)
    rows = (1 + (np.arange(H, dtype=np.int64) * 7919) % 32767).astype(np.int16)
    yield "rows", np.repeat(rows[:, None], W, axis=1)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    yield "spikes", np.where((u + v) % 2 == 0, 1, 32767).astype(np.int16)


@pytest.mark.parametrize("spec", ["fma", "survey"])
@pytest.mark.parametrize("W,H", SIZES)
def test_identity_associates_every_pixel_with_itself(W, H, spec):
    K = oracle.viewer_K(W, H)
    own = np.arange(W * H, dtype=np.int32)
    for name, d in _depth_images(W, H):
        with oracle.spec(spec):
            idx = oracle.associate(d, d, EYE, K, dist_thresh=1e9)
        m = idx >= 0
        assert np.array_equal(idx[m], own[m]), (name, np.flatnonzero(idx[m] != own[m])[:4])
        nx, ny, nz = oracle.normals(*oracle.backproject(d, K))
        has_n = ((nx != 0) | (ny != 0) | (nz != 0)).ravel()
        assert int(m.sum()) == int(has_n.sum()) > 0, name
        assert np.array_equal(m, has_n), name


def ident_reduce_np(S, Tg, Nt, thr, spec):
    """The identity form of spec a7-a9: P' = P, the target is the same pixel;
    then the gate, r, J and the 29 sums of exact float64 products in pixel
    order, as reduce_np (test_oracle_numpy.py) forms them."""
    q0, q1, q2 = (a.ravel() for a in S)
    tX, tY, tZ = (a.ravel() for a in Tg)
    nx, ny, nz = (a.ravel() for a in Nt)
    ok = (q2 > 0) & (tZ > 0) & ~((nx == 0) & (ny == 0) & (nz == 0))
    dx, dy, dz = q0 - tX, q1 - tY, q2 - tZ
    d2 = (dx * dx + dy * dy) + dz * dz if spec == "survey" else fma32(dz, dz, fma32(dy, dy, dx * dx))
    ok &= d2 < f32(thr) * f32(thr)
    q0, q1, q2, dx, dy, dz, nx, ny, nz = (a[ok] for a in (q0, q1, q2, dx, dy, dz, nx, ny, nz))
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
    return np.array([np.cumsum(t)[-1] if t.size else 0.0 for t in terms], f64)


def _pairs():
    g = np.load(GOLDEN + "/pair_160x120.npz")
    yield "pair_160x120", g["src"], g["dst"], oracle.K_of(g["K"]), float(g["dist_thresh"])
    # random depths: a smooth surface 1.5 .. 2.5 m seen twice with independent
    # +-3 mm noise and 3 % holes each, so the gate both passes and rejects
    rng = np.random.default_rng(0x1DE7)
    W, H = 97, 53
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    base = 2000 + 400 * np.sin(u / 17.0) + 300 * np.cos(v / 11.0)
    frames = []
    for _ in range(2):
        d = base + rng.integers(-3, 4, size=(H, W))
        d[rng.random((H, W)) < 0.03] = 0
        frames.append(d.astype(np.int16))
    yield "random_97x53", frames[0], frames[1], oracle.viewer_K(W, H), 0.10


@pytest.mark.parametrize("spec", ["fma", "survey"])
@pytest.mark.parametrize("case", list(_pairs()), ids=lambda c: c[0])
def test_shortcut_step_equals_oracle_reduce_bitwise(case, spec):
    _, src, dst, K, thr = case
    S, Tg = backproject_np(src, K), backproject_np(dst, K)
    Nt = normals_np(*Tg)
    neq = ident_reduce_np(S, Tg, Nt, thr, spec)
    with oracle.spec(spec):
        o_neq = oracle.reduce(src, dst, EYE, K, thr)
    assert np.array_equal(neq.view(np.uint64), o_neq.view(np.uint64))
    # the gate is exercised both ways: some pixels match, some valid ones do not
    valid = int(((src > 0) & (dst > 0)).sum())
    assert 0 < neq[28] < valid
