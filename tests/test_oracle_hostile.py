"""The C oracle pinned by the numpy restatement (tests/oracle_np.py) BIT FOR
BIT on hostile values: tests/icp_hostile.py's frames (holes, -1, -32768, 32767,
a checkerboard, a depth cliff, depths of 1..5 mm), poses that put valid sources
behind the camera, a depth scale of 2^20, islands of 5 and 6 usable pixels, and
the cameras at and just past the corners of the identity-first gate
(icp_api.cpp ident_first_ok).  CPU only.

tests/test_gpu_icp_hostile.py holds the kernels to the oracle on the same
inputs; here the oracle itself is kept from resting on one reading there, and
every condition the inputs must meet is asserted from the oracle and the
counters alone:

  hostile_pair     oracle status 0, >= 1000 matches at iteration 0 at 160x120
                   (>= 200 at 97x53), >= 1 match inside the near-sensor patch
                   at the identity, behind_count >= 64 under t_z = -0.003 with
                   the align from there status 0 and finite;
  tiny_scale_pair  fallback_count >= 100, no NaN normal, >= 1000 matches;
  island_pair      count exactly k, FEW_MATCHES at 5, DEGENERATE at 6, the pose
                   the identity.
Measured: 1705 matches, 169 in the patch and 182 behind at 97x53; 6876, 165 and
184 at 160x120; 816 fallback pixels in the tiny-scale target and 3795 matches.
"""
import numpy as np
import pytest

import icp_hostile as ih
import oracle
from oracle_np import associate_np, backproject_np, normals_np, reduce_np

f32 = np.float32
SPECS = ("fma", "survey")
FEW_MATCHES, DEGENERATE = 2, 1      # icp_oracle.h / youth_icp.h status bits
THR = 0.10


def _bits(a, b):
    """Equal bit for bit; a NaN equals any NaN (IEEE 754 leaves a NaN's sign
    and payload open, and numpy's and the C compiler's differ)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def _pin(src, dst, K, poses, what):
    """Back-projection, normals, association and the 29 sums of the numpy
    restatement against the oracle's, bit for bit, in both specs -> {(pose,
    spec): (idx, sums)}."""
    Ko = oracle.K_of(K)
    with np.errstate(all="ignore"):
        S, Tg = backproject_np(src, Ko), backproject_np(dst, Ko)
        Nt = normals_np(*Tg)
    oS, oT = oracle.backproject(src, Ko), oracle.backproject(dst, Ko)
    for name, a, b in zip("XYZXYZ", S + Tg, oS + oT):
        assert _bits(a, b), (what, "back-projection", name)
    for name, a, b in zip("XYZ", Nt, oracle.normals(*oT)):
        assert _bits(a, b), (what, "normal", name, np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:4])
    out = {}
    for pose in poses:
        T12 = ih.pose32(pose)
        for spec in SPECS:
            with np.errstate(all="ignore"):
                neq, idx = reduce_np(S, Tg, Nt, T12, Ko, THR, spec)
            with oracle.spec(spec):
                o_idx = oracle.associate(src, dst, T12, Ko, THR)
                o_neq = oracle.reduce(src, dst, T12, Ko, THR)
            assert np.array_equal(idx, o_idx), (what, pose, spec, np.flatnonzero(idx != o_idx)[:4])
            assert _bits(neq, o_neq), (what, pose, spec, neq - o_neq)
            assert neq[28] == (idx >= 0).sum()
            out[pose, spec] = (idx, neq)
    return out


@pytest.mark.parametrize("W,H", ih.SIZES)
def test_hostile_pair_pins_the_oracle(W, H):
    src, dst = ih.hostile_pair(W, H)
    K = ih.viewer_camera(W, H)
    Ko = oracle.K_of(K)
    got = _pin(src, dst, K, list(ih.POSES), (W, H))
    v0, v1, u0, u1 = ih.patch_box(W, H)
    assert v1 - v0 >= 10 and u1 - u0 >= 32 and v0 > 0 and u0 > 0 and v1 < H - 1 and u1 < W - 1
    for spec in SPECS:
        # the half turn: every valid source behind the camera
        assert ih.behind_count(src, K, ih.pose32("half_turn"), spec) == (src > 0).sum() > 0
        idx, neq = got["half_turn", spec]
        assert (idx < 0).all() and not neq.any() and not np.signbit(neq).any()
        # the inputs' conditions
        idx0 = got["identity", spec][0].reshape(H, W)
        assert (idx0[v0:v1, u0:u1] >= 0).sum() >= 1
        behind = ih.behind_mask(src, K, ih.pose32("behind"), spec)
        assert behind.sum() >= 64 and behind[v0:v1, u0:u1].sum() == behind.sum()
        assert (got["behind", spec][0].reshape(H, W)[behind] < 0).all()
        with oracle.spec(spec):
            T64, _, st, stats = oracle.align(src, dst, Ko, iters=10)
            assert st == 0 and stats[0, 0] >= (1000 if W == 160 else 200), (spec, st, stats[:, 0])
            assert stats[0, 0] == got["identity", spec][1][28]
            Tb, _, stb, statsb = oracle.align(src, dst, Ko, iters=10, T_init=ih.POSES["behind"])
            assert stb == 0 and np.isfinite(Tb).all() and np.isfinite(statsb).all(), (spec, stb)
            assert statsb[0, 0] == got["behind", spec][1][28]
            # a turned-round start finds nothing and leaves the pose where it was
            Th, _, sth, statsh = oracle.align(src, dst, Ko, iters=3, T_init=ih.POSES["half_turn"])
            assert sth == FEW_MATCHES and not statsh.any() and np.array_equal(Th, ih.POSES["half_turn"])


@pytest.mark.parametrize("W,H", ih.SIZES)
def test_hostile_sequence_aligns(W, H):
    """Each frame of hostile_sequence aligns to the one before it: status 0 and
    as many matches as hostile_pair is asked for."""
    seq = ih.hostile_sequence(W, H)
    Ko = oracle.K_of(ih.viewer_camera(W, H))
    for k in range(len(seq) - 1):
        _pin(seq[k + 1], seq[k], ih.viewer_camera(W, H), ["identity"], (W, H, k))
        for spec in SPECS:
            with oracle.spec(spec):
                _, _, st, stats = oracle.align(seq[k + 1], seq[k], Ko, iters=10)
            assert st == 0 and stats[:, 0].min() >= (1000 if W == 160 else 200), (k, spec, stats[:, 0])


def test_tiny_scale_pins_the_oracle():
    W, H = 97, 53
    src, dst = ih.tiny_scale_pair(W, H)
    K = ih.tiny_scale_camera(W, H)
    assert src.min() == 1 and src.max() == 3 and dst.max() == 3 and (dst == 0).sum() > 0
    got = _pin(src, dst, K, ["identity", "small", "half_turn"], "tiny")
    assert ih.fallback_count(dst, K) >= 100
    assert ih.fallback_count(dst, ih.viewer_camera(W, H)._replace(depth_scale=5000.0)) == 0
    N = oracle.normals(*oracle.backproject(dst, oracle.K_of(K)))
    assert not any(np.isnan(n).any() for n in N)
    for spec in SPECS:
        assert got["identity", spec][1][28] >= 1000
        assert got["half_turn", spec][1][28] == 0


@pytest.mark.parametrize("k", [5, 6])
def test_islands_pin_the_oracle_and_sit_on_the_threshold(k):
    src, dst = ih.island_pair(k)
    H, W = src.shape
    K = ih.viewer_camera(W, H)
    got = _pin(src, dst, K, ["identity", "behind", "half_turn"], ("island", k))
    valid = (src > 0).sum()
    assert valid == 3 * (k + 2)
    for spec in SPECS:
        idx = got["identity", spec][0]
        assert (idx >= 0).sum() == k and (idx[idx >= 0] == np.flatnonzero(idx >= 0)).all()
        with oracle.spec(spec):
            T64, _, st, stats = oracle.align(src, dst, oracle.K_of(K), iters=4)
        assert np.array_equal(stats[:, 0], [k] * 4), (spec, stats[:, 0])
        assert st == (FEW_MATCHES if k == 5 else DEGENERATE), (spec, st)
        assert _bits(T64, np.eye(4))


CORNERS = ih.corner_intrinsics(97, 53)
# depth scale 2^-20 spreads the points over 10^10 m: with the smallest focal
# length, or a far principal point, most or all neighbours fail the gate
NONFINITE = {"f=lo,s=lo,cx=-", "f=lo,s=lo,cx=+"}
LEMMA_FEW = {"f=lo,s=lo,cx=-", "f=lo,s=lo,cx=v", "f=lo,s=lo,cx=+", "f=v,s=lo,cx=-", "f=v,s=lo,cx=+"}


def test_corner_cameras_cover_the_gate():
    names = [n for n, _, _ in CORNERS]
    assert len(names) == len(set(names)) == 30 and sum(i for _, _, i in CORNERS) == 27
    assert LEMMA_FEW <= set(names)
    lo, hi = 2.0 ** -20, 2.0 ** 20
    for _, K, inside in CORNERS:
        mid = all(lo <= v <= hi for v in (K.fx, K.fy, K.depth_scale))
        assert inside == (mid and abs(K.cx) <= 65536 and abs(K.cy) <= 65536)
        assert K.cy == 53 / 2 - 0.25 and all(float(f32(v)) == v for v in K)
    assert ih.viewer_camera(97, 53)._replace(cy=26.25) in [K for _, K, _ in CORNERS]


@pytest.mark.parametrize("name,K,inside", CORNERS, ids=[n for n, _, _ in CORNERS])
def test_corner_cameras_pin_the_oracle(name, K, inside):
    """Every corner camera on the hostile pair (identity and the behind-camera
    pose) and on the lemma frame.  The identity lemma on the truth: under a
    camera inside the gate every pixel the oracle matches at the identity pose
    is matched to itself, for depths over all of 1..32767."""
    W, H = 97, 53
    src, dst = ih.hostile_pair(W, H)
    _pin(src, dst, K, ["identity", "behind"], name)
    d = ih.lemma_frame(W, H)
    assert set((1, 2, 3, 255, 256, 16384, 32766, 32767)) <= set(d.ravel().tolist()) and d.min() >= 1
    got = _pin(d, d, K, ["identity"], (name, "lemma"))
    for spec in SPECS:
        idx = got["identity", spec][0]
        m = idx >= 0
        assert (idx[m] == np.flatnonzero(m)).all(), (name, spec)
        if name not in LEMMA_FEW:
            assert m.sum() >= 1000, (name, spec, int(m.sum()))
        # |c|^2 overflows there: normals of 0 / NaN, sums with inf - inf
        assert np.isfinite(got["identity", spec][1]).all() == (name not in NONFINITE), (name, spec)
