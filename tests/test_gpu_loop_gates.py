"""The four gate values of youth_loop_close (include/youth_loop.h, DESIGN.md
§15) against independent computations: every verified pair against the same
two alignments done directly on an RgbdContext and put through
loop_truth.gates, with and without a level schedule; the C5 revisit against
the numpy alignment; every gate rejecting on its own; the status gate; and the
host and device ways of adding a keyframe."""
import numpy as np
import pytest
import torch

import loop_truth
import rgbd_truth
import youth_icp
import youth_loop
import youth_rgbd
import youth_synth

pytestmark = pytest.mark.gpu

K160 = (142.575, 142.575, 80.0, 60.0, 1000.0)
W, H, N = 160, 120, 160 * 120
WIDE = 65535 + 64 * 255          # max_cell_dist: every earlier keyframe is a candidate
OPEN = dict(min_overlap=0.0, max_gray_rms=1e30, fb_rot_deg=1e30, fb_trans_m=1e30)
GATES = ("overlap", "gray_rms", "fb_rot_deg", "fb_trans_m")

# --- bars against the direct alignment -------------------------------------
# The project's launch-shape bar (test_launch_shape_moves_only_the_last_bits):
# poses within 1e-9 per entry, both counts equal at every iteration.
POSE_BAR = 1e-9
# E = T_fwd T_bwd.  With every entry of both poses within d: an entry of R_E
# moves by at most sum_k |dA_ik| |B_kj| + |A_ik| |dB_kj| <= 2 sqrt(3) d (rows and
# columns of a rotation have 1-norm <= sqrt(3)).  v is half a difference of two
# entries, so |dv_i| <= 2 sqrt(3) d and d|v| <= 6 d; the cosine term is half a sum
# of three, <= 3 sqrt(3) d.  atan2's gradient has norm 1 on the unit circle, so
# the angle moves by at most sqrt(36 + 27) d < 8 d rad.
ROT_BAR_DEG = float(np.degrees(8 * POSE_BAR))                   # 4.6e-7 deg


def _trans_bar(t_bwd):
    """t_E = R_f t_b + t_f: per component <= d (3 |t_b|_inf + sqrt(3) + 1), the norm sqrt(3) times that."""
    return float(np.sqrt(3) * POSE_BAR * (3 * np.abs(t_bwd).max() + np.sqrt(3) + 1))


# The RMS is no smooth function of the pose: a pixel's terms are fp32 functions
# of the fp32 pose and of the nearest target pixel.  What the launch-shape bar
# adds is that both counts are equal at every iteration, so the association is
# the same, and an fp64 pose within 1e-9 rounds to the same fp32 pose away from
# a rounding boundary.  The terms of sum rp^2 are then the same numbers and only
# their order differs: two fp64 sums of N = 19200 non-negative terms differ by at
# most 2 N 2^-53 = 4.3e-12 relative, the root by half of it.  The bar is the
# pose's own 1e-9, relative: the same head-room over the sums' rounding.
RMS_BAR_REL = 1e-9

# --- bars against the numpy truth (the C5 revisit, edge (0, 16)) -----------
# The project's pose bar against rgbd_truth.align is 1e-5 per entry.  Two poses
# each within 1e-5 move an entry of their product by at most about 6e-5 (three
# or four products per entry, each factor at most about 1: 2 sqrt(3) 1e-5 for
# the rotation, (3 |t_b| + sqrt(3) + 1) 1e-5 for the translation, both below
# 6e-5 here).  v is half a difference of two entries: |dv| <= sqrt(3) 6e-5 rad =
# 0.006 deg at this small angle; the translation norm: sqrt(3) 6e-5 = 0.104 mm.
TRUTH_ROT_BAR_DEG = float(np.degrees(np.sqrt(3) * 6e-5))
TRUTH_TRANS_BAR_M = float(np.sqrt(3) * 6e-5)
# gray_rms against the truth: nothing to derive it from (it rides on where ten
# iterations land).  Measured on the MI355X: GPU - truth = -1.138e-8 grey levels
# at a truth of 0.7638 (the closer divides by the fp32 lambda 0.1f, the truth by
# 0.1: 0.7638 x 1.49e-8; the alignments themselves agree far closer here, the
# fb values to 9e-14 deg and 5e-13 mm).  The bar is ten times the observed
# difference and must stay below 1 % of the 1.5 threshold.
RMS_OBSERVED = 1.14e-8
TRUTH_RMS_BAR = 10 * RMS_OBSERVED
assert TRUTH_RMS_BAR < 0.01 * 1.5


def _dev(a):
    """A device copy, complete before the library's own (non-blocking) stream reads it."""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def kfs():
    """The 17 C5 keyframes (frames 0, 40, ..., 600, 630 at 160 x 120 under K160)."""
    K = youth_icp.Intrinsics(*K160)
    fr, X, rgb = [], [], []
    for f in loop_truth.KF_FRAMES:
        a, T, c = youth_synth.sequence_rgb(f, 1, W, H, K=K)
        fr.append(a[0]), X.append(T[0]), rgb.append(c[0])
    fr, X, rgb = np.array(fr), np.array(X), np.array(rgb)
    gray = youth_synth.luma(rgb)
    sig = np.array([loop_truth.signature(fr[k], gray[k]) for k in range(17)])
    return dict(fr=fr, X=X, rgb=rgb, gray=gray, sig=sig, K=K)


@pytest.fixture(scope="module")
def truth16(kfs):
    """rgbd_truth.align of the revisit both ways: forward is source 16, target 0."""
    fr, g, K = kfs["fr"], kfs["gray"], kfs["K"]
    fwd = rgbd_truth.align(fr[16], g[16], fr[0], g[0], K=K)
    bwd = rgbd_truth.align(fr[0], g[0], fr[16], g[16], K=K)
    assert fwd[2] == 0 and bwd[2] == 0
    return dict(fwd=fwd, bwd=bwd, cnt=int(min(fwd[3][-1, 1], bwd[3][-1, 1])),
                gates=loop_truth.gates(fwd[0], fwd[3], bwd[0], bwd[3], N, 0.1))


def _direct(ctx, kfs, q, cand, levels):
    """Keyframe q against every candidate, both ways, on a plain context: pair
    2 p forward (source q), 2 p + 1 backward, which is not the closer's order.
    -> (T64 [2K], status [2K], the last level's statistics [2K, iters, 4])."""
    fr, g = kfs["fr"], kfs["gray"]
    src = [q if d == 0 else k for k in cand for d in (0, 1)]
    dst = [k if d == 0 else q for k in cand for d in (0, 1)]
    n = len(src)
    ctx.set_levels(levels)
    ctx.align_pairs_device(_dev(fr[src]), _dev(g[src]), _dev(fr[dst]), _dev(g[dst]), n)
    T64, _, st = ctx.poses(n)
    if levels:
        stats = ctx.level_stats(len(levels) - 1, n, levels[-1][1])
    else:
        stats = ctx.stats(n)
    return T64, st, stats


def _same(a, b, bar):
    """Within bar, or the same non-finite value."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.all((a == b) | (np.abs(a - b) <= bar)))


def _verify(lc, ctx, kfs, q, levels, worst):
    """close(q) on lc against the direct alignments.  -> per pair (cnt_f, cnt_b,
    rms_f, rms_b, the statistics of both ways)."""
    P = lc.params
    lc.set_levels(levels)
    cand = lc.candidates(q)[0].tolist()
    assert cand == loop_truth.candidates(lc.distances(kfs["sig"][q:q + 1])[0], q, P.min_gap, WIDE, 16)
    assert len(cand) == q - 1
    before = lc.edges()
    added = lc.close(q)
    v = lc.last_verified()
    new = lc.edges()[before.shape[0]:]
    assert [(int(e["i"]), int(e["j"])) for e in v] == [(k, q) for k in cand]
    T, st, stats = _direct(ctx, kfs, q, cand, levels)
    out = []
    for p, e in enumerate(v):
        f, b = 2 * p, 2 * p + 1
        ov, rms, rot, trans = loop_truth.gates(T[f], stats[f], T[b], stats[b], N, ctx.params.lam)
        what = (levels, int(e["i"]), q)
        assert e["overlap"] == ov, what
        assert _same(e["Z"], T[f], POSE_BAR), what
        assert _same(e["gray_rms"], rms, RMS_BAR_REL * max(1.0, rms)), (what, e["gray_rms"], rms)
        assert _same(e["fb_rot_deg"], rot, ROT_BAR_DEG), (what, e["fb_rot_deg"], rot)
        assert _same(e["fb_trans_m"], trans, _trans_bar(T[b][:3, 3])), (what, e["fb_trans_m"], trans)
        if np.isfinite(T[f]).all():
            worst["Z"] = max(worst["Z"], float(np.abs(e["Z"] - T[f]).max()))
        if np.isfinite(rms):
            worst["gray_rms"] = max(worst["gray_rms"], abs(e["gray_rms"] - rms) / max(1.0, rms))
        worst["fb_rot_deg"] = max(worst["fb_rot_deg"], abs(e["fb_rot_deg"] - rot))
        worst["fb_trans_m"] = max(worst["fb_trans_m"], abs(e["fb_trans_m"] - trans))
        # the decision: both statuses 0, finite poses, the four gates on the closer's own values
        ok = (st[f] == 0 and st[b] == 0 and np.isfinite(T[f]).all() and np.isfinite(T[b]).all()
              and e["overlap"] >= P.min_overlap and e["gray_rms"] <= P.max_gray_rms
              and e["fb_rot_deg"] <= P.fb_rot_deg and e["fb_trans_m"] <= P.fb_trans_m)
        assert e["w"] == (1.0 if ok else 0.0), what
        out.append((stats[f], stats[b]))
    assert added == int((v["w"] == 1.0).sum()) == new.shape[0]
    assert new.tobytes() == v[v["w"] == 1.0].tobytes()
    return v, out


def _directions(stats_f, stats_b):
    """(the way with the smaller count, the way with the larger RMS), 0 forward, 1
    backward, None on a tie or without photometric pixels."""
    cf, cb = stats_f[-1, 1], stats_b[-1, 1]
    if min(stats_f[-1, 3], stats_b[-1, 3]) <= 0 or cf == cb:
        return None
    rf, rb = stats_f[-1, 2] / stats_f[-1, 3], stats_b[-1, 2] / stats_b[-1, 3]
    return (0 if cf < cb else 1), (0 if rf > rb else 1)


SCHEDULES = [None, [(2, 10), (1, 10)], [(2, 10), (1, 6)]]


def test_every_verified_pair_against_the_direct_alignment(kfs):
    """K = 15 (30 pairs in one batch) and K = 8, then K = 15 under two schedules;
    the second one's last level has 6 iterations where the context has 10.
    Worst observed on the MI355X over the 53 pairs: Z and gray_rms equal bit
    for bit, fb_rot_deg 2.8e-14 deg, fb_trans_m 4.4e-16 m."""
    worst = dict.fromkeys(("Z",) + GATES[1:], 0.0)
    with youth_loop.LoopCloser(W, H, 32, K=kfs["K"], min_gap=2, max_candidates=16,
                               max_cell_dist=WIDE) as lc, \
            youth_rgbd.RgbdContext(W, H, 32, K=kfs["K"]) as ctx:
        for k in range(17):
            assert lc.add_keyframe(kfs["fr"][k], kfs["rgb"][k], kfs["X"][k]) == k
        for levels, qs in zip(SCHEDULES, ((16, 9), (16,), (16,))):
            for q in qs:
                v, stats = _verify(lc, ctx, kfs, q, levels, worst)
                if q != 16:
                    continue
                # the inputs can show the mistakes: counts that differ between the
                # ways, a pair where min and max pick different ways, a last
                # iteration that is not the one before it (nor, under a
                # schedule, the first level's last)
                assert any(f[-1, 1] != b[-1, 1] for f, b in stats)
                dirs = [_directions(f, b) for f, b in stats]
                assert any(d is not None and d[0] != d[1] for d in dirs), dirs
                assert any(f[-1, 1] != f[-2, 1] and f[-1, 2] != f[-2, 2] for f, _ in stats)
                if levels:
                    first = ctx.level_stats(0, 2 * len(stats), levels[0][1])
                    assert any(first[2 * p, -1, 1] != f[-1, 1] for p, (f, _) in enumerate(stats))
        assert lc.levels() == SCHEDULES[-1]
    print("closer against the direct alignment, worst: " +
          ", ".join(f"{k} {x:.2e}" for k, x in worst.items()))


def test_the_revisit_against_the_numpy_truth(kfs, truth16):
    """Edge (0, 16) with the other fourteen candidates in the same batch."""
    with youth_loop.LoopCloser(W, H, 32, K=kfs["K"], min_gap=2, max_candidates=16,
                               max_cell_dist=WIDE) as lc:
        for k in range(17):
            lc.add_keyframe(kfs["fr"][k], kfs["rgb"][k], kfs["X"][k])
        assert lc.close(16) >= 1
        v = lc.last_verified()
    e = v[[int(i) for i in v["i"]].index(0)]
    ov, rms, rot, trans = truth16["gates"]
    print(f"(0, 16) GPU - truth: overlap {e['overlap'] - ov:.1e}, grey rms {e['gray_rms'] - rms:.3e} "
          f"(truth {rms:.4f}), fb {e['fb_rot_deg'] - rot:.3e} deg (truth {rot:.5f}), "
          f"{(e['fb_trans_m'] - trans) * 1e3:.3e} mm (truth {trans * 1e3:.4f})")
    assert e["w"] == 1.0
    assert e["overlap"] == ov == truth16["cnt"] / N
    assert np.abs(e["Z"][:3] - truth16["fwd"][0][:3]).max() <= 1e-5
    assert abs(e["fb_rot_deg"] - rot) <= TRUTH_ROT_BAR_DEG
    assert abs(e["fb_trans_m"] - trans) <= TRUTH_TRANS_BAR_M
    assert abs(e["gray_rms"] - rms) <= TRUTH_RMS_BAR


def _pair_closer(kfs, **params):
    """Keyframes 0 and 16 alone, stored as 0 and 1."""
    lc = youth_loop.LoopCloser(W, H, 2, K=kfs["K"], min_gap=1, max_candidates=1, max_cell_dist=WIDE,
                               **params)
    for k in (0, 16):
        lc.add_keyframe(kfs["fr"][k], kfs["rgb"][k], kfs["X"][k])
    return lc


@pytest.mark.parametrize("gate", GATES)
def test_each_gate_rejects_alone(kfs, truth16, gate):
    """The other three thresholds wide open (finite: the parameters refuse inf),
    the tested one just on the wrong side of the truth's value, then just on the
    right side.  The margins (half a pixel; twice the bar against the truth)
    keep the fp32 rounding of the threshold and the GPU's distance from the
    truth out of the decision.  The truth's fb values, 0.0019 deg and 0.15 mm,
    are below twice their bars and the parameters refuse a negative threshold,
    so there the wrong side is 0: the gate is `value <= threshold` and the
    value is not 0."""
    ov, rms, rot, trans = truth16["gates"]
    cnt = truth16["cnt"]
    name = {"overlap": "min_overlap", "gray_rms": "max_gray_rms", "fb_rot_deg": "fb_rot_deg",
            "fb_trans_m": "fb_trans_m"}[gate]
    value, bar = {"gray_rms": (rms, TRUTH_RMS_BAR), "fb_rot_deg": (rot, TRUTH_ROT_BAR_DEG),
                  "fb_trans_m": (trans, TRUTH_TRANS_BAR_M), "overlap": (ov, None)}[gate]
    if gate == "overlap":
        wrong, right = (cnt + 0.5) / N, (cnt - 0.5) / N
    else:
        wrong, right = max(value - 2 * bar, 0.0), value + 2 * bar
    for threshold, want in ((wrong, 0), (right, 1)):
        with _pair_closer(kfs, **{**OPEN, name: threshold}) as lc:
            assert lc.close(1) == want
            v, edges = lc.last_verified(), lc.edges()
        assert v.shape[0] == 1 and (int(v[0]["i"]), int(v[0]["j"])) == (0, 1)
        assert v[0]["w"] == float(want) and edges.shape[0] == want
        if want:
            assert edges.tobytes() == v.tobytes()
        # rejected or not, the measures are reported
        assert v[0]["overlap"] == ov and abs(v[0]["gray_rms"] - rms) <= TRUTH_RMS_BAR
        assert abs(v[0]["fb_rot_deg"] - rot) <= TRUTH_ROT_BAR_DEG and v[0]["fb_rot_deg"] > 0.0
        assert abs(v[0]["fb_trans_m"] - trans) <= TRUTH_TRANS_BAR_M and v[0]["fb_trans_m"] > 0.0
        assert np.abs(v[0]["Z"][:3] - truth16["fwd"][0][:3]).max() <= 1e-5


def test_status_rejects_whatever_the_thresholds(kfs):
    """A keyframe without depth and one with three lone valid pixels: no
    alignment there (status not 0), so no edge although every gate is open."""
    fr, rgb, X = kfs["fr"], kfs["rgb"], kfs["X"]
    empty = np.zeros_like(fr[0])
    three = np.zeros_like(fr[0])
    three[30, 40], three[60, 80], three[90, 120] = 1500, 1600, 1700
    with youth_loop.LoopCloser(W, H, 4, K=kfs["K"], min_gap=1, max_candidates=4, max_cell_dist=WIDE,
                               **OPEN) as lc:
        lc.add_keyframe(empty, rgb[0], X[0])
        lc.add_keyframe(three, rgb[0], X[0])
        lc.add_keyframe(fr[0], rgb[0], X[0])
        assert sorted(lc.candidates(2)[0].tolist()) == [0, 1]
        assert lc.close(2) == 0
        v = lc.last_verified()
        assert v.shape[0] == 2 and (v["w"] == 0.0).all() and lc.edges().shape[0] == 0
        assert (v["overlap"] == 0.0).all() and np.isinf(v["gray_rms"]).all()
        # the same store still verifies a pair that aligns: the frame against itself
        lc.add_keyframe(fr[0], rgb[0], X[0])
        assert lc.close(3) == 1
        v = lc.last_verified()
        assert [(int(e["i"]), e["w"]) for e in v] == [(2, 1.0), (0, 0.0), (1, 0.0)]
        assert lc.edges().tobytes() == v[:1].tobytes()


def test_host_add_equals_device_add(kfs):
    fr, rgb, X = kfs["fr"], kfs["rgb"], kfs["X"]
    ks = (0, 5, 9, 16)
    sigs = np.array([loop_truth.signature(fr[k], kfs["gray"][k]) for k in ks])
    res = []
    for device in (False, True):
        with youth_loop.LoopCloser(W, H, 4, K=kfs["K"], min_gap=1, max_candidates=4,
                                   max_cell_dist=WIDE) as lc:
            for k in ks:
                if device:
                    d, g = _dev(fr[k]), youth_rgbd.luma_device(_dev(rgb[k]))
                    torch.cuda.synchronize()
                    lc.add_keyframe_device(d.data_ptr(), g.data_ptr(), X[k])
                else:
                    lc.add_keyframe(fr[k], rgb[k], X[k])
            D = lc.distances(sigs)
            added = lc.close(3)
            res.append((D, added, lc.last_verified(), lc.edges()))
    (D0, a0, v0, e0), (D1, a1, v1, e1) = res
    assert np.array_equal(D0, D1) and (np.diag(D0) == 0).all() and D0[3, 0] > 0
    assert a0 == a1 == 1 and v0.shape[0] == 3
    assert v0.tobytes() == v1.tobytes() and e0.tobytes() == e1.tobytes()
