"""Randomised parity of the RGB-D path (csrc/rgbd_align.hip) against its numpy
truth (tests/rgbd_truth.py), away from the one camera of tests/test_gpu_rgbd.py:
focal lengths with fx != fy (the photometric Jacobian's two constants kx and ky
differ), off-centre principal points and depth scales that between them run all
four variants of k_rgbd_reduce, poses up to 15 degrees, lambda and the distance
gate off their defaults, frames down to 3 x 3, hostile depth and intensity
values, and the streamed paths under such a camera.

The draws are seeded (tests/rgbd_draws.py) and the truth runs on the host.  The
sums compare at the project's bar (rtol 1e-11, atol 1e-9), poses at 1e-9 +
4e-16 cond(A), the bound of
tests/test_gpu_fuzz.py::test_tiny_and_ragged_frames_every_path."""
import numpy as np
import pytest
import torch

import rgbd_draws
import rgbd_truth
import youth_icp
import youth_rgbd
import youth_synth
from test_gpu_fuzz import _pose

pytestmark = pytest.mark.gpu

f32 = np.float32
REST = [k for k in range(31) if k not in (28, 30)]
LAMS = (0.1, 1.0)
THRS = (0.10, 0.05)
MIN_MATCHES = 1000
FUZZ_SIZES = [(160, 120), (162, 122)]
TINY_SIZES = [(3, 3), (4, 3), (5, 4), (8, 8), (31, 7), (65, 3), (3, 65), (130, 66)]


def _dev(a):
    """A device copy, complete before the library's own (non-blocking) stream reads it."""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _scene(index, n, W, H, k):
    """n colour pairs rendered with camera k (None: the viewer's) -> depth and
    intensity of source and target, [n][H][W] each."""
    K = None if k is None else rgbd_draws.intrinsics(k)
    src, dst, _, srgb, drgb = youth_synth.pairs_rgb(index, n, W, H, K=K)
    return src, rgbd_truth.luma(srgb), dst, rgbd_truth.luma(drgb)


def _context(W, H, n, k, **kw):
    return youth_rgbd.RgbdContext(W, H, n, K=None if k is None else rgbd_draws.intrinsics(k), **kw)


def _check_sums(ctx, src, sg, dst, dg, T12, k, thr, lam, tag):
    """ctx.reduce_host against the truth: both counts equal, the other 29 values
    within rtol 1e-11 / atol 1e-9 -> (the truth's sums, the worst error as a
    fraction of that bar)."""
    got = ctx.reduce_host(src, sg, dst, dg, T12)
    want = rgbd_truth.reduce(src, sg, dst, dg, T12, k, thr, lam)
    assert got[28] == want[28] and got[30] == want[30], (tag, got[[28, 30]], want[[28, 30]])
    np.testing.assert_allclose(got[REST], want[REST], rtol=1e-11, atol=1e-9, err_msg=str(tag))
    return want, float((np.abs(got - want) / (1e-9 + 1e-11 * np.abs(want)))[REST].max())


def _pose_bound(src, sg, dst, dg, T64, k, thr, lam):
    """1e-9 + 4e-16 cond(A), A from the truth's sums at its final pose."""
    neq = rgbd_truth.reduce(src, sg, dst, dg, T64[:3].astype(f32), k, thr, lam)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = neq[:21]
    A = A + np.triu(A, 1).T
    with np.errstate(all="ignore"):
        return 1e-9 + 4e-16 * float(np.linalg.cond(A))


def _check_align(ctx, src, sg, dst, dg, k, thr, lam, iters, T_init, tag, only_status0=False):
    """One align_pairs_device call over the given pairs against the truth's
    aligns: statuses and both count rows equal, poses within the cond(A) bound.
    -> (worst pose error, worst error / bound, statuses, the first pair's counts)."""
    n = src.shape[0]
    d = [_dev(a) for a in (src, sg, dst, dg)]
    ctx.align_pairs_device(d[0], d[1], d[2], d[3], n, T_init=T_init)
    T64, _, st = ctx.poses(n)
    stats = ctx.stats(n, iters)
    worst, ratio = 0.0, 0.0
    for p in range(n):
        Ti = None if T_init is None else np.asarray(T_init).reshape(-1, 4, 4)[p]
        T_t, _, st_t, stats_t = rgbd_truth.align(src[p], sg[p], dst[p], dg[p], k, iters, thr, lam,
                                                 T_init=Ti)
        assert st[p] == st_t, (tag, p, st[p], st_t)
        assert np.array_equal(stats[p][:, [1, 3]], stats_t[:, [1, 3]]), \
            (tag, p, stats[p][:, [1, 3]], stats_t[:, [1, 3]])
        if only_status0 and st_t != 0:
            continue
        err = float(np.abs(T64[p, :3] - T_t[:3]).max())
        bound = _pose_bound(src[p], sg[p], dst[p], dg[p], T_t, k, thr, lam)
        assert err <= bound, (tag, p, err, bound)
        worst, ratio = max(worst, err), max(ratio, err / bound)
    return worst, ratio, st, stats[0][:, [1, 3]]


def _sum_cases(W, H):
    """Per draw of camera_draws(W, H): (k, [(pose, lambda, gate)] x 2): a pose of
    at most 2 degrees / 2 cm and one of at most 15 degrees / 10 cm, with
    opposite choices of lambda and the gate.  The seed is one under which every
    case keeps at least MIN_MATCHES matches (the large poses and the 5 cm gate
    leave few under some)."""
    rng = np.random.default_rng(0x5AD7 + W)
    cases = []
    for d, k in enumerate(rgbd_draws.camera_draws(W, H)):
        a, b = d % 2, (d // 2) % 2
        cases.append((k, [(_pose(rng, 2.0, 0.02)[:3].astype(f32), LAMS[a], THRS[b]),
                          (_pose(rng, 15.0, 0.10)[:3].astype(f32), LAMS[1 - a], THRS[1 - b])]))
    return cases


# ---------------------------------------------------------------- coverage --
def test_draws_reach_every_reduce_variant():
    """k_rgbd_reduce<kFast, kAligned>: kFast is the context's fast-division
    verdict, kAligned needs W % 4 == 0 and centred_exact.  The draws give both
    verdicts among the cameras of 160 x 120 that keep the aligned loop and both
    at 162 x 122 (never aligned); the far principal point loses the aligned
    loop at 160 x 120."""
    fast = {}
    for W, H in FUZZ_SIZES:
        for k in rgbd_draws.camera_draws(W, H):
            with youth_icp.IcpContext(W, H, 2, K=rgbd_draws.intrinsics(k)) as icp:
                fast[(W, k)] = icp.fastdiv
    exact = {k: rgbd_draws.centred_exact(k[2], 160) for k in rgbd_draws.camera_draws(160, 120)}
    assert set(exact.values()) == {True, False}
    assert not exact[rgbd_draws.camera_draws(160, 120)[-1]]
    assert all(rgbd_draws.centred_exact(k[2], 162) for k in rgbd_draws.camera_draws(162, 122))
    assert {fast[(160, k)] for k, e in exact.items() if e} == {True, False}
    assert {fast[(162, k)] for k in rgbd_draws.camera_draws(162, 122)} == {True, False}


# -------------------------------------------------------------------- sums --
@pytest.mark.parametrize("W,H", FUZZ_SIZES)
def test_sums_random_intrinsics_and_poses(W, H):
    """Every draw, two poses each: counts 28 and 30 equal the truth's (at least
    1000 matches), the other 29 values within rtol 1e-11 / atol 1e-9, the
    project's bar for these sums.  No value of these draws cancels far enough
    to need more than that bar."""
    worst = 0.0
    for d, (k, poses) in enumerate(_sum_cases(W, H)):
        src, sg, dst, dg = (a[0] for a in _scene(400 + d, 1, W, H, k))
        for T12, lam, thr in poses:
            with _context(W, H, 2, k, lam=lam, dist_thresh=thr) as ctx:
                want, frac = _check_sums(ctx, src, sg, dst, dg, T12, k, thr, lam, (d, k, lam, thr))
            assert want[28] >= MIN_MATCHES and want[30] >= MIN_MATCHES, (d, k, want[[28, 30]])
            worst = max(worst, frac)
    print(f"{W}x{H}: worst sum error {worst:.3f} of the rtol 1e-11 / atol 1e-9 bar")


# ------------------------------------------------------------------ aligns --
@pytest.mark.parametrize("W,H", FUZZ_SIZES)
def test_align_random_intrinsics(W, H):
    """Every draw, 1 and 6 iterations, a pair from a random initial pose (at
    most 2 degrees / 2 cm) and a pair from none: status and per-iteration
    counts equal the truth's, the pose within 1e-9 + 4e-16 cond(A)."""
    rng = np.random.default_rng(0xA119 + W)
    worst, ratio = 0.0, 0.0
    for d, k in enumerate(rgbd_draws.camera_draws(W, H)):
        src, sg, dst, dg = _scene(500 + d, 2, W, H, k)
        lam, thr = LAMS[(d + 1) % 2], THRS[d % 2]
        T_init = _pose(rng, 2.0, 0.02)
        for iters in (1, 6):
            with _context(W, H, 2, k, iters=iters, lam=lam, dist_thresh=thr) as ctx:
                for p, Ti in ((0, T_init[None]), (1, None)):
                    w, r, _, cnt = _check_align(ctx, src[p:p + 1], sg[p:p + 1], dst[p:p + 1],
                                                dg[p:p + 1], k, thr, lam, iters, Ti,
                                                (d, k, iters, p))
                    assert cnt.min() >= MIN_MATCHES, (d, k, iters, p, cnt)
                    worst, ratio = max(worst, w), max(ratio, r)
    print(f"{W}x{H}: max |T - truth| {worst:.3e}, at most {ratio:.3f} of its bound")


# ------------------------------------------------------------- tiny frames --
def _tiny_camera(W, H):
    """A wide camera with fx != fy for a frame of a few pixels."""
    fx = f32(0.9 * max(W, H) + 0.37)
    return tuple(float(f32(v)) for v in (fx, fx * f32(1.3), W / 2 - 0.23, H / 2 + 0.31, 1000.0))


def _prep_check(ctx, W, H, rng):
    rgb = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    rgb[:, :, 0] = 0
    rgb[:, :, W - 1] = 255
    rgb[:, 0, W // 2] = 255
    Y = rgbd_truth.luma(rgb)
    d_gray = torch.full((2, H, W), 7, dtype=torch.uint8, device="cuda")
    d_photo = torch.zeros((2, H * W), dtype=torch.int32, device="cuda")
    d_photo1 = torch.zeros_like(d_photo)
    d_in, d_Y = _dev(rgb), _dev(Y)
    ctx.prep_device(d_in, 3, 2, d_gray, d_photo)
    ctx.prep_device(d_Y, 1, 2, None, d_photo1)
    ctx.sync()
    assert np.array_equal(d_gray.cpu().numpy(), Y)
    words = d_photo.cpu().numpy().view(np.uint32).reshape(2, H, W)
    assert np.array_equal(d_photo1.cpu().numpy().view(np.uint32).reshape(2, H, W), words)
    for f in range(2):
        gx, gy, valid = rgbd_truth.photo_record(Y[f])
        uY, ugx, ugy, uvalid = youth_rgbd.unpack_photo(words[f])
        assert np.array_equal(uY, Y[f]) and np.array_equal(uvalid, valid)
        assert np.array_equal(ugx, gx) and np.array_equal(ugy, gy)


@pytest.mark.parametrize("W,H", TINY_SIZES)
def test_tiny_and_ragged_frames(W, H):
    """Frames down to 3 x 3 and one-row / one-column shapes, under the viewer's
    camera and a wide fx != fy one: the packed photometric words equal numpy's,
    the sums equal the truth's, and a 5-iteration align gives the truth's status
    and both count rows (few or no matches on most of these sizes: the GPU
    reproduces that), poses within the cond(A) bound where the status is 0."""
    rng = np.random.default_rng(0x7111 + W * 131 + H)
    iters = 5
    for k in (None, _tiny_camera(W, H)):
        src, sg, dst, dg = _scene(96, 2, W, H, k)
        T12 = _pose(rng, 1.0, 0.01)[:3].astype(f32)
        with _context(W, H, 2, k, iters=iters) as ctx:
            _prep_check(ctx, W, H, rng)
            want, _ = _check_sums(ctx, src[0], sg[0], dst[0], dg[0], T12, k, 0.10, 0.1, (W, H, k))
            _, _, st, cnt = _check_align(ctx, src, sg, dst, dg, k, 0.10, 0.1, iters, None,
                                         (W, H, k), only_status0=True)
        print(f"{W}x{H} {'viewer' if k is None else 'wide'}: {int(want[28])} matches at the "
              f"pose, align status {st.tolist()}, counts of pair 0 {cnt[:, 0].astype(int).tolist()}")


# ---------------------------------------------------------- hostile pixels --
def _hostile(W, H, k):
    """A pair with holes, negative and saturated depths in both frames, target
    stripes of 0 / 255 (gradients of +-255) and source intensities of 0 and 255."""
    src, sg, dst, dg = (a[0].copy() for a in _scene(600, 1, W, H, k))
    rng = np.random.default_rng(0xBAD0 + W)
    n = W * H
    parts = np.cumsum([int(0.05 * n), int(0.01 * n), int(0.005 * n), int(0.005 * n)])
    for depth in (src, dst):
        idx = rng.permutation(n)
        flat = depth.reshape(-1)
        flat[idx[:parts[0]]] = 0
        flat[idx[parts[0]:parts[1]]] = -1
        flat[idx[parts[1]:parts[2]]] = -32768
        flat[idx[parts[2]:parts[3]]] = 32767
        v0, u0 = int(rng.integers(H // 4, H // 2)), int(rng.integers(W // 4, W // 2))
        depth[v0:v0 + 5, u0:u0 + 9] = 0
    dg[H // 2:, :W // 2] = np.where(np.arange(W // 2) % 4 < 2, 0, 255).astype(np.uint8)[None, :]
    sg[:H // 2, :] = 0
    sg[H // 2:, W // 2:] = 255
    return src, sg, dst, dg


@pytest.mark.parametrize("W,H", [(160, 120), (97, 53)])
def test_hostile_pixels(W, H):
    """Depth holes, -1, -32768 and 32767 in both frames and +-255 gradients
    under matched pixels, lambda 1: the sums equal the truth's; a 3-iteration
    align gives its status, counts and (cond(A) bound) pose."""
    k = rgbd_draws.camera_draws(W, H)[1]
    src, sg, dst, dg = _hostile(W, H, k)
    rng = np.random.default_rng(0xBAD1 + W)
    T12 = _pose(rng, 2.0, 0.02)[:3].astype(f32)
    lam, thr, iters = 1.0, 0.10, 3
    _, _, _, rp, pv, _, j = rgbd_truth.terms(src, sg, dst, dg, T12, k, thr, lam)
    gx = rgbd_truth.photo_record(dg)[0].ravel()[j]
    print(f"{W}x{H}: {j.size} matches, {int((np.abs(gx[pv]) == 255).sum())} with |gx| = 255, "
          f"max |rp| {float(np.abs(rp[pv]).max()):.3f}")
    assert j.size >= MIN_MATCHES
    assert (np.abs(gx[pv]) == 255).sum() >= 100 and np.abs(rp[pv]).max() >= 0.9
    with _context(W, H, 2, k, iters=iters, lam=lam, dist_thresh=thr) as ctx:
        _check_sums(ctx, src, sg, dst, dg, T12, k, thr, lam, (W, H, k))
        w, r, st, cnt = _check_align(ctx, src[None], sg[None], dst[None], dg[None], k, thr, lam,
                                     iters, None, (W, H, k))
    print(f"{W}x{H}: align status {st.tolist()}, max |T - truth| {w:.3e}, {r:.3f} of its bound")
    assert cnt.min() >= MIN_MATCHES


# ---------------------------------------------------------- streamed paths --
def test_streamed_paths_with_unequal_focals(monkeypatch):
    """align_sequence_device, track_host_sequence and track_submit /
    track_collect under an fx != fy camera: bit for bit the pairwise align
    under the same camera (one launch shape: YOUTH_RGBD_CHUNKS fixed)."""
    monkeypatch.setenv("YOUTH_RGBD_CHUNKS", "7")
    W, H, n = 128, 96, 6
    k = rgbd_draws.camera_draws(W, H)[0]
    fr, _, rgb = youth_synth.sequence_rgb(0, n, W, H, K=rgbd_draws.intrinsics(k))
    g = rgbd_truth.luma(rgb)
    with _context(W, H, n - 1, k) as ctx:
        d = [_dev(a) for a in (fr[1:], g[1:], fr[:-1], g[:-1])]
        ctx.align_pairs_device(d[0], d[1], d[2], d[3], n - 1)
        T_pair, _, st_pair = ctx.poses(n - 1)
        stats_pair = ctx.stats(n - 1)
        ctx.align_sequence_device(_dev(fr), _dev(g), n)
        T_seq, _, st_seq = ctx.poses(n - 1)
        stats_seq = ctx.stats(n - 1)
        T_host, st_host = ctx.track_host_sequence(fr, rgb)
    with _context(W, H, 8, k) as ctx:
        assert ctx.track_set_batch(4) == 1
        ctx.track_submit(list(fr[:2]), list(rgb[:2]))
        ctx.track_submit(list(fr[2:]), list(rgb[2:]))
        got = [ctx.track_collect() for _ in range(n)]
    assert st_pair.max() == 0 and stats_pair[:, :, 1].min() >= MIN_MATCHES
    T_host[:, 3, :] = (0.0, 0.0, 0.0, 1.0)
    assert [h for _, h, _ in got] == [0] + [1] * (n - 1) and np.array_equal(got[0][0], np.eye(4))
    T_trk = np.array([t for t, _, _ in got[1:]])
    st_trk = np.array([s for _, _, s in got[1:]])
    for T, st in ((T_seq, st_seq), (T_host, st_host), (T_trk, st_trk)):
        assert np.array_equal(T.view(np.uint64), T_pair.view(np.uint64))
        assert np.array_equal(st, st_pair)
    assert np.array_equal(stats_seq.view(np.uint64), stats_pair.view(np.uint64))
    # and the camera matters: the viewer's gives other poses on these frames
    with youth_rgbd.RgbdContext(W, H, n - 1) as ctx:
        ctx.align_pairs_device(d[0], d[1], d[2], d[3], n - 1)
        T_def, _, _ = ctx.poses(n - 1)
    assert np.abs(T_def - T_pair).max() > 1e-6
