"""RGB-D alignment on the GPU (include/youth_rgbd.h) against
its numpy truth (tests/rgbd_truth.py), the C oracle at lambda = 0 and the
depth-only ICP path."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import rgbd_truth
import youth_icp
import youth_rgbd
import youth_synth

pytestmark = pytest.mark.gpu

f32 = np.float32


def _dev(a):
    """A device copy, complete before the library's own (non-blocking) stream reads it."""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _poses3():
    """identity, a small motion, 3 degrees / 4 cm (tests/test_oracle_numpy.py)."""
    th = np.deg2rad(3.0)
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    return [np.eye(4)[:3].astype(f32),
            np.hstack([np.eye(3), [[0.004], [-0.002], [0.003]]]).astype(f32),
            np.hstack([R, [[0.04], [0.01], [-0.02]]]).astype(f32)]


@pytest.fixture(scope="module")
def pairs160():
    """4 colour pairs of 160x120 and the truth's aligns of them at lambda 0.1."""
    src, dst, T_gt, srgb, drgb = youth_synth.pairs_rgb(0, 4, 160, 120)
    sg, dg = rgbd_truth.luma(srgb), rgbd_truth.luma(drgb)
    truth = [rgbd_truth.align(src[p], sg[p], dst[p], dg[p], lam=0.1) for p in range(4)]
    return src, sg, dst, dg, truth


def _align_pairs(ctx, src, sg, dst, dg, T_init=None):
    n = src.shape[0]
    d = [_dev(a) for a in (src, sg, dst, dg)]
    ctx.align_pairs_device(d[0], d[1], d[2], d[3], n, T_init=T_init)
    T64, _, st = ctx.poses(n)
    return T64, st, ctx.stats(n)


# -------------------------------------------------------------------- prep --
@pytest.mark.parametrize("W,H,offset", [(97, 53, 0), (160, 120, 0), (160, 120, 1)],
                         ids=["97x53", "160x120", "160x120_offset1"])
def test_prep_equals_numpy(W, H, offset):
    rng = np.random.default_rng(W + offset)
    rgb = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    rgb[:, :, 5] = 0
    rgb[:, :, 6] = 255
    rgb[:, :, 7] = 255
    rgb[:, :, 8] = 0
    rgb[:, :, W - 1] = 255
    rgb[:, 0, :] = 0
    buf = torch.zeros(rgb.size + offset, dtype=torch.uint8, device="cuda")
    d_in = buf[offset:]
    d_in.copy_(torch.from_numpy(rgb.reshape(-1)))
    assert d_in.data_ptr() % 4 == offset
    d_gray = torch.full((2, H, W), 7, dtype=torch.uint8, device="cuda")
    d_photo = torch.zeros((2, H * W), dtype=torch.int32, device="cuda")
    Y = rgbd_truth.luma(rgb)
    d_photo1 = torch.zeros_like(d_photo)
    torch.cuda.synchronize()
    with youth_rgbd.RgbdContext(W, H, 2) as ctx:
        ctx.prep_device(d_in, 3, 2, d_gray, d_photo)
        ctx.sync()
        got_Y = d_gray.cpu().numpy()
        words = d_photo.cpu().numpy().view(np.uint32).reshape(2, H, W)
        # the grey path: the same words from the intensity frames
        ctx.prep_device(_dev(Y), 1, 2, None, d_photo1)
        ctx.sync()
        words1 = d_photo1.cpu().numpy().view(np.uint32).reshape(2, H, W)
    assert np.array_equal(got_Y, Y)
    for f in range(2):
        gx, gy, valid = rgbd_truth.photo_record(Y[f])
        uY, ugx, ugy, uvalid = youth_rgbd.unpack_photo(words[f])
        assert np.array_equal(uY, Y[f])
        assert np.array_equal(ugx, gx) and np.array_equal(ugy, gy)
        assert np.array_equal(uvalid, valid)
        assert abs(gx).max() == 255
    assert np.array_equal(words1, words)


# -------------------------------------------------------------------- sums --
@pytest.mark.parametrize("W,H", [(80, 60), (97, 53), (160, 120)])
def test_sums_against_truth_and_oracle(W, H):
    src, dst, _, srgb, drgb = youth_synth.pairs_rgb(11, 1, W, H)
    src, dst = src[0], dst[0]
    sg, dg = rgbd_truth.luma(srgb[0]), rgbd_truth.luma(drgb[0])
    K = oracle.viewer_K(W, H)
    rest = [k for k in range(31) if k not in (28, 30)]
    with youth_rgbd.RgbdContext(W, H, 2, lam=0.1) as ctx, \
            youth_rgbd.RgbdContext(W, H, 2, lam=0.0) as ctx0:
        for T12 in _poses3():
            got = ctx.reduce_host(src, sg, dst, dg, T12)
            want = rgbd_truth.reduce(src, sg, dst, dg, T12, K, 0.10, 0.1)
            assert got[28] == want[28] > 0 and got[30] == want[30] > 0
            np.testing.assert_allclose(got[rest], want[rest], rtol=1e-11, atol=1e-9)
            got0 = ctx0.reduce_host(src, sg, dst, dg, T12)
            with oracle.spec("survey"):
                o = oracle.reduce(src, dst, T12, K, 0.10)
            assert got0[28] == o[28] and got0[29] == 0.0
            np.testing.assert_allclose(got0[:28], o[:28], rtol=1e-11, atol=1e-9)


# ----------------------------------------------------------------- aligns --
def test_lambda_zero_is_the_depth_only_align(pairs160):
    src, sg, dst, dg, _ = pairs160
    with youth_icp.IcpContext(160, 120, 4) as icp:
        ds, dd = _dev(src), _dev(dst)
        icp.align_pairs_device(ds.data_ptr(), dd.data_ptr(), 4)
        T_icp, _, st_icp = icp.get_poses(4)
        cnt_icp, r2_icp = icp.get_stats(4, 10)
    with youth_rgbd.RgbdContext(160, 120, 4, lam=0.0) as ctx:
        T, st, stats = _align_pairs(ctx, src, sg, dst, dg)
    assert np.abs(T[:, :3] - T_icp[:, :3]).max() <= 1e-9
    assert np.array_equal(st, st_icp)
    assert np.array_equal(stats[:, :, 1], cnt_icp)
    assert np.array_equal(stats[:, :, 3], cnt_icp) and not stats[:, :, 2].any()


@pytest.mark.parametrize("W,H,fastdiv", [(97, 53, True), (160, 120, True), (160, 120, False),
                                         (97, 53, False)],
                         ids=["97x53_unaligned", "160x120_aligned", "160x120_ieee_division",
                              "97x53_unaligned_ieee_division"])
def test_lambda_zero_equals_the_per_iteration_align_bit_for_bit(W, H, fastdiv, monkeypatch):
    """k_rgbd_reduce and k_reduce's fused solve run one text of a7-a9, of the
    wave sum and of the hand-off (csrc/icp_device.h), on the same chunks: at
    lambda 0 (photometric products of +-0 onto sums that are never -0) the
    RGB-D align is the depth-only per-iteration align, bit for bit."""
    src, dst, _, srgb, drgb = youth_synth.pairs_rgb(0, 2, W, H)
    sg, dg = rgbd_truth.luma(srgb), rgbd_truth.luma(drgb)
    monkeypatch.setenv("YOUTH_ICP_NO_COOP", "1")
    monkeypatch.setenv("YOUTH_ICP_NO_PERSISTENT", "1")
    if not fastdiv:
        monkeypatch.setenv("YOUTH_ICP_NO_FASTDIV", "1")
    with youth_icp.IcpContext(W, H, 2) as icp:
        ds, dd = _dev(src), _dev(dst)
        icp.align_pairs_device(ds.data_ptr(), dd.data_ptr(), 2)
        T_icp, _, st_icp = icp.get_poses(2)
        cnt_icp, r2_icp = icp.get_stats(2, 10)
        assert "per-iteration" in icp.get_plan()["kernel"]
        assert fastdiv or not icp.fastdiv
    with youth_rgbd.RgbdContext(W, H, 2, lam=0.0) as ctx:
        T, st, stats = _align_pairs(ctx, src, sg, dst, dg)
    assert cnt_icp.min() > 0
    assert np.array_equal(np.ascontiguousarray(T[:, :3]).view(np.uint64),
                          np.ascontiguousarray(T_icp[:, :3]).view(np.uint64))
    assert np.array_equal(st, st_icp)
    assert np.array_equal(stats[:, :, 1].copy().view(np.uint64), cnt_icp.view(np.uint64))
    assert np.array_equal(stats[:, :, 0].copy().view(np.uint64), r2_icp.view(np.uint64))


def test_pose_against_truth(pairs160):
    src, sg, dst, dg, truth = pairs160
    with youth_rgbd.RgbdContext(160, 120, 4) as ctx:
        T, st, stats = _align_pairs(ctx, src, sg, dst, dg)
    worst = 0.0
    for p in range(4):
        T64, _, st_t, stats_t = truth[p]
        worst = max(worst, float(np.abs(T[p, :3] - T64[:3]).max()))
        assert st[p] == st_t
        assert np.array_equal(stats[p, 0, [1, 3]], stats_t[0, [1, 3]])   # same start, same matches
    fr, _, rgb = youth_synth.sequence_rgb(0, 2)
    g = rgbd_truth.luma(rgb)
    T64, _, _, _ = rgbd_truth.align(fr[1], g[1], fr[0], g[0], lam=0.1)
    with youth_rgbd.RgbdContext(640, 480, 2) as ctx:
        T, st, _ = _align_pairs(ctx, fr[1:2], g[1:2], fr[0:1], g[0:1])
    big = float(np.abs(T[0, :3] - T64[:3]).max())
    print(f"max |T - truth|: 160x120 {worst:.3e}, 640x480 {big:.3e}")
    assert worst <= 1e-5 and big <= 1e-5 and st[0] == 0


@pytest.mark.parametrize("W,H", [(97, 53), (160, 120)])
def test_launch_shape_moves_only_the_last_bits(W, H, monkeypatch):
    src, dst, _, srgb, drgb = youth_synth.pairs_rgb(20, 2, W, H)
    sg, dg = rgbd_truth.luma(srgb), rgbd_truth.luma(drgb)
    res = []
    for chunks in ("1", "7", None, "7"):
        if chunks is None:
            monkeypatch.delenv("YOUTH_RGBD_CHUNKS", raising=False)
        else:
            monkeypatch.setenv("YOUTH_RGBD_CHUNKS", chunks)
        with youth_rgbd.RgbdContext(W, H, 2) as ctx:
            res.append(_align_pairs(ctx, src, sg, dst, dg))
    T0, st0, stats0 = res[0]
    assert stats0[:, :, 1].min() > 0
    for T, st, stats in res[1:]:
        assert np.abs(T - T0).max() <= 1e-9
        assert np.array_equal(st, st0)
        assert np.array_equal(stats[:, :, [1, 3]], stats0[:, :, [1, 3]])
    # the same shape again: bit for bit
    assert np.array_equal(res[3][0].view(np.uint64), res[1][0].view(np.uint64))
    assert np.array_equal(res[3][2].view(np.uint64), res[1][2].view(np.uint64))


def test_sequence_and_host_paths_equal_the_pairwise_align():
    W, H, n = 128, 96, 6
    fr, _, rgb = youth_synth.sequence_rgb(0, n, W, H)
    g = rgbd_truth.luma(rgb)
    d_gray = youth_rgbd.luma_device(_dev(rgb))
    torch.cuda.synchronize()
    assert np.array_equal(d_gray.cpu().numpy(), g)          # RGB in = grey in
    with youth_rgbd.RgbdContext(W, H, n - 1) as ctx:
        T_pair, st_pair, stats_pair = _align_pairs(ctx, fr[1:], g[1:], fr[:-1], g[:-1])
        d_T = torch.zeros((n - 1, 16), dtype=torch.float32, device="cuda")
        d_depth = _dev(fr)
        torch.cuda.synchronize()
        ctx.align_sequence_device(d_depth, d_gray, n, d_T_out=d_T)
        T_seq, T32_seq, st_seq = ctx.poses(n - 1)
        assert np.array_equal(d_T.cpu().numpy().reshape(-1, 4, 4), T32_seq)
        stats_seq = ctx.stats(n - 1)
        T_host, st_host = ctx.track_host_sequence(fr, rgb)
    assert st_pair.max() == 0
    for T, st in ((T_seq, st_seq), (T_host, st_host)):
        assert np.array_equal(T.view(np.uint64), T_pair.view(np.uint64))
        assert np.array_equal(st, st_pair)
    assert np.array_equal(stats_seq.view(np.uint64), stats_pair.view(np.uint64))


# -------------------------------------------------------- the feature test --
def test_colour_settles_the_flat_valley():
    """Frames 0-7 of the 640x480 sequence: depth alone slides along the wall
    (>= 1 degree on pair 0->1); with the photometric term the pair and the
    composed pose at frame 7 are within the bounds of the definition
    (tests/test_rgbd.py)."""
    fr, Twc, rgb = youth_synth.sequence_rgb(0, 8)
    with youth_rgbd.RgbdContext(640, 480, 8) as ctx:
        T_rel, st = ctx.track_host_sequence(fr, rgb)
    assert T_rel.shape == (7, 4, 4) and not st.any()
    gt01 = np.linalg.inv(Twc[0]) @ Twc[1]
    e01 = rgbd_truth.pose_error(T_rel[0], gt01)
    T = np.eye(4)
    for k in range(7):
        T = T @ T_rel[k]
    e7 = rgbd_truth.pose_error(T, np.linalg.inv(Twc[0]) @ Twc[7])
    with youth_icp.IcpContext(640, 480, 4) as icp:
        T_icp, _ = icp.track_host_sequence(fr[:2])
    e_icp = rgbd_truth.pose_error(T_icp[-1], gt01)
    print(f"pair 0->1: rgbd {e01[0]:.4f} deg / {e01[1]:.3f} mm, depth only {e_icp[0]:.3f} deg / "
          f"{e_icp[1]:.2f} mm; frame 7: {e7[0]:.4f} deg / {e7[1]:.3f} mm")
    assert e01[0] <= rgbd_truth.BOUND_PAIR_0_1[0] and e01[1] <= rgbd_truth.BOUND_PAIR_0_1[1]
    assert e7[0] <= rgbd_truth.BOUND_FRAME_7[0] and e7[1] <= rgbd_truth.BOUND_FRAME_7[1]
    assert e_icp[0] >= 1.0


# --------------------------------------------------------------- arguments --
def test_bad_arguments_are_refused_and_leave_the_context_intact(pairs160):
    src, sg, dst, dg, _ = pairs160
    lib = youth_rgbd.load_library()
    EINVAL = youth_icp.YOUTH_EINVAL

    def refused(fn, *a, **kw):
        with pytest.raises(youth_icp.IcpError) as ei:
            fn(*a, **kw)
        assert ei.value.code == EINVAL
        assert len(str(ei.value)) > len("youth_icp error -1: ")

    for kw in (dict(width=2), dict(height=2), dict(width=16385), dict(max_frames=1),
               dict(lam=-0.1), dict(lam=float("nan")), dict(lam=float("inf")),
               dict(dist_thresh=float("nan")), dict(iters=-1)):
        args = dict(width=160, height=120, max_frames=4)
        args.update(kw)
        refused(youth_rgbd.RgbdContext, **args)

    with youth_rgbd.RgbdContext(160, 120, 4) as ctx:
        before = _align_pairs(ctx, src, sg, dst, dg)
        d = [_dev(a) for a in (src, sg, dst, dg)]
        for k in range(4):
            a = list(d)
            a[k] = None
            refused(ctx.align_pairs_device, *a, 4)
        refused(ctx.align_pairs_device, *d, 0)
        refused(ctx.align_pairs_device, *d, 5)
        bad = np.tile(np.eye(4), (4, 1, 1))
        bad[2, 1, 3] = np.inf
        refused(ctx.align_pairs_device, *d, 4, T_init=bad)
        refused(ctx.align_sequence_device, None, d[1], 4)
        refused(ctx.align_sequence_device, d[0], None, 4)
        refused(ctx.align_sequence_device, d[0], d[1], 1)
        refused(ctx.align_sequence_device, d[0], d[1], 6)
        refused(ctx.prep_device, None, 1, 1, None, None)
        refused(ctx.prep_device, d[1], 2, 1, None, None)
        refused(ctx.poses, 5)
        refused(ctx.stats, 4, 3)
        rgb = _dev(np.zeros((1, 120, 160, 3), np.uint8))
        for a in ((0, None, d[1].data_ptr(), 1, 160, 120, None),
                  (0, rgb.data_ptr(), None, 1, 160, 120, None),
                  (0, rgb.data_ptr(), d[1].data_ptr(), -1, 160, 120, None),
                  (0, rgb.data_ptr(), d[1].data_ptr(), 1, 2, 120, None),
                  (99, rgb.data_ptr(), d[1].data_ptr(), 1, 160, 120, None)):
            assert lib.youth_rgbd_luma_device(*a) == EINVAL
            assert lib.youth_rgbd_last_error()
        neq = np.zeros(31)
        T12 = np.eye(4, dtype=f32)[:3].copy()
        P16, P8 = ctypes.POINTER(ctypes.c_int16), ctypes.POINTER(ctypes.c_uint8)
        PF, PD = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
        full = [src[0].ctypes.data_as(P16), sg[0].ctypes.data_as(P8), dst[0].ctypes.data_as(P16),
                dg[0].ctypes.data_as(P8), T12.ctypes.data_as(PF), neq.ctypes.data_as(PD)]
        for k in range(6):
            a = list(full)
            a[k] = None
            assert lib.youth_rgbd_reduce_host(ctx._ctx, *a) == EINVAL
            assert lib.youth_rgbd_last_error()
        Tn = T12.copy()
        Tn[0, 0] = np.nan
        full[4] = Tn.ctypes.data_as(PF)
        assert lib.youth_rgbd_reduce_host(ctx._ctx, *full) == EINVAL
        Tr = np.zeros((4, 16))
        rgb_h = np.zeros((4, 120, 160, 3), np.uint8)
        for a in ((None, rgb_h.ctypes.data_as(P8), 4, Tr.ctypes.data_as(PD), None),
                  (src.ctypes.data_as(P16), None, 4, Tr.ctypes.data_as(PD), None),
                  (src.ctypes.data_as(P16), rgb_h.ctypes.data_as(P8), 4, None, None),
                  (src.ctypes.data_as(P16), rgb_h.ctypes.data_as(P8), 1, Tr.ctypes.data_as(PD), None),
                  (src.ctypes.data_as(P16), rgb_h.ctypes.data_as(P8), 6, Tr.ctypes.data_as(PD), None)):
            assert lib.youth_rgbd_track_host_sequence(ctx._ctx, *a) == EINVAL
            assert lib.youth_rgbd_last_error()
        after = _align_pairs(ctx, src, sg, dst, dg)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(before[0].view(np.uint64), after[0].view(np.uint64))
