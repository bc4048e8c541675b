"""The level schedule of the RGB-D alignment on the GPU (include/youth_rgbd.h,
DESIGN.md §16): k_rgbd_decimate bit for bit against numpy slicing; a scheduled
align bit for bit against the composition of existing aligns it is defined as;
against the numpy truth (tests/rgbd_levels_truth.py); what it gains on two C5
pairs; the loop closer and the drop-in with a schedule; the arguments."""
import numpy as np
import pytest
import torch

import loop_truth
import rgbd_levels_truth as lt
import rgbd_truth
import youth_icp
import youth_loop
import youth_rgbd
import youth_synth

pytestmark = pytest.mark.gpu


def _dev(a):
    """A device copy, complete before the library's own (non-blocking) stream reads it."""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------- decimation --
DEPTH_GUARD, GRAY_GUARD = 0x5A5B, 0xA5
GUARD = 64


def _planes(n, W, H, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(-32768, 32768, (n, H, W)).astype(np.int16)
    d[rng.random((n, H, W)) < 0.2] = 0
    d[:, ::3, ::5] = -1
    d[:, 0, 0], d[:, H - 1, W - 1], d[:, H // 2, W // 2] = -32768, 32767, -32768
    d[:, (H - 1) // 16 * 16, (W - 1) // 16 * 16] = 32767     # a pixel every stride keeps
    y = rng.integers(0, 256, (n, H, W)).astype(np.uint8)
    return d, y


def _gpu_decimate(d, y, s, offset=0):
    """The stage entry on device copies; offset 1 places all four planes one
    element off alignment (the element path).  Outputs pre-filled with a
    sentinel, with guard words after the end that must survive."""
    n, H, W = d.shape
    Hs, Ws = (H + s - 1) // s, (W + s - 1) // s
    td = torch.zeros(d.size + 16, dtype=torch.int16, device="cuda")
    ty = torch.zeros(y.size + 16, dtype=torch.uint8, device="cuda")
    td[offset:offset + d.size] = torch.from_numpy(d.ravel()).cuda()
    ty[offset:offset + y.size] = torch.from_numpy(y.ravel()).cuda()
    m = n * Hs * Ws
    od = torch.full((offset + m + GUARD,), DEPTH_GUARD, dtype=torch.int16, device="cuda")
    oy = torch.full((offset + m + GUARD,), GRAY_GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert td.data_ptr() % 16 == 0 and ty.data_ptr() % 16 == 0 and od.data_ptr() % 16 == 0
    youth_rgbd.decimate_device(td.data_ptr() + 2 * offset, ty.data_ptr() + offset, n, W, H, s,
                               od.data_ptr() + 2 * offset, oy.data_ptr() + offset)
    torch.cuda.synchronize()
    od, oy = od.cpu().numpy(), oy.cpu().numpy()
    assert (od[:offset] == DEPTH_GUARD).all() and (od[offset + m:] == DEPTH_GUARD).all()
    assert (oy[:offset] == GRAY_GUARD).all() and (oy[offset + m:] == GRAY_GUARD).all()
    return od[offset:offset + m].reshape(n, Hs, Ws), oy[offset:offset + m].reshape(n, Hs, Ws)


DECIMATE_CASES = [(160, 120, s) for s in (2, 4, 8)] + [(97, 53, s) for s in (2, 4, 8, 16)] + [(640, 480, 8)]


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("W,H,s", DECIMATE_CASES, ids=lambda v: str(v))
def test_decimation_is_numpy_slicing(W, H, s, n):
    d, y = _planes(n, W, H, 1000 * s + W)
    gd, gy = _gpu_decimate(d, y, s)
    assert gd.shape == lt.decimate(d, s).shape
    assert np.array_equal(gd, lt.decimate(d, s)) and np.array_equal(gy, lt.decimate(y, s))
    assert {0, -1, -32768, 32767} <= set(np.unique(gd).tolist())
    if (W, H, s) == (97, 53, 16):
        assert gd.shape == (n, 4, 7)


@pytest.mark.parametrize("W,H,s", [(160, 120, 2), (160, 120, 8), (97, 53, 4)], ids=lambda v: str(v))
def test_decimation_does_not_depend_on_the_load_width(W, H, s):
    d, y = _planes(3, W, H, 7 + s)
    gd, gy = _gpu_decimate(d, y, s, offset=1)
    assert np.array_equal(gd, lt.decimate(d, s)) and np.array_equal(gy, lt.decimate(y, s))


# ----------------------------------------------- bit-equality with what exists --
SCHEDULES = [[(2, 3), (1, 3)], [(4, 2), (2, 2), (1, 2)], [(8, 4)], [(4, 3), (2, 0), (1, 3)]]


def _level_K(K, s):
    return youth_icp.Intrinsics(K.fx / s, K.fy / s, K.cx / s, K.cy / s, K.depth_scale)


def _small_poses(n, seed):
    rng = np.random.default_rng(seed)
    return np.array([loop_truth.se3_exp(rng.normal(0, 0.004, 6)) for _ in range(n)])


def _composed(ctxs, levels, planes, n, T_init):
    """The schedule as a composition of existing calls: frames decimated in
    numpy, one existing align per level on a context of the level's size and
    camera, each level's fp64 pose the next one's T_init."""
    out, T = [], T_init
    for (s, iters), ctx in zip(levels, ctxs):
        d = [_dev(lt.decimate(a[:n], s)) for a in planes]
        ctx.align_pairs_device(*d, n, T_init=T)
        T64, T32, st = ctx.poses(n)
        out.append((T64, T32, st, ctx.stats(n, iters) if iters else None))
        T = T64
    return out


def _check_levels(ctx, levels, want, n):
    """The scheduled call's results on ctx against the composition `want`."""
    T64, T32, st = ctx.poses(n)
    st_or = np.zeros(n, np.int32)
    for l, (s, iters) in enumerate(levels):
        w64, w32, wst, wstats = want[l]
        g64, gst = ctx.level_poses(l, n)
        assert np.array_equal(_bits(g64), _bits(w64)), (l, s)
        assert np.array_equal(gst, wst)
        if iters:
            assert np.array_equal(_bits(ctx.level_stats(l, n, iters)), _bits(wstats)), (l, s)
            assert s > 4 or wstats[:, :, 1].min() > 0
        st_or |= wst
    assert np.array_equal(_bits(T64), _bits(want[-1][0]))
    assert np.array_equal(T32.view(np.uint32), want[-1][1].view(np.uint32))
    assert np.array_equal(st, st_or)
    if levels[-1][1]:
        assert np.array_equal(_bits(ctx.stats(n, levels[-1][1])), _bits(want[-1][3]))


@pytest.mark.parametrize("levels", SCHEDULES, ids=lambda lv: "_".join(f"{s}x{i}" for s, i in lv))
@pytest.mark.parametrize("W,H", [(160, 120), (97, 53)], ids=lambda v: str(v))
def test_a_schedule_is_the_composition_of_existing_aligns(W, H, levels):
    src, dst, _, srgb, drgb = youth_synth.pairs_rgb(30, 6, W, H)
    planes = [src, rgbd_truth.luma(srgb), dst, rgbd_truth.luma(drgb)]
    fr, _, rgb = youth_synth.sequence_rgb(0, 7, W, H)
    g = rgbd_truth.luma(rgb)
    K = youth_icp.default_intrinsics(W, H)
    ctxs = [youth_rgbd.RgbdContext((W + s - 1) // s, (H + s - 1) // s, 6, K=_level_K(K, s), iters=it)
            for s, it in levels]
    try:
        with youth_rgbd.RgbdContext(W, H, 6) as ctx:
            ctx.set_levels(levels)
            assert ctx.levels() == levels
            d = [_dev(a) for a in planes]
            for n in (1, 6):
                for T_init in (None, _small_poses(n, n)):
                    want = _composed(ctxs, levels, planes, n, T_init)
                    ctx.align_pairs_device(*d, n, T_init=T_init)
                    _check_levels(ctx, levels, want, n)
            # the sequence entry: bit-equal to the pairwise one on the same frames
            seq_planes = [fr[1:], g[1:], fr[:-1], g[:-1]]
            want = _composed(ctxs, levels, seq_planes, 6, None)
            ctx.align_pairs_device(*[_dev(a) for a in seq_planes], 6)
            _check_levels(ctx, levels, want, 6)
            d_T = torch.zeros((6, 16), dtype=torch.float32, device="cuda")
            d_depth, d_gray = _dev(fr), _dev(g)
            ctx.align_sequence_device(d_depth, d_gray, 7, d_T_out=d_T)
            _check_levels(ctx, levels, want, 6)
            assert np.array_equal(d_T.cpu().numpy().reshape(6, 4, 4).view(np.uint32),
                                  want[-1][1].view(np.uint32))
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("W,H", [(160, 120), (97, 53)], ids=lambda v: str(v))
def test_one_full_resolution_level_is_the_context_without_a_schedule(W, H):
    src, dst, _, srgb, drgb = youth_synth.pairs_rgb(40, 3, W, H)
    d = [_dev(a) for a in (src, rgbd_truth.luma(srgb), dst, rgbd_truth.luma(drgb))]
    with youth_rgbd.RgbdContext(W, H, 3, iters=4) as ctx:
        assert ctx.levels() == []
        ctx.align_pairs_device(*d, 3)
        T64, T32, st = ctx.poses(3)
        stats = ctx.stats(3, 4)
        ctx.set_levels([(1, 4)])
        ctx.align_pairs_device(*d, 3)
        U64, U32, ust = ctx.poses(3)
        assert np.array_equal(_bits(U64), _bits(T64)) and np.array_equal(U32.view(np.uint32), T32.view(np.uint32))
        assert np.array_equal(ust, st) and np.array_equal(_bits(ctx.stats(3, 4)), _bits(stats))
        ctx.set_levels([(1, 7)])          # params.iters is not used
        ctx.align_pairs_device(*d, 3)
        assert ctx.stats(3, 7).shape == (3, 7, 4) and ctx.stats(3, 7)[:, 6, 1].min() > 0
        ctx.set_levels(None)
        ctx.align_pairs_device(*d, 3)
        assert ctx.levels() == [] and np.array_equal(_bits(ctx.poses(3)[0]), _bits(T64))
        assert np.array_equal(_bits(ctx.stats(3, 4)), _bits(stats))


# ------------------------------------------------ the truth and the value --
@pytest.fixture(scope="module")
def c5_pairs():
    """The two C5 pairs of rgbd_levels_truth at 160x120 under K160: frames,
    ground truth, the truth's scheduled align, and the GPU's aligns with and
    without the schedule."""
    K = youth_icp.Intrinsics(*lt.K160)
    out = []
    with youth_rgbd.RgbdContext(160, 120, 2, K=K) as ctx:
        for tgt, src in (lt.PAIR_REVISIT, lt.PAIR_NEAR):
            (dt,), (Xt,), (ct,) = youth_synth.sequence_rgb(tgt, 1, 160, 120, K=K)
            (ds,), (Xs,), (cs,) = youth_synth.sequence_rgb(src, 1, 160, 120, K=K)
            gt, gs = rgbd_truth.luma(ct), rgbd_truth.luma(cs)
            d = [_dev(a[None]) for a in (ds, gs, dt, gt)]
            ctx.set_levels(None)
            ctx.align_pairs_device(*d, 1)
            flat = ctx.poses(1)[0][0]
            ctx.set_levels(lt.SCHEDULE_160)
            ctx.align_pairs_device(*d, 1)
            T64, _, st = ctx.poses(1)
            per = [(ctx.level_poses(l, 1), ctx.level_stats(l, 1, it)) for l, (_, it) in enumerate(lt.SCHEDULE_160)]
            out.append(dict(planes=(ds, gs, dt, gt), T_gt=np.linalg.inv(Xt) @ Xs, K=K, flat=flat,
                            T64=T64[0], st=int(st[0]), per=per,
                            truth=lt.align_levels(ds, gs, dt, gt, lt.SCHEDULE_160, K=K)))
    return out


def _against_truth(per_gpu, st_gpu, truth, levels, p=0):
    """The project's bars: poses within 1e-5, status and both counts equal at
    every iteration of every level."""
    T64, _, st, per = truth
    worst = 0.0
    for l, (s, iters) in enumerate(levels):
        (g64, gst), gstats = per_gpu[l]
        t64, _, tst, tstats = per[l]
        worst = max(worst, float(np.abs(g64[p][:3] - t64[:3]).max()))
        assert gst[p] == tst, (l, s)
        assert np.array_equal(gstats[p][:, [1, 3]], tstats[:, [1, 3]]), (l, s)
    assert st_gpu == st
    return worst


def test_levels_against_the_numpy_truth(c5_pairs):
    for c in c5_pairs:
        worst = _against_truth(c["per"], c["st"], c["truth"], lt.SCHEDULE_160)
        print(f"C5 pair: max |T - truth| over the levels {worst:.3e}")
        assert worst <= 1e-5
    # two draws of the pair generator, three levels
    levels = [(4, 3), (2, 3), (1, 4)]
    src, dst, _, srgb, drgb = youth_synth.pairs_rgb(50, 2, 160, 120)
    sg, dg = rgbd_truth.luma(srgb), rgbd_truth.luma(drgb)
    with youth_rgbd.RgbdContext(160, 120, 2) as ctx:
        ctx.set_levels(levels)
        ctx.align_pairs_device(*[_dev(a) for a in (src, sg, dst, dg)], 2)
        _, _, st = ctx.poses(2)
        per = [(ctx.level_poses(l, 2), ctx.level_stats(l, 2, it)) for l, (_, it) in enumerate(levels)]
    for p in range(2):
        truth = lt.align_levels(src[p], sg[p], dst[p], dg[p], levels)
        worst = _against_truth(per, int(st[p]), truth, levels, p)
        print(f"draw {50 + p}: max |T - truth| over the levels {worst:.3e}")
        assert worst <= 1e-5


def test_the_schedule_reaches_what_the_identity_start_misses(c5_pairs):
    for c, bound in zip(c5_pairs, (lt.BOUND_REVISIT, lt.BOUND_NEAR)):
        flat = rgbd_truth.pose_error(c["flat"], c["T_gt"])
        lev = rgbd_truth.pose_error(c["T64"], c["T_gt"])
        print(f"identity {flat[0]:.4f} deg / {flat[1]:.3f} mm, 2:10 -> 1:10 {lev[0]:.4f} deg / {lev[1]:.3f} mm")
        assert c["st"] == 0
        assert lev[0] <= bound[0] and lev[1] <= bound[1]
        assert flat[0] > lt.IDENTITY_FLOOR[0] and flat[1] > lt.IDENTITY_FLOOR[1]


# ------------------------------------------------------------ the loop closer --
def test_the_closer_verifies_a_revisit_it_missed(c5_pairs):
    c = c5_pairs[0]
    K = c["K"]
    with youth_loop.LoopCloser(160, 120, 4, K=K, min_gap=1, max_cell_dist=500) as lc:
        for k, f in enumerate(lt.PAIR_REVISIT):
            a, T, rgb = youth_synth.sequence_rgb(f, 1, 160, 120, K=K)
            assert lc.add_keyframe(a[0], rgb[0], T[0], tag=f) == k
        assert lc.levels() == []
        assert lc.close(1) == 0
        v = lc.last_verified()
        assert v.shape[0] == 1 and v[0]["w"] == 0.0 and (int(v[0]["i"]), int(v[0]["j"])) == (0, 1)
        print(f"no schedule: overlap {v[0]['overlap']:.3f} grey rms {v[0]['gray_rms']:.2f} fb "
              f"{v[0]['fb_rot_deg']:.4f} deg / {v[0]['fb_trans_m'] * 1e3:.3f} mm")
        assert v[0]["gray_rms"] > 5.0 and v[0]["fb_rot_deg"] > 1.0
        lc.set_levels(lt.SCHEDULE_160)
        assert lc.levels() == lt.SCHEDULE_160
        assert lc.close(1) == 1
        e = lc.edges()
    assert [(int(x["i"]), int(x["j"])) for x in e] == [(0, 1)]
    e = e[0]
    print(f"2:10 -> 1:10: overlap {e['overlap']:.3f} grey rms {e['gray_rms']:.2f} fb "
          f"{e['fb_rot_deg']:.4f} deg / {e['fb_trans_m'] * 1e3:.3f} mm")
    P = youth_loop.default_params()
    assert e["w"] == 1.0 and e["overlap"] >= P.min_overlap and e["gray_rms"] <= P.max_gray_rms
    assert e["fb_rot_deg"] <= P.fb_rot_deg and e["fb_trans_m"] <= P.fb_trans_m
    assert 0.6 <= e["overlap"] <= 0.7 and e["gray_rms"] <= 1.1
    assert np.abs(e["Z"][:3] - c["truth"][0][:3]).max() <= 1e-5
    deg, mm = rgbd_truth.pose_error(e["Z"], c["T_gt"])
    assert deg <= lt.BOUND_REVISIT[0] and mm <= lt.BOUND_REVISIT[1]


# ------------------------------------------------------------------ arguments --
def _refused(fn, *a, **kw):
    with pytest.raises(youth_icp.IcpError) as ei:
        fn(*a, **kw)
    assert ei.value.code == youth_icp.YOUTH_EINVAL
    assert len(str(ei.value)) > len("youth_icp error -1: ")


def test_bad_schedules_are_refused_and_leave_the_context_intact():
    src, dst, _, srgb, drgb = youth_synth.pairs_rgb(60, 2, 160, 120)
    d = [_dev(a) for a in (src, rgbd_truth.luma(srgb), dst, rgbd_truth.luma(drgb))]
    lib = youth_rgbd.load_library()
    keep = [(2, 2), (1, 2)]

    def run(ctx):
        ctx.align_pairs_device(*d, 2)
        return ctx.poses(2), ctx.stats(2, 2)

    with youth_rgbd.RgbdContext(160, 120, 2, iters=2) as ctx:
        for levels in (None, keep):
            ctx.set_levels(levels)
            before = run(ctx)
            for bad in ([(0, 3)], [(3, 3)], [(32, 3)], [(2, 3), (2, 3)], [(2, 3), (4, 3)],
                        [(16, 1), (8, 1), (4, 1), (2, 1), (1, 1)], [(2, -1), (1, 3)], [(1, -1)],
                        [(64, 3)]):
                _refused(ctx.set_levels, bad)
            assert lib.youth_rgbd_set_levels(ctx._ctx, None, 2) == youth_icp.YOUTH_EINVAL
            assert lib.youth_rgbd_last_error()
            _refused(ctx.level_poses, len(levels or ()), 1)
            _refused(ctx.level_stats, -1, 1, 2)
            assert ctx.levels() == (levels or [])
            after = run(ctx)
            assert np.array_equal(_bits(before[0][0]), _bits(after[0][0]))
            assert np.array_equal(before[0][2], after[0][2])
            assert np.array_equal(_bits(before[1]), _bits(after[1]))
        # the streaming tracker does not run schedules, and a schedule does not
        # arrive while frames are pending
        depth = [np.ascontiguousarray(src[0])]
        rgb = [np.ascontiguousarray(srgb[0])]
        _refused(ctx.track_submit, depth, rgb)
        assert ctx.track_pending() == 0
        ctx.set_levels(None)
        ctx.track_submit(depth, rgb)
        assert ctx.track_pending() == 1
        _refused(ctx.set_levels, keep)
        ctx.track_collect()
        ctx.set_levels(keep)
        after = run(ctx)
        assert np.array_equal(_bits(before[0][0]), _bits(after[0][0]))
    # a level below 3 pixels
    with youth_rgbd.RgbdContext(17, 9, 2) as small:
        _refused(small.set_levels, [(8, 3), (1, 3)])
        small.set_levels([(2, 3), (1, 3)])
    # decimation's own arguments
    t = torch.zeros(64 * 64, dtype=torch.int16, device="cuda")
    g = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    for a in ((0, g.data_ptr(), 1, 64, 64, 2, t.data_ptr(), g.data_ptr()),
              (t.data_ptr(), g.data_ptr(), 1, 64, 64, 2, t.data_ptr(), 0),
              (t.data_ptr(), g.data_ptr(), 1, 64, 64, 1, t.data_ptr(), g.data_ptr()),
              (t.data_ptr(), g.data_ptr(), 1, 64, 64, 3, t.data_ptr(), g.data_ptr()),
              (t.data_ptr(), g.data_ptr(), -1, 64, 64, 2, t.data_ptr(), g.data_ptr()),
              (t.data_ptr(), g.data_ptr(), 1, 2, 64, 2, t.data_ptr(), g.data_ptr())):
        _refused(youth_rgbd.decimate_device, *a)
    # the closer's schedule ends at full resolution
    with youth_loop.LoopCloser(160, 120, 4) as lc:
        _refused(lc.set_levels, [(8, 10)])
        _refused(lc.set_levels, [(2, 10), (1, 0)])
        _refused(lc.set_levels, [(2, 10), (3, 10), (1, 10)])
        assert lc.levels() == []
        lc.set_levels([(4, 5), (1, 5)])
        _refused(lc.set_levels, [(4, 5), (2, 5)])
        assert lc.levels() == [(4, 5), (1, 5)]


# ----------------------------------------------------------------- the drop-in --
def test_the_drop_in_reads_its_schedule_from_the_environment(tmp_path):
    import test_gpu_slam_loop as sl

    env = {"YOUTH_SLAM_RGBD": "1", "YOUTH_SLAM_LOOP": "1", "YOUTH_SLAM_LOOP_KF_M": "0.045",
           "YOUTH_SLAM_LOOP_KF_DEG": "90", "YOUTH_SLAM_LOOP_MIN_GAP": "2"}
    unset = sl._run_child(tmp_path, "unset", env)
    one = sl._run_child(tmp_path, "one", dict(env, YOUTH_SLAM_LOOP_LEVELS="1:10"))
    bad = sl._run_child(tmp_path, "bad", dict(env, YOUTH_SLAM_LOOP_LEVELS="8:10;1:10"))
    names = sorted(p.name for p in unset[0].iterdir() if p.name.startswith("map"))
    assert "map_keyframes.txt" in names and "map_trajectory_closed.txt" in names
    assert unset[2]["edges"].shape[0] >= 1
    for other in (one, bad):
        assert sorted(p.name for p in other[0].iterdir() if p.name.startswith("map")) == names
        for name in names:
            assert (other[0] / name).read_bytes() == (unset[0] / name).read_bytes(), name
        assert np.array_equal(other[2]["edges"], unset[2]["edges"])
    assert "YOUTH_SLAM_LOOP_LEVELS" not in unset[3] and "YOUTH_SLAM_LOOP_LEVELS" not in one[3]
    assert bad[3].count("YOUTH_SLAM_LOOP_LEVELS=8:10;1:10") == 1 and "ignored" in bad[3]
