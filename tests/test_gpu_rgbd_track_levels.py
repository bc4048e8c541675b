"""The streaming RGB-D tracker's level schedule on the GPU (include/youth_rgbd.h
youth_rgbd_track_set_levels): the scheduled tracker's
independence of how a sequence is split, and its bit-equality, level by level,
with the scheduled sequence align (so with the decimated frames its ingest
makes: k_rgbd_pull, then one k_rgbd_decimate); one full-resolution level; the depth filter in front of the
levels; what it is worth on pairs ten frames apart; its protocol; the drop-in's
YOUTH_SLAM_RGBD_LEVELS."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rgbd_levels_truth as lt
import rgbd_track_levels_truth as tt
import rgbd_truth
import test_gpu_slam_rgbd as sr
import youth_filter
import youth_icp
import youth_rgbd
import youth_synth
from conftest import ORACLE, PKG

pytestmark = pytest.mark.gpu

E = youth_icp.YOUTH_EINVAL


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------- tracker helpers --
def _track(ctx, depth, rgb, split):
    """trk._track that also gathers track_last_levels of every frame."""
    T, has, st, lv = [], [], [], []
    sizes = []

    def collect():
        for _ in range(sizes.pop(0)):
            t, h, s = ctx.track_collect()
            T.append(t)
            has.append(h)
            st.append(s)
            lv.append(ctx.track_last_levels())

    f = 0
    for m in split:
        if len(sizes) == 2:
            collect()
        ctx.track_submit(depth[f:f + m], rgb[f:f + m])
        sizes.append(m)
        f += m
    while sizes:
        collect()
    assert f == len(depth) and ctx.track_pending() == 0
    return np.array(T), np.array(has), np.array(st), lv


def _same(a, b):
    """Two _track results, bit for bit."""
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2], b[2]) and len(a[3]) == len(b[3])
    for (Ta, sa), (Tb, sb) in zip(a[3], b[3]):
        assert np.array_equal(_bits(Ta), _bits(Tb)) and np.array_equal(sa, sb)


@pytest.fixture(scope="module")
def seq160():
    depth, _, rgb = youth_synth.sequence_rgb(0, 9, 160, 120)
    return list(depth), list(rgb), depth, rgb


@pytest.fixture(scope="module")
def seq97():
    depth, _, rgb = youth_synth.sequence_rgb(0, 9, 97, 53)
    return list(depth), list(rgb), depth, rgb


# Submissions of at most b frames: at b = 8 §14's splits; at b = 3 an 8-frame
# submission is refused, so [1, 8] and [8, 1] become the splits nearest to them
# that fit.
SPLIT_CASES = {
    "160x120_b8": (160, 120, 8, [(2, 3), (1, 3)], ([1] * 9, [1, 8], [3, 3, 3], [8, 1])),
    "97x53_b3": (97, 53, 3, [(4, 2), (2, 0), (1, 2)], ([1] * 9, [1, 3, 3, 2], [3, 3, 3], [3, 3, 2, 1])),
}


def _splits_agree(case, seq):
    W, H, b, levels, splits = SPLIT_CASES[case]
    dl, cl, depth, rgb = seq
    runs = []
    for split in splits:
        with youth_rgbd.RgbdContext(W, H, 16) as ctx:
            assert ctx.track_set_batch(b) == 1
            ctx.track_set_levels(levels)
            assert ctx.track_levels() == levels and ctx.levels() == []
            runs.append(_track(ctx, dl, cl, split))
    first = runs[0]
    assert first[1].tolist() == [0] + [1] * 8 and np.array_equal(first[0][0], np.eye(4))
    assert first[3][0][0].shape == (0, 4, 4)           # no reference: no levels to report
    for k in range(1, 9):
        Tl, sl = first[3][k]
        assert Tl.shape == (len(levels), 4, 4) and np.array_equal(_bits(Tl[-1]), _bits(first[0][k]))
        assert int(np.bitwise_or.reduce(sl)) == first[2][k]
    for other in runs[1:]:
        _same(first, other)
    with youth_rgbd.RgbdContext(W, H, 16) as ctx:
        ctx.set_levels(levels)
        Tseq, stseq = ctx.track_host_sequence(depth, rgb)
        per = [ctx.level_poses(l, 8) for l in range(len(levels))]
    Tseq[:, 3, :] = (0.0, 0.0, 0.0, 1.0)
    return first, Tseq, stseq, per


@pytest.mark.parametrize("case", sorted(SPLIT_CASES))
def test_splits_are_bit_identical_and_equal_the_scheduled_sequence(case, seq160, seq97, monkeypatch):
    monkeypatch.setenv("YOUTH_RGBD_CHUNKS", "7")
    (T, _, st, lv), Tseq, stseq, per = _splits_agree(case, seq160 if case.startswith("160") else seq97)
    assert np.array_equal(_bits(T[1:]), _bits(Tseq)) and np.array_equal(st[1:], stseq)
    for l, (T64, s) in enumerate(per):
        for k in range(8):
            assert np.array_equal(_bits(lv[k + 1][0][l]), _bits(T64[k])), (l, k)
            assert lv[k + 1][1][l] == s[k], (l, k)
    assert (st == 0).all()


@pytest.mark.parametrize("case", sorted(SPLIT_CASES))
def test_splits_without_the_knob_within_launch_shape_bar(case, seq160, seq97, monkeypatch):
    monkeypatch.delenv("YOUTH_RGBD_CHUNKS", raising=False)
    (T, _, st, lv), Tseq, stseq, per = _splits_agree(case, seq160 if case.startswith("160") else seq97)
    worst = np.abs(T[1:] - Tseq).max()
    for l, (T64, s) in enumerate(per):
        worst = max(worst, max(np.abs(lv[k + 1][0][l] - T64[k]).max() for k in range(8)))
        assert [int(lv[k + 1][1][l]) for k in range(8)] == s.tolist()
    print("max |T - T_seq| over poses and levels:", worst)
    assert worst <= 1e-9 and np.array_equal(st[1:], stseq)


# ------------------------------------------------------------- one level --
def test_one_full_resolution_level_is_the_tracker_without_a_schedule(seq160):
    dl, cl, _, _ = seq160
    with youth_rgbd.RgbdContext(160, 120, 16) as ctx:
        ctx.track_set_batch(4)
        flat = _track(ctx, dl[:6], cl[:6], [2, 4])
        assert all(l[0].shape[0] == 0 for l in flat[3])
        ctx.track_set_levels([(1, 10)])
        one = _track(ctx, dl[:6], cl[:6], [2, 4])
        assert one[1].tolist() == [0, 1, 1, 1, 1, 1]       # set_levels started a new sequence
        for a, b in zip(flat[:3], one[:3]):
            assert np.array_equal(a, b)
        assert all(l[0].shape[0] == 1 for l in one[3][1:])
        ctx.track_set_levels([(1, 4)])                      # params.iters is not used
        four = _track(ctx, dl[:6], cl[:6], [2, 4])
        ctx.track_set_levels(None)
        assert ctx.track_levels() == []
        again = _track(ctx, dl[:6], cl[:6], [2, 4])
        for a, b in zip(flat[:3], again[:3]):
            assert np.array_equal(a, b)
    with youth_rgbd.RgbdContext(160, 120, 16, iters=4) as ctx:
        ctx.track_set_batch(4)
        want = _track(ctx, dl[:6], cl[:6], [2, 4])
    for a, b in zip(four[:3], want[:3]):
        assert np.array_equal(a, b)
    assert not np.array_equal(four[0], flat[0])


# ---------------------------------------------------------- depth filter --
def test_depth_filter_in_front_of_the_levels_equals_prefiltered_frames(seq160):
    dl, cl, depth, _ = seq160
    filtered = list(youth_filter.depth_filter_host(depth[:6], 8, 96))
    # the filter changes pixels the coarse level keeps, so a level decimated
    # from the raw frame would show
    assert any(not np.array_equal(a[::2, ::2], b[::2, ::2]) for a, b in zip(filtered, dl))
    with youth_rgbd.RgbdContext(160, 120, 16) as ctx:
        ctx.track_set_batch(4)
        ctx.track_set_levels([(2, 3), (1, 3)])
        ctx.track_set_depth_filter(8, 96)
        on = _track(ctx, dl[:6], cl[:6], [2, 4])
        ctx.track_reset()
        ctx.track_set_depth_filter(None)
        off = _track(ctx, filtered, cl[:6], [2, 4])
        ctx.track_reset()
        raw = _track(ctx, dl[:6], cl[:6], [2, 4])
    _same(on, off)
    assert not np.array_equal(on[0], raw[0])


# ----------------------------------------------------------------- value --
def test_the_schedule_keeps_a_track_of_distant_pairs():
    depth, rgb, _ = tt.frames()
    K = youth_icp.Intrinsics(*lt.K160)
    ends = {}
    for name, levels in (("schedule", tt.SCHEDULE), ("flat", None)):
        want_T, want_st, want_per = tt.track(levels or tt.FLAT)
        with youth_rgbd.RgbdContext(160, 120, 8, K=K) as ctx:
            ctx.track_set_batch(4)
            ctx.track_set_levels(levels)
            T, has, st, lv = _track(ctx, list(depth), list(rgb), [4, 4, 3])
        assert has.tolist() == [0] + [1] * 10
        worst = np.abs(T[1:, :3] - want_T[:, :3]).max()
        if levels:
            for k in range(10):
                for l in range(len(levels)):
                    worst = max(worst, np.abs(lv[k + 1][0][l][:3] - want_per[k][l][0][:3]).max())
                    assert lv[k + 1][1][l] == want_per[k][l][1]
        print(f"{name}: max |T - truth| {worst:.3e}")
        assert worst <= 1e-5 and np.array_equal(st[1:], want_st)
        ends[name] = tt.end_error(T[1:])
    lev, flat = ends["schedule"], ends["flat"]
    print(f"no schedule {flat[0]:.3f} deg / {flat[1]:.2f} mm, 2:10 -> 1:10 {lev[0]:.3f} deg / {lev[1]:.2f} mm")
    assert lev[0] <= tt.BOUND_SCHEDULE[0] and lev[1] <= tt.BOUND_SCHEDULE[1]
    assert flat[0] > tt.FLOOR_FLAT[0] and flat[1] > tt.FLOOR_FLAT[1]


# -------------------------------------------------------------- protocol --
def _refused(fn, *a, **kw):
    with pytest.raises(youth_icp.IcpError) as ei:
        fn(*a, **kw)
    assert ei.value.code == E
    assert len(str(ei.value)) > len("youth_icp error -1: ")
    return str(ei.value)


BAD_SCHEDULES = ([(0, 3)], [(3, 3)], [(32, 3)], [(2, 3), (2, 3)], [(2, 3), (4, 3)],
                 [(16, 1), (8, 1), (4, 1), (2, 1), (1, 1)], [(2, -1), (1, 3)], [(1, -1)], [(64, 3)])


def test_protocol_and_refusals(seq160):
    dl, cl, depth, rgb = seq160
    keep = [(2, 2), (1, 2)]
    with youth_rgbd.RgbdContext(160, 120, 8, iters=2) as ctx:
        lib, h = ctx._lib, ctx._ctx
        ctx.track_set_batch(4)
        ctx.track_set_levels(keep)
        want = _track(ctx, dl[:6], cl[:6], [2, 4])
        ctx.track_reset()
        # a last stride other than 1, and everything set_levels refuses
        for bad in ([(8, 10)], [(4, 3), (2, 3)]) + BAD_SCHEDULES:
            assert "youth_rgbd_track_set_levels" in _refused(ctx.track_set_levels, bad)
        assert lib.youth_rgbd_track_set_levels(h, None, 2) == E
        assert ctx.track_levels() == keep
        _same(_track(ctx, dl[:6], cl[:6], [2, 4]), want)
        # not while frames are pending
        ctx.track_reset()
        ctx.track_submit(dl[:2], cl[:2])
        assert "pending" in _refused(ctx.track_set_levels, None)
        assert "pending" in _refused(ctx.track_set_levels, [(1, 3)])
        got = [ctx.track_collect() for _ in range(2)]
        assert np.array_equal(got[1][0], want[0][1]) and ctx.track_levels() == keep
        # the align schedule still bars the tracker, and the text names the new call
        ctx.set_levels([(2, 2)])
        assert "youth_rgbd_track_set_levels" in _refused(ctx.track_submit, dl[:1], cl[:1])
        assert ctx.track_pending() == 0
        ctx.set_levels(None)
        # every entry point that shares the workspace starts a new sequence
        d_depth, d_gray = torch.from_numpy(depth[:3]).cuda(), torch.from_numpy(rgbd_truth.luma(rgb[:3])).cuda()
        torch.cuda.synchronize()
        sharers = (lambda: ctx.align_sequence_device(d_depth, d_gray, 3),
                   lambda: ctx.align_pairs_device(d_depth[1:], d_gray[1:], d_depth[:2], d_gray[:2], 2),
                   lambda: ctx.track_host_sequence(depth[:3], rgb[:3]),
                   lambda: ctx.reduce_host(depth[1], rgbd_truth.luma(rgb[1]), depth[0],
                                           rgbd_truth.luma(rgb[0]), np.eye(4)[:3]),
                   lambda: ctx.track_set_levels(keep))
        for share in sharers:
            ctx.track_submit(dl[:1], cl[:1])
            ctx.track_collect()
            share()
            ctx.sync()
            ctx.track_submit(dl[:2], cl[:2])
            first, second = ctx.track_collect(), ctx.track_collect()
            assert first[1] == 0 and np.array_equal(first[0], np.eye(4))
            assert ctx.track_last_levels()[0].shape[0] == 2
            assert second[1] == 1 and np.array_equal(second[0], want[0][1]) and second[2] == want[2][1]
        # track_set_batch keeps the schedule; every level follows the new b
        ctx.track_reset()
        assert ctx.track_set_batch(2) == 4 and ctx.track_levels() == keep
        two = _track(ctx, dl[:6], cl[:6], [2, 2, 1, 1])
        assert two[1].tolist() == [0, 1, 1, 1, 1, 1] and (two[2] == 0).all()
        print("b = 2 against b = 4:", np.abs(two[0] - want[0]).max())
        assert np.abs(two[0] - want[0]).max() <= 1e-9
    with youth_rgbd.RgbdContext(160, 120, 8, iters=2) as ctx:     # b = 2 from the start: the same bits
        ctx.track_set_batch(2)
        ctx.track_set_levels(keep)
        _same(_track(ctx, dl[:6], cl[:6], [2, 2, 1, 1]), two)
    # a level below 3 pixels
    d17, _, c17 = youth_synth.sequence_rgb(0, 3, 17, 9)
    with youth_rgbd.RgbdContext(17, 9, 2) as small:
        _refused(small.track_set_levels, [(8, 3), (1, 3)])
        small.track_set_levels([(2, 3), (1, 3)])
        T, has, st, lv = _track(small, list(d17), list(c17), [1, 1, 1])
        assert has.tolist() == [0, 1, 1] and lv[2][0].shape[0] == 2


# ------------------------------------------------------------ the drop-in --
def _run_child(tmp_path, name, env_extra, **plan):
    """test_gpu_slam_rgbd's child, 8 frames of 160x120; also returns its stderr."""
    out = tmp_path / name
    out.mkdir()
    plan = dict({"W": 160, "H": 120, "n": 8, "color": True, "backlog": True}, **plan)
    env = {k: v for k, v in os.environ.items()
           if not k.startswith(("YOUTH_SLAM_", "YOUTH_ICP_DEPTH_FILTER", "YOUTH_RGBD_"))}
    env.update(env_extra, PYTHONPATH=os.pathsep.join([PKG, ORACLE] + [p for p in sys.path if p]))
    r = subprocess.run([sys.executable, "-c", sr._CHILD, str(out), json.dumps(plan)], env=env,
                       timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return out, json.loads(line[len("RESULT "):]), np.load(out / "res.npz", allow_pickle=False), r.stderr


def _saved(out):
    return {p.name: p.read_bytes() for p in sorted(out.iterdir()) if p.name.startswith("map")}


def test_the_drop_in_tracks_with_its_schedule(tmp_path):
    fr, _, rgb = youth_synth.sequence_rgb(0, 8, 160, 120)
    with youth_rgbd.RgbdContext(160, 120, 8) as ctx:
        ctx.set_levels(tt.SCHEDULE)
        T_rel, st = ctx.track_host_sequence(fr, rgb)
        ctx.set_levels(None)
        flat, _ = ctx.track_host_sequence(fr, rgb)
    assert not st.any() and not np.array_equal(T_rel, flat)
    T_rel[:, 3, :] = (0.0, 0.0, 0.0, 1.0)
    want = [np.eye(4)]
    for k in range(7):
        want.append(want[-1] @ T_rel[k])
    env = {"YOUTH_SLAM_RGBD": "1", "YOUTH_SLAM_RGBD_LEVELS": "2:10,1:10"}
    _, info, res, err = _run_child(tmp_path, "backlog", env)
    assert info["active"] == 1 and res["ts"].tolist() == list(range(8))
    assert "YOUTH_SLAM_RGBD_LEVELS" not in err
    T = res["T"].reshape(-1, 4, 4)
    print("max |T - composed scheduled sequence align|:", np.abs(T - np.array(want)).max())
    assert np.abs(T - np.array(want)).max() <= 1e-9
    _, live, res1, _ = _run_child(tmp_path, "live", env, backlog=False)
    assert live["active"] == 1 and live["batched"] == 0
    assert np.array_equal(res1["T"], res["T"]) and np.array_equal(res1["ts"], res["ts"])


def test_the_drop_in_with_one_level_or_a_malformed_value_is_the_drop_in_without(tmp_path):
    env = {"YOUTH_SLAM_RGBD": "1", "YOUTH_SLAM_MAP_VPM": "100"}
    unset = _run_child(tmp_path, "unset", env)
    one = _run_child(tmp_path, "one", dict(env, YOUTH_SLAM_RGBD_LEVELS="1:10"))
    bad = _run_child(tmp_path, "bad", dict(env, YOUTH_SLAM_RGBD_LEVELS="2:10;1:10"))
    files = _saved(unset[0])
    assert len(files) >= 1 and unset[1]["active"] == 1
    for other in (one, bad):
        assert _saved(other[0]) == files
        assert np.array_equal(other[2]["T"], unset[2]["T"]) and np.array_equal(other[2]["vox"], unset[2]["vox"])
    assert "YOUTH_SLAM_RGBD_LEVELS" not in unset[3] and "YOUTH_SLAM_RGBD_LEVELS" not in one[3]
    lines = [ln for ln in bad[3].splitlines() if "YOUTH_SLAM_RGBD_LEVELS" in ln]
    assert len(lines) == 1 and "YOUTH_SLAM_RGBD_LEVELS=2:10;1:10" in lines[0] and "ignored" in lines[0]


def test_the_variable_alone_leaves_default_mode_alone(tmp_path):
    plain = _run_child(tmp_path, "plain", {})
    alone = _run_child(tmp_path, "alone", {"YOUTH_SLAM_RGBD_LEVELS": "2:10,1:10"})
    assert plain[1]["active"] == 0 and alone[1]["active"] == 0
    assert np.array_equal(alone[2]["T"], plain[2]["T"]) and np.array_equal(alone[2]["ts"], plain[2]["ts"])
    assert _saved(alone[0]) == _saved(plain[0])
    assert "YOUTH_SLAM_RGBD_LEVELS" not in alone[3]
