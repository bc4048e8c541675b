"""The level schedule of the RGB-D alignment, CPU side: what
the numpy truth (tests/rgbd_levels_truth.py) gains on two C5 pairs that the
align misses from the identity, the exact geometry of a decimated level, the
default schedules and the new symbols."""
import ctypes
import os

import numpy as np
import pytest

import oracle
import rgbd_levels_truth as lt
import rgbd_truth
import youth_icp
import youth_loop
import youth_rgbd
import youth_synth
from conftest import PKG, ROOT


def _frame(f, K):
    a, T, c = youth_synth.sequence_rgb(f, 1, 160, 120, K=K)
    return a[0], rgbd_truth.luma(c[0]), T[0]


@pytest.mark.parametrize("pair,bound", [(lt.PAIR_REVISIT, lt.BOUND_REVISIT),
                                        (lt.PAIR_NEAR, lt.BOUND_NEAR)], ids=["250_868", "150_155"])
def test_the_schedule_reaches_what_the_identity_start_misses(pair, bound):
    K = youth_icp.Intrinsics(*lt.K160)
    dt, gt, Xt = _frame(pair[0], K)
    ds, gs, Xs = _frame(pair[1], K)
    T_gt = np.linalg.inv(Xt) @ Xs
    flat = rgbd_truth.pose_error(rgbd_truth.align(ds, gs, dt, gt, K=K)[0], T_gt)
    T64, _, st, per = lt.align_levels(ds, gs, dt, gt, lt.SCHEDULE_160, K=K)
    lev = rgbd_truth.pose_error(T64, T_gt)
    print(f"target {pair[0]}, source {pair[1]}: identity {flat[0]:.4f} deg / {flat[1]:.3f} mm, "
          f"2:10 -> 1:10 {lev[0]:.4f} deg / {lev[1]:.3f} mm")
    assert st == 0 and len(per) == 2 and per[0][3].shape == (10, 4)
    assert lev[0] <= bound[0] and lev[1] <= bound[1]
    assert flat[0] > lt.IDENTITY_FLOOR[0] and flat[1] > lt.IDENTITY_FLOOR[1]


@pytest.mark.parametrize("K", [None, (142.575, 139.25, 47.3, 27.9, 1000.0)], ids=["viewer", "odd"])
def test_a_level_pixel_is_the_full_resolution_point_bit_for_bit(K):
    W, H = 97, 53
    rng = np.random.default_rng(16)
    d = rng.integers(-50, 9000, (H, W)).astype(np.int16)
    d[::7, ::5] = 0
    d[3, 8], d[8, 16], d[16, 32] = -32768, 32767, -1
    K = oracle.K_of(K) if K is not None else oracle.viewer_K(W, H)
    full = oracle.backproject(d, K)
    for s in (2, 4, 8):
        ds = lt.decimate(d, s)
        assert ds.shape == ((H + s - 1) // s, (W + s - 1) // s)
        lev = oracle.backproject(ds, lt.level_K(K, s))
        for a, b in zip(lev, full):
            assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(b[::s, ::s]).view(np.uint32)), s
        assert (lev[2] > 0).sum() > ds.size // 2


def test_default_levels():
    for (W, H), want in (((640, 480), [(8, 10), (1, 10)]), ((320, 240), [(4, 10), (1, 10)]),
                         ((160, 120), [(2, 10), (1, 10)]), ((100, 60), [(1, 10)])):
        assert youth_rgbd.default_levels(W, H) == want == lt.default_levels(W, H)
        lt.check_schedule(want, W, H)
    assert youth_rgbd.parse_levels("auto", 640, 480) == [(8, 10), (1, 10)]
    assert youth_rgbd.parse_levels("8:10,4:0,1:5", 640, 480) == [(8, 10), (4, 0), (1, 5)]
    assert youth_rgbd.parse_levels("", 640, 480) == []


def test_new_symbols_are_declared_exported_and_bound():
    new_rgbd = ["youth_rgbd_default_levels", "youth_rgbd_set_levels", "youth_rgbd_get_levels",
                "youth_rgbd_get_level_poses", "youth_rgbd_get_level_stats",
                "youth_rgbd_decimate_device"]
    new_loop = ["youth_loop_set_levels", "youth_loop_get_levels"]
    lib = ctypes.CDLL(os.path.join(PKG, "libyouth_icp.so"))
    for header, names, mod in (("youth_rgbd.h", new_rgbd, youth_rgbd), ("youth_loop.h", new_loop, youth_loop)):
        declared = youth_icp.declared_functions(os.path.join(ROOT, "include", header))
        for n in names:
            assert n in declared and hasattr(lib, n) and n in mod._SIGS, n
        assert set(declared) <= set(mod._SIGS)
    assert ctypes.sizeof(youth_rgbd.RgbdLevel) == 8 and youth_rgbd.MAX_LEVELS == 4
    assert ctypes.sizeof(youth_loop.LoopParams) == 36 and ctypes.sizeof(youth_rgbd.RgbdParams) == 12
    text = open(os.path.join(ROOT, "include", "youth_rgbd.h")).read()
    assert "#define YOUTH_RGBD_MAX_LEVELS 4" in text


def test_null_arguments_are_refused_without_a_device():
    lib = youth_rgbd.load_library()
    lv = (youth_rgbd.RgbdLevel * 4)()
    EINVAL = youth_icp.YOUTH_EINVAL
    assert lib.youth_rgbd_default_levels(640, 480, None) == EINVAL
    assert lib.youth_rgbd_set_levels(None, lv, 1) == EINVAL
    assert lib.youth_rgbd_get_levels(None, lv, 4) == EINVAL
    assert lib.youth_rgbd_get_level_poses(None, 0, 1, None, None) == EINVAL
    assert lib.youth_rgbd_get_level_stats(None, 0, 1, 1, None) == EINVAL
    assert lib.youth_rgbd_decimate_device(0, None, None, 1, 160, 120, 2, None, None, None) == EINVAL
    assert b"null" in lib.youth_rgbd_last_error()
    lp = youth_loop.load_library()
    assert lp.youth_loop_set_levels(None, lv, 1) == EINVAL
    assert lp.youth_loop_get_levels(None, lv, 4) == EINVAL
    assert lp.youth_loop_last_error()
