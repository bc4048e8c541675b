"""The streaming tracker's level schedule (include/youth_rgbd.h
youth_rgbd_track_set_levels), CPU side: the new symbols,
NULL without a device, and what the schedule is worth on pairs ten frames apart
by the numpy truth (tests/rgbd_track_levels_truth.py)."""
import ctypes
import os

import numpy as np

import rgbd_track_levels_truth as tt
import youth_icp
import youth_rgbd
from conftest import PKG, ROOT

NEW = ["youth_rgbd_track_set_levels", "youth_rgbd_track_get_levels", "youth_rgbd_track_last_levels"]


def test_new_symbols_are_declared_exported_and_bound():
    declared = youth_icp.declared_functions(os.path.join(ROOT, "include", "youth_rgbd.h"))
    lib = ctypes.CDLL(os.path.join(PKG, "libyouth_icp.so"))
    for n in NEW:
        assert n in declared and hasattr(lib, n) and n in youth_rgbd._SIGS, n
    assert set(declared) <= set(youth_rgbd._SIGS)
    bound = youth_rgbd.load_library()
    for n in NEW:
        assert getattr(bound, n).argtypes is not None
    for m in ("track_set_levels", "track_levels", "track_last_levels"):
        assert callable(getattr(youth_rgbd.RgbdContext, m)), m


def test_null_arguments_are_refused_without_a_device():
    lib = youth_rgbd.load_library()
    lv = (youth_rgbd.RgbdLevel * 4)()
    T = (ctypes.c_double * 64)()
    st = (ctypes.c_int32 * 4)()
    E = youth_icp.YOUTH_EINVAL
    text = lambda: (lib.youth_rgbd_last_error() or b"").decode()
    assert lib.youth_rgbd_track_set_levels(None, lv, 1) == E
    assert "youth_rgbd_track_set_levels" in text() and "null" in text()
    assert lib.youth_rgbd_track_set_levels(None, None, 0) == E
    assert lib.youth_rgbd_track_get_levels(None, lv, 4) == E
    assert "youth_rgbd_track_get_levels" in text()
    assert lib.youth_rgbd_track_get_levels(None, None, 0) == E
    assert lib.youth_rgbd_track_last_levels(None, T, st) == E
    assert "youth_rgbd_track_last_levels" in text()
    assert lib.youth_rgbd_track_last_levels(None, None, None) == E


def test_the_schedule_keeps_a_track_of_distant_pairs():
    T, st, per = tt.track(tt.SCHEDULE)
    F, fst, _ = tt.track(tt.FLAT)
    lev, flat = tt.end_error(T), tt.end_error(F)
    print(f"frames {tt.FRAMES[0]} .. {tt.FRAMES[-1]} by tens: no schedule {flat[0]:.3f} deg / "
          f"{flat[1]:.2f} mm, 2:10 -> 1:10 {lev[0]:.3f} deg / {lev[1]:.2f} mm")
    assert T.shape == (10, 4, 4) and len(per) == 10 and all(len(p) == 2 for p in per)
    assert (st == 0).all() and (fst == 0).all()
    assert lev[0] <= tt.BOUND_SCHEDULE[0] and lev[1] <= tt.BOUND_SCHEDULE[1]
    assert flat[0] > tt.FLOOR_FLAT[0] and flat[1] > tt.FLOOR_FLAT[1]
    # the constants are the figures measured here
    assert np.allclose(lev, tt.END_SCHEDULE, rtol=0.01) and np.allclose(flat, tt.END_FLAT, rtol=0.01)
