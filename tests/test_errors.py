"""The error texts of libyouth_icp.so's five modules (ICP, RGB-D, viewer cloud,
voxel map with its render, depth filter): every validation failure that needs no
device gives its exact code and text; the four channels (ICP with RGB-D, cloud,
map, filter) do not touch one another; each is per thread.  No GPU needed, and
none used: every call below is refused before the device is."""
import ctypes
import threading

import numpy as np
import pytest

import youth_filter
import youth_icp
import youth_map
import youth_rgbd
import youth_viewer
from youth_icp import YOUTH_EHIP, YOUTH_EINVAL, YOUTH_ENODEV

E = YOUTH_EINVAL
# a non-null context nothing reads before the check under test refuses the call
# (zeroed and large, should a later edit read it after all), and frame buffers
_FAKE = ctypes.create_string_buffer(1 << 16)
_BUF = np.zeros(4096, np.int16)
CTX = ctypes.addressof(_FAKE)
PA = _BUF.ctypes.data
PB = PA + 4096          # [PA, PA + 1024) and [PB, PB + 1024) do not overlap

FILTER_SIZE = "need 0 <= frames <= 65535, 3 <= W, H <= 16384, W*H <= 2^26"


@pytest.fixture(scope="module")
def lib():
    for m in (youth_viewer, youth_map, youth_filter, youth_rgbd):
        m.load_library()
    return youth_icp.load_library()


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _text(lib, channel):
    return (getattr(lib, f"youth_{channel}_last_error")() or b"").decode()


def _refused(lib, channel, fn, args, code, text):
    rc = getattr(lib, fn)(*args)
    got = _text(lib, channel)
    assert (rc, got) == (code, text), (fn, args, rc, got)


def test_icp_texts(lib):
    P16, PD, PF = ctypes.POINTER(ctypes.c_int16), ctypes.POINTER(ctypes.c_double), \
        ctypes.POINTER(ctypes.c_float)
    d16, f64, f32 = ctypes.cast(PA, P16), ctypes.cast(PA, PD), ctypes.cast(PA, PF)
    for fn, args, text in (
            ("youth_icp_set_spec", (None, 5), "set_spec: bad arguments (5)"),
            ("youth_icp_set_reduce", (None, 7), "set_reduce: bad arguments (7)"),
            ("youth_icp_get_reduce", (None,), "get_reduce: null context"),
            ("youth_icp_get_lanes", (None, None), "get_lanes: bad arguments"),
            ("youth_icp_set_concurrency", (None, 1), "set_concurrency: bad arguments (1)"),
            ("youth_icp_get_spec", (None,), "get_spec: null context"),
            ("youth_icp_align_pairs_device", (None, PA, PB, 1, None, None, None),
             "align_pairs: bad arguments 1"),
            ("youth_icp_align_sequence_device", (None, PA, 3, None, None),
             "align_sequence: bad arguments 3"),
            ("youth_icp_sync", (None, None), "sync: null context"),
            ("youth_icp_get_poses", (None, 3, None, None, None), "get_poses: bad arguments 3"),
            ("youth_icp_get_stats", (None, 1, 4, None, None), "get_stats: bad arguments 4"),
            ("youth_icp_set_timing", (None, 1), "set_timing: null context"),
            ("youth_icp_get_timing", (None, 0, None, None), "get_timing: bad kind 0"),
            ("youth_icp_get_sched_stats", (None, None, None), "get_sched_stats: null context"),
            ("youth_icp_get_plan", (None, None, None), "get_plan: null context"),
            ("youth_icp_selftest_projdiv", (0, -1, 1, None, None), "selftest_projdiv: n < 0"),
            ("youth_icp_selftest_projquot", (0, -1, 1, None, None, None),
             "selftest_projquot: n < 0"),
            ("youth_icp_selftest_normalize", (0, -1, 1, None, None, None),
             "selftest_normalize: n < 0"),
            ("youth_icp_prepare_host", (None, d16, 2, 0, None, None, None, None, None, None),
             "prepare_host: bad arguments 2"),
            ("youth_icp_reduce_host", (None, d16, d16, f32, None, None),
             "reduce_host: bad arguments"),
            ("youth_icp_solve_host", (None, f64, f64), "solve_host: bad arguments"),
            ("youth_icp_align_batch", (None, d16, 4, 16, 8, None, 10, f32, None),
             "align_batch: bad arguments 4"),
            ("youth_icp_align_batch", (d16, d16, 4, 2, 8, None, 10, f32, None),
             "align_batch: bad arguments 4"),
            ("youth_icp_shard_range", (-1, 1, 0, None, None), "shard_range: bad arguments"),
            ("youth_icp_align_batch_multi", (d16, d16, 0, 16, 8, None, 10, None, 0, f32, None),
             "align_batch_multi: bad arguments 0"),
            ("youth_icp_set_depth_filter", (None, None), "set_depth_filter: null context"),
            ("youth_icp_get_depth_filter", (None, None), "get_depth_filter: null context"),
            ("youth_icp_track_submit", (None, d16, None), "track_submit: bad arguments"),
            ("youth_icp_track_submit_batch", (None, d16, 9),
             "track_submit_batch: bad arguments (9 frames)"),
            ("youth_icp_track_submit_pinned", (None, None, 1),
             "track_submit_pinned: bad arguments (1 frames)"),
            ("youth_icp_track_collect", (None, f64, None), "track_collect: bad arguments"),
            ("youth_icp_track_realign", (None, d16, d16, None, f64),
             "track_realign: bad arguments"),
            ("youth_icp_track_host_sequence", (None, d16, 2, f64, None),
             "track_host_sequence: bad arguments"),
            ("youth_icp_track_frame", (None, d16, None, f64, None), "track_frame: bad arguments"),
            ("youth_icp_track_set_batch", (None, 2), "track_set_batch: bad arguments (2)")):
        _refused(lib, "icp", fn, args, E, text)
        assert _text(lib, "rgbd") == text   # one channel, two readers


def test_icp_create_texts_and_codes(lib, has_gpu):
    need = "(need 3 <= W, H <= 16384, W*H <= 2^26, max_frames >= 2)"
    for (W, H, mf) in ((2, 8, 2), (16, 2, 2), (16385, 8, 2), (16384, 16384, 2), (16, 8, 1)):
        assert not lib.youth_icp_create(0, W, H, mf, None, None)
        assert _text(lib, "icp") == f"youth_icp_create: bad size {W}x{H} / max_frames {mf} {need}"
    # the wrapper's code for a refused size, and the host batch API's
    with pytest.raises(youth_icp.IcpError) as e:
        youth_icp.IcpContext(2, 8, 2)
    assert e.value.code == YOUTH_EHIP
    d16 = ctypes.cast(PA, ctypes.POINTER(ctypes.c_int16))
    f32 = ctypes.cast(PA, ctypes.POINTER(ctypes.c_float))
    _refused(lib, "icp", "youth_icp_align_batch", (d16, d16, 1, 16385, 8, None, 10, f32, None),
             YOUTH_EHIP, f"youth_icp_create: bad size 16385x8 / max_frames 2 {need}")
    if not has_gpu:
        assert not lib.youth_icp_create(0, 16, 8, 2, None, None)
        assert _text(lib, "icp") == "youth_icp_create: no HIP device 0"
        _refused(lib, "icp", "youth_icp_align_batch", (d16, d16, 1, 16, 8, None, 10, f32, None),
                 YOUTH_ENODEV, "youth_icp_create: no HIP device 0")
        _refused(lib, "icp", "youth_icp_align_batch_multi",
                 (d16, d16, 1, 16, 8, None, 10, None, 0, f32, None), YOUTH_ENODEV,
                 "align_batch_multi: no HIP device")
        _refused(lib, "icp", "youth_icp_selftest_projdiv", (0, 1, 1, None, None), YOUTH_ENODEV,
                 "selftest_projdiv: no HIP device 0")
        with pytest.raises(youth_icp.IcpError) as e:
            youth_icp.IcpContext(16, 8, 2)
        assert e.value.code == YOUTH_ENODEV


def test_rgbd_texts(lib, has_gpu):
    RP = youth_rgbd.RgbdParams
    need = "(need iters >= 0, dist_thresh > 0 and lambda >= 0, both finite)"
    for prm, shown in (((-1, 0.5, 0.25), "iters -1, dist_thresh 0.5, lambda 0.25"),
                       ((10, 0.0, 0.25), "iters 10, dist_thresh 0, lambda 0.25"),
                       ((10, float("inf"), 0.25), "iters 10, dist_thresh inf, lambda 0.25"),
                       ((10, 0.5, -1.0), "iters 10, dist_thresh 0.5, lambda -1"),
                       ((10, 0.5, float("nan")), "iters 10, dist_thresh 0.5, lambda nan")):
        assert not lib.youth_rgbd_create(0, 16, 8, 2, None, ctypes.byref(RP(*prm)))
        assert _text(lib, "rgbd") == f"youth_rgbd_create: bad parameters: {shown} {need}"
    need = "(need 3 <= W, H <= 16384, W*H <= 2^26, 2 <= max_frames <= 65535)"
    for (W, H, mf) in ((2, 8, 2), (16, 2, 2), (16385, 8, 2), (16384, 16384, 2), (16, 8, 1),
                       (16, 8, 65536)):
        assert not lib.youth_rgbd_create(0, W, H, mf, None, None)
        assert _text(lib, "rgbd") == \
            f"youth_rgbd_create: bad size {W}x{H} / max_frames {mf} {need}"
        assert _text(lib, "icp") == _text(lib, "rgbd")
    with pytest.raises(youth_icp.IcpError) as e:
        youth_rgbd.RgbdContext(2, 8, 2)
    assert e.value.code == E
    who = "youth_rgbd_luma_device"
    for args, text in (((0, None, PB, 1, 16, 8, None), f"{who}: null buffer"),
                       ((0, PA, None, 1, 16, 8, None), f"{who}: null buffer"),
                       ((0, PA, PB, -1, 16, 8, None), f"{who}: -1 frames of 16x8 ({FILTER_SIZE})"),
                       ((0, PA, PB, 65536, 16, 8, None),
                        f"{who}: 65536 frames of 16x8 ({FILTER_SIZE})"),
                       ((0, PA, PB, 1, 2, 8, None), f"{who}: 1 frames of 2x8 ({FILTER_SIZE})"),
                       ((0, PA, PB, 1, 16384, 16384, None),
                        f"{who}: 1 frames of 16384x16384 ({FILTER_SIZE})")):
        _refused(lib, "rgbd", who, args, E, text)
    P16, PU8 = ctypes.POINTER(ctypes.c_int16), ctypes.POINTER(ctypes.c_uint8)
    PD, PF = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    d16, u8 = ctypes.cast(PA, P16), ctypes.cast(PA, PU8)
    nan12 = np.full(12, np.nan, np.float32)
    for fn, args, text in (
            ("youth_rgbd_prep_device", (None, PA, 1, 1, None, None, None),
             "youth_rgbd_prep_device: bad arguments (channels 1, 1 frames)"),
            ("youth_rgbd_prep_device", (CTX, PA, 2, 1, None, None, None),
             "youth_rgbd_prep_device: bad arguments (channels 2, 1 frames)"),
            ("youth_rgbd_prep_device", (CTX, PA, 3, 65536, None, None, None),
             "youth_rgbd_prep_device: bad arguments (channels 3, 65536 frames)"),
            ("youth_rgbd_align_pairs_device", (None, PA, PA, PA, PA, 1, None, None, None),
             "youth_rgbd_align_pairs_device: null context"),
            ("youth_rgbd_align_pairs_device", (CTX, PA, None, PA, PA, 1, None, None, None),
             "youth_rgbd_align_pairs_device: null buffer"),
            ("youth_rgbd_align_sequence_device", (None, PA, PA, 2, None, None),
             "youth_rgbd_align_sequence_device: null context"),
            ("youth_rgbd_align_sequence_device", (CTX, PA, None, 2, None, None),
             "youth_rgbd_align_sequence_device: null buffer"),
            ("youth_rgbd_sync", (None, None), "youth_rgbd_sync: null context"),
            ("youth_rgbd_get_poses", (None, 3, None, None, None),
             "youth_rgbd_get_poses: bad arguments (3 poses)"),
            ("youth_rgbd_get_stats", (None, 1, 2, None),
             "youth_rgbd_get_stats: bad arguments (1 pairs, 2 iterations)"),
            ("youth_rgbd_reduce_host", (None, d16, u8, d16, u8, _p(nan12, ctypes.c_float),
                                        ctypes.cast(PA, PD)),
             "youth_rgbd_reduce_host: null context"),
            ("youth_rgbd_reduce_host", (CTX, d16, u8, d16, u8, None, ctypes.cast(PA, PD)),
             "youth_rgbd_reduce_host: null buffer"),
            ("youth_rgbd_reduce_host", (CTX, d16, u8, d16, u8, _p(nan12, ctypes.c_float),
                                        ctypes.cast(PA, PD)),
             "youth_rgbd_reduce_host: non-finite pose"),
            ("youth_rgbd_track_host_sequence", (None, d16, u8, 2, ctypes.cast(PA, PD), None),
             "youth_rgbd_track_host_sequence: null context"),
            ("youth_rgbd_track_host_sequence", (CTX, d16, None, 2, ctypes.cast(PA, PD), None),
             "youth_rgbd_track_host_sequence: null buffer")):
        _refused(lib, "rgbd", fn, args, E, text)
    if not has_gpu:
        _refused(lib, "rgbd", who, (0, PA, PB, 1, 16, 8, None), YOUTH_ENODEV,
                 f"{who}: no HIP device visible")
        assert not lib.youth_rgbd_create(0, 16, 8, 2, None, None)
        assert _text(lib, "rgbd") == "youth_icp_create: no HIP device 0"


def test_cloud_texts(lib, has_gpu):
    P16, PF = ctypes.POINTER(ctypes.c_int16), ctypes.POINTER(ctypes.c_float)
    for fn, args, text in (
            ("youth_cloud_build_device", (None, PA, None, 1, 16, 8, None, PA, PA, None),
             "youth_cloud_build_device: null argument"),
            ("youth_cloud_build_device", (CTX, None, None, 1, 16, 8, None, PA, PA, None),
             "youth_cloud_build_device: null argument"),
            ("youth_cloud_build_device", (CTX, PA, None, 1, 16, 8, None, PA, None, None),
             "youth_cloud_build_device: null argument"),
            ("youth_cloud_build_device_posed",
             (CTX, PA, None, 1, 16, 8, None, None, None, PA, None),
             "youth_cloud_build_device: null argument"),
            ("youth_cloud_build_host", (None, ctypes.cast(PA, P16), None, 16, 8, None,
                                        ctypes.cast(PB, PF), 128),
             "youth_cloud_build_host: null argument"),
            ("youth_cloud_build_host", (CTX, ctypes.cast(PA, P16), None, 16, 8, None,
                                        ctypes.cast(PB, PF), -1),
             "youth_cloud_build_host: null argument"),
            ("youth_cloud_sync", (None, None), "youth_cloud_sync: null context")):
        _refused(lib, "cloud", fn, args, E, text)
    if not has_gpu:
        assert not lib.youth_cloud_create(0, 16, 8, 1)
        assert _text(lib, "cloud") == "youth_cloud_create: no HIP device visible"
        with pytest.raises(youth_icp.IcpError) as e:
            youth_viewer.CloudBuilder(16, 8)
        assert e.value.code == YOUTH_ENODEV


def test_map_texts(lib, has_gpu, tmp_path):
    need = "(need finite vpm > 0, 1 <= slots <= 2^28)"
    for vpm, slots, shown in ((0.0, 16, "vpm 0, 16 slots"), (-2.0, 16, "vpm -2, 16 slots"),
                              (float("nan"), 16, "vpm nan, 16 slots"),
                              (float("inf"), 16, "vpm inf, 16 slots"),
                              (64.0, 0, "vpm 64, 0 slots"),
                              (64.0, (1 << 28) + 1, "vpm 64, 268435457 slots")):
        assert not lib.youth_map_create(0, vpm, slots)
        assert _text(lib, "map") == f"youth_map_create: {shown} {need}"
    with pytest.raises(youth_icp.IcpError) as e:
        youth_map.VoxelMap(0.0)
    assert e.value.code == E
    P16, PD, PF = ctypes.POINTER(ctypes.c_int16), ctypes.POINTER(ctypes.c_double), \
        ctypes.POINTER(ctypes.c_float)
    d16 = ctypes.cast(PA, P16)
    T = np.eye(4).reshape(-1)
    T_nan = T.copy()
    T_nan[7] = np.nan
    T_big = T.copy()
    T_big[3] = 1e300     # finite in fp64, not in fp32
    vox = np.zeros(3, youth_map.VOXEL_DTYPE)
    vox["count"] = (1, 0, 1)
    out6 = np.zeros((3, 6), np.float32)
    view = youth_map.MapView(16, 8, 0, 0)
    for fn, args, text in (
            ("youth_map_clear", (None,), "youth_map_clear: null map"),
            ("youth_map_set_max_depth", (None, 1),
             "youth_map_set_max_depth: null map or negative depth"),
            ("youth_map_set_max_depth", (CTX, -1),
             "youth_map_set_max_depth: null map or negative depth"),
            ("youth_map_integrate_device", (None, PA, None, 1, 16, 8, None, None, None),
             "youth_map_integrate_device: null argument"),
            ("youth_map_integrate_device", (CTX, None, None, 1, 16, 8, None, None, None),
             "youth_map_integrate_device: null argument"),
            ("youth_map_integrate_host", (None, d16, None, 16, 8, None, None),
             "youth_map_integrate_host: null argument"),
            ("youth_map_integrate_host", (CTX, None, None, 16, 8, None, None),
             "youth_map_integrate_host: null argument"),
            ("youth_map_integrate_host", (CTX, d16, None, 0, 8, None, None),
             "youth_map_integrate_host: 0x8 frame"),
            ("youth_map_integrate_host", (CTX, d16, None, 16385, 8, None, None),
             "youth_map_integrate_host: 16385x8 frame"),
            ("youth_map_integrate_host", (CTX, d16, None, 16384, 16384, None, None),
             "youth_map_integrate_host: 16384x16384 frame"),
            ("youth_map_integrate_host", (CTX, d16, None, 16, 8, None, _p(T_nan, ctypes.c_double)),
             "youth_map_integrate_host: pose entry 7 is not finite"),
            ("youth_map_integrate_host", (CTX, d16, None, 16, 8, None, _p(T_big, ctypes.c_double)),
             "youth_map_integrate_host: pose entry 3 is not finite"),
            ("youth_map_voxels", (None,), "youth_map_voxels: null map"),
            ("youth_map_stats", (None, None), "youth_map_stats: null argument"),
            ("youth_map_stats", (CTX, None), "youth_map_stats: null argument"),
            ("youth_map_extract", (None, None, 0), "youth_map_extract: null argument"),
            ("youth_map_extract", (CTX, None, -1), "youth_map_extract: null argument"),
            ("youth_map_extract", (CTX, None, 4), "youth_map_extract: null argument"),
            ("youth_map_sync", (None, None), "youth_map_sync: null map"),
            ("youth_map_points", (vox.ctypes.data, -1, 64.0, _p(out6, ctypes.c_float)),
             "youth_map_points: bad argument"),
            ("youth_map_points", (None, 3, 64.0, _p(out6, ctypes.c_float)),
             "youth_map_points: bad argument"),
            ("youth_map_points", (vox.ctypes.data, 3, 0.0, _p(out6, ctypes.c_float)),
             "youth_map_points: bad argument"),
            ("youth_map_points", (vox.ctypes.data, 3, 64.0, _p(out6, ctypes.c_float)),
             "youth_map_points: record 1 is empty"),
            ("youth_map_write_ply", (None, vox.ctypes.data, 3, 64.0),
             "youth_map_write_ply: bad argument"),
            ("youth_map_write_ply", (b"x.ply", None, 3, 64.0), "youth_map_write_ply: bad argument"),
            ("youth_map_write_ply", (b"x.ply", vox.ctypes.data, 3, float("nan")),
             "youth_map_write_ply: bad argument"),
            ("youth_map_write_ply", (str(tmp_path / "x.ply").encode(), vox.ctypes.data, 3, 64.0),
             "youth_map_write_ply: record 1 is empty"),
            ("youth_map_write_ply", (str(tmp_path / "none" / "x.ply").encode(), vox.ctypes.data,
                                     1, 64.0),
             f"youth_map_write_ply: cannot open {tmp_path / 'none' / 'x.ply'}"),
            ("youth_map_view_from_pose", (None, _p(out6, ctypes.c_float)),
             "youth_map_view_from_pose: null argument"),
            ("youth_map_view_from_pose", (_p(T, ctypes.c_double), None),
             "youth_map_view_from_pose: null argument"),
            ("youth_map_view_from_pose", (_p(T_nan, ctypes.c_double), _p(out6, ctypes.c_float)),
             "youth_map_view_from_pose: pose entry 7 is not finite"),
            ("youth_map_view_from_pose", (_p(T_big, ctypes.c_double), _p(out6, ctypes.c_float)),
             "youth_map_view_from_pose: entry 3 of the view is not finite"),
            ("youth_map_render_device", (None, 1, ctypes.byref(view), None, PA, PA, None, None),
             "youth_map_render_device: null argument"),
            ("youth_map_render_device", (CTX, 1, ctypes.byref(view), None, None, PA, None, None),
             "youth_map_render_device: null argument"),
            ("youth_map_render_host", (None, ctypes.byref(view), None, None, d16, None),
             "youth_map_render_host: null argument"),
            ("youth_map_render_host", (CTX, ctypes.byref(view), None, None, None, None),
             "youth_map_render_host: null argument"),
            ("youth_map_render_host", (CTX, ctypes.byref(view), None, _p(T_nan, ctypes.c_double),
                                       d16, None),
             "youth_map_view_from_pose: pose entry 7 is not finite")):
        _refused(lib, "map", fn, args, E, text)
    assert not (tmp_path / "x.ply").exists()
    if not has_gpu:
        assert not lib.youth_map_create(0, 64.0, 1024)
        assert _text(lib, "map") == "youth_map_create: no HIP device visible"
        with pytest.raises(youth_icp.IcpError) as e:
            youth_map.VoxelMap(64.0, 1024)
        assert e.value.code == YOUTH_ENODEV


def test_filter_texts(lib, has_gpu):
    FP = youth_icp.FilterParams
    P16 = ctypes.POINTER(ctypes.c_int16)
    ha, hb = ctypes.cast(PA, P16), ctypes.cast(PB, P16)
    for who, a, b, tail in (("youth_depth_filter_device", PA, PB, (None,)),
                            ("youth_depth_filter_host", ha, hb, ())):
        for args, text in (
                ((0, None, b, 1, 16, 8, None), f"{who}: null buffer"),
                ((0, a, None, 1, 16, 8, None), f"{who}: null buffer"),
                ((0, a, b, -1, 16, 8, None), f"{who}: -1 frames of 16x8 ({FILTER_SIZE})"),
                ((0, a, b, 65536, 16, 8, None), f"{who}: 65536 frames of 16x8 ({FILTER_SIZE})"),
                ((0, a, b, 1, 2, 8, None), f"{who}: 1 frames of 2x8 ({FILTER_SIZE})"),
                ((0, a, b, 1, 16, 2, None), f"{who}: 1 frames of 16x2 ({FILTER_SIZE})"),
                ((0, a, b, 1, 16385, 8, None), f"{who}: 1 frames of 16385x8 ({FILTER_SIZE})"),
                ((0, a, b, 1, 16384, 16384, None),
                 f"{who}: 1 frames of 16384x16384 ({FILTER_SIZE})"),
                ((0, a, b, 1, 16, 8, ctypes.byref(FP(0, 96))),
                 f"{who}: t0 0, t2 96 (need 1 <= t0 <= 255, 0 <= t2 <= 1000)"),
                ((0, a, b, 1, 16, 8, ctypes.byref(FP(256, 96))),
                 f"{who}: t0 256, t2 96 (need 1 <= t0 <= 255, 0 <= t2 <= 1000)"),
                ((0, a, b, 1, 16, 8, ctypes.byref(FP(8, -1))),
                 f"{who}: t0 8, t2 -1 (need 1 <= t0 <= 255, 0 <= t2 <= 1000)"),
                ((0, a, b, 1, 16, 8, ctypes.byref(FP(8, 1001))),
                 f"{who}: t0 8, t2 1001 (need 1 <= t0 <= 255, 0 <= t2 <= 1000)")):
            _refused(lib, "depth_filter", who, args + tail, E, text)
    who = "youth_depth_filter_device"
    for out in (PA, PA + 2 * 100, PA - 2 * 100):     # the same buffer, overlapping either way
        _refused(lib, "depth_filter", who, (0, PA, out, 1, 16, 8, None, None), E,
                 f"{who}: the output overlaps the input")
    if not has_gpu:
        for who, args in (("youth_depth_filter_device", (0, PA, PB, 1, 16, 8, None, None)),
                          ("youth_depth_filter_host", (0, ha, hb, 1, 16, 8, None))):
            _refused(lib, "depth_filter", who, args, YOUTH_ENODEV,
                     f"{who}: no HIP device visible")


# one refused call per channel, and a second one with another text
CHANNELS = {
    "icp": (("youth_icp_sync", (None, None), "sync: null context"),
            ("youth_icp_get_spec", (None,), "get_spec: null context")),
    "cloud": (("youth_cloud_sync", (None, None), "youth_cloud_sync: null context"),
              ("youth_cloud_build_host", (None, None, None, 16, 8, None, None, 0),
               "youth_cloud_build_host: null argument")),
    "map": (("youth_map_sync", (None, None), "youth_map_sync: null map"),
            ("youth_map_clear", (None,), "youth_map_clear: null map")),
    "depth_filter": (("youth_depth_filter_device", (0, None, None, 1, 16, 8, None, None),
                      "youth_depth_filter_device: null buffer"),
                     ("youth_depth_filter_host", (0, None, None, 1, 16, 8, None),
                      "youth_depth_filter_host: null buffer")),
}


def _fail(lib, channel, which):
    fn, args, text = CHANNELS[channel][which]
    assert getattr(lib, fn)(*args) == E
    assert _text(lib, channel) == text
    return text


def test_channels_are_independent(lib):
    """A failure in one module leaves the other three modules' texts as they
    were: every ordered pair (failing channel, observed channel)."""
    for a in CHANNELS:
        before = {c: _fail(lib, c, 0) for c in CHANNELS}
        assert _text(lib, "rgbd") == before["icp"]
        changed = _fail(lib, a, 1)
        assert changed != before[a]
        for b in CHANNELS:
            if b != a:
                assert _text(lib, b) == before[b], (a, b)
        assert _text(lib, "rgbd") == (changed if a == "icp" else before["icp"])


def test_texts_are_per_thread(lib):
    mine = {c: _fail(lib, c, 0) for c in CHANNELS}
    seen = {}

    def other():
        seen["fresh"] = {c: _text(lib, c) for c in CHANNELS}
        seen["own"] = {c: _fail(lib, c, 1) for c in CHANNELS}
        seen["after"] = {c: _text(lib, c) for c in CHANNELS}

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen["fresh"] == {c: "" for c in CHANNELS}     # a new thread has no error yet
    assert seen["after"] == seen["own"] == {c: CHANNELS[c][1][2] for c in CHANNELS}
    assert {c: _text(lib, c) for c in CHANNELS} == mine   # and this thread's texts stand
