"""GPU tests of the C-ABI's argument checks with a live context (youth_icp.h):
every documented bad argument is refused with YOUTH_EINVAL before anything is
launched, the error text names the call, and the context aligns bit for bit
as before afterwards.  The NULL-context sweep is CPU-side (test_abi.py).  Then
the checks of the viewer cloud, the voxel map with its render, the depth filter
and the RGB-D luma entry that need a device or a live context, with their exact
texts (those that need neither: test_errors.py)."""
import ctypes

import numpy as np
import pytest
import torch

import youth_icp
import youth_synth

pytestmark = pytest.mark.gpu

E = youth_icp.YOUTH_EINVAL


def test_create_refuses_bad_sizes_and_devices():
    lib = youth_icp.load_library()
    for W, H, mf in ((2, 480, 2), (640, 2, 2), (16385, 8, 2), (8, 16385, 2),
                     (16384, 4097, 2), (640, 480, 1), (640, 480, 0), (-640, 480, 2)):
        assert not lib.youth_icp_create(0, W, H, mf, None, None), (W, H, mf)
        assert b"bad size" in lib.youth_icp_last_error()
    assert not lib.youth_icp_create(lib.youth_icp_device_count(), 64, 48, 2, None, None)
    assert b"no HIP device" in lib.youth_icp_last_error()
    assert not lib.youth_icp_create(-1, 64, 48, 2, None, None)


def test_bad_arguments_refused_context_unchanged():
    W, H, n = 160, 120, 4
    src, dst, _ = youth_synth.pairs(0, n, W, H)
    ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    seq = torch.from_numpy(np.concatenate([src, dst[-1:]])).cuda()
    ctx = youth_icp.IcpContext(W, H, n)
    lib, h = ctx._lib, ctx.handle
    ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n)
    T0, _, st0 = ctx.get_poses(n)
    assert (st0 == 0).all()

    P16 = ctypes.POINTER(ctypes.c_int16)
    host = np.zeros(W * H, np.int16)
    hp = host.ctypes.data_as(P16)
    T = np.zeros(16, np.float64)
    Tp = T.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    has = ctypes.c_int()
    ms, cnt = ctypes.c_double(), ctypes.c_int()
    calls = {
        "align_pairs null src": lambda: lib.youth_icp_align_pairs_device(
            h, None, dd.data_ptr(), 1, None, None, None),
        "align_pairs null dst": lambda: lib.youth_icp_align_pairs_device(
            h, ds.data_ptr(), None, 1, None, None, None),
        "align_pairs 0 pairs": lambda: lib.youth_icp_align_pairs_device(
            h, ds.data_ptr(), dd.data_ptr(), 0, None, None, None),
        "align_pairs -1 pairs": lambda: lib.youth_icp_align_pairs_device(
            h, ds.data_ptr(), dd.data_ptr(), -1, None, None, None),
        "align_pairs > max_frames": lambda: lib.youth_icp_align_pairs_device(
            h, ds.data_ptr(), dd.data_ptr(), n + 1, None, None, None),
        "align_sequence 1 frame": lambda: lib.youth_icp_align_sequence_device(
            h, seq.data_ptr(), 1, None, None),
        "align_sequence > max_frames": lambda: lib.youth_icp_align_sequence_device(
            h, seq.data_ptr(), n + 2, None, None),
        "get_poses > max_frames": lambda: lib.youth_icp_get_poses(h, n + 1, None, None, None),
        "get_poses -1": lambda: lib.youth_icp_get_poses(h, -1, None, None, None),
        "get_stats other iters": lambda: lib.youth_icp_get_stats(h, n, 11, None, None),
        "get_timing kind 3": lambda: lib.youth_icp_get_timing(h, 3, ctypes.byref(ms),
                                                              ctypes.byref(cnt)),
        "set_spec 7": lambda: lib.youth_icp_set_spec(h, 7),
        "set_reduce 9": lambda: lib.youth_icp_set_reduce(h, 9),
        "set_concurrency 0": lambda: lib.youth_icp_set_concurrency(h, 0),
        "set_concurrency > max": lambda: lib.youth_icp_set_concurrency(h, 99),
        "track_set_batch 0": lambda: lib.youth_icp_track_set_batch(h, 0),
        "track_set_batch > max": lambda: lib.youth_icp_track_set_batch(h, 99),
        "track_collect nothing in flight": lambda: lib.youth_icp_track_collect(
            h, Tp, ctypes.byref(has)),
        "track_collect null T": lambda: lib.youth_icp_track_collect(h, None, ctypes.byref(has)),
        "track_submit null frame": lambda: lib.youth_icp_track_submit(h, None, None),
        "track_submit_batch 0 frames": lambda: lib.youth_icp_track_submit_batch(h, hp, 0),
        "track_submit_batch > max": lambda: lib.youth_icp_track_submit_batch(h, hp, 99),
        "track_submit_pinned null list": lambda: lib.youth_icp_track_submit_pinned(h, None, 1),
        "track_submit_pinned null frame": lambda: lib.youth_icp_track_submit_pinned(
            h, (P16 * 1)(), 1),
        "track_frame null T_rel": lambda: lib.youth_icp_track_frame(h, hp, None, None, None),
        "track_realign null ref": lambda: lib.youth_icp_track_realign(h, None, hp, None, Tp),
        "track_host_sequence -1 frames": lambda: lib.youth_icp_track_host_sequence(
            h, hp, -1, Tp, None),
    }
    for name, call in calls.items():
        rc = call()
        assert rc == E, (name, rc)
        assert lib.youth_icp_last_error(), name
    # still the same context: same plan, same spec / reduction, bit-identical poses
    assert ctx.spec == youth_icp.SPEC_SURVEY
    assert lib.youth_icp_track_pending(h) == 0
    ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n)
    T1, _, st1 = ctx.get_poses(n)
    assert (st1 == 0).all() and np.array_equal(T0, T1)
    ctx.close()


# ---- the other modules' checks that need a device or a live context: exact code
# and text (the checks that need neither are CPU-side, test_errors.py)
def _refused(lib, channel, rc, code, text):
    got = (getattr(lib, f"youth_{channel}_last_error")() or b"").decode()
    assert (rc, got) == (code, text)


def test_device_index_checks_of_the_four_modules():
    """device = the device count: one text in every module that takes a device."""
    import youth_filter, youth_map, youth_rgbd, youth_viewer   # noqa: E401
    lib = youth_icp.load_library()
    for m in (youth_filter, youth_map, youth_rgbd, youth_viewer):
        m.load_library()
    n = lib.youth_icp_device_count()
    buf = torch.zeros(2 * 16 * 8 * 3, dtype=torch.uint8, device="cuda")
    a, b = buf.data_ptr(), buf.data_ptr() + 16 * 8 * 3
    assert not lib.youth_cloud_create(n, 16, 8, 1)
    _refused(lib, "cloud", E, E, f"youth_cloud_create: device {n} of {n}")
    assert not lib.youth_cloud_create(-1, 16, 8, 1)
    _refused(lib, "cloud", E, E, f"youth_cloud_create: device -1 of {n}")
    assert not lib.youth_map_create(n, 64.0, 1024)
    _refused(lib, "map", E, E, f"youth_map_create: device {n} of {n}")
    _refused(lib, "rgbd", lib.youth_rgbd_luma_device(n, a, b, 1, 16, 8, None), E,
             f"youth_rgbd_luma_device: device {n} of {n}")
    _refused(lib, "depth_filter", lib.youth_depth_filter_device(n, a, b, 1, 16, 8, None, None), E,
             f"youth_depth_filter_device: device {n} of {n}")
    with pytest.raises(youth_icp.IcpError) as e:
        youth_map.VoxelMap(64.0, 1024, device=n)
    assert e.value.code == E
    with pytest.raises(youth_icp.IcpError) as e:
        youth_viewer.CloudBuilder(16, 8, device=n)
    assert e.value.code == youth_icp.YOUTH_EHIP     # the wrapper's code for every other text


def test_cloud_checks_with_a_device():
    import youth_viewer
    lib = youth_viewer.load_library()
    need = "(need 1 <= W,H <= 16384, W*H <= 2^26, 1 <= frames <= 65535)"
    for W, H, mf in ((0, 8, 1), (16, 0, 1), (16385, 8, 1), (16384, 16384, 1), (16, 8, 0),
                     (16, 8, 65536)):
        assert not lib.youth_cloud_create(0, W, H, mf)
        _refused(lib, "cloud", E, E, f"youth_cloud_create: {W}x{H} x {mf} frames {need}")
    depth = np.full((8, 16), 1000, np.int16)
    d = torch.from_numpy(np.stack([depth] * 3)).cuda()
    out = torch.zeros(3 * 16 * 8 * 6, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
    with youth_viewer.CloudBuilder(16, 8, max_frames=2) as cb:
        h = cb._ctx
        for nf, W, H in ((3, 16, 8), (-1, 16, 8), (1, 17, 8), (1, 16, 9), (1, 0, 8), (1, 32, 4)):
            rc = lib.youth_cloud_build_device(h, d.data_ptr(), None, nf, W, H, None,
                                              out.data_ptr(), cnt.data_ptr(), None)
            _refused(lib, "cloud", rc, E, f"youth_cloud_build_device: {nf} frames of {W}x{H} "
                                          "(context: 2 of 16x8)")
        P16, PF = ctypes.POINTER(ctypes.c_int16), ctypes.POINTER(ctypes.c_float)
        host = np.zeros((16 * 8, 6), np.float32)
        rc = lib.youth_cloud_build_host(h, depth.ctypes.data_as(P16), None, 17, 8, None,
                                        host.ctypes.data_as(PF), 128)
        _refused(lib, "cloud", rc, E, "youth_cloud_build_host: 17x8 frame (context 16x8)")
        rc = lib.youth_cloud_build_host(h, depth.ctypes.data_as(P16), None, 16, 8, None,
                                        host.ctypes.data_as(PF), 127)
        _refused(lib, "cloud", rc, E, "youth_cloud_build_host: 128 vertices, room for 127")
        assert cb.build(depth).shape == (128, 6)      # and the context still builds


def test_map_checks_with_a_live_map():
    import youth_map
    lib = youth_map.load_library()
    depth = np.full((8, 16), 1000, np.int16)
    d = torch.from_numpy(depth).cuda()
    V = torch.from_numpy(np.eye(4, dtype=np.float32)[:3].copy()).cuda()
    o = torch.zeros(16 * 8, dtype=torch.int16, device="cuda")
    MV = youth_map.MapView
    with youth_map.VoxelMap(100.0, slots=1024) as m:
        h = m._map
        need = "(need 0 <= frames <= 65535, 1 <= W,H <= 16384, W*H <= 2^26)"
        for nf, W, H in ((-1, 16, 8), (65536, 16, 8), (1, 0, 8), (1, 16, 0), (1, 16385, 8),
                         (1, 16384, 16384)):
            rc = lib.youth_map_integrate_device(h, d.data_ptr(), None, nf, W, H, None, None, None)
            _refused(lib, "map", rc, E,
                     f"youth_map_integrate_device: {nf} frames of {W}x{H} {need}")
        m.integrate(depth)
        n = m.voxels()
        assert n > 1
        rec = np.zeros(n, youth_map.VOXEL_DTYPE)
        _refused(lib, "map", lib.youth_map_extract(h, rec.ctypes.data, n - 1), E,
                 f"youth_map_extract: {n} voxels, room for {n - 1}")
        who = "youth_map_render_device"

        def render(nv, view, K=None):
            return lib.youth_map_render_device(h, nv, view, K, V.data_ptr(), o.data_ptr(), None,
                                               None)

        for nv in (0, 65536):
            _refused(lib, "map", render(nv, ctypes.byref(MV(16, 8, 0, 0))), E,
                     f"{who}: {nv} views (need 1..65535)")
        _refused(lib, "map", render(1, None), E, f"{who}: null view")
        for W, H in ((0, 8), (16, 0), (16385, 8), (16384, 16384)):
            _refused(lib, "map", render(1, ctypes.byref(MV(W, H, 0, 0))), E,
                     f"{who}: {W}x{H} view (need 1 <= W,H <= 16384, W*H <= 2^26)")
        for ms in (-1, 17):
            _refused(lib, "map", render(1, ctypes.byref(MV(16, 8, ms, 0))), E,
                     f"{who}: max_splat {ms} (need 0 or 1..16)")
        for K in ((0.0, 8.0, 8.0, 4.0, 1000.0), (8.0, 8.0, float("nan"), 4.0, 1000.0),
                  (8.0, 8.0, 8.0, 4.0, -1.0), (8.0, float("inf"), 8.0, 4.0, 1000.0)):
            _refused(lib, "map", render(1, ctypes.byref(MV(16, 8, 0, 0)),
                                        ctypes.byref(youth_icp.Intrinsics(*K))), E,
                     f"{who}: intrinsics must be finite with fx, fy, depth_scale > 0")
        assert m.extract().shape == (n,)      # and the map is as it was
