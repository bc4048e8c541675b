"""GPU parity of the map render (include/youth_map_render.h):
k_map_render_splat / k_map_render_resolve against the numpy restatement of the
definition (render_truth.py) applied to the map's own extract().  The render is
a minimum over integers built from fp32 evaluated as written, so every
comparison is exact equality of the depth and RGB bytes; nothing is
tolerance-based.  Every case runs the kernels' real launch geometry."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import youth_icp
import youth_map
from conftest import ORACLE, PKG, ROOT
from render_truth import candidates, project, render, view_from_pose
from test_gpu_map import _frame, _pose
from test_render import scene_case, scene_figures

pytestmark = pytest.mark.gpu

K_RAND = (525.0, 523.5, 81.25, 59.5, 5000.0)


def _same(got, want):
    assert got[0].dtype == np.int16 and got[0].shape == want[0].shape
    assert got[0].tobytes() == want[0].tobytes(), \
        f"{int((got[0] != want[0]).sum())} depth pixels differ"
    if want[1] is not None and got[1] is not None:
        assert got[1].dtype == np.uint8 and got[1].tobytes() == want[1].tobytes(), \
            f"{int((got[1] != want[1]).any(-1).sum())} colour pixels differ"


def _render_device(m, Vs, W, H, K, rgb=True, offset=0, stream=0, fill=0x5a, **kw):
    """render_device into torch buffers -> [(depth, rgb)] per view; the
    outputs start `offset` elements into their allocations."""
    n = len(Vs)
    d_V = torch.from_numpy(np.ascontiguousarray(np.stack(Vs), np.float32).reshape(n, 12)).cuda()
    d_d = torch.full((n * H * W + offset,), fill, dtype=torch.int16, device="cuda")
    d_c = torch.full((n * H * W * 3 + offset,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    m.render_device(d_V.data_ptr(), d_d.data_ptr() + 2 * offset,
                    d_c.data_ptr() + offset if rgb else 0, n, W, H, K, stream=stream, **kw)
    m.sync(stream)
    dd = d_d.cpu().numpy()
    cc = d_c.cpu().numpy()
    assert (dd[:offset] == fill).all() and (cc[:offset] == fill).all()
    if not rgb:
        assert (cc == fill).all()
    dd, cc = dd[offset:].reshape(n, H, W), cc[offset:].reshape(n, H, W, 3)
    return [(dd[k], cc[k] if rgb else None) for k in range(n)]


# ---------------------------------------------------- 1 the hand-made scene --
HAND_K_IN = (8.0, 8.0, 4.0, 3.0, 1000.0)
HAND_VPM = 50.0


def hand_frames():
    """8x6 frames: a near wall (0.2 m: footprints of 2 px that overlap, equal d
    with different colours), a wall at 1 m, single-point voxels at 3 m, a row
    at 0.02 m (a 16-px footprint before the clamp); the same scene again turned
    behind the camera; the near wall a second time (count 2)."""
    rng = np.random.default_rng(8)
    depth = np.zeros((6, 8), np.int16)
    depth[0:2], depth[2:4], depth[4], depth[5] = 200, 1000, 3000, 20
    depth[3, 6] = 0
    again = np.zeros_like(depth)
    again[0:2] = 200
    turn = np.array([[-1, 0, 0, 0.02], [0, 1, 0, 0.01], [0, 0, -1, -0.3]], np.float32)
    K = youth_icp.Intrinsics(*HAND_K_IN)
    eye = np.eye(4, dtype=np.float32)[:3]
    return [(depth, rng.integers(0, 256, (6, 8, 3)).astype(np.uint8), K, eye),
            (depth, rng.integers(0, 256, (6, 8, 3)).astype(np.uint8), K, turn),
            (again, rng.integers(0, 256, (6, 8, 3)).astype(np.uint8), K, eye)]


def hand_views():
    """(V, K, max_splat, min_count) at 16x12."""
    K = youth_icp.Intrinsics(16.0, 16.0, 8.0, 6.0, 1000.0)
    eye = np.eye(4)
    views = [(view_from_pose(eye), K, ms, mc) for ms, mc in ((16, 1), (3, 1), (1, 1), (16, 2))]
    for dx, dy in ((0.25, 0.0), (-0.25, 0.0), (0.0, 0.2), (0.0, -0.2), (2.2, 0.0)):
        T = eye.copy()
        T[:3, 3] = (dx, dy, -0.05)
        views.append((view_from_pose(T), K, 16, 1))
    views.append((view_from_pose(eye), youth_icp.Intrinsics(16.0, 16.0, 8.0, 6.0, 0.4), 16, 1))
    views.append((view_from_pose(eye), youth_icp.Intrinsics(16.0, 16.0, 8.0, 6.0, 60000.0), 16, 1))
    return views


def hand_scene_properties(rec):
    """What the hand-made scene exercises, counted on the truth."""
    W, H = 16, 12
    got = dict(behind=0, d_zero=0, d_far=0, left=0, right=0, top=0, bottom=0, outside=0,
               clamped=0, nearer=0, tie=0, few=0)
    for V, K, ms, mc in hand_views():
        why = {}
        u0, v0, s, val = project(rec, HAND_VPM, V, K, W, H, ms, mc, why)
        for k in ("behind", "d_zero", "d_far"):
            got[k] += why[k]
        inx, iny = (u0 < W) & (u0 + s > 0), (v0 < H) & (v0 + s > 0)
        got["left"] += int(((u0 < 0) & inx & iny).sum())
        got["right"] += int(((u0 + s > W) & inx & iny).sum())
        got["top"] += int(((v0 < 0) & inx & iny).sum())
        got["bottom"] += int(((v0 + s > H) & inx & iny).sum())
        got["outside"] += int((~(inx & iny)).sum())
        got["clamped"] += int(((s == ms) & (ms < 16)).sum())
        got["few"] += int(mc == 2 and (rec["count"] == 1).any())
        pix, vals = candidates(u0, v0, s, val, W, H)
        z = np.full(W * H, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(z, pix, vals)
        got["nearer"] += int(((vals >> 24) > (z[pix] >> 24)).sum())
        got["tie"] += int((((vals >> 24) == (z[pix] >> 24)) & (vals != z[pix])).sum())
    return got


def test_hand_made_scene():
    frames = hand_frames()
    with youth_map.VoxelMap(HAND_VPM, slots=1024) as m:
        for d, c, K, T in frames:
            m.integrate(d, c, K, T)
        rec = m.extract()
        props = hand_scene_properties(rec)
        assert all(v > 0 for v in props.values()), props
        for V, K, ms, mc in hand_views():
            want = render(rec, HAND_VPM, V, K, 16, 12, ms, mc)
            got = _render_device(m, [V], 16, 12, K, max_splat=ms, min_count=mc)[0]
            _same(got, want)
        # the row at 0.02 m: 16 px asked for, max_splat rules
        areas = [int((render(rec, HAND_VPM, hand_views()[k][0], hand_views()[k][1], 16, 12,
                             hand_views()[k][2], 1)[0] == 20).sum()) for k in range(3)]
        assert areas[0] > areas[1] > areas[2] > 0


def test_zbuffer_and_staging_grow_and_are_reused():
    """youth_map_render_host at 4x4 (depth only), 16x8 with colour, 4x4 with
    colour on one map: the z-buffer grows and its new words must read all ones,
    the colour staging grows on its own, and the smaller view then runs on the
    larger buffers."""
    with youth_map.VoxelMap(HAND_VPM, slots=1024) as m:
        for d, c, K, T in hand_frames():
            m.integrate(d, c, K, T)
        rec = m.extract()
        for W, H, rgb in ((4, 4, False), (16, 8, True), (4, 4, True)):
            K = youth_icp.Intrinsics(float(W), float(W), W / 2.0, H / 2.0, 1000.0)
            want = render(rec, HAND_VPM, view_from_pose(np.eye(4)), K, W, H)
            assert (want[0] > 0).sum() > W * H // 4
            _same(m.render(np.eye(4), W, H, K, want_rgb=rgb), want)


# ---------------------------------------------------- 2 random colour frames --
def _random_map(m, W, H, n=3, seed=0):
    rng = np.random.default_rng(seed)
    K = youth_icp.Intrinsics(*K_RAND)
    for f in range(n):
        d, c = _frame(W, H, seed * 10 + f)
        m.integrate(d, c, K, _pose(rng))
    return K


def _three_views(rec, vpm):
    rng = np.random.default_rng(77)
    near = np.vstack([_pose(rng), [0, 0, 0, 1]]).astype(np.float64)
    big = np.eye(4)
    big[:3, :3] = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], float)     # from the side, along -x
    big[:3, 3] = (3.0, 0.1, 3.0)
    inside = np.eye(4)
    mid = rec[rec.shape[0] // 2]
    inside[:3, 3] = (mid["ix"] / vpm, mid["iy"] / vpm, mid["iz"] / vpm)     # in the cloud
    return [view_from_pose(T) for T in (near, big, inside)]


@pytest.mark.parametrize("W,H,Wo,Ho,offset", [(97, 53, 97, 53, 0), (97, 53, 64, 48, 1),
                                              (160, 120, 161, 75, 0), (160, 120, 320, 240, 0)])
def test_random_frames_three_views(W, H, Wo, Ho, offset):
    """Output sizes other than the input's, odd W (the element-wise resolve),
    outputs offset by one element (misaligned: element-wise too); one call of
    three views == three calls of one == the truth.  On a torch stream."""
    vpm = 100.0
    stream = torch.cuda.current_stream().cuda_stream
    with youth_map.VoxelMap(vpm, slots=1 << 17) as m:
        K = _random_map(m, W, H, seed=W)
        rec = m.extract()
        Ko = youth_icp.Intrinsics(K.fx * Wo / W, K.fy * Wo / W, K.cx * Wo / W, K.cy * Ho / H,
                                  K.depth_scale)
        Vs = _three_views(rec, vpm)
        want = [render(rec, vpm, V, Ko, Wo, Ho) for V in Vs]
        kept = [int((w[0] > 0).sum()) for w in want]
        seen = [project(rec, vpm, V, Ko, Wo, Ho)[0].size for V in Vs]
        assert kept[0] > Wo * Ho // 20 and kept[1] > 0 and kept[2] > 0
        assert seen[1] < rec.shape[0] // 2 < seen[0]      # the side view culls most voxels
        together = _render_device(m, Vs, Wo, Ho, Ko, offset=offset, stream=stream)
        for k, V in enumerate(Vs):
            _same(together[k], want[k])
            _same(_render_device(m, [V], Wo, Ho, Ko, offset=offset, stream=stream)[0], want[k])


# -------------------------------------------------------- 3 both splat paths --
_PATH_CHILD = r"""
import sys
import numpy as np
import youth_icp, youth_map
sys.path.insert(0, sys.argv[2])
from test_gpu_map import _frame, _pose
from render_truth import view_from_pose
out = sys.argv[1]
K = youth_icp.Intrinsics(525.0, 523.5, 81.25, 59.5, 5000.0)
rng = np.random.default_rng(4)
res = {}
with youth_map.VoxelMap(100.0, slots=1 << 16) as m:
    for f in range(2):
        d, c = _frame(160, 120, 900 + f)
        m.integrate(d, c, K, _pose(rng))
    T = np.vstack([_pose(rng), [0, 0, 0, 1]]).astype(np.float64)
    res["rec0"], st0 = m.extract(), m.stats()
    res["d0"], res["c0"] = m.render(T, 160, 120, K)
    res["d1"], res["c1"] = m.render(T, 160, 120, K)
    res["d_small"], res["c_small"] = m.render(T, 40, 30, K, max_splat=2)
    res["d2"], res["c2"] = m.render(T, 160, 120, K)
    res["rec1"], st1 = m.extract(), m.stats()
    assert st0 == st1, (st0, st1)
    d, c = _frame(160, 120, 950)
    m.integrate(d, c, K, _pose(rng))
    res["rec2"] = m.extract()
    res["d3"], res["c3"] = m.render(T, 160, 120, K)
np.savez(out, T=T, **res)
"""


def _path_child(tmp_path, queue):
    out = tmp_path / f"queue{queue}.npz"
    env = dict(os.environ, YOUTH_MAP_RENDER_QUEUE=str(queue),
               PYTHONPATH=os.pathsep.join([PKG, ORACLE] + [p for p in sys.path if p]))
    r = subprocess.run([sys.executable, "-c", _PATH_CHILD, str(out), os.path.join(ROOT, "tests")],
                       env=env, timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return np.load(out, allow_pickle=False)


def test_both_splat_paths_give_identical_bytes(tmp_path):
    """YOUTH_MAP_RENDER_QUEUE is read at create, so each path runs in a child.
    Per path: a second render of a view is identical (the resolve reset the
    z-buffer), also after a render of another size in between; extract() and
    stats() are unchanged by rendering; a render after one more integrate sees
    the new voxels.  Across paths: the same bytes, which are the truth's."""
    runs = [_path_child(tmp_path, q) for q in (0, 1)]
    K = youth_icp.Intrinsics(*K_RAND)
    a = runs[0]
    V = view_from_pose(a["T"])
    want = render(a["rec0"], 100.0, V, K, 160, 120)
    want3 = render(a["rec2"], 100.0, V, K, 160, 120)
    assert (want[0] > 0).sum() > 1000 and not np.array_equal(want[0], want3[0])
    for r in runs:
        assert r["rec0"].tobytes() == a["rec0"].tobytes() == r["rec1"].tobytes()
        for k in "012":
            _same((r["d" + k], r["c" + k]), want)
        _same((r["d_small"], r["c_small"]), render(a["rec0"], 100.0, V, K, 40, 30, 2))
        _same((r["d3"], r["c3"]), want3)


# ------------------------------------------------------------ 4 table sizes --
@pytest.mark.parametrize("slots,W,H,vpm", [(64, 8, 6, 20.0), (1 << 20, 97, 53, 100.0)])
def test_table_sizes(slots, W, H, vpm):
    """64 slots: a grid smaller than one workgroup, the table more than half
    full; 2^20 slots: 1024 workgroups, almost all of them empty."""
    with youth_map.VoxelMap(vpm, slots=slots) as m:
        d, c = _frame(W, H, 31, holes=0.0, negative=False)
        K = youth_icp.Intrinsics(*K_RAND)
        m.integrate(d, c, K)
        st, rec = m.stats(), m.extract()
        assert st["capacity"] == slots and st["dropped"] == 0
        if slots == 64:
            assert rec.shape[0] > 32
        V = view_from_pose(np.eye(4))
        _same(_render_device(m, [V], W, H, K)[0], render(rec, vpm, V, K, W, H))


# ------------------------------------------- 5 depth only, colourless map --
def test_depth_only_and_colourless():
    W, H, vpm = 97, 53, 100.0
    K = youth_icp.Intrinsics(*K_RAND)
    d, c = _frame(W, H, 61)
    V = view_from_pose(np.eye(4))
    with youth_map.VoxelMap(vpm, slots=1 << 16) as m:
        m.integrate(d, c, K)
        want = render(m.extract(), vpm, V, K, W, H)
        for offset in (0, 1):                            # rgb NULL: never written
            _same(_render_device(m, [V], W, H, K, rgb=False, offset=offset)[0], (want[0], None))
        depth, rgb = m.render(None, W, H, K, want_rgb=False)
        assert rgb is None and np.array_equal(depth, want[0])
        m.clear()
        m.integrate(d, None, K)                          # a colourless map
        got = _render_device(m, [V], W, H, K)[0]
        _same(got, render(m.extract(), vpm, V, K, W, H))
        assert np.array_equal(got[0], want[0]) and (got[1] == 0).all()


# ------------------------------------------------------------ 6 render_host --
def test_render_host_equals_render_device():
    W, H, vpm = 97, 53, 100.0
    rng = np.random.default_rng(6)
    with youth_map.VoxelMap(vpm, slots=1 << 16) as m:
        K = _random_map(m, W, H, seed=6)
        rec = m.extract()
        T = np.vstack([_pose(rng), [0, 0, 0, 1]]).astype(np.float64)
        V = youth_map.view_from_pose(T)
        assert np.array_equal(V.view(np.uint32), view_from_pose(T).view(np.uint32))
        host = m.render(T, 120, 90, K, max_splat=4, min_count=1)
        _same(host, _render_device(m, [V], 120, 90, K, max_splat=4, min_count=1)[0])
        _same(host, render(rec, vpm, V, K, 120, 90, 4, 1))
        _same(m.render(T[:3], 120, 90, K, max_splat=4), host)       # 3x4 accepted
        eye = m.render(None, 120, 90, K)                 # NULL pose = the identity
        _same(eye, m.render(np.eye(4), 120, 90, K))
        _same(eye, render(rec, vpm, np.eye(4)[:3], K, 120, 90))
        # K NULL: the viewer's intrinsics of the output size
        _same(m.render(None, 120, 90), render(rec, vpm, np.eye(4)[:3],
                                              youth_icp.Intrinsics(570.3, 570.3, 60.0, 45.0, 1000.0),
                                              120, 90))


# ----------------------------------------------------------------- 7 EINVAL --
def test_einval_sweep_leaves_outputs_untouched():
    W, H = 16, 12
    lib = youth_map.load_library()
    K = youth_icp.Intrinsics(*K_RAND)
    with youth_map.VoxelMap(100.0, slots=1024) as m:
        m.integrate(*_frame(W, H, 3), K)
        d_V = torch.from_numpy(np.eye(4, dtype=np.float32)[:3].reshape(1, 12).copy()).cuda()
        d_d = torch.full((W * H,), 0x5a5a, dtype=torch.int16, device="cuda")
        d_c = torch.full((W * H * 3,), 0x5a, dtype=torch.uint8, device="cuda")
        h_d = np.full((H, W), 0x5a5a, np.int16)
        h_c = np.full((H, W, 3), 0x5a, np.uint8)
        torch.cuda.synchronize()
        before = m.extract()
        nan_K = youth_icp.Intrinsics(float("nan"), 523.5, 81.25, 59.5, 5000.0)
        zero_K = youth_icp.Intrinsics(525.0, 523.5, 81.25, 59.5, 0.0)
        bad = [dict(n=0), dict(n=-1), dict(n=65536), dict(W=0), dict(H=0), dict(W=16385),
               dict(H=16385), dict(W=16384, H=8192), dict(max_splat=17), dict(max_splat=-1),
               dict(K=nan_K), dict(K=zero_K), dict(d_V=0), dict(d_depth=0), dict(view=None)]
        for case in bad:
            a = dict(n=1, W=W, H=H, max_splat=0, min_count=0, K=K, d_V=d_V.data_ptr(),
                     d_depth=d_d.data_ptr(), view=True)
            a.update(case)
            view = youth_map.MapView(a["W"], a["H"], a["max_splat"], a["min_count"])
            rc = lib.youth_map_render_device(m._map, a["n"], ctypes.byref(view) if a["view"] else None,
                                             ctypes.byref(a["K"]), a["d_V"] or None,
                                             a["d_depth"] or None, d_c.data_ptr(), None)
            assert rc == youth_icp.YOUTH_EINVAL, case
            assert b"youth_map_render_device" in lib.youth_map_last_error(), case
            if not {"d_V", "d_depth", "n", "view"} & set(case) and a["W"] * a["H"] < 1 << 24:
                with pytest.raises(youth_icp.IcpError) as e:
                    m.render(None, a["W"], a["H"], a["K"], a["max_splat"])
                assert e.value.code == youth_icp.YOUTH_EINVAL and "render_host" in str(e.value)
        badT = np.eye(4)
        badT[0, 3] = np.nan
        with pytest.raises(youth_icp.IcpError) as e:
            m.render(badT, W, H, K)
        assert e.value.code == youth_icp.YOUTH_EINVAL
        p16, p8 = ctypes.POINTER(ctypes.c_int16), ctypes.POINTER(ctypes.c_uint8)
        view = youth_map.MapView(W, H, 17, 0)
        assert lib.youth_map_render_host(m._map, ctypes.byref(view), None, None,
                                         h_d.ctypes.data_as(p16), h_c.ctypes.data_as(p8)) == \
            youth_icp.YOUTH_EINVAL
        view = youth_map.MapView(W, H, 0, 0)
        assert lib.youth_map_render_host(m._map, ctypes.byref(view), None, None, None,
                                         h_c.ctypes.data_as(p8)) == youth_icp.YOUTH_EINVAL
        m.sync()
        torch.cuda.synchronize()
        assert (d_d.cpu().numpy() == 0x5a5a).all() and (d_c.cpu().numpy() == 0x5a).all()
        assert (h_d == 0x5a5a).all() and (h_c == 0x5a).all()
        assert m.extract().tobytes() == before.tobytes()
        # and the map still renders
        V = view_from_pose(np.eye(4))
        _same(_render_device(m, [V], W, H, K)[0], render(before, 100.0, V, K, W, H))


# ------------------------------------------------------ 8 the synthetic scene --
def test_synthetic_scene_on_the_gpu():
    """The case of test_render.py through the kernels: equality with the truth,
    so the same bounds hold."""
    used, K, T4, clean = scene_case()
    with youth_map.VoxelMap(100.0, slots=1 << 18) as m:
        for d, _, _, T in used:
            m.integrate(d, None, K, T)
        rec = m.extract()
        got = m.render(T4, 160, 120, K)
    _same(got, render(rec, 100.0, view_from_pose(T4), K, 160, 120))
    fig = scene_figures(got[0], clean)
    assert fig["coverage"] >= 0.98 and fig["ghost"] <= 0.005
    assert fig["median"] <= 2 and fig["p90"] <= 5


# ---------------------------------------------------------------- 9 drop-in --
_SLAM_CHILD = r"""
import json, sys
import numpy as np
import youth_icp, youth_map, youth_synth
out = sys.argv[1]
K = youth_icp.Intrinsics(142.575, 142.575, 80.0, 60.0, 1000.0)
frames, _ = youth_synth.sequence(0, 4, 160, 120, K)
youth_icp.initSlamModule(None)
assert youth_icp.isSlamModuleRunning() == 1
res = {}
try:
    before = youth_map.slam_map_render(160, 120)          # no pose recorded yet
    vpm = youth_map.slam_map_vpm()
    for k in range(4):
        assert youth_icp.processSlamFrame(frames[k], None, 160, 120, k) == 1
        assert youth_icp.slam_wait_idle(20000) == 1
    ts, T = youth_icp.slam_trajectory()
    vox = youth_map.slam_map_extract()
    last = youth_map.slam_map_render(160, 120)
    first = youth_map.slam_map_render(160, 120, T_world=T[0], want_rgb=False)
finally:
    youth_icp.stopSlamModule()
info = {"before": before is None, "last": last is not None, "first": first is not None,
        "vpm": vpm, "after_stop": youth_map.slam_map_render(160, 120) is None}
if last is not None:
    res.update(d_last=last[0], c_last=last[1], d_first=first[0])
np.savez(out, ts=ts, T=T, vox=vox, **res)
print("RESULT " + json.dumps(info))
"""


def _slam_child(tmp_path, name, extra_env):
    out = tmp_path / (name + ".npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("YOUTH_SLAM_MAP_")}
    env.update(extra_env, PYTHONPATH=os.pathsep.join([PKG, ORACLE] + [p for p in sys.path if p]))
    r = subprocess.run([sys.executable, "-c", _SLAM_CHILD, str(out)], env=env, timeout=120,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):]), np.load(out, allow_pickle=False)


def test_slam_module_map_render_drop_in(tmp_path):
    """With YOUTH_SLAM_MAP_VPM: slam_map_render() at the last recorded pose ==
    the truth render of slam_map_extract() at slam_trajectory()'s last pose, with
    the intrinsics the module tracks the frames with; an explicit pose likewise.
    Without it: 0, the outputs left alone."""
    on, res = _slam_child(tmp_path, "on", {"YOUTH_SLAM_MAP_VPM": "100"})
    assert on == {"before": True, "last": True, "first": True, "vpm": 100.0, "after_stop": True}
    T = res["T"]
    assert len(res["ts"]) == 4
    K = youth_icp.default_intrinsics(160, 120)
    want = render(res["vox"], 100.0, view_from_pose(T[-1]), K, 160, 120)
    assert (want[0] > 0).sum() > 160 * 120 // 2
    _same((res["d_last"], res["c_last"]), want)
    assert (res["c_last"] == 0).all()                    # the module's map is colourless
    _same((res["d_first"], None), (render(res["vox"], 100.0, view_from_pose(T[0]), K, 160, 120)[0],
                                   None))
    off, res_off = _slam_child(tmp_path, "off", {})
    assert off == {"before": True, "last": False, "first": False, "vpm": 0.0, "after_stop": True}
    assert np.array_equal(res_off["T"], T)
    lib = youth_map.load_library()                       # no map here either: outputs left alone
    view = youth_map.MapView(16, 12, 0, 0)
    h_d = np.full((12, 16), 0x5a5a, np.int16)
    h_c = np.full((12, 16, 3), 0x5a, np.uint8)
    assert lib.youth_slam_map_render(ctypes.byref(view), None, None,
                                     h_d.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                                     h_c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) == 0
    assert (h_d == 0x5a5a).all() and (h_c == 0x5a).all()
