"""GPU parity of the voxel map (include/youth_map.h): the HIP
integration against the numpy restatement of the map's definition
(map_truth.py; world points from the C oracle's viewer list).  The map is
specified in integers, so every comparison is exact equality of the sorted
40-byte records unless a test says otherwise; nothing is tolerance-based.  Every
case runs the kernel's real launch geometry (2048-pixel tiles, the 1024-slot
LDS table): no test-only tile size exists."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import youth_icp
import youth_map
from conftest import GOLDEN, ORACLE, PKG
from map_truth import frame_points, restate, restate_frames

pytestmark = pytest.mark.gpu


def _frame(W, H, seed, holes=0.1, negative=True):
    """The recipe of test_gpu_viewer.py: random depth with holes and negatives."""
    rng = np.random.default_rng(seed)
    lo = -500 if negative else 0
    depth = rng.integers(lo, 32768, size=(H, W)).astype(np.int16)
    depth[rng.random((H, W)) < holes] = 0
    rgb = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    return depth, rgb


def _pose(rng, big=False):
    """A random camera -> world pose, row-major 3x4 fp32 (test_gpu_viewer.py)."""
    w = rng.normal(size=3) * (1.0 if big else 0.05)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / max(th, 1e-12)
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.normal(size=3) * (5.0 if big else 0.1)
    return np.hstack([R, t[:, None]]).astype(np.float32)


def _same(got, want):
    assert got.dtype == want.dtype == youth_map.VOXEL_DTYPE
    assert got.shape == want.shape, (got.shape, want.shape)
    assert got.tobytes() == want.tobytes()


def _key(rec):
    return ((rec["iz"].astype(np.int64) + (1 << 20)) << 42) | \
           ((rec["iy"].astype(np.int64) + (1 << 20)) << 21) | (rec["ix"].astype(np.int64) + (1 << 20))


# --------------------------------------------------------------- 1 one frame --
def test_one_frame_identity_pose_colour():
    depth, rgb = _frame(97, 53, 97 * 7 + 53)
    want, oor = restate(*frame_points(depth, rgb), 100.0)
    with youth_map.VoxelMap(100.0) as m:
        m.integrate(depth, rgb)
        got, st = m.extract(), m.stats()
    _same(got, want)
    assert oor == 0 and st["out_of_range"] == 0 and st["dropped"] == 0
    assert st["occupied"] == want.shape[0] and st["integrated"] == int((depth > 0).sum())
    assert st["capacity"] == 1 << 20


def test_host_staging_and_extract_buffer_grow_and_are_reused():
    """youth_map_integrate_host's depth and colour staging grow separately (4x3
    depth only, then 9x7 with colour) and a smaller frame reuses the larger
    buffers (4x3 with colour); youth_map_extract's record buffer grows between
    the two extracts."""
    frames = [(_frame(4, 3, 1)[0], None, None, None), _frame(9, 7, 2) + (None, None),
              _frame(4, 3, 3) + (None, None)]
    with youth_map.VoxelMap(100.0, slots=4096) as m:
        m.integrate(frames[0][0])
        first = m.extract()
        m.integrate(*frames[1][:2])
        second = m.extract()
        m.integrate(*frames[2][:2])
        third, st = m.extract(), m.stats()
    for got, k in ((first, 1), (second, 2), (third, 3)):
        _same(got, restate_frames(frames[:k], 100.0)[0])
    assert 0 < first.shape[0] < second.shape[0] < third.shape[0]
    assert st["dropped"] == 0 and st["out_of_range"] == 0


# -------------------------------------------- 2 many frames, every octant --
def _device_batch(frames, offset=0):
    n, (H, W) = len(frames), frames[0][0].shape
    d_all = torch.zeros(n * H * W + offset, dtype=torch.int16, device="cuda")
    c_all = torch.zeros(n * H * W * 3 + offset, dtype=torch.uint8, device="cuda")
    d_all[offset:] = torch.from_numpy(np.stack([f[0] for f in frames]).reshape(-1)).cuda()
    c_all[offset:] = torch.from_numpy(np.stack([f[1] for f in frames]).reshape(-1)).cuda()
    return d_all, c_all


def test_many_frames_any_split_any_order():
    """The determinism contract: one call of 4 frames == four calls of 1 frame
    == the frames in reverse order == the restatement."""
    W, H, n, vpm = 160, 120, 4, 100.0
    rng = np.random.default_rng(5)
    frames = [_frame(W, H, 200 + f) for f in range(n)]
    T = np.stack([_pose(rng, big=f % 2 == 1) for f in range(n)])
    K = youth_icp.Intrinsics(525.0, 523.5, 81.25, 59.5, 5000.0)
    want, oor = restate_frames([(d, c, K, T[f]) for f, (d, c) in enumerate(frames)], vpm)
    cells = np.stack([want["ix"], want["iy"], want["iz"]], 1)
    assert oor == 0 and len({tuple(s) for s in (cells >= 0)}) == 8      # every octant
    d_all, c_all = _device_batch(frames)
    d_T = torch.from_numpy(T.reshape(n, 12)).cuda()
    rev = list(range(n))[::-1]
    d_rev, c_rev = _device_batch([frames[f] for f in rev])
    d_Trev = torch.from_numpy(np.ascontiguousarray(T[rev]).reshape(n, 12)).cuda()
    torch.cuda.synchronize()
    runs = []
    with youth_map.VoxelMap(vpm) as m:
        m.integrate_device(d_all.data_ptr(), c_all.data_ptr(), n, W, H, d_T.data_ptr(), K)
        runs.append(m.extract())
        m.clear()
        for f in range(n):
            m.integrate_device(d_all.data_ptr() + f * W * H * 2, c_all.data_ptr() + f * W * H * 3,
                               1, W, H, d_T.data_ptr() + f * 48, K)
        runs.append(m.extract())
        m.clear()
        m.integrate_device(d_rev.data_ptr(), c_rev.data_ptr(), n, W, H, d_Trev.data_ptr(), K)
        runs.append(m.extract())
        assert m.stats()["dropped"] == 0
    for got in runs:
        _same(got, want)


# ------------------------------------------------------------ 3 contention --
def test_contention_wall_in_few_voxels():
    W, H, vpm = 320, 240, 4.0
    depth = np.full((H, W), 2000, np.int16)
    rgb = np.random.default_rng(1).integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    want, _ = restate(*frame_points(depth, rgb), vpm)
    assert want.shape[0] <= 64 and want["count"].max() >= 2000
    with youth_map.VoxelMap(vpm, slots=4096) as m:
        m.integrate(depth, rgb)
        m.integrate(depth, rgb)
        got = m.extract()
    twice = want.copy()
    for name in ("count", "sum_q", "sum_c"):
        twice[name] = want[name] * 2
    _same(got, twice)
    assert int(got["count"].sum()) == 2 * W * H


# ---------------------------------------------------------- 4 LDS overflow --
def test_lds_overflow_takes_the_direct_path(monkeypatch):
    """Almost every pixel its own voxel: a tile's 1024-slot LDS table fills and
    the rest goes straight to the global table; YOUTH_MAP_LDS=0 (read at
    create) sends everything there.  Both are exact and identical."""
    W, H, vpm = 320, 240, 1000.0
    depth, rgb = _frame(W, H, 41)
    want, oor = restate(*frame_points(depth, rgb), vpm)
    valid = int((depth > 0).sum())
    assert oor == 0 and want.shape[0] > W * H // 2
    with youth_map.VoxelMap(vpm) as m:
        m.integrate(depth, rgb)
        got, st = m.extract(), m.stats()
    _same(got, want)
    assert 0 < st["direct"] < valid and st["dropped"] == 0 and st["integrated"] == valid
    monkeypatch.setenv("YOUTH_MAP_LDS", "0")
    with youth_map.VoxelMap(vpm) as m:
        m.integrate(depth, rgb)
        got0, st0 = m.extract(), m.stats()
    _same(got0, want)
    assert st0["direct"] == valid and st0["integrated"] == valid


# ------------------------------------------------- 5 boundaries and floor --
def test_voxel_faces_and_floor_of_negatives():
    W, H, vpm = 8, 8, 100.0
    depth = np.full((H, W), 1000, np.int16)          # Z = 1.0 -> s = 100.0: on a face
    want, _ = restate(*frame_points(depth), vpm)
    assert (want["iz"] == 100).all() and (want["sum_q"][:, 2] == 0).all()
    # the centre pixel (x = y = 0) moved to (-0.005, -0.005, -0.005): s = -0.5,
    # floor gives -1 where truncation would give 0
    T = np.array([[1, 0, 0, -0.005], [0, 1, 0, -0.005], [0, 0, 1, -1.005]], np.float64)
    want_neg, _ = restate(*frame_points(depth, None, None, T), vpm)
    with youth_map.VoxelMap(vpm, slots=1024) as m:
        m.integrate(depth)
        got = m.extract()
        m.clear()
        m.integrate(depth, T_world=T)
        got_neg = m.extract()
    _same(got, want)
    _same(got_neg, want_neg)
    # Z = -0.005 for every pixel; X = (u - 4) * 0.00175.. - 0.005 is in [-0.01, 0)
    # for u = 2..6 and in [0, 0.01) for u = 7 alone (Y likewise): truncation
    # would put u = 4..6 in cell 0
    def cell(ix, iy, iz):
        r = got_neg[(got_neg["ix"] == ix) & (got_neg["iy"] == iy) & (got_neg["iz"] == iz)]
        return int(r["count"][0]) if r.shape[0] else 0
    assert (got_neg["iz"] == -1).all()
    assert cell(-1, -1, -1) == 25 and cell(0, 0, -1) == 1 and cell(0, -1, -1) == 5


# --------------------------------------------------- 6 ragged and misaligned --
@pytest.mark.parametrize("W,H", [(5, 7), (1, 1), (1, 300), (2049, 3)])
def test_ragged_and_narrow_frames(W, H):
    depth, rgb = _frame(W, H, W * 7 + H)
    depth[0, 0] = 1234                                   # 1x1: a contributing pixel
    T = _pose(np.random.default_rng(W + H))
    with youth_map.VoxelMap(100.0, slots=1 << 14) as m:
        m.integrate(depth, rgb, T_world=T)
        got = m.extract()
        m.clear()
        m.integrate(depth, None, T_world=T)
        got_nc = m.extract()
    _same(got, restate(*frame_points(depth, rgb, None, T), 100.0)[0])
    _same(got_nc, restate(*frame_points(depth, None, None, T), 100.0)[0])


@pytest.mark.parametrize("offset", [0, 1])
def test_device_pointers_offset_by_one_element(offset):
    """offset 1 misaligns depth and colour (the scalar-load path); offset 0 runs
    the 16-byte loads.  On a torch stream."""
    W, H, n, vpm = 64, 48, 3, 100.0
    rng = np.random.default_rng(9)
    frames = [_frame(W, H, 300 + f) for f in range(n)]
    T = np.stack([_pose(rng) for _ in range(n)])
    d_all, c_all = _device_batch(frames, offset)
    d_T = torch.from_numpy(T.reshape(n, 12)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    with youth_map.VoxelMap(vpm, slots=1 << 16) as m:
        torch.cuda.synchronize()
        m.sync()                                         # the create-time clear, before our stream
        m.integrate_device(d_all.data_ptr() + offset * 2, c_all.data_ptr() + offset, n, W, H,
                           d_T.data_ptr(), stream=stream)
        m.sync(stream)
        got = m.extract()
    _same(got, restate_frames([(d, c, None, T[f]) for f, (d, c) in enumerate(frames)], vpm)[0])


# ----------------------------------------------------------- 7 out of range --
def test_out_of_range_points_are_skipped_and_counted():
    depth, rgb = _frame(97, 53, 12)
    T = np.array([[1, 0, 0, 3000.0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float64)
    want, oor = restate(*frame_points(depth, rgb, None, T), 1000.0)
    valid = int((depth > 0).sum())
    assert want.shape[0] == 0 and oor == valid
    with youth_map.VoxelMap(1000.0, slots=1024) as m:
        m.integrate(depth, rgb, T_world=T)
        st = m.stats()
        assert m.voxels() == 0 and m.extract().shape == (0,)
    assert st["out_of_range"] == valid and st["integrated"] == 0 and st["dropped"] == 0


# ------------------------------------------------------------- 8 full table --
def test_full_table_drops_and_counts():
    W, H, vpm = 160, 120, 1000.0
    depth, rgb = _frame(W, H, 77)
    want, _ = restate(*frame_points(depth, rgb), vpm)
    assert want.shape[0] > 4096
    valid = int((depth > 0).sum())
    with youth_map.VoxelMap(vpm, slots=1024) as m:
        m.integrate(depth, rgb)                          # returns: probing is bounded
        got, st = m.extract(), m.stats()
        assert m.voxels() == got.shape[0]
    assert st["capacity"] == 1024 and 0 < got.shape[0] <= 1024
    kg, kw = _key(got), _key(want)
    assert np.unique(kg).shape[0] == kg.shape[0] and (np.diff(kg) > 0).all()   # unique, sorted
    at = np.searchsorted(kw, kg)
    assert (at < kw.shape[0]).all() and (kw[np.minimum(at, kw.shape[0] - 1)] == kg).all()
    sub = want[at]
    assert (got["count"] >= 1).all() and (got["count"] <= sub["count"]).all()
    assert (got["sum_q"] <= sub["sum_q"]).all() and (got["sum_c"] <= sub["sum_c"]).all()
    assert st["dropped"] > 0 and st["dropped"] + int(got["count"].sum()) == valid
    assert st["integrated"] == int(got["count"].sum())


# -------------------------------------------------------------- 9 lifecycle --
def test_lifecycle_clear_gate_and_rejections():
    W, H, vpm = 97, 53, 100.0
    rng = np.random.default_rng(2)
    frames = [_frame(W, H, 500 + f) for f in range(3)]
    T = [_pose(rng) for _ in range(3)]
    lib = youth_map.load_library()
    with youth_map.VoxelMap(vpm) as m:
        m.integrate(frames[0][0], frames[0][1], T_world=T[0])
        _same(m.extract(), restate_frames([(*frames[0], None, T[0])], vpm)[0])
        for f in (1, 2):                                 # integration continues after extract
            m.integrate(frames[f][0], frames[f][1], T_world=T[f])
        allf = restate_frames([(*frames[f], None, T[f]) for f in range(3)], vpm)[0]
        _same(m.extract(), allf)
        n = m.voxels()
        buf = np.zeros(n, youth_map.VOXEL_DTYPE)
        assert lib.youth_map_extract(m._map, buf.ctypes.data, n - 1) == youth_icp.YOUTH_EINVAL
        assert lib.youth_map_extract(m._map, buf.ctypes.data, n) == n      # still whole
        _same(buf, allf)
        m.clear()
        assert m.voxels() == 0 and m.extract().shape == (0,)
        assert all(v == 0 for k, v in m.stats().items() if k != "capacity")
        m.set_max_depth(9000)
        m.integrate(frames[0][0], frames[0][1], T_world=T[0])
        gated, _ = restate(*frame_points(frames[0][0], frames[0][1], None, T[0], max_depth=9000),
                           vpm)
        _same(m.extract(), gated)
        assert m.stats()["integrated"] == int(((frames[0][0] > 0) & (frames[0][0] <= 9000)).sum())
        m.set_max_depth(0)
        before = m.extract()
        bad = np.eye(4)
        bad[1, 2] = np.nan
        with pytest.raises(youth_icp.IcpError) as e:
            m.integrate(frames[0][0], T_world=bad)
        assert e.value.code == youth_icp.YOUTH_EINVAL
        bad[1, 2] = np.inf
        with pytest.raises(youth_icp.IcpError):
            m.integrate(frames[0][0], T_world=bad)
        with pytest.raises(youth_icp.IcpError) as e:
            m.integrate_device(0, 0, 1, W, H)            # null device pointers
        assert e.value.code == youth_icp.YOUTH_EINVAL
        with pytest.raises(youth_icp.IcpError):
            m.integrate_device(1 << 20, 0, 1, 0, H)      # refused before any launch
        with pytest.raises(youth_icp.IcpError):
            m.set_max_depth(-1)
        _same(m.extract(), before)                       # the refused calls changed nothing


# ---------------------------------------------------------------- 10 drop-in --
_CHILD = r"""
import json, os, sys
import numpy as np
import youth_icp, youth_map
out, golden = sys.argv[1], sys.argv[2]
frames = np.load(golden, allow_pickle=False)["frames"]
n, H, W = frames.shape
youth_icp.initSlamModule(None)
assert youth_icp.isSlamModuleRunning() == 1
try:
    for k in range(n):
        assert youth_icp.processSlamFrame(frames[k], None, W, H, k) == 1
        assert youth_icp.slam_wait_idle(20000) == 1
    ts, T = youth_icp.slam_trajectory()
    res = {"voxels": youth_map.slam_map_voxels(), "vpm": youth_map.slam_map_vpm()}
    vox = youth_map.slam_map_extract()
    assert youth_icp.saveSlamMap(os.path.join(out, "map")) == 1
    youth_icp.resetSlam()
    res["after_reset"] = youth_map.slam_map_voxels()
    assert youth_icp.processSlamFrame(frames[0], None, W, H, 99) == 1
    assert youth_icp.slam_wait_idle(20000) == 1
    res["after_restart"] = youth_map.slam_map_voxels()
finally:
    youth_icp.stopSlamModule()
res["after_stop"] = youth_map.slam_map_voxels()
np.savez(os.path.join(out, "res.npz"), ts=ts, T=T, vox=vox)
print("RESULT " + json.dumps(res))
"""


def _run_child(tmp_path, name, extra_env):
    out = tmp_path / name
    out.mkdir()
    env = {k: v for k, v in os.environ.items() if not k.startswith("YOUTH_SLAM_MAP_")}
    env.update(extra_env, PYTHONPATH=os.pathsep.join([PKG, ORACLE] + [p for p in sys.path if p]))
    r = subprocess.run([sys.executable, "-c", _CHILD, str(out),
                        os.path.join(GOLDEN, "seq_128x96.npz")], env=env, timeout=120,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return out, json.loads(line[len("RESULT "):]), np.load(out / "res.npz", allow_pickle=False)


def test_slam_module_map_drop_in(tmp_path):
    """The module reads YOUTH_SLAM_MAP_VPM at init, so each setting runs in a
    fresh child process.  With it: the module's map == the restatement of the
    recorded frames under the recorded poses (first 12 entries rounded to fp32),
    saveSlamMap adds _map.ply, resetSlam empties the map.  Without it: no map,
    no _map.ply, and the same trajectory file."""
    frames = np.load(os.path.join(GOLDEN, "seq_128x96.npz"), allow_pickle=False)["frames"]
    H, W = frames.shape[1:]
    on_dir, on, res = _run_child(tmp_path, "on", {"YOUTH_SLAM_MAP_VPM": "100"})
    off_dir, off, res_off = _run_child(tmp_path, "off", {})
    K = youth_icp.default_intrinsics(W, H)
    ts, T = res["ts"], res["T"]
    assert len(ts) >= 2 and on["vpm"] == 100.0
    want, oor = restate_frames(
        [(frames[int(t)], None, K, T[k].reshape(-1)[:12].astype(np.float32).reshape(3, 4))
         for k, t in enumerate(ts)], 100.0)
    assert oor == 0
    _same(res["vox"], want)
    assert on["voxels"] == want.shape[0] and (res["vox"]["sum_c"] == 0).all()   # colourless
    ply = (on_dir / "map_map.ply").read_text().splitlines()
    assert f"element vertex {want.shape[0]}" in ply
    assert len(ply) - (ply.index("end_header") + 1) == want.shape[0]
    assert on["after_reset"] == 0 and on["after_stop"] == 0
    first, _ = restate(*frame_points(frames[0], None, K), 100.0)
    assert on["after_restart"] == first.shape[0]         # the new sequence's origin frame only
    # without the variable: byte-identical trajectory, no map
    assert np.array_equal(res_off["T"], T) and np.array_equal(res_off["ts"], ts)
    assert (off_dir / "map_trajectory.txt").read_bytes() == (on_dir / "map_trajectory.txt").read_bytes()
    assert (off_dir / "map_keyframes.txt").read_bytes() == (on_dir / "map_keyframes.txt").read_bytes()
    assert not (off_dir / "map_map.ply").exists()
    assert off == {"voxels": 0, "vpm": 0.0, "after_reset": 0, "after_restart": 0, "after_stop": 0}
    assert res_off["vox"].shape == (0,)
