"""Re-integration of the SLAM module's voxel map after a loop closure
(include/youth_map.h "the drop-in"): YOUTH_SLAM_MAP_KEEP makes
the module keep its integrated frames on the device, and
youth_slam_map_reintegrate moves them to a corrected trajectory.  The module
reads its environment at initSlamModule, so each setting runs in a fresh child
process, as in test_gpu_slam_loop.py, whose sequence this is: C5 frames 0-29
followed by frames 628-657 at 160 x 120, tracked with colour, loop closing on.

Every comparison is byte equality: of sorted voxel records against a fresh
VoxelMap fed the same 60 frames with the corrected trajectory, and of files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import youth_icp
import youth_map
import youth_synth
from conftest import ORACLE, PKG

pytestmark = pytest.mark.gpu

W, H = 160, 120
K = (142.575, 142.575, 80.0, 60.0, 1000.0)
PARTS = [(0, 30), (628, 30)]   # (first frame, frames) of C5
VPM = 100.0

_CHILD = r"""
import ctypes, json, os, sys
import numpy as np
import youth_icp, youth_loop, youth_map, youth_synth
out, plan = sys.argv[1], json.loads(sys.argv[2])
W, H = plan["W"], plan["H"]
K = youth_icp.Intrinsics(*plan["K"])
fr, rgb = [], []
for f0, n in plan["parts"]:
    a, _, c = youth_synth.sequence_rgb(f0, n, W, H, K=K)
    fr.extend(a), rgb.extend(c)
youth_icp.initSlamModule(plan["config"])
assert youth_icp.isSlamModuleRunning() == 1
res, arr = {}, {}
try:
    for i in range(len(fr)):
        assert youth_icp.processSlamFrame(fr[i], rgb[i], W, H, 100 + i) == 1
        assert youth_icp.slam_wait_idle(20000) == 1
    ts, T = youth_icp.slam_trajectory()
    closed = youth_loop.slam_loop_trajectory()
    res["kept"] = youth_map.slam_map_kept()
    arr["live"] = youth_map.slam_map_extract()
    if plan["keep"]:
        lib = youth_map.load_library()
        bad = np.ascontiguousarray(closed, np.float64).copy()
        bad[41, 1, 2] = np.nan
        res["bad"] = lib.youth_slam_map_reintegrate(
            bad.shape[0], bad.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        arr["after_bad"] = youth_map.slam_map_extract()
        res["changed"] = youth_map.slam_map_reintegrate(closed)
        arr["moved"] = youth_map.slam_map_extract()
        res["again"] = youth_map.slam_map_reintegrate(closed)
        # back to the live poses: exact, so saveSlamMap below starts from the map it
        # would have had
        res["back"] = youth_map.slam_map_reintegrate(T)
        arr["back"] = youth_map.slam_map_extract()
    assert youth_icp.saveSlamMap(os.path.join(out, "map")) == 1
    arr["saved"] = youth_map.slam_map_extract()
    res["voxels_saved"] = youth_map.slam_map_voxels()
    youth_icp.resetSlam()
    res["kept_after_reset"] = youth_map.slam_map_kept()
finally:
    youth_icp.stopSlamModule()
res["kept_after_stop"] = youth_map.slam_map_kept()
np.savez(os.path.join(out, "res.npz"), ts=ts, T=T, closed=closed, **arr)
print("RESULT " + json.dumps(res))
"""


def _run_child(tmp, name, env_extra, keep):
    out = tmp / name
    out.mkdir()
    cfg = tmp / (name + "_camera.yaml")
    cfg.write_text("%YAML:1.0\nCamera.type: \"PinHole\"\n"
                   + "".join(f"Camera.{n}: {float(np.float32(v))!r}\n" for n, v in zip(("fx", "fy", "cx", "cy"), K))
                   + f"Camera.width: {W}\nCamera.height: {H}\nDepthMapFactor: {K[4]!r}\n")
    plan = {"W": W, "H": H, "K": [float(np.float32(v)) for v in K], "parts": PARTS,
            "config": str(cfg), "keep": keep}
    env = {k: v for k, v in os.environ.items()
           if not k.startswith(("YOUTH_SLAM_", "YOUTH_ICP_DEPTH_FILTER", "YOUTH_RGBD_", "YOUTH_MAP_"))}
    env.update(env_extra, PYTHONPATH=os.pathsep.join([PKG, ORACLE] + [p for p in sys.path if p]))
    r = subprocess.run([sys.executable, "-c", _CHILD, str(out), json.dumps(plan)], env=env, timeout=120,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return out, json.loads(line[len("RESULT "):]), np.load(out / "res.npz", allow_pickle=False), r.stderr


def _fresh_map(T):
    """A fresh VoxelMap fed the 60 frames with the poses T [60, 4, 4]."""
    Ki = youth_icp.Intrinsics(*[float(np.float32(v)) for v in K])
    with youth_map.VoxelMap(VPM, slots=1 << 22) as m:
        i = 0
        for f0, n in PARTS:
            depth, _, rgb = youth_synth.sequence_rgb(f0, n, W, H, K=Ki)
            for k in range(n):
                m.integrate(depth[k], rgb[k], Ki, T[i])
                i += 1
        assert m.stats()["dropped"] == 0
        return m.extract()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("slam_map_reintegrate")
    env = {"YOUTH_SLAM_RGBD": "1", "YOUTH_SLAM_LOOP": "1", "YOUTH_SLAM_LOOP_KF_M": "0.045",
           "YOUTH_SLAM_LOOP_KF_DEG": "90", "YOUTH_SLAM_LOOP_MIN_GAP": "2", "YOUTH_SLAM_MAP_VPM": "100"}
    keep = _run_child(tmp, "keep", dict(env, YOUTH_SLAM_MAP_KEEP="64"), True)
    plain = _run_child(tmp, "plain", env, False)
    res = keep[2]
    return keep, plain, _fresh_map(res["T"]), _fresh_map(res["closed"])


def _same(got, want):
    assert got.dtype == want.dtype == youth_map.VOXEL_DTYPE
    assert got.shape == want.shape, (got.shape, want.shape)
    assert got.tobytes() == want.tobytes()


def test_kept_frames_move_to_the_corrected_trajectory(runs):
    (out, info, res, log), _, fresh_live, fresh_closed = runs
    assert "keeps up to 64 frames" in log
    assert info["kept"] == 60 and res["closed"].shape == (60, 4, 4)
    assert info["kept_after_reset"] == 0 and info["kept_after_stop"] == 0
    _same(res["live"], fresh_live)
    assert (res["live"]["sum_c"] != 0).any()             # tracked with colour: a coloured map
    assert info["changed"] >= 1 and info["again"] == 0 and info["back"] == info["changed"]
    changed = sum(not np.array_equal(a.reshape(-1)[:12].astype(np.float32),
                                     b.reshape(-1)[:12].astype(np.float32))
                  for a, b in zip(res["T"], res["closed"]))
    assert info["changed"] == changed
    _same(res["moved"], fresh_closed)
    assert res["moved"].tobytes() != res["live"].tobytes()
    _same(res["back"], fresh_live)                       # and back again: removal is exact


def test_a_non_finite_pose_is_refused_and_changes_nothing(runs):
    (_, info, res, _), _, fresh_live, _ = runs
    assert info["bad"] == youth_icp.YOUTH_EINVAL
    _same(res["after_bad"], fresh_live)


def test_save_writes_the_closed_map_beside_the_live_one(runs, tmp_path):
    (out, info, res, _), (plain, _, _, _), fresh_live, fresh_closed = runs
    files = sorted(p.name for p in out.iterdir())
    assert files == ["map_keyframes.txt", "map_map.ply", "map_map_closed.ply", "map_trajectory.txt",
                     "map_trajectory_closed.txt", "res.npz"]
    # _map.ply first and unchanged: the live map, as the run without the store writes it
    assert (out / "map_map.ply").read_bytes() == (plain / "map_map.ply").read_bytes()
    want = tmp_path / "closed.ply"
    youth_map.write_ply(str(want), fresh_closed, VPM)
    assert (out / "map_map_closed.ply").read_bytes() == want.read_bytes()
    # the module's map is the re-integrated, compacted one from then on
    _same(res["saved"], fresh_closed)
    assert info["voxels_saved"] == fresh_closed.shape[0]
    # the trajectory files are those of the run without the store
    for name in ("map_trajectory.txt", "map_keyframes.txt", "map_trajectory_closed.txt"):
        assert (out / name).read_bytes() == (plain / name).read_bytes()


def test_without_the_variable_nothing_changes(runs, tmp_path):
    _, (plain, info, res, log), fresh_live, _ = runs
    assert info["kept"] == 0 and info["kept_after_reset"] == 0 and "keeps up to" not in log
    files = sorted(p.name for p in plain.iterdir())
    assert files == ["map_keyframes.txt", "map_map.ply", "map_trajectory.txt",
                     "map_trajectory_closed.txt", "res.npz"]
    _same(res["live"], fresh_live)
    _same(res["saved"], fresh_live)                      # saveSlamMap left the map alone
    assert info["voxels_saved"] == fresh_live.shape[0]
    want = tmp_path / "live.ply"
    youth_map.write_ply(str(want), fresh_live, VPM)
    assert (plain / "map_map.ply").read_bytes() == want.read_bytes()
