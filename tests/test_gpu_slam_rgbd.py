"""Colour through the SLAM.h drop-in: YOUTH_SLAM_RGBD=1 tracks
with the streaming RGB-D tracker, YOUTH_SLAM_MAP_COLOR=1 carries colour to the
voxel map, and with neither set the module does what it always did.  The module
reads its environment at initSlamModule, so every case runs in a fresh child
process with its own environment."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rgbd_truth
import youth_icp
import youth_map
import youth_rgbd
import youth_synth
from conftest import ORACLE, PKG

pytestmark = pytest.mark.gpu

_CHILD = r"""
import json, os, sys
import numpy as np
import youth_icp, youth_map, youth_synth
out, plan = sys.argv[1], json.loads(sys.argv[2])
W, H, n = plan["W"], plan["H"], plan["n"]
K = youth_icp.Intrinsics(*plan["K"]) if plan.get("K") else None
fr, _, rgb = youth_synth.sequence_rgb(0, n, W, H, K=K)
res = {}
youth_icp.initSlamModule(plan.get("config"))
assert youth_icp.isSlamModuleRunning() == 1
try:
    res["active"] = youth_icp.slam_rgbd_active()
    for k in range(n):
        if k == plan.get("reset_before", -1):
            assert youth_icp.slam_wait_idle(20000) == 1
            res["len_before_reset"] = youth_icp.slam_trajectory()[1].shape[0]
            youth_icp.resetSlam()
        c = rgb[k] if plan["color"] else None
        assert youth_icp.processSlamFrame(fr[k], c, W, H, k) == 1
        if not plan["backlog"]:
            assert youth_icp.slam_wait_idle(20000) == 1
    assert youth_icp.slam_wait_idle(20000) == 1
    ts, T = youth_icp.slam_trajectory()
    res["batched"] = youth_icp.slam_batched_frames()
    res["points"] = youth_icp.getSlamMapPoints()
    if plan.get("refuse_none"):
        res["none_push"] = youth_icp.processSlamFrame(fr[0], None, W, H, 77)
        assert youth_icp.slam_wait_idle(20000) == 1
        res["len_after_none"] = youth_icp.slam_trajectory()[1].shape[0]
    if plan.get("then_small"):
        fs, _, cs = youth_synth.sequence_rgb(0, 3, 160, 120)
        for k in range(3):
            assert youth_icp.processSlamFrame(fs[k], cs[k], 160, 120, 100 + k) == 1
        assert youth_icp.slam_wait_idle(20000) == 1
        ts2, T2 = youth_icp.slam_trajectory()
        np.savez(os.path.join(out, "small.npz"), ts=ts2, T=T2)
    vox = youth_map.slam_map_extract()
    assert youth_icp.saveSlamMap(os.path.join(out, "map")) == 1
finally:
    youth_icp.stopSlamModule()
res["active_after_stop"] = youth_icp.slam_rgbd_active()
np.savez(os.path.join(out, "res.npz"), ts=ts, T=T, vox=vox)
print("RESULT " + json.dumps(res))
"""


def _run_child(tmp_path, name, env_extra, **plan):
    out = tmp_path / name
    out.mkdir()
    plan = dict({"W": 640, "H": 480, "n": 8, "color": True, "backlog": True}, **plan)
    env = {k: v for k, v in os.environ.items()
           if not k.startswith(("YOUTH_SLAM_", "YOUTH_ICP_DEPTH_FILTER", "YOUTH_RGBD_"))}
    env.update(env_extra, PYTHONPATH=os.pathsep.join([PKG, ORACLE] + [p for p in sys.path if p]))
    r = subprocess.run([sys.executable, "-c", _CHILD, str(out), json.dumps(plan)], env=env,
                       timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return out, json.loads(line[len("RESULT "):]), np.load(out / "res.npz", allow_pickle=False)


@pytest.fixture(scope="module")
def seq8():
    """Frames 0-7 of the 640x480 sequence, their true poses and the composed
    poses of the sequence align (youth_rgbd_track_host_sequence)."""
    fr, Twc, rgb = youth_synth.sequence_rgb(0, 8)
    with youth_rgbd.RgbdContext(640, 480, 8) as ctx:
        T_rel, st = ctx.track_host_sequence(fr, rgb)
    assert not st.any()
    T_rel[:, 3, :] = (0.0, 0.0, 0.0, 1.0)
    traj = [np.eye(4)]
    for k in range(7):
        traj.append(traj[-1] @ T_rel[k])
    return fr, Twc, rgb, np.array(traj)


def _mat_mul4(A, B):
    """The worker's composition (slam_api.cpp mat_mul4): plain fp64 products
    summed in k order, which a BLAS matmul does not promise."""
    C = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += float(A[i, k]) * float(B[k, j])
            C[i, j] = s
    return C


def _frame7_error(T, Twc):
    return rgbd_truth.pose_error(T[7].reshape(4, 4), np.linalg.inv(Twc[0]) @ Twc[7])


# --------------------------------------------------------------- RGB-D mode --
def test_rgbd_mode_tracks_with_colour(tmp_path, seq8):
    _, Twc, _, want = seq8
    _, info, res = _run_child(tmp_path, "backlog", {"YOUTH_SLAM_RGBD": "1"})
    assert info["active"] == 1 and info["active_after_stop"] == 0
    assert res["ts"].tolist() == list(range(8)) and info["points"] > 0
    T = res["T"].reshape(-1, 4, 4)
    print("max |T - composed sequence align|:", np.abs(T - want).max())
    assert np.abs(T - want).max() <= 1e-9
    e7 = _frame7_error(T, Twc)
    print(f"frame 7: {e7[0]:.4f} deg / {e7[1]:.3f} mm, batched frames {info['batched']}")
    assert e7[0] <= rgbd_truth.BOUND_FRAME_7[0] and e7[1] <= rgbd_truth.BOUND_FRAME_7[1]
    # a live camera: one frame at a time, the worker idle in between
    _, live, res1 = _run_child(tmp_path, "live", {"YOUTH_SLAM_RGBD": "1"}, backlog=False)
    assert live["active"] == 1 and live["batched"] == 0
    assert np.array_equal(res1["T"], res["T"]) and np.array_equal(res1["ts"], res["ts"])


def test_rgbd_mode_tracks_with_the_camera_of_the_config_file(tmp_path):
    """initSlamModule with a camera file whose fx != fy: the worker hands that
    camera to its RGB-D tracker (slam_api.cpp intrinsics_for ->
    youth_rgbd_create), so the trajectory is the composed track of a context
    made with it, bit for bit, and not the one the viewer's camera gives."""
    W, H, n = 160, 120, 4
    k = tuple(float(np.float32(v)) for v in (131.7, 197.3, 77.4, 62.6, 1000.0))
    cfg = tmp_path / "camera.yaml"
    cfg.write_text("%YAML:1.0\nCamera.type: \"PinHole\"\n"
                   + "".join(f"Camera.{name}: {v!r}\n" for name, v in zip(("fx", "fy", "cx", "cy"), k))
                   + f"Camera.width: {W}\nCamera.height: {H}\nDepthMapFactor: {k[4]!r}\n")
    K, Wc, Hc = youth_icp.parse_camera_yaml(str(cfg))
    assert (Wc, Hc) == (W, H) and K.as_tuple() == k and K.fx != K.fy
    _, info, res = _run_child(tmp_path, "yaml", {"YOUTH_SLAM_RGBD": "1"}, W=W, H=H, n=n,
                              backlog=False, config=str(cfg), K=list(k))
    assert info["active"] == 1 and res["ts"].tolist() == list(range(n))
    T = res["T"].reshape(-1, 4, 4)
    fr, _, rgb = youth_synth.sequence_rgb(0, n, W, H, K=youth_icp.Intrinsics(*k))
    trajs = []
    for Kc in (youth_icp.Intrinsics(*k), None):
        with youth_rgbd.RgbdContext(W, H, 16, K=Kc) as ctx:
            ctx.track_set_batch(8)
            ctx.track_submit(list(fr), list(rgb))
            traj = [np.eye(4)]
            for f in range(n):
                T_rel, has, st = ctx.track_collect()
                assert st == 0 and has == int(f > 0)
                if has:
                    traj.append(_mat_mul4(traj[-1], T_rel))
        trajs.append(np.array(traj))
    assert np.array_equal(T, trajs[0])
    print("max |T - T under the viewer's camera|:", np.abs(T - trajs[1]).max())
    assert np.abs(T - trajs[1]).max() > 1e-4


# ------------------------------------------------------------- default mode --
def test_default_mode_ignores_colour(tmp_path, seq8):
    _, Twc, _, _ = seq8
    _, with_c, res_c = _run_child(tmp_path, "colour", {})
    _, without, res_n = _run_child(tmp_path, "none", {}, color=False)
    assert with_c["active"] == 0 and without["active"] == 0
    assert res_c["ts"].tolist() == list(range(8))
    assert np.array_equal(res_c["T"], res_n["T"]) and np.array_equal(res_c["ts"], res_n["ts"])
    e7 = _frame7_error(res_c["T"].reshape(-1, 4, 4), Twc)
    print(f"depth-only frame 7: {e7[0]:.3f} deg / {e7[1]:.2f} mm")
    # depth alone slides along the wall: far outside the RGB-D bound, so the
    # bound of test_rgbd_mode_tracks_with_colour discriminates
    assert e7[0] > 10 * rgbd_truth.BOUND_FRAME_7[0] and e7[1] > 10 * rgbd_truth.BOUND_FRAME_7[1]
    assert res_c["vox"].shape == (0,)


# -------------------------------------------------------- reset and refusal --
def test_reset_refusal_and_size_change(tmp_path, seq8):
    fr, _, rgb, _ = seq8
    out, info, res = _run_child(tmp_path, "reset", {"YOUTH_SLAM_RGBD": "1"}, backlog=False,
                                reset_before=4, refuse_none=True, then_small=True)
    assert info["active"] == 1 and info["len_before_reset"] == 4
    # frame 4 is the new origin: the trajectory restarts at the identity
    T = res["T"].reshape(-1, 4, 4)
    assert res["ts"].tolist() == [4, 5, 6, 7] and np.array_equal(T[0], np.eye(4))
    with youth_rgbd.RgbdContext(640, 480, 16) as ctx:
        ctx.track_set_batch(8)
        ctx.track_submit(list(fr[4:8]), list(rgb[4:8]))
        want = np.eye(4)
        for k in range(4):
            T_rel, has, st = ctx.track_collect()
            want = _mat_mul4(want, T_rel) if has else np.eye(4)
            assert st == 0 and np.array_equal(T[k], want), k
    # a push without colour is refused and leaves the trajectory alone
    assert info["none_push"] == 0 and info["len_after_none"] == 4
    # another frame size: the worker drains, makes a new context and goes on
    small = np.load(out / "small.npz", allow_pickle=False)
    assert small["ts"].tolist() == [100, 101, 102]
    assert np.array_equal(small["T"][0].reshape(4, 4), np.eye(4))
    assert not np.array_equal(small["T"][2], small["T"][0])


# -------------------------------------------------------------- coloured map --
@pytest.mark.parametrize("rgbd", [False, True], ids=["depth_tracking", "rgbd_tracking"])
def test_map_carries_colour(tmp_path, rgbd):
    W, H, n = 160, 120, 4
    fr, _, rgb = youth_synth.sequence_rgb(0, n, W, H)
    env = {"YOUTH_SLAM_MAP_VPM": "100", "YOUTH_SLAM_MAP_COLOR": "1"}
    if rgbd:
        env["YOUTH_SLAM_RGBD"] = "1"
    out, info, res = _run_child(tmp_path, "map", env, W=W, H=H, n=n)
    assert info["active"] == int(rgbd) and res["ts"].tolist() == list(range(n))
    K = youth_icp.default_intrinsics(W, H)
    with youth_map.VoxelMap(100.0, 1 << 22) as m:
        for k in range(n):
            m.integrate(fr[k], rgb[k], K, res["T"][k])
        want = m.extract()
    assert want.shape[0] > 0 and np.array_equal(res["vox"], want)
    assert (res["vox"]["sum_c"] != 0).any()
    ply = (out / "map_map.ply").read_text().splitlines()
    body = ply[ply.index("end_header") + 1:]
    assert len(body) == want.shape[0]
    cols = np.array([[int(float(v)) for v in ln.split()[-3:]] for ln in body])
    assert ((cols[:, 0] != cols[:, 1]) | (cols[:, 1] != cols[:, 2])).any()   # not grey


def test_map_without_the_variables_stays_colourless(tmp_path):
    W, H, n = 160, 120, 4
    fr, _, _ = youth_synth.sequence_rgb(0, n, W, H)
    _, info, res = _run_child(tmp_path, "plain", {"YOUTH_SLAM_MAP_VPM": "100"}, W=W, H=H, n=n)
    assert info["active"] == 0
    K = youth_icp.default_intrinsics(W, H)
    with youth_map.VoxelMap(100.0, 1 << 22) as m:
        for k in range(n):
            m.integrate(fr[k], None, K, res["T"][k])
        want = m.extract()
    assert want.shape[0] > 0 and np.array_equal(res["vox"], want)
    assert (res["vox"]["sum_c"] == 0).all()
