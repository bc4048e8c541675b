"""Loop closing through the SLAM.h drop-in: YOUTH_SLAM_LOOP=1
makes the worker keep keyframes and close loops; without it the module does
what it always did.  The module reads its environment at initSlamModule, so
each case runs in a fresh child process.

The sequence is C5 frames 0-29 followed by frames 628-657, 60 frames at
160 x 120 tracked with colour.  The camera of C5 circles with phi = 0.01 k, so
frame k + 628 stands within 17 mm of frame k: the keyframes of the second part
close onto those of the first.  No resetSlam at the jump (a reset empties the
keyframe store): frame 628 is tracked against frame 29 like any other frame,
whatever that gives, and nothing here composes poses across the gap.  The
loop edges do not depend on the trajectory: they are checked against the
ground-truth poses of the two frames they join."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import loop_truth
import youth_synth
from conftest import ORACLE, PKG

pytestmark = pytest.mark.gpu

W, H = 160, 120
K = (142.575, 142.575, 80.0, 60.0, 1000.0)
PARTS = [(0, 30), (628, 30)]   # (first frame, frames) of C5
FRAMES = [f0 + k for f0, n in PARTS for k in range(n)]

_CHILD = r"""
import json, os, sys
import numpy as np
import youth_icp, youth_loop, youth_synth
out, plan = sys.argv[1], json.loads(sys.argv[2])
W, H = plan["W"], plan["H"]
K = youth_icp.Intrinsics(*plan["K"])
fr, rgb = [], []
for f0, n in plan["parts"]:
    a, _, c = youth_synth.sequence_rgb(f0, n, W, H, K=K)
    fr.extend(a), rgb.extend(c)
youth_icp.initSlamModule(plan["config"])
assert youth_icp.isSlamModuleRunning() == 1
try:
    assert youth_icp.slam_rgbd_active() == 1
    for i in range(len(fr)):
        assert youth_icp.processSlamFrame(fr[i], rgb[i], W, H, 100 + i) == 1
        assert youth_icp.slam_wait_idle(20000) == 1
    ts, T = youth_icp.slam_trajectory()
    res = {"keyframes": youth_loop.slam_loop_keyframes()}
    kf_frames = youth_loop.slam_loop_keyframe_frames()
    edges = youth_loop.slam_loop_edges()
    closed = youth_loop.slam_loop_trajectory()
    assert youth_icp.saveSlamMap(os.path.join(out, "map")) == 1
finally:
    youth_icp.stopSlamModule()
res["keyframes_after_stop"] = youth_loop.slam_loop_keyframes()
np.savez(os.path.join(out, "res.npz"), ts=ts, T=T, kf_frames=kf_frames, edges=edges, closed=closed)
print("RESULT " + json.dumps(res))
"""


def _run_child(tmp, name, env_extra):
    out = tmp / name
    out.mkdir()
    cfg = tmp / (name + "_camera.yaml")
    cfg.write_text("%YAML:1.0\nCamera.type: \"PinHole\"\n"
                   + "".join(f"Camera.{n}: {float(np.float32(v))!r}\n" for n, v in zip(("fx", "fy", "cx", "cy"), K))
                   + f"Camera.width: {W}\nCamera.height: {H}\nDepthMapFactor: {K[4]!r}\n")
    plan = {"W": W, "H": H, "K": [float(np.float32(v)) for v in K], "parts": PARTS,
            "config": str(cfg)}
    env = {k: v for k, v in os.environ.items()
           if not k.startswith(("YOUTH_SLAM_", "YOUTH_ICP_DEPTH_FILTER", "YOUTH_RGBD_"))}
    env.update(env_extra, PYTHONPATH=os.pathsep.join([PKG, ORACLE] + [p for p in sys.path if p]))
    r = subprocess.run([sys.executable, "-c", _CHILD, str(out), json.dumps(plan)], env=env, timeout=120,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return out, json.loads(line[len("RESULT "):]), np.load(out / "res.npz", allow_pickle=False), r.stderr


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("slam_loop")
    env = {"YOUTH_SLAM_RGBD": "1"}
    on = _run_child(tmp, "on", dict(env, YOUTH_SLAM_LOOP="1", YOUTH_SLAM_LOOP_KF_M="0.045",
                                    YOUTH_SLAM_LOOP_KF_DEG="90", YOUTH_SLAM_LOOP_MIN_GAP="2"))
    off = _run_child(tmp, "off", env)
    return on, off, np.concatenate([youth_synth.sequence(f0, n, 32, 24)[1] for f0, n in PARTS])


def test_worker_closes_the_second_visit_onto_the_first(runs):
    (out, info, res, log), _, X = runs
    kf = res["kf_frames"]
    print("keyframes at frames", kf.tolist())
    assert info["keyframes"] == kf.shape[0] >= 6 and kf[0] == 0 and (np.diff(kf) > 0).all()
    assert info["keyframes_after_stop"] == 0
    assert res["ts"].tolist() == [100 + i for i in range(60)]
    edges = res["edges"]
    assert edges.shape[0] >= 1 and "loop closing on" in log
    for e in edges:
        i, j = int(e["i"]), int(e["j"])
        assert 0 <= i < j < kf.shape[0] and j - i >= 2
        deg, mm = loop_truth.pose_error(e["Z"], np.linalg.inv(X[kf[i]]) @ X[kf[j]])
        print(f"edge ({i}, {j}) = C5 frames ({FRAMES[kf[i]]}, {FRAMES[kf[j]]}): {deg:.4f} deg / {mm:.3f} mm off the truth; "
              f"overlap {e['overlap']:.3f}, grey rms {e['gray_rms']:.2f}, fb {e['fb_rot_deg']:.4f} deg / "
              f"{e['fb_trans_m'] * 1e3:.3f} mm")
    for e in edges:
        deg, mm = loop_truth.pose_error(e["Z"], np.linalg.inv(X[kf[e["i"]]]) @ X[kf[e["j"]]])
        assert deg <= 0.05 and mm <= 1.0, (int(e["i"]), int(e["j"]), deg, mm)


def test_saved_files_with_the_variable(runs):
    (out, info, res, _), _, X = runs
    lines = (out / "map_keyframes.txt").read_text().splitlines()
    assert len(lines) == info["keyframes"]
    assert [int(float(ln.split()[0])) for ln in lines] == [100 + int(f) for f in res["kf_frames"]]
    closed = (out / "map_trajectory_closed.txt").read_text().splitlines()
    assert len(closed) == 60 and res["closed"].shape == (60, 4, 4)
    # the corrected trajectory starts where the recorded one does, and the
    # recorded one is what the query returns
    assert np.array_equal(res["closed"][0], res["T"][0])
    X0 = np.linalg.inv(X[0])
    for name, T in (("recorded", res["T"]), ("closed", res["closed"])):
        deg, mm = loop_truth.pose_error(T[59], X0 @ X[59])
        print(f"C5 frame 657, {name}: {deg:.4f} deg / {mm:.3f} mm off the truth")


def test_without_the_variable_nothing_changes(runs):
    (on, _, res_on, _), (off, info, res_off, log), _ = runs
    assert info["keyframes"] == 0 and res_off["kf_frames"].shape == (0,) and res_off["edges"].shape == (0,)
    assert res_off["closed"].shape == (0, 4, 4) and "loop closing" not in log
    assert not (off / "map_trajectory_closed.txt").exists()
    # the live trajectory is never rewritten: the same bytes with and without
    assert (on / "map_trajectory.txt").read_bytes() == (off / "map_trajectory.txt").read_bytes()
    assert np.array_equal(res_on["T"], res_off["T"])
    assert (off / "map_keyframes.txt").read_bytes() == (off / "map_trajectory.txt").read_bytes()
