"""Lens rectification through the SLAM.h drop-in: with
YOUTH_SLAM_RECTIFY=1 and a YAML that has distortion coefficients the module
rectifies each frame once, in place, before anything else sees it; without the
variable it does what it always did and says that the coefficients are
ignored.  The module reads its environment at initSlamModule, so every case
runs in a fresh child process with its own environment."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rectify_truth as rt
import youth_rectify
from conftest import ORACLE, PKG
from test_rectify import D_BARREL, K160, intr, value_frames

pytestmark = pytest.mark.gpu

W, H, N = 160, 120, 8

_CHILD = r"""
import json, os, sys
import numpy as np
import youth_icp, youth_rectify
out, config, frames = sys.argv[1], sys.argv[2], np.load(sys.argv[3])
d, c = frames["d"], frames["c"]
res = {}
youth_icp.initSlamModule(config)
assert youth_icp.isSlamModuleRunning() == 1
try:
    res["active"] = youth_rectify.slam_rectify_active()
    res["rgbd"] = youth_icp.slam_rgbd_active()
    for k in range(len(d)):
        assert youth_icp.processSlamFrame(d[k], c[k], d.shape[2], d.shape[1], 10 + k) == 1
        if k == 2:      # a live frame, then a backlog
            assert youth_icp.slam_wait_idle(20000) == 1
    assert youth_icp.slam_wait_idle(20000) == 1
    ts, T = youth_icp.slam_trajectory()
    res["points"] = youth_icp.getSlamMapPoints()
    assert youth_icp.saveSlamMap(os.path.join(out, "map")) == 1
finally:
    youth_icp.stopSlamModule()
res["active_after_stop"] = youth_rectify.slam_rectify_active()
np.savez(os.path.join(out, "res.npz"), ts=ts, T=T)
print("RESULT " + json.dumps(res))
"""


def _yaml(path, D):
    keys = ("k1", "k2", "p1", "p2", "k3")
    path.write_text("\n".join(
        ["%YAML:1.0", 'Camera.type: "PinHole"', f"Camera.fx: {K160[0]}", f"Camera.fy: {K160[1]}",
         f"Camera.cx: {K160[2]}", f"Camera.cy: {K160[3]}"]
        + [f"Camera.{k}: {v!r}" for k, v in zip(keys, D)]
        + [f"Camera.width: {W}", f"Camera.height: {H}", "Camera.fps: 30.0", "DepthMapFactor: 1000.0", ""]))
    return str(path)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """The distorted frames, the same frames rectified beforehand by
    youth_rectify_host (which are the restatement's), and the two YAMLs."""
    base = tmp_path_factory.mktemp("rectify")
    d, c, _ = value_frames(D_BARREL, N)
    with youth_rectify.Rectifier(W, H, intr(K160), D_BARREL) as r:
        rd, rc = r.host(d, c)
    want_d, want_c = rt.rectify(d, c, W, H, K160, D_BARREL)
    assert np.array_equal(rd, want_d) and np.array_equal(rc, want_c) and (rd != d).any()
    np.savez(base / "raw.npz", d=d, c=c)
    np.savez(base / "rect.npz", d=rd, c=rc)
    return {"base": base, "raw": str(base / "raw.npz"), "rect": str(base / "rect.npz"),
            "lens": _yaml(base / "lens.yaml", D_BARREL), "plain": _yaml(base / "plain.yaml", (0.0,) * 5)}


def _run_child(setup, name, env_extra, config, frames):
    out = setup["base"] / name
    out.mkdir()
    env = {k: v for k, v in os.environ.items()
           if not k.startswith(("YOUTH_SLAM_", "YOUTH_ICP_DEPTH_FILTER", "YOUTH_RGBD_", "YOUTH_RECTIFY_"))}
    env.update(env_extra, PYTHONPATH=os.pathsep.join([PKG, ORACLE] + [p for p in sys.path if p]))
    r = subprocess.run([sys.executable, "-c", _CHILD, str(out), setup[config], setup[frames]], env=env,
                       timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    notices = [ln for ln in r.stderr.splitlines() if "YOUTH_SLAM_RECTIFY" in ln]
    return out, json.loads(line[len("RESULT "):]), np.load(out / "res.npz", allow_pickle=False), notices


def _same(a, b):
    assert a["ts"].tolist() == b["ts"].tolist() == [10 + k for k in range(N)]
    assert a["T"].tobytes() == b["T"].tobytes()


@pytest.mark.parametrize("mode", ["depth_map", "rgbd"])
def test_rectifying_module_equals_a_module_fed_rectified_frames(setup, mode):
    extra = {"YOUTH_SLAM_MAP_VPM": "100"} if mode == "depth_map" else {"YOUTH_SLAM_RGBD": "1"}
    on_dir, on, res_on, notes = _run_child(setup, mode + "_on", dict(extra, YOUTH_SLAM_RECTIFY="1"), "lens", "raw")
    assert on["active"] == 1 and on["active_after_stop"] == 0 and not notes
    assert on["rgbd"] == (mode == "rgbd")
    pre_dir, pre, res_pre, notes = _run_child(setup, mode + "_pre", extra, "plain", "rect")
    assert pre["active"] == 0 and not notes
    _same(res_on, res_pre)
    assert on["points"] == pre["points"] > 0
    assert (on_dir / "map_trajectory.txt").read_bytes() == (pre_dir / "map_trajectory.txt").read_bytes()
    if mode == "depth_map":
        ply = (on_dir / "map_map.ply").read_bytes()
        assert len(ply) > 1000 and ply == (pre_dir / "map_map.ply").read_bytes()


def test_without_the_variable_nothing_changes_but_one_notice(setup):
    _, plain, res_plain, notes = _run_child(setup, "plain", {}, "plain", "raw")
    assert plain["active"] == 0 and not notes
    _, lens, res_lens, notes = _run_child(setup, "lens_off", {}, "lens", "raw")
    assert lens["active"] == 0
    assert len(notes) == 1 and "ignored" in notes[0], notes
    _same(res_lens, res_plain)
    assert lens["points"] == plain["points"]
    # the variable without coefficients: nothing to rectify
    _, zero, res_zero, notes = _run_child(setup, "zero_on", {"YOUTH_SLAM_RECTIFY": "1"}, "plain", "raw")
    assert zero["active"] == 0 and not notes
    _same(res_zero, res_plain)
    # and rectifying does change the trajectory of these frames
    _, on, res_on, _ = _run_child(setup, "on", {"YOUTH_SLAM_RECTIFY": "1"}, "lens", "raw")
    assert on["active"] == 1 and res_on["T"].tobytes() != res_plain["T"].tobytes()
