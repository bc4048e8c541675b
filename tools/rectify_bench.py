#!/usr/bin/env python3
"""The lens rectifier (csrc/rectify.hip) by the numbers, run by
hand (not part of bench.py):

  (default)  k_rectify timed with HIP events at 640x480, depth + RGB, per frame,
             for 1 and 512 frames per call, the map words recomputed per pixel
             and read from the rectifier's map (YOUTH_RECTIFY_MAP=0 / 1 at
             create), with the fraction of the 6.48 TB/s read-stream and
             5.9 TB/s write-stream ceilings on the algorithmic
             10 B/px (5 read, 5 written)
  slam       the drop-in's backlogged rate, processSlamFrame from one Python
             thread, with YOUTH_SLAM_RECTIFY=1 and without, one child process
             each (the module reads its environment at initSlamModule)

The last line is one JSON object.
usage: python tools/rectify_bench.py [slam] [rounds] [reps]"""
import json
import os
import subprocess
import sys
import tempfile

import torch  # noqa: F401  (first: shared HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-rgbd_amd"))
import numpy as np  # noqa: E402

import youth_icp  # noqa: E402
import youth_rectify  # noqa: E402
import youth_synth  # noqa: E402

W, H = 640, 480
D = (-0.28, 0.07, 8e-4, -6e-4, 0.0)
READ_TBS, WRITE_TBS = 6.48, 5.9


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3),
            "max": round(float(np.max(v)), 3)}


def kernel_times(rounds, reps):
    K = youth_icp.default_intrinsics(W, H)
    fr, _, rgb = youth_synth.sequence_rgb(0, 8, W, H)
    s = torch.cuda.Stream()
    floor_us = W * H * 5 / (READ_TBS * 1e12) * 1e6 + W * H * 5 / (WRITE_TBS * 1e12) * 1e6
    out = {"floor_us_per_frame": round(floor_us, 3)}
    for mode in ("recompute", "map"):
        os.environ["YOUTH_RECTIFY_MAP"] = "1" if mode == "map" else "0"
        with youth_rectify.Rectifier(W, H, K, D) as r:
            for n in (1, 512):
                idx = np.arange(n) % 8
                d = torch.from_numpy(np.ascontiguousarray(fr[idx])).cuda()
                c = torch.from_numpy(np.ascontiguousarray(rgb[idx])).cuda()
                do, co = torch.empty_like(d), torch.empty_like(c)
                calls = max(1, 256 // n)
                t = []
                for rd in range(rounds + 1):               # round 0 warms up
                    for _ in range(reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(s)
                        for _ in range(calls):
                            r.device_frames(d, do, c, co, stream=s.cuda_stream)
                        e1.record(s)
                        e1.synchronize()
                        if rd > 0:
                            t.append(e0.elapsed_time(e1) / (calls * n) * 1e3)
                st = stats(t)
                st["of_stream_ceilings"] = round(floor_us / st["median"], 4)
                out[f"{mode}_{n}"] = st
                print(f"kernel {mode:9s} {n:4d} frames/call: {st} us/frame", flush=True)
                del d, c, do, co
    os.environ.pop("YOUTH_RECTIFY_MAP", None)
    return out


_SLAM_CHILD = r"""
import ctypes, json, sys, time
import numpy as np
import youth_icp, youth_rectify, youth_synth
config, n, passes = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
fr, _ = youth_synth.sequence(0, n)
lib = youth_icp.load_library()
ptrs = [fr[f].ctypes.data_as(ctypes.POINTER(ctypes.c_int16)) for f in range(n)]
youth_icp.initSlamModule(config)
rates = []
try:
    active = youth_rectify.slam_rectify_active()
    for p in range(passes + 1):                      # pass 0 warms up
        youth_icp.resetSlam()
        youth_icp.slam_wait_idle(20000)
        t0 = time.perf_counter()
        for f in range(n):
            while lib.youth_slam_queue_size() >= 10:
                pass
            lib.processSlamFrame(ptrs[f], None, 640, 480, f)
        youth_icp.slam_wait_idle(60000)
        dt = time.perf_counter() - t0
        if p > 0:
            rates.append(n / dt)
        assert lib.youth_slam_trajectory_length() == n
finally:
    youth_icp.stopSlamModule()
print("RESULT " + json.dumps({"active": active, "frames_per_s": rates}))
"""


def slam_rates(n=400, passes=3):
    tmp = tempfile.mkdtemp()
    cfg = os.path.join(tmp, "lens.yaml")
    with open(cfg, "w") as f:
        f.write("%YAML:1.0\nCamera.fx: 570.3\nCamera.fy: 570.3\nCamera.cx: 320.0\nCamera.cy: 240.0\n"
                + "".join(f"Camera.{k}: {v!r}\n" for k, v in zip(("k1", "k2", "p1", "p2", "k3"), D))
                + "Camera.width: 640\nCamera.height: 480\nDepthMapFactor: 1000.0\n")
    out = {"frames": n, "producer": "one Python thread, ctypes processSlamFrame"}
    for name in ("off", "on"):
        env = {k: v for k, v in os.environ.items() if not k.startswith("YOUTH_SLAM_")}
        if name == "on":
            env["YOUTH_SLAM_RECTIFY"] = "1"
        env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "slam-rgbd_amd")] + [p for p in sys.path if p])
        r = subprocess.run([sys.executable, "-c", _SLAM_CHILD, cfg, str(n), str(passes)], env=env,
                           capture_output=True, text=True, timeout=600)
        if r.returncode:
            raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
        res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        assert res["active"] == (name == "on")
        out[name] = stats(res["frames_per_s"])
        print(f"slam rectify {name:3s}: {out[name]} frames/s", flush=True)
    out["on_over_off"] = round(out["on"]["median"] / out["off"]["median"], 4)
    return out


def main():
    args = sys.argv[1:]
    slam = bool(args) and args[0] == "slam"
    args = args[1:] if slam else args
    rounds = int(args[0]) if len(args) > 0 else 3
    reps = int(args[1]) if len(args) > 1 else 3
    if slam:
        res = {"size": [W, H], "D": list(D), "slam_backlogged": slam_rates(passes=rounds)}
    else:
        res = {"size": [W, H], "D": list(D), "planes": "int16 depth + uint8 RGB",
               "kernel_us_per_frame": kernel_times(rounds, reps)}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
