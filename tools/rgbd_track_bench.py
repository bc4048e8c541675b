#!/usr/bin/env python3
"""The streaming RGB-D tracker (csrc/rgbd_track.cpp) by the
numbers, run by hand (not part of bench.py).  One MI355X, 640x480, 10
iterations, the variants alternating within every round:

  (a) ingest    k_rgbd_pull per frame at m = 1 and 8 page-locked frames, with
                and without the RGB copy (youth_rgbd_pull_host), against what
                youth_rgbd_track_host_sequence does for the same frames:
                hipMemcpyAsync of depth and RGB, then k_rgbd_prep<3> to grey
  (b) stream    frames/s through youth_rgbd_track_submit / _collect from
                page-locked buffers at b = 1 and 8, two submissions in flight,
                against youth_rgbd_track_host_sequence on 9-frame pieces
  (c) drop-in   processSlamFrame backlogged (frames/s) and live (ms from push
                to pose), with YOUTH_SLAM_RGBD=1 and in default mode; one child
                process per mode (the module reads its environment at init)

With --levels auto|LIST (the tracker's own schedule, youth_rgbd_track_set_levels):

  (a) ingest    also k_rgbd_pull followed by k_rgbd_decimate for the schedule's
                coarse strides on the same stream, the scheduled tracker's ingest
  (b) stream    also submit_b1 / submit_b8 with the schedule set
  (c) drop-in   also YOUTH_SLAM_RGBD=1 with YOUTH_SLAM_RGBD_LEVELS

The last line is one JSON object.
usage: python tools/rgbd_track_bench.py [rounds] [reps] [--levels auto|LIST] [ingest] [stream] [drop-in]"""
import json
import os
import subprocess
import sys
import time

import torch  # noqa: F401  (first: shared HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-rgbd_amd"))
import numpy as np  # noqa: E402

import youth_icp  # noqa: E402
import youth_rgbd  # noqa: E402
import youth_synth  # noqa: E402

W, H = 640, 480
N = W * H


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3),
            "max": round(float(np.max(v)), 3)}


def pinned_frames(fr, rgb):
    pd, pc = [], []
    for d, c in zip(fr, rgb):
        a, b = youth_icp.PinnedFrame(H, W), youth_rgbd.PinnedColor(H, W)
        a.array[:] = d
        b.array[:] = c
        pd.append(a)
        pc.append(b)
    return pd, pc


LEVELS = []   # --levels: the tracker's schedule


def ingest(pd, pc, rounds, reps):
    s = torch.cuda.Stream()
    strides = [st for st, _ in LEVELS if st > 1]
    out = {}
    with youth_rgbd.RgbdContext(W, H, 16) as ctx:
        for m in (1, 8):
            dl, cl = [p.array for p in pd[:m]], [p.array for p in pc[:m]]
            d_d = torch.empty((m, H, W), dtype=torch.int16, device="cuda")
            d_g = torch.empty((m, H, W), dtype=torch.uint8, device="cuda")
            d_c = torch.empty((m, H, W, 3), dtype=torch.uint8, device="cuda")
            td = [torch.from_numpy(a) for a in dl]
            tc = [torch.from_numpy(a) for a in cl]

            def memcpy_prep():
                with torch.cuda.stream(s):
                    for i in range(m):
                        d_d[i].copy_(td[i], non_blocking=True)
                        d_c[i].copy_(tc[i], non_blocking=True)
                ctx.prep_device(d_c, 3, m, d_g, None, stream=s.cuda_stream)

            run = {"pull": lambda: ctx.pull_host(dl, cl, d_d, d_g, None, stream=s.cuda_stream),
                   "pull_with_rgb": lambda: ctx.pull_host(dl, cl, d_d, d_g, d_c, stream=s.cuda_stream),
                   "memcpy_and_prep3": memcpy_prep}
            if strides:
                shapes = [((H + st - 1) // st, (W + st - 1) // st) for st in strides]
                lv_d = [torch.empty((m, h, w), dtype=torch.int16, device="cuda") for h, w in shapes]
                lv_g = [torch.empty((m, h, w), dtype=torch.uint8, device="cuda") for h, w in shapes]

                def pull_then_decimate():
                    ctx.pull_host(dl, cl, d_d, d_g, None, stream=s.cuda_stream)
                    for st, od, og in zip(strides, lv_d, lv_g):
                        youth_rgbd.decimate_device(d_d.data_ptr(), d_g.data_ptr(), m, W, H, st,
                                                   od.data_ptr(), og.data_ptr(), stream=s.cuda_stream)

                run = {"pull_then_decimate": pull_then_decimate, **run}
            t = {k: [] for k in run}
            for r in range(rounds + 1):                # round 0 warms up
                for _ in range(reps):
                    for name, fn in run.items():
                        e0 = torch.cuda.Event(enable_timing=True)
                        e1 = torch.cuda.Event(enable_timing=True)
                        e0.record(s)
                        for _ in range(4):
                            fn()
                        e1.record(s)
                        e1.synchronize()
                        if r > 0:
                            t[name].append(e0.elapsed_time(e1) / (4 * m) * 1e3)
            res = {k: stats(v) for k, v in t.items()}      # us per frame
            res["pull_GBs_over_the_bus"] = round(5 * N / (res["pull"]["median"] * 1e-6) / 1e9, 2)
            out[str(m)] = res
            print(f"ingest m={m}: {res}", flush=True)
    return out


def stream(pd, pc, fr, rgb, rounds, reps):
    n = len(pd)
    out = {}

    def tracked(ctx, b):
        sizes, f = [], 0
        t0 = time.perf_counter()
        while f < n:
            m = min(b, n - f)
            if len(sizes) == 2:
                for _ in range(sizes.pop(0)):
                    ctx.track_collect()
            ctx.track_submit([p.array for p in pd[f:f + m]], [p.array for p in pc[f:f + m]])
            sizes.append(m)
            f += m
        while ctx.track_pending():
            ctx.track_collect()
        return n / (time.perf_counter() - t0)

    def pieces(ctx):
        t0 = time.perf_counter()
        for f in range(0, n - 8, 8):                    # 9-frame pieces sharing an end frame
            ctx.track_host_sequence(fr[f:f + 9], rgb[f:f + 9])
        return (n - 1) // 8 * 8 / (time.perf_counter() - t0)

    ctxs = {}
    for b in (1, 8):
        ctxs[b] = youth_rgbd.RgbdContext(W, H, 16)
        ctxs[b].track_set_batch(b)
    seq = youth_rgbd.RgbdContext(W, H, 16)
    run = {"submit_b1": lambda: tracked(ctxs[1], 1), "submit_b8": lambda: tracked(ctxs[8], 8),
           "host_sequence_9": lambda: pieces(seq)}
    if LEVELS:
        for b in (1, 8):
            ctxs[-b] = youth_rgbd.RgbdContext(W, H, 16)
            ctxs[-b].track_set_batch(b)
            ctxs[-b].track_set_levels(LEVELS)
        run["submit_b1_levels"] = lambda: tracked(ctxs[-1], 1)
        run["submit_b8_levels"] = lambda: tracked(ctxs[-8], 8)
    t = {k: [] for k in run}
    for r in range(rounds + 1):
        for _ in range(reps):
            for name, fn in run.items():
                for c in ctxs.values():
                    c.track_reset()
                v = fn()
                if r > 0:
                    t[name].append(v)
    for c in list(ctxs.values()) + [seq]:
        c.close()
    out = {k: stats(v) for k, v in t.items()}           # frames/s
    print(f"stream: {out}", flush=True)
    return out


_SLAM_CHILD = r"""
import json, sys, time
import numpy as np
import youth_icp, youth_synth
n, rounds = int(sys.argv[1]), int(sys.argv[2])
fr, _, rgb = youth_synth.sequence_rgb(0, n)
youth_icp.initSlamModule(None)
res = {"rgbd_active": youth_icp.slam_rgbd_active(), "backlog_fps": [], "live_ms": []}
try:
    for r in range(rounds + 1):
        youth_icp.resetSlam()
        t0 = time.perf_counter()
        for k in range(n):
            while youth_icp.slam_queue_size() >= 10:
                assert time.perf_counter() - t0 < 60.0, "queue stuck"
            assert youth_icp.processSlamFrame(fr[k], rgb[k], 640, 480, k) == 1
        assert youth_icp.slam_wait_idle(60000) == 1
        dt = time.perf_counter() - t0
        assert youth_icp.slam_trajectory()[1].shape[0] == n
        if r > 0:
            res["backlog_fps"].append(n / dt)
        youth_icp.resetSlam()
        lat = []
        lib = youth_icp.load_library()
        for k in range(n):
            t0 = time.perf_counter()
            assert youth_icp.processSlamFrame(fr[k], rgb[k], 640, 480, k) == 1
            while lib.youth_slam_trajectory_length() <= k:
                assert time.perf_counter() - t0 < 10.0, "no pose within 10 s"
            lat.append((time.perf_counter() - t0) * 1e3)
        if r > 0:
            res["live_ms"].append(float(np.median(lat[1:])))
    res["batched"] = youth_icp.slam_batched_frames()
finally:
    youth_icp.stopSlamModule()
print("RESULT " + json.dumps(res))
"""


def drop_in(rounds):
    out = {}
    modes = [("default", {}), ("rgbd", {"YOUTH_SLAM_RGBD": "1"})]
    if LEVELS:
        spec = ",".join(f"{st}:{it}" for st, it in LEVELS)
        modes.append(("rgbd_levels", {"YOUTH_SLAM_RGBD": "1", "YOUTH_SLAM_RGBD_LEVELS": spec}))
    for mode, extra in modes:
        env = {k: v for k, v in os.environ.items() if not k.startswith("YOUTH_SLAM_")}
        env.update(extra, PYTHONPATH=os.path.join(ROOT, "slam-rgbd_amd"))
        r = subprocess.run([sys.executable, "-c", _SLAM_CHILD, "64", str(rounds)], env=env,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"drop-in child ({mode}) failed:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        out[mode] = {"rgbd_active": res["rgbd_active"], "batched_frames": res["batched"],
                     "backlog_frames_per_s": stats(res["backlog_fps"]),
                     "live_ms_push_to_pose": stats(res["live_ms"])}
        print(f"drop-in {mode}: {out[mode]}", flush=True)
    return out


def main():
    global LEVELS
    args = sys.argv[1:]
    if "--levels" in args:
        k = args.index("--levels")
        LEVELS = youth_rgbd.parse_levels(args[k + 1], W, H)
        del args[k:k + 2]
    parts = [a for a in args if not a.isdigit()] or ["ingest", "stream", "drop-in"]
    nums = [int(a) for a in args if a.isdigit()]
    rounds = nums[0] if len(nums) > 0 else 3
    reps = nums[1] if len(nums) > 1 else 3
    fr, _, rgb = youth_synth.sequence_rgb(0, 33, W, H)
    pd, pc = pinned_frames(fr, rgb)
    res = {"size": [W, H], "params": list(youth_rgbd.default_params()),
           "levels": [list(l) for l in LEVELS]}
    if "ingest" in parts:
        res["ingest_us_per_frame"] = ingest(pd, pc, rounds, reps)
    if "stream" in parts:
        res["stream_frames_per_s"] = stream(pd, pc, fr, rgb, rounds, reps)
    for p in pd + pc:
        p.close()
    if "drop-in" in parts:
        res["drop_in"] = drop_in(rounds)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
