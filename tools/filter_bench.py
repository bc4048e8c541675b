#!/usr/bin/env python3
"""The edge-preserving depth filter (csrc/depth_filter.hip) by
the numbers, run by hand (not part of bench.py):

  (1) kernel    k_depth_filter timed with HIP events at 640x480, per frame, for
                1, 64 and 1024 frames per call (SURVEY-noise frames, defaults)
  (2) tracker   track_host_sequence, micro-batches of 8, 200 frames of the
                synthetic sequence: one context with the filter on and one
                with it off in one process, alternating within every round
  (3) accuracy  the 8 SURVEY-noise and default-noise 640x480 pairs through
                track_frame (dst, then src), filter off and on: rotation and
                translation error against the generator's T_gt

The last line is one JSON object.
usage: python tools/filter_bench.py [rounds] [reps]"""
import json
import os
import sys
import time

import torch  # noqa: F401  (first: shared HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-rgbd_amd"))
import numpy as np  # noqa: E402

import youth_filter  # noqa: E402
import youth_icp  # noqa: E402
import youth_synth  # noqa: E402

W, H = 640, 480


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3),
            "max": round(float(np.max(v)), 3)}


def kernel_times(rounds, reps):
    base = youth_synth.pairs(0, 8, W, H, flags=youth_synth.SURVEY_FLAGS)[0]
    s = torch.cuda.Stream()
    out = {}
    for n in (1, 64, 1024):
        d = torch.from_numpy(np.ascontiguousarray(base[np.arange(n) % 8])).cuda()
        o = torch.empty_like(d)
        calls = max(1, 256 // n)                       # calls per timed sweep
        t = []
        for r in range(rounds + 1):                    # round 0 warms up
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(calls):
                    youth_filter.depth_filter_device(d, o, 8, 96, stream=s.cuda_stream)
                e1.record(s)
                e1.synchronize()
                if r > 0:
                    t.append(e0.elapsed_time(e1) / (calls * n) * 1e3)
        out[str(n)] = stats(t)
        print(f"kernel {n:5d} frames/call: {out[str(n)]} us/frame", flush=True)
        del d, o
    return out


def tracker_ab(rounds, reps):
    frames, _ = youth_synth.sequence(0, 200)
    ctx = {}
    for name in ("off", "on"):
        c = youth_icp.IcpContext(W, H, 16)
        c.track_set_batch(8)
        if name == "on":
            c.set_depth_filter(8, 96)
        ctx[name] = c
    t = {"off": [], "on": []}
    for r in range(rounds + 1):
        for _ in range(reps):
            for name in ("off", "on"):
                c = ctx[name]
                c.track_reset()
                t0 = time.perf_counter()
                T, st = c.track_host_sequence(frames)
                dt = time.perf_counter() - t0
                assert T.shape[0] == 199 and not (st & 4).any()
                if r > 0:
                    t[name].append(len(frames) / dt)
        if r > 0:
            print(f"round {r}: " + "  ".join(f"{k} {np.median(v[-reps:]):8.0f}" for k, v in t.items())
                  + "  frames/s", flush=True)
    for c in ctx.values():
        c.close()
    res = {k: stats(v) for k, v in t.items()}
    res["on_over_off"] = round(float(np.median(t["on"]) / np.median(t["off"])), 4)
    return res


def pose_error(T, T_gt):
    R = T[:3, :3] @ T_gt[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3]) * 1000.0)


def accuracy():
    out = {}
    with youth_icp.IcpContext(W, H, 2) as ctx:
        for noise, flags in (("survey", youth_synth.SURVEY_FLAGS),
                             ("default", youth_synth.DEFAULT_FLAGS)):
            src, dst, T_gt = youth_synth.pairs(0, 8, W, H, flags=flags)
            for name in ("raw", "filtered"):
                ctx.set_depth_filter(8, 96) if name == "filtered" else ctx.set_depth_filter(None)
                err = []
                for p in range(8):
                    ctx.track_reset()
                    ctx.track_frame(dst[p])
                    err.append(pose_error(ctx.track_frame(src[p])[0], T_gt[p]))
                e = np.array(err)
                out[f"{noise}_{name}"] = {
                    "rot_deg_median": round(float(np.median(e[:, 0])), 4),
                    "rot_deg_max": round(float(e[:, 0].max()), 4),
                    "trans_mm_median": round(float(np.median(e[:, 1])), 3),
                    "trans_mm_max": round(float(e[:, 1].max()), 3)}
                print(f"{noise:8s} {name:9s} {out[f'{noise}_{name}']}", flush=True)
    return out


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    res = {"size": [W, H], "params": list(youth_filter.default_params()),
           "kernel_us_per_frame": kernel_times(rounds, reps),
           "tracker_frames_per_s": tracker_ab(rounds, reps),
           "accuracy_8_pairs": accuracy()}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
