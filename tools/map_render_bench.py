#!/usr/bin/env python3
"""The map render (csrc/map_render.hip) by the numbers, run by
hand (not part of bench.py), in one process:

  (1) render    youth_map_render_device at 640x480, 1 view and 8 views per call,
                for the two splat paths: "loop" (YOUTH_MAP_RENDER_QUEUE=0, a lane
                walks its own footprints) and "queue" (=1, the LDS queue).  The
                map is the 640x480 synthetic sequence (youth_synth) at its
                ground-truth poses, 100 voxels per metre, 2^22 slots.  The
                variants alternate within every round; HIP events on one stream.
                A call is two kernels; they are told apart by two more variants
                on the same maps and sizes:
                  "scan"     min_count = 2^32-1: every voxel fails the first
                             test, so the splat is the key scan and the record
                             loads of the occupied slots, without atomics
                  "resolve"  a 64-slot map: the splat is one workgroup, what is
                             left is k_map_render_resolve (and two launches)
                so splat = call - resolve, and the atomics' share = call - scan.
  (2) yardsticks  k_map_integrate per frame into an empty map in the same run;
                the device's copy bandwidth (torch, 256 MiB) and what reading
                the 32 MiB of keys costs at that rate; the pixels the footprints
                put forward per view (an upper bound of the atomics issued),
                counted on the host from the map's records.
  (3) tracking  exploratory, not gated: the sequence tracked frame-to-frame and
                frame-to-model (each frame aligned against the view rendered at
                the previous estimate from the map of the frames so far), depth
                filter off and on; drift against the ground truth at frames 16
                and 31.  `notrack` as the last argument skips it.

The two paths' outputs are compared bytewise.  The last line is one JSON object.
usage: python tools/map_render_bench.py [frames] [rounds] [reps] [notrack]"""
import json
import os
import sys

import torch  # noqa: F401  (first: shared HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-rgbd_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))      # render_truth: the host-side count
import numpy as np  # noqa: E402

import youth_icp  # noqa: E402
import youth_map  # noqa: E402
import youth_synth  # noqa: E402
from render_truth import candidates, project  # noqa: E402

W, H = 640, 480
VPM = 100.0
SLOTS = 1 << 22


def stats(v):
    return {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1),
            "max": round(float(np.max(v)), 1)}


def pose_error(T, T_gt):
    R = T[:3, :3].T @ T_gt[:3, :3]
    ang = np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
    return round(float(ang), 4), round(float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3]) * 1000.0), 2)


def tracking(frames, T_wc):
    """Drift of frame-to-frame and frame-to-model tracking, filter off / on."""
    n = frames.shape[0]
    out = {}
    with youth_icp.IcpContext(W, H, 2) as ctx:
        for filt in ("raw", "filtered"):
            ctx.set_depth_filter(8, 96) if filt == "filtered" else ctx.set_depth_filter(None)
            for mode in ("frame", "model"):
                T = T_wc[0].copy()
                errs = {}
                with youth_map.VoxelMap(VPM, SLOTS) as m:
                    for k in range(1, n):
                        if mode == "model":
                            m.integrate(frames[k - 1], None, None, T)
                            ref = m.render(T, W, H, want_rgb=False)[0]
                        else:
                            ref = frames[k - 1]
                        ctx.track_reset()
                        ctx.track_frame(ref)
                        T_rel, st, _ = ctx.track_frame(frames[k])    # P_ref = T_rel P_k
                        T = T @ T_rel
                        if k in (16, 31):
                            errs[str(k)] = pose_error(T, T_wc[k])
                out[f"{filt}_{mode}"] = errs
                print(f"tracking {filt:8s} frame-to-{mode:5s}: (deg, mm) at frame {errs}", flush=True)
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "notrack"]
    n = int(args[0]) if len(args) > 0 else 32
    rounds = int(args[1]) if len(args) > 1 else 3
    reps = int(args[2]) if len(args) > 2 else 5
    frames, T_wc = youth_synth.sequence(0, n)
    rgb = np.random.default_rng(5).integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    T32 = np.ascontiguousarray(T_wc.reshape(n, 16)[:, :12], np.float32)
    d = torch.from_numpy(frames).cuda()
    c = torch.from_numpy(rgb).cuda()
    dT = torch.from_numpy(T32).cuda()
    s = torch.cuda.Stream()
    maps = {}
    for name, env in (("loop", "0"), ("queue", "1")):
        os.environ["YOUTH_MAP_RENDER_QUEUE"] = env       # read at create
        maps[name] = youth_map.VoxelMap(VPM, SLOTS)
        maps[name].integrate_device(d.data_ptr(), c.data_ptr(), n, W, H, dT.data_ptr())
        maps[name].sync()
    os.environ.pop("YOUTH_MAP_RENDER_QUEUE")
    tiny = youth_map.VoxelMap(VPM, 64)
    fresh = youth_map.VoxelMap(VPM, SLOTS)
    tiny.sync()
    fresh.sync()
    view_at = [(4 * k + 2) % n for k in range(8)]
    V8 = np.stack([youth_map.view_from_pose(T_wc[f]) for f in view_at]).reshape(8, 12)
    dV = torch.from_numpy(np.ascontiguousarray(V8)).cuda()
    out_d = torch.zeros((8, H, W), dtype=torch.int16, device="cuda")
    out_c = torch.zeros((8, H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def timed(fn, per):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / per * 1e3           # us per unit

    def render(m, nv, min_count=0):
        def fn():
            for _ in range(16 // nv):                    # 16 views per timed sweep
                m.render_device(dV.data_ptr(), out_d.data_ptr(), out_c.data_ptr(), nv, W, H,
                                min_count=min_count, stream=s.cuda_stream)
        return fn

    def integrate():
        for f in range(n):
            fresh.integrate_device(d.data_ptr() + f * H * W * 2, c.data_ptr() + f * H * W * 3, 1,
                                   W, H, dT.data_ptr() + f * 48, stream=s.cuda_stream)

    variants = [(f"{name}_{nv}", render(maps[name], nv)) for name in ("loop", "queue")
                for nv in (1, 8)]
    variants += [(f"scan_{nv}", render(maps["queue"], nv, 0xffffffff)) for nv in (1, 8)]
    variants += [(f"resolve_{nv}", render(tiny, nv)) for nv in (1, 8)]
    times = {k: [] for k, _ in variants}
    times["integrate"] = []
    for r in range(rounds + 1):                          # round 0 warms every shape up
        for _ in range(reps):
            for k, fn in variants:
                t = timed(fn, 16)
                if r > 0:
                    times[k].append(t)
            fresh.clear()
            fresh.sync()                                 # the clear runs on the map's stream
            t = timed(integrate, n)
            if r > 0:
                times["integrate"].append(t)
        if r > 0:
            print(f"round {r}: " + "  ".join(f"{k} {np.median(v[-reps:]):.1f}"
                                             for k, v in times.items()) + "  us", flush=True)
    # the two paths: identical bytes
    got = {}
    for name in ("loop", "queue"):
        maps[name].render_device(dV.data_ptr(), out_d.data_ptr(), out_c.data_ptr(), 8, W, H)
        maps[name].sync()
        got[name] = (out_d.cpu().numpy().tobytes(), out_c.cpu().numpy().tobytes())
    same = got["loop"] == got["queue"]
    # copy bandwidth, and the key scan at that rate
    x = torch.empty(1 << 26, dtype=torch.int32, device="cuda")
    y = torch.empty_like(x)
    bw = []
    with torch.cuda.stream(s):
        for r in range(6):
            t = timed(lambda: y.copy_(x), 1)
            if r > 0:
                bw.append(2 * x.numel() * 4 / t / 1e3)   # GB/s, read + write
    bw = float(np.median(bw))
    # pixels put forward per view (host)
    rec = maps["queue"].extract()
    K = youth_synth.viewer_intrinsics(W, H)
    fwd, vox_in = [], []
    for k in range(8):
        u0, v0, sz, val = project(rec, VPM, V8[k], K, W, H)
        fwd.append(int(candidates(u0, v0, sz, val, W, H)[0].size))
        vox_in.append(int(u0.size))
    covered = [int((out_d[k] > 0).sum().item()) for k in range(8)]
    us = {k: stats(v) for k, v in times.items()}
    res = {"size": [W, H], "frames": n, "vpm": VPM, "slots": SLOTS, "voxels": int(rec.shape[0]),
           "occupancy": round(rec.shape[0] / SLOTS, 4), "paths_identical": same,
           "us_per_view": {k: v for k, v in us.items() if k != "integrate"},
           "integrate_us_per_frame": us["integrate"],
           "copy_GBps": round(bw, 0), "key_scan_us_at_copy_rate": round(SLOTS * 8 / bw / 1e3, 1),
           "per_view": {"voxels_in_view": int(np.median(vox_in)),
                        "pixels_put_forward": int(np.median(fwd)),
                        "pixels_covered": int(np.median(covered))}}
    for m in list(maps.values()) + [tiny, fresh]:
        m.close()
    if "notrack" not in sys.argv[1:]:
        res["tracking_drift_deg_mm"] = tracking(frames, T_wc)
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
