#!/usr/bin/env python3
"""A/B of the voxel map's integration kernel (csrc/voxel_map.hip) in one
process, run by hand (not part of bench.py):

  (a) lds     k_map_integrate with the per-workgroup LDS table (the default)
  (b) direct  YOUTH_MAP_LDS=0: every run of pixels straight to the global table
  (c) cloud   youth_cloud_build_device_posed on the same frames: the yardstick,
              the same bytes read and 24 B per pixel written, no atomics

on the synthetic 640x480 sequence (youth_synth) with its ground-truth poses at
100 voxels per metre, one frame per call as the SLAM worker integrates them.
The variants alternate within every round; each is timed with HIP events on one
stream, "fresh" = the sequence into an empty map (every voxel inserted),
"revisit" = the same sequence again (every voxel found).  The records of (a)
and (b) are compared bytewise.  The last line is one JSON object.
usage: python tools/map_bench.py [frames] [rounds] [reps]

`python tools/map_bench.py remove [frames] [rounds] [reps]` times removal, move
and compaction (youth_map_remove.h) beside integration: the same frames, one
process, (a) and (b) alternating within every round.  Per repetition a map
takes the sequence twice (fresh, revisit), gives it back twice (remove_shared:
the voxels stay live; remove_last: every voxel is vacated), takes it again and
is moved to poses 2 cm away, one frame per call (move) and back in one call of
all frames (move_batch); then youth_map_compact runs, timed on the host with
its allocation and its wait (compact, also in us per frame of the sequence)."""
import json
import os
import sys

import torch  # noqa: F401  (first: shared HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-rgbd_amd"))
import numpy as np  # noqa: E402

import youth_map  # noqa: E402
import youth_synth  # noqa: E402
import youth_viewer  # noqa: E402

VPM = 100.0
SLOTS = 1 << 22


def main_remove(argv):
    import time

    n = int(argv[0]) if len(argv) > 0 else 32
    rounds = int(argv[1]) if len(argv) > 1 else 3
    reps = int(argv[2]) if len(argv) > 2 else 5
    frames, T_wc = youth_synth.sequence(0, n)
    n, H, W = frames.shape
    rgb = np.random.default_rng(5).integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    T32 = np.ascontiguousarray(T_wc.reshape(n, 16)[:, :12], np.float32)
    T32b = T32.copy()
    T32b[:, 3] += np.float32(0.02)                   # 2 cm along x: two voxels away
    d = torch.from_numpy(frames).cuda()
    c = torch.from_numpy(rgb).cuda()
    dT, dTb = torch.from_numpy(T32).cuda(), torch.from_numpy(T32b).cuda()
    s = torch.cuda.Stream()
    maps = {}
    for name, env in (("lds", "1"), ("direct", "0")):
        os.environ["YOUTH_MAP_LDS"] = env            # read at create
        maps[name] = youth_map.VoxelMap(VPM, SLOTS)
        maps[name].sync()
    os.environ.pop("YOUTH_MAP_LDS")
    torch.cuda.synchronize()

    def sweep(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for f in calls:
            fn(f)
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / n * 1e3         # us per frame

    def frame(f, count=1):
        return d.data_ptr() + f * H * W * 2, c.data_ptr() + f * H * W * 3, count, W, H

    legs = ("fresh", "revisit", "remove_shared", "remove_last", "move", "move_batch", "compact")
    times = {name + "_" + leg: [] for name in maps for leg in legs}
    compact_ms = {name: [] for name in maps}
    exact = True
    for r in range(rounds + 1):                      # round 0 warms every shape up
        for name, m in maps.items():
            for _ in range(reps):
                add = lambda f: m.integrate_device(*frame(f), dT.data_ptr() + f * 48, stream=s.cuda_stream)
                sub = lambda f: m.remove_device(*frame(f), dT.data_ptr() + f * 48, stream=s.cuda_stream)
                mov = lambda f: m.move_device(*frame(f), dT.data_ptr() + f * 48, dTb.data_ptr() + f * 48,
                                              stream=s.cuda_stream)
                back = lambda f: m.move_device(*frame(0, n), dTb.data_ptr(), dT.data_ptr(),
                                               stream=s.cuda_stream)
                m.clear()
                m.sync()                             # the clear runs on the map's stream
                t = {"fresh": sweep(add, range(n)), "revisit": sweep(add, range(n)),
                     "remove_shared": sweep(sub, range(n)), "remove_last": sweep(sub, range(n))}
                empty = m.extract().shape[0] == 0
                sweep(add, range(n))
                want = m.extract()
                t["move"] = sweep(mov, range(n))
                t["move_batch"] = sweep(back, [0])
                m.sync()
                t0 = time.perf_counter()
                m.compact()
                ms = (time.perf_counter() - t0) * 1e3
                t["compact"] = ms * 1e3 / n
                rs = m.remove_stats()
                exact = exact and empty and m.extract().tobytes() == want.tobytes() and \
                    rs["missing"] == rs["underflow"] == rs["stale"] == rs["vacant"] == 0 and \
                    m.stats()["dropped"] == 0
                if r > 0:
                    for k, v in t.items():
                        times[name + "_" + k].append(v)
                    compact_ms[name].append(ms)
        if r > 0:
            print(f"round {r}: " + "  ".join(f"{k} {np.median(v[-reps:]):7.1f}"
                                             for k, v in times.items()) + "  us/frame", flush=True)
    res = {"frames": n, "vpm": VPM, "slots": SLOTS, "exact": bool(exact),
           "voxels": int(maps["lds"].voxels()),
           "us_per_frame": {k: {"median": round(float(np.median(v)), 1),
                                "min": round(float(np.min(v)), 1),
                                "max": round(float(np.max(v)), 1)} for k, v in times.items()},
           "compact_ms": {k: round(float(np.median(v)), 3) for k, v in compact_ms.items()}}
    for m in maps.values():
        m.close()
    print(json.dumps(res))
    return 0 if exact else 1


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "remove":
        return main_remove(sys.argv[2:])
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    frames, T_wc = youth_synth.sequence(0, n)
    n, H, W = frames.shape
    rgb = np.random.default_rng(5).integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    T32 = np.ascontiguousarray(T_wc.reshape(n, 16)[:, :12], np.float32)
    d = torch.from_numpy(frames).cuda()
    c = torch.from_numpy(rgb).cuda()
    dT = torch.from_numpy(T32).cuda()
    s = torch.cuda.Stream()
    maps = {}
    for name, env in (("lds", "1"), ("direct", "0")):
        os.environ["YOUTH_MAP_LDS"] = env            # read at create
        maps[name] = youth_map.VoxelMap(VPM, SLOTS)
        maps[name].sync()
    os.environ.pop("YOUTH_MAP_LDS")
    cb = youth_viewer.CloudBuilder(W, H, max_frames=1)
    verts = torch.zeros((H * W, 6), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def sweep(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for f in range(n):
            fn(f)
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / n * 1e3         # us per frame

    def integrate(m):
        return lambda f: m.integrate_device(d.data_ptr() + f * H * W * 2,
                                            c.data_ptr() + f * H * W * 3, 1, W, H,
                                            dT.data_ptr() + f * 48, stream=s.cuda_stream)

    def cloud(f):
        cb.build_device_posed(d.data_ptr() + f * H * W * 2, c.data_ptr() + f * H * W * 3, 1, W, H,
                              dT.data_ptr() + f * 48, verts.data_ptr(), cnt.data_ptr(),
                              stream=s.cuda_stream)

    times = {"lds_fresh": [], "lds_revisit": [], "direct_fresh": [], "direct_revisit": [],
             "cloud": []}
    for r in range(rounds + 1):                      # round 0 warms every shape up
        for name in ("lds", "direct", "cloud"):
            for _ in range(reps):
                if name == "cloud":
                    t = {"cloud": sweep(cloud)}
                else:
                    m = maps[name]
                    m.clear()
                    m.sync()                         # the clear runs on the map's stream
                    t = {name + "_fresh": sweep(integrate(m)),
                         name + "_revisit": sweep(integrate(m))}
                if r > 0:
                    for k, v in t.items():
                        times[k].append(v)
        if r > 0:
            print(f"round {r}: " + "  ".join(f"{k} {np.median(v[-reps:]):7.1f}"
                                             for k, v in times.items()) + "  us/frame", flush=True)
    # the maps hold the sequence twice (fresh + revisit): identical records
    rec = {k: m.extract() for k, m in maps.items()}
    st = {k: m.stats() for k, m in maps.items()}
    same = rec["lds"].tobytes() == rec["direct"].tobytes()
    res = {"frames": n, "vpm": VPM, "slots": SLOTS, "records_identical": same,
           "voxels": int(rec["lds"].shape[0]),
           "us_per_frame": {k: {"median": round(float(np.median(v)), 1),
                                "min": round(float(np.min(v)), 1),
                                "max": round(float(np.max(v)), 1)} for k, v in times.items()},
           "stats": st,
           "left_lds_share": st["lds"]["direct"] / max(1, st["lds"]["integrated"])}
    for m in maps.values():
        m.close()
    cb.close()
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
